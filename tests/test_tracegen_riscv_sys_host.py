"""CPU: the rows of SyscallInstrs, SyscallCore, StateBump and MemoryBump, and SyscallCore's Global events, as the device kernels
compute them, run on the host. tests/native/riscv_sys_rows (built by __graft_entry__.build()) includes
sp1_amd/csrc/tg_riscv_sys_rows.hpp unchanged; its `host` form runs the same row functions the kernels of tracegen_riscv_sys.hip call
on the CPU, and never opens a GPU.

* the four chips, word for word against the host fillers (Tracer.syscall_instrs, EventTracer.state_chain, Tracer._bump_rows fed the
  canonically ordered tuples), padding included, at (records, height) = (0, 32), (1, 32), (32, 32), (33, 64), (257, 288) and the
  whole set at its pad32, on the three hand-assembled programs shifted across 2^24 cycles and unshifted, and on the synthetic ECALL,
  StateBump and MemoryBump events of rv64_partition_cases;
* MemoryBump's canonical table equals the host tracer's own table (made chip by chip) as a multiset of rows, on the shifted shards;
* SyscallCore's Global events equal eval_interactions over the host table, reduced to 9 words;
* the program's column constants equal R.chip(name)[0].layout and its widths main_width.
Everything is bit-exact; there are no tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import riscv_row_cases as C  # noqa: E402
import rv64_partition_cases as PC  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(PC.EXE), "tests/native/riscv_sys_rows is not built: run __graft_entry__.build()"


@pytest.mark.parametrize("name", PC.SYS_CHIPS)
@pytest.mark.parametrize("source", PC.SOURCES, ids=lambda s: "%s-%s" % s)
def test_rows_equal_the_host_fillers(source, name, tmp_path):
    for n, height in PC.shapes(source, name):
        rec, want = PC.case(source, name, n, height)
        got = PC.run_rows(name, rec.reshape(-1, PC.BIN_WORDS[PC.BINS.index(name)]), height, tmp_path)
        msg = C.first_difference(name, want, got, n)
        assert msg is None, msg


def test_every_chip_has_rows_somewhere():
    for name in PC.SYS_CHIPS:
        assert sum(len(PC.host_tables(s)[1][name]) for s in PC.SOURCES) >= 8, name
    lay = R.chip("SyscallInstrs")[0].layout
    t = PC.host_tables(("ecalls", None))[0]["SyscallInstrs"].numpy()
    for k in ("is_halt", "is_enter_unconstrained.result", "is_hint_len.result", "is_commit.result", "is_commit_deferred_proofs.result",
              "op_b_range_check", "op_c_range_check"):
        assert t[:, lay[k]].any() and not t[:, lay[k]].all(), k
    assert t[:, lay["index_bitmap"]:lay["index_bitmap"] + 8].any(axis=0).all()
    sb = PC.host_tables(("state", None))[0]["StateBump"].numpy()
    lay = R.chip("StateBump")[0].layout
    assert sb[:, lay["is_clk"]].any() and not sb[:, lay["is_clk"]].all() and (sb[:, lay["pc"]] > 0xFFFF).any()
    mb = PC.host_tables(("bumps", None))[0]["MemoryBump"].numpy()
    lay = R.chip("MemoryBump")[0].layout
    assert (mb[:, lay["access.diff_high_limb"]] == 1).any() and (mb[:, lay["access.diff_low_limb"]] == 1).any() and (mb[:, lay["access.prev_high"]] == 0).any()


@pytest.mark.parametrize("which", PC.PROGRAMS)
def test_memory_bump_is_the_tracers_table_as_a_multiset(which):
    ex, sh = PC.shard(which, True)
    tr = X.EventTracer(ex, sh, "cpu")
    tr.build()
    own = tr.tables["MemoryBump"]
    canonical = PC.host_tables((which, True))[0]["MemoryBump"].numpy()
    assert own.n == len(canonical) > 0
    assert sorted(map(tuple, own.main[:own.n].numpy().tolist())) == sorted(map(tuple, canonical.tolist()))
    sb = tr.tables["StateBump"]
    assert np.array_equal(sb.main[:sb.n].numpy(), PC.host_tables((which, True))[0]["StateBump"].numpy())


@pytest.mark.parametrize("source", [s for s in PC.SOURCES if s[0] in ("core", "ecalls")], ids=lambda s: "%s-%s" % s)
def test_syscall_core_global_events(source, tmp_path):
    _, records, events = PC.host_tables(source)
    rec = records["SyscallCore"]
    assert len(rec) == len(events) > 0
    got = PC.run_global(rec, tmp_path)
    assert got.shape == events.shape and np.array_equal(got, events), np.argwhere(got != events)[:4]
    assert (got[:, 8] == R.SYSCALL << 8).all()


def test_column_constants_and_widths_equal_the_transcribed_chips():
    text = subprocess.run([PC.EXE, "host", "layout"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, col = line.split()
        air = R.chip(chip)[0]
        assert int(col) == (air.main_width if key == "width" else air.layout[key]), line
        seen.setdefault(chip, set()).add(key)
    for name in PC.SYS_CHIPS:
        assert seen[name] == set(R.chip(name)[0].layout) | {"width"}, name
    text = subprocess.run([PC.EXE, "host", "width"], check=True, capture_output=True, timeout=60).stdout.decode()
    assert [tuple(l.split()) for l in text.splitlines()] == [(n, str(R.chip(n)[0].main_width)) for n in PC.SYS_CHIPS]
