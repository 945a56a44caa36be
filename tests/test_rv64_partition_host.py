"""CPU: where an executed instruction goes and what it becomes there, as the partition kernels compute it, run on the host.
tests/native/riscv_sys_rows (built by __graft_entry__.build()) includes sp1_amd/csrc/tg_rv64_partition.hpp unchanged; its `host`
form runs the classification and the packers the kernels of tracegen_rv64_partition.hip call on the CPU, and never opens a GPU.

* every opcode with rd = 0 and rd != 0 and both immediate flags: bins 0..25 equal chip_of_events, the records pack_alu_events /
  pack_mem_events, bit for bit and in order;
* the three hand-assembled programs' events, unshifted and shifted across 2^24 cycles, and the synthetic ECALL / StateBump /
  MemoryBump events: every bin equal to the numpy stable partition (rv64_partition_cases.reference_partition; bins 26..28 from the
  three conditions restated there), counts included; together the programs fill all 26 instruction bins;
* the shifted shards have the StateBump and MemoryBump rows they should;
* the record widths and the bin order equal the api's.
Everything is bit-exact; there are no tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rv64_partition_cases as PC  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(PC.EXE), "tests/native/riscv_sys_rows is not built: run __graft_entry__.build()"


def _check(ev, tmp_path):
    want = PC.reference_partition(ev)
    want_counts, want_arena = PC.arena_of(want)
    counts, arena = PC.run_partition(ev, tmp_path)
    assert counts.tolist() == want_counts.tolist(), dict(zip(PC.BINS, zip(counts.tolist(), want_counts.tolist())))
    at = 0
    for name, w in zip(PC.BINS, PC.BIN_WORDS):
        got = arena[at:at + len(want[name]) * w].reshape(-1, w)
        assert np.array_equal(got, want[name]), (name, np.argwhere(got != want[name])[:4])
        at += got.size
    assert at == arena.size == want_arena.size
    return want


def every_opcode_events():
    """One event per opcode up to ECALL x (rd = 0, rd != 0) x the four settings of the immediate flags, every word distinct."""
    rows = []
    for op in range(R.OPC["ECALL"] + 1):
        for rd in (0, 7):
            for flags in range(4):
                i = len(rows)
                e = [PC.K.s64(0x1111_0000_0000_0000 * w + 0x10001 * i + w) for w in range(X.EV_WORDS)]
                e[X.E_OP], e[X.E_OPA], e[X.E_OPB], e[X.E_OPC], e[X.E_FLAGS] = op, rd, 0x100 + 11 + i % 5, 0x200 + 12 + i % 7, flags
                e[X.E_PC], e[X.E_CLK] = 0x7800_0000 + 4 * i, 8 * i + 1
                e[X.E_A_PREV] = 0x0101 if i % 2 else 0x0002
                e[X.E_A_PTS], e[X.E_B_PTS], e[X.E_C_PTS] = max(8 * i - 11, 0), max(8 * i - 3, 0), max(8 * i - 20, 0)
                rows.append(e)
    return np.array(rows, dtype=np.int64)


def test_every_opcode_goes_where_chip_of_events_sends_it(tmp_path):
    ev = every_opcode_events()
    want = _check(ev, tmp_path)
    assert sum(len(want[n]) for n in PC.BINS[:26]) == len(ev) == 51 * 8
    assert all(len(want[n]) for n in PC.BINS[:27])
    assert len(want["AluX0"]) == 29 * 4 and len(want["LoadX0"]) == 7 * 4 and len(want["SyscallInstrs"]) == 8 and len(want["SyscallCore"]) == 4


@pytest.mark.parametrize("source", PC.SOURCES, ids=lambda s: "%s-%s" % s)
def test_events_are_partitioned_as_numpy_does(source, tmp_path):
    _check(PC.source_events(source)[2], tmp_path)


def test_the_programs_fill_every_instruction_bin_and_the_shifted_ones_bump(tmp_path):
    seen = set()
    bumps = {}
    for which in PC.PROGRAMS:
        for shift in (False, True):
            parts = PC.reference_partition(PC.shard(which, shift)[1].events)
            seen |= {n for n in PC.BINS[:26] if len(parts[n])}
            bumps[which, shift] = (len(parts["StateBump"]), len(parts["MemoryBump"]))
    assert seen == set(PC.BINS[:26])
    assert [bumps[w, False] for w in PC.PROGRAMS] == [(0, 0)] * 3
    assert [bumps[w, True] for w in PC.PROGRAMS] == [(1, 9), (1, 6), (1, 8)]
    ex, sh = PC.program("core")
    far = PC.shifted(sh, PC.shift_of(sh) + 2 * PC.WINDOW - 320)
    assert len(PC.reference_partition(far.events)["MemoryBump"]) == 12
    assert len(PC.reference_partition(sh.events)["SyscallCore"]) == 1
    _check(far.events, tmp_path)


def test_synthetic_events_reach_every_case():
    sc, sb, pc_carry, inc, bumps = PC.conditions(PC.synthetic_state_events())
    assert sb.any() and not sb.all() and pc_carry.any() and (sb & ~pc_carry).any() and (inc == PC.ECALL_INC).any()
    ev = PC.synthetic_state_events()
    ecall_only = sb & ~pc_carry & (((ev[:, X.E_CLK] & 0xFFFFFF) + 8) < PC.WINDOW)
    assert ecall_only.any()                                    # an ECALL's step straddles 2^24 where 8 would not
    bumps = PC.conditions(PC.synthetic_bump_events())[4]
    assert {tuple(r) for r in bumps.tolist()} >= {(True, True, True), (True, False, False), (True, True, False), (False, False, False)}
    tup = PC.bump_tuples(PC.synthetic_bump_events())
    back = (tup[:, 3] >> 24) - (tup[:, 1] >> 24)
    assert {1, 2, 70_000} <= set(back.tolist()) and (tup[:, 1] == 0).any()
    sc = PC.conditions(PC.synthetic_ecalls())[0]
    assert sc.any() and not sc.all()


def test_bins_and_record_widths_equal_the_api():
    from sp1_amd import api
    assert api.RV64_BINS == PC.BINS and api.RV64_BIN_WORDS == PC.BIN_WORDS and len(PC.BINS) == 29
    assert PC.BINS[:14] == tuple(api.RISCV_ALU_CHIPS) and PC.BINS[14:23] == tuple(api.RISCV_MEM_CHIPS)
    text = subprocess.run([PC.EXE, "host", "bins"], check=True, capture_output=True, timeout=60).stdout.decode()
    assert [tuple(int(v) for v in l.split()) for l in text.splitlines()] == list(enumerate(PC.BIN_WORDS))
