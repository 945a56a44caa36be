"""CPU: the rows of MemoryGlobalInit / MemoryGlobalFinalize and SyscallPrecompile, the Global events of their rows and the
MemoryLocal records of a precompile's calls, as the device kernels compute them, run on the host. tests/native/riscv_memglobal_rows
(built by __graft_entry__.build()) includes sp1_amd/csrc/tg_riscv_memglobal_rows.hpp unchanged; its `host` form runs the same row
functions the kernels of tracegen_riscv_memglobal.hip call, with the same read of record i - 1's address, and never opens a GPU.

* MemoryGlobal, both kinds, the cases and shapes of tests/memory_global_cases.py: every word of the table, padding rows included,
  equals riscv_more_trace.memory_shard_from's, and the events equal its `gev`, reduced to 9 words, in order;
* the cases reach what they are meant to: the uncompared row, every limb as the compared one, the top address, the value bytes;
* the constraints of both chips vanish on the host-form table — which does not depend on the host filler;
* SyscallPrecompile and the MemoryLocal records of Keccak (1, 2, 11 calls) and secp256k1 add / double (1, 33 calls of multiples of G):
  the table and events equal precompile_shard_from / secp256k1_*_shard_from's, and the records are the ones their MemoryLocal
  tables stand for, word for word, in the order of the host builders' rows;
* the program's column constants equal R.chip(name)[0].layout and its widths main_width.
Everything is bit-exact; there are no tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import machine_check as MC  # noqa: E402
import memory_global_cases as G  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(G.EXE), "tests/native/riscv_memglobal_rows is not built: run __graft_entry__.build()"


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("case,n,height", G.CASE_SHAPES)
def test_memory_global_equals_the_host_filler(kind, case, n, height, tmp_path):
    want, want_events = G.host_table(case, kind, n, height)
    rec = G.records3(case, kind, n)
    got = G.run_rows(G.CHIP[kind], rec, height, tmp_path, (G.PREVIOUS[case],))
    msg = G.first_difference(G.CHIP[kind], want, got, n)
    assert msg is None, msg
    events = G.run_global(G.CHIP[kind], rec, tmp_path)
    assert events.shape == want_events.shape == (n, 9)
    assert np.array_equal(events, want_events), np.argwhere(events != want_events)[:4]
    assert (events[:, 8] == ((kind == "finalize") | R.MEMORY << 8)).all()
    if kind == "init":
        assert not events[:, :2].any()                        # timestamp zero whatever the clk columns hold


def test_the_cases_reach_what_they_are_meant_to():
    lay = R.chip("MemoryGlobalInit")[0].layout
    for case in G.CASES:
        tables = G.host_shard(case, 300)[1]
        for kind in G.KINDS:
            t = tables[G.CHIP[kind]][1][:300].numpy()
            flags = t[:, lay["lt_cols.u16_flags"]:lay["lt_cols.u16_flags"] + 4]
            assert flags[:, :3].any(axis=0).all() and not flags[:, 3].any(), (case, kind)      # limbs 0, 1, 2 compared; addresses have three
            assert (t[:, lay["is_comp"]] == 0).sum() == (case == "first") and t[0, lay["is_comp"]] == (case != "first")
            if case == "first":
                assert not t[0, lay["lt_cols.bit"]:lay["lt_cols.bit"] + 8].any() and t[0, lay["prev_valid"]] == 1
            assert (t[:, lay["addr"]:lay["addr"] + 3] == [0xFFF8, 0xFFFF, 0xFFFF]).all(axis=1).any()                 # 2^48 - 8
            seen = set(zip(t[:, lay["value_lower"]].tolist(), t[:, lay["value_upper"]].tolist()))
            assert {(0, 0), (255, 0), (0, 255), (255, 255)} <= seen, (case, kind)
            assert {0, 1, 1 << 16}.issubset(set(t[:, lay["clk_high"]].tolist())) and {0, 1, (1 << 24) - 1}.issubset(set(t[:, lay["clk_low"]].tolist()))
    a = G.addresses("continuing", 300)
    for lo, hi in zip(G.NEIGHBOURS[0::2], G.NEIGHBOURS[1::2]):
        assert a.index(hi) == a.index(lo) + 1                  # neighbours stayed neighbours


@pytest.mark.parametrize("kind", G.KINDS)
def test_memory_global_constraints_vanish_on_the_host_form_table(kind, tmp_path):
    air = R.chip(G.CHIP[kind])[0]
    publics = np.zeros(X.PV_WORDS, dtype=np.uint64)           # the chip reads no public value
    for case, n in (("first", 300), ("continuing", 257), ("continuing", 1)):
        height = RT.pad32(n)
        main = MC.from_monty(G.run_rows(G.CHIP[kind], G.records3(case, kind, n), height, tmp_path, (G.PREVIOUS[case],)).T)
        cv = MC.constraint_values(air, None, main, publics)
        assert cv.shape == (height, air.num_constraints) and not cv.any(), (case, n, sorted(set(np.argwhere(cv != 0)[:, 1]))[:8])


@pytest.mark.parametrize("kind,n", [(k, n) for k in G.PRECOMPILES for n in G.PRECOMPILE_COUNTS[k]])
def test_precompile_closing_chips_equal_the_host_builders(kind, n, tmp_path):
    ev = G.precompile_events(kind, n)
    _, tables, _, gev = G.host_precompile_shard(kind, n)
    words, syscall_id, arg2_word = G.PRECOMPILE_CHIP_ARGS[kind]
    sp, ml = tables["SyscallPrecompile"][1], tables["MemoryLocal"][1]
    per_call = sum(s[1] for s in G.SEGMENTS[kind])
    assert sp.shape[0] == RT.pad32(n) and ml.shape[0] == RT.pad32(per_call * n) and gev.shape[0] == (2 * per_call + 1) * n
    got = G.run_rows("SyscallPrecompile", ev, int(sp.shape[0]), tmp_path, (words, syscall_id, arg2_word))
    msg = G.first_difference("SyscallPrecompile", G.montgomery_col_major(sp), got, n)
    assert msg is None, msg
    events = G.run_global("SyscallPrecompile", ev, tmp_path, (words, syscall_id, arg2_word))
    want_events = G.reduce_global_events(gev)
    assert np.array_equal(events, want_events[2 * per_call * n:]) and (events[:, 8] == (1 | R.SYSCALL << 8)).all()
    # the records, word for word, are the ones the host builder's MemoryLocal rows stand for, in its order; through the pinned
    # MemoryLocal row function they give its table and its events
    records = G.run_records(ev, G.SEGMENTS[kind], tmp_path)
    assert records.shape == (per_call * n, 5)
    assert np.array_equal(records, G.local_records_of(ml[:per_call * n])), np.argwhere(records != G.local_records_of(ml[:per_call * n]))[:4]
    import riscv_core_row_cases as K
    table = K.run_rows("MemoryLocal", records, int(ml.shape[0]), tmp_path)
    msg = K.first_difference("MemoryLocal", G.montgomery_col_major(ml), table, per_call * n)
    assert msg is None, msg
    assert np.array_equal(K.run_global(records, tmp_path), want_events[:2 * per_call * n])


def test_descriptors_are_the_ones_the_api_uses():
    from sp1_amd import api
    assert set(api.PRECOMPILE_DESCRIPTORS) == set(G.PRECOMPILES) == set(X.DEVICE_PRECOMPILE_KINDS)
    for kind in G.PRECOMPILES:
        assert api.PRECOMPILE_DESCRIPTORS[kind] == G.PRECOMPILE_CHIP_ARGS[kind] + (G.SEGMENTS[kind],), kind


def test_column_constants_and_widths_equal_the_transcribed_chips():
    text = subprocess.run([G.EXE, "host", "layout"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, col = line.split()
        air = R.chip(chip)[0]
        assert int(col) == (air.main_width if key == "width" else air.layout[key]), line
        seen.setdefault(chip, set()).add(key)
    chips = ("MemoryGlobalInit", "MemoryGlobalFinalize", "SyscallPrecompile")
    for name in chips:
        assert seen[name] == set(R.chip(name)[0].layout) | {"width"}, name
    text = subprocess.run([G.EXE, "host", "width"], check=True, capture_output=True, timeout=60).stdout.decode()
    assert [tuple(l.split()) for l in text.splitlines()] == [(n, str(R.chip(n)[0].main_width)) for n in chips]
