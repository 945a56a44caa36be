"""CPU: the rows of the EdAddAssign, EdDecompress and Uint256Ops chips and the touched words' MemoryLocal records as the device kernels
compute them, run on the host. tests/native/ed_u256_rows (built by __graft_entry__.build()) includes
sp1_amd/csrc/tg_ed_uint256_rows.hpp unchanged; its `host` form runs the functions the kernels of tracegen_ed_uint256_ops.hip call —
phase A over the rows and phase B over (block, row) for the two Edwards chips, one function per row for Uint256Ops — on the CPU, and
never opens a GPU.

* every word of the three tables equals the host filler's chip table (riscv_more_trace.family_shard_from: Python integers), padding
  rows included, at (events, height) = (0, 32), (1, 32), (32, 32) — no padding —, (33, 64) and (300, 320), over the operand sets of
  tests/ed_u256_cases.py; everything is bit-exact, there are no tolerances;
* the header's widths, event sizes, witness offset and column constants equal R.chip(name)[0].layout;
* the records equal what family_shard_from hands _close_precompile_shard, in order;
* the chips' constraints vanish and the buses balance (machine_check.check_shard) with a host-form table substituted into the shards
  of the ed25519 program and the carry program of tests/test_riscv_precompiles.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed_u256_cases as C  # noqa: E402
import machine_check as MC  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more as M  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(C.EXE), "tests/native/ed_u256_rows is not built: run __graft_entry__.build()"


def test_the_case_file_covers_what_it_says():
    add, dec, ops = C.operands("ed_add"), C.operands("ed_decompress"), C.operands("uint256_ops")
    assert (0, 1) in {q[:2] for q in add} and (0, 1) in {q[2:] for q in add} and any(q[:2] == q[2:] and q[0] > 3 for q in add)
    assert {C.root_path(C.u_div_v(y)) for y in dec} == {(False, False), (False, True), (True, False), (True, True)}
    assert C.events("ed_decompress", 64)[:, 2].tolist() == [0, 1] * 32
    ev = C.events("uint256_ops", 300)
    assert (ev[:, 3] & 0xFF).tolist() == [0x30, 0x31] * 150
    assert ops[121][:3] == (C.TOP, C.TOP - 1, C.TOP) and ops[122][:3] == (C.TOP,) * 3               # a product (odd row), a sum with carry 2
    assert ev[122, 54] == 2 and not ev[122, 55:58].any()
    assert any(o[3] for o in ops) and bool((ev[:, 5] == ev[:, 1]).any())                            # d aliased onto a
    assert bool((ev[:, 7:10] < (5 << 24)).any()) and bool((ev[:, 7:10] >= (5 << 24)).any())        # register timestamps on both sides of 2^24


@pytest.mark.parametrize("kind,n,height", C.KIND_SHAPES)
def test_every_word_equals_the_host_filler(kind, n, height, tmp_path):
    want = C.montgomery_col_major(C.host_table(kind, n, height))
    got = C.run_rows("host", kind, C.events(kind, n), height, tmp_path)
    assert got.shape == want.shape
    msg = C.first_difference(kind, want, got, n)
    assert msg is None, msg


@pytest.mark.parametrize("kind", C.KINDS)
def test_more_events_than_rows_are_refused(kind, tmp_path):
    with pytest.raises(subprocess.CalledProcessError):
        C.run_rows("host", kind, C.events(kind, 33), 32, tmp_path)


def test_the_result_columns_are_the_words_written(tmp_path):
    inv = pow(1 << 32, -1, RT.P)
    for kind, names in (("ed_add", ("x3_ins", "y3_ins")), ("uint256_ops", ("field_op.result", "field_op.carry"))):
        n, height = 33, 64
        ev = C.events(kind, n)
        got = C.run_rows("host", kind, ev, height, tmp_path)
        lay = R.chip(C.CHIPS[kind])[0].layout
        u = ev.view(np.uint64)
        for r in range(n):
            for c, name in enumerate(names):
                by = [int(got[lay[name if "." in name else name + ".result"] + i, r]) * inv % RT.P for i in range(32)]
                assert all(b < 256 for b in by)
                written = u[r, ev.shape[1] - (2 - c) * 4:][:4]
                assert sum(b << (8 * i) for i, b in enumerate(by)) == sum(int(w) << (64 * i) for i, w in enumerate(written)), (kind, r, name)


def test_widths_and_column_constants_equal_the_transcribed_chips():
    text = subprocess.run([C.EXE, "host", "layout", "-", "-"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, value = line.split()
        if chip == "all":
            assert key == "witness_offset" and int(value) == M.WITNESS_OFFSET == 1 << 14, line
            continue
        air = R.chip(chip)[0]
        kind = next(k for k in C.KINDS if C.CHIPS[k] == chip)
        if key == "width":
            assert int(value) == air.main_width, line
        elif key == "event_words":
            assert int(value) == C.EVENT_WORDS[kind] == C.events(kind, 1).shape[1], line
        elif key == "ops":
            assert int(value) == sum(1 for k in air.layout if k.endswith(".witness")), line
        else:
            assert int(value) == air.layout[key], line
        seen.setdefault(chip, set()).add(key)
    assert set(seen) == set(C.CHIPS.values())
    for chip, keys in seen.items():                                  # every field operation and range check of the chip is among them
        lay = R.chip(chip)[0].layout
        assert {k for k in lay if k.endswith((".witness", ".carry", ".byte_flags", ".rhs_comparison_byte"))} <= keys, chip
        assert {k for k in lay if k in ("is_add", "is_mul", "is_real", "clk_high", "clk_low", "sign", "x.lsb")} <= keys, chip


@pytest.mark.parametrize("kind", ("ed_decompress", "uint256_ops"))
@pytest.mark.parametrize("n", (1, 33, 300))
def test_the_records_are_what_the_host_filler_hands_on(kind, n, tmp_path):
    want = C.host_records(kind, n)
    got = C.run_records("host", kind, C.events(kind, n), tmp_path)
    assert want.shape == (n * C.RECORDS_PER_CALL[kind], 5) == got.shape
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d words differ, first at record %d word %d" % (kind, len(bad), bad[0][0], bad[0][1])


def test_no_events_give_no_records(tmp_path):
    for kind in ("ed_decompress", "uint256_ops"):
        assert C.run_records("host", kind, C.events(kind, 0), tmp_path).shape == (0, 5)


# --------------------------------------------------------------------------------------- a host-form table substituted into a shard
@pytest.fixture(scope="module")
def program_shards():
    """{kind: (events, host_shard)} from the ed25519 program and the carry program."""
    out = {}
    for elf in (C.ed_program(), C.carry_program()):
        ex = X.Executor(elf, stdin=[])
        for rec in X.run_records(ex, 1 << 20):
            if rec.kind in C.KINDS:
                out[rec.kind] = (np.ascontiguousarray(rec.events), X.host_shard(ex, rec))
    assert set(out) == set(C.KINDS)
    return out


@pytest.mark.parametrize("kind", C.KINDS)
def test_constraints_vanish_and_buses_balance_with_the_host_form_table(kind, program_shards, tmp_path):
    ev, (machine, tables, publics, _) = program_shards[kind]
    chip = C.CHIPS[kind]
    main = tables[chip][1]
    assert ev.shape == (C.CALLS_PER_ROUND[kind], C.EVENT_WORDS[kind])
    got = C.run_rows("host", kind, ev, int(main.shape[0]), tmp_path)
    msg = C.first_difference(kind, C.montgomery_col_major(main), got, len(ev))
    assert msg is None, msg
    if kind != "ed_add":
        assert np.array_equal(C.run_records("host", kind, ev, tmp_path), C.filler(kind, ev)[1])
    tabs = dict(tables)
    tabs[chip] = (tables[chip][0], torch.as_tensor(MC.from_monty(got.T).astype(np.int64)))
    assert tabs[chip][1] is not main
    assert frozenset(a.name for a, _ in machine) in RT.chip_clusters()
    bad, imbalance = MC.check_shard(machine, tabs, publics, PVM.program())
    assert not bad and not imbalance, (bad, imbalance)
