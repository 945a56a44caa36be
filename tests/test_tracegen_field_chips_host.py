"""CPU: the two-phase rows of the Weierstrass and Fp / Fp2 precompile chips as the device kernels compute them, run on the host.
tests/native/field_chip_rows (built by __graft_entry__.build()) includes sp1_amd/csrc/tg_field_chip_rows.hpp unchanged; its `host`
form runs phase A over the rows and then phase B over (operation, row) as loops — the functions the kernels of
tracegen_field_chips.hip call — on the CPU, and never opens a GPU.

* every word of all twelve tables equals the host filler's chip table (riscv_more_trace.family_shard_from: Python integers),
  padding rows included, at (events, height) = (0, 32), (1, 32), (32, 32) — no padding —, (33, 64), and at (300, 320) for one
  N = 8 and one N = 12 kind of each shape, over the operand sets of tests/field_chip_cases.py; everything is bit-exact, there are
  no tolerances;
* the result columns are the words the events carry, which field_chip_cases computes in Python integers;
* the header's widths, event sizes, witness offsets and column constants equal R.chip(name)[0].layout and riscv_more's tables;
* the chips' constraints vanish and the buses balance (machine_check) with a host-form table substituted into a shard of a
  hand-assembled program, for one kind per shape and N."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_chip_cases as C  # noqa: E402
import machine_check as MC  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more as M  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(C.EXE), "tests/native/field_chip_rows is not built: run __graft_entry__.build()"


def test_the_generated_events_mix_the_opcodes_inside_a_wave():
    for kind, n_codes in (("bn254_fp", 3), ("bls12381_fp", 3), ("bn254_fp2_addsub", 2), ("bls12381_fp2_addsub", 2)):
        codes = C.events(kind, 64)[:, 3] & 0xFF
        assert len(set(codes[:8].tolist())) == n_codes and all(codes[i] != codes[i + 1] for i in range(63)), kind


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


@pytest.mark.parametrize("kind", C.KINDS)
def test_the_result_columns_are_the_words_written(kind, tmp_path):
    n, height = 33, 64
    ev = C.events(kind, n)
    got = C.run_rows("host", kind, ev, height, tmp_path)
    lay = R.chip(C.CHIPS[kind])[0].layout
    nl = C.field_of(kind)[2]
    names = {"curve_add": ("x3_ins", "y3_ins"), "curve_double": ("x3_ins", "y3_ins"), "fp": ("output",), "fp2_addsub": ("c0", "c1"), "fp2_mul": ("c0", "c1")}[C.SHAPE[kind]]
    inv = pow(1 << 32, -1, RT.P)
    u = ev.view(np.uint64)
    for r in range(n):
        for c, name in enumerate(names):
            by = [int(got[lay[name + ".result"] + i, r]) * inv % RT.P for i in range(nl)]
            assert all(b < 256 for b in by)
            written = u[r, ev.shape[1] - (len(names) - c) * (nl // 8):][:nl // 8]
            assert sum(b << (8 * i) for i, b in enumerate(by)) == sum(int(w) << (64 * i) for i, w in enumerate(written)), (kind, r, name)


def test_widths_and_column_constants_equal_the_transcribed_chips():
    text = subprocess.run([C.EXE, "host", "layout", "-", "-"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, value = line.split()
        air = R.chip(chip)[0]
        kind = next(k for k in C.KINDS if C.CHIPS[k] == chip)
        if key == "width":
            assert int(value) == air.main_width, line
        elif key == "event_words":
            assert int(value) == C.event_words(kind), line
        elif key == "witness_offset":
            name = C.field_of(kind)[0]
            assert int(value) == (M.CURVES[name][4] if C.SHAPE[kind].startswith("curve") else M.FP_FIELDS[name][3]), line
        elif key == "ops":
            assert int(value) == sum(1 for k in air.layout if k.endswith(".witness")), line
        else:
            assert int(value) == air.layout[key], line
        seen.setdefault(chip, set()).add(key)
    assert set(seen) == set(C.CHIPS.values())
    for chip, keys in seen.items():                                  # every field operation and range check of the chip is among them
        lay = R.chip(chip)[0].layout
        assert {k for k in lay if k.endswith((".witness", ".carry", ".byte_flags", ".rhs_comparison_byte"))} <= keys, chip
        assert {k for k in lay if k in ("is_add", "is_sub", "is_mul", "is_real", "clk_high", "clk_low")} <= keys, chip


# --------------------------------------------------------------------------------------- a host-form table substituted into a shard
CHECKED = {"Bn254": ("bn254_add", "bn254_double", "bn254_fp", "bn254_fp2_addsub", "bn254_fp2_mul"),
           "Bls12381": ("bls12381_add", "bls12381_double", "bls12381_fp", "bls12381_fp2_addsub", "bls12381_fp2_mul")}


@pytest.fixture(scope="module")
def program_shards():
    """{kind: (events, host_shard)} from the curve and the tower program of each field."""
    out = {}
    for name in CHECKED:
        for elf in (C.curve_program(name), C.tower_program(name)):
            ex = X.Executor(elf, stdin=[])
            for rec in X.run_records(ex, 1 << 20):
                if rec.kind in CHECKED[name]:
                    out[rec.kind] = (np.ascontiguousarray(rec.events), X.host_shard(ex, rec))
    assert set(out) == set(CHECKED["Bn254"] + CHECKED["Bls12381"])
    return out


@pytest.mark.parametrize("kind", CHECKED["Bn254"] + CHECKED["Bls12381"])
def test_constraints_vanish_and_buses_balance_with_the_host_form_table(kind, program_shards, tmp_path):
    ev, (machine, tables, publics, _) = program_shards[kind]
    chip = C.CHIPS[kind]
    main = tables[chip][1]
    assert ev.shape == ({"curve_add": 1, "curve_double": 2, "fp": 4, "fp2_addsub": 2, "fp2_mul": 1}[C.SHAPE[kind]], C.event_words(kind))
    got = C.run_rows("host", kind, ev, int(main.shape[0]), tmp_path)
    msg = C.first_difference(kind, C.montgomery_col_major(main), got, len(ev))
    assert msg is None, msg
    tabs = dict(tables)
    tabs[chip] = (tables[chip][0], torch.as_tensor(MC.from_monty(got.T).astype(np.int64)))
    assert tabs[chip][1] is not main
    assert frozenset(a.name for a, _ in machine) in RT.chip_clusters()
    bad, imbalance = MC.check_shard(machine, tabs, publics, PVM.program())
    assert not bad and not imbalance, (bad, imbalance)
