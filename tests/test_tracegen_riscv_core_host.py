"""CPU: the rows of DivRem, AluX0 and MemoryLocal, and MemoryLocal's Global events, as the device kernels compute them, run on the
host. tests/native/riscv_core_rows (built by __graft_entry__.build()) includes sp1_amd/csrc/tg_riscv_core_rows.hpp unchanged; its
`host` form runs the same row functions the kernels of tracegen_riscv_core.hip call — DivRem in the same four column groups — on the
CPU, and never opens a GPU.

* DivRem on synthetic events: the 8 opcodes on every ordered pair of 0, 1, 2, -1, -2, INT64_MIN, INT64_MAX, 0x80000000, 0x7FFFFFFF,
  0xFFFFFFFF, 0xFFFFFFFF80000000, 2^32, 0x0000FFFF0000FFFF (8 x 169 rows), a from divrem_result: every word equals divrem_rows plus
  the tracer's state and adapter columns, at (events, height) = (0, 32), (1, 32), (32, 32), (33, 64), (257, 288) and the whole set
  at its pad32; the padding row is the "0 / 1" template;
* DivRem and AluX0 of a hand-assembled executed program (every DIV / REM form, c = 0, INT_MIN / -1 in both widths, rd = x0 forms
  with a register and an immediate c): every word equals riscv_exec.shard_tables, the row counts are asserted, and DivRem's
  constraints vanish on the host-form table — which does not depend on the host filler;
* the same two with clk and the previous timestamps rewritten around multiples of 2^24;
* MemoryLocal from the executed program's records and from synthetic ones (register addresses, three-limb addresses up to
  2^48 - 8, initial clk 0, clks around multiples of 2^24, bytes 4 and 5 of the values 0x00 / 0xFF): the table equals the tracer's
  and the events equal eval_interactions over the host table, reduced to 9 words, in order;
* the program's column constants equal R.chip(name)[0].layout and its widths main_width;
* pack_alu_events of the fourteen earlier chips, ALU_TRACEGEN_CHIPS, api.RISCV_ALU_CHIPS and core_device_tables' chips are as before.
Everything is bit-exact; there are no tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import machine_check as MC  # noqa: E402
import riscv_core_row_cases as K  # noqa: E402
import riscv_row_cases as C  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(K.EXE), "tests/native/riscv_core_rows is not built: run __graft_entry__.build()"


def _check(name, n, height, source, tmp_path):
    ev, want = K.case(name, n, height, source)
    got = K.run_rows(name, ev, height, tmp_path)
    msg = K.first_difference(name, want, got, n)
    assert msg is None, msg
    return got


@pytest.mark.parametrize("which", range(6))
def test_divrem_synthetic_events_equal_divrem_rows(which, tmp_path):
    ev, _ = K.events("DivRem", "synthetic")
    assert len(ev) == 8 * 169
    n, height = K.shapes("DivRem", "synthetic")[which]
    _check("DivRem", n, height, "synthetic", tmp_path)


def test_divrem_synthetic_events_reach_every_case():
    ev, tab = K.events("DivRem", "synthetic")
    lay = R.chip("DivRem")[0].layout
    col = lambda k: tab[:, lay[k]].numpy()
    for flag in ("is_div", "is_divu", "is_rem", "is_remu", "is_divw", "is_remw", "is_divuw", "is_remuw"):
        assert col(flag).sum() == 169, flag
    for k in ("is_overflow", "is_c_0.result", "rem_neg", "c_neg", "b_neg", "quot_msb", "remainder_lt_operation.bit", "c_times_quotient_upper.b_sign_extend"):
        assert col(k).any() and not col(k).all(), k
    word = col("is_real_not_word") == 0
    assert (col("is_overflow")[word]).any() and (col("is_overflow")[~word]).any()              # INT_MIN / -1 in both widths
    assert (col("is_c_0.result")[word] & (ev[word, 5] != 0)).any()                               # a W form's zero divisor under a non-zero upper half


def test_divrem_padding_is_the_template(tmp_path):
    got = K.run_rows("DivRem", K.events("DivRem")[0][:0], 32, tmp_path)
    lay = R.chip("DivRem")[0].layout
    one = (1 << 32) % RT.P
    ones = {lay[k] for k in ("is_divu", "adapter.op_c_memory.prev_value", "abs_c", "c", "max_abs_c_or_1", "b_not_neg_not_overflow",
                             "is_c_0.is_zero_limb.0.inverse", "is_c_0.is_zero_limb.1.result", "is_c_0.is_zero_limb.2.result",
                             "is_c_0.is_zero_limb.3.result", "is_c_0.is_zero_second_half")}
    assert len(ones) == 11
    for col in range(got.shape[0]):
        assert (got[col] == (one if col in ones else 0)).all(), col


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("name", K.CHIPS)
def test_executed_program_equals_the_host_tracer(name, which, tmp_path):
    n, height = K.shapes(name)[which]
    _check(name, n, height, "program", tmp_path)


def test_the_program_reaches_the_chips_with_the_rows_it_should():
    _, sh, _, tabs, rows = K.executed()
    names = X.chip_of_events(sh.events)
    assert rows["DivRem"] == 16 * 9 and rows["AluX0"] == 17
    for name in ("DivRem", "AluX0"):
        assert int((names == name).sum()) == rows[name] == len(K.events(name)[0]), name
        assert tabs[name].shape[0] == RT.pad32(rows[name])
    ev = K.events("DivRem")[0]
    assert set(ev[:, 2] & 0xFF) == {R.OPC[n.upper()] for n in K.DIVREM_OPS}
    assert (ev[:, 5] == 0).any() and ((ev[:, 4] == -(1 << 63)) & (ev[:, 5] == -1)).any()
    assert (((ev[:, 4] & 0xFFFFFFFF) == 0x80000000) & ((ev[:, 5] & 0xFFFFFFFF) == 0xFFFFFFFF) & ((ev[:, 2] & 0xFF) == R.OPC["DIVW"])).any()
    x0 = K.events("AluX0")[0]
    imm_c = (x0[:, 2] >> 33) & 1
    assert imm_c.any() and not imm_c.all() and len(set(x0[:, 2] & 0xFF)) >= 12 and ((x0[:, 2] >> 8) & 0xFF == 0).all()
    assert len(sh.local) == tabs["MemoryLocal"].shape[0] - (RT.pad32(len(sh.local)) - len(sh.local))
    assert (sh.local[:, 0] < 32).any() and (sh.local[:, 0] >= K.DATA).any()


def test_divrem_constraints_vanish_on_the_host_form_table(tmp_path):
    air = R.chip("DivRem")[0]
    publics = np.zeros(X.PV_WORDS, dtype=np.uint64)           # DivRem reads no public value
    for source in ("program", "synthetic"):
        ev, _ = K.events("DivRem", source)
        height = RT.pad32(len(ev))
        main = MC.from_monty(K.run_rows("DivRem", ev, height, tmp_path).T)
        cv = MC.constraint_values(air, None, main, publics)
        assert cv.shape == (height, air.num_constraints) and not cv.any(), (source, sorted(set(np.argwhere(cv != 0)[:, 1]))[:8])


def test_clock_windows(tmp_path):
    for name, (ev, want) in K.clock_window_tables().items():
        n = ev.shape[0]
        got = K.run_rows(name, ev, want.shape[1], tmp_path)
        msg = K.first_difference(name, want, got, n)
        assert msg is None, msg
        crossed = got[R.chip(name)[0].layout["adapter.op_a_memory.prev_low"], :n] == 0
        assert crossed.any() and not crossed.all(), name       # both kinds of previous access occurred


@pytest.mark.parametrize("source", ["program", "synthetic"])
def test_memory_local_records(source, tmp_path):
    records = K.executed()[1].local if source == "program" else K.synthetic_records()
    table, events = K.memory_local_host(records)
    n, height = len(records), table.shape[0]
    if source == "program":
        assert np.array_equal(table.numpy(), K.executed()[3]["MemoryLocal"].numpy())
    else:
        lay = R.chip("MemoryLocal")[0].layout
        t = table[:n].numpy()
        assert (t[:, lay["addr"]:lay["addr"] + 3] != 0).all(axis=1).any() and (t[:, lay["initial_clk_high"]] != 0).any()
        assert (t[:, lay["initial_clk_low"]] == (1 << 24) - 1).any() and (t[:, lay["initial_clk_low"]] == 0).any()
        for tag in ("initial", "final"):
            seen = set(zip(t[:, lay[tag + "_value_lower"]].tolist(), t[:, lay[tag + "_value_upper"]].tolist()))
            assert {(0, 0), (255, 0), (0, 255), (255, 255)} <= seen, tag
    got = K.run_rows("MemoryLocal", records, height, tmp_path)
    msg = K.first_difference("MemoryLocal", C.montgomery_col_major(table), got, n)
    assert msg is None, msg
    got_events = K.run_global(records, tmp_path)
    assert got_events.shape == events.shape == (2 * n, 9)
    assert np.array_equal(got_events, events), np.argwhere(got_events != events)[:4]
    assert (got_events[0::2, 8] == (1 | R.MEMORY << 8)).all() and (got_events[1::2, 8] == R.MEMORY << 8).all()


def test_column_constants_and_widths_equal_the_transcribed_chips():
    text = subprocess.run([K.EXE, "host", "layout"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, col = line.split()
        air = R.chip(chip)[0]
        assert int(col) == (air.main_width if key == "width" else air.layout[key]), line
        seen.setdefault(chip, set()).add(key)
    for name in K.CHIPS:
        assert seen[name] == set(R.chip(name)[0].layout) | {"width"}, name
    text = subprocess.run([K.EXE, "host", "width"], check=True, capture_output=True, timeout=60).stdout.decode()
    assert [tuple(l.split()) for l in text.splitlines()] == [(n, str(R.chip(n)[0].main_width)) for n in K.CHIPS]


def _pack_alu_events_before(events, chip):
    """pack_alu_events as it stood when the device made the fourteen chips, restated."""
    ev = events[np.nonzero(X.chip_of_events(np.asarray(events)) == chip)[0]]
    flags = ev[:, X.E_FLAGS]
    imm_b, imm_c = flags & 1, (flags & 2) >> 1
    ops = (ev[:, X.E_OP] | (ev[:, X.E_OPA] << 8) | (((1 - imm_b) * (ev[:, X.E_OPB] & 0xFF)) << 16) | (((1 - imm_c) * (ev[:, X.E_OPC] & 0xFF)) << 24)
           | ((flags & 3) << 32))
    b = np.where(imm_b == 1, ev[:, X.E_OPB], ev[:, X.E_B])
    c = np.where(imm_c == 1, ev[:, X.E_OPC], ev[:, X.E_C])
    cols = [ev[:, X.E_PC], ev[:, X.E_CLK], ops, ev[:, X.E_A], b, c, ev[:, X.E_A_PREV], ev[:, X.E_A_PTS], ev[:, X.E_B_PTS], ev[:, X.E_C_PTS],
            ev[:, X.E_NEXT_PC]]
    return np.stack(cols, 1)


def test_existing_behaviour_is_unchanged():
    from sp1_amd import api
    assert tuple(X.ALU_TRACEGEN_CHIPS) == C.CHIPS
    assert api.RISCV_ALU_CHIPS == {n: i for i, n in enumerate(C.CHIPS)}
    assert not set(K.CHIPS + ("Global",)) & set(X.ALU_TRACEGEN_CHIPS + X.MEM_TRACEGEN_CHIPS)   # core_device_tables iterates over exactly these
    _, csh, _, _ = C.corner()
    some = 0
    for name in C.CHIPS:
        now, before = X.pack_alu_events(csh.events, name), _pack_alu_events_before(csh.events, name)
        assert now.dtype == before.dtype and now.shape == before.shape and now.tobytes() == before.tobytes(), name
        some += now.shape[0] > 0
    assert some == 14
