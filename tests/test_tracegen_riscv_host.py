"""CPU: the rows of the fourteen RISC-V instruction chips as the device kernels compute them, run on the host.
tests/native/riscv_rows (built by __graft_entry__.build()) includes sp1_amd/csrc/tg_riscv_rows.hpp unchanged; its `host` form runs
the same fill_row<CHIP> the kernels of tracegen_riscv.hip call, on the CPU, and never opens a GPU.

* every word of every column equals the host tracer's (riscv_exec.shard_tables on the CPU), padding rows included, for all
  fourteen chips at (events, height) = (0, 32), (1, 32), (32, 32) — no padding —, (33, 64), the whole corner set at its pad32 and
  (257, 288) — more than one 256-lane workgroup —, over the programs of tests/riscv_row_cases.py: xor / or / and / slt / sltu on
  every pair of the value list, their immediate forms with -2048, -1, 0, 2047, rs1 = x0, rs1 = rs2, rd = x0 (AluX0's row, not
  Bitwise's: the row count is asserted), sll / sllw / slli / slliw by 0 .. 63 and by a register holding 2^64 - 1, lui / auipc with
  sign-extending immediates and rd = x0, jal forward and backward with rd = x0 / x1, jalr with immediates 0, positive, negative, an
  odd target, rd = x0 and rd = rs1;
* the same with clk and the previous timestamps rewritten around multiples of 2^24 (an access just below, exactly on and just above
  the boundary; a previous access in the window before), for the chips whose host filler is a method of the tracer;
* the program's column constants equal R.chip(name)[0].layout and its widths main_width;
* pack_alu_events produces for the eight first chips exactly the records it produced before the six were added.
Everything is bit-exact; there are no tolerances."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import riscv_row_cases as C  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(C.EXE), "tests/native/riscv_rows is not built: run __graft_entry__.build()"


def test_the_chips_are_the_device_chips():
    from sp1_amd import api
    assert tuple(X.ALU_TRACEGEN_CHIPS) == C.CHIPS
    assert api.RISCV_ALU_CHIPS == {n: i for i, n in enumerate(C.CHIPS)}


def test_the_corner_program_reaches_every_chip_with_the_rows_it_should():
    _, sh, tabs, rows = C.corner()
    names = X.chip_of_events(sh.events)
    for name in C.NEW_CHIPS:
        assert int((names == name).sum()) == rows[name] == len(C.corner_events(name)), name
        assert tabs[name].shape[0] == RT.pad32(rows[name])
    assert rows["AluX0"] >= 3 * len(C.VALUES) and int((names == "AluX0").sum()) >= rows["AluX0"]     # rd = x0 went there (and the nops)
    for name in C.OLD_CHIPS:
        assert len(C.corner_events(name)) > 32, name
    ev = C.corner_events("Jalr")
    assert ((ev[:, 4] + ev[:, 5]) & 1).any() and not ((ev[:, 4] + ev[:, 5]) & 1).all()               # odd and even targets
    assert (C.corner_events("Jal")[:, 4] < 0).any() and (C.corner_events("Jal")[:, 4] > 0).any()     # backward and forward
    for name in ("UType", "Jal"):
        assert ((C.corner_events(name)[:, 2] >> 32) & 1).all()                                       # operand b is the immediate


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("name", C.CHIPS)
def test_every_word_equals_the_host_tracer(name, which, tmp_path):
    n, height = C.shapes(name)[which]
    ev, want = C.case(name, n, height)
    got = C.run_rows("host", name, ev, height, tmp_path)
    msg = C.first_difference(name, want, got, n)
    assert msg is None, msg


def test_shift_left_padding_is_the_template(tmp_path):
    got = C.run_rows("host", "ShiftLeft", C.corner_events("ShiftLeft")[:0], 32, tmp_path)
    lay = R.chip("ShiftLeft")[0].layout
    one = (1 << 32) % RT.P
    ones = sorted(lay[k] for k in ("v_01", "v_012", "v_0123"))
    for col in range(got.shape[0]):
        assert (got[col] == (one if col in ones else 0)).all(), col


def test_clock_windows(tmp_path):
    seen = 0
    for name, (ev, want) in C.clock_window_tables().items():
        n = ev.shape[0]
        got = C.run_rows("host", name, ev, want.shape[1], tmp_path)
        msg = C.first_difference(name, want, got, n)
        assert msg is None, msg
        lay = R.chip(name)[0].layout
        crossed = got[lay["adapter.op_a_memory.prev_low"], :n] == 0
        seen += int(crossed.any() and not crossed.all())
    assert seen == len(C.CLOCK_CHIPS)                          # both kinds of previous access occurred in every chip


def test_column_constants_and_widths_equal_the_transcribed_chips():
    text = subprocess.run([C.EXE, "host", "layout"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, col = line.split()
        air = R.chip(chip)[0]
        assert int(col) == (air.main_width if key == "width" else air.layout[key]), line
        seen.setdefault(chip, set()).add(key)
    for name in C.CHIPS:
        assert seen[name] == set(R.chip(name)[0].layout) | {"width"}, name
    text = subprocess.run([C.EXE, "host", "width"], check=True, capture_output=True, timeout=60).stdout.decode()
    assert [tuple(l.split()) for l in text.splitlines()] == [(n, str(R.chip(n)[0].main_width)) for n in C.CHIPS]


def _pack_alu_events_before(events, chip):
    """pack_alu_events as it stood when the device made eight chips, restated."""
    ev = events[np.nonzero(X.chip_of_events(np.asarray(events)) == chip)[0]]
    flags = ev[:, X.E_FLAGS]
    imm_c = (flags & 2) >> 1
    ops = ev[:, X.E_OP] | (ev[:, X.E_OPA] << 8) | ((ev[:, X.E_OPB] & 0xFF) << 16) | (((1 - imm_c) * (ev[:, X.E_OPC] & 0xFF)) << 24) | ((flags & 3) << 32)
    c = np.where(imm_c == 1, ev[:, X.E_OPC], ev[:, X.E_C])
    cols = [ev[:, X.E_PC], ev[:, X.E_CLK], ops, ev[:, X.E_A], ev[:, X.E_B], c, ev[:, X.E_A_PREV], ev[:, X.E_A_PTS], ev[:, X.E_B_PTS], ev[:, X.E_C_PTS],
            ev[:, X.E_NEXT_PC]]
    return np.stack(cols, 1)


def test_packing_of_the_first_eight_chips_is_unchanged():
    ex = X.Executor(X.guest_file("fibonacci.elf"), stdin=[struct.pack("<Q", 200)])
    sh = ex.run_shard(1 << 20)
    assert sh.halted
    some = 0
    for name in C.OLD_CHIPS:
        now, before = X.pack_alu_events(sh.events, name), _pack_alu_events_before(sh.events, name)
        assert now.dtype == before.dtype and now.shape == before.shape and now.tobytes() == before.tobytes(), name
        some += now.shape[0] > 0
    assert some >= 7
    _, csh, _, _ = C.corner()
    for name in C.OLD_CHIPS:
        assert X.pack_alu_events(csh.events, name).tobytes() == _pack_alu_events_before(csh.events, name).tobytes(), name
