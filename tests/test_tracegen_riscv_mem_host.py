"""CPU: the rows of the nine load and store chips as the device kernels compute them, run on the host.
tests/native/riscv_mem_rows (built by __graft_entry__.build()) includes sp1_amd/csrc/tg_riscv_mem_rows.hpp unchanged; its `host` form
runs the same fill_mem_row<CHIP> the kernels of tracegen_riscv_mem.hip call, on the CPU, and never opens a GPU.

* every word of every column equals the host tracer's (riscv_exec.shard_tables on the CPU: Tracer.fill_mem_chip driven by
  EventTracer.memory_instructions), zero padding rows included, for all nine chips at (events, height) = (0, 32), (1, 32), (32, 32)
  — no padding —, (33, 64), the whole corner set at its pad32 and (257, 288) — more than one 256-lane workgroup —, over the program
  of tests/riscv_mem_row_cases.py: every load at every alignment of words that set and clear the sign bit of every byte, half and
  word, each load with rd = x0 (LoadX0's rows: the count is asserted) and rd = rs1, sb at all 8 offsets with register bytes 0, 0x7f,
  0x80, 0xff into words of zeros and of ones (both signs of `increment` in both byte lanes), sh / sw / sd at every alignment, rs2 =
  x0, rs1 = rs2, immediates -2048, -1, 0, 2047, first and repeated accesses to a word;
* the same with clk and the previous timestamps of op_a, op_b and the memory word rewritten around multiples of 2^24: the memory
  access below, on and above the boundary against a previous access in the same window, the window before and many windows before,
  with diff_high_limb != 0 in both kinds of comparison;
* the program's column constants equal R.chip(name)[0].layout and its widths main_width;
* pack_mem_events gives the same records from numpy and from torch input.
Everything is bit-exact; there are no tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import riscv_mem_row_cases as M  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(M.EXE), "tests/native/riscv_mem_rows is not built: run __graft_entry__.build()"


def test_the_chips_are_the_device_chips():
    from sp1_amd import api
    assert tuple(X.MEM_TRACEGEN_CHIPS) == M.CHIPS
    assert api.RISCV_MEM_CHIPS == {n: i for i, n in enumerate(M.CHIPS)}
    assert api.MEM_EVENT_WORDS == 12
    assert tuple(R.RECORDED[n][0] for n in M.CHIPS) == M.WIDTHS == tuple(R.chip(n)[0].main_width for n in M.CHIPS)


def test_the_corner_program_reaches_every_chip_with_the_rows_it_should():
    _, sh, tabs, rows = M.corner()
    names = X.chip_of_events(sh.events)
    for name in M.CHIPS:
        assert int((names == name).sum()) == rows[name] == len(M.corner_events(name)) > 0, name
        assert tabs[name].shape[0] == RT.pad32(rows[name])
        assert not tabs[name][rows[name]:].any(), name           # the host tracer pads these nine with zero rows
    assert rows["LoadX0"] == 7 + len(M.IMMEDIATES)
    x0 = M.corner_events("LoadX0")
    assert sorted(set(int(o) for o in x0[:, 2] & 0xFF)) == sorted(RT.OPC[n] for n in RT.LOAD_KINDS["LoadX0"])    # each of the seven loads
    assert not ((x0[:, 2] >> 8) & 0xFF).any()
    lay = R.chip("StoreByte")[0].layout
    sb, t = M.corner_events("StoreByte"), tabs["StoreByte"]
    inc, bit0 = t[:rows["StoreByte"], lay["increment"]], t[:rows["StoreByte"], lay["offset_bit"]]
    for lane in (0, 1):                                          # both signs of `increment` (and zero) in both byte lanes
        v = inc[bit0 == lane]
        assert ((v > 0) & (v < RT.P // 2)).any() and (v > RT.P // 2).any() and (v == 0).any(), lane
    assert sorted(set(int(a) & 7 for a in sb[:, 8])) == list(range(8))
    for name in ("StoreByte", "StoreHalf", "StoreWord", "StoreDouble"):
        ev = M.corner_events(name)
        ra, rb = (ev[:, 2] >> 8) & 0xFF, (ev[:, 2] >> 16) & 0xFF
        assert (ra == 0).any() and (ra == rb).any(), name        # rs2 = x0, rs1 = rs2
    for name in ("LoadByte", "LoadHalf", "LoadWord", "LoadDouble"):
        ev = M.corner_events(name)
        assert (((ev[:, 2] >> 8) & 0xFF) == ((ev[:, 2] >> 16) & 0xFF)).any(), name                               # rd = rs1
        assert (ev[:, 9] == 0).any() and (ev[:, 9] != 0).any(), name                                             # first and repeated accesses
        msb = tabs[name][:rows[name], R.chip(name)[0].layout["msb"]] if name != "LoadDouble" else None
        assert msb is None or ((msb == 1).any() and (msb == 0).any()), name
    for name in ("LoadByte", "LoadDouble", "StoreByte", "StoreDouble"):
        assert set(M.IMMEDIATES) <= set(int(i) for i in M.corner_events(name)[:, 4]), name


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("name", M.CHIPS)
def test_every_word_equals_the_host_tracer(name, which, tmp_path):
    n, height = M.shapes(name)[which]
    ev, want = M.case(name, n, height)
    got = M.run_rows("host", name, ev, height, tmp_path)
    msg = M.first_difference(name, want, got, n)
    assert msg is None, msg


def test_clock_windows(tmp_path):
    for name, (ev, want) in M.clock_window_tables().items():
        n = ev.shape[0]
        got = M.run_rows("host", name, ev, want.shape[1], tmp_path)
        msg = M.first_difference(name, want, got, n)
        assert msg is None, msg
        lay = R.chip(name)[0].layout
        col = lambda key: got[lay[key], :n]
        crossed = col("adapter.op_b_memory.prev_low") == 0
        assert crossed.any() and not crossed.all(), name         # a register's previous access in the window before, and in its own
        low = col("memory_access.compare_low") != 0
        high = col("memory_access.diff_high_limb") != 0
        assert (low & high).any() and (~low & high).any() and (low & ~high).any() and (~low & ~high).any(), name


def test_column_constants_and_widths_equal_the_transcribed_chips():
    text = subprocess.run([M.EXE, "host", "layout"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, col = line.split()
        air = R.chip(chip)[0]
        assert int(col) == (air.main_width if key == "width" else air.layout[key]), line
        seen.setdefault(chip, set()).add(key)
    for name in M.CHIPS:
        assert seen[name] == set(R.chip(name)[0].layout) | {"width"}, name
    text = subprocess.run([M.EXE, "host", "width"], check=True, capture_output=True, timeout=60).stdout.decode()
    assert [tuple(l.split()) for l in text.splitlines()] == [(n, str(w)) for n, w in zip(M.CHIPS, M.WIDTHS)]


def test_packing_agrees_between_numpy_and_torch():
    _, sh, _, _ = M.corner()
    names = X.chip_of_events(sh.events)
    for name in M.CHIPS:
        a = X.pack_mem_events(sh.events, name)
        b = X.pack_mem_events(torch.as_tensor(sh.events), name)
        assert isinstance(a, np.ndarray) and torch.is_tensor(b) and b.is_contiguous() and b.dtype == torch.int64
        assert a.dtype == np.int64 and a.shape == tuple(b.shape) == (int((names == name).sum()), 12)
        assert np.array_equal(a, b.numpy()), name
        rows = np.nonzero(names == name)[0]                      # the events' order is the row order, and a selection packs the same
        assert np.array_equal(a, X.pack_mem_events(sh.events[rows])), name
        assert np.array_equal(a[:, 1], sh.events[rows, X.E_CLK]) and np.array_equal(a[:, 8], sh.events[rows, X.E_MADDR])
        assert np.array_equal(a[:, 8], a[:, 3] + a[:, 4]), name  # address = base + immediate
