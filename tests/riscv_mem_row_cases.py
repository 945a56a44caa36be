"""What tests/test_tracegen_riscv_mem_host.py (CPU) and tests/test_gpu_tracegen_riscv_mem.py (GPU) share: a hand-assembled program
that reaches the corner cases of the nine load and store chips whose tables the device generates, its host tables (made once), the
packed event records, and tests/native/riscv_mem_rows (built by __graft_entry__.build()) behind a function.

As in riscv_row_cases, a row of these chips is a function of its own event alone (the executor recorded address, previous word and
new word), so the host table of a PREFIX of a chip's events is the first rows of the full table followed by zero rows, and the table
of the events repeated is the rows repeated. Everything is bit-exact; there are no tolerances."""
import copy
import functools
import os
import struct
import subprocess

import numpy as np
import torch

import riscv_row_cases as C
import rv_asm as A
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_trace as RT

EXE = os.path.join(C.ROOT, "tests", "native", "riscv_mem_rows")
CHIPS = ("LoadByte", "LoadHalf", "LoadWord", "LoadDouble", "LoadX0", "StoreByte", "StoreHalf", "StoreWord", "StoreDouble")   # index = SP1HIP_RV64_MEM_CHIP_*
WIDTHS = (47, 44, 44, 39, 48, 50, 45, 44, 39)
M64 = C.M64
DATA = 0x78100000                                              # rv_asm.elf's data segment
# the sign bit of every byte, half and word position set and clear
EDGE = [0, M64, 0x0080_0080_0080_0080, 0xFF7F_FF7F_FF7F_FF7F, 0x8000_0000_7FFF_FFFF, 0x7FFF_FFFF_8000_0000, 0x0123_4567_89AB_CDEF]
REGISTER_BYTES = [0, 0x7F, 0x80, 0xFF]
IMMEDIATES = C.IMMEDIATES                                      # -2048, -1, 0, 2047
LOADS = {"lb": "LoadByte", "lbu": "LoadByte", "lh": "LoadHalf", "lhu": "LoadHalf", "lw": "LoadWord", "lwu": "LoadWord", "ld": "LoadDouble"}
STORES = {"sb": "StoreByte", "sh": "StoreHalf", "sw": "StoreWord", "sd": "StoreDouble"}
SIZE = {"lb": 1, "lbu": 1, "lh": 2, "lhu": 2, "lw": 4, "lwu": 4, "ld": 8, "sb": 1, "sh": 2, "sw": 4, "sd": 8}
# the data segment: the edge words, then a fresh word for every sb (32 of zeros, 32 of ones: a byte store into a word of zeros can
# only add to its limb, into a word of ones only take away), then words the wider stores write over and over
ZEROS, ONES, SCRATCH = 8 * len(EDGE), 8 * len(EDGE) + 256, 8 * len(EDGE) + 512
SCRATCH_WORDS = [0x0123_4567_89AB_CDEF, M64, 0, 0x8000_0000_7FFF_FFFF, 0, 0, 0, 0]
DATA_WORDS = EDGE + [0] * 32 + [M64] * 32 + SCRATCH_WORDS
BASE, OTHER, DEST = 5, 6, 7                                    # x5 holds DATA throughout; x6 is the register that changes


class Program(C.Program):
    def mem(self, name, ra, rs1, imm):
        """One load (ra = rd) or store (ra = rs2) at rs1 + imm."""
        self.words.append(A.enc(name, ra, rs1, imm))
        chip = LOADS.get(name) or STORES[name]
        chip = "LoadX0" if name in LOADS and ra == 0 else chip
        self.rows[chip] = self.rows.get(chip, 0) + 1


def every_aligned(name, word_offset):
    return [word_offset + off for off in range(0, 8, SIZE[name])]


def corner_program():
    p = Program()
    p.li(BASE, DATA)
    for i in range(len(EDGE)):                                 # every load at every alignment of every edge word; another load goes
        for name in (list(LOADS) * 2)[i:i + len(LOADS)]:       # first at each word, so every chip has a first access and repeated ones
            for at in every_aligned(name, 8 * i):
                p.mem(name, DEST, BASE, at)
    for k, name in enumerate(LOADS):                           # rd = x0: LoadX0's rows (7 here, 4 below), whatever the width
        p.mem(name, 0, BASE, 8 * (k % len(EDGE)) + (8 - SIZE[name]))
    for name in LOADS:                                         # rd = rs1
        p.li(OTHER, DATA + 8 * 3)
        p.mem(name, OTHER, OTHER, 8 - SIZE[name])
    for imm in IMMEDIATES:                                     # the base register adjusted so that the address stays in the segment
        for name, target in (("lb", 8 * 2 + 3), ("lhu", 8 * 3 + 6), ("lw", 8 * 4 + 4), ("ld", 8 * 5), ("lbu", 8 * 6 + 7)):
            p.li(OTHER, DATA + target - imm)
            p.mem(name, DEST, OTHER, imm)
        p.li(OTHER, DATA + 8 - imm)
        p.mem("ld", 0, OTHER, imm)
    fresh = {ZEROS: 0, ONES: 0}
    for region in (ZEROS, ONES):                               # sb: 8 offsets x 4 register bytes x memory words 0 and 2^64 - 1
        for off in range(8):
            for rb in REGISTER_BYTES:
                p.li(OTHER, 0x5A00 | rb)                       # only the low byte is stored
                p.mem("sb", OTHER, BASE, region + 8 * fresh[region] + off)
                fresh[region] += 1
    p.li(OTHER, 0xFEDC_BA98_7654_3210)
    for w in range(4):                                         # sh at 4 offsets, sw at 2, sd: over four different words, each written
        for name in ("sh", "sw", "sd"):                        # again and again (the previous word is the last store's)
            for at in every_aligned(name, SCRATCH + 8 * w):
                p.mem(name, OTHER, BASE, at)
        p.mem("ld", DEST, BASE, SCRATCH + 8 * w)               # ... and read back
    for name in STORES:                                        # rs2 = x0 (op_a_0 set) and rs1 = rs2 (the address is the value stored)
        p.mem(name, 0, BASE, SCRATCH + 8 * 4 + (8 - SIZE[name]))
        p.mem(name, BASE, BASE, SCRATCH + 8 * 5)
    for imm in IMMEDIATES:
        for name, target in (("sb", SCRATCH + 8 * 6 + 5), ("sh", SCRATCH + 8 * 6 + 2), ("sw", SCRATCH + 8 * 7 + 4), ("sd", SCRATCH + 8 * 7)):
            p.li(DEST, DATA + target - imm)
            p.mem(name, OTHER, DEST, imm)
    return p


def data_bytes(words=None):
    return b"".join(struct.pack("<Q", w) for w in (DATA_WORDS if words is None else words))


@functools.lru_cache(maxsize=None)
def corner():
    """(executor, shard, host tables {name: int64 [pad32(rows), width]}, expected rows per chip) of the corner program, made once."""
    p = corner_program()
    ex = X.Executor(A.elf(p.words + A.halt(0), data=data_bytes(), data_addr=DATA), stdin=[])
    sh = ex.run_shard(1 << 20)
    assert sh.halted and sh.exit_code == 0
    _, tabs, _ = X.shard_tables(ex, sh, device="cpu")
    return ex, sh, {n: tabs[n][1] for n in tabs}, dict(p.rows)


@functools.lru_cache(maxsize=None)
def corner_events(name):
    """The chip's packed records of the corner shard: int64 numpy [rows, 12]."""
    _, sh, _, _ = corner()
    return np.ascontiguousarray(X.pack_mem_events(sh.events, name))


def case(name, n, height):
    """(packed events [n, 12], the Montgomery column-major host table [width, height]) of the chip's first n corner events, repeated
    from the start when there are fewer; the rows behind them are zero rows."""
    _, _, tabs, _ = corner()
    ev = corner_events(name)
    assert len(ev) or n == 0
    full = tabs[name][:len(ev)]
    want = torch.cat([C.take(full, n), torch.zeros((height - n, full.shape[1]), dtype=RT.I64)])
    return np.ascontiguousarray(C.take(ev, n)), C.montgomery_col_major(want)


def shapes(name):
    n = len(corner_events(name))
    return C.SMALL_SHAPES + [(n, RT.pad32(n)), C.TWO_WORKGROUPS]


first_difference = C.first_difference


def run_rows(form, name, ev, height, tmp_path, timeout=120):
    """tests/native/riscv_mem_rows FORM rows on an event file: the table as uint32 numpy [width, height]."""
    tag = "%s_%s_%d_%d" % (form, name, ev.shape[0], height)
    src, dst = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(ev, dtype=np.int64).tobytes())
    subprocess.run([EXE, form, "rows", str(CHIPS.index(name)), src, str(height), dst], check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.uint32).reshape(R.chip(name)[0].main_width, height)


# ---------------------------------------------------------------------------------------------------------------- clock windows
WINDOW = C.WINDOW
FAR = 70000                                                    # windows: a difference of the windows' numbers that needs diff_high_limb
# (clk, the previous timestamps of op_a / op_b / the memory word), all relative to a multiple of 2^24. The memory access stands at
# clk + 1, the accesses of op_b and op_a at clk + 3 and clk + 4.
CLOCK_PATTERNS = [
    (-5, (-100, -50, -7)),                                     # everything just below the boundary, previous accesses in the same window
    (-2, (-100, -50, -2)),                                     # memory just below (difference 0), the registers just above against the window before
    (-1, (-100, -100, -9)),                                    # memory exactly on the boundary against the window before: windows differ by 1
    (-1, (0, 1, -3 * WINDOW - 5)),                           # ... against four windows before; the registers in their own window
    (0, (1, 2, 0)),                                            # memory just above against the boundary itself: low difference 0
    (0, (-100, -100, -FAR * WINDOW + 5)),                      # many windows before: diff_high_limb != 0 in the comparison of windows
    (8, (9, 10, -1)),                                          # everything above, memory against the window before
    (100000, (11, 12, 5)),                                     # same window, low difference >= 2^16: diff_high_limb != 0 in the low comparison
    (-4, (-100, -3, -WINDOW - 3)),                             # op_a exactly on the boundary; memory against the window before, both below
    (-3, (-4, -100, -WINDOW * 2)),                             # op_b exactly on the boundary; memory against a boundary two windows before
]


def clock_window_tables():
    """{name: (packed events, Montgomery column-major host table)} of the corner shard with clk and the previous-timestamp words of
    the two registers and of the memory word rewritten to CLOCK_PATTERNS around multiples of 2^24. Both sides get the same records:
    the host side is EventTracer.memory_instructions() over the edited shard, so the records need not be an executable history."""
    ex, sh, _, _ = corner()
    ev = sh.events.copy()
    k = np.arange(len(ev))
    base = (FAR + 10 + k // len(CLOCK_PATTERNS) % 5) * WINDOW
    pat = k % len(CLOCK_PATTERNS)
    ev[:, X.E_CLK] = base + np.array([c for c, _ in CLOCK_PATTERNS])[pat]
    for slot, word in enumerate((X.E_A_PTS, X.E_B_PTS, X.E_M_PTS)):
        ev[:, word] = base + np.array([p[slot] for _, p in CLOCK_PATTERNS])[pat]
    edited = copy.copy(sh)
    edited.events = ev
    tr = X.EventTracer(ex, edited, "cpu")
    tr.memory_instructions()
    return {n: (np.ascontiguousarray(X.pack_mem_events(ev, n)), C.montgomery_col_major(tr.tables[n].main)) for n in CHIPS}


# ------------------------------------------------------------------------------------------------------- a small provable program
def all_nine_program():
    """A few dozen instructions with rows in each of the nine chips (and UType, Addi, Addw, ShiftLeft, Bitwise from the constants)."""
    p = Program()
    p.li(BASE, DATA)
    p.li(OTHER, 0xFEDC_BA98_7654_3280)
    for name, at in (("lb", 8 * 2 + 1), ("lbu", 8 * 3 + 7), ("lh", 8 * 2 + 2), ("lhu", 8 * 3 + 6), ("lw", 8 * 4 + 4), ("lwu", 8 * 5), ("ld", 8 * 6)):
        p.mem(name, DEST, BASE, at)
    p.mem("lw", 0, BASE, 8)
    p.mem("ld", 0, BASE, 16)
    for name, at in (("sb", ZEROS + 3), ("sb", ONES + 6), ("sh", SCRATCH + 2), ("sw", SCRATCH + 8 + 4), ("sd", SCRATCH + 16), ("sd", SCRATCH + 16)):
        p.mem(name, OTHER, BASE, at)
    p.mem("sb", 0, BASE, ONES + 8)
    p.mem("ld", DEST, BASE, SCRATCH + 16)
    return p
