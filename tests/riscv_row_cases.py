"""What tests/test_tracegen_riscv_host.py (CPU) and tests/test_gpu_tracegen_riscv_more.py (GPU) share: hand-assembled programs that
reach the corner cases of the fourteen instruction chips whose tables the device generates, their host tables (made once), the
packed event records, and tests/native/riscv_rows (built by __graft_entry__.build()) behind a function.

A row of these chips is a function of its own event alone, so the host table of a PREFIX of a chip's events is the first rows of
the full table followed by padding rows, and the table of the events repeated is the rows repeated: `case(name, n, height)` builds
both sides of every (events, height) shape that way. Everything is bit-exact; there are no tolerances."""
import copy
import functools
import os
import subprocess

import numpy as np
import torch

import rv_asm as A
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_trace as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "riscv_rows")
OLD_CHIPS = ("Add", "Addi", "Sub", "Addw", "Subw", "Mul", "ShiftRight", "Branch")
NEW_CHIPS = ("Bitwise", "Lt", "ShiftLeft", "UType", "Jal", "Jalr")
CHIPS = OLD_CHIPS + NEW_CHIPS                                  # index = SP1HIP_RV64_CHIP_*
M64 = (1 << 64) - 1
VALUES = [0, 1, M64, 1 << 63, (1 << 63) - 1, 0x8000_0000, 0x7FFF_FFFF, 0xFFFF_FFFF, 0x1234_5678_9ABC_DEF0, 0xFFFF_0000_FFFF_0001,
          0xFFFF, 0x1_0000]                                    # the last two: a compare that differs only in limb 0 / only in limb 1
IMMEDIATES = [-2048, -1, 0, 2047]
AMOUNTS = [0, 1, 15, 16, 31, 32, 47, 63]
SMALL_SHAPES = [(0, 32), (1, 32), (32, 32), (33, 64)]
TWO_WORKGROUPS = (257, 288)
NOP = A.enc("addi", 0, 0, 0)


class Program:
    """Instruction words and, beside them, how many rows each chip must get (an ALU instruction with rd = x0 is AluX0's)."""

    def __init__(self):
        self.words, self.rows = [], {}

    def count(self, chip, rd=1):
        chip = "AluX0" if rd == 0 and chip not in ("UType", "Jal", "Jalr", "Branch") else chip
        self.rows[chip] = self.rows.get(chip, 0) + 1

    def op(self, chip, name, *a):
        self.words.append(A.enc(name, *a))
        self.count(chip, a[0])

    def li(self, rd, value):
        for w in A.li(rd, value):                              # lui / addi / addiw / slli / ori, rd != x0
            opc, f3 = w & 0x7F, (w >> 12) & 7
            self.count({0x37: "UType", 0x1B: "Addw"}.get(opc) or {0: "Addi", 1: "ShiftLeft", 6: "Bitwise"}[f3])
            self.words.append(w)

    def skipped(self):
        self.words.append(NOP)                                 # jumped over: never executed, no row


def corner_program():
    """The corner cases of the six chips Bitwise, Lt, ShiftLeft, UType, Jal, Jalr, and enough of the eight others to give each of
    them rows (Add / Sub / Addw / Subw / Mul / ShiftRight on a third of the pairs, branches both ways, addi / addiw immediates)."""
    p = Program()
    for i, v in enumerate(VALUES):
        p.li(5, v)
        for j, w in enumerate(VALUES):
            p.li(6, w)
            for name in ("xor", "or", "and"):
                p.op("Bitwise", name, 7, 5, 6)
            for name in ("slt", "sltu"):                       # every pair: equal, limb 0 / 1 / 3 only, both signs at 2^63 / 2^63 - 1
                p.op("Lt", name, 7, 5, 6)
            if j % 3 == i % 3:
                for name, chip in (("mul", "Mul"), ("mulh", "Mul"), ("mulhu", "Mul"), ("mulhsu", "Mul"), ("mulw", "Mul"), ("add", "Add"), ("sub", "Sub"),
                                   ("addw", "Addw"), ("subw", "Subw"), ("srl", "ShiftRight"), ("sra", "ShiftRight"), ("srlw", "ShiftRight"),
                                   ("sraw", "ShiftRight")):
                    p.op(chip, name, 7, 5, 6)
                for name in ("beq", "bne", "blt", "bge", "bltu", "bgeu"):
                    p.words += [A.enc(name, 5, 6, 8), NOP]     # taken or not, execution goes on 8 bytes on; the nop runs when not taken
                    p.count("Branch")
        for name in ("xor", "or", "and"):
            p.op("Bitwise", name, 7, 0, 5)                     # rs1 = x0
            p.op("Bitwise", name, 7, 5, 5)                     # rs1 = rs2
            p.op("Bitwise", name, 0, 5, 6)                     # rd = x0: AluX0's row, not Bitwise's
        for name in ("slt", "sltu"):
            p.op("Lt", name, 7, 5, 5)                          # equal operands through one register
        for imm in IMMEDIATES:
            for name in ("xori", "ori", "andi"):
                p.op("Bitwise", name, 7, 5, imm)
            for name in ("slti", "sltiu"):                     # sltiu with -1 compares against 2^64 - 1
                p.op("Lt", name, 7, 5, imm)
        for amount in AMOUNTS + [M64]:                         # a register amount: only the low 6 (sll) or 5 (sllw) bits count
            p.li(6, amount)
            p.op("ShiftLeft", "sll", 7, 5, 6)
            p.op("ShiftLeft", "sllw", 7, 5, 6)
        for amount in AMOUNTS:
            p.op("ShiftLeft", "slli", 7, 5, amount)
            p.op("ShiftRight", "srli", 7, 5, amount)
            p.op("ShiftRight", "srai", 7, 5, amount)
            if amount < 32:                                    # 0x8000_0000 / 0x7FFF_FFFF by 0 and 1: sllw_msb set and clear
                p.op("ShiftLeft", "slliw", 7, 5, amount)
                p.op("ShiftRight", "srliw", 7, 5, amount)
                p.op("ShiftRight", "sraiw", 7, 5, amount)
        p.op("Addi", "addi", 7, 5, -2048)
        p.op("Addi", "addi", 7, 5, 2047)
        p.op("Addw", "addiw", 7, 5, -1)
    for imm in (0, 0x7FFFF000, 0x80000000, 0xFFFFF000):        # 0x80000000 and above sign-extend
        p.op("UType", "lui", 7, imm)
    for imm in (0, 0x12345000, 0x80000000):
        p.op("UType", "auipc", 7, imm)
    p.op("UType", "lui", 0, 0x1000)                            # rd = x0: still UType's rows, op_a_0 set
    p.op("UType", "auipc", 0, 0x1000)
    for rd in (0, 1):
        # forward over a skipped word; then  A: jal +8 -> C | B: jal rd, +8 -> D | C: jal rd, -4 -> B | D: ...
        p.op("Jal", "jal", rd, 8)
        p.skipped()
        p.op("Jal", "jal", 0, 8)
        p.op("Jal", "jal", rd, 8)
        p.op("Jal", "jal", rd, -4)
    for rd in (1, 0, 9):                                       # 9: rd = rs1
        for imm, odd in ((0, 0), (12, 0), (-8, 0), (2047, 0), (-2031, 0), (1, 1), (-3, 1)):
            # P: auipc x8, 0 | addi x9, x8, 16 + odd - imm | P + 8: jalr rd, x9, imm -> (P + 16 + odd) & ~1 | P + 12: skipped | P + 16: ...
            p.op("UType", "auipc", 8, 0)
            p.op("Addi", "addi", 9, 8, 16 + odd - imm)
            p.op("Jalr", "jalr", rd, 9, imm)
            p.skipped()
    return p


@functools.lru_cache(maxsize=None)
def corner():
    """(executor, shard, host tables {name: int64 [pad32(rows), width]}, expected rows per chip) of the corner program, made once."""
    p = corner_program()
    ex = X.Executor(A.elf(p.words + A.halt(0)), stdin=[])
    sh = ex.run_shard(1 << 20)
    assert sh.halted and sh.exit_code == 0
    _, tabs, _ = X.shard_tables(ex, sh, device="cpu")
    return ex, sh, {n: tabs[n][1] for n in tabs}, dict(p.rows)


@functools.lru_cache(maxsize=None)
def corner_events(name):
    """The chip's packed records of the corner shard: int64 numpy [rows, 11]."""
    _, sh, _, _ = corner()
    return np.ascontiguousarray(X.pack_alu_events(sh.events, name))


def padding_rows(name, rows):
    air = R.chip(name)[0]
    t = torch.zeros((rows, air.main_width), dtype=RT.I64)
    if name == "ShiftLeft":                                    # the reference's padded row template (alu/sll/mod.rs:L154-L160)
        for col in ("v_01", "v_012", "v_0123"):
            t[:, air.layout[col]] = 1
    elif name == "ShiftRight":                                 # alu/sr/mod.rs:L165-L171
        for col, v in (("v_01", 16), ("v_012", 256), ("v_0123", 65536)):
            t[:, air.layout[col]] = v
    return t


def take(rows, n):
    """The first n of `rows` (events or table rows), repeating them from the start when there are fewer."""
    idx = np.arange(n) % max(len(rows), 1)
    return rows[idx] if len(rows) else rows[:0]


def case(name, n, height):
    """(packed events [n, 11], the Montgomery column-major host table [width, height]) of the chip's first n corner events."""
    _, _, tabs, _ = corner()
    ev = corner_events(name)
    assert len(ev) or n == 0
    full = tabs[name][:len(ev)]
    want = torch.cat([take(full, n), padding_rows(name, height - n)])
    return np.ascontiguousarray(take(ev, n)), montgomery_col_major(want)


def shapes(name):
    n = len(corner_events(name))
    return SMALL_SHAPES + [(n, RT.pad32(n)), TWO_WORKGROUPS]


def montgomery_col_major(table):
    """int64 [height, width] canonical -> uint32 numpy [width, height] Montgomery words: what the device and the native program write."""
    return np.ascontiguousarray(RT.to_monty_np(table).T)


def group(name, col):
    lay = R.chip(name)[0].layout
    at = max(c for c in lay.values() if c <= col)
    return sorted(k for k, c in lay.items() if c == at)[0]


def first_difference(name, want, got, n):
    """None, or a message naming the first differing word of two [width, height] arrays by column, layout group and row."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: shape %s, want %s" % (name, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if not bad.shape[0]:
        return None
    col, row = (int(v) for v in bad[0])
    return ("%s with %d events: %d words differ; first at column %d (group %s), row %d (%s): got %#x, want %#x"
            % (name, n, bad.shape[0], col, group(name, col), row, "event" if row < n else "padding", int(got[col, row]), int(want[col, row])))


def run_rows(form, name, ev, height, tmp_path, timeout=120):
    """tests/native/riscv_rows FORM rows on an event file: the table as uint32 numpy [width, height]."""
    tag = "%s_%s_%d_%d" % (form, name, ev.shape[0], height)
    src, dst = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(ev, dtype=np.int64).tobytes())
    subprocess.run([EXE, form, "rows", str(CHIPS.index(name)), src, str(height), dst], check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.uint32).reshape(R.chip(name)[0].main_width, height)


# ---------------------------------------------------------------------------------------------------------------- clock windows
WINDOW = 1 << 24
# (clk relative to a multiple of 2^24, the previous timestamps of a / b / c relative to the same multiple). The accesses of c, b, a
# stand at clk + 2, + 3, + 4: -5 puts all three just below the boundary; -3 puts c just below, b exactly on it, a just above; -4
# puts a exactly on it; +8 puts all above. A previous access at -100 is in the window before whenever the current one is at >= 0.
CLOCK_PATTERNS = [(-5, (-100, -50, -7)), (-3, (-100, -2, -2)), (-3, (0, -100, -100)), (-4, (-100, -3, -3)), (-4, (-WINDOW + 5, -9, -9)),
                  (8, (-100, 1, 2)), (8, (11, -100, 9)), (-2, (1, -100, -100)), (-2, (-100, 0, -1))]
CLOCK_CHIPS = ("ShiftLeft", "UType", "Jal", "Jalr", "ShiftRight", "Mul", "Branch")


def clock_window_tables():
    """{name: (packed events, Montgomery column-major host table)} of the corner shard with clk and the three previous-timestamp
    words of every event rewritten to CLOCK_PATTERNS around multiples of 2^24. Both sides get the same records: the host side is
    the tracer's own fillers over the edited shard — the methods that fill one chip each; Bitwise, Lt and the value chips are
    closures of Tracer.build and share their adapters with ShiftLeft, Mul and Branch — so the records need not be an executable
    history."""
    ex, sh, _, _ = corner()
    ev = sh.events.copy()
    k = np.arange(len(ev))
    base = (3 + k // len(CLOCK_PATTERNS) % 5) * WINDOW
    pat = k % len(CLOCK_PATTERNS)
    ev[:, X.E_CLK] = base + np.array([c for c, _ in CLOCK_PATTERNS])[pat]
    for slot, word in enumerate((X.E_A_PTS, X.E_B_PTS, X.E_C_PTS)):
        ev[:, word] = base + np.array([p[slot] for _, p in CLOCK_PATTERNS])[pat]
    edited = copy.copy(sh)
    edited.events = ev
    tr = X.EventTracer(ex, edited, "cpu")
    tr.simple_alu("ShiftLeft", "ALU", tr.sll_extra)
    tr.simple_alu("ShiftRight", "ALU", tr.sr_extra)
    tr.simple_alu("Mul", "R", tr.mul_extra)
    tr.utype()
    tr.jal()
    tr.jalr()
    tr.branch()
    return {n: (np.ascontiguousarray(X.pack_alu_events(ev, n)), montgomery_col_major(tr.tables[n].main)) for n in CLOCK_CHIPS}


# ------------------------------------------------------------------------------------------------------- a small provable program
def all_six_program():
    """A small program with rows in each of Bitwise, Lt, ShiftLeft, UType, Jal, Jalr (and Add, Addi, Sub, Mul, Branch beside them)."""
    p = Program()
    for v, w in ((0x1234_5678_9ABC_DEF0, 0xFFFF_0000_FFFF_0001), (1 << 63, (1 << 63) - 1), (0xFFFF, 0x1_0000)):
        p.li(5, v)
        p.li(6, w)
        for chip, name in (("Bitwise", "xor"), ("Bitwise", "or"), ("Bitwise", "and"), ("Lt", "slt"), ("Lt", "sltu"), ("ShiftLeft", "sll"),
                           ("ShiftLeft", "sllw"), ("Add", "add"), ("Sub", "sub"), ("Mul", "mul")):
            p.op(chip, name, 7, 5, 6)
        p.op("Bitwise", "andi", 7, 5, -2048)
        p.op("Lt", "sltiu", 7, 5, -1)
        p.op("ShiftLeft", "slliw", 7, 5, 31)
        p.words += [A.enc("blt", 5, 6, 8), NOP]
        p.op("UType", "lui", 7, 0x80000000)
        p.op("Jal", "jal", 1, 8)
        p.skipped()
        p.op("UType", "auipc", 8, 0)
        p.op("Jalr", "jalr", 1, 8, 13)                         # an odd sum: execution goes on at the even address, 12 bytes on
        p.skipped()
    return p
