"""What tests/test_tracegen_riscv_core_host.py (CPU) and tests/test_gpu_tracegen_riscv_core.py (GPU) share: the events and records
of DivRem, AluX0 and MemoryLocal — synthetic ones on every corner of the division, a hand-assembled executed program, clocks around
multiples of 2^24 —, their host tables (made once, by the host tracer's own fillers) and tests/native/riscv_core_rows (built by
__graft_entry__.build()) behind functions.

A row of these chips is a function of its own event alone, so the host table of a PREFIX of a chip's events is the first rows of
the full table followed by padding rows, and the table of the events repeated is the rows repeated: `case(name, n, height)` builds
both sides of every (events, height) shape that way. Everything is bit-exact; there are no tolerances."""
import copy
import functools
import os
import subprocess

import numpy as np
import torch

import riscv_row_cases as C
import rv_asm as A
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_trace as RT

ROOT = C.ROOT
EXE = os.path.join(ROOT, "tests", "native", "riscv_core_rows")
CHIPS = ("DivRem", "AluX0", "MemoryLocal")
M64 = (1 << 64) - 1
DIVREM_OPS = ("div", "divu", "rem", "remu", "divw", "divuw", "remw", "remuw")
# 0, +-1, +-2, the ends of both signed ranges, the 32-bit ends zero- and sign-extended, 2^32 (a W form's zero divisor with a
# non-zero upper half) and a value whose limbs alternate
DIVREM_VALUES = [0, 1, 2, M64, M64 - 1, 1 << 63, (1 << 63) - 1, 0x8000_0000, 0x7FFF_FFFF, 0xFFFF_FFFF, 0xFFFF_FFFF_8000_0000, 0x1_0000_0000,
                 0x0000_FFFF_0000_FFFF]
SMALL_SHAPES = C.SMALL_SHAPES
TWO_WORKGROUPS = C.TWO_WORKGROUPS
DATA = 0x78100000                                              # rv_asm.elf's data segment

s64 = lambda v: (v & M64) - (1 << 64) if (v & M64) >> 63 else v & M64


# ------------------------------------------------------------------------------------------------------------ the executed program
def program():
    """Every DIV / REM form on operand pairs that include c = 0, INT_MIN / -1 in both widths and W operands with garbage upper
    halves; ALU instructions with rd = x0, a register and an immediate c; stores and loads, so that MemoryLocal has memory rows."""
    p = C.Program()
    pairs = [(7, 2), (M64 - 6, 2), (7, M64 - 1), (M64 - 6, M64 - 1), (5, 0), (M64, 0), (0x1234_5678_8000_0001, 0), (1 << 63, M64), (0x8000_0000, 0xFFFF_FFFF),
             (0xFFFF_FFFF_8000_0000, M64), (0xDEAD_BEEF_0000_0064, 0xFFFF_0001_0000_0007), (0x1_0000_0000, 0x1_0000_0000), (0, 5), (3, 3),
             (0x0000_FFFF_0000_FFFF, 0x1_0001), ((1 << 63) - 1, 1 << 63)]
    for b, c in pairs:
        p.li(5, b)
        p.li(6, c)
        for name in DIVREM_OPS:
            p.op("DivRem", name, 7, 5, 6)
        p.op("DivRem", "div", 5, 5, 6)                         # rd = rs1
    p.li(5, 0x1234_5678_9ABC_DEF0)
    p.li(6, 0xFFFF_0000_FFFF_0001)
    for chip, name in (("DivRem", "div"), ("DivRem", "remuw"), ("Add", "add"), ("Sub", "sub"), ("Bitwise", "xor"), ("ShiftLeft", "sll"), ("Mul", "mulh"),
                       ("Lt", "sltu"), ("ShiftRight", "sra"), ("Addw", "addw")):
        p.op(chip, name, 0, 5, 6)                              # rd = x0, c a register: AluX0's row
    for chip, name, imm in (("Addi", "addi", -2048), ("Bitwise", "xori", 2047), ("Bitwise", "andi", -1), ("Lt", "slti", 5), ("ShiftLeft", "slli", 63),
                            ("ShiftRight", "srai", 1), ("Addw", "addiw", -1)):
        p.op(chip, name, 0, 5, imm)                            # rd = x0, c an immediate
    p.li(8, DATA)
    for k, reg in enumerate((5, 6, 7)):
        p.words.append(A.enc("sd", reg, 8, 8 * k))
        p.count("StoreDouble")
    p.words.append(A.enc("sb", 6, 8, 29))                      # bytes 4 and 5 of the word at DATA + 24
    p.count("StoreByte")
    p.words.append(A.enc("ld", 9, 8, 8))
    p.count("LoadDouble")
    p.words.append(A.enc("ld", 9, 8, 40))                      # read only: initial value = final value
    p.count("LoadDouble")
    p.li(10, DATA + 64)                                        # KECCAK_PERMUTE on the 25 words at DATA + 64: a SyscallCore row, whose
    p.op("Addi", "addi", 11, 0, 0)                             # Global event goes behind MemoryLocal's
    p.li(5, KECCAK_PERMUTE)
    p.words.append(A.enc("ecall"))
    p.count("SyscallInstrs")
    return p


KECCAK_PERMUTE = 0x00010109                                    # SyscallCode::KECCAK_PERMUTE


def data_bytes():
    words = [0, 0, 0, 0x0000_FF00_0000_0000, 0x0000_00FF_1234_5678, 0xFFFF_FFFF_FFFF_FFFF, 0, 0] + list(range(1, 26))
    return b"".join(int(w).to_bytes(8, "little") for w in words)


@functools.lru_cache(maxsize=None)
def executed():
    """(executor, shard, the host tracer after build(), host tables {name: int64 [pad32(rows), width]}, expected rows per chip)."""
    p = program()
    ex = X.Executor(A.elf(p.words + A.halt(0), data=data_bytes(), data_addr=DATA), stdin=[])
    sh = ex.run_shard(1 << 20)
    assert sh.halted and sh.exit_code == 0
    tr = X.EventTracer(ex, sh, "cpu")
    _, tabs, _ = tr.build()
    return ex, sh, tr, {n: tabs[n][1] for n in tabs}, dict(p.rows)


# -------------------------------------------------------------------------------------------------------- synthetic DivRem events
@functools.lru_cache(maxsize=None)
def synthetic_divrem():
    """(packed events [8 x 169, 11], host table int64 [pad32, 246]): every opcode on every ordered pair of DIVREM_VALUES, a from
    divrem_result, clocks and previous timestamps of a plausible history. The host side is the tracer's simple_alu over these
    records: CPUState and the R adapter from fill_state / fill_adapter, everything else from divrem_rows."""
    ex, sh, _, _, _ = executed()
    rows = []
    for name in DIVREM_OPS:
        for b in DIVREM_VALUES:
            for c in DIVREM_VALUES:
                i = len(rows)
                e = [0] * X.EV_WORDS
                clk = sh.clk_start + 8 * (i + 3)
                e[X.E_PC], e[X.E_CLK], e[X.E_OP], e[X.E_NEXT_PC] = 0x78000000 + 4 * i, clk, R.OPC[name.upper()], 0x78000000 + 4 * i + 4
                e[X.E_OPA], e[X.E_OPB], e[X.E_OPC] = 7 + i % 3, 5, 6
                e[X.E_B], e[X.E_C] = s64(b), s64(c)
                e[X.E_A] = RT.divrem_result(e[X.E_OP], s64(b), s64(c))[0]
                e[X.E_A_PREV] = s64(0x0123_4567_89AB_CDEF * (i + 1))
                e[X.E_A_PTS], e[X.E_B_PTS], e[X.E_C_PTS] = max(clk - 20 - i % 7, 0), clk - 8 + 3, clk - 8 * (1 + i % 4) + 2
                rows.append(e)
    ev = np.array(rows, dtype=np.int64)
    edited = copy.copy(sh)
    edited.events = ev
    tr = X.EventTracer(ex, edited, "cpu")
    tr.simple_alu("DivRem", "R", tr.divrem_extra)
    return np.ascontiguousarray(X.pack_alu_events(ev, "DivRem")), tr.tables["DivRem"].main


@functools.lru_cache(maxsize=None)
def events(name, source="program"):
    """Packed records and the host rows (no padding) of `name` from the executed program, or DivRem's synthetic set."""
    if source == "synthetic":
        ev, tab = synthetic_divrem()
        return ev, tab[:len(ev)]
    _, sh, _, tabs, _ = executed()
    ev = np.ascontiguousarray(sh.local if name == "MemoryLocal" else X.pack_alu_events(sh.events, name))
    return ev, tabs[name][:len(ev)]


def padding_rows(name, rows):
    air = R.chip(name)[0]
    if name == "DivRem":                                       # the reference's "0 / 1" rows, as divrem_rows appends them
        return torch.as_tensor(RT.divrem_rows(air.layout, air.main_width, rows, [], [], []))
    return torch.zeros((rows, air.main_width), dtype=RT.I64)


def case(name, n, height, source="program"):
    """(records [n, words], the Montgomery column-major host table [width, height]) of the first n records of the source."""
    ev, full = events(name, source)
    assert len(ev) or n == 0
    want = torch.cat([C.take(full, n), padding_rows(name, height - n)])
    return np.ascontiguousarray(C.take(ev, n)), C.montgomery_col_major(want)


def shapes(name, source="program"):
    n = len(events(name, source)[0])
    return SMALL_SHAPES + [TWO_WORKGROUPS, (n, RT.pad32(n))]


def first_difference(name, want, got, n):
    return C.first_difference(name, want, got, n)


# ---------------------------------------------------------------------------------------------------------------- clock windows
def clock_window_tables():
    """{name: (packed events, Montgomery column-major host table)} for DivRem and AluX0 of the executed shard with clk and the three
    previous-timestamp words of every event rewritten to riscv_row_cases.CLOCK_PATTERNS around multiples of 2^24; the host side is
    the tracer's own fillers over the edited shard (simple_alu with divrem_extra, and EventTracer.build's AluX0 closure restated)."""
    ex, sh, _, _, _ = executed()
    ev = sh.events.copy()
    k = np.arange(len(ev))
    base = (3 + k // len(C.CLOCK_PATTERNS) % 5) * C.WINDOW
    pat = k % len(C.CLOCK_PATTERNS)
    ev[:, X.E_CLK] = base + np.array([c for c, _ in C.CLOCK_PATTERNS])[pat]
    for slot, word in enumerate((X.E_A_PTS, X.E_B_PTS, X.E_C_PTS)):
        ev[:, word] = base + np.array([p[slot] for _, p in C.CLOCK_PATTERNS])[pat]
    edited = copy.copy(sh)
    edited.events = ev
    tr = X.EventTracer(ex, edited, "cpu")
    tr.simple_alu("DivRem", "R", tr.divrem_extra)

    def alu_x0(tb, k, p, a, bv, cv):
        tb.set("opcode", tr.ex.op[p])
        tb.set("is_real", 1)
    tr.simple_alu("AluX0", "ALU", alu_x0)
    return {n: (np.ascontiguousarray(X.pack_alu_events(ev, n)), C.montgomery_col_major(tr.tables[n].main)) for n in ("DivRem", "AluX0")}


# ------------------------------------------------------------------------------------------------------------ MemoryLocal records
def synthetic_records():
    """[48, 5] int64 records { addr, initial clk, initial value, final clk, final value }: register addresses below 32, addresses
    with all three limbs set up to 2^48 - 8, initial clk 0, clks one below, on and above multiples of 2^24, and values whose bytes 4
    and 5 are 0x00 / 0xFF in each combination (initial and final independently)."""
    addrs = [0, 5, 31, DATA, 0x1234_5678_9AB8, 0xFFFF_FFFF_FFF8, (1 << 48) - 8, 0x0001_0000_0000]
    W = 1 << 24
    clks = [(0, 9), (0, W), (W - 1, W), (W - 1, W + 1), (W, W + 1), (W + 1, 3 * W - 1), (2 * W, 2 * W + 5), (5 * W - 1, 5 * W), (7, 7 * W + 1)]
    byte45 = [(0x00, 0x00), (0xFF, 0x00), (0x00, 0xFF), (0xFF, 0xFF), (0x80, 0x7F)]
    rec = []
    for i in range(48):
        (it, ft), (i4, i5), (f4, f5) = clks[i % len(clks)], byte45[i % len(byte45)], byte45[(i // 5 + i) % len(byte45)]
        iv = 0xA1B2_0000_0000_C3D4 + (i << 16) | i4 << 32 | i5 << 40
        fv = (0xFFFF_0000_0000_0000 if i % 3 else 0x0001_0000_FFFF_0000) | f4 << 32 | f5 << 40 | i
        rec.append([addrs[i % len(addrs)], it, s64(iv), ft, s64(fv)])
    return np.array(rec, dtype=np.int64)


def memory_local_host(records):
    """(the tracer's MemoryLocal table of `records`: int64 [pad32(n), 20]; its rows' Global events in the 9-word form, int32
    [2 n, 9]: eval_interactions over the host table, receive then send per row, reduced to message[8], is_receive | kind << 8)."""
    ex, sh, _, _, _ = executed()
    edited = copy.copy(sh)
    edited.local = np.ascontiguousarray(records)
    tr = X.EventTracer(ex, edited, "cpu")
    tr.memory_local_and_bumps()
    ml = tr.tables["MemoryLocal"]
    (_, recv, _), (_, send, _) = RT.eval_interactions(R.chip("MemoryLocal")[1], ml.main[:ml.n], None, kinds=(R.GLOBAL,))
    ev11 = torch.stack([recv, send], dim=1).reshape(-1, 11)
    return ml.main, reduce_global_events(ev11)


def reduce_global_events(ev11):
    ev11 = ev11.cpu().numpy().astype(np.int64)
    return np.concatenate([ev11[:, :8], (ev11[:, 9] | (ev11[:, 10] << 8))[:, None]], axis=1).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------- the native program
def run_rows(name, ev, height, tmp_path, timeout=120):
    """tests/native/riscv_core_rows host rows on a record file: the table as uint32 numpy [width, height]."""
    tag = "%s_%d_%d" % (name, ev.shape[0], height)
    src, dst = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(ev, dtype=np.int64).tobytes())
    subprocess.run([EXE, "host", "rows", name, src, str(height), dst], check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.uint32).reshape(R.chip(name)[0].main_width, height)


def run_global(records, tmp_path, timeout=120):
    """tests/native/riscv_core_rows host global: the records' Global events as int32 numpy [2 n, 9]."""
    src, dst = os.path.join(str(tmp_path), "global_%d.in" % len(records)), os.path.join(str(tmp_path), "global_%d.out" % len(records))
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(records, dtype=np.int64).tobytes())
    subprocess.run([EXE, "host", "global", src, dst], check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.int32).reshape(-1, 9)
