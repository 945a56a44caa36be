"""What the trace-generation tests of the Weierstrass and Fp / Fp2 precompile chips share (tests/test_tracegen_field_chips_host.py on
the CPU, tests/test_gpu_tracegen_field_chips.py on the GPU): the operand sets with the modulus as a parameter, the family event
records made from them, the host filler's chip tables (riscv_more_trace.family_shard_from: the reference of every comparison, made
once per shape), the file interface of tests/native/field_chip_rows and the hand-assembled programs. It follows tests/secp_cases.py.

Operands. Per field of modulus p and L byte limbs, eleven edge elements: 0, 1, 2, 3, p - 1, p - 2, (p - 1) / 2, (p + 1) / 2,
2^128 - 1, 2^(8 (L - 1)) - 1 and 0xAB 2^(8 (L - 2)) + 0xCD (zero bytes in the middle).
* curve additions: every ordered pair (p.x, q.x) of distinct edge elements (110) with p.y, q.y drawn from the same list by a seeded
  generator, one case with p.y = q.y (slope 0), 16 pairs of multiples of the generator (checked against Python's affine
  arithmetic), then seeded random elements;
* curve doublings: every (p.x, p.y) of edge elements with p.y != 0 (110), 16 multiples of the generator, random elements;
* Fp: every ordered pair (x, y) of edge elements (121), then random pairs; the opcode cycles by row, i % 3 = add, sub, mul, so every
  wave mixes the three (and every pair meets every opcode, since 121 is no multiple of 3, once the set is cycled);
* Fp2 add / sub and mul: the same pairs in component 0 with the pair 37 places on in component 1, then random; add / sub cycles
  i % 2.
The points need not lie on a curve: the filler does not care. The words written are computed here in Python integers; the host
builder asserts them. Clocks, previous timestamps and pointers follow secp_cases._timing: a call on the first tick of a 2^24
window, previous timestamps on both sides of the boundary and at clk - 1, pointers with full upper limbs, a pointer where + 8 i
carries into the second limb."""
import os
import random
import struct
import subprocess

import numpy as np
import torch

from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_more as M
from sp1_amd.machines import riscv_more_trace as MT
from sp1_amd.machines import riscv_trace as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "field_chip_rows")
KINDS = tuple(X.FAMILIES)[:12]                                      # in SP1HIP_RV64_FAMILY_* order
FAMILY = {k: X.FAMILIES[k][0] for k in KINDS}
CHIPS = {k: X.FAMILIES[k][1] for k in KINDS}
SHAPE = {k: MT.FAMILY_SHAPES[k][1] for k in KINDS}
M64 = (1 << 64) - 1
CLK0 = (5 << 24) + 1001
SHAPES = [(0, 32), (1, 32), (32, 32), (33, 64)]                     # (events, height) for every kind
LARGE = (300, 320)                                                  # crosses a 256-lane workgroup; one N = 8 and one N = 12 kind per shape
LARGE_KINDS = ("bn254_add", "bls12381_add", "secp256r1_double", "bls12381_double", "bn254_fp", "bls12381_fp", "bn254_fp2_addsub",
               "bls12381_fp2_addsub", "bn254_fp2_mul", "bls12381_fp2_mul")
KIND_SHAPES = [(k, n, h) for k in KINDS for n, h in SHAPES] + [(k,) + LARGE for k in LARGE_KINDS]
N_MULTIPLES = 16
GENERATORS = {"Secp256r1": (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296, 0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5),
              "Bn254": (1, 2),
              "Bls12381": (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
                           0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)}


def field_of(kind):
    """(name in riscv_more's tables, modulus, byte limbs, a coefficient or None) of a kind's field."""
    chip = CHIPS[kind]
    name = next(c for c in ("Secp256r1", "Bn254", "Bls12381") if chip.startswith(c))
    if SHAPE[kind].startswith("curve"):
        p, a, nl = M.CURVES[name][:3]
        return name, p, nl, a
    p, nl = M.FP_FIELDS[name][:2]
    return name, p, nl, None


def words_of(kind):
    return MT.FAMILY_SHAPES[kind][3]                                # u64 words per operand


def event_words(kind):
    return 4 + (3 if SHAPE[kind] == "curve_double" else 5) * words_of(kind)


def syscall_codes(kind):
    """The system-call codes a kind's events carry (word 3), in the order the rows cycle through them."""
    name = field_of(kind)[0]
    shape = SHAPE[kind]
    if shape == "curve_add":
        return [0x00010100 | M.CURVE_SYSCALLS[name][0]]
    if shape == "curve_double":
        return [0x00000100 | M.CURVE_SYSCALLS[name][1]]
    lo, hi = {"fp": (0, 3), "fp2_addsub": (3, 5), "fp2_mul": (5, 6)}[shape]
    return [0x00010100 | c for c in M.FP_SYSCALLS[name][lo:hi]]


def edge(p, nl):
    out = [0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 128) - 1, (1 << (8 * (nl - 1))) - 1, (0xAB << (8 * (nl - 2))) + 0xCD]
    assert len(set(out)) == 11 and all(0 <= v < p for v in out)
    return out


def affine_add(p, q, modulus, a):
    """Python's affine arithmetic on y^2 = x^3 + a x + b (the formulas only: the points need not be on the curve)."""
    lam = ((3 * p[0] * p[0] + a) * pow(2 * p[1], modulus - 2, modulus) if p == q else (q[1] - p[1]) * pow(q[0] - p[0], modulus - 2, modulus)) % modulus
    x = (lam * lam - p[0] - q[0]) % modulus
    return x, (lam * (p[0] - x) - p[1]) % modulus


def multiples(name, n):
    p, a = M.CURVES[name][:2]
    g = GENERATORS[name]
    out, cur = [g], g
    for _ in range(n - 1):
        cur = affine_add(cur, g, p, a)
        out.append(cur)
    return out


_OPERANDS = {}


def operands(kind):
    """The operand set of a kind: [(x, y)] with x, y tuples of one or two field elements (a doubling: y is None)."""
    if kind in _OPERANDS:
        return _OPERANDS[kind]
    name, p, nl, _ = field_of(kind)
    shape = SHAPE[kind]
    ed = edge(p, nl)
    rng = random.Random(2024 + FAMILY[kind])
    if shape == "curve_add":
        out = [((px, rng.choice(ed)), (qx, rng.choice(ed))) for px in ed for qx in ed if px != qx]
        out.append(((ed[3], ed[5]), (ed[6], ed[5])))                 # p.y = q.y: slope 0
        mg = multiples(name, 2 * N_MULTIPLES + 1)
        out += [(mg[k], mg[2 * N_MULTIPLES - k]) for k in range(N_MULTIPLES)]        # (k + 1) G + (2 n + 1 - k) G, never equal
        while len(out) < 300:
            x, y = (rng.randrange(p), rng.randrange(p)), (rng.randrange(p), rng.randrange(p))
            if x[0] != y[0]:
                out.append((x, y))
    elif shape == "curve_double":
        out = [((px, py), None) for px in ed for py in ed if py != 0]
        out += [(g, None) for g in multiples(name, N_MULTIPLES)]
        out += [((rng.randrange(p), rng.randrange(1, p)), None) for _ in range(300 - len(out))]
    else:
        pairs = [(a, b) for a in ed for b in ed]
        if shape == "fp":
            out = [((a,), (b,)) for a, b in pairs]
            out += [((rng.randrange(p),), (rng.randrange(p),)) for _ in range(300 - len(out))]
        else:
            out = [((a, pairs[(i + 37) % 121][0]), (b, pairs[(i + 37) % 121][1])) for i, (a, b) in enumerate(pairs)]
            out += [((rng.randrange(p), rng.randrange(p)), (rng.randrange(p), rng.randrange(p))) for _ in range(300 - len(out))]
    _OPERANDS[kind] = out
    return out


def result_of(kind, code, x, y):
    """The field elements a call writes, in Python integers."""
    name, p, _, a = field_of(kind)
    shape = SHAPE[kind]
    if shape == "curve_add":
        return affine_add(x, y, p, a)
    if shape == "curve_double":
        return affine_add(x, x, p, a)
    if shape == "fp2_mul":
        return ((x[0] * y[0] - x[1] * y[1]) % p, (x[0] * y[1] + x[1] * y[0]) % p)
    op = M.FP_SYSCALLS[name].index(code & 0xFF) % 3                 # add, sub, mul
    return tuple(((a_ + b_) % p, (a_ - b_) % p, a_ * b_ % p)[op] for a_, b_ in zip(x, y))


def _timing(n, seed, reads):
    """clk [n], pointers [n, 2], previous timestamps [n, reads] as Python ints, in the pattern of secp_cases._timing."""
    gen = torch.Generator()
    gen.manual_seed(seed)
    clk = (CLK0 + 320 * torch.arange(n, dtype=torch.int64)).tolist()
    slots = torch.randperm(8 * n + 8, generator=gen)
    ptrs = [[0x20_0000 + 256 * int(slots[2 * i]), 0x20_0000 + 256 * int(slots[2 * i + 1])] for i in range(n)]
    t_prev = torch.randint(1, CLK0 - 8, (n, reads), generator=gen, dtype=torch.int64).tolist()      # both sides of the 5 << 24 boundary
    if n:
        t_prev[0][0] = clk[0] - 1                                    # the access just before
        t_prev[0][1] = (5 << 24) - 1                                 # the last tick of the window before clk's
        t_prev[0][2] = 5 << 24                                       # the first tick of clk's window
        t_prev[0][3] = 1
    if n >= 4:
        clk[n - 1] = (6 << 24) + 1                                   # a call on the first cycle of a window
        t_prev[n - 1][0], t_prev[n - 1][1], t_prev[n - 1][2] = 6 << 24, (6 << 24) - 1, 1
        t_prev[n - 1][reads - 1] = 6 << 24                           # (two operands: a read of y, made at clk itself)
        ptrs[1] = [0xFFFF_FFFF_0000, 0xFFFF_FFFF_0100]               # both upper limbs full: top_two_limb_max is zero
        ptrs[2] = [0x0001_0002_FFF8, 0x0003_FFFF_FFC8]               # + 8 i carries into the second limb (and on into the third)
        ptrs[3] = [0x1234_0000_0100, 0x7FFF_0001_0000]
    return clk, ptrs, t_prev


def _element_words(v, nl):
    return [(v >> (64 * i)) & M64 for i in range(nl // 8)]


_EVENTS = {}


def events(kind, n, start=0):
    """n event records of `kind` (int64 [n, event_words(kind)]) from the operand set, cycled, beginning at `start`: clk, arg1, arg2,
    code, (previous timestamp, word) of x and of y, the words written."""
    key = (kind, n, start)
    if key in _EVENTS:
        return _EVENTS[key]
    nl, nw, ops, codes = field_of(kind)[2], words_of(kind), operands(kind), syscall_codes(kind)
    two = SHAPE[kind] != "curve_double"
    clk, ptrs, t_prev = _timing(n, 7 * n + FAMILY[kind], 2 * nw if two else nw)
    rows = []
    for i in range(n):
        x, y = ops[(start + i) % len(ops)]
        code = codes[i % len(codes)]
        xw = [w for v in x for w in _element_words(v, nl)]
        row = [clk[i], ptrs[i][0], ptrs[i][1] if two else 0, code]
        for k in range(nw):
            row += [t_prev[i][k], xw[k]]
        if two:
            yw = [w for v in y for w in _element_words(v, nl)]
            for k in range(nw):
                row += [t_prev[i][nw + k], yw[k]]
        rows.append(row + [w for v in result_of(kind, code, x, y) for w in _element_words(v, nl)])
    width = event_words(kind)
    _EVENTS[key] = np.array(rows, dtype=np.uint64).reshape(n, width).view(np.int64) if n else np.zeros((0, width), dtype=np.int64)
    return _EVENTS[key]


def filler_table(kind, ev, device="cpu"):
    """The chip table family_shard_from fills for these events (int64 [pad32(n), width], canonical), without the rest of the shard:
    the builder runs up to the point where it hands its Tracer to _close_precompile_shard — every line that makes the chip's rows —
    and the tables around it (Byte, Range, Global: seconds per shard) are not made."""
    closing = MT._close_precompile_shard
    MT._close_precompile_shard = lambda tr, *args, **kwargs: tr
    try:
        tr = MT.family_shard_from(kind, ev, device)
    finally:
        MT._close_precompile_shard = closing
    return tr.tables[CHIPS[kind]].main


_HOST = {}


def host_table(kind, n, height, start=0):
    """The host filler's table of events(kind, n, start): int64 [height, width] canonical values, made once. Without an event the
    filler makes no table: every row is then the padding row of a one-event table."""
    key = (kind, n, height, start)
    if key not in _HOST:
        tb = filler_table(kind, events(kind, n, start)) if n else filler_table(kind, events(kind, 1))[1:2].expand(height, -1)
        assert tb.shape == (height, R.chip(CHIPS[kind])[0].main_width) and RT.pad32(max(n, 1)) == height
        _HOST[key] = tb.contiguous()
    return _HOST[key]


def montgomery_col_major(table):
    """int64 [height, width] canonical -> uint32 numpy [width, height] Montgomery words: what the device and the native program write."""
    return np.ascontiguousarray(RT.to_monty_np(table).T)


def group(kind, col):
    lay = R.chip(CHIPS[kind])[0].layout
    at = max(c for c in lay.values() if c <= col)
    return sorted(k for k, c in lay.items() if c == at)[0]


def first_difference(kind, want, got, n):
    """None, or a message naming the first differing word of two [width, height] arrays by column, layout group and row."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if not bad.shape[0]:
        return None
    col, row = (int(v) for v in bad[0])
    return ("%s with %d events: %d words differ; first at column %d (group %s), row %d (%s): got %#x, want %#x"
            % (CHIPS[kind], n, bad.shape[0], col, group(kind, col), row, "event" if row < n else "padding", int(got[col, row]), int(want[col, row])))


def run_rows(form, kind, ev, height, tmp_path):
    """tests/native/field_chip_rows FORM FAMILY on an event file: the table as uint32 numpy [width, height]."""
    stem = os.path.join(str(tmp_path), "%s_%s_%d" % (form, kind, ev.shape[0]))
    with open(stem + ".in", "wb") as f:
        f.write(np.array([ev.shape[0], height], dtype=np.uint32).tobytes() + np.ascontiguousarray(ev).tobytes())
    subprocess.run([EXE, form, str(FAMILY[kind]), stem + ".in", stem + ".out"], check=True, capture_output=True, timeout=300)
    return np.fromfile(stem + ".out", dtype=np.uint32).reshape(R.chip(CHIPS[kind])[0].main_width, height)


# ------------------------------------------------------------------------------------------------------ hand-assembled programs
DATA = 0x78100000


def _call(code, a0, a1):
    import rv_asm as A
    return [A.enc("addi", 10, 28, a0), A.enc("addi", 11, 28, a1) if a1 is not None else A.enc("addi", 11, 0, 0)] + A.li(5, code) + [A.enc("ecall")]


def _bytes(v, n):
    return b"".join(struct.pack("<Q", (v >> (64 * i)) & M64) for i in range(n))


def _curve_calls(name, calls):
    """(instructions, data) of `calls` rounds of p <- 2 p, q <- q + p, q <- 2 q over fresh copies of the curve's generator, relative
    to x28, which each round moves past its data."""
    import rv_asm as A
    n = M.CURVES[name][2] // 8
    g = GENERATORS[name]
    add_code, double_code = 0x00010100 | M.CURVE_SYSCALLS[name][0], 0x00000100 | M.CURVE_SYSCALLS[name][1]
    pt = _bytes(g[0], n) + _bytes(g[1], n)
    size = 2 * 8 * n
    prog, data = [], b""
    for _ in range(calls):
        prog += _call(double_code, 0, None) + _call(add_code, size, 0) + _call(double_code, size, None) + [A.enc("addi", 28, 28, 2 * size)]
        data += pt + pt
    return prog, data


def _tower_calls(name, calls):
    """(instructions, data) of `calls` rounds over fresh operands: per round 4 Fp operations (add, mul, sub, mul: three opcodes in one
    shard), 1 Fp2 product, 1 Fp2 addition and 1 Fp2 subtraction."""
    import rv_asm as A
    p, nl = M.FP_FIELDS[name][:2]
    n = nl // 8
    codes = [0x00010100 | c for c in M.FP_SYSCALLS[name]]
    slot = 8 * n
    at = lambda k: k * slot
    prog, data = [], b""
    for c in range(calls):
        a, b = (3 ** 200 + 12345 + c) % p, p - 7 - c
        c0, c1, d0, d1 = 5 ** 150 % p, p - 1 - c, 7 ** 130 % p, (11 ** 100 + c) % p
        prog += _call(codes[0], at(0), at(1)) + _call(codes[2], at(2), at(2)) + _call(codes[1], at(3), at(4)) + _call(codes[2], at(4), at(0))
        prog += _call(codes[5], at(5), at(7)) + _call(codes[3], at(9), at(7)) + _call(codes[4], at(11), at(7)) + [A.enc("addi", 28, 28, 13 * slot)]
        data += b"".join(_bytes(v, n) for v in [a, b, a, a, b, c0, c1, d0, d1, c0, c1, c0, c1])
    return prog, data


def _elf(*parts):
    import rv_asm as A
    prog, data = A.li(28, DATA), b""
    for instrs, d in parts:
        prog, data = prog + instrs, data + d
    return A.elf(prog + A.halt(0), data=data + bytes(32))


def curve_program(name, calls=1):
    """The ELF of tests/test_riscv_precompiles.py's curve program, `calls` times over: one round is 1 addition and 2 doublings."""
    return _elf(_curve_calls(name, calls))


def tower_program(name, calls=1):
    """The ELF of tests/test_riscv_precompiles.py's tower program, `calls` times over."""
    return _elf(_tower_calls(name, calls))


def mixed_program(curve, field, calls=1):
    """One program that calls a curve's and a tower field's precompiles: the two above, one after the other."""
    return _elf(_curve_calls(curve, calls), _tower_calls(field, calls))
