"""What the secp256k1 trace-generation tests share (tests/test_tracegen_secp_host.py on the CPU, tests/test_gpu_tracegen_secp.py
on the GPU): the operand set, the event records made from it, the host filler's tables (the reference of every comparison, made
once per shape) and the file interface of tests/native/secp_rows.

Operands. Eleven edge field elements — 0, 1, 2, 255, 256, 2^128 - 1, 2^255, 2^32 + 976, 2^32 + 977 (= 2^256 mod p), p - 2, p - 1.
* additions: every ordered pair (p.x, q.x) of distinct edge values (11 x 10 = 110) with p.y, q.y drawn from the same list by a
  seeded generator, and one case with p.y = q.y (slope 0): 111;
* doublings: every (p.x, p.y) pair of edge values with p.y != 0: 11 x 10 = 110;
* then 40 multiples of G, then seeded random reduced elements.
(The issue this answers speaks of 131 + 132 edge cases; its own rule, ordered pairs of the 11 listed elements, gives the 111 + 110
here, and no element count gives both of its figures. Every case the rule defines is in the set.)
The points need not lie on the curve: the filler does not care. Clocks, previous timestamps and pointers follow
tests/test_gpu_tracegen_keccak.py::_calls: a call on the first tick of a 2^24 window, previous timestamps on both sides of the
boundary and at clk - 1, pointers with full upper limbs, a pointer where + 8 i carries into the second limb."""
import os
import random
import subprocess

import numpy as np
import torch

from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_more_trace as MT
from sp1_amd.machines import riscv_trace as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "secp_rows")
P = MT.M.SECP256K1_P
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
EDGE = [0, 1, 2, 255, 256, (1 << 128) - 1, 1 << 255, (1 << 32) + 976, (1 << 32) + 977, P - 2, P - 1]
CHIPS = MT.SECP256K1_CHIPS                                          # kind -> chip name
WORDS = {"add": 43, "double": 26}
M64 = (1 << 64) - 1
CLK0 = (5 << 24) + 1001                                             # clk_high = 5
N_MULTIPLES, N_RANDOM = 40, 149                                     # 111 + 40 + 149 = 300 additions, 110 + 40 + 150 doublings
SHAPES = [(0, 32), (1, 32), (32, 32), (33, 64), (300, 320)]         # (events, height); 300 events cross a 256-lane workgroup


def affine_add(p, q):
    """Python's affine arithmetic on y^2 = x^3 + 7 (the formulas only: the points need not be on the curve)."""
    lam = (3 * p[0] * p[0] * pow(2 * p[1], P - 2, P) if p == q else (q[1] - p[1]) * pow(q[0] - p[0], P - 2, P)) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def multiples_of_g(n):
    out, cur = [G], G
    for _ in range(n - 1):
        cur = affine_add(cur, G)
        out.append(cur)
    return out


def add_operands():
    """[(p, q)]: the 111 edge cases, N_MULTIPLES pairs (k G, (k + 1) G ... ) of multiples of G, N_RANDOM random pairs."""
    rng = random.Random(2024)
    out = [((px, rng.choice(EDGE)), (qx, rng.choice(EDGE))) for px in EDGE for qx in EDGE if px != qx]
    out.append(((EDGE[3], EDGE[9]), (EDGE[6], EDGE[9])))            # p.y = q.y: slope 0
    assert len(out) == 111
    mg = multiples_of_g(2 * N_MULTIPLES + 1)
    out += [(mg[k], mg[2 * N_MULTIPLES - k]) for k in range(N_MULTIPLES)]   # k G + (81 - k) G, never equal
    for _ in range(N_RANDOM):
        p, q = (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))
        assert p[0] != q[0]
        out.append((p, q))
    return out


def double_operands():
    rng = random.Random(2025)
    out = [(px, py) for px in EDGE for py in EDGE if py != 0]
    assert len(out) == 110
    out += multiples_of_g(N_MULTIPLES)
    out += [(rng.randrange(P), rng.randrange(1, P)) for _ in range(300 - len(out))]
    return out


def _words(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def _timing(n, seed, reads):
    """clk [n], pointers [n, 2], previous timestamps [n, reads] as Python ints, in the pattern of the Keccak test's _calls."""
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
        t_prev[n - 1][reads - 1] = 6 << 24                           # (for an addition: a read of q, made at clk itself)
        ptrs[1] = [0xFFFF_FFFF_0000, 0xFFFF_FFFF_0100]               # both upper limbs full: top_two_limb_max is zero
        ptrs[2] = [0x0001_0002_FFF8, 0x0003_FFFF_FFC8]               # + 8 i carries into the second limb (and on into the third)
        ptrs[3] = [0x1234_0000_0100, 0x7FFF_0001_0000]
    return clk, ptrs, t_prev


def _s64(rows, width):
    a = np.array(rows, dtype=np.uint64).reshape(len(rows), width)
    return a.view(np.int64)


_EVENTS = {}


def events(kind, n, start=0):
    """n event records of `kind` ("add": int64 [n, 43], "double": [n, 26]) from the operand set, cycled, beginning at `start`."""
    key = (kind, n, start)
    if key in _EVENTS:
        return _EVENTS[key]
    ops = add_operands() if kind == "add" else double_operands()
    clk, ptrs, t_prev = _timing(n, 7 * n + (kind == "add"), 16 if kind == "add" else 8)
    rows = []
    for i in range(n):
        if kind == "add":
            p, q = ops[(start + i) % len(ops)]
            pw, qw = _words(p[0]) + _words(p[1]), _words(q[0]) + _words(q[1])
            x3, y3 = affine_add(p, q)
            row = [clk[i], ptrs[i][0], ptrs[i][1]]
            for k in range(8):
                row += [t_prev[i][k], pw[k]]
            for k in range(8):
                row += [t_prev[i][8 + k], qw[k]]
        else:
            p = ops[(start + i) % len(ops)]
            pw = _words(p[0]) + _words(p[1])
            x3, y3 = affine_add(p, p)
            row = [clk[i], ptrs[i][0]]
            for k in range(8):
                row += [t_prev[i][k], pw[k]]
        rows.append(row + _words(x3) + _words(y3))
    _EVENTS[key] = _s64(rows, WORDS[kind]) if n else np.zeros((0, WORDS[kind]), dtype=np.int64)
    return _EVENTS[key]


_HOST = {}


def host_table(kind, n, height, start=0):
    """The host filler's table of events(kind, n, start): int64 [height, width] canonical values, made once. Without an event the
    filler makes no table: every row is then the padding row of a one-event table."""
    key = (kind, n, height, start)
    if key not in _HOST:
        build = MT.secp256k1_add_table if kind == "add" else MT.secp256k1_double_table
        if n:
            tb = build(events(kind, n, start), torch.device("cpu"))[0].main
        else:
            tb = build(events(kind, 1), torch.device("cpu"))[0].main[1:2].expand(height, -1)
        assert tb.shape == (height, R.chip(CHIPS[kind])[0].main_width) and RT.pad32(max(n, 1)) == height
        _HOST[key] = tb.contiguous()
    return _HOST[key]


def montgomery_col_major(table):
    """int64 [height, width] canonical -> uint32 numpy [width, height] Montgomery words: what the device and the native program write."""
    return np.ascontiguousarray(RT.to_monty_np(table).T)


def group(kind, col):
    """The layout group a column belongs to (for failure messages)."""
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
    """tests/native/secp_rows FORM add|double on an event file: the table as uint32 numpy [width, height]."""
    src, dst = os.path.join(str(tmp_path), "%s_%s_%d.in" % (form, kind, ev.shape[0])), os.path.join(str(tmp_path), "%s_%s_%d.out" % (form, kind, ev.shape[0]))
    with open(src, "wb") as f:
        f.write(np.array([ev.shape[0], height], dtype=np.uint32).tobytes() + np.ascontiguousarray(ev).tobytes())
    subprocess.run([EXE, form, kind, src, dst], check=True, capture_output=True, timeout=120)
    width = R.chip(CHIPS[kind])[0].main_width
    return np.fromfile(dst, dtype=np.uint32).reshape(width, height)


def result_words(kind, table_cm, rows):
    """x3 and y3 of `rows` from a [width, height] Montgomery table: [(x3, y3)] read from x3_ins.result / y3_ins.result byte limbs."""
    lay = R.chip(CHIPS[kind])[0].layout
    inv = pow(1 << 32, -1, RT.P)
    out = []
    for r in rows:
        vals = []
        for name in ("x3_ins.result", "y3_ins.result"):
            by = [int(table_cm[lay[name] + i, r]) * inv % RT.P for i in range(32)]
            assert all(b < 256 for b in by)
            vals.append(sum(b << (8 * i) for i, b in enumerate(by)))
        out.append(tuple(vals))
    return out
