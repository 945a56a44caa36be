"""What the trace-generation tests of the EdAddAssign, EdDecompress and Uint256Ops chips share (tests/test_tracegen_ed_u256_host.py on
the CPU, tests/test_gpu_tracegen_ed_u256.py on the GPU): the operand sets, the family event records made from them, the host filler's
chip tables and MemoryLocal records (riscv_more_trace.family_shard_from: the reference of every comparison, made once per shape), the
file interface of tests/native/ed_u256_rows and the hand-assembled programs. It follows tests/field_chip_cases.py.

Operands. EDGE = field_chip_cases.edge(p, 32) for p = 2^255 - 19: 0, 1, 2, 3, p - 1, p - 2, (p - 1) / 2, (p + 1) / 2, 2^128 - 1,
2^248 - 1, 0xAB 2^240 + 0xCD.
* ed_add: every ordered pair of edge elements as (x1, x2) (121) with y1, y2 drawn from the list by a seeded generator; the identity
  (0, 1) on either side; P + P and P + (-P) for multiples P of the base point; 16 pairs of multiples of B (checked against the
  Python ed_add of tests/test_riscv_precompiles.py); seeded random elements up to 300. A quadruple whose denominator
  1 +- d x1 x2 y1 y2 vanishes is drawn again (none of the edge quadruples does: asserted).
* ed_decompress: the six edge elements y for which u / v = (y^2 - 1) / (d y^2 + 1) is a square — 0, 1, 3, p - 1, 2^128 - 1,
  0xAB 2^240 + 0xCD (asserted; y = 1 and y = p - 1 give the root 0) —, the y of 16 multiples of B, then seeded random y filtered to
  squares up to 300. The sign bit alternates by row. All four combinations occur and are asserted: the root needed the
  multiplication by sqrt(-1) or did not, and the candidate root was odd or even.
* uint256_ops: a, b, c from {0, 1, 2, 3, 2^256 - 1, 2^256 - 2, 2^255 - 1, 2^255, 2^128 - 1, 2^248 - 1, 0xAB 2^240 + 0xCD}: every
  ordered pair (a, b) with c cycling through the list (121), then the product of the two largest (an odd row: a multiplication), the
  sum of three times 2^256 - 1 (an even row: an addition with carry 2), calls with d aliased onto a, then random cases up to 300. The
  opcode is i % 2 by row, so every wave mixes both system calls.
The words written are computed here in Python integers; the host builder asserts them. Clocks, previous timestamps and pointers
follow secp_cases._timing: a call on the first tick of a 2^24 window, previous timestamps (the registers' among them) on both sides
of the boundary and at clk - 1, pointers with full upper limbs, a pointer where + 8 i carries."""
import os
import random
import subprocess

import numpy as np

import field_chip_cases as F
import secp_cases

from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_more as M
from sp1_amd.machines import riscv_more_trace as MT
from sp1_amd.machines import riscv_trace as RT
from test_riscv_precompiles import DATA, ED_B, call, ed_add, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "ed_u256_rows")
KINDS = ("ed_add", "ed_decompress", "uint256_ops")                 # SP1HIP_RV64_FAMILY_* 12, 13, 14
FAMILY = {k: X.FAMILIES[k][0] for k in KINDS}
CHIPS = {k: X.FAMILIES[k][1] for k in KINDS}
EVENT_WORDS = {"ed_add": 44, "ed_decompress": 24, "uint256_ops": 58}
RECORDS_PER_CALL = {"ed_add": 16, "ed_decompress": 8, "uint256_ops": 23}
CODES = {"ed_add": (0x00010107,), "ed_decompress": (0x00000108,), "uint256_ops": (0x00010130, 0x00010131)}
M64 = (1 << 64) - 1
TOP = (1 << 256) - 1
P, D = M.ED25519_P, M.ED25519_D
SQRT_M1 = pow(2, (P - 1) // 4, P)
EDGE = F.edge(P, 32)
SHAPES = [(0, 32), (1, 32), (32, 32), (33, 64), (300, 320)]         # (events, height); 300 events cross a 256-lane workgroup
KIND_SHAPES = [(k, n, h) for k in KINDS for n, h in SHAPES]
LARGE = (300, 320)
N_MULTIPLES = 16
U256 = [0, 1, 2, 3, TOP, TOP - 1, (1 << 255) - 1, 1 << 255, (1 << 128) - 1, (1 << 248) - 1, (0xAB << 240) + 0xCD]


def multiples_of_b(n):
    out, cur = [ED_B], ED_B
    for _ in range(n - 1):
        cur = ed_add(cur, ED_B)
        out.append(cur)
    return out


def denominators_vanish(x1, y1, x2, y2):
    f = D * x1 * x2 * y1 * y2 % P
    return (1 + f) % P == 0 or (1 - f) % P == 0


def u_div_v(y):
    return (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P


def root_path(a):
    """(the root needed the multiplication by sqrt(-1), the candidate root was odd) of a square a; None for a non-square."""
    beta = pow(a, (P + 3) // 8, P)
    needed = beta * beta % P == (P - a) % P
    if needed:
        beta = beta * SQRT_M1 % P
    return (needed, bool(beta & 1)) if beta * beta % P == a else None


_OPERANDS = {}


def operands(kind):
    """ed_add: [(x1, y1, x2, y2)]; ed_decompress: [y]; uint256_ops: [(a, b, c, d aliased onto a)] — 300 each."""
    if kind in _OPERANDS:
        return _OPERANDS[kind]
    rng = random.Random(2024 + FAMILY[kind])
    if kind == "ed_add":
        out = [(x1, rng.choice(EDGE), x2, rng.choice(EDGE)) for x1 in EDGE for x2 in EDGE]
        assert not any(denominators_vanish(a, b, c, d) for a in EDGE for b in EDGE for c in EDGE for d in EDGE)
        assert not any(denominators_vanish(*q) for q in out)
        mb = multiples_of_b(2 * N_MULTIPLES + 1)
        out += [(0, 1) + mb[3], mb[4] + (0, 1), (0, 1, 0, 1)]                                  # the identity on either side
        out += [mb[k] + mb[k] for k in (0, 5)] + [mb[k] + ((P - mb[k][0]) % P, mb[k][1]) for k in (0, 6)]   # P + P, P + (-P)
        out += [mb[k] + mb[2 * N_MULTIPLES - k] for k in range(N_MULTIPLES)]
        for q in out[-N_MULTIPLES:]:                                                           # on the curve: the law is the group's
            assert ed_add(q[:2], q[2:]) == ed_add(q[2:], q[:2])
        assert ed_add(mb[0], mb[1]) == mb[2] and ed_add(mb[0], ((P - mb[0][0]) % P, mb[0][1])) == (0, 1)
        while len(out) < 300:
            q = tuple(rng.randrange(P) for _ in range(4))
            if not denominators_vanish(*q):
                out.append(q)
    elif kind == "ed_decompress":
        squares = [y for y in EDGE if root_path(u_div_v(y)) is not None]
        assert squares == [0, 1, 3, P - 1, (1 << 128) - 1, (0xAB << 240) + 0xCD]
        assert u_div_v(1) == 0 and u_div_v(P - 1) == 0
        out = squares + [pt[1] for pt in multiples_of_b(N_MULTIPLES)]
        while len(out) < 300:
            y = rng.randrange(P)
            if root_path(u_div_v(y)) is not None:
                out.append(y)
        assert {root_path(u_div_v(y)) for y in out} == {(False, False), (False, True), (True, False), (True, True)}
    else:
        out = [(a, b, U256[i % 11], False) for i, (a, b) in enumerate((a, b) for a in U256 for b in U256)]
        assert len(out) == 121
        out += [(TOP, TOP - 1, TOP, False), (TOP, TOP, TOP, False), (TOP, TOP, TOP, True), (3 ** 150, 5 ** 100, 7, True), (1, 2, 3, True), (TOP, TOP - 1, TOP, True)]
        while len(out) < 300:
            out.append((rng.randrange(1 << 256), rng.randrange(1 << 256), rng.randrange(1 << 256), rng.random() < 0.1))
    assert len(out) == 300
    _OPERANDS[kind] = out
    return out


def _w4(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


_EVENTS = {}


def events(kind, n):
    """n event records of `kind` (int64 [n, EVENT_WORDS[kind]]) from the first n of the operand set (n <= 300)."""
    key = (kind, n)
    if key in _EVENTS:
        return _EVENTS[key]
    assert n <= 300
    ops = operands(kind)
    reads = {"ed_add": 16, "ed_decompress": 8, "uint256_ops": 23}[kind]
    clk, ptrs, t_prev = secp_cases._timing(n, 7 * n + FAMILY[kind], reads)
    rng = random.Random(99 + FAMILY[kind])
    rows = []
    for i in range(n):
        code = CODES[kind][i % len(CODES[kind])]
        if kind == "ed_add":
            x1, y1, x2, y2 = ops[i]
            xw, yw = _w4(x1) + _w4(y1), _w4(x2) + _w4(y2)
            row = [clk[i], ptrs[i][0], ptrs[i][1], code]
            for k in range(8):
                row += [t_prev[i][k], xw[k]]
            for k in range(8):
                row += [t_prev[i][8 + k], yw[k]]
            x3, y3 = ed_add((x1, y1), (x2, y2))
            row += _w4(x3) + _w4(y3)
        elif kind == "ed_decompress":
            y, sign = ops[i], i % 2
            root = MT.ed25519_even_sqrt(u_div_v(y))
            before = _w4(rng.randrange(1 << 256))
            row = [clk[i], ptrs[i][0], sign, code]
            for k in range(4):
                row += [t_prev[i][k], before[k]]
            for k in range(4):
                row += [t_prev[i][4 + k], _w4(y)[k]]
            row += _w4((P - root) % P if sign else root)
        else:
            a, b, c, alias = ops[i]
            a_ptr, b_ptr = ptrs[i]
            c_ptr, d_ptr, e_ptr = a_ptr + 64, a_ptr if alias else a_ptr + 128, b_ptr + 64
            full = (a * b if code & 0xFF == 0x31 else a + b) + c
            row = [clk[i], a_ptr, b_ptr, code, c_ptr, d_ptr, e_ptr] + t_prev[i][:3]
            blocks = [_w4(a), _w4(b), _w4(c), _w4(a) if alias else _w4(rng.randrange(1 << 256)), _w4(rng.randrange(1 << 256))]
            for j in range(5):
                for k in range(4):
                    row += [clk[i] if alias and j == 3 else t_prev[i][3 + 4 * j + k], blocks[j][k]]     # d over a: a was read at clk
            row += _w4(full & TOP) + _w4(full >> 256)
        assert len(row) == EVENT_WORDS[kind]
        rows.append(row)
    width = EVENT_WORDS[kind]
    _EVENTS[key] = np.array(rows, dtype=np.uint64).reshape(n, width).view(np.int64) if n else np.zeros((0, width), dtype=np.int64)
    return _EVENTS[key]


def out_of_domain_events():
    """{kind: one event outside the kernels' preconditions}: ed_decompress of y = 2 (u / v is not a square) and an ed_add whose
    1 + d x1 x2 y1 y2 is 0. Python's filler refuses them; the native program's host and device forms must still agree."""
    assert root_path(u_div_v(2)) is None
    y2 = (P - pow(D, P - 2, P)) % P
    assert (1 + D * y2) % P == 0
    clk, ptrs, t_prev = secp_cases._timing(1, 5, 16)
    add = [clk[0], ptrs[0][0], ptrs[0][1], 0x00010107]
    for k, w in enumerate(_w4(1) + _w4(1) + _w4(1) + _w4(y2)):
        add += [t_prev[0][k], w]
    dec = [clk[0], ptrs[0][0], 0, 0x00000108]
    for k, w in enumerate(_w4(0) + _w4(2)):
        dec += [t_prev[0][k], w]
    as_events = lambda row: np.array([row], dtype=np.uint64).view(np.int64)
    return {"ed_add": as_events(add + [0] * 8), "ed_decompress": as_events(dec + [0] * 4)}


def filler(kind, ev, device="cpu"):
    """(the chip table, the MemoryLocal records [m, 5] int64) family_shard_from makes of these events, without the rest of the
    shard: the builder runs up to the point where it hands its Tracer and the touched words to _close_precompile_shard."""
    closing = MT._close_precompile_shard
    seen = {}

    def capture(tr, syscall_id, clk, ptr_limbs, word_addr, t_initial, t_final, v_initial, v_final, **kwargs):
        seen["records"] = np.stack([np.asarray(v.cpu()) for v in (word_addr, t_initial, v_initial, t_final, v_final)], axis=1).astype(np.int64)
        return tr
    MT._close_precompile_shard = capture
    try:
        tr = MT.family_shard_from(kind, ev, device)
    finally:
        MT._close_precompile_shard = closing
    return tr.tables[CHIPS[kind]].main, seen["records"]


_HOST = {}


def host_table(kind, n, height):
    """The host filler's table of events(kind, n): int64 [height, width] canonical values, made once. Without an event the filler
    makes no table: every row is then the padding row of a one-event table."""
    key = (kind, n, height)
    if key not in _HOST:
        tb = filler(kind, events(kind, n))[0] if n else filler(kind, events(kind, 1))[0][1:2].expand(height, -1)
        assert tb.shape == (height, R.chip(CHIPS[kind])[0].main_width) and RT.pad32(max(n, 1)) == height
        _HOST[key] = tb.contiguous()
    return _HOST[key]


def host_records(kind, n):
    return filler(kind, events(kind, n))[1]


montgomery_col_major = F.montgomery_col_major


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


def _run(form, what, ev, height, tmp_path):
    stem = os.path.join(str(tmp_path), "%s_%s_%d" % (form, what, ev.shape[0]))
    with open(stem + ".in", "wb") as f:
        f.write(np.array([ev.shape[0], height], dtype=np.uint32).tobytes() + np.ascontiguousarray(ev).tobytes())
    subprocess.run([EXE, form, what, stem + ".in", stem + ".out"], check=True, capture_output=True, timeout=300)
    return stem + ".out"


def run_rows(form, kind, ev, height, tmp_path):
    """tests/native/ed_u256_rows FORM KIND on an event file: the table as uint32 numpy [width, height]."""
    return np.fromfile(_run(form, kind, ev, height, tmp_path), dtype=np.uint32).reshape(R.chip(CHIPS[kind])[0].main_width, height)


def run_records(form, kind, ev, tmp_path):
    """tests/native/ed_u256_rows FORM records_KIND: the MemoryLocal records as int64 numpy [n * records per call, 5]."""
    return np.fromfile(_run(form, "records_" + kind, ev, RT.pad32(max(len(ev), 1)), tmp_path), dtype=np.int64).reshape(-1, 5)


# ------------------------------------------------------------------------------------------------------ hand-assembled programs
def _decompress(offset, sign):
    import rv_asm as A
    return [A.enc("addi", 10, 28, offset), A.enc("addi", 11, 0, sign)] + A.li(5, 0x00000108) + [A.enc("ecall")]


def ed_results():
    """2B, 3B, and the two x coordinates ED_DECOMPRESS writes in one round of ed_program."""
    b2 = ed_add(ED_B, ED_B)
    b3 = ed_add(b2, ED_B)
    return b2, b3, b3[0], P - b2[0]


ED_ROUND = 352


def ed_program(calls=1):
    """The ELF of tests/test_riscv_precompiles.py's ed25519 program, `calls` times over: one round is 2 ED_ADD (2B, 3B) and 2
    ED_DECOMPRESS (x(3B) with its own sign bit, x(-2B) from y(2B) with the other sign bit)."""
    import rv_asm as A
    b2, b3, _, _ = ed_results()
    pt = words(ED_B[0], 4) + words(ED_B[1], 4)
    prog, data = A.li(28, DATA), b""
    for _ in range(calls):
        prog += call(0x00010107, 0, 64) + call(0x00010107, 128, 0) + _decompress(192, b3[0] & 1) + _decompress(256, 1 - (b2[0] & 1))
        prog += [A.enc("addi", 28, 28, ED_ROUND)]
        data += pt + pt + pt + bytes(32) + words(b3[1], 4) + bytes(32) + words(b2[1], 4) + bytes(32)
        assert len(data) % ED_ROUND == 0
    return A.elf(prog + A.halt(0), data=data + bytes(32))


CARRY_CASES = [(0x00010130, TOP, TOP, TOP), (0x00010131, TOP, TOP - 5, TOP), (0x00010131, 3 ** 150, 5 ** 100, 7), (0x00010130, 1, 2, 3)]
CARRY_ROUND = 160 * len(CARRY_CASES)


def carry_program(calls=1):
    """The ELF of tests/test_riscv_precompiles.py's carry program, `calls` times over: one round is 4 calls (add, mul, mul, add; the
    second writes d over its own operand a)."""
    import rv_asm as A
    prog, data = A.li(28, DATA), b""
    for _ in range(calls):
        for i, (code, a, b, c) in enumerate(CARRY_CASES):
            base = 160 * i
            data += words(a, 4) + words(b, 4) + words(c, 4) + bytes(64)
            d_off = base if i == 1 else base + 96
            prog += [A.enc("addi", 12, 28, base + 64), A.enc("addi", 13, 28, d_off), A.enc("addi", 14, 28, base + 128)] + call(code, base, base + 32)
        prog += [A.enc("addi", 28, 28, CARRY_ROUND)]
    return A.elf(prog + A.halt(0), data=data + bytes(32))


PROGRAMS = {"ed_add": ed_program, "ed_decompress": ed_program, "uint256_ops": carry_program}
CALLS_PER_ROUND = {"ed_add": 2, "ed_decompress": 2, "uint256_ops": 4}
