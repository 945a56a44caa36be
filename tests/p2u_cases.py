"""The cases of the Poseidon2 / Uint256MulMod trace-generation tests (test_tracegen_p2u_host.py on the CPU, test_gpu_tracegen_p2u.py
on the device): POSEIDON2 and UINT256_MUL event records written in Python integers — independent of the C++ —, the host builders'
tables of them (riscv_more_trace.poseidon2_shard_from / uint256_shard_from, made once and shared), the two hand-assembled programs
of tests/test_riscv_exec.py restated, and the runners of tests/native/p2u_rows.

POSEIDON2 events. The sixteen halves of the words read are drawn from HALVES = 0, 1, 0x7EFFFFFF, 0x7F000000 (= p - 1), 0x0000FFFF,
0x00010000 and a random value below p, rotated by event and position so that every value — and so both values of every input
range-checker bit — occurs at every position within seven consecutive events. The words written are the library's host permutation
of the words read (sp1hip_poseidon2_permute_host), so the row satisfies the chip — except on every fourth event (e % 4 == 3), whose
words written are drawn from HALVES in the same rotation: a permutation's output is p - 1 with probability 2^-31, and the
hash_result range-checker bits need both values at every position too. The filler does not care (it recomputes the permutation
from the words read), and neither do the row functions. Event 1's pointer has both upper limbs 0xFFFF (top_two_limb_max is the
zero case), event 2's low limb carries under + 8 i. Clocks stand just above, on, and just below a multiple of 2^24 and in the middle
of a window, by e % 4; the previous timestamp of word k is, by k % 3, the tick before the access, in the access's 2^24 window (where
the window has room), or in an earlier window.

UINT256_MUL events. (x, y, m) over every ordered triple of the eleven values of EDGE, then N_RANDOM random 256-bit triples whose x
and y are reduced below m' where the quotient would not fit. A triple is in the chip's domain when x y // m' < 2^256 (m' = m, or
2^256 for m = 0): only those are kept (TRIPLES), and the module asserts on import that at least half of all triples survive and that
the zero modulus, an even modulus, m = 1, result = 0, carry = 0 and a FieldLt hit at byte 31 and at byte 0 occur among them.
OUTSIDE are two triples beyond the domain, for the division alone.

SHAPES are (events, height) pairs on the wave and workgroup edges, with padding present and absent; the shapes walk through the
operand list one after another (START), so together they reach 974 of its entries."""
import ctypes
import os
import random
import struct
import subprocess

import numpy as np
import torch

from sp1_amd import _lib
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_more as M
from sp1_amd.machines import riscv_more_trace as MT
from sp1_amd.machines import riscv_trace as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "p2u_rows")
KINDS = ("poseidon2", "uint256")
CHIPS = {"poseidon2": "Poseidon2", "uint256": "Uint256MulMod"}
KIND_OF = {c: k for k, c in CHIPS.items()}
WORDS = {"poseidon2": 26, "uint256": 31}
SYSCALL = {"poseidon2": (M.SYS_POSEIDON2, -1), "uint256": (M.SYS_UINT256_MUL, 2)}               # (id, arg2 word)
# (ptr_word, count, pairs_word, final_word | None, final_clk_delta): what the two host builders hand _close_precompile_shard, restated
SEGMENTS = {"poseidon2": ((1, 8, 2, 18, 0),), "uint256": ((1, 4, 3, 27, 1), (2, 8, 11, None, 0))}
SHAPES = [(0, 32), (1, 32), (32, 32), (63, 64), (65, 96), (256, 256), (257, 288), (300, 320)]
START = {n: sum(m for m, _ in SHAPES[:i]) for i, (n, _) in enumerate(SHAPES)}                   # where a shape begins in the operand list
KIND_SHAPES = [(k, n, h) for k in KINDS for n, h in SHAPES]
SHARD_CALLS = (1, 6)
P = RT.P
M64, WINDOW, B256 = (1 << 64) - 1, 1 << 24, 1 << 256
HALVES = [0, 1, 0x7EFFFFFF, 0x7F000000, 0x0000FFFF, 0x00010000, None]                           # None: random below p
assert P == 0x7F000001 and (P - 1) >> 16 == 0x7F00

TOP_ZERO = 0x00A1B2C3D4E5F60718293A4B5C6D7E8F9FAEBDCCDBEAF90817263544536271F0                   # the top byte is zero
BYTE0 = B256 - 189 - 0x40                                                                       # differs from 2^256 - 189 only in byte 0
EDGE = [0, 1, 2, 1 << 128, 1 << 200, 1 << 255, B256 - 1, B256 - 189, TOP_ZERO, BYTE0, (1 << 255) + 12345]
N_RANDOM = 200
OUTSIDE = [(B256 - 1, B256 - 1, 1), (1 << 255, 1 << 200, 2)]


def modulus_of(m):
    return m if m else B256


def in_domain(x, y, m):
    return x * y // modulus_of(m) < B256


def _all_triples():
    rng = random.Random(2026)
    out = [(x, y, m) for x in EDGE for y in EDGE for m in EDGE]
    for i in range(N_RANDOM):
        x, y, m = rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256)
        if i % 5 == 0:
            m &= ~1                                                 # an even random modulus
        if i % 7 == 0:
            m >>= 8 * (1 + i % 24)                                  # a short one
        if m and not in_domain(x, y, m):                            # reduced into the domain
            x, y = x % m, y % m
        out.append((x, y, m))
    return out


ALL_TRIPLES = _all_triples()
TRIPLES = [t for t in ALL_TRIPLES if in_domain(*t)]


def _lt_byte(result, m):
    """The byte at which FieldLtCols flags result < m: the most significant one that differs."""
    return max(i for i in range(32) if (result >> (8 * i)) & 0xFF != (m >> (8 * i)) & 0xFF)


def _check_triples():
    assert 2 * len(TRIPLES) >= len(ALL_TRIPLES), (len(TRIPLES), len(ALL_TRIPLES))
    assert all(in_domain(*t) for t in TRIPLES) and not any(in_domain(*t) for t in OUTSIDE)
    res = [(x * y % modulus_of(m), x * y // modulus_of(m), m) for x, y, m in TRIPLES]
    assert any(m == 0 for _, _, m in res) and any(m and m % 2 == 0 for _, _, m in res) and any(m == 1 for _, _, m in res)
    assert any(r == 0 for r, _, _ in res) and any(c == 0 for _, c, _ in res) and any(c >= 1 << 255 for _, c, _ in res)
    hits = {_lt_byte(r, m) for r, _, m in res if m}
    assert {0, 31} <= hits, sorted(hits)


_check_triples()


# ------------------------------------------------------------------------------------------------------------------ the events
def permute(states):
    """The library's host Poseidon2 permutation of [n, 16] canonical words (uint64 numpy) -> the same shape."""
    m = np.ascontiguousarray((states.astype(np.uint64) << np.uint64(32)) % np.uint64(P), dtype=np.uint32)
    if len(m):
        _lib.check(_lib.load().sp1hip_poseidon2_permute_host(m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(m), 1))
    return (m.astype(np.uint64) * np.uint64(pow(1 << 32, -1, P))) % np.uint64(P)


def _previous(rng, k, t):
    """A previous timestamp for an access at time t, three ways by k mod 3: t - 1; in t's 2^24 window (where it has room); earlier."""
    start = t & ~(WINDOW - 1)
    if k % 3 == 0:
        return t - 1
    if k % 3 == 1 and t - start >= 2:
        return rng.randrange(start, t - 1)
    return ((t >> 24) - 1 - k % 2) * WINDOW + rng.randrange(WINDOW)


def _clk(e):
    """By e mod 4: just above a multiple of 2^24, on it, just below it, in the middle of a window."""
    return [(6 << 24) + 1, 7 << 24, (8 << 24) - 1, (9 << 24) + 1001 + 8 * e][e % 4]


def _pointer(rng, e, base):
    return {1: 0xFFFF_FFFF_0000, 2: 0x0001_0002_FFD0}.get(e, base + 256 * rng.randrange(1 << 12))


def _half(rng, e, j):
    v = HALVES[(e + j) % len(HALVES)]
    return rng.randrange(P) if v is None else v


def _words4(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def _poseidon2_events(n):
    rng = random.Random(2027)
    pre = np.array([[_half(rng, e, j) for j in range(16)] for e in range(n)], dtype=np.uint64).reshape(n, 16)
    post = permute(pre)
    rows = []
    for e in range(n):
        clk = _clk(e)
        row = [clk, _pointer(rng, e, 0x20_0000)]
        for i in range(8):
            row += [_previous(rng, i + e, clk), int(pre[e, 2 * i]) | (int(pre[e, 2 * i + 1]) << 32)]
        if e % 4 == 3:
            out = [_half(rng, e // 4, j) for j in range(16)]
        else:
            out = [int(v) for v in post[e]]
        rows.append(row + [out[2 * i] | (out[2 * i + 1] << 32) for i in range(8)])
    return rows


def _uint256_events(n):
    rng = random.Random(2028)
    rows = []
    for e in range(n):
        x, y, m = TRIPLES[e % len(TRIPLES)]
        clk = _clk(e)
        row = [clk, _pointer(rng, e, 0x40_0000), _pointer(rng, e + 1 if e in (1, 2) else e, 0x80_0000)]
        for i, w in enumerate(_words4(x)):
            row += [_previous(rng, i + e, clk + 1), w]
        for i, w in enumerate(_words4(y) + _words4(m)):
            row += [_previous(rng, i + e + 1, clk), w]
        rows.append(row + _words4(x * y % modulus_of(m)))
    return rows


_ALL, _TABLES, _SHARDS = {}, {}, {}
N_EVENTS = sum(n for n, _ in SHAPES)


def events(kind, n, start=None):
    """n event records of `kind`, int64 [n, words]: entries start .. start + n of the kind's list (start: where the shape of n events
    begins, START[n]; 0 for another n)."""
    if kind not in _ALL:
        rows = (_poseidon2_events if kind == "poseidon2" else _uint256_events)(N_EVENTS)
        _ALL[kind] = np.array(rows, dtype=np.uint64).view(np.int64).reshape(N_EVENTS, WORDS[kind])
    start = START.get(n, 0) if start is None else start
    assert start + n <= N_EVENTS
    return np.ascontiguousarray(_ALL[kind][start:start + n])


def triple_of(ev_row):
    """(x, y, m) of a UINT256_MUL record."""
    w = [int(v) & M64 for v in ev_row]
    word = lambda at: sum(w[at + 2 * i] << (64 * i) for i in range(4))
    return word(4), word(12), word(20)


# the first event on the first kind of clock whose operands, modulus and result are all above 2^128, the modulus odd
SHARD_START = next(e for e in range(4, 900, 4) if min(TRIPLES[e] + (TRIPLES[e][0] * TRIPLES[e][1] % modulus_of(TRIPLES[e][2]),)) > 1 << 128 and TRIPLES[e][2] % 2)


def shard_events(kind, n):
    """The events of the n-call shard the tests build whole (SHARD_CALLS): events SHARD_START .. SHARD_START + n of the list. The
    first is an ordinary call with full-size operands and a satisfying row: the one-call shard is also proved. The six-call shard
    has all four kinds of clock, and so rows that no run produces; it is only compared."""
    return events(kind, n, start=SHARD_START)


def _build(kind, ev, ctx=None):
    if kind == "uint256":
        return MT.uint256_shard_from(ev, "cpu", ctx=ctx)
    t = torch.as_tensor(ev)
    rd = t[:, 2:18].reshape(-1, 8, 2)
    return MT.poseidon2_shard_from(t[:, 0], t[:, 1], rd[:, :, 1].contiguous(), rd[:, :, 0].contiguous(), t[:, 18:26].contiguous(), "cpu", ctx=ctx)


def host_shard(kind, n):
    """The host builder's shard of shard_events(kind, n): (machine, tables, publics, global events [m, 11]); made once."""
    if (kind, n) not in _SHARDS:
        _SHARDS[(kind, n)] = _build(kind, shard_events(kind, n))
    return _SHARDS[(kind, n)]


def host_table(kind, n, height):
    """The host filler's table of events(kind, n): int64 numpy [height, width] canonical values, made once and left unchanged. The
    builder runs as it is (uint256_shard_from asserts that the words written are x y mod m'), and what it would hand on to close the
    shard is dropped. Without an event the filler makes no table: every row is then the padding row of a one-event table."""
    key = (kind, n, height)
    if key not in _TABLES:
        seen = {}

        def keep(tr, *args, **kwargs):
            seen["main"] = tr.tables[CHIPS[kind]].main
        closing, MT._close_precompile_shard = MT._close_precompile_shard, keep
        try:
            _build(kind, events(kind, max(n, 1)))
        finally:
            MT._close_precompile_shard = closing
        tb = seen["main"].numpy()
        if n == 0:
            tb = np.repeat(tb[1:2], height, axis=0)
        assert tb.shape == (height, R.chip(CHIPS[kind])[0].main_width) and RT.pad32(max(n, 1)) == height
        tb.setflags(write=False)
        _TABLES[key] = tb
    return _TABLES[key]


def montgomery_col_major(table):
    """int64 [height, width] canonical -> uint32 numpy [width, height] Montgomery words: what the device and the native program write."""
    return np.ascontiguousarray(RT.to_monty_np(torch.as_tensor(np.array(table))).T)


def first_difference(kind, want, got, n):
    """None when the two [width, height] word arrays are equal, else a line naming the first column and row that differ."""
    chip = CHIPS[kind]
    if want.shape != got.shape:
        return "%s: shape %s, want %s" % (chip, got.shape, want.shape)
    bad = np.argwhere(want != got)
    if not len(bad):
        return None
    col, row = (int(v) for v in bad[0])
    lay = R.chip(chip)[0].layout
    key = max((k for k, v in lay.items() if v <= col), key=lambda k: lay[k])
    return "%s with %d events: %d words differ, first at column %d (%s), row %d (%s): got %#x, want %#x" % (
        chip, n, len(bad), col, key, row, "event" if row < n else "padding", int(got[col, row]), int(want[col, row]))


def from_bytes_columns(table_cm, at, row):
    """The integer of 32 byte-limb columns at..at + 31 of row `row` of a [width, height] Montgomery table."""
    inv = pow(1 << 32, -1, P)
    by = [int(table_cm[at + i, row]) * inv % P for i in range(32)]
    assert all(b < 256 for b in by)
    return sum(b << (8 * i) for i, b in enumerate(by))


# ------------------------------------------------------------------------------------- the hand-assembled programs, restated
POSEIDON2_STATE = [(17 * i + 3, (1 << 30) + i) for i in range(8)]
UINT256_CASES = [(0x1234567890ABCDEF << 130 | 77, (1 << 255) + 12345, B256 - 189), (3, 5, 0), (B256 - 1, B256 - 1, 0), (7, 9, 1 << 200)]
DATA_AT = 0x78100000


def poseidon2_program():
    """Two POSEIDON2 calls on one state, the CPU copying a word in between (tests/test_riscv_exec.py): the ELF image."""
    import rv_asm as A
    data = b"".join(struct.pack("<II", lo, hi) for lo, hi in POSEIDON2_STATE) + bytes(64)
    w = A.li(10, DATA_AT) + A.li(11, 0) + A.li(5, 0x133) + [A.enc("ecall")] + [A.enc("ld", 13, 10, 0), A.enc("sd", 13, 10, 64)] \
        + A.li(5, 0x133) + [A.enc("ecall")] + A.halt(0)
    return A.elf(w, data=data)


def poseidon2_program_memory():
    """What the program leaves: {address: word} of the state after two permutations and of the copied word."""
    once = permute(np.array([[x for pair in POSEIDON2_STATE for x in pair]], dtype=np.uint64))
    twice = permute(once)
    out = {DATA_AT + 8 * i: int(twice[0, 2 * i]) | (int(twice[0, 2 * i + 1]) << 32) for i in range(8)}
    out[DATA_AT + 64] = int(once[0, 0]) | (int(once[0, 1]) << 32)
    return out


def uint256_program():
    """UINT256_MUL on the four operand sets of UINT256_CASES (tests/test_riscv_exec.py): the ELF image."""
    import rv_asm as A
    words = lambda v: b"".join(struct.pack("<Q", w) for w in _words4(v))
    data, prog = b"", A.li(28, DATA_AT)
    for i, (x, y, m) in enumerate(UINT256_CASES):
        data += words(x) + words(y) + words(m)
        prog += [A.enc("addi", 10, 28, 96 * i), A.enc("addi", 11, 28, 96 * i + 32)] + A.li(5, 0x0001011D) + [A.enc("ecall")]
    return A.elf(prog + A.halt(0), data=data + bytes(32))


def uint256_program_memory():
    out = {}
    for i, (x, y, m) in enumerate(UINT256_CASES):
        out.update({DATA_AT + 96 * i + 8 * k: w for k, w in enumerate(_words4(x * y % modulus_of(m)))})
    return out


PROGRAMS = {"poseidon2": (poseidon2_program, poseidon2_program_memory, 2), "uint256": (uint256_program, uint256_program_memory, 4)}


# ----------------------------------------------------------------------------------------------------------- the native program
def _write(tmp_path, tag, array, dtype=np.int64):
    src, dst = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(array, dtype=dtype).tobytes())
    return src, dst


def run_rows(form, kind, ev, height, tmp_path, timeout=120):
    """tests/native/p2u_rows FORM rows: the table as uint32 numpy [width, height]."""
    src, dst = _write(tmp_path, "%s_%s_%d_%d" % (form, kind, len(ev), height), ev)
    subprocess.run([EXE, form, "rows", CHIPS[kind], src, str(height), dst], check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.uint32).reshape(R.chip(CHIPS[kind])[0].main_width, height)


def run_div(form, triples, tmp_path, timeout=120):
    """tests/native/p2u_rows FORM div: [(result, carry)] of the (x, y, m) triples as Python integers."""
    limbs = lambda v: [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    rec = np.array([limbs(x) + limbs(y) + limbs(m) for x, y, m in triples], dtype=np.uint32).reshape(len(triples), 24)
    src, dst = _write(tmp_path, "%s_div_%d" % (form, len(triples)), rec, np.uint32)
    subprocess.run([EXE, form, "div", src, dst], check=True, capture_output=True, timeout=timeout)
    out = np.fromfile(dst, dtype=np.uint32).reshape(len(triples), 16)
    value = lambda ws: sum(int(w) << (32 * i) for i, w in enumerate(ws))
    return [(value(r[:8]), value(r[8:])) for r in out]
