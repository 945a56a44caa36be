"""The KoalaBear operations of sp1_amd/csrc/kb31.hpp at their edges, in both forms: the KB_HD code on the host and a gfx950
kernel with one lane per record (tests/native/kb31_ops.hip, which includes the header unchanged). Every result word is checked
against Python integers computed here from p and R = 2^32 alone; the extension field comes from oracle/kb_py.py (canonical
integers, no Montgomery words). Nothing here is compared with kb31.hpp itself.

Kernels see stored (Montgomery) words, so the edges are chosen in that domain: words whose 16-bit halves are 0 or 0xffff
under the largest high half (0x7effffff, p - 1 = 0x7f000000), the Montgomery one and its negative, and the values around
p/2. The delayed-reduction accumulators (dot_add, edot_add) are driven for exactly as many terms as their comments allow,
of the largest terms there are; the 64-bit reducers are called at the ends of their documented domains and never outside.
test_documented_bounds restates each comment's range argument as arithmetic, so that a comment which drifts from the code
is noticed."""
import functools
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kb_py  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "kb31_ops.hip")
EXE = os.path.join(ROOT, "tests", "native", "kb31_ops")

P = 0x7F000001
R = 1 << 32
R_INV = pow(R, -1, P)
R1 = R % P
M32 = R - 1
assert P == 2 ** 31 - 2 ** 24 + 1 and R1 == 0x01FFFFFE and kb_py.P == P

OP_NAMES = ["add", "sub", "neg", "dbl", "mul", "sqr", "to_monty", "from_monty", "monty_reduce_lazy", "monty_reduce",
            "monty_reduce_wide", "pow", "inv", "two_adic_generator", "reverse_bits_len", "ext_add", "ext_sub", "ext_mul_base",
            "ext_mul", "ext_inv", "dot", "edot", "dot_reduce64"]
(OP_ADD, OP_SUB, OP_NEG, OP_DBL, OP_MUL, OP_SQR, OP_TO_MONTY, OP_FROM_MONTY, OP_REDUCE_LAZY, OP_REDUCE, OP_REDUCE_WIDE, OP_POW,
 OP_INV, OP_GEN, OP_REVBITS, OP_EXT_ADD, OP_EXT_SUB, OP_EXT_MUL_BASE, OP_EXT_MUL, OP_EXT_INV, OP_DOT, OP_EDOT,
 OP_DOT_REDUCE64) = range(23)

# stored words at the edges (all < p)
EDGE_WORDS = [0, 1, 2, R1, P - R1, P - 2, P - 1, (P - 1) // 2, (P + 1) // 2, 0xFFFF, 0x10000, 0x00FFFFFF, 0x01000000, 0x7EFFFFFF,
              0x7EFF0000]
EXT_POOL = [0, 1, P - 1, 0x7EFFFFFF]
MAX_DOT_TERMS = 1 << 16        # kb31.hpp: dot_add, "at most 2^16 calls between dot_init and dot_finish"
MAX_EDOT_TERMS = 1 << 14       # kb31.hpp: edot_add, "At most 2^14 terms"

# the documented domains of the 64-bit reducers (exclusive upper ends)
LAZY_TOP = 1 << 63             # monty_reduce_lazy: "Needs x < 2^63"
REDUCE_TOP = R * P             # monty_reduce: "x < 2^32 * p"
WIDE_TOP = 4 * (P - 1) ** 2 + 1  # monty_reduce_wide: any sum of four products of reduced words
DOT64_TOP = 1 << 63            # dot_reduce64: "S < 2^63"


def test_documented_bounds():
    """Each range argument in kb31.hpp's comments, as arithmetic."""
    assert all(w < P for w in EDGE_WORDS + EXT_POOL)
    # monty_reduce_lazy: (x + t p) >> 32 with t < 2^32 must not overflow 64 bits, and lies in [x / 2^32, x / 2^32 + p)
    assert (LAZY_TOP - 1) + M32 * P < 1 << 64
    # ... so below 2^32 p it is in [0, 2p), which is what monty_reduce's single conditional subtraction needs
    assert ((REDUCE_TOP - 1) >> 32) + P < 2 * P
    # monty_reduce_wide: 4 (p - 1)^2 = 2^64 - 2^58 + 2^50 fits 64 bits; its high word is 2^32 - 2^26 + 2^18 < 2p, so one
    # conditional subtraction of p from the high word brings x under 2^32 p
    assert 4 * (P - 1) ** 2 == 2 ** 64 - 2 ** 58 + 2 ** 50 < 1 << 64
    assert (4 * (P - 1) ** 2) >> 32 == 2 ** 32 - 2 ** 26 + 2 ** 18 < 2 * P < 1 << 32
    assert WIDE_TOP - 1 < R * 2 * P
    # the wrap multiples of ext_mul are reduced words, so a coefficient is a sum of four products of words <= p - 1
    assert 4 * (P - 1) * (P - 1) < WIDE_TOP
    # dot_add: 2^16 partial products of a reduced word and a 16-bit half stay under dot_reduce64's 2^63
    assert MAX_DOT_TERMS * (P - 1) * 0xFFFF < DOT64_TOP
    assert (P - 1) * 0xFFFF < 1 << 47
    # edot_add: four partial products per term and coordinate, 2^14 terms
    assert 4 * MAX_EDOT_TERMS * (P - 1) * 0xFFFF < DOT64_TOP
    # dot_reduce64: the high word of S < 2^63 is < 2^31 < 2p (one conditional subtraction), the low word is < 2^32 p
    assert (DOT64_TOP - 1) >> 32 < 1 << 31 < 2 * P
    assert M32 < REDUCE_TOP
    # dot_finish's constant: to_monty(2^16)
    assert (1 << 48) % P == (1 << 16) * R % P
    # the high half of a reduced word is at most 0x7f00: the hi accumulator is the smaller of the two
    assert (P - 1) >> 16 == 0x7F00


def _rot(e, k):
    return [e[(i + k) & 3] for i in range(4)]


def reducer_inputs():
    """[(op, x)], every x inside the function's documented domain."""
    rng = np.random.default_rng(3131)
    base = [0, 1, 2, M32, R, R + 1, R * P - 1, R * P, (1 << 63) - 1, 1 << 62, (1 << 62) - 1]
    base += [k << 32 for k in (1, 2, 0xFFFF, 0x10000, P - 1, P, P + 1, (1 << 31) - 1, 0x7EFFFFFF)]      # zero low word
    base += [(k << 32) | lo for k in (0, 1, P - 1, (1 << 31) - 1) for lo in (M32, 1, P, P - 1, 0x7EFFFFFF, 0x81000001, 0x80000000)]
    # a high word in [p, 2^31) over a low word that reduces to p - 1 and p - 2: dot_reduce64's sum of the two lands on 2p and above
    base += [(h << 32) | lo for h in (P, P + 1, (1 << 31) - 1) for lo in (P - R1, (P - 2) * R % P)]
    wide = [k * (P - 1) ** 2 for k in (1, 2, 3, 4)] + [4 * (P - 1) ** 2 - 1, (P << 32) - 1, P << 32, (P << 32) | M32,
                                                       ((4 * (P - 1) ** 2) >> 32) << 32]
    wide += [a * b + c * d + e * f + g * h for a, b, c, d, e, f, g, h in
             [[int(v) for v in rng.choice(np.array(EDGE_WORDS, dtype=np.uint64), 8)] for _ in range(2048)]]
    recs = []
    for op, top, extra in ((OP_REDUCE_LAZY, LAZY_TOP, []), (OP_REDUCE, REDUCE_TOP, []), (OP_REDUCE_WIDE, WIDE_TOP, wide),
                           (OP_DOT_REDUCE64, DOT64_TOP, [])):
        xs = [x for x in base + extra if x < top]
        xs += [int(v) % top for v in rng.integers(0, 1 << 64, 4096, dtype=np.uint64)]
        xs += [int(v) % min(top, REDUCE_TOP) for v in rng.integers(0, 1 << 64, 4096, dtype=np.uint64)]
        recs += [(op, x) for x in xs]
    return recs


@functools.lru_cache(maxsize=None)
def operand_set():
    """[(op, n, a[4], b[4], c[4], x)] with every operand inside the operation's contract."""
    rng = np.random.default_rng(3100)
    Z = [0, 0, 0, 0]
    recs = []

    def base(op, a=0, b=0, n=0, x=0):
        recs.append((op, n, [a, 0, 0, 0], [b, 0, 0, 0], Z, x))

    pairs = [(a, b) for a in EDGE_WORDS for b in EDGE_WORDS]
    pairs += [(int(a), int(b)) for a, b in rng.integers(0, P, (1 << 16, 2))]
    for a, b in pairs:
        for op in (OP_ADD, OP_SUB, OP_MUL):
            base(op, a, b)
    singles = EDGE_WORDS + [int(a) for a in rng.integers(0, P, 4096)]
    for a in singles:
        for op in (OP_NEG, OP_DBL, OP_SQR, OP_TO_MONTY, OP_FROM_MONTY):
            base(op, a)
        if a:
            base(OP_INV, a)
    for a in EDGE_WORDS + singles[-64:]:
        for e in (0, 1, 2, 3, P - 2, P - 1, P, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 63, int(rng.integers(0, 1 << 63))):
            base(OP_POW, a, x=e)
    for op, x in reducer_inputs():
        base(op, x=x)
    for bits in range(kb_py.TWO_ADICITY + 1):
        base(OP_GEN, n=bits)
    for bits in range(33):
        top = (1 << bits) - 1
        for x in sorted({0, 1, top, top >> 1, (top >> 1) + 1 if bits else 0, top & 0x55555555, top & 0xAAAAAAAA, M32, 0x80000000,
                         0x7F000001, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)) & top}):
            base(OP_REVBITS, x, n=bits)
    # extension elements: all 4-tuples over the pool, all ordered pairs of them; random ones
    tuples = [[a, b, c, d] for a in EXT_POOL for b in EXT_POOL for c in EXT_POOL for d in EXT_POOL]
    epairs = [(a, b) for a in tuples for b in tuples]
    rnd = rng.integers(0, P, (4096, 2, 4)).tolist()
    epairs += [(a, b) for a, b in rnd]
    epairs += [(a, tuples[i % len(tuples)]) for i, (a, _) in enumerate(rnd[:512])]
    for a, b in epairs:
        for op in (OP_EXT_ADD, OP_EXT_SUB, OP_EXT_MUL):
            recs.append((op, 0, a, b, Z, 0))
    for a in tuples + [r[0] for r in rnd[:256]]:
        for s in EDGE_WORDS:
            recs.append((OP_EXT_MUL_BASE, 0, a, [s, 0, 0, 0], Z, 0))
        if any(a):
            recs.append((OP_EXT_INV, 0, a, Z, Z, 0))
    for a in [[w, 0, 0, 0] for w in EDGE_WORDS if w] + [[0, w, 0, 0] for w in EDGE_WORDS if w] + [[w] * 4 for w in EDGE_WORDS if w]:
        recs.append((OP_EXT_INV, 0, a, Z, Z, 0))
    # the accumulators at their stated lengths, of the largest terms
    top, v16 = [P - 1] * 4, 0x7EFFFFFF
    for n in (MAX_DOT_TERMS, MAX_DOT_TERMS - 1, 1, 0, 4097):
        for e, v in ((top, [v16] * 4), (top, top), ([v16] * 4, [v16] * 4), ([0x7EFF0000] * 4, [0xFFFF] * 4), ([R1, 0, P - 1, v16], [v16, P - 1, 1, 0])):
            recs.append((OP_DOT, n, e, v, Z, 0))
    for n in (MAX_DOT_TERMS, 1000, 5):
        for e, v in (([P - 1, v16, 0, 1], [v16, P - 1, 0xFFFF, 0x7EFF0000]), (rnd[0][0], rnd[0][1])):
            recs.append((OP_DOT, n, e, v, Z, 1))
    three = lambda a: [3 * w % P for w in a]
    for n in (MAX_EDOT_TERMS, MAX_EDOT_TERMS - 1, 1, 0, 4097):
        for a, b in ((top, top), (top, [v16] * 4), ([v16] * 4, [v16] * 4), ([(P + 1) // 2 - 1] * 4, [v16] * 4), ([R1, 0, P - 1, v16], [v16, P - 1, 1, 0])):
            recs.append((OP_EDOT, n, a, b, three(a), 0))
    for n in (MAX_EDOT_TERMS, 1000, 5):
        for a, b in (([P - 1, v16, 0, 1], [v16, P - 1, 0xFFFF, 0x7EFF0000]), (rnd[1][0], rnd[1][1])):
            recs.append((OP_EDOT, n, a, b, three(a), 1))
    return recs


def _stored_ext_mul(a, b):
    """The stored words of the product of two stored extension elements: the product is bilinear, so one factor 2^-32."""
    return kb_py.ext_scale(kb_py.ext_mul(a, b), R_INV)


def expected(rec):
    """The result words, or a predicate on them for monty_reduce_lazy (which promises a range, not a value)."""
    op, n, a, b, c, x = rec
    a0, b0 = a[0], b[0]
    one = lambda v: [v, 0, 0, 0]
    if op == OP_ADD:
        return one((a0 + b0) % P)
    if op == OP_SUB:
        return one((a0 - b0) % P)
    if op == OP_NEG:
        return one(-a0 % P)
    if op == OP_DBL:
        return one(2 * a0 % P)
    if op == OP_MUL:
        return one(a0 * b0 * R_INV % P)
    if op == OP_SQR:
        return one(a0 * a0 * R_INV % P)
    if op == OP_TO_MONTY:
        return one(a0 * R % P)
    if op == OP_FROM_MONTY:
        return one(a0 * R_INV % P)
    if op in (OP_REDUCE, OP_REDUCE_WIDE, OP_DOT_REDUCE64):
        return one(x * R_INV % P)
    if op == OP_POW:
        return one(pow(a0 * R_INV % P, x, P) * R % P)
    if op == OP_INV:
        return one(pow(a0 * R_INV % P, -1, P) * R % P)
    if op == OP_GEN:
        return one(kb_py.two_adic_generator(n) * R % P)
    if op == OP_REVBITS:
        return one(kb_py.reverse_bits_len(a0 & ((1 << n) - 1), n))
    if op == OP_EXT_ADD:
        return kb_py.ext_add(a, b)
    if op == OP_EXT_SUB:
        return kb_py.ext_sub(a, b)
    if op == OP_EXT_MUL_BASE:
        return kb_py.ext_scale(a, b0 * R_INV % P)
    if op == OP_EXT_MUL:
        return _stored_ext_mul(a, b)
    if op == OP_EXT_INV:
        return kb_py.ext_scale(kb_py.ext_inv(kb_py.ext_scale(a, R_INV)), R)
    if op in (OP_DOT, OP_EDOT):
        # the four rotations repeat with period 4: n terms are q whole periods and the first n % 4 terms once more
        acc = [0, 0, 0, 0]
        for r in range(4):
            count = n // 4 + (1 if r < n % 4 else 0) if x & 1 else (n if r == 0 else 0)
            if not count:
                continue
            if op == OP_DOT:
                term = kb_py.ext_scale(_rot(a, r), b[r & 3])
            else:
                assert c == [3 * w % P for w in a]
                term = kb_py.ext_mul(_rot(a, r), _rot(b, r))
            acc = kb_py.ext_add(acc, kb_py.ext_scale(term, count))
        return kb_py.ext_scale(acc, R_INV)
    raise ValueError(op)


def check(rec, got):
    op, n, a, b, c, x = rec
    if op == OP_REDUCE_LAZY:
        r = got[0]
        ok = got[1:] == [0, 0, 0] and r % P == x * R_INV % P and x <= r << 32 < x + R * P      # [x / 2^32, x / 2^32 + p)
        if x < REDUCE_TOP:
            ok = ok and r < 2 * P
        return ok
    want = expected(rec)
    if got != want:
        return False
    if op == OP_EXT_INV:        # a * a^-1 = 1 (the stored one)
        return _stored_ext_mul(a, got) == [R1, 0, 0, 0]
    if op == OP_INV:
        return a[0] * got[0] * R_INV % P == R1
    if op == OP_GEN:            # order exactly 2^bits
        g = got[0] * R_INV % P
        return pow(g, 1 << n, P) == 1 and (n == 0 or pow(g, 1 << (n - 1), P) != 1)
    return True


def _encode(recs):
    words = np.zeros((len(recs), 16), np.uint32)
    words[:, 0] = [r[0] for r in recs]
    words[:, 1] = [r[1] for r in recs]
    words[:, 2:6] = [r[2] for r in recs]
    words[:, 6:10] = [r[3] for r in recs]
    words[:, 10:14] = [r[4] for r in recs]
    words[:, 14] = [r[5] & M32 for r in recs]
    words[:, 15] = [r[5] >> 32 for r in recs]
    return np.concatenate([np.array([len(recs)], np.uint32), words.reshape(-1)])


def run_and_check(exe, form, timeout):
    recs = operand_set()
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        _encode(recs).tofile(fin)
        r = subprocess.run([exe, form, fin, fout], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout + r.stderr
        out = np.fromfile(fout, dtype="<u4").reshape(-1, 4)
    assert out.shape[0] == len(recs)
    bad = [(OP_NAMES[rec[0]], rec[1], [hex(v) for v in rec[2]], [hex(v) for v in rec[3]], hex(rec[5]), [hex(v) for v in got])
           for rec, got in zip(recs, out.tolist()) if not check(rec, got)]
    assert not bad, "%s: %d of %d wrong, first: %s" % (form, len(bad), len(recs), bad[:8])
    return len(recs)


def test_operand_set_covers_the_edges():
    """The set itself: every operation appears, every operand is a reduced word inside its function's domain, and the cases
    that sit on a bound are in it."""
    recs = operand_set()
    assert {r[0] for r in recs} == set(range(len(OP_NAMES)))
    by_op = lambda op: [r for r in recs if r[0] == op]
    for r in recs:
        if r[0] not in (OP_REVBITS,):
            assert all(w < P for w in r[2] + r[3] + r[4]), r
    assert all(r[5] < LAZY_TOP for r in by_op(OP_REDUCE_LAZY)) and any(r[5] == LAZY_TOP - 1 for r in by_op(OP_REDUCE_LAZY))
    assert all(r[5] < REDUCE_TOP for r in by_op(OP_REDUCE)) and any(r[5] == REDUCE_TOP - 1 for r in by_op(OP_REDUCE))
    assert all(r[5] < WIDE_TOP for r in by_op(OP_REDUCE_WIDE))
    assert {k * (P - 1) ** 2 for k in (1, 2, 3, 4)} <= {r[5] for r in by_op(OP_REDUCE_WIDE)}
    assert all(r[5] < DOT64_TOP for r in by_op(OP_DOT_REDUCE64)) and any(r[5] == DOT64_TOP - 1 for r in by_op(OP_DOT_REDUCE64))
    assert all(r[1] <= MAX_DOT_TERMS for r in by_op(OP_DOT)) and all(r[1] <= MAX_EDOT_TERMS for r in by_op(OP_EDOT))
    assert (OP_DOT, MAX_DOT_TERMS, [P - 1] * 4, [0x7EFFFFFF] * 4, [0] * 4, 0) in recs
    assert (OP_DOT, MAX_DOT_TERMS, [P - 1] * 4, [P - 1] * 4, [0] * 4, 0) in recs
    assert (OP_EDOT, MAX_EDOT_TERMS, [P - 1] * 4, [P - 1] * 4, [P - 3] * 4, 0) in recs
    assert (OP_EDOT, MAX_EDOT_TERMS, [P - 1] * 4, [0x7EFFFFFF] * 4, [P - 3] * 4, 0) in recs
    assert {0, 1} <= {r[1] for r in by_op(OP_DOT)} and {0, 1} <= {r[1] for r in by_op(OP_EDOT)}
    adds = {(r[2][0], r[3][0]) for r in by_op(OP_ADD)}
    assert (1, P - 1) in adds and (P - 1, P - 1) in adds and ((P + 1) // 2, (P - 1) // 2) in adds      # s == p, the largest s
    assert (0, P - 1) in {(r[2][0], r[3][0]) for r in by_op(OP_SUB)}
    assert {r[1] for r in by_op(OP_GEN)} == set(range(25)) and {r[1] for r in by_op(OP_REVBITS)} == set(range(33))


def _host_compiler():
    gxx = shutil.which("g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if gxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        return None, None
    return gxx, rocm


def test_host_form_matches_python():
    """kb31.hpp's KB_HD code compiled for the CPU by a plain C++ compiler: no GPU is opened."""
    gxx, rocm = _host_compiler()
    if gxx is None:
        pytest.skip("no g++ or no HIP headers")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "kb31_ops_host")
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                               "-I" + os.path.join(ROOT, "sp1_amd", "csrc"), "-x", "c++", SRC, "-o", exe])
        assert run_and_check(exe, "host", timeout=300) > 1 << 18


@pytest.mark.gpu
def test_device_form_matches_python():
    assert os.path.exists(EXE), "tests/native/kb31_ops is not built (__graft_entry__.build())"
    assert run_and_check(EXE, "device", timeout=120) > 1 << 18
