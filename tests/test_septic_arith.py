"""The septic field, the curve addition and the root choice of sp1_amd/csrc/septic.hpp, operation by operation, in both forms:
the KB_HD code on the host (no GPU is opened) and a gfx950 kernel with one lane per record (tests/native/septic_ops.hip, which
includes the header unchanged; the device form under `-m gpu`). Every result is checked against tests/septic_model.py: Python
integers, and none of the header's routes — products by the schoolbook rule, inverses as a^(q - 2), squareness by Euler's
criterion in F_q, Frobenius maps as a^(p^k), roots verified by squaring and never computed, sums verified by the AIR's two
inversion-free relations. Nothing here is compared with septic.hpp or with sp1_amd/machines/septic.py.

The coefficient pool is canonical: the stored-domain edge words of tests/kb_edges.py plus the ends of the ranges the lift decides
on (63 2^24, 64 2^24, 16-bit limbs, p / 2)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_cases as G  # noqa: E402
import kb_edges  # noqa: E402
import septic_model as M  # noqa: E402

P = M.P
Y6 = M.Y6_LIMIT
POOL = sorted(set(kb_edges.EDGE_CANONICAL + [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 0xFFFF, 0x10000, Y6, Y6 + 1, 64 << 24]))
Z6 = [0, 0, 0, 0, 0, 0, 1]
FP_SQRT_INPUTS = [0, 1, 4, P - 1] + [pow(pow(3, 127, P), 1 << k, P) for k in range(24)]      # g = 3^127 has order 2^24: every 2-adic order
# last coordinates of a root around both ends of both ranges
Y6_EDGES = [0, 1, 2, Y6 - 1, Y6, Y6 + 1, (64 << 24) - 1, 64 << 24, (64 << 24) + 1, P - 2, P - 1]
NORM_EXP = (M.Q - 1) // (P - 1)                                                             # r = 1 + p + ... + p^6


@functools.lru_cache(maxsize=None)
def elements():
    """pool-drawn and random elements, squares of some of each, 0, 1, z, z^6"""
    rng = np.random.default_rng(777)
    pool = [[POOL[i] for i in rng.integers(0, len(POOL), 7)] for _ in range(200)]
    pool += [[w] * 7 for w in (P - 1, P - 2, 0x7EFFFFFF * G.R_INV % P)] + [[w] + [0] * 6 for w in POOL[:8]]
    rnd = [[int(v) for v in row] for row in rng.integers(0, P, (200, 7))]
    squares = [M.mul(a, a) for a in pool[:60] + rnd[:60]]
    return pool + rnd + squares + [M.ZERO, M.ONE, M.Z, Z6]


@functools.lru_cache(maxsize=None)
def points(n, seed):
    """n points on the curve with pairwise distinct x: x random, y a root from the host form's s7_sqrt, VERIFIED here as y^2 = rhs."""
    rng = np.random.default_rng(seed)
    xs = [[int(v) for v in row] for row in rng.integers(0, P, (3 * n + 16, 7))]
    can, raw = G.run_ops("host", [(G.OP_SQRT, 0, M.curve_rhs(x)) for x in xs])
    pts = [(x, [int(v) for v in can[i, 1:8]]) for i, x in enumerate(xs) if raw[i, 0] == 1][:n]
    assert len(pts) == n and all(M.on_curve(p) for p in pts)
    return pts


@functools.lru_cache(maxsize=None)
def records():
    """[(record, check(canonical result words, raw result words) -> bool)]"""
    E = elements()
    rng = np.random.default_rng(778)
    recs = []

    def first7(want):
        return lambda can, raw, want=want: can[:7].tolist() == want and not raw[7:].any()
    for i, a in enumerate(E):                                                   # products: neighbours, squares, by the pool's heavy elements
        for b in (E[(i + 1) % len(E)], a, E[i % 11]):
            recs.append(((G.OP_MUL, 0, a, b), first7(M.mul(a, b))))
        recs.append(((G.OP_CURVE_RHS, 0, a), first7(M.curve_rhs(a))))
    some = E[:12] + E[211:223] + E[411:419] + E[-4:]                            # pool-drawn, random, squares, 0 / 1 / z / z^6
    for a in some:
        for k in range(1, 7):
            recs.append(((G.OP_FROB, k, a), first7(M.frob(a, k))))
        t, n = M.spow(a, NORM_EXP - 1), M.spow(a, NORM_EXP)
        assert n[1:] == [0] * 6                                                 # the norm lies in F_p
        recs.append(((G.OP_NORM_PARTS, 0, a), lambda can, raw, t=t, n=n: can[:7].tolist() == t and can[7] == n[0] and not raw[8:].any()))
    for k in range(1, 7):                                                       # make_frob_tables(): row i of map k is (z^i)^(p^k)
        for i in range(7):
            zi = [int(j == i) for j in range(7)]
            recs.append(((G.OP_FROB_TABLE, k | (i << 8)), first7(M.spow(zi, P ** k))))
    for a in E[:100] + E[211:311] + E[-4:]:
        # s7_inv(0) is pinned to what the code returns, 0 (a^(q - 2) is 0 there too). The reference's inverse is not defined at
        # 0 (its try_inverse returns None); the curve addition meets it only for two points of equal x, which is out of scope.
        want = M.inv(a)
        assert a == M.ZERO or M.mul(a, want) == M.ONE
        recs.append(((G.OP_INV, 0, a), first7(want)))
    for a in FP_SQRT_INPUTS:
        if a == 0 or pow(a, (P - 1) // 2, P) == 1:                              # a residue: the result squares back to it
            recs.append(((G.OP_FP_SQRT, 0, [a]), lambda can, raw, a=a: can[0] * can[0] % P == a and not raw[1:].any()))
        else:                                                                   # g itself: no root to promise, a reduced word still
            recs.append(((G.OP_FP_SQRT, 0, [a]), lambda can, raw: raw[0] < P and not raw[1:].any()))
    for a in E:
        # flag == Euler's criterion, on squares and non-squares alike; root^2 = n under the flag. s7_sqrt(0) is pinned to what the
        # code returns: NOT a square. The reference's sqrt returns Some(0) at 0; a root of 0 has y6 = 0, which its lift rejects
        # as an exception, so the lift agrees either way.
        sq = M.is_square(a)

        def chk(can, raw, a=a, sq=sq):
            if raw[0] != int(sq) or raw[8:].any():
                return False
            root = can[1:8].tolist()
            return M.mul(root, root) == a if sq else not raw[1:8].any()
        recs.append(((G.OP_SQRT, 0, a), chk))
    for y6 in Y6_EDGES:
        for recv in (1, 0):
            for _ in range(2):
                root = [int(v) for v in rng.integers(0, P, 6)] + [y6]
                neg6 = -y6 % P
                pos_ok, neg_ok = 1 <= y6 <= Y6, 1 <= neg6 <= Y6
                assert not (pos_ok and neg_ok)                                  # the two ranges are disjoint
                if not pos_ok and not neg_ok:
                    recs.append(((G.OP_PICK_ROOT, recv, root), lambda can, raw: not raw.any()))
                    continue
                recv_root = root if pos_ok else M.neg(root)                     # last coordinate in [1, 63 2^24]
                y = recv_root if recv else M.neg(recv_root)
                value = y[6] - 1 if recv else P - 1 - y[6]
                assert 0 <= value < Y6 and value >> 24 <= 62
                recs.append(((G.OP_PICK_ROOT, recv, root),
                             lambda can, raw, y=y, value=value: raw[0] == 1 and can[1:8].tolist() == y and raw[8] == value and not raw[9:].any()))
    # curve additions: random pairs, start + dummy, and chains of 40 (each link's inputs are values of the integer model)
    pts = points(104, 991)

    def add_check(p1, p2):
        def chk(can, raw, p1=p1, p2=p2):
            p3 = (can[:7].tolist(), can[7:14].tolist())
            return M.sum_holds(p1, p2, p3) and M.on_curve(p3) and not raw[14:].any()
        return chk
    for i in range(0, 24, 2):
        recs.append(((G.OP_EC_ADD, 0, pts[i][0], pts[i][1], pts[i + 1][0], pts[i + 1][1]), add_check(pts[i], pts[i + 1])))
    assert M.on_curve(M.START) and M.on_curve(M.DUMMY)
    recs.append(((G.OP_EC_ADD, 0, M.START[0], M.START[1], M.DUMMY[0], M.DUMMY[1]), add_check(M.START, M.DUMMY)))
    for acc, chain in ((M.START, pts[24:64]), (M.DUMMY, pts[64:104])):           # chains of 40 from the start and the dummy point
        for pt in chain:
            recs.append(((G.OP_EC_ADD, 0, acc[0], acc[1], pt[0], pt[1]), add_check(acc, pt)))
            acc = M.ec_add(acc, pt)
    return recs


def run_and_check(form):
    recs = records()
    can, raw = G.run_ops(form, [r for r, _ in recs])
    bad = [(r[0], r[1], [hex(v) for v in (r[2] if len(r) > 2 else [])], raw[i].tolist()) for i, (r, chk) in enumerate(recs) if not chk(can[i], raw[i])]
    assert not bad, "%s: %d of %d wrong, first: %s" % (form, len(bad), len(recs), bad[:4])
    return len(recs)


def test_operand_set_covers_the_edges():
    recs = [r for r, _ in records()]
    assert {r[0] for r in recs} == set(range(10))
    E = elements()
    assert all(0 <= v < P for a in E for v in a) and M.ZERO in E and M.ONE in E and M.Z in E and Z6 in E
    assert {Y6, Y6 + 1, 64 << 24, 0xFFFF, 0x10000, (P - 1) // 2, (P + 1) // 2, P - 1, P - 2} <= set(POOL)
    squares = sum(M.is_square(a) for a in E[:40])
    assert 5 < squares < 35                                                     # squares and non-squares both
    # every 2-adic order: g^(2^k) has order 2^(24 - k)
    g = pow(3, 127, P)
    assert all(pow(pow(g, 1 << k, P), 1 << (24 - k), P) == 1 and pow(pow(g, 1 << k, P), 1 << (23 - k), P) != 1 for k in range(24))
    picks = [(r[1], r[2][6]) for r in recs if r[0] == G.OP_PICK_ROOT]
    assert {(d, y) for d in (0, 1) for y in Y6_EDGES} == set(picks)
    # the rejected last coordinates are 0 and [63 2^24 + 1, 64 2^24]: p - 63 2^24 = 64 2^24 + 1 is the first of a send's range
    assert P - Y6 == (64 << 24) + 1
    assert all(not (1 <= y <= Y6 or 1 <= -y % P <= Y6) for y in (0, Y6 + 1, (64 << 24) - 1, 64 << 24))
    assert all(1 <= y <= Y6 or 1 <= -y % P <= Y6 for y in (1, 2, Y6 - 1, Y6, (64 << 24) + 1, P - 2, P - 1))


def test_host_form_matches_the_integer_model():
    assert run_and_check("host") > 2000


@pytest.mark.gpu
def test_device_form_matches_the_integer_model():
    assert run_and_check("device") > 2000
