"""An independent reference for the septic field F_p^7 = F_p[z] / (z^7 - 3 z - 5), the curve y^2 = x^3 + 45 x + 41 z^3 over it and
the Global chip's lift rule, in plain Python integers (canonical residues, 7-lists) — by none of the routes that
sp1_amd/csrc/septic.hpp and sp1_amd/machines/septic.py take:

* a product is the schoolbook product reduced by z^7 = 3 z + 5, one coefficient at a time;
* an inverse is a^(q - 2), q = p^7 (no norm, no Frobenius table);
* squareness is Euler's criterion a^((q - 1) / 2) (no norm);
* a square root is never computed: a claimed root is verified as y^2 = n;
* a Frobenius map is a^(p^k) by exponentiation (no table);
* a curve sum is verified by the two inversion-free relations the AIR uses (`sum_holds`); `ec_add` below, which divides by
  a^(q - 2), is used only where a value is needed (the sequential running sum);
* the lift rule (`lift_check`) restates operations/global_interaction.rs and septic_curve.rs::lift_x as conditions on a row.

Slow on purpose: Euler's criterion and the inverse are 217-bit exponentiations, a few milliseconds each. Callers keep the
integer model to a few hundred elements and use septic.py, which this model pins, for larger sizes."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import kb_py  # noqa: E402

P = 0x7F000001
Q = P ** 7
Y6_LIMIT = 63 << 24
ZERO, ONE, Z = [0] * 7, [1, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0]
# CURVE_CUMULATIVE_SUM_START (septic_digest.rs: the digits of sqrt 2, pi, ...) and CURVE_WITNESS_DUMMY_POINT (septic_curve.rs)
START = ([0x1414213, 0x5623730, 0x9504880, 0x1688724, 0x2096980, 0x7856967, 0x1875376],
         [2020310104, 1513506566, 1843922297, 2003644209, 805967281, 1882435203, 1623804682])
DUMMY = ([0x2718281 + (1 << 24), 0x8284590, 0x4523536, 0x0287471, 0x3526624, 0x9775724, 0x7093699],
         [1250555984, 1592495468, 656721246, 420301347, 2125819749, 819876460, 17687681])


def add(a, b):
    return [(x + y) % P for x, y in zip(a, b)]


def sub(a, b):
    return [(x - y) % P for x, y in zip(a, b)]


def neg(a):
    return [-x % P for x in a]


def mul(a, b):
    t = [0] * 13
    for i in range(7):
        for j in range(7):
            t[i + j] += a[i] * b[j]
    for s in range(12, 6, -1):              # z^s = z^(s - 7) (3 z + 5), highest power first
        t[s - 7] += 5 * t[s]
        t[s - 6] += 3 * t[s]
        t[s] = 0
    return [v % P for v in t[:7]]


def spow(a, e):
    r = list(ONE)
    while e:
        if e & 1:
            r = mul(r, a)
        a = mul(a, a)
        e >>= 1
    return r


def inv(a):
    """a^(q - 2); 0 for a = 0."""
    return spow(a, Q - 2)


def is_square(a):
    """Euler's criterion; 0 counts as no square here (0^e = 0 != 1), which is what the kernels' flag says of it too."""
    return spow(a, (Q - 1) // 2) == ONE


def frob(a, k):
    return spow(a, P ** k)


def curve_rhs(x):
    r = add(mul(mul(x, x), x), [45 * v % P for v in x])
    r[3] = (r[3] + 41) % P
    return r


def on_curve(pt):
    return mul(pt[1], pt[1]) == curve_rhs(pt[0])


def sum_holds(p1, p2, p3):
    """p3 = p1 + p2 by the AIR's two relations (global_accumulation.rs), which hold for x1 != x2 only:
    (x3 + x1 + x2) (x2 - x1)^2 = (y2 - y1)^2 and (y3 + y1) (x2 - x1) = (y2 - y1) (x1 - x3)."""
    (x1, y1), (x2, y2), (x3, y3) = p1, p2, p3
    dx, dy = sub(x2, x1), sub(y2, y1)
    if dx == ZERO:
        return False
    return (mul(add(add(x3, x1), x2), mul(dx, dx)) == mul(dy, dy) and mul(add(y3, y1), dx) == mul(dy, sub(x1, x3)))


def ec_add(p1, p2):
    (x1, y1), (x2, y2) = p1, p2
    slope = mul(sub(y2, y1), inv(sub(x2, x1)))
    x3 = sub(sub(mul(slope, slope), x1), x2)
    return x3, sub(mul(slope, sub(x1, x3)), y1)


def sequential_sum(points, start=START):
    """[start + P_0, start + P_0 + P_1, ...], one addition after the other."""
    out, acc = [], start
    for pt in points:
        acc = ec_add(acc, pt)
        out.append(acc)
    return out


def digest_x(message, kind, offset):
    """get_digest's x: Poseidon2 of (message[0] + kind 2^24, message[1..7], message[7] + offset 2^16, 0 x 8), first 7 words."""
    m = [int(w) % P for w in message] + [0] * 8
    m[0] = (m[0] + (int(kind) << 24)) % P
    m[7] = (m[7] + (int(offset) << 16)) % P
    return kb_py.permute(m)[:7], m


def offset_is_rejected(message, kind, offset, claimed_root=None):
    """No point at this offset: the right-hand side is no square, or — given a root of it, which this model cannot compute —
    neither +-root has its last coordinate in [1, 63 2^24]."""
    x, _ = digest_x(message, kind, offset)
    n = curve_rhs(x)
    if not is_square(n):
        return True
    if claimed_root is None:
        return None                                  # a square: the caller must supply a root to decide
    assert mul(claimed_root, claimed_root) == n
    y6 = claimed_root[6]
    return not (1 <= y6 <= Y6_LIMIT or 1 <= (P - y6) % P <= Y6_LIMIT)


def lift_check(event, row, roots_below=None):
    """event = (message[8], is_receive, kind); row = {"x": [7], "y": [7], "offset": int, "bytes": [4], "perm_in": [16],
    "perm_out": [16]} in canonical words. `roots_below[o]` is a root (from the code under test, verified here by squaring) of the
    right-hand side at offset o < row["offset"] where that one is a square. Returns a list of what is wrong (empty: accepted)."""
    message, is_recv, kind = event
    bad = []
    off = row["offset"]
    if not 0 <= off < 256:
        return ["offset out of range"]
    for o in range(off):
        rej = offset_is_rejected(message, kind, o, (roots_below or {}).get(o))
        if rej is None:
            bad.append("offset %d has a square right-hand side and no root was supplied to show it is out of range" % o)
        elif not rej:
            bad.append("offset %d below the stored one already has a point" % o)
    x, m = digest_x(message, kind, off)
    if row["perm_in"] != m:
        bad.append("permutation input is not the message with kind and offset folded in")
    if row["perm_out"][:7] != x or row["x"] != x:
        bad.append("x is not the digest")
    if not on_curve((row["x"], row["y"])):
        bad.append("the stored point is not on the curve")
    y6 = row["y"][6]
    if is_recv and not 1 <= y6 <= Y6_LIMIT:
        bad.append("a receive's y6 is outside [1, 63 2^24]")
    if not is_recv and not P - Y6_LIMIT <= y6 <= P - 1:
        bad.append("a send's y6 is outside [p - 63 2^24, p - 1]")
    value = y6 - 1 if is_recv else P - 1 - y6
    b = row["bytes"]
    if any(not 0 <= v <= 255 for v in b) or b[0] + (b[1] << 8) + (b[2] << 16) + (b[3] << 24) != value or b[3] > 62:
        bad.append("the bytes do not decompose the range-check value, or the top byte exceeds 62")
    return bad
