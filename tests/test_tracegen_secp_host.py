"""CPU: the secp256k1 trace rows as the device kernels compute them, run on the host. tests/native/secp_rows (built by
__graft_entry__.build()) includes sp1_amd/csrc/fp256.hpp and tg_field_op.hpp unchanged; its `host` form runs the same row
functions the kernels of tracegen_weierstrass.hip call, on the CPU, and never opens a GPU.

* every word of both tables equals the host filler's (riscv_more_trace.secp256k1_add_table / _double_table: Python integers,
  checked row by row against the chips' constraints in test_riscv_exec.py), padding rows included, at (events, height) =
  (0, 32), (1, 32), (32, 32) — no padding —, (33, 64) and the whole edge set at its pad32, over the operand set of
  tests/secp_cases.py; everything is bit-exact, there are no tolerances;
* x3 and y3 in the rows equal the words the events carry and, for multiples of G, Python's affine arithmetic;
* fp256 alone against Python integers — add, sub, mul, inv and the quotient — on the edge elements, on products that land on 0
  and p - 1, on random elements, and modulo two more primes and an odd composite, since the modulus is data;
* the header's column constants equal R.chip(name)[0].layout."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import secp_cases as SC  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

EDGE_SETS = {"add": 111, "double": 110}


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(SC.EXE), "tests/native/secp_rows is not built: run __graft_entry__.build()"


def _shapes(kind):
    n = EDGE_SETS[kind]
    return SC.SHAPES[:4] + [(n, RT.pad32(n))]


@pytest.mark.parametrize("kind", ["add", "double"])
@pytest.mark.parametrize("which", range(5))
def test_every_word_equals_the_host_filler(kind, which, tmp_path):
    n, height = _shapes(kind)[which]
    want = SC.montgomery_col_major(SC.host_table(kind, n, height))
    got = SC.run_rows("host", kind, SC.events(kind, n), height, tmp_path)
    assert got.shape == want.shape
    msg = SC.first_difference(kind, want, got, n)
    assert msg is None, msg


@pytest.mark.parametrize("kind", ["add", "double"])
def test_rows_past_the_edge_set_multiples_of_g_and_random(kind, tmp_path):
    """The 64 events after the edge set: the 40 multiples of G and 24 random ones. Their x3 / y3 are Python's affine arithmetic."""
    start, n, height = EDGE_SETS[kind], 64, 64
    ev = SC.events(kind, n, start)
    got = SC.run_rows("host", kind, ev, height, tmp_path)
    msg = SC.first_difference(kind, SC.montgomery_col_major(SC.host_table(kind, n, height, start)), got, n)
    assert msg is None, msg
    mg = SC.multiples_of_g(2 * SC.N_MULTIPLES + 1)
    if kind == "add":
        want = [SC.affine_add(mg[2 * SC.N_MULTIPLES], SC.G)] * SC.N_MULTIPLES              # (k + 1) G + (81 - k) G = 82 G
    else:
        want = [mg[2 * k + 1] for k in range(SC.N_MULTIPLES)]                              # 2 (k + 1) G
    assert SC.result_words(kind, got, range(SC.N_MULTIPLES)) == want


@pytest.mark.parametrize("kind", ["add", "double"])
def test_x3_y3_are_the_words_written(kind, tmp_path):
    n = EDGE_SETS[kind]
    ev = SC.events(kind, n)
    got = SC.run_rows("host", kind, ev, RT.pad32(n), tmp_path)
    u = ev.view(np.uint64)
    written = [(sum(int(w) << (64 * i) for i, w in enumerate(r[-8:-4])), sum(int(w) << (64 * i) for i, w in enumerate(r[-4:]))) for r in u]
    assert SC.result_words(kind, got, range(n)) == written


def test_column_constants_equal_the_transcribed_layouts():
    text = subprocess.run([SC.EXE, "host", "layout", "-", "-"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {"Secp256k1AddAssign": 0, "Secp256k1DoubleAssign": 0}
    for line in text.splitlines():
        chip, key, value = line.split()
        air = R.chip(chip)[0]
        assert int(value) == (air.main_width if key == "width" else air.layout[key]), line
        seen[chip] += 1
    # every field operation and range check of either chip is among them
    for chip, n_ops in (("Secp256k1AddAssign", 10), ("Secp256k1DoubleAssign", 11)):
        ops = {k.rsplit(".", 1)[0] for k in R.chip(chip)[0].layout if k.endswith(".witness")}
        assert len(ops) == n_ops and all(("%s %s.witness " % (chip, o)) in text for o in ops)
        assert seen[chip] >= 3 * n_ops + 6 + 6


# ---------------------------------------------------------------------------------------------------------------- fp256 alone
OPS = {"add": 0, "sub": 1, "mul": 2, "inv": 3}
MODULI = {"secp256k1": SC.P,
          "secp256r1": (1 << 256) - (1 << 224) + (1 << 192) + (1 << 96) - 1,
          "bn254": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
          "small": 65537}


def _limbs(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def _fp(records, p, tmp_path, form="host"):
    """[(op, a, b)] -> [(result, quotient)] by tests/native/secp_rows FORM fp."""
    src, dst = os.path.join(str(tmp_path), "fp.in"), os.path.join(str(tmp_path), "fp.out")
    body = [len(records)] + _limbs(p)
    for op, a, b in records:
        body += [OPS[op]] + _limbs(a) + _limbs(b)
    with open(src, "wb") as f:
        f.write(np.array(body, dtype=np.uint32).tobytes())
    subprocess.run([SC.EXE, form, "fp", src, dst], check=True, capture_output=True, timeout=120)
    out = np.fromfile(dst, dtype=np.uint32).reshape(len(records), 16)
    word = lambda ws: sum(int(w) << (32 * i) for i, w in enumerate(ws))
    return [(word(r[:8]), word(r[8:])) for r in out]


def fp_records(p, seed):
    """Operand records modulo p: all pairs of edge elements (reduced), products that land on 0 and on p - 1, random pairs."""
    rng = random.Random(seed)
    edge = sorted({v % p for v in SC.EDGE} | {p - 1, p - 2, 0, 1, 2})
    pairs = [(a, b) for a in edge for b in edge]
    for _ in range(40):                                              # a * b = p - 1 and a * b = 1 (mod p), b = 0 (product 0)
        a = rng.randrange(1, p)
        try:
            inv = pow(a, -1, p)
        except ValueError:                                           # (not a unit of a composite modulus)
            continue
        pairs += [(a, (p - inv) % p), (a, inv), (a, 0), (0, a)]
    pairs += [(rng.randrange(p), rng.randrange(p)) for _ in range(200)]
    return [(op, a, b) for a, b in pairs for op in ("add", "sub", "mul")] + [("inv", a, 0) for a in sorted({a for a, _ in pairs})]


def fp_expected(records, p):
    out = []
    for op, a, b in records:
        if op == "add":
            out.append(((a + b) % p, (a + b) // p))
        elif op == "sub":
            out.append(((a - b) % p, 0))
        elif op == "mul":
            out.append((a * b % p, a * b // p))
        else:
            out.append((pow(a, p - 2, p), 0))                       # Fermat's power: the inverse modulo a prime, 0 for 0
    return out


@pytest.mark.parametrize("name", sorted(MODULI))
def test_fp256_against_python_integers(name, tmp_path):
    p = MODULI[name]
    records = fp_records(p, 11)
    got = _fp(records, p, tmp_path)
    want = fp_expected(records, p)
    bad = [(r, g, w) for r, g, w in zip(records, got, want) if g != w]
    assert not bad, "%d of %d differ modulo %s; first: %s(%#x, %#x) gave %s, want %s" % (
        len(bad), len(records), name, bad[0][0][0], bad[0][0][1], bad[0][0][2], [hex(v) for v in bad[0][1]], [hex(v) for v in bad[0][2]])
    if name == "secp256k1":
        mul = [(r, w) for r, w in zip(records, want) if r[0] == "mul"]
        assert any(w[0] == 0 and r[1] and r[2] == 0 for r, w in mul) and any(w[0] == p - 1 for r, w in mul) and any(w[0] == 1 and w[1] for r, w in mul)
        assert all(a * g[0] % p == 1 for (op, a, _), g in zip(records, got) if op == "inv" and a)


def test_fp256_modulo_an_odd_composite(tmp_path):
    """The modulus is data and need not be prime for add, sub, mul and the quotient (inv is a^(p-2), whatever that is)."""
    p = 3 * ((1 << 254) + 1)
    records = [r for r in fp_records(p, 5) if r[0] != "inv"]
    assert _fp(records, p, tmp_path) == fp_expected(records, p)
