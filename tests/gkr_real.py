"""Arbitrary tables of the real chips' interaction programs for LogUp-GKR (tests/test_gkr_real_host.py,
tests/test_gpu_gkr_real.py): no executor, no trace generator, no witness. The LogUp-GKR prover is a deterministic function of
whatever tables it is given and oracle/kb_gkr.hpp restates it densely, so the two are compared byte for byte on tables whose every
cell is drawn from a seeded numpy Generator or from the stored-domain edge pool (tests/kb_edges.py): multiplicities that are not
flags, limbs near p - 1, `is_real` that is not a bit. That is where a wrong beta index past 16, a wrong term behind a multiplicity
that a satisfying trace leaves at zero, or a wrong weight on a limb that is always below 2^16 shows.

Arbitrary tables do not balance, and the verifier then stops at the cumulative sum. So every chip with rows gets a MIRROR: the
same InteractionProgram with sends and receives swapped, named name + "~", over the same tables. Every fraction m / d of the chip
meets -m / d of the mirror, whatever the cells hold: the pair proves and the verifier accepts. A chip of zero rows adds
interactions and no fractions and needs no mirror, which is how the number of interactions is made odd."""
import struct

import numpy as np

import kb_py
import pyoracle as orc
from kb_edges import EdgeSource
from sp1_amd.air import InteractionProgram
from sp1_amd.machines import recursion, riscv

P = 0x7F000001
GRINDING_BITS = 12

_RECURSION = {}


def program(name):
    """The InteractionProgram of a chip of the RISC-V machine, or of the recursion machine where the name is one of its chips."""
    if not _RECURSION:
        _RECURSION.update({it.name: it for _, it in recursion.compress_machine()})
    return _RECURSION[name] if name in _RECURSION else riscv.chip(name)[1]


def mirror(prog):
    """The same interactions with sends and receives swapped, over the same columns."""
    m = InteractionProgram(prog.name + "~", prog.main_width, prog.prep_width)
    m.sends, m.receives = list(prog.receives), list(prog.sends)
    return m


def _renamed(prog, name):
    m = InteractionProgram(name, prog.main_width, prog.prep_width)
    m.sends, m.receives = list(prog.sends), list(prog.receives)
    return m


def _draw(source, rows, width):
    canonical = np.asarray(source.integers(0, P, size=(rows, width), dtype=np.uint64))
    return orc.to_monty(canonical.astype(np.uint32))


def real_gkr_chips(spec, source):
    """spec: [(name, rows, mirrored)]. Returns [(InteractionProgram, main [rows][w] Montgomery row-major, prep or None)] in name
    order, the form orc.gkr_prove takes (and, with the tables on the device, api.logup_gkr). Every main and preprocessed cell is
    drawn from `source` (a seeded numpy Generator or kb_edges.EdgeSource); a chip and its mirror share their arrays. An unmirrored
    chip has no rows. A name that comes again in `spec` is given as name#2, name#3, ...: chip names are distinct."""
    chips, seen = [], {}
    for name, rows, mirrored in spec:
        assert mirrored or rows == 0, "%s: %d rows without a mirror do not balance" % (name, rows)
        prog = program(name)
        seen[name] = seen.get(name, 0) + 1
        if seen[name] > 1:
            prog = _renamed(prog, "%s#%d" % (name, seen[name]))
        main = _draw(source, rows, prog.main_width)
        prep = _draw(source, rows, prog.prep_width) if prog.prep_width else None
        chips.append((prog, main, prep))
        if mirrored:
            chips.append((mirror(prog), main, prep))
    chips.sort(key=lambda c: c[0].name)
    return chips


def source_of(kind, seed):
    return np.random.default_rng(seed) if kind == "rand" else EdgeSource(seed)


def num_interactions(chips):
    return sum(c[0].num_interactions for c in chips)


def shape_stats(prog):
    """What an interaction program asks of the first-layer kernels, over its sends and receives:
      values          most values in a message
      folded          most constant values in a message (no terms: folded into the head of the denominator)
      live            the set of live (non-constant) value counts, which fix the flushes and the tail of first_layers_kernel
      mult_terms      most terms in a multiplicity
      const_mults     multiplicities without a term
      value_terms     most terms in a value's linear form
      weights_not_one terms of a value or a multiplicity whose weight is not one
      interactions    sends + receives"""
    every = prog.sends + prog.receives
    folded = [sum(1 for v in values if not v.terms) for _, values, _ in every]
    return {
        "values": max(len(values) for _, values, _ in every),
        "folded": max(folded),
        "live": {len(values) - f for (_, values, _), f in zip(every, folded)},
        "mult_terms": max(len(m.terms) for _, _, m in every),
        "const_mults": sum(1 for _, _, m in every if not m.terms),
        "value_terms": max([len(v.terms) for _, values, _ in every for v in values] + [0]),
        "weights_not_one": sum(1 for _, values, m in every for v in values + [m] for t in v.terms if t[2] != 1),
        "interactions": len(every),
    }


# ---- the cases ------------------------------------------------------------------------------------------------------------------
HEIGHTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 37, 64, 111, 130, 255, 256]
CORE = sorted(riscv.CHIPS)
RECURSION = [it.name for _, it in recursion.compress_machine()]    # BaseAlu .. Select, eight chips in name order


def _cycled(names, shift):
    return [(n, HEIGHTS[(i + shift) % len(HEIGHTS)], True) for i, n in enumerate(names)]


def _mirrored(pairs):
    return [(n, h, True) for n, h in pairs]


# name -> (spec, L, source kind, seed, number of interactions)
CASES = {
    # every quad residue of a height (0 .. 9), one tile and one tile less a row (256 / 255); all 30 chips of the core machine
    "core-rand": (_cycled(CORE, 0), 8, "rand", 2, 1138),
    "core-edge": (_cycled(CORE, 5), 8, "edge", 5, 1138),
    # the number of interactions at, one past and well below a power of two
    "k16": (_mirrored([("Byte", 37), ("Program", 8), ("Range", 130)]), 8, "rand", 21, 16),
    "k17": (_mirrored([("Byte", 37), ("Program", 8), ("Range", 130)]) + [("Range", 0, False)], 8, "edge", 22, 17),
    "k5": (_mirrored([("Program", 8), ("Range", 130)]) + [("Range", 0, False)], 8, "rand", 23, 5),
    # complete 512-entry blocks of a level plus an incomplete one, at several levels of the tree
    "blocks": (_mirrored([("Add", 1030), ("Byte", 2052), ("DivRem", 516), ("LoadX0", 1030), ("Mul", 4100), ("Program", 1024),
                          ("Range", 513)]), 13, "rand", 3, 474),
    # 106 / 105 live values, 25 values of 16-term forms, 2,640-column openings
    "wide-edge": (_mirrored([("KeccakPermute", 6), ("KeccakPermuteControl", 37), ("ShaCompress", 130), ("ShaExtend", 3)]), 8, "edge", 7, 926),
    "keccak-1030": (_mirrored([("KeccakPermute", 1030), ("KeccakPermuteControl", 130)]), 11, "rand", 7, 562),
    # thousands of interactions on a handful of rows
    "bls-5": (_mirrored([("Bls12381DoubleAssign", 5)]), 3, "rand", 8, 3396),
    "bls-1": (_mirrored([("Bls12381DoubleAssign", 1)]), 1, "edge", 8, 3396),
    "curves": (_mirrored([("Bls12381AddAssign", 37), ("Secp256k1AddAssign", 130)]), 8, "rand", 9, 5620),
    # multiplicities of up to seven terms and of none
    "mults-edge": (_mirrored([("DivRem", 111), ("LoadX0", 37), ("Mul", 6)]), 7, "edge", 11, 416),
    # preprocessed columns in values and multiplicities
    "recursion-rand": (_cycled(RECURSION, 3), 8, "rand", 10, 106),
    "recursion-edge": (_cycled(RECURSION, 3), 8, "edge", 10, 106),
}

_made = {}


def case(name):
    """(chips, L): made once per name and shared, never changed."""
    if name not in _made:
        spec, L, kind, seed, k = CASES[name]
        chips = real_gkr_chips(spec, source_of(kind, seed))
        assert k is None or num_interactions(chips) == k, (name, num_interactions(chips))
        assert all(c[1].shape[0] <= 1 << L for c in chips)
        _made[name] = (chips, L)
    return _made[name]


def seeded(challenger, L):
    """The transcript before LogUp-GKR in these tests: nine seeded felts observed."""
    challenger.observe(orc.random_felts((9,), L))
    return challenger


_proved = {}


def oracle_proof(name):
    """(chips, L, the dense oracle's proof, its transcript state after it): once per case."""
    if name not in _proved:
        chips, L = case(name)
        ch = seeded(orc.Challenger(), L)
        want = orc.gkr_prove(chips, L, ch)
        _proved[name] = (chips, L, want, np.array(ch.state()))
    return _proved[name]


# ---- bincode(LogupGkrProof), as far as these tests read it themselves -------------------------------------------------------------
def decode_proof(blob):
    """The sections of a bincode(LogupGkrProof) in canonical words: {"numerator", "denominator": [2 * 2^niv][4], "rounds": [bytes
    per layer], "round_polys": [[bytes per sumcheck round] per layer], "openings": bytes, "witness": int}. The layers and the openings are
    kept as bytes: they are compared, not read."""
    o = 0

    def u64():
        nonlocal o
        v = struct.unpack_from("<Q", blob, o)[0]
        o += 8
        return v

    def skip_exts(k):
        nonlocal o
        o += 16 * k

    out = {}
    for key in ("numerator", "denominator"):
        n = u64()
        out[key] = np.frombuffer(blob, dtype="<u4", count=4 * n, offset=o).reshape(n, 4).astype(np.uint32)
        o += 16 * n
        assert (u64(), u64(), u64()) == (2, n, 1)
    out["rounds"], out["round_polys"] = [], []
    for _ in range(u64()):
        start = o
        skip_exts(4)
        polys = []
        for _ in range(u64()):
            p0 = o
            skip_exts(u64())
            polys.append(blob[p0:o])
        skip_exts(1)
        skip_exts(u64())
        skip_exts(1)
        out["rounds"].append(blob[start:o])
        out["round_polys"].append(polys)
    out["openings"] = blob[o:len(blob) - 4]
    out["witness"] = struct.unpack_from("<I", blob, len(blob) - 4)[0]
    return out


def first_difference(got, want):
    """Where two proofs first differ, for a failure message: the circuit output, a layer and its sumcheck round, or the openings."""
    if got == want:
        return None
    try:
        g, w = decode_proof(got), decode_proof(want)
    except (struct.error, ValueError, AssertionError):
        return "the proof does not parse (%d bytes, %d expected)" % (len(got), len(want))
    for key in ("numerator", "denominator"):
        if g[key].shape != w[key].shape:
            return "circuit output: %d %ss, %d expected" % (len(g[key]), key, len(w[key]))
        bad = np.nonzero((g[key] != w[key]).any(axis=1))[0]
        if len(bad):
            return "circuit output: %s %d (interaction %d, half %d), %d entries differ" % (key, bad[0], bad[0] // 2, bad[0] % 2, len(bad))
    if len(g["rounds"]) != len(w["rounds"]):
        return "%d layers, %d expected" % (len(g["rounds"]), len(w["rounds"]))
    for layer, (a, b) in enumerate(zip(g["rounds"], w["rounds"])):
        if a != b:
            pa, pb = g["round_polys"][layer], w["round_polys"][layer]
            rnd = next((r for r, (x, y) in enumerate(zip(pa, pb)) if x != y), None)
            where = "sumcheck round %d of %d" % (rnd, len(pb)) if rnd is not None else "outside the round polynomials"
            return "layer %d of %d: %s" % (layer + 1, len(w["rounds"]), where)
    if g["openings"] != w["openings"]:
        return "the openings"
    return "the grinding witness"


# ---- a model of the first layer and the fraction tree in Python integers -----------------------------------------------------------
def _log2_ceil(n):
    return max(n - 1, 0).bit_length()


def _partial_lagrange(point):
    """eq(point, i) for every i, the first coordinate the most significant bit."""
    ev = [kb_py.ext_from_base(1)]
    for x in point:
        nxt = []
        for e in ev:
            prod = kb_py.ext_mul(e, x)
            nxt += [kb_py.ext_sub(e, prod), prod]
        ev = nxt
    return ev


def circuit_output_model(chips, L, challenger, witness):
    """The circuit output of LogUp-GKR (2 * 2^niv numerators and denominators, canonical 4-lists) from the definition, in Python
    integers: no constant is folded, no row is skipped, nothing is shared with the oracle or the device code.

    `challenger`: a kb_py.Challenger at the state LogUp-GKR starts from. The head of the transcript is replayed: the 12-bit
    grind (the proof's `witness` is checked, not searched for), alpha, log2_ceil(max arity) beta seeds, one sample that the
    shard's public values would use, the betas as the partial Lagrange basis of the seeds. Then every interaction's
    (+-multiplicity, alpha + beta_0 kind + sum beta_(1+j) value_j) on every row by VCol.apply, (0, 1) on padding rows, and adjacent
    rows combined pairwise as (n_a d_b + n_b d_a, d_a d_b) until two rows are left. Entry 2 i + r is row r of interaction i."""
    assert challenger.check_witness(GRINDING_BITS, witness), "the grinding witness does not open the transcript"
    alpha = challenger.sample_ext()
    arity = max(len(values) + 1 for prog, _, _ in chips for _, values, _ in prog.sends + prog.receives)
    seeds = [challenger.sample_ext() for _ in range(_log2_ceil(arity))]
    challenger.sample_ext()
    betas = _partial_lagrange(seeds)
    mul, add = kb_py.ext_mul, kb_py.ext_add
    zero, one = kb_py.ext_from_base(0), kb_py.ext_from_base(1)
    fractions = []
    for prog, main, prep in chips:
        main_c = orc.from_monty(main).tolist()
        prep_c = orc.from_monty(prep).tolist() if prep is not None else [None] * len(main_c)
        for sign, lst in ((1, prog.sends), (-1, prog.receives)):
            for kind, values, mult in lst:
                rows = []
                for r in range(1 << L):
                    if r >= len(main_c):
                        rows.append((zero, one))
                        continue
                    d = add(alpha, kb_py.ext_scale(betas[0], kind))
                    for j, v in enumerate(values):
                        d = add(d, kb_py.ext_scale(betas[1 + j], v.apply(prep_c[r], main_c[r])))
                    rows.append((kb_py.ext_from_base(sign * mult.apply(prep_c[r], main_c[r])), d))
                while len(rows) > 2:
                    rows = [(add(mul(na, db), mul(nb, da)), mul(da, db)) for (na, da), (nb, db) in zip(rows[0::2], rows[1::2])]
                fractions.append(rows)
    fractions += [[(zero, one), (zero, one)]] * ((1 << _log2_ceil(len(fractions))) - len(fractions))
    numerator = [f[r][0] for f in fractions for r in range(2)]
    denominator = [f[r][1] for f in fractions for r in range(2)]
    return numerator, denominator
