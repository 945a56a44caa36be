"""Pure-Python jagged PCS — commit wrap, prover and verifier — generic in the hash (TEST INFRASTRUCTURE ONLY).

Restates `JaggedProver::commit_multilinears` / `prove_trusted_evaluations` (/root/reference/slop/crates/jagged/src/prover.rs:
L106-L328), `StackedPcsProver::commit_multilinears` (stacked/src/prover.rs:L59-L94) and `JaggedPcsVerifier::
verify_trusted_evaluations` (jagged/src/verifier.rs:L109-L383 with stacked/src/verifier.rs:L39-L99) over CANONICAL ints, on
top of tests/outer_basefold_model.py: its `Config` (INNER: KoalaBear Poseidon2, OUTER: Poseidon2-BN254 and the
MultiField32Challenger), `CommittedRound`, `basefold_prove` and `basefold_verify`.

The protocol logic here is hash-free and is pinned twice: the INNER instance gives the C++ oracle's bytes (which are pinned on
the reference's real inner proof), and the OUTER verifier accepts the reference's real wrap proof
(tests/test_outer_jagged_model.py). The partial jagged table and the boolean branching-program evaluation come from the oracle
(pyoracle.partial_jagged_table / full_jagged_eval); the branching program at a non-boolean prefix-sum point, which the
jagged-eval sumcheck needs, is restated below as a product of 4x4 transfer matrices.

Variable order of the jagged-eval sumcheck: the point is (bits of t_c, bits of t_{c+1}), each most significant first, and
the sumcheck binds the LAST variable first, as every sumcheck of the reference does."""
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import kb_py as kb  # noqa: E402
import outer_basefold_model as BM  # noqa: E402
from outer_basefold_model import _observe_ext, _sample_ext, partial_lagrange, eval_ext_mle  # noqa: E402

P = kb.P
ZERO, ONE = [0, 0, 0, 0], [1, 0, 0, 0]


def log2_ceil(x):
    return max(int(x) - 1, 0).bit_length()


# ------------------------------------------------------------------------------------------------ commit
def jagged_counts(shapes, max_log_row_count, lsh):
    """shapes: (rows, cols) of every table. Returns (rows, cols) with the two padding tables appended, the padded area and the
    number of padding columns."""
    rows, cols = [int(r) for r, _ in shapes], [int(c) for _, c in shapes]
    area = sum(r * c for r, c in zip(rows, cols))
    H, M = 1 << lsh, 1 << max_log_row_count
    padded = max(-(-area // H) * H, H)
    added = padded - area
    added_cols = max(-(-added // M), 1)
    return rows + [M, added - (added_cols - 1) * M], cols + [added_cols - 1, 1], padded, added_cols


def jagged_wrap(cfg, stacked_commit, rows, cols):
    """compress(stacked commitment, hash([n, rows.., cols..])): rows / cols with the padding tables."""
    return cfg.compress(stacked_commit, cfg.hash_row([len(rows)] + list(rows) + list(cols)))


class StackedRound:
    """StackedPcsProver::commit_multilinears: tables = row-major lists / arrays of canonical ints."""

    def __init__(self, cfg, tables, lsh, batch_size, log_blowup):
        self.cfg, self.lsh = cfg, lsh
        dense = []
        for t in tables:
            t = [[int(x) for x in row] for row in t]
            if t and t[0]:
                for c in range(len(t[0])):
                    dense += [row[c] for row in t]
        H = 1 << lsh
        self.area = len(dense)
        assert self.area > 0, "the outer commitment of no data is refused by the library; not modelled"
        self.padded = -(-self.area // H) * H
        self.num_added_vals = self.padded - self.area
        self.dense = dense + [0] * self.num_added_vals
        self.columns = [self.dense[k * H:(k + 1) * H] for k in range(self.padded // H)]
        mles = []
        for c0 in range(0, len(self.columns), batch_size):
            cs = self.columns[c0:c0 + batch_size]
            mles.append([[c[i] for c in cs] for i in range(H)])
        self.pcs = BM.CommittedRound(cfg, mles, log_blowup)
        self.stacked_commit = self.pcs.commit


class JaggedRound(StackedRound):
    """JaggedProver::commit_multilinears: zero-row tables are counted, not committed."""

    def __init__(self, cfg, tables, max_log_row_count, lsh, batch_size, log_blowup):
        shapes = [(len(t), len(t[0]) if len(t) else int(getattr(t, "shape", (0, 0))[1])) for t in tables]
        super().__init__(cfg, [t for t in tables if len(t)], lsh, batch_size, log_blowup)
        self.max_log_row_count = max_log_row_count
        self.rows, self.cols, padded, self.padding_column_count = jagged_counts(shapes, max_log_row_count, lsh)
        assert padded == self.padded
        self.commit = jagged_wrap(cfg, self.stacked_commit, self.rows, self.cols)


# ------------------------------------------------------------------------------------------------ branching program
def _layer_matrices(z_row, z_index, D):
    """mats[layer][2 cb + nb] = sparse 4x4 {(m, m'): ext}: state m = carry + 2 * comparison (poly.rs:L120-L160)."""
    def lsb(p, i):
        return ZERO if len(p) <= i else p[len(p) - 1 - i]
    out = []
    for layer in range(D):
        zr, zi = lsb(z_row, layer), lsb(z_index, layer)
        er, ei = [kb.ext_sub(ONE, zr), zr], [kb.ext_sub(ONE, zi), zi]
        per = []
        for cb in range(2):
            for nb in range(2):
                mat = {}
                for m in range(4):
                    carry, cmp_ = m & 1, m >> 1
                    for rb in range(2):
                        for ib in range(2):
                            s = rb + carry + cb
                            if ib != (s & 1):
                                continue
                            new_cmp = cmp_ if ib == nb else nb
                            key = (m, (s >> 1) + 2 * new_cmp)
                            mat[key] = kb.ext_add(mat.get(key, ZERO), kb.ext_mul(er[rb], ei[ib]))
                per.append(mat)
        out.append(per)
    return out


def _interp_matrix(per, cb, nb):
    """The layer matrix at extension-valued (cb, nb): multilinear in both."""
    wc, wn = [kb.ext_sub(ONE, cb), cb], [kb.ext_sub(ONE, nb), nb]
    mat = {}
    for c in range(2):
        for n in range(2):
            w = kb.ext_mul(wc[c], wn[n])
            if not any(w):
                continue
            for key, v in per[2 * c + n].items():
                mat[key] = kb.ext_add(mat.get(key, ZERO), kb.ext_mul(w, v))
    return mat


def branching_program_eval(mats, curr_le, next_le):
    """e_initial^T prod_layers M_layer(curr bit, next bit) e_success; bits least significant first, ints 0/1 or ext."""
    vec = {0: ONE}
    for layer, per in enumerate(mats):
        cb, nb = curr_le[layer], next_le[layer]
        mat = per[2 * cb + nb] if isinstance(cb, int) and isinstance(nb, int) else \
            _interp_matrix(per, kb.ext_from_base(cb) if isinstance(cb, int) else cb, kb.ext_from_base(nb) if isinstance(nb, int) else nb)
        nxt = {}
        for (m, m2), v in mat.items():
            if m in vec:
                nxt[m2] = kb.ext_add(nxt.get(m2, ZERO), kb.ext_mul(vec[m], v))
        vec = nxt
    return vec.get(2, ZERO)          # success = {carry 0, comparison 1}


# ------------------------------------------------------------------------------------------------ sumchecks
def _poly_eval(c, x):
    return kb.ext_add(kb.ext_mul(kb.ext_add(kb.ext_mul(c[2], x), c[1]), x), c[0])


def _enc_sumcheck(sc):
    out = [struct.pack("<Q", len(sc["polys"]))]
    for p in sc["polys"]:
        out.append(struct.pack("<Q12I", 3, *[w for c in p for w in c]))
    out.append(struct.pack("<4I", *sc["claimed_sum"]))
    out.append(struct.pack("<Q", len(sc["point"])))
    for e in sc["point"]:
        out.append(struct.pack("<4I", *e))
    out.append(struct.pack("<4I", *sc["eval"]))
    return b"".join(out)


def _round(ch, polys, alphas, y0, y1, y2):
    """Degree-2 round polynomial through y(0), y(1), y(2) -> coefficients; observe, sample."""
    inv2 = kb.ext_from_base(pow(2, P - 2, P))
    c2 = kb.ext_mul(kb.ext_add(kb.ext_sub(y2, kb.ext_add(y1, y1)), y0), inv2)
    poly = [y0, kb.ext_sub(kb.ext_sub(y1, y0), c2), c2]
    polys.append(poly)
    for c in poly:
        _observe_ext(ch, c)
    alpha = _sample_ext(ch)
    alphas.append(alpha)
    return _poly_eval(poly, alpha)


def hadamard_sumcheck(q, j, claim, ch):
    """sum_x q(x) j(x) over ext tables of 2^n entries, binding the last variable (the index's low bit) first."""
    q, j = [list(e) for e in q], [list(e) for e in j]
    two = kb.ext_from_base(2)
    polys, alphas, claimed = [], [], claim
    while len(q) > 1:
        y0, y2 = ZERO, ZERO
        for i in range(0, len(q), 2):
            y0 = kb.ext_add(y0, kb.ext_mul(q[i], j[i]))
            q2 = kb.ext_sub(kb.ext_mul(two, q[i + 1]), q[i])
            j2 = kb.ext_sub(kb.ext_mul(two, j[i + 1]), j[i])
            y2 = kb.ext_add(y2, kb.ext_mul(q2, j2))
        claim = _round(ch, polys, alphas, y0, kb.ext_sub(claim, y0), y2)
        a = alphas[-1]
        q = [kb.ext_add(q[i], kb.ext_mul(a, kb.ext_sub(q[i + 1], q[i]))) for i in range(0, len(q), 2)]
        j = [kb.ext_add(j[i], kb.ext_mul(a, kb.ext_sub(j[i + 1], j[i]))) for i in range(0, len(j), 2)]
    return dict(polys=polys, claimed_sum=claimed, point=alphas[::-1], eval=claim), q[0], j[0]


def _bits_be(x, n):
    return [(x >> (n - 1 - i)) & 1 for i in range(n)]


def jagged_eval_prove(prefix, log_m, z_row, z_col, z_trace, ch):
    D = log_m + 1
    col_eq = partial_lagrange(z_col)
    mats = _layer_matrices(z_row, z_trace, D)
    cols = [(_bits_be(prefix[c], D) + _bits_be(prefix[c + 1], D), col_eq[c]) for c in range(len(prefix) - 1)]
    claimed = ZERO
    for bits, w in cols:
        claimed = kb.ext_add(claimed, kb.ext_mul(w, branching_program_eval(mats, bits[:D][::-1], bits[D:][::-1])))
    _observe_ext(ch, claimed)
    claim, polys, alphas = claimed, [], []
    bound = []                                   # challenges of variables v + 1 .. 2D - 1, in variable order
    weights = [w for _, w in cols]               # zcol_c * eq(bound, bits of c at the bound variables)
    two, minus1 = kb.ext_from_base(2), kb.ext_from_base(P - 1)
    for v in range(2 * D - 1, -1, -1):
        y0, y2 = ZERO, ZERO
        for (bits, _), w in zip(cols, weights):
            if not any(w):
                continue
            for X, acc in ((0, 0), (2, 1)):
                eqx = (ONE if bits[v] == 0 else ZERO) if X == 0 else (minus1 if bits[v] == 0 else two)
                if not any(eqx):
                    continue
                pt = bits[:v] + [X if X == 0 else two] + bound
                bp = branching_program_eval(mats, pt[:D][::-1], pt[D:][::-1])
                term = kb.ext_mul(kb.ext_mul(w, eqx), bp)
                if acc == 0:
                    y0 = kb.ext_add(y0, term)
                else:
                    y2 = kb.ext_add(y2, term)
        claim = _round(ch, polys, alphas, y0, kb.ext_sub(claim, y0), y2)
        a = alphas[-1]
        bound = [a] + bound
        na = kb.ext_sub(ONE, a)
        weights = [kb.ext_mul(w, a if bits[v] else na) for (bits, _), w in zip(cols, weights)]
    return dict(polys=polys, claimed_sum=claimed, point=alphas[::-1], eval=claim)


def _verify_sumcheck(sc, ch, n_vars):
    """partially_verify_sumcheck for degree 2. Returns None or the failing check's name."""
    if len(sc["polys"]) != n_vars or len(sc["point"]) != n_vars or n_vars == 0:
        return "SumcheckShape"
    claim = sc["claimed_sum"]
    for k, poly in enumerate(sc["polys"]):
        if len(poly) != 3:
            return "SumcheckDegree"
        for c in poly:
            _observe_ext(ch, c)
        alpha = _sample_ext(ch)
        if alpha != sc["point"][n_vars - 1 - k]:
            return "SumcheckPoint"
        if kb.ext_add(poly[0], _poly_eval(poly, ONE)) != claim:
            return "SumcheckRound"
        claim = _poly_eval(poly, alpha)
    return None if claim == sc["eval"] else "SumcheckEval"


# ------------------------------------------------------------------------------------------------ prover
def _column_heights(rounds_counts):
    return [r for rows, cols in rounds_counts for r, c in zip(rows, cols) for _ in range(c)]


def _oracle_ext(points):
    import pyoracle as orc
    import numpy as np
    return orc.to_monty(np.array(points, dtype=np.uint32).reshape(-1, 4))


def jagged_prove(cfg, z_row, claims_per_round, rounds, ch, log_blowup, num_queries, pow_bits):
    """rounds: JaggedRound list; claims_per_round[r]: ext evaluations at z_row of round r's columns; ch: a challenger of cfg,
    advanced in place. Returns bincode(JaggedPcsProof)."""
    import numpy as np
    import pyoracle as orc
    z_row = [list(map(int, e)) for e in z_row]
    L, lsh = len(z_row), rounds[0].lsh
    heights = _column_heights([(r.rows, r.cols) for r in rounds])
    z_col = [_sample_ext(ch) for _ in range(log2_ceil(len(heights)))]
    column_claims = []
    for r, cl in zip(rounds, claims_per_round):
        column_claims += [list(map(int, e)) for e in cl] + [ZERO] * r.padding_column_count
    assert len(column_claims) == len(heights)
    claim = eval_ext_mle(column_claims, z_col)
    total = sum(r.padded for r in rounds)
    assert total == sum(heights)
    log_m = log2_ceil(total)
    q = [kb.ext_from_base(x) for r in rounds for x in r.dense] + [ZERO] * ((1 << log_m) - total)
    jt = orc.from_monty(orc.partial_jagged_table(heights, L, _oracle_ext(z_row), _oracle_ext(z_col) if z_col else np.zeros((0, 4), np.uint32)))
    sumcheck, q_eval, _ = hadamard_sumcheck(q, [[int(x) for x in e] for e in jt], claim, ch)
    final_point = sumcheck["point"]
    prefix = [0]
    for h in heights:
        prefix.append(prefix[-1] + h)
    jagged_eval = jagged_eval_prove(prefix, log_m, z_row, z_col, final_point, ch)
    _observe_ext(ch, q_eval)
    stack_point = final_point[len(final_point) - lsh:]
    eq = partial_lagrange(stack_point)
    batch_evals = []
    for r in rounds:
        evs = []
        for col in r.columns:
            acc = ZERO
            for e, v in zip(eq, col):
                if v:
                    acc = kb.ext_add(acc, kb.ext_scale(e, v))
            evs.append(acc)
        batch_evals.append(evs)
    flat = [e for evs in batch_evals for e in evs]
    for e in flat:
        _observe_ext(ch, e)
    out = [BM.basefold_prove(cfg, stack_point, [r.pcs for r in rounds], flat, ch, log_blowup, num_queries, pow_bits)]
    out.append(struct.pack("<Q", len(rounds)))
    for evs in batch_evals:
        out.append(struct.pack("<Q", len(evs)) + b"".join(struct.pack("<4I", *e) for e in evs) + struct.pack("<QQ", 1, len(evs)))
    out.append(_enc_sumcheck(sumcheck))
    out.append(_enc_sumcheck(jagged_eval))
    out.append(struct.pack("<Q", len(rounds)))
    for r in rounds:
        out.append(struct.pack("<Q", len(r.rows)) + b"".join(struct.pack("<QQ", a, b) for a, b in zip(r.rows, r.cols)))
    out.append(struct.pack("<Q", len(rounds)))
    for r in rounds:
        out.append(cfg.enc_digest(r.stacked_commit))
    out.append(struct.pack("<4IQQ", *q_eval, L, log_m))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ parser / verifier
def parse_jagged_tail(cfg, blob, o):
    """Everything of bincode(JaggedPcsProof) behind the BaseFold proof, from offset o."""
    r = BM._R(blob)
    r.o = o

    def sumcheck():
        polys = []
        for _ in range(r.u64()):
            if r.u64() != 3:
                raise ValueError("sumcheck degree")
            v = r.felts(12)
            polys.append([v[0:4], v[4:8], v[8:12]])
        claimed = r.felts(4)
        point = [r.felts(4) for _ in range(r.u64())]
        return dict(polys=polys, claimed_sum=claimed, point=point, eval=r.felts(4))

    batch = []
    for _ in range(r.u64()):
        n = r.u64()
        evs = [r.felts(4) for _ in range(n)]
        if [r.u64(), r.u64()] != [1, n]:
            raise ValueError("batch evaluation dims")
        batch.append(evs)
    sc, je = sumcheck(), sumcheck()
    counts = [[(r.u64(), r.u64()) for _ in range(r.u64())] for _ in range(r.u64())]
    commits = []
    for _ in range(r.u64()):
        d, r.o = cfg.dec_digest(r.b, r.o)
        commits.append(d)
    expected_eval = r.felts(4)
    L, log_m = r.u64(), r.u64()
    if r.o != len(r.b):
        raise ValueError("trailing bytes")
    return dict(batch_evaluations=batch, sumcheck=sc, jagged_eval=je, counts=counts, merkle_tree_commitments=commits,
                expected_eval=expected_eval, max_log_row_count=L, log_m=log_m)


def basefold_length(cfg, blob):
    """Length of the BaseFold proof at the head of a JaggedPcsProof (walks its openings)."""
    r = BM._R(blob)
    n = r.u64()
    r.o += 32 * n
    n = r.u64()
    r.o += cfg.digest_size * n
    for _ in range(2):
        for _ in range(r.u64()):
            BM._read_opening(cfg, r)
    return r.o + 16 + 8


def parse_proof(cfg, blob):
    n = basefold_length(cfg, blob)
    p = parse_jagged_tail(cfg, blob, n)
    p["basefold"] = bytes(blob[:n])
    return p


def jagged_verify_fields(cfg, commitments, z_row, claims_per_round, p, lsh, ch, log_blowup, num_queries, pow_bits):
    """JaggedPcsVerifier::verify_trusted_evaluations on a parsed proof p (parse_proof's dict; p["basefold"] the BaseFold bytes,
    which may carry fewer than the configured queries when num_queries says so). commitments[r]: the JAGGED commitment of
    round r. Returns "ok" or the name of the failing check. ch is advanced in place."""
    z_row = [list(map(int, e)) for e in z_row]
    counts = p["counts"]
    if any(len(c) < 2 for c in counts) or not counts:
        return "Shape"
    rows = [[a for a, _ in c] for c in counts]
    cols = [[b for _, b in c] for c in counts]
    heights = _column_heights(list(zip(rows, cols)))
    prefix = [0]
    for h in heights:
        prefix.append(prefix[-1] + h)
    if p["max_log_row_count"] != len(z_row) or p["log_m"] != log2_ceil(prefix[-1]) or p["log_m"] >= 30:
        return "Shape"
    L, log_m, nr = len(z_row), p["log_m"], len(commitments)
    z_col = [_sample_ext(ch) for _ in range(log2_ceil(len(heights)))]
    if len(claims_per_round) != nr or len(counts) != nr or len(p["merkle_tree_commitments"]) != nr or len(p["batch_evaluations"]) != nr:
        return "Shape"
    H, M = 1 << lsh, 1 << L
    column_claims, areas = [], []
    for r in range(nr):
        if len(claims_per_round[r]) != sum(cols[r][:-2]):
            return "ClaimCount"
        if jagged_wrap(cfg, p["merkle_tree_commitments"][r], rows[r], cols[r]) != commitments[r]:
            return "CommitmentWrap"
        area = sum(a * b for a, b in zip(rows[r][:-2], cols[r][:-2]))
        if area == 0 or area >= 1 << 30 or any(a > M for a in rows[r]):
            return "Area"
        erows, ecols, padded, added_cols = jagged_counts(list(zip(rows[r][:-2], cols[r][:-2])), L, lsh)
        if erows[-2:] != rows[r][-2:] or ecols[-2:] != cols[r][-2:]:
            return "PaddingTables"
        areas.append(padded)
        column_claims += [list(map(int, e)) for e in claims_per_round[r]] + [ZERO] * added_cols
    if len(column_claims) != len(heights):
        return "Shape"
    if eval_ext_mle(column_claims, z_col) != p["sumcheck"]["claimed_sum"]:
        return "ColumnClaims"
    bad = _verify_sumcheck(p["sumcheck"], ch, log_m)
    if bad:
        return "Jagged" + bad
    point = p["sumcheck"]["point"]
    # jagged-eval
    je = p["jagged_eval"]
    _observe_ext(ch, je["claimed_sum"])
    D = log_m + 1
    bad = _verify_sumcheck(je, ch, 2 * D)
    if bad:
        return "JaggedEval" + bad
    col_eq = partial_lagrange(z_col)
    acc, memo = ZERO, {}
    for c in range(len(heights)):
        key = (prefix[c], prefix[c + 1])
        if key not in memo:
            fe = ONE
            for b, x in zip(_bits_be(key[0], D) + _bits_be(key[1], D), je["point"]):
                fe = kb.ext_mul(fe, x if b else kb.ext_sub(ONE, x))
            memo[key] = fe
        acc = kb.ext_add(acc, kb.ext_mul(col_eq[c], memo[key]))
    mats = _layer_matrices(z_row, point, D)
    bp = branching_program_eval(mats, je["point"][:D][::-1], je["point"][D:][::-1])
    if kb.ext_mul(acc, bp) != je["eval"]:
        return "JaggedEvalBranchingProgram"
    if kb.ext_mul(p["expected_eval"], je["claimed_sum"]) != p["sumcheck"]["eval"]:
        return "ExpectedEval"
    # stacked verify_untrusted_evaluation
    _observe_ext(ch, p["expected_eval"])
    if len(point) < lsh:
        return "Shape"
    batch_point, stack_point = point[:len(point) - lsh], point[len(point) - lsh:]
    flat = []
    for r in range(nr):
        if areas[r] // H != len(p["batch_evaluations"][r]):
            return "BatchShape"
        flat += p["batch_evaluations"][r]
    if len(flat) > 1 << len(batch_point):
        return "BatchShape"
    if eval_ext_mle(flat, batch_point) != p["expected_eval"]:
        return "BatchEvaluations"
    for e in flat:
        _observe_ext(ch, e)
    res = BM.basefold_verify(cfg, p["merkle_tree_commitments"], stack_point, p["batch_evaluations"], p["basefold"], ch, log_blowup,
                             num_queries, pow_bits)
    return "ok" if res == "ok" else "Basefold" + res


def jagged_verify(cfg, commitments, z_row, claims_per_round, blob, lsh, ch, log_blowup, num_queries, pow_bits):
    try:
        p = parse_proof(cfg, blob)
    except (ValueError, struct.error) as e:
        return "Parse: %s" % e
    return jagged_verify_fields(cfg, commitments, z_row, claims_per_round, p, lsh, ch, log_blowup, num_queries, pow_bits)
