"""Pure-Python BaseFold prover and verifier, generic in the hash (TEST INFRASTRUCTURE ONLY).

Restates `BasefoldProver::commit_mles` / `prove_trusted_mle_evaluations`
(/root/reference/slop/crates/basefold-prover/src/prover.rs:L78-L243, fri.rs:L31-L129) and
`BasefoldVerifier::verify_mle_evaluations` (/root/reference/slop/crates/basefold/src/verifier.rs:L122-L430) over CANONICAL
ints, parameterised on a `Config`: (hash_row, compress, challenger, digest encoding). Two instances:

  INNER  kb_py.hash_felts / kb_py.compress / kb_py.Challenger, a digest = 8 KoalaBear words (32 bytes);
  OUTER  outer_model.hash_row / compress / Challenger (digests observed through observe_commitment), a digest = one BN254
         value, bincoded as u64(32) + its 32 little-endian bytes (40 bytes: serde of Hash<KoalaBear, Bn254Fr, 1>).

Field, extension and fold arithmetic are oracle/kb_py.py's. Grinds return the SMALLEST witness, as the library does. A zero
last coordinate of the evaluation point: the library's extension inverse maps 0 to 0 (Fermat), so one_val = zero_val; the
model does the same (`ext_inv0`).

Everything runs in the calling process (no worker processes: the GPU tests call this with the device open). About 0.1-0.35 ms
per outer permutation, so a tree of 2^15 leaves is several seconds."""
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import kb_py as kb  # noqa: E402
import outer_model as M  # noqa: E402

P = kb.P
BATCH_GRINDING_BITS = 5


# ------------------------------------------------------------------------------------------------ configurations
class _InnerChallenger:
    def __init__(self, ch=None):
        self.ch = ch if ch is not None else kb.Challenger()

    def clone(self):
        c = kb.Challenger()
        c.state, c.inp, c.out = list(self.ch.state), list(self.ch.inp), list(self.ch.out)
        return _InnerChallenger(c)

    def observe(self, x):
        self.ch.observe(x)

    def observe_digest(self, d):
        self.ch.observe_many(d)

    def sample(self):
        return self.ch.sample()

    def sample_bits(self, bits):
        return self.ch.sample_bits(bits)


class _OuterChallenger:
    """tests/outer_model.py's Challenger speaks Montgomery KoalaBear words; this adapter speaks canonical ones."""

    def __init__(self, ch=None):
        self.ch = ch if ch is not None else M.Challenger()

    def clone(self):
        return _OuterChallenger(self.ch.clone())

    def observe(self, x):
        self.ch.observe(M.kb_to_monty(x))

    def observe_digest(self, d):
        self.ch.observe_commitment(d)

    def sample(self):
        return M.kb_from_monty(self.ch.sample())

    def sample_bits(self, bits):
        return self.ch.sample_bits(bits)


def _observe_ext(ch, e):
    for x in e:
        ch.observe(x)


def _sample_ext(ch):
    return [ch.sample() for _ in range(4)]


def _check_witness(ch, bits, w):
    ch.observe(w)
    return ch.sample_bits(bits) == 0


def _grind(ch, bits):
    for w in range(P):
        if _check_witness(ch.clone(), bits, w):
            assert _check_witness(ch, bits, w)
            return w
    raise AssertionError("no witness")


class Config:
    def __init__(self, name, hash_row, compress, challenger, digest_size, enc, dec):
        self.name, self.hash_row, self.compress, self.challenger = name, hash_row, compress, challenger
        self.digest_size, self.enc_digest, self.dec_digest = digest_size, enc, dec

    def commitment(self, root, lg_height, width):
        return self.compress(root, self.hash_row([lg_height, width]))


def _enc_inner(d):
    return struct.pack("<8I", *d)


def _dec_inner(b, o):
    d = list(struct.unpack_from("<8I", b, o))
    if any(x >= P for x in d):
        raise ValueError("non-canonical digest word")
    return d, o + 32


def _enc_outer(d):
    return struct.pack("<Q", 32) + int(d).to_bytes(32, "little")


def _dec_outer(b, o):
    if struct.unpack_from("<Q", b, o)[0] != 32:
        raise ValueError("digest length prefix")
    d = int.from_bytes(b[o + 8:o + 40], "little")
    if d >= M.P:
        raise ValueError("non-canonical digest")
    return d, o + 40


INNER = Config("inner", lambda row: kb.hash_felts(list(row)), lambda l, r: kb.compress(l, r), _InnerChallenger, 32,
               _enc_inner, _dec_inner)
OUTER = Config("outer", lambda row: M.hash_row(list(row)), M.compress, _OuterChallenger, 40, _enc_outer, _dec_outer)


# ------------------------------------------------------------------------------------------------ trees
class Tree:
    def __init__(self, cfg, rows, width):
        """rows: list of rows (lists of canonical ints), a power of two of them."""
        self.cfg, self.width = cfg, width
        self.lg = len(rows).bit_length() - 1
        assert len(rows) == 1 << self.lg
        self.layers = [[cfg.hash_row(r) for r in rows]]
        while len(self.layers[-1]) > 1:
            cur = self.layers[-1]
            self.layers.append([cfg.compress(cur[2 * k], cur[2 * k + 1]) for k in range(len(cur) // 2)])
        self.root = self.layers[-1][0]
        self.commit = cfg.commitment(self.root, self.lg, width)

    def paths(self, idx):
        return [[self.layers[k][(i >> k) ^ 1] for k in range(self.lg)] for i in idx]


# ------------------------------------------------------------------------------------------------ field helpers
def ext_inv0(a):
    return [0, 0, 0, 0] if not any(a) else kb.ext_inv(a)


def partial_lagrange(point):
    ev = [kb.ext_from_base(1)]
    for x in point:
        nx = []
        for e in ev:
            prod = kb.ext_mul(e, x)
            nx += [kb.ext_sub(e, prod), prod]
        ev = nx
    return ev


def rs_encode_columns(cols, log_blowup):
    """cols: list of columns (each 2^n canonical ints) -> their codewords: zero-pad to N = 2^(n + log_blowup), radix-2
    decimation in frequency, natural order in, bit-reversed order out (FriCpuProver / Dft of the reference)."""
    n = len(cols[0])
    N = n << log_blowup
    lg = N.bit_length() - 1
    g = kb.two_adic_generator(lg)
    tw = [1] * max(N // 2, 1)
    for i in range(1, N // 2):
        tw[i] = tw[i - 1] * g % P
    out = []
    for col in cols:
        a = [int(x) for x in col] + [0] * (N - n)
        for s in range(lg, 0, -1):
            half, stride = 1 << (s - 1), N >> s
            for blk in range(0, N, 2 * half):
                for j in range(half):
                    x, y = a[blk + j], a[blk + half + j]
                    a[blk + j] = (x + y) % P
                    a[blk + half + j] = (x - y) * tw[j * stride] % P
        out.append(a)
    return out


def fold_even_odd(cw, beta):
    N = len(cw)
    lg = N.bit_length() - 1
    g = kb.two_adic_generator(lg)
    out = []
    for i in range(N // 2):
        x = pow(g, kb.reverse_bits_len(2 * i, lg), P)
        out.append(kb.fold_query(cw[2 * i], cw[2 * i + 1], beta, x))
    return out


def eval_ext_mle(vals, point):
    eq = partial_lagrange(point)
    acc = [0, 0, 0, 0]
    for e, v in zip(eq, vals):
        acc = kb.ext_add(acc, kb.ext_mul(e, v))
    return acc


def eval_mle_columns(mle, point):
    """mle: rows of canonical ints -> one extension evaluation per column."""
    eq = partial_lagrange(point)
    w = len(mle[0])
    acc = [[0, 0, 0, 0] for _ in range(w)]
    for e, row in zip(eq, mle):
        for c in range(w):
            acc[c] = kb.ext_add(acc[c], kb.ext_scale(e, int(row[c])))
    return acc


# ------------------------------------------------------------------------------------------------ prover
class CommittedRound:
    """BasefoldProver::commit_mles: mles = list of tables (rows of canonical ints, all 2^n rows)."""

    def __init__(self, cfg, mles, log_blowup):
        self.cfg, self.log_blowup = cfg, log_blowup
        self.mles = [[[int(x) for x in row] for row in m] for m in mles]
        n = len(self.mles[0])
        self.log_n = n.bit_length() - 1
        self.width = sum(len(m[0]) for m in self.mles)
        cols = [[row[c] for row in m] for m in self.mles for c in range(len(m[0]))]
        cw = rs_encode_columns(cols, log_blowup)
        self.rows = [[cw[c][i] for c in range(self.width)] for i in range(n << log_blowup)]
        self.tree = Tree(cfg, self.rows, self.width)
        self.commit = self.tree.commit


def _write_opening(cfg, out, values, nq, width, tree, idx):
    out.append(struct.pack("<Q", nq * width))
    out.append(struct.pack("<%dI" % (nq * width), *[x for row in values for x in row]))
    out.append(struct.pack("<QQQ", 2, nq, width))
    out.append(cfg.enc_digest(tree.root))
    out.append(struct.pack("<QQQ", tree.lg, width, nq * tree.lg))
    for path in tree.paths(idx):
        for d in path:
            out.append(cfg.enc_digest(d))
    out.append(struct.pack("<QQQ", 2, nq, tree.lg))


def basefold_prove(cfg, point, rounds, claims, ch, log_blowup, num_queries, pow_bits):
    """point: [dim] ext; rounds: CommittedRound list; claims: flat list of ext, one per committed column; ch: a challenger of
    cfg (advanced in place). Returns the bincode of BasefoldProof."""
    point = [list(map(int, e)) for e in point]
    dim = len(point)
    batch_witness = _grind(ch, BATCH_GRINDING_BITS)
    total = sum(r.width for r in rounds)
    assert total == len(claims)
    coeffs = partial_lagrange([_sample_ext(ch) for _ in range((total - 1).bit_length())])
    n = 1 << dim
    cur_mle = [[0, 0, 0, 0] for _ in range(n)]
    off = 0
    for r in rounds:
        for m in r.mles:
            for i, row in enumerate(m):
                acc = cur_mle[i]
                for c, v in enumerate(row):
                    acc = kb.ext_add(acc, kb.ext_scale(coeffs[off + c], v))
                cur_mle[i] = acc
            off += len(m[0])
    cur_claim = [0, 0, 0, 0]
    for c, k in zip(claims, coeffs):
        cur_claim = kb.ext_add(cur_claim, kb.ext_mul(list(map(int, c)), k))
    cw_cols = rs_encode_columns([[e[k] for e in cur_mle] for k in range(4)], log_blowup)
    cur_cw = [[cw_cols[k][i] for k in range(4)] for i in range(n << log_blowup)]
    ch.observe(dim)
    uni, commits, trees, leaves_per_round = [], [], [], []
    pt = list(point)
    for _ in range(dim):
        last = pt.pop()
        zero_val = eval_ext_mle(cur_mle[0::2], pt)
        one_val = kb.ext_add(kb.ext_mul(kb.ext_sub(cur_claim, zero_val), ext_inv0(last)), zero_val)
        uni.append((zero_val, one_val))
        _observe_ext(ch, zero_val)
        _observe_ext(ch, one_val)
        leaves = [cur_cw[2 * i] + cur_cw[2 * i + 1] for i in range(len(cur_cw) // 2)]
        t = Tree(cfg, leaves, 8)
        ch.observe_digest(t.commit)
        beta = _sample_ext(ch)
        leaves_per_round.append(leaves)
        trees.append(t)
        commits.append(t.commit)
        cur_cw = fold_even_odd(cur_cw, beta)
        cur_mle = [kb.ext_add(cur_mle[2 * i], kb.ext_mul(beta, cur_mle[2 * i + 1])) for i in range(len(cur_mle) // 2)]
        cur_claim = kb.ext_add(zero_val, kb.ext_mul(beta, one_val))
    final_poly = cur_cw[0]
    _observe_ext(ch, final_poly)
    pow_witness = _grind(ch, pow_bits)
    q = [ch.sample_bits(dim + log_blowup) for _ in range(num_queries)]

    out = [struct.pack("<Q", dim)]
    for z, o in uni:
        out.append(struct.pack("<8I", *(z + o)))
    out.append(struct.pack("<Q", dim))
    for c in commits:
        out.append(cfg.enc_digest(c))
    out.append(struct.pack("<Q", len(rounds)))
    for r in rounds:
        _write_opening(cfg, out, [r.rows[i] for i in q], num_queries, r.width, r.tree, q)
    out.append(struct.pack("<Q", dim))
    idx = list(q)
    for k in range(dim):
        idx = [i >> 1 for i in idx]
        _write_opening(cfg, out, [leaves_per_round[k][i] for i in idx], num_queries, 8, trees[k], idx)
    out.append(struct.pack("<4I", *final_poly))
    out.append(struct.pack("<II", pow_witness, batch_witness))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ proof parser / verifier
class _R:
    def __init__(self, b):
        self.b, self.o = bytes(b), 0

    def u64(self):
        if self.o + 8 > len(self.b):
            raise ValueError("truncated")
        v = struct.unpack_from("<Q", self.b, self.o)[0]
        self.o += 8
        return v

    def felts(self, k):
        if self.o + 4 * k > len(self.b):
            raise ValueError("truncated")
        v = list(struct.unpack_from("<%dI" % k, self.b, self.o))
        self.o += 4 * k
        if any(x >= P for x in v):
            raise ValueError("non-canonical field element")
        return v


def _read_opening(cfg, r):
    n = r.u64()
    if n > len(r.b):
        raise ValueError("count")
    vals = r.felts(n)
    dims = [r.u64() for _ in range(3)]
    root, r.o = cfg.dec_digest(r.b, r.o)
    lg_h, width, npath = r.u64(), r.u64(), r.u64()
    if npath > len(r.b):
        raise ValueError("count")
    paths = []
    for _ in range(npath):
        d, r.o = cfg.dec_digest(r.b, r.o)
        paths.append(d)
    pdims = [r.u64() for _ in range(3)]
    if dims[0] != 2 or pdims[0] != 2 or dims[1] * dims[2] != n or pdims[1] * pdims[2] != npath:
        raise ValueError("tensor dims")
    return dict(values=vals, n_idx=dims[1], width=dims[2], root=root, lg_h=lg_h, pwidth=width, paths=paths,
                path_dims=pdims[1:])


def parse_proof(cfg, blob):
    r = _R(blob)
    uni = [(lambda v: (v[:4], v[4:]))(r.felts(8)) for _ in range(r.u64())]
    commits = []
    for _ in range(r.u64()):
        d, r.o = cfg.dec_digest(r.b, r.o)
        commits.append(d)
    comps = [_read_opening(cfg, r) for _ in range(r.u64())]
    folds = [_read_opening(cfg, r) for _ in range(r.u64())]
    final_poly = r.felts(4)
    pow_witness, batch_witness = r.felts(2)
    if r.o != len(r.b):
        raise ValueError("trailing bytes")
    return dict(uni=uni, commits=commits, comps=comps, folds=folds, final_poly=final_poly, pow_witness=pow_witness,
                batch_witness=batch_witness)


def _merkle_verify(cfg, commit, idx, o, expected_width, expected_lg):
    if o["pwidth"] != expected_width or o["lg_h"] != expected_lg or o["width"] != expected_width:
        return False
    if o["path_dims"] != [len(idx), expected_lg] or o["n_idx"] != len(idx):
        return False
    if cfg.commitment(o["root"], expected_lg, expected_width) != commit:
        return False
    w = expected_width
    for q, i in enumerate(idx):
        node = cfg.hash_row(o["values"][q * w:(q + 1) * w])
        for k in range(expected_lg):
            sib = o["paths"][q * expected_lg + k]
            node = cfg.compress(sib, node) if (i >> k) & 1 else cfg.compress(node, sib)
        if node != o["root"]:
            return False
    return True


def basefold_verify(cfg, commitments, point, claims_per_round, blob, ch, log_blowup, num_queries, pow_bits):
    """Returns "ok" or the name of the check that failed (verifier.rs's error variants). ch is advanced in place."""
    try:
        p = parse_proof(cfg, blob)
    except (ValueError, struct.error) as e:
        return "Parse: %s" % e
    if not _check_witness(ch, BATCH_GRINDING_BITS, p["batch_witness"]):
        return "BatchPow"
    total = sum(len(c) for c in claims_per_round)
    coeffs = partial_lagrange([_sample_ext(ch) for _ in range((total - 1).bit_length())])
    eval_claim, k = [0, 0, 0, 0], 0
    for cr in claims_per_round:
        for e in cr:
            eval_claim = kb.ext_add(eval_claim, kb.ext_mul(list(map(int, e)), coeffs[k]))
            k += 1
    if len(claims_per_round) != len(commitments) or len(commitments) != len(p["comps"]):
        return "IncorrectShape"
    n = len(p["commits"])
    if n != len(p["uni"]) or n != len(point) or n == 0:
        return "SumcheckFriLengthMismatch"
    pt = [list(map(int, e)) for e in point][::-1]
    ch.observe(n)
    betas = []
    for i in range(n):
        _observe_ext(ch, p["uni"][i][0])
        _observe_ext(ch, p["uni"][i][1])
        ch.observe_digest(p["commits"][i])
        betas.append(_sample_ext(ch))
    one = kb.ext_from_base(1)
    expected = eval_claim
    for i in range(n):
        z, o = p["uni"][i]
        if expected != kb.ext_add(kb.ext_mul(kb.ext_sub(one, pt[i]), z), kb.ext_mul(pt[i], o)):
            return "Sumcheck"
        expected = kb.ext_add(z, kb.ext_mul(betas[i], o))
    _observe_ext(ch, p["final_poly"])
    if not _check_witness(ch, pow_bits, p["pow_witness"]):
        return "Pow"
    lg_max = n + log_blowup
    if lg_max > kb.TWO_ADICITY:
        return "TwoAdicityOverflow"
    q = [ch.sample_bits(lg_max) for _ in range(num_queries)]
    batch_evals = [[0, 0, 0, 0] for _ in q]
    off = 0
    for r, o in enumerate(p["comps"]):
        w = len(claims_per_round[r])
        if o["n_idx"] != len(q) or o["width"] != w or len(o["values"]) != len(q) * w:
            return "IncorrectShape"
        for j in range(len(q)):
            acc = batch_evals[j]
            for c in range(w):
                acc = kb.ext_add(acc, kb.ext_scale(coeffs[off + c], o["values"][j * w + c]))
            batch_evals[j] = acc
        off += w
    for r, o in enumerate(p["comps"]):
        if not _merkle_verify(cfg, commitments[r], q, o, len(claims_per_round[r]), lg_max):
            return "Tcs"
    if len(p["folds"]) != n:
        return "IncorrectShape"
    g = kb.two_adic_generator(lg_max)
    xis = [pow(g, kb.reverse_bits_len(i, lg_max), P) for i in q]
    folded, idx = batch_evals, list(q)
    for r in range(n):
        o = p["folds"][r]
        if o["n_idx"] != len(idx) or o["width"] != 8 or len(o["values"]) != 8 * len(idx):
            return "IncorrectShape"
        for j in range(len(idx)):
            ev = [o["values"][8 * j:8 * j + 4], o["values"][8 * j + 4:8 * j + 8]]
            if ev[idx[j] & 1] != folded[j]:
                return "QueryValueMismatch"
            x0 = xis[j] if idx[j] & 1 == 0 else (P - xis[j]) % P       # the point of the pair's even entry
            folded[j] = kb.fold_query(ev[0], ev[1], betas[r], x0)
            idx[j] >>= 1
            xis[j] = xis[j] * xis[j] % P
        if not _merkle_verify(cfg, p["commits"][r], idx, o, 8, lg_max - 1 - r):
            return "Tcs"
    if any(f != p["final_poly"] for f in folded):
        return "QueryFinalPolyMismatch"
    z, o = p["uni"][-1]
    if p["final_poly"] != kb.ext_add(z, kb.ext_mul(betas[-1], o)):
        return "SumcheckFinalPolyMismatch"
    return "ok"
