#!/usr/bin/env python3
"""Replay the reference's one real OUTER (BN254) shard proof under the Python model and record it as fixtures.

Sources (read-only, only in the build container):
  /root/reference/crates/prover/wrapped_proof.bin   bincode(ShardProof<SP1OuterGlobalContext>), 1,340,837 bytes, written by the
                                                    reference's wrap prover (crates/prover/src/build.rs:L797-L831)
  /root/reference/crates/prover/wrap_vk.bin         its MachineVerifyingKey, 112 bytes

The whole (vk, ShardProof) pair is parsed (every length and shape field asserted; the layout is the inner proof's of
make_transcript.py with every digest as u64(32) + the 32 little-endian bytes of the canonical Bn254Fr, asserted at every digest)
and the verifier's challenger calls are re-enacted in the order listed in make_transcript.py's docstring, with
tests/outer_model.py's MultiField32Challenger (digests through observe_commitment). Parameters: wrap_fri_config()
(/root/reference/crates/primitives/src/fri_params.rs): log_blowup 3, 22 proof-of-work bits, 94 queries; 12-bit GKR and 5-bit
batch grinds.

Asserted here, and again by tests/test_outer_golden.py on the committed fixtures alone:
  Merkle layer  for the first 12 queries of both component rounds and all 21 fold rounds, hash_row(values) walked up the stored
                path gives the stored root, and compress(root, hash([log_height, width])) equals the commitment the proof carries
                for that tree: the two stacked-PCS commitments inside JaggedPcsProof (of which main_commitment and the vk's
                preprocessed_commit are the jagged wraps: hashes with the row / column counts, not modelled here) and every
                fri_commitments[r]. Pins reduce_31 packing, the sponge's short-last-block rule, compress, the commitment cap.
  Transcript    the 12-bit, 5-bit and 22-bit grinding witnesses pass check_witness; every sumcheck's sampled point equals the
                stored one (20 GKR rounds, zerocheck, jagged sumcheck, jagged eval) and the GKR claim equations hold; the 21
                sampled BaseFold betas satisfy the fold equation on the opened pairs of every kept query down to final_poly;
                the sampled query indices are the ones the Merkle paths verify at. Pins absorb order, duplexing, split_32
                sample order, sample_bits and digest observation.

Output tests/golden/outer_wrap_basefold.npz: basefold_proof_q12 (the reference's own bytes of BasefoldProof restricted to the
first 12 queries, only the per-opening counts rewritten), commits (the two stacked commitments, 32 LE bytes each), point
(stack_point), claims0 / claims1 (the batch evaluations of the two rounds), betas, query_indices, and the challenger at BaseFold
entry (entry_sponge: 3 x 32 LE bytes canonical; entry_inp, entry_out: canonical KoalaBear words) and at the end of the replay.
tests/golden/outer_wrap_transcript.npz: the tape (ops / data as in kb_shrink_transcript.npz, plus opcode 4 OBSERVE_DIGEST whose
data are the digest's 8 LE u32 words) and the final state."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import kb_py as kb  # noqa: E402
import outer_model as M  # noqa: E402
from make_transcript import Reader, eval_mle, full_lagrange_eval  # noqa: E402

DIR = "/root/reference/crates/prover/"
P = kb.P
GKR_GRINDING_BITS, BATCH_GRINDING_BITS, POW_BITS, NUM_QUERIES, LOG_BLOWUP = 12, 5, 22, 94, 3
NQ_KEEP = 12


class OReader(Reader):
    def digest(self):
        assert self.u64() == 32, "digest length prefix: parse is off"
        v = int.from_bytes(self.b[self.o:self.o + 32], "little")
        self.o += 32
        assert v < M.P, "non-canonical digest"
        return v

    def opening(self, nq):
        """MerkleTreeOpeningAndProof with 40-byte digests. Returns (parsed first nq queries, trimmed bytes)."""
        n = self.u64()
        v0 = self.o
        self.o += 4 * n
        dims = [self.u64() for _ in range(self.u64())]
        assert len(dims) == 2 and dims[0] * dims[1] == n and dims[0] >= nq
        width = dims[1]
        r0 = self.o
        root = self.digest()
        root_bytes = self.b[r0:self.o]
        log_h, pwidth = self.u64(), self.u64()
        npath = self.u64()
        p0 = self.o
        for k in range(npath):
            assert struct.unpack_from("<Q", self.b, p0 + 40 * k)[0] == 32, "path digest length prefix"
        self.o += 40 * npath
        pd = [self.u64() for _ in range(self.u64())]
        assert pd == [dims[0], log_h] and pwidth == width and npath == dims[0] * log_h
        vals = list(struct.unpack_from("<%dI" % (nq * width), self.b, v0))
        assert all(x < P for x in vals)
        paths = [int.from_bytes(self.b[p0 + 40 * k + 8:p0 + 40 * k + 40], "little") for k in range(nq * log_h)]
        assert all(x < M.P for x in paths)
        q = struct.pack
        blob = (q("<Q", nq * width) + self.b[v0:v0 + 4 * nq * width] + q("<QQQ", 2, nq, width) + root_bytes +
                q("<QQ", log_h, width) + q("<Q", nq * log_h) + self.b[p0:p0 + 40 * nq * log_h] + q("<QQQ", 2, nq, log_h))
        return dict(values=[vals[i * width:(i + 1) * width] for i in range(nq)], width=width, root=root, log_h=log_h,
                    paths=[paths[i * log_h:(i + 1) * log_h] for i in range(nq)]), blob


class Tape:
    """make_transcript.py's tape over the outer challenger (canonical KoalaBear words in and out)."""

    def __init__(self):
        self.ch = M.Challenger()
        self.ops, self.data = [], []

    def _push(self, op, arg, words, pinned):
        self.ops.append((op, arg, len(self.data), pinned))
        self.data.extend(int(w) for w in words)

    def observe(self, words):
        words = [int(w) for w in words]
        self._push(0, len(words), words, 1)
        for w in words:
            self.ch.observe(M.kb_to_monty(w))

    def observe_digest(self, d):
        self._push(4, 8, [(d >> (32 * i)) & 0xFFFFFFFF for i in range(8)], 1)
        self.ch.observe_commitment(d)

    def observe_exts(self, es):
        self.observe([w for e in es for w in e])

    def observe_var_exts(self, es):
        self.observe([len(es)] + [w for e in es for w in e])

    def sample_ext(self, expect=None, pinned=False):
        got = [M.kb_from_monty(self.ch.sample()) for _ in range(4)]
        if expect is not None:
            assert got == list(expect), "sampled challenge differs from the proof's"
        self._push(1, 4, got, int(expect is not None or pinned))
        return got

    def sample_bits(self, bits, expect=None):
        got = self.ch.sample_bits(bits)
        if expect is not None:
            assert got == expect, "sampled bits differ"
        self._push(2, bits, [got], int(expect is not None))
        return got

    def check_witness(self, bits, w):
        assert self.ch.check_witness(bits, M.kb_to_monty(w)), "grinding witness rejected"
        self._push(3, bits, [w], 1)

    def sumcheck(self, sc, degree):
        n = len(sc["polys"])
        for k, poly in enumerate(sc["polys"]):
            assert len(poly) == degree + 1
            self.observe_exts(poly)
            self.sample_ext(expect=sc["point"][n - 1 - k])

    def fork(self):
        t = Tape()
        t.ch, t.ops, t.data = self.ch.clone(), list(self.ops), list(self.data)
        return t


def verify_opening(o, commit, idx):
    """The Merkle layer of one opening at the given indices (tests/outer_model.py primitives only)."""
    assert M.commitment(o["root"], o["log_h"], o["width"]) == commit, "commitment cap"
    for q, i in enumerate(idx):
        node = M.hash_row(o["values"][q])
        for k in range(o["log_h"]):
            sib = o["paths"][q][k]
            node = M.compress(sib, node) if (i >> k) & 1 else M.compress(node, sib)
        assert node == o["root"], "Merkle path does not reach the stored root (query %d)" % q


def check_folds(comps, folds, coeffs, betas, idx, final_poly, lg_max):
    """verify_queries on the kept queries: batched component values -> fold chain -> final_poly."""
    g = kb.two_adic_generator(lg_max)
    for j, q in enumerate(idx):
        acc, off = [0, 0, 0, 0], 0
        for o in comps:
            for c, v in enumerate(o["values"][j]):
                acc = kb.ext_add(acc, kb.ext_scale(coeffs[off + c], v))
            off += o["width"]
        x, i = pow(g, kb.reverse_bits_len(q, lg_max), P), q
        for r, o in enumerate(folds):
            ev = [o["values"][j][:4], o["values"][j][4:]]
            assert ev[i & 1] == acc, "query value mismatch (query %d, round %d)" % (j, r)
            acc = kb.fold_query(ev[0], ev[1], betas[r], x if i & 1 == 0 else (P - x) % P)
            i >>= 1
            x = x * x % P
        assert acc == final_poly, "fold chain does not end in final_poly (query %d)" % j


def partial_lagrange(point):
    ev = [kb.ext_from_base(1)]
    for x in point:
        nx = []
        for e in ev:
            prod = kb.ext_mul(e, x)
            nx += [kb.ext_sub(e, prod), prod]
        ev = nx
    return ev


def main():
    vkb = open(DIR + "wrap_vk.bin", "rb").read()
    assert len(vkb) == 112
    v = OReader(vkb)
    pc_start = v.felts(3)
    gcs_x, gcs_y = v.felts(7), v.felts(7)
    pre_commit = v.digest()
    enable_untrusted = v.felts(1)[0]
    assert v.o == 112
    b = open(DIR + "wrapped_proof.bin", "rb").read()
    r = OReader(b)
    public_values = r.felts(r.u64())
    assert len(public_values) == 187
    main_commit = r.digest()
    numer, nd = r.tensor_ext(2)
    denom, dd = r.tensor_ext(2)
    assert nd == dd and nd[1] == 1
    rounds = []
    for _ in range(r.u64()):
        n0, n1, d0, d1 = r.ext(), r.ext(), r.ext(), r.ext()
        rounds.append(dict(n0=n0, n1=n1, d0=d0, d1=d1, sc=r.sumcheck()))
    logup_point = r.vec_ext()
    gkr_openings = []
    for _ in range(r.u64()):
        name = r.string()
        main_ev, _ = r.tensor_ext(1)
        prep_ev = r.tensor_ext(1)[0] if r.u8() else None
        gkr_openings.append((name, prep_ev, main_ev))
    gkr_witness = r.felts(1)[0]
    zerocheck = r.sumcheck()
    opened = []
    for _ in range(r.u64()):
        name = r.string()
        prep, mainv = r.vec_ext(), r.vec_ext()
        degree = r.felts(r.u64())
        opened.append((name, prep, mainv, degree))
    assert [o[0] for o in opened] == [g[0] for g in gkr_openings] == sorted(o[0] for o in opened)
    max_log_row_count = len(rounds) + 1
    assert all(len(o[3]) == max_log_row_count + 1 for o in opened)
    bf_start = r.o
    n_uni = r.u64()
    uni = [r.exts(2) for _ in range(n_uni)]
    fri_commits = [r.digest() for _ in range(r.u64())]
    assert len(fri_commits) == n_uni
    blob = bytearray(b[bf_start:r.o])
    parsed = []
    for _ in range(2):
        cnt = r.u64()
        blob += struct.pack("<Q", cnt)
        group = []
        for _ in range(cnt):
            o, ob = r.opening(NQ_KEEP)
            group.append(o)
            blob += ob
        parsed.append(group)
    comps, folds = parsed
    assert len(comps) == 2 and len(folds) == n_uni
    tail = r.o
    final_poly = r.ext()
    pow_witness, batch_witness = r.felts(1)[0], r.felts(1)[0]
    blob += b[tail:r.o]
    batch_evals = [r.tensor_ext(1)[0] for _ in range(r.u64())]
    jagged_sc = r.sumcheck()
    jagged_eval_sc = r.sumcheck()
    rc = [[(r.u64(), r.u64()) for _ in range(r.u64())] for _ in range(r.u64())]
    mt_commits = [r.digest() for _ in range(r.u64())]
    expected_eval = r.ext()
    assert r.u64() == max_log_row_count
    log_m = r.u64()
    assert r.o == len(b), "trailing bytes: %d of %d parsed" % (r.o, len(b))
    assert len(mt_commits) == 2 and [len(be) for be in batch_evals] == [o["width"] for o in comps]
    print("parsed the whole outer shard proof: %d bytes, %d chips, %d fold rounds, log_m %d; every digest is u64(32) + 32 bytes"
          % (r.o, len(opened), n_uni, log_m))

    # ======================= replay ==============================================================
    t = Tape()
    t.observe_digest(pre_commit)
    t.observe(pc_start)
    t.observe(gcs_x)
    t.observe(gcs_y)
    t.observe([enable_untrusted])
    t.observe([0] * 6)
    t.observe(public_values)
    t.observe_digest(main_commit)
    t.observe([len(opened)])
    for name, _, _, degree in opened:
        acc = 0
        for x in degree:
            acc = (x + 2 * acc) % P
        t.observe([acc, len(name)] + list(name.encode()))
    head = t
    niv = (len(numer).bit_length() - 1) - 1
    found = None
    for beta_seed_dim in range(1, 9):
        t = head.fork()
        try:
            t.check_witness(GKR_GRINDING_BITS, gkr_witness)
            t.sample_ext()
            for _ in range(beta_seed_dim):
                t.sample_ext()
            t.sample_ext()
            t.observe_var_exts(numer)
            t.observe_var_exts(denom)
            eval_point = [t.sample_ext(pinned=True) for _ in range(niv + 1)]
            num_eval, den_eval = eval_mle(numer, eval_point), eval_mle(denom, eval_point)
            for i, rd in enumerate(rounds):
                lam = t.sample_ext(pinned=True)
                assert rd["sc"]["claimed_sum"] == kb.ext_add(kb.ext_mul(num_eval, lam), den_eval), "gkr claim"
                assert len(rd["sc"]["polys"]) == i + niv + 1
                t.sumcheck(rd["sc"], 3)
                eq = full_lagrange_eval(rd["sc"]["point"], eval_point)
                nse = kb.ext_add(kb.ext_mul(rd["n0"], rd["d1"]), kb.ext_mul(rd["n1"], rd["d0"]))
                dse = kb.ext_mul(rd["d0"], rd["d1"])
                assert rd["sc"]["eval"] == kb.ext_mul(eq, kb.ext_add(kb.ext_mul(nse, lam), dse)), "gkr final eval"
                t.observe_exts([rd["n0"], rd["n1"], rd["d0"], rd["d1"]])
                last = t.sample_ext(pinned=True)
                eval_point = list(rd["sc"]["point"]) + [last]
                num_eval = kb.ext_add(rd["n0"], kb.ext_mul(kb.ext_sub(rd["n1"], rd["n0"]), last))
                den_eval = kb.ext_add(rd["d0"], kb.ext_mul(kb.ext_sub(rd["d1"], rd["d0"]), last))
            found = beta_seed_dim
            break
        except AssertionError:
            if beta_seed_dim == 8:
                raise
    print("LogUp-GKR transcript OK: 12-bit witness, beta_seed_dim", found, ", 20 rounds' points and claim equations")
    assert eval_point[niv:] == logup_point and len(logup_point) == max_log_row_count
    t.observe([len(opened)])
    for name, prep_ev, main_ev in gkr_openings:
        if prep_ev is not None:
            t.observe_var_exts(prep_ev)
        t.observe_var_exts(main_ev)
    t.sample_ext()
    t.sample_ext()
    t.sample_ext()
    assert len(zerocheck["polys"]) == max_log_row_count
    t.sumcheck(zerocheck, 4)
    t.observe([len(opened)])
    for name, prep, mainv, _ in opened:
        t.observe_var_exts(prep)
        t.observe_var_exts(mainv)
    col_counts = [[c for _, c in rnd] for rnd in rc]
    n_prefix = sum(sum(c) for c in col_counts) + 1
    num_col_variables = (n_prefix - 1 - 1).bit_length() if n_prefix > 2 else 0
    for _ in range(num_col_variables):
        t.sample_ext()
    t.sumcheck(jagged_sc, 2)
    t.observe_exts([jagged_eval_sc["claimed_sum"]])
    t.sumcheck(jagged_eval_sc, 2)
    print("zerocheck, jagged sumcheck and jagged-eval sumcheck points OK")
    t.observe_exts([expected_eval])
    for be in batch_evals:
        t.observe_exts(be)
    entry = t.ch.clone()                                     # BaseFold entry: verify_mle_evaluations starts here
    entry_op = len(t.ops)
    t.check_witness(BATCH_GRINDING_BITS, batch_witness)
    total = sum(len(be) for be in batch_evals)
    coeffs = partial_lagrange([t.sample_ext() for _ in range((total - 1).bit_length())])
    t.observe([n_uni])
    betas = []
    for k in range(n_uni):
        t.observe_exts(uni[k])
        t.observe_digest(fri_commits[k])
        betas.append(t.sample_ext(pinned=True))              # pinned by the fold equation below
    t.observe_exts([final_poly])
    t.check_witness(POW_BITS, pow_witness)
    qi = [t.sample_bits(n_uni + LOG_BLOWUP) for _ in range(NUM_QUERIES)]
    idx = qi[:NQ_KEEP]
    print("BaseFold transcript: 5-bit and 22-bit witnesses OK")

    # ======================= Merkle layer + fold chain on the kept queries ========================
    lg_max = n_uni + LOG_BLOWUP
    for o, c in zip(comps, mt_commits):
        assert o["log_h"] == lg_max
        verify_opening(o, c, idx)
    cur = list(idx)
    for k, o in enumerate(folds):
        cur = [i >> 1 for i in cur]
        assert o["log_h"] == lg_max - 1 - k and o["width"] == 8
        verify_opening(o, fri_commits[k], cur)
    print("Merkle layer OK: 2 component rounds + %d fold rounds x %d queries reach their roots at the SAMPLED indices; every"
          " commitment = compress(root, hash([log_height, width]))" % (n_uni, NQ_KEEP))
    check_folds(comps, folds, coeffs, betas, idx, final_poly, lg_max)
    z, o1 = uni[-1]
    assert final_poly == kb.ext_add(z, kb.ext_mul(betas[-1], o1))
    print("fold equation OK with the sampled betas on every kept query, down to final_poly")

    log_stacking_height = n_uni
    stack_point = jagged_sc["point"][len(jagged_sc["point"]) - log_stacking_height:]

    def b32(x):
        return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)

    p1 = os.path.join(HERE, "outer_wrap_basefold.npz")
    np.savez_compressed(p1, basefold_proof_q12=np.frombuffer(bytes(blob), dtype=np.uint8),
                        commits=np.stack([b32(c) for c in mt_commits]), point=np.array(stack_point, dtype=np.uint32),
                        claims0=np.array(batch_evals[0], dtype=np.uint32), claims1=np.array(batch_evals[1], dtype=np.uint32),
                        betas=np.array(betas, dtype=np.uint32), query_indices=np.array(qi, dtype=np.uint32),
                        entry_sponge=np.stack([b32(x) for x in entry.sponge]), entry_inp=np.array(entry.inp, dtype=np.uint32),
                        entry_out=np.array(entry.out, dtype=np.uint32),
                        vk_preprocessed_commit=b32(pre_commit), main_commitment=b32(main_commit),
                        vk_bytes=np.frombuffer(vkb, dtype=np.uint8))
    p2 = os.path.join(HERE, "outer_wrap_transcript.npz")
    np.savez_compressed(p2, ops=np.array(t.ops, dtype=np.int32), data=np.array(t.data, dtype=np.uint32),
                        final_state=t.ch.state(), beta_seed_dim=np.int32(found), basefold_entry_op=np.int32(entry_op))
    for p in (p1, p2):
        assert os.path.getsize(p) <= 216 * 1024, (p, os.path.getsize(p))
        print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
