"""The reference's one real outer (BN254) shard proof, crates/prover/wrapped_proof.bin, under the Python model, from the
committed fixtures alone (tests/golden/outer_wrap_*.npz, written by tests/golden/make_outer_golden.py; the reference tree is
not read). What passes here is pinned on the reference's own bytes: reduce_31 packing, the sponge's short-last-block rule,
compress, the commitment cap, the MultiField32Challenger (absorb order, duplexing, split_32 sample order, sample_bits, digest
observation) and the 40-byte digest encoding."""
import os
import struct

import numpy as np

import kb_py as kb
import outer_basefold_model as BM
import outer_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF = np.load(os.path.join(GOLD, "outer_wrap_basefold.npz"))
TAPE = np.load(os.path.join(GOLD, "outer_wrap_transcript.npz"))
LOG_BLOWUP, POW_BITS, NUM_QUERIES, NQ_KEEP = 3, 22, 94, 12


def _int(b):
    return int.from_bytes(bytes(b), "little")


def test_digest_encoding_at_every_digest_of_the_basefold_proof():
    blob = BF["basefold_proof_q12"].tobytes()
    p = BM.parse_proof(BM.OUTER, blob)                       # raises unless every digest is u64(32) + 32 bytes of a value < p
    assert len(p["commits"]) == 21 and len(p["comps"]) == 2 and len(p["folds"]) == 21
    n_digests = 21 + sum(1 + len(o["paths"]) for o in p["comps"] + p["folds"])
    assert blob.count(struct.pack("<Q", 32)) >= n_digests
    vk = BF["vk_bytes"].tobytes()                            # 12 B pc_start, 56 B septic digest, the digest, 4 B untrusted_config
    assert len(vk) == 112 and vk[68:76] == struct.pack("<Q", 32) and vk[76:108] == BF["vk_preprocessed_commit"].tobytes()


def test_transcript_replays_on_the_library_model():
    """Every op of the tape on tests/outer_model.py's Challenger: the pinned samples (sumcheck points, GKR last coordinates and
    lambdas, betas), the three grinding witnesses and the query indices come out as the reference's proof has them."""
    ch = M.Challenger()
    ops, data = TAPE["ops"], TAPE["data"]
    pinned = witnesses = 0
    bits_seen = []
    for op, arg, off, pin in ops:
        words = [int(w) for w in data[off:off + (arg if op in (0, 1) else 8 if op == 4 else 1)]]
        if op == 0:
            for w in words:
                ch.observe(M.kb_to_monty(w))
        elif op == 4:
            ch.observe_commitment(sum(w << (32 * i) for i, w in enumerate(words)))
        elif op == 1:
            assert [M.kb_from_monty(ch.sample()) for _ in range(arg)] == words
            pinned += pin
        elif op == 2:
            assert ch.sample_bits(arg) == words[0]
        else:
            assert ch.check_witness(arg, M.kb_to_monty(words[0])), "grinding witness rejected"
            witnesses += 1
            bits_seen.append(int(arg))
    assert bits_seen == [12, 5, POW_BITS] and pinned >= 500
    assert np.array_equal(ch.state(), TAPE["final_state"])
    q = [int(data[off]) for op, arg, off, _ in ops if op == 2]
    assert q == BF["query_indices"].tolist() and len(q) == NUM_QUERIES


def test_merkle_layer_and_fold_chain_of_the_kept_queries():
    p = BM.parse_proof(BM.OUTER, BF["basefold_proof_q12"].tobytes())
    idx = BF["query_indices"].tolist()[:NQ_KEEP]
    commits = [_int(c) for c in BF["commits"]]
    lg_max = 21 + LOG_BLOWUP

    def walk(o, commit, at):
        w, lg = o["width"], o["lg_h"]
        assert M.commitment(o["root"], lg, w) == commit
        for j, i in enumerate(at):
            node = M.hash_row(o["values"][j * w:(j + 1) * w])
            for k in range(lg):
                sib = o["paths"][j * lg + k]
                node = M.compress(sib, node) if (i >> k) & 1 else M.compress(node, sib)
            assert node == o["root"]

    for o, c, claims in zip(p["comps"], commits, (BF["claims0"], BF["claims1"])):
        assert o["lg_h"] == lg_max and o["width"] == len(claims)
        walk(o, c, idx)
    cur = list(idx)
    for r, o in enumerate(p["folds"]):
        cur = [i >> 1 for i in cur]
        assert o["lg_h"] == lg_max - 1 - r and o["width"] == 8
        walk(o, p["commits"][r], cur)
    # the sampled betas satisfy the fold equation on the opened pairs, down to final_poly
    betas = BF["betas"].tolist()
    g = kb.two_adic_generator(lg_max)
    for j, q in enumerate(idx):
        x, i = pow(g, kb.reverse_bits_len(q, lg_max), kb.P), q
        acc = None
        for r, o in enumerate(p["folds"]):
            ev = [o["values"][8 * j:8 * j + 4], o["values"][8 * j + 4:8 * j + 8]]
            assert acc is None or ev[i & 1] == acc
            acc = kb.fold_query(ev[0], ev[1], betas[r], x if i & 1 == 0 else (kb.P - x) % kb.P)
            i >>= 1
            x = x * x % kb.P
        assert acc == p["final_poly"]
