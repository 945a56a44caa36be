#!/usr/bin/env python3
"""Record the jagged PCS part of the reference's one real OUTER (BN254) shard proof as a fixture.

Sources (read-only, only in the build container): the same wrapped_proof.bin / wrap_vk.bin as make_outer_golden.py, parsed with
its OReader, and the tape that generator recorded (tests/golden/outer_wrap_transcript.npz), replayed under
tests/outer_model.py's challenger up to the point where `JaggedPcsVerifier::verify_trusted_evaluations` starts: after the
opened values of every chip are observed, before the z_col samples. The ops that follow on the tape are asserted to be the
jagged ones (the z_col samples, 27 + 56 sumcheck rounds, the expected_eval and batch-evaluation observes) right up to the
recorded BaseFold entry.

Output tests/golden/outer_wrap_jagged.npz (data only):
  counts0 / counts1      (rows, cols) of every table of the preprocessed / main round, the two padding tables included
  z_row                  the zerocheck point
  claims0 / claims1      every chip's opened preprocessed / main values in chip order: the column claims the verifier consumes
  batch0 / batch1        JaggedPcsProof.batch_evaluations
  js_* / je_*            the jagged and the jagged-eval sumcheck (polys, claimed_sum, point, eval)
  expected_eval, max_log_row_count, log_m
  entry_sponge (3 x 32 LE bytes, canonical), entry_inp, entry_out (canonical KoalaBear words): the challenger at jagged entry
The BaseFold proof, the two stacked commitments, main_commitment and the vk's preprocessed_commit are in
outer_wrap_basefold.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import outer_model as M  # noqa: E402
from make_outer_golden import DIR, NQ_KEEP, OReader  # noqa: E402


def parse():
    b = open(DIR + "wrapped_proof.bin", "rb").read()
    r = OReader(b)
    r.felts(r.u64())
    r.digest()
    r.tensor_ext(2)
    r.tensor_ext(2)
    n_gkr = r.u64()
    for _ in range(n_gkr):
        r.ext(), r.ext(), r.ext(), r.ext()
        r.sumcheck()
    r.vec_ext()
    for _ in range(r.u64()):
        r.string()
        r.tensor_ext(1)
        if r.u8():
            r.tensor_ext(1)
    r.felts(1)
    zerocheck = r.sumcheck()
    opened = []
    for _ in range(r.u64()):
        name = r.string()
        prep, mainv = r.vec_ext(), r.vec_ext()
        r.felts(r.u64())
        opened.append((name, prep, mainv))
    n_uni = r.u64()
    for _ in range(n_uni):
        r.exts(2)
    for _ in range(r.u64()):
        r.digest()
    for _ in range(2):
        for _ in range(r.u64()):
            r.opening(NQ_KEEP)
    r.ext()
    r.felts(2)
    batch = [r.tensor_ext(1)[0] for _ in range(r.u64())]
    js, je = r.sumcheck(), r.sumcheck()
    rc = [[(r.u64(), r.u64()) for _ in range(r.u64())] for _ in range(r.u64())]
    for _ in range(r.u64()):
        r.digest()
    expected_eval = r.ext()
    L, log_m = r.u64(), r.u64()
    assert r.o == len(b) and L == n_gkr + 1 == len(zerocheck["point"]) and len(rc) == 2 and len(batch) == 2
    return dict(zerocheck=zerocheck, opened=opened, batch=batch, js=js, je=je, rc=rc, expected_eval=expected_eval, L=L, log_m=log_m)


def replay(tape, stop):
    ch = M.Challenger()
    ops, data = tape["ops"], tape["data"]
    for op, arg, off, _ in ops[:stop]:
        w = [int(x) for x in data[off:off + (4 if op == 1 else 8 if op == 4 else 1 if op in (2, 3) else arg)]]
        if op == 0:
            for x in w:
                ch.observe(M.kb_to_monty(x))
        elif op == 1:
            assert [M.kb_from_monty(ch.sample()) for _ in range(4)] == w
        elif op == 2:
            assert ch.sample_bits(arg) == w[0]
        elif op == 3:
            assert ch.check_witness(arg, M.kb_to_monty(w[0]))
        else:
            ch.observe_commitment(sum(x << (32 * i) for i, x in enumerate(w)))
    return ch


def main():
    p = parse()
    tape = np.load(os.path.join(HERE, "outer_wrap_transcript.npz"))
    n_cols = sum(c for rnd in p["rc"] for _, c in rnd)
    ncv = max(n_cols - 1, 0).bit_length()
    log_m, D = p["log_m"], p["log_m"] + 1
    assert len(p["js"]["polys"]) == log_m and len(p["je"]["polys"]) == 2 * D
    n_ops = ncv + 2 * log_m + 1 + 2 * 2 * D + 1 + 2
    entry = int(tape["basefold_entry_op"]) - n_ops
    ops, data = tape["ops"], tape["data"]
    # the ops from `entry` on are the jagged ones
    k = entry
    assert all(ops[k + i][0] == 1 for i in range(ncv))
    k += ncv
    for poly, want in zip(p["js"]["polys"], p["js"]["point"][::-1]):
        assert ops[k][0] == 0 and [int(x) for x in data[ops[k][2]:ops[k][2] + 12]] == [w for c in poly for w in c]
        assert ops[k + 1][0] == 1 and [int(x) for x in data[ops[k + 1][2]:ops[k + 1][2] + 4]] == list(want)
        k += 2
    assert ops[k][0] == 0 and [int(x) for x in data[ops[k][2]:ops[k][2] + 4]] == list(p["je"]["claimed_sum"])
    # ... and the op before is the observe of the last chip's opened main values
    last = p["opened"][-1][2]
    assert ops[entry - 1][0] == 0 and [int(x) for x in data[ops[entry - 1][2]:ops[entry - 1][2] + 1 + 4 * len(last)]] == \
        [len(last)] + [w for e in last for w in e]
    ch = replay(tape, entry)

    def b32(x):
        return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)

    def ext(es):
        return np.array(es, dtype=np.uint32).reshape(-1, 4)

    out = dict(counts0=np.array(p["rc"][0], dtype=np.uint64), counts1=np.array(p["rc"][1], dtype=np.uint64),
               z_row=ext(p["zerocheck"]["point"]),
               claims0=ext([e for _, prep, _ in p["opened"] for e in prep]),
               claims1=ext([e for _, _, mainv in p["opened"] for e in mainv]),
               batch0=ext(p["batch"][0]), batch1=ext(p["batch"][1]), expected_eval=ext([p["expected_eval"]])[0],
               max_log_row_count=np.int64(p["L"]), log_m=np.int64(log_m),
               entry_sponge=np.stack([b32(x) for x in ch.sponge]), entry_inp=np.array(ch.inp, dtype=np.uint32),
               entry_out=np.array(ch.out, dtype=np.uint32))
    for tag, sc in (("js", p["js"]), ("je", p["je"])):
        out[tag + "_polys"] = np.array(sc["polys"], dtype=np.uint32)
        out[tag + "_claimed_sum"] = ext([sc["claimed_sum"]])[0]
        out[tag + "_point"] = ext(sc["point"])
        out[tag + "_eval"] = ext([sc["eval"]])[0]
    path = os.path.join(HERE, "outer_wrap_jagged.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 216 * 1024, os.path.getsize(path)
    print("wrote", path, os.path.getsize(path), "bytes; jagged entry at tape op", entry)


if __name__ == "__main__":
    main()
