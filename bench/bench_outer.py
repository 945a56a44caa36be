#!/usr/bin/env python3
"""The outer (BN254) commitment layer on one GPU: batched Poseidon2-BN254 permutations, outer Merkle commitments, outer
commit_mles beside the inner (KoalaBear Poseidon2) commit_mles on the same input, and the device grind. Prints one JSON line.

Every workload is timed (median of --repeat runs after one warm-up, host clock around a device synchronise), then — unless
--no-pmc — run once more in a child process under `rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES` (a counter run of its own, no
tracing) to get its VALU instructions per permutation (SQ_INSTS_VALU counts wave instructions; a wave carries 64
permutations) and the fraction of the measured 32-bit integer add rate (profiles/r01_ubench_int.txt: 53.9 T lane-ops/s) that
the timed run issued.

  python bench/bench_outer.py [--repeat R] [--no-pmc] [--pmc-dir DIR]
  python bench/bench_outer.py --one NAME        (one run of one workload: what the counter runs execute)
  python bench/bench_outer.py --basefold        (the outer BaseFold opening: profiles/outer_basefold_bench.json)
  python bench/bench_outer.py --jagged          (the outer stacked + jagged PCS: profiles/outer_jagged_bench.json)

--basefold times sp1hip_outer_basefold_prove at 2^16 and 2^20 rows, blowup 8, width 32, 94 queries, 22 proof-of-work bits
(median of --repeat), splits one run by the library's ScopedTimers (batch + encode, commit phase, grinds, openings: event time
on the stream, the commit phase includes its per-round host hand-overs), compares that commit phase with the same rounds done
as separate sp1hip_outer_merkle_commit calls plus the inner fold kernels (alternating in one process), and measures the small-tree regime: the time of an
outer 2^k x 8 tree for k = 1..12 minus its permutations at the batched rate, per level.

--jagged runs sp1hip_outer_jagged_commit of both rounds and sp1hip_outer_jagged_prove at the real wrap proof's shape (the
(rows, cols) of tests/golden/outer_wrap_jagged.npz, seeded random tables, max_log_row_count = log_stacking_height = 21, blowup 8,
94 queries, 22 bits): medians of --repeat with min / max (host clock around a device synchronise), one run split by the
library's ScopedTimers, and, alternating in the same process on the same tables, what a caller had before these entry points:
sp1hip_outer_commit_mles_data on the stacked columns (commit), and sp1hip_jagged_prove under the inner configuration minus
its own sp1hip_basefold_prove plus sp1hip_outer_basefold_prove on the same stacked columns (prove).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ADD_RATE = 53.9438e12          # lane-ops/s, v_add_u32 (profiles/r01_ubench_int.txt)
KB_P = 0x7F000001
MERKLE = [(20, 16), (20, 64), (20, 256), (22, 64)]
GRIND_BITS = 16


def _workloads():
    w = {"permute_2^22": None, "permute_2^22_lohi": None}
    for lg, width in MERKLE:
        w["merkle_2^%d_x%d" % (lg, width)] = (lg, width)
    w["outer_commit_mles_2^20_b4_x64"] = None
    w["inner_commit_mles_2^20_b4_x64"] = None
    w["grind_%d" % GRIND_BITS] = None
    return list(w)


def _perms(name):
    """Permutations one run performs (None: counted from the waves, see main)."""
    if name.startswith("permute"):
        return 1 << 22
    if name.startswith("merkle") or name.startswith("outer_commit_mles"):
        lg, width = (22, 64) if name.startswith("outer_commit") else next((l, w) for l, w in MERKLE if name == "merkle_2^%d_x%d" % (l, w))
        h = 1 << lg
        return h * ((width + 15) // 16) + (h - 1) + 2
    return None


class Runner:
    def __init__(self):
        import torch
        from sp1_amd import api
        self.torch, self.api = torch, api
        torch.cuda.set_device(0)
        self.g = torch.Generator(device="cuda").manual_seed(7)

    def _kb(self, n):
        t = self.torch
        return t.randint(0, KB_P, (n,), generator=self.g, device="cuda", dtype=t.int64).to(t.int32)

    def setup(self, name):
        api, t = self.api, self.torch
        if name.startswith("permute"):
            n = 1 << 22
            top = t.randint(0, 0x30644E72, (n, 3, 1), generator=self.g, device="cuda", dtype=t.int64).to(t.int32)
            low = t.randint(-(1 << 31), (1 << 31) - 1, (n, 3, 7), generator=self.g, device="cuda", dtype=t.int64).to(t.int32)
            states = t.cat([low, top], dim=2).reshape(-1).contiguous()           # each lane < p (top word below p's)
            lohi = name.endswith("lohi")

            def run():
                os.environ["SP1HIP_OUTER_MUL"] = "lohi" if lohi else "mad"
                api.outer_poseidon2_permute(states)
            return run
        if name.startswith("merkle"):
            lg, width = next((l, w) for l, w in MERKLE if name == "merkle_2^%d_x%d" % (l, w))
            cm = api.ColMajor(self._kb(width << lg), 1 << lg, width)
            prover = api.OuterMerkleTcsProver()
            return lambda: prover.commit_tensors([cm])
        if name.endswith("commit_mles_2^20_b4_x64"):
            mles = [api.ColMajor(self._kb(64 << 20), 1 << 20, 64)]
            if name.startswith("outer"):
                return lambda: api.outer_commit_mles(mles, 2)
            prover = api.BasefoldProver(2, 124, 16)
            return lambda: prover.commit_mles(mles)
        if name.startswith("grind"):
            def run():
                ch = api.OuterChallenger()
                ch.observe(list(range(1, 10)))
                return ch.grind(GRIND_BITS)
            return run
        raise KeyError(name)

    def time(self, name, repeat):
        run = self.setup(name)
        run()
        self.torch.cuda.synchronize()
        ts = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            run()
            self.torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2]


def counters(name, pmc_dir):
    """SQ_INSTS_VALU and SQ_WAVES summed over the outer_* kernels (the inner commit: every sp1hip kernel) of one run."""
    d = os.path.join(pmc_dir, name.replace("^", ""))
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_WAVES", "--output-format", "csv", "-d", d,
           "-o", "pmc", "--", sys.executable, os.path.abspath(__file__), "--one", name]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("counter run of %s failed (%d): %s" % (name, r.returncode, r.stderr[-2000:]))
    want = (lambda k: "outer_" in k) if not name.startswith("inner") else (lambda k: "sp1hip" in k and "at::" not in k)
    tot = {"SQ_INSTS_VALU": 0.0, "SQ_WAVES": 0.0}
    for fn in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(fn)):
            if want(row["Kernel_Name"]) and row["Counter_Name"] in tot:
                tot[row["Counter_Name"]] += float(row["Counter_Value"])
    return tot


BF_STAGES = ["outer_bf_batch_encode", "outer_bf_commit_phase", "outer_bf_grind", "outer_bf_openings", "outer_leaf_hash_pairs",
             "outer_compress"]


def basefold_bench(repeat):
    import ctypes as C
    r = Runner()
    api, t = r.api, r.torch
    from sp1_amd._lib import FriConfig
    lib = api._L()
    out = {"workload": "outer (BN254) BaseFold opening", "gpus": 1, "log_blowup": 3, "num_queries": 94, "pow_bits": 22, "width": 32}
    cfg = FriConfig(3, 94, 22)
    prover = api.OuterBasefoldProver()
    for dim in (16, 20):
        mles = [api.ColMajor(r._kb(32 << dim), 1 << dim, 32)]
        commit, pd = prover.commit_mles(mles, 3)
        ch0 = api.OuterChallenger()
        ch0.observe_commitment(commit)
        point = ch0.sample_point(dim)
        claims = api.BasefoldProver().evaluate_mles(mles, point)

        def run():
            return prover.prove(point, [pd], claims, ch0.clone(), cfg)
        run()
        ts = []
        for _ in range(repeat):
            t.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        out["outer_basefold_prove_2^%d_b8_x32_ms" % dim] = round(ts[len(ts) // 2], 3)
        out["outer_basefold_prove_2^%d_b8_x32_min_max_ms" % dim] = [round(ts[0], 3), round(ts[-1], 3)]
        # the commit phase against what a caller could do before this prover existed: per round one sp1hip_outer_merkle_commit
        # on a width-8 pair tensor (root and commitment read back, as the transcript needs them) plus the two inner fold
        # kernels; fused and yardstick alternate in one process
        lg0 = dim + 3
        pair = [api.ColMajor(r._kb(8 << (lg0 - 1 - k)), 1 << (lg0 - 1 - k), 8) for k in range(dim)]
        cw = [api.device_words(4 << (lg0 - k)) for k in range(dim + 1)]
        ml = [api.device_words(4 << (dim - k)) for k in range(dim + 1)]
        cw[0].copy_(r._kb(4 << lg0))
        ml[0].copy_(r._kb(4 << dim))
        beta = api._ext(point[0])
        tcs = api.OuterMerkleTcsProver()

        def yardstick():
            for k in range(dim):
                tcs.commit_tensors([pair[k]])
                api.check(lib.sp1hip_fold_even_odd(api._dptr(cw[k]), lg0 - k, beta, api._dptr(cw[k + 1]), None))
                api.check(lib.sp1hip_fold_mle(api._dptr(ml[k]), dim - k, beta, api._dptr(ml[k + 1]), None))
            t.cuda.synchronize()

        def read_stages():
            stages = {}
            for name in BF_STAGES:
                n_, ms_ = C.c_uint64(), C.c_double()
                api.check(lib.sp1hip_timers_read(name.encode(), C.byref(n_), C.byref(ms_)))
                stages[name] = {"launches": n_.value, "ms": round(ms_.value, 3)}
            return stages

        yardstick()
        fused, yard, stages = [], [], {}
        for _ in range(max(repeat, 5)):
            api.check(lib.sp1hip_timers_reset())
            api.check(lib.sp1hip_timers_enable(1))
            run()
            stages = read_stages()
            api.check(lib.sp1hip_timers_enable(0))
            fused.append(stages["outer_bf_commit_phase"]["ms"])
            t.cuda.synchronize()
            t0 = time.perf_counter()
            yardstick()
            yard.append((time.perf_counter() - t0) * 1e3)
        fused.sort()
        yard.sort()
        out["stages_2^%d" % dim] = stages
        out["commit_phase_2^%d" % dim] = {"fused_ms": round(fused[len(fused) // 2], 3), "fused_min_max_ms": [round(fused[0], 3), round(fused[-1], 3)],
                                          "yardstick_ms": round(yard[len(yard) // 2], 3), "yardstick_min_max_ms": [round(yard[0], 3), round(yard[-1], 3)]}
        del pair, cw, ml
        del pd, mles
        t.cuda.empty_cache()
    # small trees: time of a 2^k x 8 tree against its 2^(k+1) permutations at the batched rate
    rate = (1 << 22) / r.time("permute_2^22", 3) * 1e3
    tcs = api.OuterMerkleTcsProver()
    small = {}
    for k in range(1, 13):
        cm = api.ColMajor(r._kb(8 << k), 1 << k, 8)
        tcs.commit_tensors([cm])
        ts = []
        for _ in range(max(repeat, 5)):
            t.cuda.synchronize()
            t0 = time.perf_counter()
            tcs.commit_tensors([cm])
            t.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        ms = ts[len(ts) // 2]
        thr = ((2 << k) + 1) / rate * 1e3
        small["2^%d" % k] = {"ms": round(ms, 4), "throughput_ms": round(thr, 4), "per_level_ms": round((ms - thr) / (k + 2), 4)}
    out["permute_per_s"] = round(rate)
    out["small_tree_x8"] = small
    print(json.dumps(out))


JG_STAGES = ["ntt_pass0", "ntt_pass1", "ntt_pass2", "outer_leaf_hash", "outer_compress", "jagged_round0_sum", "jagged_fold0_sum", "jagged_fold_sum", "jagged_batch_evals",
             "outer_bf_batch_encode", "outer_bf_commit_phase", "outer_bf_grind", "outer_bf_openings"]


def jagged_bench(repeat):
    import ctypes as C
    import numpy as np
    r = Runner()
    api, t = r.api, r.torch
    from sp1_amd._lib import FriConfig
    lib = api._L()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "outer_wrap_jagged.npz"))
    L = lsh = 21
    lb, nq, pw, batch = 3, 94, 22, 64
    cfg = FriConfig(lb, nq, pw)
    shapes = [[(int(a), int(c)) for a, c in fx["counts%d" % k]][:-2] for k in range(2)]
    tabs = [[api.ColMajor(r._kb(h * w), h, w) for h, w in sh] for sh in shapes]
    ojp, ijp = api.OuterJaggedProver(L, lsh, batch, lb), api.JaggedProver(L, lsh, batch, lb)
    obf, ibf = api.OuterBasefoldProver(), api.BasefoldProver(lb, nq, pw)

    def timed(f):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        res = f()
        t.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    def stat(ts):
        ts = sorted(ts)
        return {"ms": round(ts[len(ts) // 2], 3), "min_max_ms": [round(ts[0], 3), round(ts[-1], 3)]}

    def read_stages():
        stages = {}
        for name in JG_STAGES:
            n_, ms_ = C.c_uint64(), C.c_double()
            api.check(lib.sp1hip_timers_read(name.encode(), C.byref(n_), C.byref(ms_)))
            stages[name] = {"launches": n_.value, "ms": round(ms_.value, 3)}
        return stages

    out = {"workload": "outer (BN254) stacked + jagged PCS at the wrap proof's shape", "gpus": 1, "log_blowup": lb, "num_queries": nq,
           "pow_bits": pw, "max_log_row_count": L, "log_stacking_height": lsh, "repeat": repeat,
           "stacked_widths": [], "areas": [sum(h * w for h, w in sh) for sh in shapes]}
    new_c, yard_c = [[], []], [[], []]
    commit_stages = None
    for it in range(repeat + 1):                           # the first pass is the warm-up
        o_rounds = []
        for k in range(2):
            if it == repeat:
                api.check(lib.sp1hip_timers_reset())
                api.check(lib.sp1hip_timers_enable(1))
            ms, (c, sd) = timed(lambda: ojp.commit_multilinears(tabs[k]))
            if it == repeat:
                commit_stages = (commit_stages or []) + [read_stages()]
                api.check(lib.sp1hip_timers_enable(0))
            o_rounds.append((c, sd))
            ms_y, pd = timed(lambda: obf.commit_mles(sd.batches, lb))
            del pd
            if it:
                new_c[k].append(ms)
                yard_c[k].append(ms_y)
        if it < repeat:
            del o_rounds
    out["stacked_widths"] = [sum(b.width for b in sd.batches) for _, sd in o_rounds]
    for k in range(2):
        out["outer_jagged_commit_round%d" % k] = stat(new_c[k])
        out["yardstick_outer_commit_mles_data_round%d" % k] = stat(yard_c[k])
        out["commit_stages_round%d" % k] = commit_stages[k]
    i_rounds = [ijp.commit_multilinears(tb) for tb in tabs]
    ch_o, ch_i = api.OuterChallenger(), api.DuplexChallenger()
    for c, _ in o_rounds:
        ch_o.observe_commitment(c)
    for c, _ in i_rounds:
        ch_i.observe(c)
    z_row = ch_o.sample_point(L)
    claims = []
    for tb in tabs:
        cl = []
        for tt in tb:
            w = t.zeros((tt.width, 1 << L), dtype=t.int32, device="cuda")
            w[:, :tt.height] = tt.words.view(tt.width, tt.height)
            cl.append(np.asarray(ibf.evaluate_mles([api.ColMajor(w.view(-1), 1 << L, tt.width)], z_row)).reshape(-1, 4))
            del w
        claims.append(np.concatenate(cl))
    pt = ch_o.clone().sample_point(lsh)
    bf_claims = np.concatenate([np.asarray(ibf.evaluate_mles(sd.batches, pt)).reshape(-1, 4) for _, sd in o_rounds])
    o_pds = [obf.commit_mles(sd.batches, lb)[1] for _, sd in o_rounds]
    runs = {
        "outer_jagged_prove": lambda: ojp.prove_trusted_evaluations(z_row, claims, [sd for _, sd in o_rounds], ch_o.clone(), nq, pw),
        "inner_jagged_prove": lambda: ijp.prove_trusted_evaluations(z_row, claims, [sd for _, sd in i_rounds], ch_i.clone(), nq, pw),
        "inner_basefold_prove": lambda: ibf.prove_trusted_mle_evaluations(pt, [sd.basefold for _, sd in i_rounds], bf_claims, ch_i.clone()),
        "outer_basefold_prove": lambda: obf.prove(pt, o_pds, bf_claims, ch_o.clone(), cfg),
    }
    ts = {k: [] for k in runs}
    yard = []
    for it in range(repeat + 1):
        one = {k: timed(f)[0] for k, f in runs.items()}     # alternating, one of each per pass
        if it:
            for k in runs:
                ts[k].append(one[k])
            yard.append(one["inner_jagged_prove"] - one["inner_basefold_prove"] + one["outer_basefold_prove"])
    for k in runs:
        out[k] = stat(ts[k])
    out["yardstick_prove (inner jagged - inner basefold + outer basefold)"] = stat(yard)
    api.check(lib.sp1hip_timers_reset())
    api.check(lib.sp1hip_timers_enable(1))
    blob = runs["outer_jagged_prove"]()
    out["prove_stages"] = read_stages()
    api.check(lib.sp1hip_timers_enable(0))
    out["proof_bytes"] = len(blob)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-pmc", action="store_true")
    ap.add_argument("--pmc-dir", default=None, help="where the counter runs write (default: a temporary directory, removed after)")
    ap.add_argument("--one")
    ap.add_argument("--basefold", action="store_true")
    ap.add_argument("--jagged", action="store_true")
    args = ap.parse_args()
    if args.basefold:
        return basefold_bench(args.repeat)
    if args.jagged:
        return jagged_bench(args.repeat)
    if args.one:
        r = Runner()
        r.setup(args.one)()
        r.torch.cuda.synchronize()
        return
    r = Runner()
    out = {"workload": "outer (BN254) commitment layer", "gpus": 1}
    times = {}
    for name in _workloads():
        times[name] = r.time(name, args.repeat if not name.startswith("merkle_2^22") else max(2, args.repeat // 2))
        r.torch.cuda.empty_cache()
    out["permute_2^22_per_s"] = round((1 << 22) / times["permute_2^22"] * 1e3)
    out["permute_2^22_lohi_per_s"] = round((1 << 22) / times["permute_2^22_lohi"] * 1e3)
    for name, ms in times.items():
        if not name.startswith("permute"):
            out[name + "_ms"] = round(ms, 3)
    if not args.no_pmc:
        valu = {}
        pmc_dir = args.pmc_dir or tempfile.mkdtemp(prefix="outer_pmc_")
        for name in _workloads():
            c = counters(name, pmc_dir)
            perms = _perms(name) or c["SQ_WAVES"] * 64                 # grind: one candidate per lane
            if name.startswith("inner"):
                valu[name] = {"valu_insts_per_row": round(c["SQ_INSTS_VALU"] * 64 / (1 << 22), 1)}
                continue
            per = c["SQ_INSTS_VALU"] * 64 / perms
            valu[name] = {"valu_insts_per_perm": round(per), "perms": int(perms),
                          "valu_fraction_of_add_rate": round(per * perms / (times[name] * 1e-3) / ADD_RATE, 3)}
        out["pmc"] = valu
        if args.pmc_dir is None:
            shutil.rmtree(pmc_dir, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
