#!/usr/bin/env python3
"""What it costs to turn a run's touched addresses into the tables of a memory shard, two ways:

  host    the path every memory shard took so far: riscv_more_trace.memory_shard_from on `cuda` (rows filled in numpy and uploaded,
          Tracer.global_chip's torch septic lift, Tracer.byte_range_tables) plus core_real.to_col_major of every main table;
  device  riscv_exec.device_memory_shard from the same pageable arrays: two [n, 3] uploads, api.tracegen_riscv_memory_global per kind,
          api.tracegen_riscv_global, device_lookup_tables. No Tracer.

at two sizes: the memory shard of a whole fibonacci run (--cycles, executed without recording), and a synthetic shard of
split_thresholds(...)["memory"] finalise rows with as many initialise rows — the size of the rsp block's large memory shards, and a
Global table taller than any a core shard has made (the line says its height and that its digest equals the host's).

The two alternate in ONE process; medians of --rounds (5) with min and max, after one untimed round of both in which every table of
the two paths is compared word for word. The device side is also timed piece by piece on its own (upload, MemoryGlobal kernels,
Global with its 14-word digest readback, lookup counts), the host side split by timing global_chip and byte_range_tables inside
memory_shard_from (row filling is the rest of it) and to_col_major apart. ONE assertion per size besides the tables: the device
path's median is not above the host path's median by more than the host path's own min-max spread. One JSON line; `--out` also
writes it to a file. Without a GPU the line says so and holds no figure.

  python bench/bench_device_memory_shard.py [--cycles 26000000] [--out profiles/device_memory_shard_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bench"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic_lists(n, seed=1):
    """n strictly increasing 8-aligned addresses above the registers with random words and timestamps, for both kinds."""
    rng = np.random.default_rng(seed)
    addrs = (np.cumsum(rng.integers(1, 64, size=n, dtype=np.int64)) * 8 + (1 << 16)).astype(np.uint64)
    rec = lambda: np.stack([rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64), rng.integers(1, 1 << 40, size=n, dtype=np.int64)], axis=1)
    return addrs, rec(), addrs, rec(), 1 << 15, 1 << 15


def measure(name, lists, ctx, prep, rounds, log):
    from core_real import to_col_major
    from sp1_amd import api
    from sp1_amd.machines import public_values as PVM, riscv_exec as X, riscv_more_trace as MT, riscv_trace as RT
    ia, ir, fa, fr, p_init, p_fin = lists
    sync = torch.cuda.synchronize
    inner = {"global_chip": 0.0, "byte_range_tables": 0.0}

    def timed(key, fn):
        def run(*a, **k):
            sync()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            sync()
            inner[key] += time.perf_counter() - t0
            return out
        return run

    def host():
        inner.update(global_chip=0.0, byte_range_tables=0.0)
        saved = RT.Tracer.global_chip, RT.Tracer.byte_range_tables
        RT.Tracer.global_chip, RT.Tracer.byte_range_tables = timed("global_chip", saved[0]), timed("byte_range_tables", saved[1])
        try:
            t0 = time.perf_counter()
            machine, tabs, publics, _ = MT.memory_shard_from(ia, ir, fr, "cuda", previous_addr=p_init, ctx=ctx, fin_addrs=fa, previous_fin_addr=p_fin)
            sync()
            t1 = time.perf_counter()
        finally:
            RT.Tracer.global_chip, RT.Tracer.byte_range_tables = saved
        chips = [(a, i, to_col_major(tabs[a.name][1]), prep.get(a.name)) for a, i in machine]
        sync()
        t2 = time.perf_counter()
        split = {"rows": t1 - t0 - inner["global_chip"] - inner["byte_range_tables"], "global_chip": inner["global_chip"],
                 "byte_range_tables": inner["byte_range_tables"], "to_col_major": t2 - t1}
        return (machine, chips, publics), split

    def device():
        made = X.device_memory_shard(ia, ir, fa, fr, prep, ctx, previous_init=p_init, previous_fin=p_fin)
        sync()
        return made

    def device_pieces():
        """device_memory_shard's steps, a synchronisation behind each."""
        t = [time.perf_counter()]
        mark = lambda: (sync(), t.append(time.perf_counter()))
        recs = [torch.from_numpy(X._memory_global_records(a, r, p, w)).cuda() for a, r, p, w in ((ia, ir, p_init, "init"), (fa, fr, p_fin, "finalize"))]
        mark()
        made, evs = {}, []
        for which, rec, previous in (("init", recs[0], p_init), ("finalize", recs[1], p_fin)):
            if rec.shape[0]:
                made[MT_NAME[which]], ev = api.tracegen_riscv_memory_global(which, rec, RT.pad32(int(rec.shape[0])), previous)
                evs.append(ev)
        gev = torch.cat(evs)
        mark()
        count = int(gev.shape[0])
        made["Global"] = api.tracegen_riscv_global(gev, RT.pad32(count))
        digest = X.global_digest(made["Global"], count)
        mark()
        pv = PVM.finalized_state(*ctx.final)
        for which, rec, previous in (("init", recs[0], p_init), ("finalize", recs[1], p_fin)):
            PVM.put(pv, "previous_%s_addr" % which, PVM.addr_limbs(previous))
            PVM.put(pv, "last_%s_addr" % which, PVM.addr_limbs(int(rec[-1, 0]) if rec.shape[0] else previous))
            PVM.put(pv, "global_%s_count" % which, int(rec.shape[0]))
        PVM.set_global(pv, count, digest)
        X._close_device_shard(made, prep, RT.MEMORY_CLUSTER, PVM.to_tensor(pv), ctx, None)
        mark()
        return dict(zip(("upload", "memory_global_kernels", "global_table_and_digest", "lookup_counts"), (b - a for a, b in zip(t, t[1:]))))

    MT_NAME = {"init": "MemoryGlobalInit", "finalize": "MemoryGlobalFinalize"}
    # the untimed round, and the check: the same machine, the same tables, the same public values
    (h_machine, h_chips, h_publics), _ = host()
    d_machine, d_chips, d_publics, _ = device()
    assert [a.name for a, _ in h_machine] == [a.name for a, _ in d_machine] and torch.equal(h_publics, d_publics), "%s: the two paths' public values differ" % name
    heights = {}
    for (a, _, hm, _), (_, _, dm, _) in zip(h_chips, d_chips):
        assert (hm.height, hm.width) == (dm.height, dm.width), a.name
        assert torch.equal(hm.words.view(torch.int32), dm.words.view(torch.int32)), "%s: %s: the device path's table differs from the host path's" % (name, a.name)
        heights[a.name] = hm.height
    device_pieces()
    del h_chips, d_chips
    torch.cuda.empty_cache()
    sec = {"host": [], "device": []}
    h_split, d_split = {}, {}
    for r in range(rounds):
        sync()
        t0 = time.perf_counter()
        got, split = host()
        sec["host"].append(time.perf_counter() - t0)
        for k, v in split.items():
            h_split.setdefault(k, []).append(v)
        del got
        torch.cuda.empty_cache()
        sync()
        t0 = time.perf_counter()
        got = device()
        sec["device"].append(time.perf_counter() - t0)
        del got
        torch.cuda.empty_cache()
        for k, v in device_pieces().items():
            d_split.setdefault(k, []).append(v)
        torch.cuda.empty_cache()
        log("%s: round %d host %.3f s device %.3f s" % (name, r, sec["host"][-1], sec["device"][-1]))
    stat = lambda v: {"median_ms": round(1e3 * statistics.median(v), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)}
    med = {k: statistics.median(v) for k, v in sec.items()}
    out = {"init_rows": int(len(ia)), "finalize_rows": int(len(fa)), "heights": heights, "tables_equal": True, "public_values_equal": True,
           "global_table_rows": heights["Global"], "global_digest_equals_the_hosts": True,
           "host_memory_shard_from_and_to_col_major": dict(stat(sec["host"]), split={k: stat(v) for k, v in h_split.items()}),
           "device_memory_shard": dict(stat(sec["device"]), pieces_timed_apart={k: stat(v) for k, v in d_split.items()}),
           "speedup_median_over_median": round(med["host"] / med["device"], 2)}
    spread = max(sec["host"]) - min(sec["host"])
    ok = med["device"] <= med["host"] + spread
    return out, ok, "%s: device_memory_shard's median (%.3f s) is above the host path's (%.3f s) by more than its spread (%.3f s)" % (
        name, med["device"], med["host"], spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="fibonacci")
    ap.add_argument("--cycles", type=int, default=26_000_000, help="size the guest's input for at least this many cycles")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"bench": "device_memory_shard"}

    def emit():
        line = json.dumps(out)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if not torch.cuda.is_available():
        out.update({"measured": False, "note": "not measured: no GPU in this run, no figure is reported"})
        return emit()

    from core_real import to_col_major
    from program_shard import stdin_of
    from sp1_amd.machines import riscv_exec as X
    torch.cuda.set_device(0)
    log = lambda s: print("bench_device_memory_shard: " + s, file=sys.stderr, flush=True)
    ex = X.Executor(X.guest_file(args.program + ".elf"), stdin=stdin_of(args.program, args.cycles))
    ex.cut_by_area()
    t0 = time.perf_counter()
    shards = [r for r in X.run_records(ex, 1 << 40, core_limit=0) if r.kind == "memory"]     # executed, nothing traced
    log("%s executed in %.1f s: %d memory shard(s)" % (args.program, time.perf_counter() - t0, len(shards)))
    r = shards[0]
    ctx, lists = r.ctx, (r.init_addrs, r.init_recs, r.fin_addrs, r.fin_recs, r.previous_init, r.previous_fin)
    prep = {k: to_col_major(t) for k, t in X.preprocessed_tables(ex, "cuda").items()}
    out.update({"measured": True, "device_name": torch.cuda.get_device_name(0), "rounds": args.rounds, "program": args.program, "cycles_asked": args.cycles,
                "memory_shards_of_the_run": len(shards)})
    failures = []
    n_large = X.split_thresholds(ex.program()[1].shape[0])["memory"]
    for name, ls in (("run", lists), ("synthetic", synthetic_lists(n_large))):
        res, ok, msg = measure(name, ls, ctx, prep, args.rounds, log)
        out[name + "_memory_shard"] = res
        if not ok:
            failures.append(msg)
    emit()
    assert not failures, "; ".join(failures)


if __name__ == "__main__":
    main()
