#!/usr/bin/env python3
"""The two ways a secp256k1 shard's Secp256k1AddAssign / Secp256k1DoubleAssign table reaches the device, at the sizes of the two
shards of the `rsp` block (profiles/r06_rsp_block_final.json: 26,880 additions, 53,760 doublings), on events drawn as multiples of G:

  generate   the pinned [n, 43] / [n, 26] event records are copied to the device and sp1hip_tracegen_riscv_secp256k1_add / _double
             makes the table there (api.tracegen_riscv_secp256k1_*): timed from the start of the event copy to the end of the kernel;
  parent     what the parent commit does for the same table: the host filler (riscv_more_trace.secp256k1_add_table / _double_table:
             Python integers, one row at a time) — timed on its own, on the CPU — and then sp1hip_stage_tables of the finished
             row-major table (Montgomery words, pinned: PCIe copy + on-GPU transpose).

generate and the staging half of parent alternate in ONE process on the same stream, medians of `--rounds` with min and max after
one untimed round of both; the filler runs `--filler-rounds` times. The device table is compared with the staged one word for
word first. No target is asserted. One JSON line; `--out` also writes it to a file. Without a GPU the line says so and holds no figure.

  python bench/bench_tracegen_secp.py [--add 26880] [--double 53760] [--out profiles/secp256k1_tracegen_bench.json]
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

M64 = (1 << 64) - 1


def draw_events(n_add, n_double):
    """Event records on consecutive multiples of G: addition i is (i + 1) G + (i + 2) G, doubling i is 2 (i + 1) G."""
    from sp1_amd.machines import riscv_more as M
    p_mod = M.SECP256K1_P
    g = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)

    def add(p, q):
        lam = (3 * p[0] * p[0] * pow(2 * p[1], p_mod - 2, p_mod) if p == q else (q[1] - p[1]) * pow(q[0] - p[0], p_mod - 2, p_mod)) % p_mod
        x = (lam * lam - p[0] - q[0]) % p_mod
        return x, (lam * (p[0] - x) - p[1]) % p_mod
    words = lambda pt: [(c >> (64 * i)) & M64 for c in pt for i in range(4)]
    mg = [g]
    for _ in range(max(n_add + 1, n_double)):
        mg.append(add(mg[-1], g))
    rng = np.random.default_rng(1)
    clk0 = (5 << 24) + 1001

    def rows(n, reads, operands, result):
        clk = clk0 + 320 * np.arange(n, dtype=np.int64)
        ptr = 0x20_0000 + 256 * rng.permutation(8 * n + 8)[:2 * n].reshape(n, 2).astype(np.int64)
        t_prev = rng.integers(1, clk0 - 8, size=(n, reads), dtype=np.int64)
        out = []
        for i in range(n):
            vals = [w for pt in operands(i) for w in words(pt)]
            row = [int(clk[i])] + [int(v) for v in ptr[i, :reads // 8]]
            for k in range(reads):
                row += [int(t_prev[i, k]), vals[k]]
            out.append(row + words(result(i)))
        return np.array(out, dtype=np.uint64).reshape(n, 1 + reads // 8 + 2 * reads + 8).view(np.int64)
    ev_add = rows(n_add, 16, lambda i: (mg[i], mg[i + 1]), lambda i: add(mg[i], mg[i + 1]))
    ev_double = rows(n_double, 8, lambda i: (mg[i],), lambda i: add(mg[i], mg[i]))
    return {"add": ev_add, "double": ev_double}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--add", type=int, default=26880, help="SECP256K1_ADD calls in the shard (the rsp block's: 26,880)")
    ap.add_argument("--double", type=int, default=53760, help="SECP256K1_DOUBLE calls in the shard (the rsp block's: 53,760)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--filler-rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"bench": "secp256k1_tracegen", "events": {"add": args.add, "double": args.double}, "events_drawn_as": "consecutive multiples of G"}

    def emit():
        line = json.dumps(out)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if not torch.cuda.is_available():
        out.update({"measured": False, "note": "no GPU in this run: nothing was measured, no figure is reported"})
        return emit()

    from sp1_amd import api
    from sp1_amd.machines import riscv_more_trace as MT, riscv_trace as RT
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    events = draw_events(args.add, args.double)
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}
    stream = torch.cuda.Stream()
    out.update({"measured": True, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "filler_rounds": args.filler_rounds})
    for kind, build in (("add", MT.secp256k1_add_table), ("double", MT.secp256k1_double_table)):
        ev = events[kind]
        n = ev.shape[0]
        fill_s = []
        for _ in range(args.filler_rounds):                      # the parent's first half: the host filler, on the CPU
            t0 = time.perf_counter()
            tb = build(ev, torch.device("cpu"))[0]
            fill_s.append(time.perf_counter() - t0)
        host = torch.from_numpy(RT.to_monty_np(tb.main).view(np.int32)).pin_memory()
        height = int(host.shape[0])
        pinned = torch.from_numpy(np.ascontiguousarray(ev)).pin_memory()
        fn = {"add": api.tracegen_riscv_secp256k1_add, "double": api.tracegen_riscv_secp256k1_double}[kind]
        del tb

        def generate():
            with torch.cuda.stream(stream):
                table = fn(pinned.to(dev, non_blocking=True), height, stream=stream)
            stream.synchronize()
            return table

        def stage():
            with torch.cuda.stream(stream):
                tabs = api.stage_tables([host], stream=stream)
            stream.synchronize()
            return tabs[0]

        made, staged = generate(), stage()                       # the untimed round: allocator and arena warm, and the check
        assert (made.width, made.height) == (staged.width, staged.height) and torch.equal(made.words, staged.words), \
            "the device table differs from the staged host table"
        del made, staged
        ms = {"generate": [], "stage": []}
        for _ in range(args.rounds):
            for name, f in (("generate", generate), ("stage", stage)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t = f()
                ms[name].append(1e3 * (time.perf_counter() - t0))
                del t
        g, s, fl = stat(ms["generate"]), stat(ms["stage"]), stat(fill_s)
        out[kind] = {"rows": height, "events": n, "table_bytes": 4 * host.numel(), "event_bytes": 8 * int(ev.size), "table_equal_word_for_word": True,
                     "generate_from_pinned_events_ms": g, "parent_host_filler_s": fl, "parent_stage_host_table_ms": s,
                     "parent_total_ms": round(1e3 * fl["median"] + s["median"], 3),
                     "generate_table_write_gb_per_s": round(4 * host.numel() / (g["median"] * 1e-3) / 1e9, 1)}
        del host, pinned
    emit()


if __name__ == "__main__":
    main()
