#!/usr/bin/env python3
"""The two ways a Keccak shard's KeccakPermute / KeccakPermuteControl tables reach the device, at the shard size the reference's
`SplitOpts` gives (riscv_exec.split_thresholds: ~5,000 KECCAK_PERMUTE calls, 1.3 GB of table from 3 MB of events):

  generate   the pinned [n, 77] event records are copied to the device and sp1hip_tracegen_riscv_keccak / _keccak_control make
             the tables there (api.tracegen_riscv_keccak*): timed from the start of the event copy to the end of the second kernel;
  stage      the host-made row-major tables of the same shard (riscv_more_trace.keccak_permute_table / keccak_control_table,
             Montgomery words, pinned) go through sp1hip_stage_tables (PCIe copy + on-GPU transpose).

The two alternate in ONE process, each on the same stream; medians of 5 with min and max, after one untimed round of both. The
device tables are compared with the staged ones word for word first. One JSON line; `--out` also writes it to a file. Without a
GPU the line says so and holds no figure.

  python bench/bench_tracegen_keccak.py [--program rsp] [--events N] [--out profiles/keccak_tracegen_bench.json]
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

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="rsp", help="the guest whose Program table sets the shard size (split_thresholds)")
    ap.add_argument("--events", type=int, default=0, help="KECCAK_PERMUTE calls in the shard (0 = the split threshold)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from sp1_amd.machines import riscv_exec as X, riscv_more_trace as MT, riscv_trace as RT
    n = args.events or X.split_thresholds(X.Executor(X.guest_file(args.program + ".elf")).program()[1].shape[0])["keccak"]
    out = {"bench": "keccak_tracegen", "events": n, "shard_size_from": "split_thresholds(%s)" % args.program if not args.events else "--events"}

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
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    I64 = torch.int64
    # the shard's calls (as riscv_more_trace.precompile_shard draws them) and its host-made tables
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    clk0 = (5 << 24) + 1001
    clk = clk0 + 320 * torch.arange(n, device=dev)
    addr = 0x20_0000 + 256 * torch.randperm(4 * n + 4, generator=gen, device=dev)[:n]
    pre = torch.randint(RT.MIN64, (1 << 63) - 1, (n, 25), generator=gen, device=dev, dtype=I64)
    t_prev = torch.randint(1, clk0 - 8, (n, 25), generator=gen, device=dev, dtype=I64)
    kp, post = MT.keccak_permute_table(clk, addr, pre, dev)
    ct, _ = MT.keccak_control_table(clk, addr, pre, t_prev, post, dev)
    monty = lambda t: ((t << 32) % RT.P).to(torch.int32)
    hosts = [monty(kp.main).cpu().pin_memory(), monty(ct.main).cpu().pin_memory()]
    heights = [int(h.shape[0]) for h in hosts]
    events = torch.zeros((n, 77), dtype=I64, device=dev)
    events[:, 0], events[:, 1] = clk, addr
    events[:, 2:52:2], events[:, 3:52:2], events[:, 52:] = t_prev, pre, post
    events = events.cpu().pin_memory()
    del kp, ct, pre, t_prev, post
    torch.cuda.empty_cache()
    table_bytes, event_bytes = 4 * sum(h.numel() for h in hosts), 8 * events.numel()

    stream = torch.cuda.Stream()

    def generate():
        with torch.cuda.stream(stream):
            ev = events.to(dev, non_blocking=True)
            tabs = (api.tracegen_riscv_keccak(ev, heights[0], stream=stream), api.tracegen_riscv_keccak_control(ev, heights[1], stream=stream))
        stream.synchronize()
        return tabs

    def stage():
        with torch.cuda.stream(stream):
            tabs = api.stage_tables(hosts, stream=stream)
        stream.synchronize()
        return tabs

    made, staged = generate(), stage()                       # the untimed round: allocator and arena warm, and the check
    for g, s in zip(made, staged):
        assert (g.width, g.height) == (s.width, s.height) and torch.equal(g.words, s.words), "device tables differ from the staged host tables"
    del made, staged
    ms = {"generate": [], "stage": []}
    for _ in range(args.rounds):
        for name, fn in (("generate", generate), ("stage", stage)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tabs = fn()
            ms[name].append(1e3 * (time.perf_counter() - t0))
            del tabs
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}
    g, s = stat(ms["generate"]), stat(ms["stage"])
    out.update({"measured": True, "device": torch.cuda.get_device_name(0), "rows": {"KeccakPermute": heights[0], "KeccakPermuteControl": heights[1]},
                "table_bytes": table_bytes, "event_bytes": event_bytes, "rounds": args.rounds, "tables_equal_word_for_word": True,
                "generate_from_pinned_events": g, "stage_host_tables": s,
                "generate_table_write_gb_per_s": round(table_bytes / (g["median_ms"] * 1e-3) / 1e9, 1),
                "stage_gb_per_s": round(table_bytes / (s["median_ms"] * 1e-3) / 1e9, 1),
                # the requirement: generation is not slower than staging beyond the staging yardstick's own min-max spread
                "generate_not_slower_than_stage_beyond_its_spread": bool(g["median_ms"] <= s["median_ms"] + (s["max_ms"] - s["min_ms"]))})
    emit()
    assert out["generate_not_slower_than_stage_beyond_its_spread"], "device generation is slower than staging the host tables"


if __name__ == "__main__":
    main()
