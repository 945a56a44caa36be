#!/usr/bin/env python3
"""The two ways the tables of the nine load and store chips (LoadByte, LoadHalf, LoadWord, LoadDouble, LoadX0, StoreByte, StoreHalf,
StoreWord, StoreDouble) reach the device, at the row counts of the reference's recorded core shard (riscv.RECORDED_ROWS: 2,573,984
rows, 111 M cells in all):

  generate   the pinned [n, 12] event records (96 bytes each) are copied to the device and sp1hip_tracegen_riscv_mem makes the nine
             tables there (api.tracegen_riscv_mem): timed from the start of the first event copy to the end of the last kernel;
  stage      the host-made row-major tables of the same rows (Tracer.fill_mem_chip driven by EventTracer.memory_instructions,
             Montgomery words, pinned) go through sp1hip_stage_tables (PCIe copy + on-GPU transpose). This is unchanged code: the
             path these tables took before.

The events are the memory events of a real guest's first shard, each chip's repeated to its recorded row count (a row is a function
of its own event alone). The two alternate in ONE process, each on the same stream; medians of 5 with min and max, after one
untimed round of both, for the nine chips together and for each alone. The device tables are compared with the staged ones word for
word first. The host filler's own seconds for those rows are recorded beside them (not asserted on). One JSON line; `--out` also
writes it to a file. Without a GPU the line says so and holds no figure.

  python bench/bench_tracegen_mem.py [--program rsp] [--out profiles/riscv_mem_tracegen_bench.json]
"""
import argparse
import copy
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

CHIPS = ("LoadByte", "LoadHalf", "LoadWord", "LoadDouble", "LoadX0", "StoreByte", "StoreHalf", "StoreWord", "StoreDouble")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="rsp", help="the guest whose first shard's events are repeated (it needs all nine kinds)")
    ap.add_argument("--cycles", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from program_shard import stdin_of
    from sp1_amd.machines import riscv as R, riscv_exec as X, riscv_trace as RT
    rows = {n: R.RECORDED_ROWS[n] for n in CHIPS}
    out = {"bench": "riscv_mem_tracegen", "chips": list(CHIPS), "rows": rows, "events_from": "%s, first shard of %d cycles, repeated" % (args.program, args.cycles)}

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
    ex = X.Executor(X.guest_file(args.program + ".elf"), stdin=stdin_of(args.program, 2 * args.cycles))
    shard = ex.run_shard(args.cycles)
    names_of = X.chip_of_events(shard.events)
    picked = []
    for n in CHIPS:
        own = shard.events[np.nonzero(names_of == n)[0]]
        assert len(own), "the guest's shard has no %s instruction" % n
        picked.append(own[np.arange(rows[n]) % len(own)])
    out["distinct_events"] = {n: int((names_of == n).sum()) for n in CHIPS}
    repeated = copy.copy(shard)
    repeated.events = np.concatenate(picked)

    # the host filler over exactly these rows: the tracer's memory_instructions alone, without the rest of a shard around it
    tracer = X.EventTracer(ex, repeated, "cpu")
    t0 = time.perf_counter()
    tracer.memory_instructions()
    host_fill_seconds = time.perf_counter() - t0
    tables = tracer.tables
    assert set(tables) == set(CHIPS) and all(tables[n].main.shape[0] == rows[n] for n in CHIPS)
    monty = lambda t: ((t << 32) % RT.P).to(torch.int32)
    hosts = {n: monty(tables[n].main).pin_memory() for n in CHIPS}
    events = {n: torch.as_tensor(np.ascontiguousarray(X.pack_mem_events(repeated.events, n))).pin_memory() for n in CHIPS}
    del tables, tracer
    stream = torch.cuda.Stream()

    def generate(chips):
        with torch.cuda.stream(stream):
            tabs = [api.tracegen_riscv_mem(n, events[n].to(dev, non_blocking=True), rows[n], stream=stream) for n in chips]
        stream.synchronize()
        return tabs

    def stage(chips):
        with torch.cuda.stream(stream):
            tabs = api.stage_tables([hosts[n] for n in chips], stream=stream)
        stream.synchronize()
        return tabs

    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}

    def measure(chips):
        made, staged = generate(chips), stage(chips)         # the untimed round: allocator and arena warm, and the check
        for n, g, s in zip(chips, made, staged):
            assert (g.width, g.height) == (s.width, s.height) and torch.equal(g.words, s.words), "%s: the device table differs from the staged host table" % n
        del made, staged
        ms = {"generate": [], "stage": []}
        for _ in range(args.rounds):
            for name, fn in (("generate", generate), ("stage", stage)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tabs = fn(chips)
                ms[name].append(1e3 * (time.perf_counter() - t0))
                del tabs
        g, s = stat(ms["generate"]), stat(ms["stage"])
        table_bytes, event_bytes = 4 * sum(hosts[n].numel() for n in chips), 8 * sum(events[n].numel() for n in chips)
        return {"table_bytes": table_bytes, "event_bytes": event_bytes, "generate_from_pinned_events": g, "stage_host_tables": s,
                # the requirement: generation is not slower than staging beyond the staging yardstick's own min-max spread
                "generate_not_slower_than_stage_beyond_its_spread": bool(g["median_ms"] <= s["median_ms"] + (s["max_ms"] - s["min_ms"]))}

    out.update({"measured": True, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "tables_equal_word_for_word": True,
                "host_fill_seconds": round(host_fill_seconds, 3), "all_nine": measure(list(CHIPS)), "per_chip": {n: measure([n]) for n in CHIPS}})
    emit()
    assert out["all_nine"]["generate_not_slower_than_stage_beyond_its_spread"], "device generation of the nine tables is slower than staging the host tables"


if __name__ == "__main__":
    main()
