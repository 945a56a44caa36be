#!/usr/bin/env python3
"""What it costs to turn one executed core shard into the tables the prover takes, two ways, on one full fibonacci core shard cut as
bench/prove_program.py cuts it (by trace area, the reference's rule):

  host    the path every core shard took so far: riscv_exec.EventTracer(...).build() on `cuda` (torch: the events are sorted with
          chip_of_events on the host, every table is filled by the tracer's fillers) plus core_real.to_col_major of every main table;
  device  riscv_exec.device_core_shard: the events and the local-memory records are uploaded as they are (pageable memory: the
          executor's buffer is neither pinned nor registered), the partition kernel routes and packs them, every table is made by a
          kernel, the lookup tables are counted on the device. No EventTracer.

The two alternate in ONE process; medians of --rounds (5) with min and max, after one untimed round of both. Reported apart for the
device path: the upload of the raw events, the partition alone on resident events (with the bytes its kernels REQUEST per second: the
count pass loads 80 of an event's 160 bytes, the scatter pass all of them, every record is written once — what the cache lines
fetch was not measured), and everything behind the upload (partition + tables + counts) on resident events. The tables of
the two paths are compared first (every chip but MemoryBump word for word; MemoryBump as a multiset of rows). ONE assertion: the
device path's median is not above the host path's minimum. One JSON line; `--out` also writes it to a file. Without a GPU the line
says so and holds no figure.

  python bench/bench_device_shard.py [--cycles 26000000] [--out profiles/device_core_shard_bench.json]
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

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="fibonacci")
    ap.add_argument("--cycles", type=int, default=26_000_000, help="size the guest's input for at least this many cycles: its first shard is a full one")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    out = {"bench": "device_core_shard", "shard_from": "%s, first core shard cut by trace area" % args.program}

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
    from sp1_amd import api
    from sp1_amd.machines import riscv_exec as X
    torch.cuda.set_device(0)
    ex = X.Executor(X.guest_file(args.program + ".elf"), stdin=stdin_of(args.program, args.cycles))
    ex.cut_by_area()
    shard = ex.run_shard(1 << 40)
    n = int(shard.events.shape[0])
    out.update({"events": n, "cycles": shard.cycles, "halted": shard.halted, "event_bytes": int(shard.events.nbytes), "local_records": int(shard.local.shape[0])})
    print("bench_device_shard: %d events, %d cycles" % (n, shard.cycles), file=sys.stderr, flush=True)
    prep = {k: to_col_major(t) for k, t in X.preprocessed_tables(ex, "cuda").items()}
    sync = torch.cuda.synchronize

    def host():
        machine, tabs, publics = X.EventTracer(ex, shard, "cuda").build()
        chips = [(a, i, to_col_major(tabs[a.name][1]), prep.get(a.name)) for a, i in machine]
        sync()
        return machine, chips, publics

    def device():
        made = X.device_core_shard(ex, shard, prep)
        sync()
        return made

    def upload():
        ev = torch.as_tensor(shard.events).cuda()
        sync()
        return ev

    resident = copy.copy(shard)
    resident.events, resident.local = upload(), torch.as_tensor(shard.local).cuda()

    def partition():
        parts = api.partition_rv64_events(resident.events)
        sync()
        return parts

    def from_resident():
        made = X.device_core_shard(ex, resident, prep)
        sync()
        return made

    # the untimed round, and the check: the same machine, the same tables, the same public values
    (h_machine, h_chips, h_publics), (d_machine, d_chips, d_publics, _) = host(), device()
    assert [a.name for a, _ in h_machine] == [a.name for a, _ in d_machine] and torch.equal(h_publics, d_publics)
    for (a, _, hm, _), (_, _, dm, _) in zip(h_chips, d_chips):
        assert (hm.height, hm.width) == (dm.height, dm.width), a.name
        if a.name == "MemoryBump" and hm.height:
            order = lambda t: sorted(map(tuple, t.words.view(t.width, t.height).T.cpu().tolist()))
            assert order(hm) == order(dm), "MemoryBump: the two paths' rows differ as multisets"
        else:
            assert torch.equal(hm.words, dm.words), "%s: the device path's table differs from the host path's" % a.name
    parts = partition()
    record_bytes = 8 * sum(int(p.numel()) for p in parts.values())
    partition_bytes = int(shard.events.nbytes) // 2 + int(shard.events.nbytes) + record_bytes      # requested: 80 + 160 bytes an event, + the records
    del h_chips, d_chips, parts
    torch.cuda.empty_cache()

    sec = {k: [] for k in ("host", "device", "upload_events", "partition", "device_from_resident_events")}
    for r in range(args.rounds):
        for what, fn in (("host", host), ("device", device), ("upload_events", upload), ("partition", partition), ("device_from_resident_events", from_resident)):
            sync()
            t0 = time.perf_counter()
            got = fn()
            sec[what].append(time.perf_counter() - t0)
            del got
            torch.cuda.empty_cache()
        print("bench_device_shard: round %d host %.3f s device %.3f s" % (r, sec["host"][-1], sec["device"][-1]), file=sys.stderr, flush=True)
    stat = lambda v: {"median_ms": round(1e3 * statistics.median(v), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3),
                      "all_ms": [round(1e3 * x, 3) for x in v]}
    med = {k: statistics.median(v) for k, v in sec.items()}
    out.update({"measured": True, "device_name": torch.cuda.get_device_name(0), "rounds": args.rounds, "tables_equal": True,
                "host_tracer_build_and_to_col_major": stat(sec["host"]), "device_core_shard": stat(sec["device"]),
                "upload_events_pageable": dict(stat(sec["upload_events"]), bytes=int(shard.events.nbytes),
                                               gb_per_s=round(shard.events.nbytes / med["upload_events"] / 1e9, 2)),
                "partition_alone": dict(stat(sec["partition"]), bytes_requested=partition_bytes, record_bytes=record_bytes,
                                        requested_gb_per_s=round(partition_bytes / med["partition"] / 1e9, 1), events_per_s=round(n / med["partition"])),
                "device_core_shard_from_resident_events": stat(sec["device_from_resident_events"]),
                "tables_and_counts_ms_resident_minus_partition": round(1e3 * (med["device_from_resident_events"] - med["partition"]), 3),
                "cycles_per_s": {"host": round(shard.cycles / med["host"]), "device": round(shard.cycles / med["device"])},
                "speedup_median_over_median": round(med["host"] / med["device"], 2)})
    emit()
    assert med["device"] <= min(sec["host"]), "device_core_shard's median (%.3f s) is above the host path's minimum (%.3f s)" % (med["device"], min(sec["host"]))


if __name__ == "__main__":
    main()
