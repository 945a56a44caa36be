#!/usr/bin/env python3
"""The two ways the chip table of an ed_add, ed_decompress or uint256_ops precompile shard reaches the device, at the shard size the
reference's `SplitOpts` gives (riscv_exec.split_thresholds: a full shard's calls), on the events of tests/ed_u256_cases.py repeated
to that size:

  device   the pinned [n, words] event records are copied to the device and api.tracegen_riscv_ed_add / _ed_decompress /
           _uint256_ops makes the table there — for the two Edwards chips the work buffer's allocation, phase A and phase B —: timed
           from the start of the event copy to the end of the last kernel;
  host     the parent path for the same table: riscv_more_trace.family_shard_from's chip filler (Python integers per field
           operation, numpy for the witnesses) — what it would go on to build around it, SyscallPrecompile, MemoryLocal, Global and
           the lookup counts, is cut off: both paths share it — and core_real.to_col_major stages it. A full shard takes that filler
           minutes, so it is timed on the FIRST 1 / --host-fraction of the rows (default 1 / 16) and the time is scaled by the
           fraction: the filler's cost is per row (every row is an event; no padding). Both figures are reported.

The two alternate in ONE process; medians of 5 with min and max, after one untimed round of both. The device table of the
fraction's events is compared with the host one word for word first. No target is asserted. One JSON line; `--out` also writes it
to a file. Without a GPU the line says so and holds no figure.

  python bench/bench_tracegen_ed_uint256_ops.py [--program fibonacci] [--events N] [--out profiles/ed_uint256_ops_tracegen_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

KINDS = ("ed_add", "ed_decompress", "uint256_ops")
WORK_WORDS_PER_ROW = {"ed_add": 8 * 40, "ed_decompress": 7 * 25, "uint256_ops": 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="fibonacci", help="the guest whose Program table sets the shard size (split_thresholds)")
    ap.add_argument("--events", type=int, default=0, help="calls in the shard (0 = the kind's split threshold)")
    ap.add_argument("--host-fraction", type=int, default=16, help="the host filler is timed on 1 / this many of the rows")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from sp1_amd.machines import riscv_exec as X, riscv_trace as RT
    limits = X.split_thresholds(X.Executor(X.guest_file(args.program + ".elf")).program()[1].shape[0])
    out = {"bench": "ed_uint256_ops_tracegen", "shard_size_from": "split_thresholds(%s)" % args.program if not args.events else "--events", "kinds": {}}

    def emit():
        line = json.dumps(out)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if not torch.cuda.is_available():
        out.update({"measured": False, "note": "no GPU in this run: nothing was measured, no figure is reported"})
        return emit()

    import core_real
    import ed_u256_cases as C
    from sp1_amd import api
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}
    out.update({"measured": True, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "host_fraction": "1/%d of the rows, scaled" % args.host_fraction})
    for kind in KINDS:
        n = args.events or limits[kind]
        chip, height = C.CHIPS[kind], RT.pad32(n)
        base = C.events(kind, 300)
        host_events = np.ascontiguousarray(base[np.arange(n) % len(base)])
        part = np.ascontiguousarray(host_events[:max(n // args.host_fraction, 1)])
        events = torch.as_tensor(host_events).pin_memory()
        make = getattr(api, "tracegen_riscv_" + kind)

        def device_path(ev=events, rows=height):
            with torch.cuda.stream(stream):
                table = make(ev.to(dev, non_blocking=True), rows, stream=stream)
            stream.synchronize()
            return table

        def host_path():
            table = core_real.to_col_major(C.filler(kind, part, dev)[0])
            torch.cuda.synchronize()
            return table

        made, staged = device_path(torch.as_tensor(part), RT.pad32(len(part))), host_path()      # the check, on the fraction's events
        assert (made.width, made.height) == (staged.width, staged.height) and torch.equal(made.words, staged.words), "device table differs from the host filler's"
        made = device_path()                                    # the untimed round of the full size: allocator warm
        table_bytes = 4 * made.words.numel()
        del made, staged
        ms = {"device": [], "host": []}
        for _ in range(args.rounds):
            for name, fn in (("device", device_path), ("host", host_path)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                table = fn()
                ms[name].append(1e3 * (time.perf_counter() - t0))
                del table
        d, h = stat(ms["device"]), stat(ms["host"])
        scale = n / len(part)
        out["kinds"][kind] = {"events": n, "rows": {chip: height}, "table_bytes": table_bytes, "event_bytes": 8 * events.numel(),
                              "work_buffer_bytes": 4 * WORK_WORDS_PER_ROW[kind] * height, "table_equal_word_for_word_on_the_fraction": True,
                              "device_from_pinned_events": d, "host_rows_timed": len(part), "host_filler_and_staging_on_the_fraction": h,
                              "host_filler_and_staging_scaled_ms": round(h["median_ms"] * scale, 1),
                              "device_table_write_gb_per_s": round(table_bytes / (d["median_ms"] * 1e-3) / 1e9, 1),
                              "host_scaled_over_device": round(h["median_ms"] * scale / d["median_ms"], 1)}
        del events
        torch.cuda.empty_cache()
    emit()


if __name__ == "__main__":
    main()
