#!/usr/bin/env python3
"""The two ways the chip tables of a SHA_EXTEND / SHA_COMPRESS shard reach the device, for each kind at the shard size the
reference's `SplitOpts` gives (riscv_exec.split_thresholds: a full shard's calls), on events synthesized by tests/sha_cases.py:

  device   the pinned [n, 786 / 155] event records are copied to the device and the kind's two kernels make the tables there
           (api.tracegen_riscv_sha_extend / _sha_extend_control, _sha_compress / _sha_compress_control): timed from the start of
           the event copy to the end of the second kernel;
  host     the host builder (riscv_more_trace.sha_extend_shard_from / sha_compress_shard_from, vectorised torch on the device, as
           bench/prove_program.py runs it) makes the kind's two tables — what it would go on to build around them, SyscallPrecompile,
           MemoryLocal, Global and the lookup counts, is cut off: both paths share it — and core_real.to_col_major stages them.

The two alternate in ONE process; medians of 5 with min and max, after one untimed round of both. The device tables are compared
with the host ones word for word first. One JSON line; `--out` also writes it to a file. Without a GPU the line says so and holds
no figure.

  python bench/bench_tracegen_sha.py [--program rsp] [--events N] [--out profiles/sha256_tracegen_bench.json]
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

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="rsp", help="the guest whose Program table sets the shard size (split_thresholds)")
    ap.add_argument("--events", type=int, default=0, help="calls in the shard (0 = the kind's split threshold)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from sp1_amd.machines import riscv_exec as X, riscv_more_trace as MT, riscv_trace as RT
    limits = X.split_thresholds(X.Executor(X.guest_file(args.program + ".elf")).program()[1].shape[0])
    out = {"bench": "sha256_tracegen", "shard_size_from": "split_thresholds(%s)" % args.program if not args.events else "--events", "kinds": {}}

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
    import sha_cases as S
    from sp1_amd import api
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}
    out.update({"measured": True, "device": torch.cuda.get_device_name(0), "rounds": args.rounds})
    for kind in S.KINDS:
        n = args.events or limits[kind]
        chip, control = S.CHIPS[kind]
        heights = (RT.pad32(S.ROWS_PER_CALL[chip] * n), RT.pad32(n))
        events = torch.as_tensor(S.events(kind, n)).pin_memory()
        on_device = events.to(dev)
        builder = MT.sha_extend_shard_from if kind == "sha_extend" else MT.sha_compress_shard_from

        def device_path():
            with torch.cuda.stream(stream):
                ev = events.to(dev, non_blocking=True)
                tabs = (api.tracegen_riscv_records(chip, ev, heights[0], stream=stream), api.tracegen_riscv_records(control, ev, heights[1], stream=stream))
            stream.synchronize()
            return tabs

        def host_path():
            made = {}

            def two_tables(tr, *a, **k):                        # the builder's call of _close_precompile_shard: keep the two tables, stop
                made.update({name: tr.tables[name].main for name in (chip, control)})
            closing, MT._close_precompile_shard = MT._close_precompile_shard, two_tables
            try:
                builder(on_device, dev)
            finally:
                MT._close_precompile_shard = closing
            tabs = (core_real.to_col_major(made[chip]), core_real.to_col_major(made[control]))
            torch.cuda.synchronize()
            return tabs

        made, staged = device_path(), host_path()               # the untimed round: allocator warm, and the check
        for g, s in zip(made, staged):
            assert (g.width, g.height) == (s.width, s.height) and torch.equal(g.words, s.words), "device tables differ from the host builder's"
        table_bytes = 4 * sum(g.words.numel() for g in made)
        del made, staged
        ms = {"device": [], "host": []}
        for _ in range(args.rounds):
            for name, fn in (("device", device_path), ("host", host_path)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tabs = fn()
                ms[name].append(1e3 * (time.perf_counter() - t0))
                del tabs
        d, h = stat(ms["device"]), stat(ms["host"])
        out["kinds"][kind] = {"events": n, "rows": {chip: heights[0], control: heights[1]}, "table_bytes": table_bytes, "event_bytes": 8 * events.numel(),
                              "tables_equal_word_for_word": True, "device_from_pinned_events": d, "host_builder_and_staging": h,
                              "device_table_write_gb_per_s": round(table_bytes / (d["median_ms"] * 1e-3) / 1e9, 1),
                              "host_over_device": round(h["median_ms"] / d["median_ms"], 1)}
        del events, on_device
        torch.cuda.empty_cache()
    emit()


if __name__ == "__main__":
    main()
