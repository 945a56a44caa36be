#!/usr/bin/env python3
"""The two ways the chip table of a POSEIDON2 / UINT256_MUL shard reaches the device, for each kind at the shard size the reference's
`SplitOpts` gives (riscv_exec.split_thresholds: a full shard's calls), on the events of tests/p2u_cases.py repeated to that size:

  device   the pinned [n, 26 / 31] event records are copied to the device and the kind's kernel makes the table there
           (api.tracegen_riscv_poseidon2 / _uint256_mul): timed from the start of the event copy to the end of the kernel;
  host     the host builder (riscv_more_trace.poseidon2_shard_from: vectorised torch on the device; uint256_shard_from: a Python
           loop over the rows, then torch — as riscv_exec.host_shard and bench/prove_program.py run them) makes the kind's table —
           what it would go on to build around it, SyscallPrecompile, MemoryLocal, Global and the lookup counts, is cut off: both
           paths share it — and core_real.to_col_major stages it.

The two alternate in ONE process; medians of 5 with min and max, after one untimed round of both. The device table is compared
with the host one word for word first. One JSON line; `--out` also writes it to a file. Without a GPU the line says so and holds
no figure.

  python bench/bench_tracegen_p2u.py [--program poseidon2] [--events N] [--out profiles/poseidon2_uint256_tracegen_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="poseidon2", help="the guest whose Program table sets the shard size (split_thresholds)")
    ap.add_argument("--events", type=int, default=0, help="calls in the shard (0 = the kind's split threshold)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from sp1_amd.machines import riscv_exec as X, riscv_more_trace as MT, riscv_trace as RT
    limits = X.split_thresholds(X.Executor(X.guest_file(args.program + ".elf")).program()[1].shape[0])
    out = {"bench": "poseidon2_uint256_tracegen", "shard_size_from": "split_thresholds(%s)" % args.program if not args.events else "--events", "kinds": {}}

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
    import p2u_cases as C
    from sp1_amd import api
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}
    out.update({"measured": True, "device": torch.cuda.get_device_name(0), "rounds": args.rounds})
    for kind in C.KINDS:
        n = args.events or limits[kind]
        chip, height = C.CHIPS[kind], RT.pad32(n)
        base = C.events(kind, C.N_EVENTS, start=0)
        host_events = np.ascontiguousarray(base[np.arange(n) % len(base)])
        events = torch.as_tensor(host_events).pin_memory()

        def device_path():
            with torch.cuda.stream(stream):
                table = api.tracegen_riscv_records(chip, events.to(dev, non_blocking=True), height, stream=stream)
            stream.synchronize()
            return table

        def host_path():
            made = {}

            def one_table(tr, *a, **k):                         # the builder's call of _close_precompile_shard: keep the table, stop
                made[chip] = tr.tables[chip].main
            closing, MT._close_precompile_shard = MT._close_precompile_shard, one_table
            try:
                if kind == "uint256":
                    MT.uint256_shard_from(host_events, dev)
                else:
                    t = torch.as_tensor(host_events).to(dev)
                    rd = t[:, 2:18].reshape(-1, 8, 2)
                    MT.poseidon2_shard_from(t[:, 0], t[:, 1], rd[:, :, 1].contiguous(), rd[:, :, 0].contiguous(), t[:, 18:26].contiguous(), dev)
            finally:
                MT._close_precompile_shard = closing
            table = core_real.to_col_major(made[chip])
            torch.cuda.synchronize()
            return table

        made, staged = device_path(), host_path()               # the untimed round: allocator warm, and the check
        assert (made.width, made.height) == (staged.width, staged.height) and torch.equal(made.words, staged.words), "device table differs from the host builder's"
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
        out["kinds"][kind] = {"events": n, "rows": {chip: height}, "table_bytes": table_bytes, "event_bytes": 8 * events.numel(),
                              "table_equal_word_for_word": True, "device_from_pinned_events": d, "host_builder_and_staging": h,
                              "device_table_write_gb_per_s": round(table_bytes / (d["median_ms"] * 1e-3) / 1e9, 1),
                              "host_over_device": round(h["median_ms"] / d["median_ms"], 1)}
        del events
        torch.cuda.empty_cache()
    emit()


if __name__ == "__main__":
    main()
