#!/usr/bin/env python3
"""The two ways the Byte, Range and Program multiplicities of a core shard are counted, over the tables of one executed shard of a
real guest, all of them already in device memory:

  device   riscv_exec.device_lookup_tables: sp1hip_lookup_count_sends over every chip's column-major table, the public values' row,
           sp1hip_lookup_count_program over the event matrix, sp1hip_lookup_counts_finish — timed to the end of the finish call,
           which synchronises;
  torch    Tracer.byte_range_tables over the same shard's canonical tables (every chip's byte sends evaluated with torch and tallied
           by sort and prefix sum) plus the bincount of the executed pcs that program_table makes. This is unchanged code: the path
           these three tables took before, run with torch on the same GPU.

The two do not walk exactly the same rows: the torch path evaluates each table's real rows only (`tbl.main[:tbl.n]`) where the
device path counts every padded row (padding rows send with multiplicity 0), and the torch path, run again on a built tracer, also
walks the Byte, Range and Program tables as senders, which have no byte sends. The results are compared word for word all the same.

The two alternate in ONE process; medians of 5 with min and max, after one untimed round of both in which the results are compared
word for word. Recorded beside them: the byte messages counted, messages per second of the device path, and the share of all
messages that went to the hottest cell. One JSON line; `--out` also writes it to a file. Without a GPU the line says so and holds no
figure.

  python bench/bench_lookup_counts.py [--program rsp] [--cycles 1048576] [--out profiles/lookup_counts_bench.json]
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

COUNTED = ("Byte", "Range", "Program")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="rsp")
    ap.add_argument("--cycles", type=int, default=1 << 20, help="length of the guest's first shard")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from program_shard import stdin_of
    from sp1_amd.machines import riscv_exec as X, riscv_trace as RT
    out = {"bench": "lookup_counts", "tables_from": "%s, first shard of %d cycles" % (args.program, args.cycles)}

    def emit():
        line = json.dumps(out)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if not torch.cuda.is_available():
        out.update({"measured": False, "note": "no GPU in this run: nothing was measured, no figure is reported"})
        return emit()

    from core_real import to_col_major
    torch.cuda.set_device(0)
    ex = X.Executor(X.guest_file(args.program + ".elf"), stdin=stdin_of(args.program, 2 * args.cycles))
    shard = ex.run_shard(args.cycles)
    tracer = X.EventTracer(ex, shard, "cuda")
    machine, tabs, publics = tracer.build()
    by_name = {a.name: (a, it) for a, it in machine}
    pc_base, program = ex.program()
    d_events = tracer.ex.ev
    staged = {n: (to_col_major(main), to_col_major(prep) if prep is not None else None)
              for n, (prep, main) in tabs.items() if n not in COUNTED and main.shape[0]}
    out["rows"] = {n: int(m.height) for n, (m, _) in staged.items()}
    out["cells"] = int(sum(m.height * m.width for m, _ in staged.values()))
    words = lambda cm: cm.words.view(cm.width, cm.height)

    def device():
        got = X.device_lookup_tables(machine, staged, publics, d_events, program, pc_base)       # finish() synchronises
        return got

    def with_torch():
        tracer.byte_range_tables(by_name, tracer.pv)
        executed = torch.bincount((d_events[:, X.E_PC] - pc_base) >> 2, minlength=len(program))
        torch.cuda.synchronize()
        return tracer.tables["Byte"].main, tracer.tables["Range"].main, executed

    got, (byte, rng, executed) = device(), with_torch()                  # the untimed round, and the check
    want_program = torch.zeros(RT.pad32(len(program)), 1, dtype=torch.int64, device="cuda")
    want_program[:len(program), 0] = executed
    for n, want in (("Byte", byte), ("Range", rng), ("Program", want_program)):
        assert torch.equal(words(got[n]), words(to_col_major(want))), "%s: the device count differs from the torch count" % n
    messages = int(byte.sum()) + int(rng.sum())
    hottest = max(int(byte.max()), int(rng.max()))
    ms = {"device": [], "torch": []}
    for _ in range(args.rounds):
        for name, fn in (("device", device), ("torch", with_torch)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            ms[name].append(1e3 * (time.perf_counter() - t0))
            del res
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "all_ms": [round(x, 3) for x in v]}
    d, t = stat(ms["device"]), stat(ms["torch"])
    out.update({"measured": True, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "tables_equal_word_for_word": True,
                "cycles": int(shard.cycles), "byte_messages": messages, "executed_pcs": int(d_events.shape[0]),
                "hottest_cell_messages": hottest, "hottest_cell_share": round(hottest / max(messages, 1), 4),
                "device_count": d, "torch_count": t, "device_messages_per_second": round(messages / (1e-3 * d["median_ms"])),
                # the requirement: the device count is not slower than the torch path beyond that yardstick's own min-max spread
                "device_not_slower_than_torch_beyond_its_spread": bool(d["median_ms"] <= t["median_ms"] + (t["max_ms"] - t["min_ms"]))})
    emit()
    assert out["device_not_slower_than_torch_beyond_its_spread"], "the device count is slower than the torch count of the same tables"


if __name__ == "__main__":
    main()
