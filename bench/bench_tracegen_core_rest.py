#!/usr/bin/env python3
"""What it costs to make the DivRem, AluX0, MemoryLocal and Global tables of a core shard, three ways, at the row counts of a core
shard of a real guest (rsp: its first shard of --cycles cycles, whose own rows are the rows measured; where that shard has no
DivRem or AluX0 instruction — rsp's has none — those two are measured at --synthetic-rows re-labelled events, and the line says so):

  generate   the pinned records (88-byte sp1hip_rv64_alu_event_t for DivRem and AluX0, 40-byte local-memory records for MemoryLocal
             and Global) are copied to the device and the table is made there (api.tracegen_riscv_divrem / _alu_x0 / _memory_local;
             Global: the MemoryLocal kernel writes the events, api.tracegen_riscv_global makes the table from them — so Global's
             figure contains MemoryLocal's): timed from the start of the record copy to the end of the last kernel;
  host_fill  the host tracer's filler of the same table, on the CPU (Tracer.simple_alu with divrem_extra — divrem_rows' Python loop —,
             EventTracer.build's AluX0 closure, EventTracer.memory_local_and_bumps, and for Global eval_interactions over the
             MemoryLocal table followed by Tracer.global_chip);
  stage      the host-made row-major table (Montgomery words, pinned) goes through sp1hip_stage_tables (PCIe copy + on-GPU
             transpose): the path these tables took before.

generate and stage alternate in ONE process on the same stream; medians of 5 with min and max, after one untimed round of both; the
host filler is run 5 times as well (DivRem: --host-rounds, its loop is slow). The device tables are compared with the staged ones
word for word first. There is no pass ratio: the file records what was measured. One JSON line; `--out` also writes it to a file.
Without a GPU the line says so and holds no figure.

  python bench/bench_tracegen_core_rest.py [--program rsp] [--out profiles/riscv_core_rest_tracegen_bench.json]
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

CHIPS = ("DivRem", "AluX0", "MemoryLocal", "Global")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="rsp", help="the guest whose first core shard is measured (it needs DivRem and AluX0 rows)")
    ap.add_argument("--cycles", type=int, default=1 << 20)
    ap.add_argument("--synthetic-rows", type=int, default=1 << 16, help="DivRem / AluX0 rows when the guest's shard has none")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=5, help="rounds of the host fillers")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from program_shard import stdin_of
    from sp1_amd.machines import riscv as R, riscv_exec as X, riscv_trace as RT
    out = {"bench": "riscv_core_rest_tracegen", "chips": list(CHIPS), "events_from": "%s, first shard of %d cycles" % (args.program, args.cycles)}

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
    own = {n: int((names_of == n).sum()) for n in ("DivRem", "AluX0")}
    out["rows_in_the_guests_shard"] = dict(own, MemoryLocal=len(shard.local), Global=2 * len(shard.local))
    # MemoryLocal and Global are measured at the shard's own rows. A shard without DivRem / AluX0 rows (rsp has none in its first
    # 4 x 10^7 cycles; the reference's recorded core shard has 8 DivRem rows) gets --synthetic-rows of them: the shard's register-
    # register ALU events with real operands and timestamps, re-labelled — the eight DivRem opcodes in turn with a from divrem_result,
    # and rd = x0 for AluX0. The other events are dropped, so each filler runs over its own rows alone.
    synthetic = {}
    for n in ("DivRem", "AluX0"):
        if own[n]:
            continue
        src = shard.events[np.nonzero((shard.events[:, X.E_OP] <= R.OPC["MULHSU"]) & (shard.events[:, X.E_FLAGS] == 0) & (shard.events[:, X.E_OPA] != 0))[0]]
        assert len(src), "the guest's shard has no register-register ALU event to re-label"
        ev = src[np.arange(args.synthetic_rows) % len(src)].copy()
        if n == "DivRem":
            ops = [R.OPC[o] for o in RT.ALU_KINDS["DivRem"]]
            ev[:, X.E_OP] = np.array(ops)[np.arange(len(ev)) % 8]
            ev[:, X.E_A] = [RT.divrem_result(int(o), int(b), int(c))[0] for o, b, c in zip(ev[:, X.E_OP], ev[:, X.E_B], ev[:, X.E_C])]
        else:
            ev[:, X.E_OPA], ev[:, X.E_A], ev[:, X.E_A_PREV] = 0, 0, 0
        synthetic[n] = ev
    if synthetic:
        shard.events = np.concatenate([shard.events[np.nonzero((names_of == "DivRem") | (names_of == "AluX0"))[0]]] + list(synthetic.values()))
        names_of = X.chip_of_events(shard.events)
        out["synthetic_rows"] = {n: "%d re-labelled register-register ALU events of the shard" % len(ev) for n, ev in synthetic.items()}
    n_rows = {"DivRem": int((names_of == "DivRem").sum()), "AluX0": int((names_of == "AluX0").sum()), "MemoryLocal": len(shard.local),
              "Global": 2 * len(shard.local)}
    assert all(n_rows.values()), "no rows for one of the tables: %r" % (n_rows,)
    heights = {n: RT.pad32(v) for n, v in n_rows.items()}
    out.update({"rows": n_rows, "heights": heights, "cycles": shard.cycles})
    print("bench_tracegen_core_rest: %r" % (n_rows,), file=sys.stderr, flush=True)

    # the host fillers over exactly these rows: one filler each, without the rest of a shard around it
    def host_fill(name):
        tr = X.EventTracer(ex, shard, "cpu")
        if name == "Global":
            tr.memory_local_and_bumps()                       # not timed: Global's own cost starts from the MemoryLocal table
        t0 = time.perf_counter()
        if name == "DivRem":
            tr.simple_alu("DivRem", "R", tr.divrem_extra)
        elif name == "AluX0":
            def alu_x0(tb, k, p, a, bv, cv):
                tb.set("opcode", tr.ex.op[p])
                tb.set("is_real", 1)
            tr.simple_alu("AluX0", "ALU", alu_x0)
        elif name == "MemoryLocal":
            tr.memory_local_and_bumps()
        else:
            ml = tr.tables["MemoryLocal"]
            (_, recv, _), (_, send, _) = RT.eval_interactions(R.chip("MemoryLocal")[1], ml.main[:ml.n], None, kinds=(R.GLOBAL,))
            tr.global_chip({}, torch.stack([recv, send], dim=1).reshape(-1, 11))
        return time.perf_counter() - t0, tr.tables[name].main

    monty = lambda t: ((t << 32) % RT.P).to(torch.int32)
    host_seconds, hosts = {}, {}
    for n in CHIPS:
        times = []
        for _ in range(args.host_rounds):
            s, table = host_fill(n)
            times.append(s)
        host_seconds[n] = times
        assert table.shape[0] == heights[n], (n, table.shape)
        hosts[n] = monty(table).pin_memory()
        print("bench_tracegen_core_rest: host %s %.3f s" % (n, statistics.median(times)), file=sys.stderr, flush=True)
    records = {n: torch.as_tensor(np.ascontiguousarray(X.pack_alu_events(shard.events, n))).pin_memory() for n in ("DivRem", "AluX0")}
    records["MemoryLocal"] = records["Global"] = torch.as_tensor(np.ascontiguousarray(shard.local)).pin_memory()
    stream = torch.cuda.Stream()

    def generate(name):
        with torch.cuda.stream(stream):
            d = records[name].to(dev, non_blocking=True)
            if name == "DivRem":
                table = api.tracegen_riscv_divrem(d, heights[name], stream=stream)
            elif name == "AluX0":
                table = api.tracegen_riscv_alu_x0(d, heights[name], stream=stream)
            else:
                table, events = api.tracegen_riscv_memory_local(d, heights["MemoryLocal"], stream=stream)
                if name == "Global":
                    table = api.tracegen_riscv_global(events, heights[name], stream=stream)
        stream.synchronize()
        return table

    def stage(name):
        with torch.cuda.stream(stream):
            table = api.stage_tables([hosts[name]], stream=stream)[0]
        stream.synchronize()
        return table

    stat = lambda v, k=1e3, unit="ms": {"median_" + unit: round(k * statistics.median(v), 3), "min_" + unit: round(k * min(v), 3),
                                        "max_" + unit: round(k * max(v), 3), "all_" + unit: [round(k * x, 3) for x in v]}

    def measure(name):
        g, s = generate(name), stage(name)                   # the untimed round: allocator and arena warm, and the check
        assert (g.width, g.height) == (s.width, s.height) and torch.equal(g.words, s.words), "%s: the device table differs from the staged host table" % name
        del g, s
        sec = {"generate": [], "stage": []}
        for _ in range(args.rounds):
            for what, fn in (("generate", generate), ("stage", stage)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                table = fn(name)
                sec[what].append(time.perf_counter() - t0)
                del table
        print("bench_tracegen_core_rest: device %s done" % name, file=sys.stderr, flush=True)
        return {"table_bytes": 4 * hosts[name].numel(), "record_bytes": 8 * records[name].numel(), "generate_from_pinned_records": stat(sec["generate"]),
                "host_fill": stat(host_seconds[name], 1.0, "s"), "stage_host_table": stat(sec["stage"])}

    out.update({"measured": True, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "host_rounds": args.host_rounds,
                "tables_equal_word_for_word": True, "per_table": {n: measure(n) for n in CHIPS}})
    emit()


if __name__ == "__main__":
    main()
