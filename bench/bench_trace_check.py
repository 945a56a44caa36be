#!/usr/bin/env python3
"""What the device trace checker costs on shards of the size it exists for, both device-made (no host table anywhere):

  core     the first core shard of a fibonacci run cut by trace area (riscv_exec.device_core_shard);
  memory   a synthetic memory shard of split_thresholds(...)["memory"] finalise rows with as many initialise rows — the 740,160-row
           shards of the rsp block (riscv_exec.device_memory_shard).

Per shard, medians of --rounds (5) with min and max, after one untimed call:
  constraints    the kernels of sp1hip_check_constraints (every constraint, every row, every chip; the non-canonical word count),
                 by the library's own event timers (sp1hip_timers_*), and the whole call by the wall clock (it synchronises);
  buses pass 1   the tally kernels and the verdict of sp1hip_check_interactions, the same two ways;
  buses pass 2   a balanced shard has none: one cell of the Global table is changed on the device (one message no longer
                 cancels) and the pass that names the records is timed on that shard, with api.check_interactions' exact tally.
Beside them tests/machine_check.check_shard (numpy, the only row-by-row checker there was) on the same tables copied to the host: on
the first 1/16 of every table's rows, the time multiplied by 16 and reported as `scaled` (buses do not balance on a slice: only the
time is used), unless --host-whole asks for the whole shard. Bytes: what each pass reads (every main and preprocessed column a
constraint or an interaction names, once per piece that loads it, counted from the compiled programs) against the tables' size.

The one thing asserted: wherever both ran, the device's reports and verdicts are the host checker's (no failing chip, balanced; on
the one-cell-changed shard the verdict is "unbalanced" and the exact tally is pairs of keys whose discrepancies cancel).
One JSON line; `--out` also writes it to a file. Without a GPU the line says so and holds no figure.

  python bench/bench_trace_check.py [--cycles 26000000] [--out profiles/trace_check_bench.json]
"""
import argparse
import ctypes as C
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

P = 0x7F000001


def stat(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}


def bytes_read(chips):
    """(constraint pass, bus pass) bytes: 4 x rows x the columns each compiled program loads (a piece loads what it needs again)."""
    from sp1_amd import _lib, air as A
    lib = _lib.load()
    cons = bus = 0
    for air, it, main, prep in chips:
        rows = main.height if main is not None else 0
        if not rows:
            continue
        if air.num_constraints:
            prog = np.ascontiguousarray(air.to_array(), dtype=np.uint32)
            n = C.c_size_t(0)
            lib.sp1hip_trace_check_compile(prog.ctypes.data_as(_lib.u32p), prog.shape[0], air.main_width, air.prep_width, air.num_constraints, 0, None, C.byref(n))
            words = np.zeros(n.value, dtype=np.uint32)
            _lib.check(lib.sp1hip_trace_check_compile(prog.ctypes.data_as(_lib.u32p), prog.shape[0], air.main_width, air.prep_width, air.num_constraints, 0,
                                                      words.ctypes.data_as(_lib.u32p), C.byref(n)))
            at = 5
            for _ in range(int(words[0])):
                k = int(words[at])
                ops = words[at + 2:at + 2 + 4 * k].reshape(k, 4)[:, 0]
                loads = ops[(ops & 0xFF) <= 1]
                cons += 4 * rows * int((((loads >> 16) & 3) + 1).sum())
                at += 2 + 4 * k
        cons += 4 * rows * (air.main_width + air.prep_width)                    # the non-canonical word count reads every word once
        for _, values, mult in it.sends + it.receives:
            bus += 4 * rows * (len(mult.terms) + sum(len(v.terms) for v in values))   # an upper bound: values are read where m != 0
    return cons, bus


def measure(name, machine, chips, publics, rounds, host_fraction, log):
    from sp1_amd import api
    from sp1_amd.machines import public_values as PVM, riscv_exec as X, riscv_trace as RT
    import machine_check as MC
    lib = api._L()
    sync = torch.cuda.synchronize
    pv = [int(v) for v in (publics.cpu().tolist() if torch.is_tensor(publics) else publics)]
    words = RT.to_monty_np(torch.as_tensor(np.asarray(pv, dtype=np.int64)))
    pv_air, pv_it = PVM.program()
    row = api.ColMajor(api.to_device(words[:pv_it.main_width]), 1, pv_it.main_width)
    with_pv = list(chips) + [(pv_air, pv_it, row, None)]
    table_bytes = sum(4 * c[2].height * (c[0].main_width + c[0].prep_width) for c in chips if c[2] is not None)
    messages = 0

    def timer(label):
        n_, ms_ = C.c_uint64(), C.c_double()
        api.check(lib.sp1hip_timers_read(label.encode(), C.byref(n_), C.byref(ms_)))
        return ms_.value / 1e3

    def timed(fn, labels):
        api.check(lib.sp1hip_timers_reset())
        sync()
        t0 = time.perf_counter()
        got = fn()
        wall = time.perf_counter() - t0
        return got, wall, [timer(l) for l in labels]

    # the untimed round, and the one assertion
    failing, imbalance = X.check_device_shard(machine, chips, publics)
    assert failing == [] and imbalance == {}, (name, failing, list(imbalance.items())[:4])
    sec = {k: [] for k in ("constraints_call", "constraints_kernels", "buses_call", "pass1_kernels")}
    for _ in range(rounds):
        reports, wall, (k,) = timed(lambda: api.check_constraints(chips, words), ["trace_check_constraints"])
        sec["constraints_call"].append(wall)
        sec["constraints_kernels"].append(k)
        buses, wall, (k,) = timed(lambda: api.check_interactions(with_pv), ["trace_check_buses_pass1"])
        sec["buses_call"].append(wall)
        sec["pass1_kernels"].append(k)
        messages = buses["messages"]
        assert buses["balanced"] and all(r["failing_rows"] == 0 and r["noncanonical"] == 0 for r in reports)
    # pass 2: one Global cell changed on the device
    g = next(c for c in chips if c[0].name == "Global")
    view = g[2].words.view(g[2].width, g[2].height)
    cols = list(dict.fromkeys(t[1] for _, values, _ in g[1].sends + g[1].receives for v in values for t in v.terms if t[0] == "main"))
    for col in cols:                                           # the first column of row 0 whose change some message carries
        cell = view[col:col + 1, 0:1]
        old = cell.clone()
        changed = RT.to_monty_np(torch.tensor([(from_monty_cell(old) + 1) % P])).view(np.int32)
        cell.copy_(torch.as_tensor(changed).to(cell.device).view(1, 1))
        if not api.check_interactions(with_pv, cap=0)["balanced"]:
            break
        cell.copy_(old)
    else:
        raise AssertionError("%s: no message of Global's row 0 changes with its columns" % name)
    sec2 = {k: [] for k in ("buses_call_unbalanced", "pass1_kernels_unbalanced", "pass2_kernels")}
    for k in range(rounds):
        buses, wall, (k1, k2) = timed(lambda: api.check_interactions(with_pv), ["trace_check_buses_pass1", "trace_check_buses_pass2"])
        sec2["buses_call_unbalanced"].append(wall)
        sec2["pass1_kernels_unbalanced"].append(k1)
        sec2["pass2_kernels"].append(k2)
    assert not buses["balanced"], "one changed message and the buses still balance"
    # one changed value: what was sent no longer meets what is received — pairs of keys whose discrepancies cancel. (Where the
    # changed message shares its bucket with a key that more than `cap` messages carry, the records are truncated and the exact
    # tally is not the whole truth: the line says so.)
    if not buses["truncated"]:
        assert len(buses["imbalance"]) >= 2 and sum(buses["imbalance"].values()) % P == 0, list(buses["imbalance"].items())[:4]
    unbalanced = {"changed_global_column": col, "records_wanted": buses["records_wanted"], "truncated_at_cap_65536": buses["truncated"], "keys": len(buses["imbalance"]),
                  "nonzero_buckets": list(buses["nonzero_buckets"])}
    cell.copy_(old)
    # the host checker on the same tables, copied
    log("%s: copying the tables to the host" % name)
    t0 = time.perf_counter()
    tabs = {}
    for a, _, main, prep in chips:
        n = main.height if host_fraction == 1 else main.height // host_fraction
        take = lambda t: None if t is None else torch.as_tensor(MC.from_monty(t.to_row_major_host()[:n]).astype(np.int64))
        tabs[a.name] = (take(prep), take(main))
    copy_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    bad, keys = MC.check_shard(machine, tabs, torch.as_tensor(np.asarray(pv, dtype=np.int64)), PVM.program())
    host_s = time.perf_counter() - t0
    assert bad == [], (name, bad)                                               # constraints hold on any slice of the rows
    if host_fraction == 1:
        assert keys == 0, (name, keys)
    cons_b, bus_b = bytes_read(with_pv)
    return {"chips": len(chips), "rows": {c[0].name: c[2].height for c in chips if c[2] is not None and c[2].height}, "cells": table_bytes // 4,
            "table_bytes": table_bytes, "messages": messages,
            "constraints": {"kernels": stat(sec["constraints_kernels"]), "whole_call": stat(sec["constraints_call"]), "bytes_read": cons_b,
                            "bytes_read_over_table_bytes": round(cons_b / table_bytes, 3)},
            "buses_pass1": {"kernels": stat(sec["pass1_kernels"]), "whole_call_balanced": stat(sec["buses_call"]), "bytes_read_at_most": bus_b,
                            "bytes_read_over_table_bytes": round(bus_b / table_bytes, 3), "log_buckets": 22},
            "buses_pass2_one_cell_changed": dict(unbalanced, kernels=stat(sec2["pass2_kernels"]), pass1_kernels=stat(sec2["pass1_kernels_unbalanced"]),
                                                 whole_call_with_exact_tally=stat(sec2["buses_call_unbalanced"]), bytes_read_at_most=bus_b),
            "machine_check_check_shard": {"rows_fraction": "1/%d" % host_fraction, "seconds": round(host_s, 2), "scaled_seconds": round(host_s * host_fraction, 2),
                                          "copy_to_host_seconds": round(copy_s, 2), "failing_chips": bad}}


def from_monty_cell(t):
    """the canonical value of a 1 x 1 int32 device tensor holding a Montgomery word."""
    return int(t.cpu().numpy().view(np.uint32).reshape(-1)[0]) * pow(1 << 32, -1, P) % P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="fibonacci")
    ap.add_argument("--cycles", type=int, default=26_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-whole", action="store_true", help="machine_check on the whole shard instead of 1/16 of its rows")
    ap.add_argument("--only", default="", help="core or memory")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"bench": "trace_check"}

    def emit():
        line = json.dumps(out)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if not torch.cuda.is_available():
        out.update({"measured": False, "note": "no GPU in this run: nothing was measured, no figure is reported"})
        return emit()
    from bench_device_memory_shard import synthetic_lists
    from core_real import to_col_major
    from program_shard import stdin_of
    from sp1_amd import api
    from sp1_amd.machines import riscv_exec as X
    torch.cuda.set_device(0)
    api.check(api._L().sp1hip_timers_enable(1))
    log = lambda s: print("bench_trace_check: " + s, file=sys.stderr, flush=True)
    ex = X.Executor(X.guest_file(args.program + ".elf"), stdin=stdin_of(args.program, args.cycles))
    ex.cut_by_area()
    shard = ex.run_shard(1 << 40)
    prep = {k: to_col_major(t) for k, t in X.preprocessed_tables(ex, "cuda").items()}
    out.update({"measured": True, "device_name": torch.cuda.get_device_name(0), "rounds": args.rounds, "program": args.program})
    fraction = 1 if args.host_whole else 16
    if args.only != "memory":
        machine, chips, publics, _ = X.device_core_shard(ex, shard, prep)
        log("core shard: %d cycles" % shard.cycles)
        out["core_shard"] = dict(measure("core", machine, chips, publics, args.rounds, fraction, log), cycles=shard.cycles)
        del machine, chips
        emit()
    if args.only != "core":
        n = X.split_thresholds(ex.program()[1].shape[0])["memory"]
        ia, ir, fa, fr, p_init, p_fin = synthetic_lists(n)
        ex2 = X.Executor(X.guest_file(args.program + ".elf"), stdin=stdin_of(args.program, args.cycles))     # the run's final state: executed, nothing traced
        ex2.cut_by_area()
        ctx = next(r for r in X.run_records(ex2, 1 << 40, core_limit=0) if r.kind == "memory").ctx
        made = X.device_memory_shard(ia, ir, fa, fr, prep, ctx, previous_init=p_init, previous_fin=p_fin)
        machine, chips, publics = made[0], made[1], made[2]
        log("memory shard: %d rows" % n)
        out["memory_shard"] = dict(measure("memory", machine, chips, publics, args.rounds, fraction, log), finalise_rows=n)
    emit()


if __name__ == "__main__":
    main()
