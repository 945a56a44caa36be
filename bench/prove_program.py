"""A WHOLE guest program proved shard by shard on one GPU: every core shard, every precompile shard (cut at the reference's
`SplitOpts` thresholds), every memory shard of one execution — what the reference's perf harness times as "core proving" and
divides the cycle count by (/root/reference/sp1-gpu/crates/perf/src/report.rs:L52-L60).

    python bench/prove_program.py --program rsp            # the Reth block of the reference's perf inputs: 9.8e7 cycles, 26 shards
    python bench/prove_program.py --program fibonacci --cycles 30000000

Per shard: the executor runs until the reference's shard-cutting rule ends the shard (trace-area estimator, host, C++), the tracer builds the tables ON THE DEVICE
(torch: plumbing; the tables of a production deployment come from the Rust host's tracegen), `sp1hip_prove_shard` proves them with
production parameters (blowup 4, 124 queries, 16-bit PoW) and the shard's own public values. Timed per shard: executor, tables,
setup (the preprocessed commitment — the proving key, per shard shape here), prove. ONE JSON line at the end:
`prove_seconds` = the sum of the prove calls (the first shard of every kind is proved once before its timed proof: that first
call also plans the kind's constraint programs, a per-process cost like the reference's prover construction, listed apart as
`first_proofs_of_a_kind_seconds`), `cycles_per_s` = cycles / prove_seconds (the harness's definition), and the same with
the tables and the executor included (this repository's Python tracer is NOT the product; the number is there so that nothing is hidden).
`--verify` runs the pinned verifier (oracle/: checker only, untimed) on the first proof of every shard kind; the Global messages of
all shards must cancel (the statement their septic digests add up to), which is checked on the events the tracer returns.
`--dry-run` builds every shard and proves nothing (no GPU needed: the CPU check of this script)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bench"))


def program_run(api, program="fibonacci", cycles=26_000_000, L=22, lsh=21):
    """bench.py's `program_run` extra: one WHOLE run of a guest under the caller's clock — every core shard (cut by trace area, the
    reference's rule), every precompile shard, the memory shard — with ONE proving key for the program (sp1hip_setup: every shard
    is a shape cluster holding Program / Byte / Range), production parameters, each shard's own public values. Returns cycles /
    (setup + prove seconds) — the perf harness's definition, /root/reference/sp1-gpu/crates/perf/src/report.rs:L52-L60 — with
    the executor's and this repository's (torch) tracer's seconds listed beside it, the cross-shard checks of SP1Prover::verify
    on the public values (they chain from the entry point to HALT, the septic digests add up to zero) and the proof of the
    LAST shard for the caller to verify."""
    import numpy as np
    import torch
    from core_real import to_col_major
    from program_shard import stdin_of
    from sp1_amd.machines import public_values as PVM, riscv_exec as X, riscv_trace as RT
    t_all = time.perf_counter()
    ex = X.Executor(X.guest_file(program + ".elf"), stdin=stdin_of(program, cycles))
    ex.cut_by_area()
    rows, pvs, kinds, pk, pk_prep, last = [], [], [], None, None, None
    n_cycles, t_prev = 0, time.perf_counter()
    for kind, machine, tabs, publics, gev, sh in X.program_shards(ex, 1 << 40, device="cuda"):
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t_prev                      # executor + tables of this shard
        area = sum(int(tabs[a.name][1].shape[0]) * (a.main_width + a.prep_width) for a, _ in machine)
        setup_s = 0.0
        if pk is None:
            vk_ints = X.verifying_key_words(ex, sh.pc_start, "cuda")     # entry point + the digest of the memory image's initialisation
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pk_prep = {a.name: to_col_major(tabs[a.name][0]) for a, _ in machine if tabs[a.name][0] is not None}
            vk_words = RT.to_monty_np(torch.tensor(vk_ints))
            pk = api.ProvingKey([pk_prep[n] for n in sorted(pk_prep)], L, lsh, 32, pc_start=vk_words[:3], initial_global_cumulative_sum=vk_words[3:])
            torch.cuda.synchronize()
            setup_s = time.perf_counter() - t0
            entry = sh.pc_start
        chips = [(a, i, to_col_major(tabs[a.name][1]), pk_prep.get(a.name)) for a, i in machine]
        tabs.clear()
        pv = RT.to_monty_np(publics)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        proof = pk.prove_shard(chips, pv)
        torch.cuda.synchronize()
        prove_s = time.perf_counter() - t0
        if sh is not None:
            n_cycles += sh.cycles
        rows.append({"kind": kind, "cells": area, "cycles": sh.cycles if sh is not None else None, "build_s": round(build_s, 3),
                     "setup_ms": round(1e3 * setup_s, 2), "prove_ms": round(1e3 * prove_s, 2), "proof_bytes": len(proof)})
        pvs.append([int(v) for v in publics])
        kinds.append(kind)
        last = {"kind": kind, "names": [a.name for a, _ in machine], "proof": proof, "vk_words": vk_words}
        del chips
        torch.cuda.empty_cache()
        t_prev = time.perf_counter()
    prove_s = sum(r["prove_ms"] for r in rows) / 1e3
    setup_s = sum(r["setup_ms"] for r in rows) / 1e3
    build_s = sum(r["build_s"] for r in rows)
    chain = PVM.verify_proof_public_values([pvs[i] for i in X.proof_order(kinds)], entry, vk_ints[3:])
    head = api.DuplexChallenger()
    pk.observe_into(head)
    out = {"program": program, "cycles": n_cycles, "shards": len(rows), "kinds": {k: kinds.count(k) for k in dict.fromkeys(kinds)},
           "cells": sum(r["cells"] for r in rows), "prove_seconds": round(prove_s, 4), "setup_seconds": round(setup_s, 4),
           "executor_and_tracer_seconds": round(build_s, 2), "wall_seconds": round(time.perf_counter() - t_all, 2),
           "cycles_per_s": n_cycles / (prove_s + setup_s), "cycles_per_s_incl_executor_and_python_tracer": n_cycles / (prove_s + setup_s + build_s),
           "public_values_chain": chain or "ok", "per_shard": rows,
           "note": "cycles / (setup + prove) is the perf harness's 'core kHz' x 1000; the executor (one host core) and this repository's torch tracer "
                   "are NOT the product (SURVEY 2: crates/core/{executor,machine} out of scope) and dominate the wall time — listed so that nothing is hidden"}
    return out, last, np.asarray(pk.preprocessed_commit).copy(), head.state()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="rsp")
    ap.add_argument("--elf", default="", help="prove this ELF file, run without input, instead of a bundled guest (a hand-assembled test program: "
                    "tests/field_chip_cases.py::mixed_program calls a curve's and a tower field's precompiles, which no bundled guest does)")
    ap.add_argument("--cycles", type=int, default=0, help="size the input for at least this many cycles (not for rsp: its input is a recorded block)")
    ap.add_argument("--shard-cycles", type=int, default=0, help="cut core shards at this many cycles instead of by trace area (the default: the "
                    "reference's rule, ShapeChecker with ELEMENT_THRESHOLD 2^28 + 2^27 / HEIGHT_THRESHOLD 2^22, inside the executor)")
    ap.add_argument("--max-shards", type=int, default=0, help="stop after this many shards (0 = the whole run)")
    ap.add_argument("--core-shards", type=int, default=0, help="trace and prove only the first N core shards (the others are executed, not "
                    "proved), then every precompile and memory shard: a bounded sample of every shard kind of the run")
    ap.add_argument("--in-flight", type=int, default=0, help="after the shard-by-shard pass, prove ALL shards again through the library's "
                    "prover pool with this many proofs in flight (tables resident in HBM; proofs must equal the first pass's)")
    ap.add_argument("--only-kinds", default="", help="comma-separated shard kinds: build every shard, prove only these (a profile of one kind)")
    ap.add_argument("--device-shard", action="store_true", help="every shard of the run (riscv_exec.DEVICE_ANY_KINDS: core, memory and every precompile kind): make the WHOLE shard on the device "
                    "from the executor's records (riscv_exec.device_shard_any over run_records — device_core_shard: the event partition kernel, every chip's table, the public "
                    "values' Global fields, the lookup counts; device_memory_shard: MemoryGlobalInit / Finalize from the run's address lists; "
                    "device_precompile_shard / device_family_shard / device_family_rest_shard: the wide tables, SyscallPrecompile, MemoryLocal from the calls' event records) — no tracer and "
                    "no host table is built for them; the public values are chained by the previous shard's, the Global events still join "
                    "the run's balance check. MemoryBump's rows stand in another order than the host tracer's, so a core shard that crosses 2^24 cycles proves "
                    "to other bytes (the same statement)")
    ap.add_argument("--check", action="store_true", help="before each proof, check the shard's device tables where they are: every constraint on every row and every "
                    "bus (riscv_exec.check_device_shard: sp1hip_check_constraints / sp1hip_check_interactions). Outside every timed region; each "
                    "row gains check_ms and check: \"ok\" or the findings")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from program_shard import FULL_CYCLES_OF, stdin_of
    from sp1_amd.machines import public_values as PVM, riscv_exec as X, riscv_trace as RT
    device = "cpu" if args.dry_run else "cuda"
    assert not (args.dry_run and args.device_shard), "--device-shard makes the tables on the GPU: there is nothing to dry-run"
    assert not (args.dry_run and args.check), "--check checks the device tables: there are none in a dry run"
    if not args.dry_run:
        from core_real import to_col_major
        import ctypes as C
        from sp1_amd import api
        torch.cuda.set_device(0)
        lib = api._L()
        api.check(lib.sp1hip_timers_enable(1))
    shard_cycles = args.shard_cycles or 1 << 40
    L, lsh = 22, 21
    if args.elf:
        with open(args.elf, "rb") as f:
            ex, args.program = X.Executor(f.read(), stdin=[]), os.path.basename(args.elf)
    else:
        ex = X.Executor(X.guest_file(args.program + ".elf"), stdin=stdin_of(args.program, args.cycles or 3 * FULL_CYCLES_OF[args.program]))
    if not args.shard_cycles:
        ex.cut_by_area()
    shards, gevs, kept, cycles, last, resident, pvs, pk, pk_prep, warmed = [], [], {}, 0, None, [], [], None, None, {}
    t_all = time.perf_counter()
    t_prev = t_all
    for rec in X.run_records(ex, shard_cycles, core_limit=args.core_shards or None):
        kind, sh, tabs, device_chips = rec.kind, rec.executed, None, None
        if args.device_shard:                                           # every kind of shard: no tracer and no host table
            if pk_prep is None:
                pk_prep = {n: to_col_major(t) for n, t in X.preprocessed_tables(ex, "cuda").items()}
            machine, device_chips, publics, gev9 = X.device_shard_any(ex, rec, pk_prep)
            gev = X.global_events_11(gev9)
        else:
            machine, tabs, publics, gev = X.host_shard(ex, rec, device)
        if device == "cuda":
            torch.cuda.synchronize()
        t_build = time.perf_counter() - t_prev                          # executor (inside run_records) + tables of this shard
        heights = {c[0].name: c[2].height for c in device_chips} if device_chips is not None else {a.name: int(tabs[a.name][1].shape[0]) for a, _ in machine}
        area = sum(heights[a.name] * (a.main_width + a.prep_width) for a, _ in machine)
        row = {"kind": kind, "chips": len(machine), "cells": area, "build_s": round(t_build, 3),
               "rows": {a.name: heights[a.name] for a, _ in machine if a.name not in ("Byte", "Range", "Program")}}
        if device_chips is not None:
            row["device_shard"] = True
        if sh is not None:
            row["cycles"], row["estimated_cells"] = sh.cycles, sh.estimated_area
            cycles, last = cycles + sh.cycles, sh
        gevs.append(gev.cpu())
        pvs.append([int(v) for v in publics])
        if args.only_kinds and kind not in args.only_kinds.split(",") and pk is not None:
            t_prev = time.perf_counter()
            continue
        if not args.dry_run:
            # ONE proving key per program (sp1hip_setup: the preprocessed commitment of Program / Byte / Range + the verifying key):
            # every shard of the run — core, precompile, memory — is a shape cluster that holds those three chips
            row["setup_ms"] = 0.0
            if pk is None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if pk_prep is None:
                    pk_prep = {a.name: to_col_major(tabs[a.name][0]) for a, _ in machine if tabs[a.name][0] is not None}
                vk_ints = X.verifying_key_words(ex, sh.pc_start, "cuda")
                # the verifying key's words (Montgomery form, like everything the transcript absorbs): the entry pc, and the digest of
                # the memory image's initialisation (one septic point per image word: program.rs:L170-L199)
                vk_words = RT.to_monty_np(torch.tensor(vk_ints))
                pk = api.ProvingKey([pk_prep[n] for n in sorted(pk_prep)], L, lsh, 32, pc_start=vk_words[:3], initial_global_cumulative_sum=vk_words[3:])
                torch.cuda.synchronize()
                row["setup_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            if device_chips is not None:
                chips = device_chips
            else:
                assert sorted(a.name for a, _ in machine if tabs[a.name][0] is not None) == sorted(pk_prep), "a shard without the program's preprocessed chips"
                chips = [(a, i, to_col_major(tabs[a.name][1]), pk_prep.get(a.name)) for a, i in machine]
            if tabs is not None:
                tabs.clear()
            if args.check:                                                                # untimed: before the proof, after build_s and setup_ms
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                failing, imbalance = X.check_device_shard(machine, chips, publics)
                row["check_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
                row["check"] = "ok" if not failing and not imbalance else {"failing": failing, "imbalance": [[list(map(str, k)) if isinstance(k, tuple) else k, v]
                                                                                                             for k, v in list(imbalance.items())[:32]]}
            pv = RT.to_monty_np(publics)
            commit = pk.preprocessed_commit
            if kind not in warmed:
                # the first proof of a shard shape in this process also plans its chips' constraint programs (cached per process
                # like the reference's compiled constraint bytecode, built once per prover): timed apart, not part of prove_ms
                t0 = time.perf_counter()
                first = pk.prove_shard(chips, pv)
                torch.cuda.synchronize()
                row["first_proof_of_kind_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
                warmed[kind] = first
            api.check(lib.sp1hip_timers_reset())
            torch.cuda.synchronize()                                                      # (the tracer's layout kernels are not the prover's time)
            t0 = time.perf_counter()
            proof = pk.prove_shard(chips, pv)                                             # from the transcript head vk.observe_into leaves
            torch.cuda.synchronize()
            row["prove_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            row["stage_ms"] = {}
            for name in ("stage_commit", "stage_logup_gkr", "stage_zerocheck", "stage_evaluation_proof"):   # the library's own stage clocks
                n_, ms_ = C.c_uint64(), C.c_double()
                api.check(lib.sp1hip_timers_read(name.encode(), C.byref(n_), C.byref(ms_)))
                row["stage_ms"][name[6:]] = round(ms_.value, 2)
            row["proof_bytes"] = len(proof)
            if "first_proof_of_kind_ms" in row:
                assert warmed[kind] == proof, "two proofs of one shard differ"
                warmed[kind] = True
            if args.verify and kind not in kept:
                kept[kind] = (machine, np.asarray(commit).copy(), proof)
            if args.in_flight:
                resident.append((pk, chips, pv, proof))
                torch.cuda.empty_cache()                                                  # the tracer's int64 intermediates go back to the driver
            else:
                del chips
        shards.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        if args.max_shards and len(shards) >= args.max_shards:
            break
        t_prev = time.perf_counter()
    wall = time.perf_counter() - t_all - sum(s.get("check_ms", 0.0) for s in shards) / 1e3     # --check is outside every timed region
    whole = (not args.max_shards or len(shards) < args.max_shards) and not args.core_shards and not args.only_kinds
    if args.core_shards:                                     # the cycles of the core shards that were executed but not proved
        out_note = "core shards beyond the first %d executed, not proved" % args.core_shards
    out = {"program": args.program, "cycles": cycles, "shards": len(shards), "whole_run": bool(whole and last is not None and last.halted),
           "exit_code": last.exit_code if last is not None and last.halted else None,
           "kinds": {k: sum(1 for s in shards if s["kind"] == k) for k in dict.fromkeys(s["kind"] for s in shards)},
           "cells": sum(s["cells"] for s in shards), "build_seconds": round(sum(s["build_s"] for s in shards), 2), "wall_seconds": round(wall, 2),
           "core_shards_cut": "by trace area (reference's ShapeChecker)" if not args.shard_cycles else "every %d cycles" % shard_cycles, "parameters": "max_log_row_count 22, stack 2^21, blowup 4, 124 queries, 16-bit PoW"}
    if args.core_shards:
        out["note"] = out_note
    if whole:
        out["global_messages_cancel"] = not X.global_events_balance(gevs + [X.image_events(ex)])   # (the image's initialisation: the verifying key's digest)
        # what SP1Prover::verify checks across the shards before it verifies each: the public values chain from the entry point to
        # HALT (timestamps, pcs, exit codes, digests, address chains) and the shards' septic digests add up to zero
        kinds_seen = [s["kind"] for s in shards]
        first_core = next(i for i, k_ in enumerate(kinds_seen) if k_ == "core")
        entry = sum(v << (16 * j) for j, v in enumerate(PVM.get(pvs[first_core], "pc_start")))
        vk_digest = vk_ints[3:] if not args.dry_run else X.verifying_key_words(ex, entry)[3:]
        out["public_values_chain"] = PVM.verify_proof_public_values([pvs[i] for i in X.proof_order(kinds_seen)], entry, vk_digest) or "ok"
    if not args.dry_run:
        prove_s = sum(s["prove_ms"] for s in shards) / 1e3
        out.update({"prove_seconds": round(prove_s, 4), "setup_seconds": round(sum(s["setup_ms"] for s in shards) / 1e3, 4),
                    "first_proofs_of_a_kind_seconds": round(sum(s.get("first_proof_of_kind_ms", 0.0) for s in shards) / 1e3, 4),
                    "cycles_per_s": round(cycles / prove_s), "cells_per_s": round(out["cells"] / prove_s),
                    "cycles_per_s_incl_python_tracegen_and_executor": round(cycles / wall),
                    "prove_ms_by_kind": {k: round(sum(s["prove_ms"] for s in shards if s["kind"] == k) / out["kinds"][k], 2) for k in out["kinds"]},
                    "stage_ms_by_kind": {k: {st: round(sum(s["stage_ms"][st] for s in shards if s["kind"] == k) / out["kinds"][k], 2)
                                             for st in ("commit", "logup_gkr", "zerocheck", "evaluation_proof")} for k in out["kinds"]}})
        if args.in_flight and args.out:                      # what has been measured so far, should the pooled pass fail
            with open(args.out, "w") as f:
                f.write(json.dumps(dict(out, per_shard=shards)) + "\n")
        if args.in_flight:
            # every shard of the run again, through the prover pool: N slots (a thread and a stream each), tables resident in HBM.
            # The direct pass's arena goes back to the driver first; should N slots' arenas not fit beside the resident tables
            # the pass is repeated with one slot fewer
            gib = lambda: [round(x / 2**30, 1) for x in torch.cuda.mem_get_info()]
            out["hbm_free_total_gib"] = {"after_direct_pass": gib()}
            released = C.c_size_t()
            api.check(lib.sp1hip_mem_trim(C.byref(released)))
            torch.cuda.empty_cache()
            out["hbm_free_total_gib"]["after_trim"] = gib()
            slots = args.in_flight
            while slots >= 1:
                pool = api.ProverPool(slots)
                try:
                    for t in [pool.submit(pk, chips, pv) for pk, chips, pv, _ in resident[:slots]]:   # fill every slot's arena (untimed)
                        pool.wait(t)
                    torch.cuda.synchronize()
                    passes = []
                    for _ in range(2):                           # the first pass meets every shard shape with cold slot arenas, the second is the steady state
                        t0 = time.perf_counter()
                        res, tickets = [], []
                        for pk, chips, pv, _ in resident:        # at most 2 N tickets outstanding: results are collected as they come
                            tickets.append(pool.submit(pk, chips, pv))
                            if len(tickets) - len(res) >= 2 * slots:
                                res.append(pool.wait(tickets[len(res)]))
                        while len(res) < len(tickets):
                            res.append(pool.wait(tickets[len(res)]))
                        torch.cuda.synchronize()
                        passes.append(time.perf_counter() - t0)
                    dt = passes[1]
                except Exception as e:                           # out of memory: fewer slots
                    out.setdefault("in_flight_failures", []).append({"slots": slots, "error": str(e)[-200:], "hbm_free_total_gib": gib()})
                    pool.close()
                    api.check(lib.sp1hip_mem_trim(C.byref(released)))
                    slots -= 1
                    continue
                pool.close()
                same = all(r[0] == want for r, (_, _, _, want) in zip(res, resident))
                out["in_flight"] = {"slots": slots, "first_pass_seconds_cold_arenas": round(passes[0], 4), "prove_seconds": round(dt, 4), "cycles_per_s": round(cycles / dt), "cells_per_s": round(out["cells"] / dt),
                                    "proofs_equal_the_direct_pass": bool(same), "proving_ms_each": [round(r[1]["proving_ms"], 1) for r in res],
                                    "hbm_free_total_gib": gib()}
                break
        if args.verify:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import pyoracle as orc                                       # the checker (test infrastructure), after everything timed
            ver = {}
            for kind, (machine, commit, proof) in kept.items():
                shapes = [(a, i, np.zeros((0, a.main_width), np.uint32), np.zeros((0, a.prep_width), np.uint32) if a.prep_width else None) for a, i in machine]
                v_ch = orc.Challenger()
                v_ch.observe(np.concatenate([commit, vk_words, np.zeros(7, np.uint32)]))   # vk.observe_into: commit, pc_start, septic x / y, flag, 6 zeros
                head = api.DuplexChallenger()
                pk.observe_into(head)
                assert np.array_equal(head.state(), v_ch.state()), "the verifier's transcript head differs from sp1hip_vk_observe_into's"
                t0 = time.perf_counter()
                rc = orc.shard_verify(shapes, commit, proof, L, lsh, v_ch, 2, 124, 16, pv_program=PVM.verifier_program())
                ver[kind] = {"rc": int(rc), "seconds": round(time.perf_counter() - t0, 2)}
            out["verified_first_of_kind"] = ver
    out["per_shard"] = shards
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
