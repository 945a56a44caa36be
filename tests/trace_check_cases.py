"""Shared by tests/test_trace_check_host.py (CPU) and tests/test_gpu_trace_check.py: the native driver of the trace checker's host
form (tests/native/trace_check), the chips both files walk, and the numpy side of every comparison (tests/machine_check.py, which
knows nothing of the library)."""
import os
import subprocess

import numpy as np

import machine_check as MC
from sp1_amd.machines import recursion, riscv
from sp1_amd.machines.riscv_more import MORE_CHIPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "trace_check")
P = 0x7F000001
RISCV = sorted(riscv.CHIPS) + sorted(MORE_CHIPS)                       # the 62 chips of the RISC-V machine
RECURSION = [air.name for air, _ in recursion.compress_machine()]


class Rejected(Exception):
    """The program was refused before anything was evaluated."""


def monty(a):
    """canonical integers -> Montgomery words."""
    return ((np.asarray(a).astype(np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def run_host(prog, main_width, prep_width, num_constraints, main, prep, publics, tmp_path, max_regs=0, timeout=300):
    """The native program over one table: prog [n][3] words, main / prep row-major Montgomery words [rows][width] (prep None for
    none), publics Montgomery words. Returns ({"pieces", "registers", "lanes"}, values [rows][num_constraints] Montgomery words);
    raises Rejected."""
    main = np.ascontiguousarray(main, dtype=np.uint32).reshape(-1, max(main_width, 1))[:, :main_width]
    rows = main.shape[0]
    names = {k: os.path.join(str(tmp_path), k + ".bin") for k in ("prog", "main", "prep", "publics", "out")}
    np.ascontiguousarray(prog, dtype=np.uint32).tofile(names["prog"])
    np.ascontiguousarray(main).tofile(names["main"])
    np.ascontiguousarray(publics, dtype=np.uint32).tofile(names["publics"])
    if prep is not None:
        np.ascontiguousarray(prep, dtype=np.uint32).tofile(names["prep"])
    r = subprocess.run([EXE, "constraints", names["prog"], str(main_width), str(prep_width), str(num_constraints), str(rows), names["main"],
                        names["prep"] if prep is not None else "-", names["publics"], str(max_regs), names["out"]],
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode == 3:
        raise Rejected(r.stderr.strip())
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = np.fromfile(names["out"], dtype=np.uint32)
    assert out.size == 4 + rows * num_constraints and out[3] == num_constraints
    return {"pieces": int(out[0]), "registers": int(out[1]), "lanes": int(out[2])}, out[4:].reshape(rows, num_constraints)


def run_host_air(air, main, prep, publics, tmp_path, max_regs=0):
    return run_host(air.to_array(), air.main_width, air.prep_width, air.num_constraints, main, prep, publics, tmp_path, max_regs)


def host_values(air, main, prep, publics):
    """machine_check.constraint_values of Montgomery tables: canonical [rows][num_constraints]."""
    return MC.constraint_values(air, None if prep is None else MC.from_monty(prep), MC.from_monty(main), MC.from_monty(publics))


def run_messages(it, main, prep, tmp_path, timeout=300):
    """The bus side of the native program over one chip: it = air.InteractionProgram, main / prep canonical [rows][width] (numpy
    or torch; prep None for none). Returns a uint64 array [messages][6]: interaction, row, canonical multiplicity, is_send, hash A,
    hash B."""
    words = it.to_array() if hasattr(it, "to_array") else it
    to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    main = to_np(main)
    rows = main.shape[0]
    names = {k: os.path.join(str(tmp_path), k + ".bin") for k in ("desc", "main", "prep", "out")}
    np.ascontiguousarray(words, dtype=np.uint32).tofile(names["desc"])
    np.ascontiguousarray(monty(main).T).tofile(names["main"])
    prep_width = 0
    if prep is not None:
        prep = to_np(prep)
        prep_width = prep.shape[1]
        np.ascontiguousarray(monty(prep).T).tofile(names["prep"])
    r = subprocess.run([EXE, "messages", names["desc"], str(main.shape[1]), str(prep_width), str(rows), names["main"],
                        names["prep"] if prep is not None else "-", names["out"]], capture_output=True, text=True, timeout=timeout)
    if r.returncode == 3:
        raise Rejected(r.stderr.strip())
    assert r.returncode == 0, (r.returncode, r.stderr)
    w = np.fromfile(names["out"], dtype=np.uint32).reshape(-1, 8).astype(np.uint64)
    return np.stack([w[:, 0], w[:, 1], w[:, 2], w[:, 3], w[:, 4] | (w[:, 5] << np.uint64(32)), w[:, 6] | (w[:, 7] << np.uint64(32))], axis=1)
