"""What the tests of the event partition and of the four small chips share (CPU: test_rv64_partition_host.py,
test_tracegen_riscv_sys_host.py; GPU: test_gpu_rv64_partition.py, test_gpu_device_core_shard.py): the three hand-assembled programs'
shards, unshifted and shifted across 2^24 cycles; synthetic ECALL, StateBump and MemoryBump events; a numpy stable partition — the
reference for every bin —; the host tracer's tables of SyscallInstrs, SyscallCore, StateBump and MemoryBump over any event list (made by
the tracer's own fillers); and tests/native/riscv_sys_rows (built by __graft_entry__.build()) behind functions.

A row of these chips is a function of its own record alone, so the host table of a PREFIX of a chip's records is the first rows of
the full table followed by zero rows, and the table of the records repeated is the rows repeated (riscv_row_cases.take).
Everything is bit-exact; there are no tolerances."""
import copy
import functools
import os
import subprocess

import numpy as np
import torch

import riscv_core_row_cases as K
import riscv_mem_row_cases as M
import riscv_row_cases as C
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_trace as RT

EXE = os.path.join(C.ROOT, "tests", "native", "riscv_sys_rows")
SYS_CHIPS = ("SyscallInstrs", "SyscallCore", "StateBump", "MemoryBump")
BINS = tuple(X.ALU_TRACEGEN_CHIPS) + tuple(X.MEM_TRACEGEN_CHIPS) + ("DivRem", "AluX0") + SYS_CHIPS
BIN_WORDS = (11,) * 14 + (12,) * 9 + (11,) * 4 + (4, 4)
SHAPES = C.SMALL_SHAPES + [C.TWO_WORKGROUPS]                    # (0, 32), (1, 32), (32, 32), (33, 64), (257, 288)
WINDOW = 1 << 24
OPC = R.OPC
ECALL_INC = 8 + RT.ECALL_EXTRA_CLK
# the register slots a chip's adapter reads (Tracer.fill_adapter): R = A B C, I = A B, ALU = A B and a register C, J = A
ADAPTER = {**{n: "R" for n in ("Add", "Sub", "Subw", "Mul", "DivRem", "SyscallInstrs")},
           **{n: "I" for n in ("Addi", "Branch", "Jalr") + tuple(X.MEM_TRACEGEN_CHIPS)},
           **{n: "ALU" for n in ("Addw", "ShiftRight", "Bitwise", "Lt", "ShiftLeft", "AluX0")}, "UType": "J", "Jal": "J"}
PROGRAMS = ("alu", "mem", "core")


@functools.lru_cache(maxsize=None)
def program(which):
    """(executor, shard) of riscv_row_cases.corner() / riscv_mem_row_cases.corner() / riscv_core_row_cases.executed()."""
    got = {"alu": C.corner, "mem": M.corner, "core": K.executed}[which]()
    return got[0], got[1]


def shift_of(sh):
    """The constant that puts the clock of the shard's middle instruction just above 2^24: a multiple of 8, as CPUState keeps every
    clock at 1 modulo 8."""
    return WINDOW - (int(sh.events[len(sh.events) // 2, X.E_CLK]) - 1)


def shifted(sh, d):
    """A copy of the shard with d added to every non-zero clock: a consistent shard that crosses a 2^24 boundary."""
    out = copy.copy(sh)
    ev, local = sh.events.copy(), sh.local.copy()
    for w in (X.E_CLK, X.E_A_PTS, X.E_B_PTS, X.E_C_PTS, X.E_M_PTS):
        ev[:, w] += d * (ev[:, w] != 0)
    for w in (1, 3):
        local[:, w] += d * (local[:, w] != 0)
    out.events, out.local, out.clk_start, out.clk_end = ev, local, sh.clk_start + d, sh.clk_end + d
    return out


@functools.lru_cache(maxsize=None)
def shard(which, shift):
    """shift: False, True (shift_of) or an integer."""
    ex, sh = program(which)
    if shift is False:
        return ex, sh
    return ex, shifted(sh, shift_of(sh) if shift is True else int(shift))


# ----------------------------------------------------------------------------------------------------------- the numpy partition
def conditions(ev):
    """The three conditions of bins 26..28 restated: (syscall_core [n], state_bump [n], pc_carry [n], inc [n], bumps [n, 3] for
    slots A, B, C)."""
    ev = np.asarray(ev, dtype=np.int64)
    op, a_prev, pc, clk = ev[:, X.E_OP], ev[:, X.E_A_PREV], ev[:, X.E_PC], ev[:, X.E_CLK]
    ecall = op == OPC["ECALL"]
    syscall_core = ecall & (((a_prev >> 8) & 0xFF) == 1)
    halt = ecall & ((a_prev & 0xFF) == 0)
    normal = ((op >= OPC["BEQ"]) & (op <= OPC["JALR"])) | halt
    pc_carry = ~normal & (((pc & 0xFFFF) + 4) > 0xFFFF)
    inc = np.where(ecall, ECALL_INC, 8)
    state_bump = pc_carry | (((clk & 0xFFFFFF) + inc) >= WINDOW)
    names = X.chip_of_events(ev)
    kind = np.array([ADAPTER[n] for n in names], dtype=object) if len(ev) else np.zeros(0, dtype=object)
    imm_c = (ev[:, X.E_FLAGS] & 2) == 2
    reads = np.stack([np.ones(len(ev), bool), kind != "J", (kind == "R") | ((kind == "ALU") & ~imm_c)], axis=1)
    cross = np.stack([(ev[:, w] >> 24) != ((clk + off) >> 24) for w, off in ((X.E_A_PTS, 4), (X.E_B_PTS, 3), (X.E_C_PTS, 2))], axis=1)
    return syscall_core, state_bump, pc_carry, inc, reads & cross


def bump_tuples(ev):
    """MemoryBump's records in the canonical order — by event, then slot A, B, C: int64 [m, 4] register, previous timestamp, value,
    window start."""
    ev = np.asarray(ev, dtype=np.int64)
    bumps = conditions(ev)[4]
    clk = ev[:, X.E_CLK]
    per = [np.stack([ev[:, r], ev[:, t], ev[:, v], ((clk + off) >> 24) << 24], axis=1)
           for r, t, v, off in ((X.E_OPA, X.E_A_PTS, X.E_A_PREV, 4), (X.E_OPB, X.E_B_PTS, X.E_B, 3), (X.E_OPC, X.E_C_PTS, X.E_C, 2))]
    return np.stack(per, axis=1).reshape(-1, 4)[bumps.reshape(-1)]


def reference_partition(ev):
    """{bin name: int64 [count, words]}: a stable partition by chip_of_events, packed by pack_alu_events / pack_mem_events."""
    ev = np.ascontiguousarray(ev, dtype=np.int64).reshape(-1, X.EV_WORDS)
    names = X.chip_of_events(ev)
    out = {}
    for name in BINS[:26]:
        rows = ev[names == name]
        out[name] = (X.pack_mem_events if name in X.MEM_TRACEGEN_CHIPS else X.pack_alu_events)(rows).reshape(-1, 12 if name in X.MEM_TRACEGEN_CHIPS else 11)
    syscall_core, state_bump, pc_carry, inc, _ = conditions(ev)
    out["SyscallCore"] = X.pack_alu_events(ev[syscall_core]).reshape(-1, 11)
    sb = ev[state_bump]
    out["StateBump"] = np.stack([sb[:, X.E_CLK], sb[:, X.E_PC], sb[:, X.E_NEXT_PC], inc[state_bump] | (pc_carry[state_bump].astype(np.int64) << 32)], axis=1)
    out["MemoryBump"] = bump_tuples(ev)
    return {n: np.ascontiguousarray(v, dtype=np.int64) for n, v in out.items()}


def arena_of(parts):
    """(counts [29], the arena as one int64 array) of a partition."""
    return np.array([len(parts[n]) for n in BINS], dtype=np.int64), np.concatenate([parts[n].reshape(-1) for n in BINS])


# -------------------------------------------------------------------------------------------------------------- synthetic events
def _base_event(which="core"):
    _, sh = program(which)
    return sh.events[sh.events[:, X.E_OP] == OPC["ECALL"]][0].copy()


@functools.lru_cache(maxsize=None)
def synthetic_ecalls():
    """ECALL events: every syscall id the IsZero columns name plus one other, each with the send bit 0 and 1; COMMIT and
    COMMIT_DEFERRED_PROOFS with each index 0..7 (and bits above the index); HALT and COMMIT_DEFERRED_PROOFS with limb 1 of op_b /
    op_c below, on and above (p - 1) >> 16."""
    base, rows = _base_event(), []
    top = (RT.P - 1) >> 16

    def add(sid, send, b, c):
        e = base.copy()
        i = len(rows)
        e[X.E_PC], e[X.E_CLK] = 0x78000000 + 4 * i + (0xFFFC if i % 5 == 0 else 0), base[X.E_CLK] + 8 * i
        e[X.E_NEXT_PC] = 1 if sid == 0 else e[X.E_PC] + 4
        e[X.E_A_PREV] = sid | send << 8 | (i % 3) << 16
        e[X.E_A] = K.s64(0x0123_4567_89AB_CDEF * (i + 1))
        e[X.E_B], e[X.E_C] = K.s64(b), K.s64(c)
        e[X.E_A_PTS], e[X.E_B_PTS], e[X.E_C_PTS] = max(e[X.E_CLK] - 20, 0), e[X.E_CLK] - 5, e[X.E_CLK] - 9 - i % 4
        rows.append(e)
    for sid in (0x03, 0xF0, 0x00, 0x10, 0x1A, 0x05):
        for send in (0, 1):
            add(sid, send, 0x1234_5678_9ABC, 0xFEDC_BA98_7654_3210)
    for sid in (0x10, 0x1A):
        for idx in range(8):
            add(sid, 0, idx | (0x50 if idx % 2 else 0), 0xA1B2_C3D4_0000_0000 | (top - 1 + idx % 3) << 16 | idx << 8 | (0xFF - idx))
    for limb in (top - 1, top, top + 1):
        add(0x00, 0, limb << 16 | 3, limb << 16 | 7)
        add(0x1A, 0, 2, limb << 16 | 9)
        add(0x10, 0, limb << 16 | 1, limb << 16)
    return np.array(rows, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def synthetic_state_events():
    """The pc's low limb at 0xFFFC and 0xFFF8 for a normal instruction, a branch, a JALR and HALT; clocks one step below a 2^24
    boundary; an ECALL's clock step straddling 2^24 where a normal instruction's does not."""
    _, sh = program("alu")
    ecall, rows = _base_event(), []
    pick = lambda name: sh.events[sh.events[:, X.E_OP] == OPC[name]][0].copy()
    for name in ("ADD", "BEQ", "JALR", "HALT", "ECALL"):
        for low in (0xFFFC, 0xFFF8):
            for clk in (3 * WINDOW + 800, 5 * WINDOW - 8, 7 * WINDOW - 100, 9 * WINDOW - ECALL_INC, 11 * WINDOW - ECALL_INC - 1):
                e = ecall.copy() if name in ("HALT", "ECALL") else pick(name)
                if name == "HALT":
                    e[X.E_A_PREV] = 0
                elif name == "ECALL":
                    e[X.E_A_PREV] = 0x0000_0002                    # WRITE
                e[X.E_PC], e[X.E_CLK] = 0x7801_0000 + low + (len(rows) << 16), clk
                e[X.E_NEXT_PC] = 1 if name == "HALT" else 0x7800_0010 + 8 * len(rows) if name in ("BEQ", "JALR") else e[X.E_PC] + 4
                for w in (X.E_A_PTS, X.E_B_PTS, X.E_C_PTS):
                    e[w] = clk - 16
                rows.append(e)
    return np.array(rows, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def synthetic_bump_events():
    """Register accesses whose previous timestamps lie 1, 2 and 70,000 windows back and at 0, on an R, an I, an ALU (register and
    immediate c) and a J instruction."""
    _, sh = program("alu")
    _, msh = program("mem")
    rows = []
    pick = lambda s, name: s.events[s.events[:, X.E_OP] == OPC[name]][0].copy()
    imm = sh.events[(sh.events[:, X.E_OP] == OPC["XOR"]) & ((sh.events[:, X.E_FLAGS] & 2) == 2) & (sh.events[:, X.E_OPA] != 0)][0].copy()
    reg = sh.events[(sh.events[:, X.E_OP] == OPC["XOR"]) & ((sh.events[:, X.E_FLAGS] & 2) == 0) & (sh.events[:, X.E_OPA] != 0)][0].copy()
    kinds = [pick(sh, "ADD"), pick(sh, "ADDI"), reg, imm, pick(sh, "LUI"), pick(msh, "SD"), _base_event()]
    w0 = 70_001
    patterns = [(1, 2, 70_000), (70_000, 1, 2), (2, 70_000, 1), (None, None, None), (0, 0, 0), (1, 0, None), (None, 2, 0)]    # windows back; None: previous timestamp 0
    for k, e0 in enumerate(kinds):
        for j, pat in enumerate(patterns):
            e = e0.copy()
            clk = w0 * WINDOW + 8 * (len(rows) + 3)
            e[X.E_CLK] = clk
            for w, back in zip((X.E_A_PTS, X.E_B_PTS, X.E_C_PTS), pat):
                e[w] = 0 if back is None else clk - back * WINDOW - (3 + j)
            rows.append(e)
    edge = pick(sh, "ADD")                                             # the access itself on a boundary: slot C below it, B and A on and above
    edge[X.E_CLK] = 3 * WINDOW - 3
    edge[X.E_A_PTS], edge[X.E_B_PTS], edge[X.E_C_PTS] = 3 * WINDOW - 9, 3 * WINDOW - 9, 3 * WINDOW - 9
    rows.append(edge)
    return np.array(rows, dtype=np.int64)


SYNTHETIC = {"ecalls": synthetic_ecalls, "state": synthetic_state_events, "bumps": synthetic_bump_events}
SOURCES = [(p, s) for p in PROGRAMS for s in (False, True)] + [(s, None) for s in SYNTHETIC]


@functools.lru_cache(maxsize=None)
def source_events(source):
    """(executor, the shard the events are set in, events [n, 20]) of a source: (program, shifted?) or (synthetic set, None)."""
    which, shift = source
    if which in SYNTHETIC:
        ex, sh = program("core")
        return ex, sh, SYNTHETIC[which]()
    ex, sh = shard(which, shift)
    return ex, sh, sh.events


# ------------------------------------------------------------------------------------------------------- the host tracer's tables
@functools.lru_cache(maxsize=None)
def host_tables(source):
    """({chip: int64 [rows, width]} of the four small chips, rows without padding, by the host tracer's fillers over the source's
    events — MemoryBump from Tracer._bump_rows fed the canonically ordered tuples —, {chip: records [rows, words]}, SyscallCore's Global
    events reduced to 9 words)."""
    ex, sh, ev = source_events(source)
    edited = copy.copy(sh)
    edited.events = np.ascontiguousarray(ev)
    tr = X.EventTracer(ex, edited, "cpu")
    tr.syscall_instrs()
    tr.state_chain()
    tup = bump_tuples(ev)
    tr.bumps = [tuple(torch.as_tensor(np.ascontiguousarray(tup[:, i])) for i in range(4))] if len(tup) else []
    tr._bump_rows()
    parts = reference_partition(ev)
    tables = {}
    for name in SYS_CHIPS:
        n = len(parts[name])
        tables[name] = tr.tables[name].main[:n] if name in tr.tables else torch.zeros((0, R.chip(name)[0].main_width), dtype=RT.I64)
        assert tables[name].shape[0] == n, (source, name, tables[name].shape[0], n)
    events = np.zeros((0, 9), dtype=np.int32)
    if "SyscallCore" in tr.tables:
        t_ = tr.tables["SyscallCore"]
        ev11 = torch.cat([v for _, v, _ in RT.eval_interactions(R.chip("SyscallCore")[1], t_.main[:t_.n], None, kinds=(R.GLOBAL,))])
        events = K.reduce_global_events(ev11)
    return tables, {n: parts[n] for n in SYS_CHIPS}, events


def case(source, name, n, height):
    """(records [n, words], the Montgomery column-major host table [width, height]) of the first n records of the source's chip."""
    tables, records, _ = host_tables(source)
    rec, full = records[name], tables[name]
    assert len(rec) or n == 0
    want = torch.cat([C.take(full, n), torch.zeros((height - n, full.shape[1]), dtype=RT.I64)])
    return np.ascontiguousarray(C.take(rec, n)), C.montgomery_col_major(want)


def shapes(source, name):
    n = len(host_tables(source)[1][name])
    return (SHAPES + [(n, RT.pad32(n))]) if n else [(0, 32)]


# ----------------------------------------------------------------------------------------------------------- the native program
def _run(args, src_data, tmp_path, tag, timeout=120):
    src, dst = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(src_data, dtype=np.int64).tobytes())
    subprocess.run([EXE, "host"] + [src if a == "IN" else dst if a == "OUT" else a for a in args], check=True, capture_output=True, timeout=timeout)
    return dst


def run_rows(name, rec, height, tmp_path):
    """tests/native/riscv_sys_rows host rows: the table as uint32 numpy [width, height]."""
    dst = _run(["rows", name, "IN", str(height), "OUT"], rec, tmp_path, "%s_%d_%d" % (name, len(rec), height))
    return np.fromfile(dst, dtype=np.uint32).reshape(R.chip(name)[0].main_width, height)


def run_global(rec, tmp_path):
    return np.fromfile(_run(["global", "IN", "OUT"], rec, tmp_path, "global_%d" % len(rec)), dtype=np.int32).reshape(-1, 9)


def run_partition(ev, tmp_path):
    """tests/native/riscv_sys_rows host partition: (counts [29], arena) as int64 numpy."""
    words = np.fromfile(_run(["partition", "IN", "OUT"], ev, tmp_path, "partition_%d" % len(ev)), dtype=np.int64)
    return words[:len(BINS)], words[len(BINS):]
