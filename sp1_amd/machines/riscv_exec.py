"""Real guest programs: the rv64im executor of libsp1hip.so (sp1_amd/csrc/rv64_exec.cpp) and, from its events, the tables of
every chip of a core shard — what `MinimalExecutor` + `TracingVM` + the chips' `generate_trace_into` do in the reference
(/root/reference/crates/core/executor/src/{minimal,tracing,vm}.rs; crates/core/machine/src/**/trace.rs as cited in
riscv_trace.py, whose column fillers this module drives with executed events instead of the synthetic loop body).

    ex = Executor(open(elf, "rb").read(), stdin=[n.to_bytes(4, "little")])
    for shard in ex.shards(max_cycles=1 << 21):               # ExecutedShard: events, local memory, public values
        machine, tables, publics = shard_tables(ex, shard, device)   # every chip's (prep, main), ready for api.prove_shard
    for rec in run_records(ex, max_cycles=1 << 21):           # ShardRecords: every shard of the run — core, precompile, memory — cut once
        machine, tables, publics, gev = host_shard(ex, rec)   # ... or device_shard(ex, rec, prep): every table made on the device

The proof statement per shard is the reference's: the chips of the shard's shape cluster (those without events at height zero),
their constraints on every row, and the Byte / Range / Program / Memory / State buses balanced against the messages the shard's
PUBLIC VALUES send and receive (`eval_public_values`, public_values.py: the initial and final CPU state, the ends of the Global
accumulation and of the memory-initialisation chains); what crosses shards (memory states, syscalls) goes through the Global chip's
digest, and the public values chain from shard to shard as `SP1Prover::verify` requires (public_values.verify_proof_public_values).
"""
import ctypes as C
import dataclasses
import functools
import gzip
import os
import types
from collections.abc import Mapping

import numpy as np
import torch

from .. import _lib
from . import public_values as PVM
from . import riscv as R
from . import riscv_trace as RT
from .riscv_trace import I64, MASK16, OPC, P, POS_OFF, Table, limbs16

EV_WORDS, KECCAK_WORDS, POSEIDON2_WORDS, SHA_EXTEND_WORDS, SHA_COMPRESS_WORDS, UINT256_WORDS = 20, 77, 26, 786, 155, 31
SECP_ADD_WORDS, SECP_DOUBLE_WORDS = 43, 26
PRECOMPILE_KINDS = ("keccak", "poseidon2", "sha_extend", "sha_compress", "uint256", "secp256k1_add", "secp256k1_double")   # ExecutedShard's attributes
# kind: (SP1HIP_RV64_FAMILY_*, chip) — the field / curve precompiles behind sp1hip_rv64_precompile_events (include/sp1hip.h)
FAMILIES = {"secp256r1_add": (0, "Secp256r1AddAssign"), "secp256r1_double": (1, "Secp256r1DoubleAssign"), "bn254_add": (2, "Bn254AddAssign"),
            "bn254_double": (3, "Bn254DoubleAssign"), "bls12381_add": (4, "Bls12381AddAssign"), "bls12381_double": (5, "Bls12381DoubleAssign"),
            "bn254_fp": (6, "Bn254FpOpAssign"), "bls12381_fp": (7, "Bls12381FpOpAssign"), "bn254_fp2_addsub": (8, "Bn254Fp2AddSubAssign"),
            "bls12381_fp2_addsub": (9, "Bls12381Fp2AddSubAssign"), "bn254_fp2_mul": (10, "Bn254Fp2MulAssign"), "bls12381_fp2_mul": (11, "Bls12381Fp2MulAssign"),
            "ed_add": (12, "EdAddAssign"), "ed_decompress": (13, "EdDecompress"), "uint256_ops": (14, "Uint256Ops")}
(E_PC, E_CLK, E_OP, E_OPA, E_OPB, E_OPC, E_FLAGS, E_A, E_B, E_C, E_A_PREV, E_A_PTS, E_B_PTS, E_C_PTS, E_MADDR, E_M_PTS, E_M_PREV, E_M_NEW,
 E_NEXT_PC, E_SPARE) = range(EV_WORDS)


GUESTS_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "bench", "programs")


def guest_file(name):
    """The bytes of bench/programs/<name>.gz: the reference's guest binaries (and rsp's input) are stored gzip-compressed,
    unmodified otherwise (bench/programs/README.md)."""
    with gzip.open(os.path.join(GUESTS_DIR, name + ".gz"), "rb") as f:
        return f.read()


class ExecutedShard:
    """One shard of an execution: `events` [n, 20] / `local` [m, 5] / `keccak` [k, 77] int64 arrays (two's complement images of
    the executor's u64 words) and the shard's public-value fields."""

    def __init__(self, info, events, local, keccak, poseidon2, sha_extend, sha_compress, uint256, secp_add, secp_double):
        self.index, self.cycles = int(info.shard), int(info.n_cycles)
        self.events, self.local, self.keccak, self.poseidon2 = events, local, keccak, poseidon2
        self.sha_extend, self.sha_compress, self.uint256 = sha_extend, sha_compress, uint256
        self.secp256k1_add, self.secp256k1_double = secp_add, secp_double
        self.families = {}                                        # kind (FAMILIES) -> [n, words] events, only the kinds that occurred
        self.pc_start, self.next_pc = int(info.pc_start), int(info.next_pc)
        self.clk_start, self.clk_end = int(info.clk_start), int(info.clk_end)
        self.halted, self.exit_code = bool(info.halted), int(info.exit_code)
        self.commit_syscall, self.commit_deferred_syscall = int(info.commit_syscall), int(info.commit_deferred_syscall)
        self.committed_value_digest = [int(x) for x in info.committed_value_digest]
        self.deferred_proofs_digest = [int(x) for x in info.deferred_proofs_digest]
        self.estimated_area, self.estimated_max_height = int(info.estimated_area), int(info.estimated_max_height)

    def precompile_events(self):
        """{kind: events} of the shard's precompile calls, only the kinds that occurred: the seven named attributes, then `families`."""
        named = {kind: getattr(self, kind) for kind in PRECOMPILE_KINDS}
        return {kind: events for kind, events in {**named, **self.families}.items() if events.shape[0]}


class Executor:
    def __init__(self, elf, stdin=()):
        self.lib = _lib.load()
        buf = (C.c_uint8 * len(elf)).from_buffer_copy(elf)
        h = C.c_void_p()
        _lib.check(self.lib.sp1hip_rv64_create(buf, len(elf), C.byref(h)))
        self.h = h
        for entry in stdin:
            self.write_stdin(entry)
        self.halted = False

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.sp1hip_rv64_destroy(self.h)
            self.h = None

    def write_stdin(self, data):
        data = bytes(data)
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        _lib.check(self.lib.sp1hip_rv64_write_stdin(self.h, buf, len(data)))

    @staticmethod
    def _matrix(ptr, rows, cols, copy=True):
        if rows == 0:
            return np.zeros((0, cols), dtype=np.int64)
        m = np.ctypeslib.as_array(ptr, shape=(rows * cols,)).view(np.int64).reshape(rows, cols)
        return m.copy() if copy else m

    def run_shard(self, max_cycles, record=True, copy=True):
        """The next shard. record=False: run it without keeping its instruction events (`events` comes back empty).
        copy=False: `events` is a view of the executor's buffer, valid until the next run_shard (a full shard is 1.3 GB)."""
        _lib.check(self.lib.sp1hip_rv64_set_recording(self.h, int(bool(record))))
        info = _lib.Rv64ShardInfo()
        _lib.check(self.lib.sp1hip_rv64_run_shard(self.h, int(max_cycles), C.byref(info)))
        n_events = info.n_events if record else 0
        shard = ExecutedShard(info, self._matrix(self.lib.sp1hip_rv64_events(self.h), n_events, EV_WORDS, copy),
                              self._matrix(self.lib.sp1hip_rv64_local_memory(self.h), info.n_local, 5),
                              self._matrix(self.lib.sp1hip_rv64_keccak_events(self.h), info.n_keccak, KECCAK_WORDS),
                              self._matrix(self.lib.sp1hip_rv64_poseidon2_events(self.h), info.n_poseidon2, POSEIDON2_WORDS),
                              self._matrix(self.lib.sp1hip_rv64_sha_extend_events(self.h), info.n_sha_extend, SHA_EXTEND_WORDS),
                              self._matrix(self.lib.sp1hip_rv64_sha_compress_events(self.h), info.n_sha_compress, SHA_COMPRESS_WORDS),
                              self._matrix(self.lib.sp1hip_rv64_uint256_events(self.h), info.n_uint256, UINT256_WORDS),
                              self._matrix(self.lib.sp1hip_rv64_secp256k1_add_events(self.h), info.n_secp256k1_add, SECP_ADD_WORDS),
                              self._matrix(self.lib.sp1hip_rv64_secp256k1_double_events(self.h), info.n_secp256k1_double, SECP_DOUBLE_WORDS))
        n_ev, n_words, data = C.c_uint64(), C.c_uint64(), C.POINTER(C.c_uint64)()
        for kind, (family, _) in FAMILIES.items():
            _lib.check(self.lib.sp1hip_rv64_precompile_events(self.h, family, C.byref(n_ev), C.byref(n_words), C.byref(data)))
            if n_ev.value:
                shard.families[kind] = self._matrix(data, n_ev.value, n_words.value)
        self.halted = shard.halted
        return shard

    def cut_by_area(self, element_threshold=None, height_threshold=None):
        """Shards end where the reference's executor would end them (`ShapeChecker`, vm/shapes.rs; thresholds opts.rs:L12-L14):
        when the estimated trace area or a table's height reaches its threshold. The cost model — columns per chip — is this
        package's chips' (pinned to rv64im_costs.json); the estimator itself runs inside the executor, instruction by instruction."""
        cost = lambda name: (lambda a: a.main_width + a.prep_width)(R.chip(name)[0])
        lim = _lib.Rv64ShardLimits()
        lim.element_threshold = ELEMENT_THRESHOLD if element_threshold is None else element_threshold
        lim.height_threshold = HEIGHT_THRESHOLD if height_threshold is None else height_threshold
        rows = self.program()[1].shape[0]
        lim.fixed_area = -(-rows // 32) * 32 * cost("Program") + (1 << 16) * cost("Byte") + (1 << 17) * cost("Range")
        chips = {}
        for name, o in OPC.items():
            if o <= OPC["REMUW"]:
                chip = _ALU_CHIP[o]
            elif name in _MEM_CHIP:
                chip = _MEM_CHIP[name]
            elif name in RT.BRANCH_OPS:
                chip = "Branch"
            else:
                chip = {"JAL": "Jal", "JALR": "Jalr", "AUIPC": "UType", "LUI": "UType", "ECALL": "SyscallInstrs"}.get(name)
            if chip is not None:
                lim.opcode_cost[o], lim.opcode_chip[o] = cost(chip), chips.setdefault(chip, len(chips))
        lim.alu_x0_cost, lim.load_x0_cost, lim.memory_local_cost, lim.global_cost = cost("AluX0"), cost("LoadX0"), cost("MemoryLocal"), cost("Global")
        lim.syscall_core_cost, lim.memory_bump_cost, lim.state_bump_cost = cost("SyscallCore"), cost("MemoryBump"), cost("StateBump")
        _lib.check(self.lib.sp1hip_rv64_set_shard_limits(self.h, C.byref(lim)))
        return self

    def shards(self, max_cycles):
        while not self.halted:
            yield self.run_shard(max_cycles)

    def program(self):
        """(pc_base, [n, 6] int64: opcode, op_a, op_b, op_c, imm_b, imm_c)."""
        base, n, tab = C.c_uint64(), C.c_uint64(), C.POINTER(C.c_uint64)()
        _lib.check(self.lib.sp1hip_rv64_program(self.h, C.byref(base), C.byref(n), C.byref(tab)))
        return int(base.value), self._matrix(tab, n.value, 6)

    def global_memory(self):
        """[t, 4] int64 per address the run touched: address, initial value, final value, final timestamp."""
        n, tab = C.c_uint64(), C.POINTER(C.c_uint64)()
        _lib.check(self.lib.sp1hip_rv64_global_memory(self.h, C.byref(n), C.byref(tab)))
        return self._matrix(tab, n.value, 4)

    def memory_image(self):
        """[m, 2] int64: (address, value) of every 8-byte word of the ELF's segments, ascending (`Program::memory_image`)."""
        n, tab = C.c_uint64(), C.POINTER(C.c_uint64)()
        _lib.check(self.lib.sp1hip_rv64_memory_image(self.h, C.byref(n), C.byref(tab)))
        return self._matrix(tab, n.value, 2)

    def output(self, which=0):
        p, n = _lib.u8p(), C.c_uint64()
        _lib.check(self.lib.sp1hip_rv64_output(self.h, which, C.byref(p), C.byref(n)))
        return bytes(np.ctypeslib.as_array(p, shape=(n.value,))) if n.value else b""


# ---------------------------------------------------------------------------------------------------------------------
# events -> tables
_OPN = {v: k for k, v in OPC.items()}
_ALU_CHIP = {}
for _chip, _ops in RT.ALU_KINDS.items():
    for _o in _ops:
        _ALU_CHIP[OPC[_o]] = _chip
_MEM_CHIP = {"LB": "LoadByte", "LBU": "LoadByte", "LH": "LoadHalf", "LHU": "LoadHalf", "LW": "LoadWord", "LWU": "LoadWord", "LD": "LoadDouble",
             "SB": "StoreByte", "SH": "StoreHalf", "SW": "StoreWord", "SD": "StoreDouble"}
PV, PV_WORDS = PVM.PV, PVM.NUM_PV_ELTS                # PublicValues word offsets (public_values.py)


def chip_of_events(ev):
    """The table every executed instruction goes to (tracing.rs: emit_alu_event L1153-L1228, emit_mem_instr_event L1096-L1150)."""
    op, rd = ev[:, E_OP], ev[:, E_OPA]
    names = np.empty(len(op), dtype=object)
    for o in np.unique(op):
        nm = _OPN[int(o)]
        m = op == o
        if o <= OPC["REMUW"]:
            names[m & (rd != 0)] = _ALU_CHIP[int(o)]
            names[m & (rd == 0)] = "AluX0"
        elif nm in _MEM_CHIP:
            names[m] = _MEM_CHIP[nm]
            if nm.startswith("L"):
                names[m & (rd == 0)] = "LoadX0"
        elif nm in RT.BRANCH_OPS:
            names[m] = "Branch"
        else:
            names[m] = {"JAL": "Jal", "JALR": "Jalr", "AUIPC": "UType", "LUI": "UType", "ECALL": "SyscallInstrs"}[nm]
    return names


class EventView:
    """An `ExecutedShard` behind the interface riscv_trace.Tracer's column fillers read an execution through: one "iteration"
    (K = 1) whose positions are the shard's executed instructions."""
    K = 1

    def __init__(self, shard, pc_base, device):
        self.dev = torch.device(device)
        ev = torch.as_tensor(shard.events, device=self.dev)
        self.ev, self.L, self.clk0 = ev, ev.shape[0], shard.clk_start
        self.op = ev[:, E_OP]
        imm_b, imm_c = (ev[:, E_FLAGS] & 1) == 1, (ev[:, E_FLAGS] & 2) == 2
        self.has_imm = imm_c
        self.imm = torch.where(self.op == OPC["JAL"], ev[:, E_OPB], ev[:, E_OPC])
        neg = torch.full_like(self.op, -1)
        self.slot_reg = {"A": ev[:, E_OPA], "B": torch.where(imm_b, neg, ev[:, E_OPB]), "C": torch.where(imm_c, neg, ev[:, E_OPC])}
        self.W = ev[:, E_A][None, :]
        self.values = {"A": ev[:, E_A_PREV], "B": ev[:, E_B], "C": ev[:, E_C]}
        self.prev_ts = {"A": ev[:, E_A_PTS], "B": ev[:, E_B_PTS], "C": ev[:, E_C_PTS]}
        self.clk_inc = torch.where(self.op == OPC["ECALL"], 8 + RT.ECALL_EXTRA_CLK, 8)
        self.body = types.SimpleNamespace(chip=chip_of_events(shard.events), pc_base=pc_base)

    def T(self, k, p):
        return self.ev[p, E_CLK]

    def pc(self, p):
        return self.ev[p, E_PC]

    def reg_value(self, k, p, slot):
        return self.values[slot][p]

    def _grid(self, positions):
        p = torch.as_tensor(np.asarray(positions, dtype=np.int64), device=self.dev)
        return torch.zeros_like(p), p


class EventTracer(RT.Tracer):
    """riscv_trace.Tracer over executed events. The per-chip column fillers (adapters, ALU / shift / multiply / divide
    operations, load / store chips, SyscallInstrs, Global) are the base class's; what changes is where the timeline comes from:
    previous timestamps and memory states are the executor's records instead of the loop body's static analysis."""

    def __init__(self, executor, shard, device="cpu", prev=None):
        """prev: the public values of the previous shard in execution order (a list of words) or None for the first — where
        prev_committed_value_digest, prev_exit_code and the prev_commit_* flags come from (verify.rs:L262-L296, L445-L480)."""
        self.pc_base, self.program = executor.program()
        self.shard, self.prev = shard, prev
        super().__init__(EventView(shard, self.pc_base, device))
        self.real_global = True

    def _prev_ts(self, k, p, slot):
        return self.ex.prev_ts[slot][p]

    def build(self):
        def alu_x0(tb, k, p, a, bv, cv):
            tb.set("opcode", self.ex.op[p])
            tb.set("is_real", 1)
        self.simple_alu("AluX0", "ALU", alu_x0)
        return super().build()

    def branch(self):
        super().branch()
        if "Branch" in self.tables:
            _, p = self.rows_of("Branch")
            self.tables["Branch"].set("next_pc", limbs16(self.ex.ev[p, E_NEXT_PC])[:, :3])

    def jalr(self):
        super().jalr()
        if "Jalr" in self.tables:
            _, p = self.rows_of("Jalr")
            tb, rd0 = self.tables["Jalr"], self.ex.slot_reg["A"][p] == 0
            tb.set("op_a_value", limbs16(self.ex.pc(p) + 4) * (~rd0).to(I64)[:, None])

    def memory_instructions(self):
        ex, ev = self.ex, self.ex.ev
        self.mem_words = None
        for c in list(RT.LOAD_KINDS) + list(RT.STORE_KINDS):
            k, p = self.rows_of(c)
            if len(p):
                self.fill_mem_chip(c, k, p, ev[p, E_MADDR], ev[p, E_CLK] + POS_OFF["M"], ev[p, E_M_PTS], ev[p, E_M_PREV], ev[p, E_M_NEW],
                                   ex.values["A"][p])

    def state_chain(self):
        ex, ev, dev = self.ex, self.ex.ev, self.dev
        T, pc, nxt_pc, inc = ev[:, E_CLK], ev[:, E_PC], ev[:, E_NEXT_PC], ex.clk_inc
        op = ex.op
        halt = (op == OPC["ECALL"]) & ((ev[:, E_A_PREV] & 0xFF) == 0)
        normal_pc = ((op >= OPC["BEQ"]) & (op <= OPC["JALR"])) | halt                    # these rows send next_pc in normal form
        pc_carry = (~normal_pc) & (((pc & MASK16) + 4) > MASK16)
        clk_carry = ((T & 0xFFFFFF) + inc) >= (1 << 24)
        need = pc_carry | clk_carry
        self.final_state = (self.shard.clk_end, self.shard.next_pc)
        if bool(need.any()):
            Tn, pcn, nxt, pcc, incn = T[need], pc[need], nxt_pc[need], pc_carry[need], inc[need]
            air, _ = R.chip("StateBump")
            tb = Table(air, len(Tn), dev)
            self.tables["StateBump"] = tb
            nT = Tn + incn
            tb.set("next_clk_32_48", nT >> 32)
            tb.set("next_clk_24_32", (nT >> 24) & 0xFF)
            tb.set("next_clk_16_24", (nT >> 16) & 0xFF)
            tb.set("next_clk_0_16", nT & MASK16)
            tb.set("clk_high", Tn >> 24)
            tb.set("clk_low", (Tn & 0xFFFFFF) + incn)
            tb.set("next_pc", limbs16(nxt)[:, :3])
            sent = limbs16(pcn)[:, :3].clone()
            sent[:, 0] += 4
            tb.set("pc", torch.where(pcc[:, None], sent, limbs16(nxt)[:, :3]))
            tb.set("is_clk", ((nT >> 24) != (Tn >> 24)).to(I64))
            tb.set("is_real", 1)

    def memory_local_and_bumps(self):
        dev = self.dev
        loc = torch.as_tensor(self.shard.local, device=dev)
        addr, it, iv, ft, fv = (loc[:, i] for i in range(5))
        air, _ = R.chip("MemoryLocal")
        tb = Table(air, len(addr), dev)
        self.tables["MemoryLocal"] = tb
        tb.set("addr", limbs16(addr)[:, :3])
        tb.set("initial_clk_high", it >> 24)
        tb.set("initial_clk_low", it & 0xFFFFFF)
        tb.set("final_clk_high", ft >> 24)
        tb.set("final_clk_low", ft & 0xFFFFFF)
        for tag, v in (("initial", iv), ("final", fv)):
            l = limbs16(v)
            tb.set(tag + "_value", l)
            tb.set(tag + "_value_lower", l[:, 2] & 0xFF)
            tb.set(tag + "_value_upper", l[:, 2] >> 8)
        tb.set("is_real", 1)
        self._bump_rows()

    def _program_table(self):
        return RT.program_table(self.program, self.pc_base, self.dev, executed_pc=self.ex.ev[:, E_PC])

    def public_values(self):
        return execution_public_values(self.shard, self.prev)

    def finish(self):
        ex, dev, sh = self.ex, self.dev, self.shard
        machine = {name: R.chip(name) for name in self.tables}
        pv = self.public_values()
        ml = self.tables["MemoryLocal"]
        (_, recv, _), (_, send, _) = RT.eval_interactions(R.chip("MemoryLocal")[1], ml.main[:ml.n], None, kinds=(R.GLOBAL,))
        events = [torch.stack([recv, send], dim=1).reshape(-1, 11)]
        if "SyscallCore" in self.tables:
            t_ = self.tables["SyscallCore"]
            events += [v for _, v, _ in RT.eval_interactions(R.chip("SyscallCore")[1], t_.main[:t_.n], None, kinds=(R.GLOBAL,))]
        self.global_events = torch.cat(events)
        PVM.set_global(pv, *self.global_chip(machine, self.global_events))
        self.tables["Program"], machine["Program"] = self._program_table()
        self.byte_range_tables(machine, pv)
        self.fill_cluster(machine, RT.smallest_cluster(machine))
        self.pv = pv
        names = sorted(machine)
        return [machine[n] for n in names], {n: (self.tables[n].prep, self.tables[n].main) for n in names}, PVM.to_tensor(pv)


ALU_TRACEGEN_CHIPS = ("Add", "Addi", "Sub", "Addw", "Subw", "Mul", "ShiftRight", "Branch",   # api.RISCV_ALU_CHIPS: tables made on the device
                      "Bitwise", "Lt", "ShiftLeft", "UType", "Jal", "Jalr")


def pack_alu_events(events, chip=None):
    """The executor's 20-word instruction events -> `sp1hip_rv64_alu_event_t` records (include/sp1hip.h: 11 u64 words — pc, clk,
    ops, a, b, c, a_prev, a_pts, b_pts, c_pts, aux) for the chips whose tables the device generates (api.tracegen_riscv_alu), in
    the events' order = the tables' row order. `events`: [n, 20] int64 (numpy or torch; all of a shard's events when `chip` names
    the chip to select, else already that chip's). An event is 88 bytes where the row it becomes is 120 (Addi) to 328 (Mul).
    An operand b that is an immediate (JAL, LUI, AUIPC: flag bit 32) travels as `b`, with 0 in the op_b field of `ops`."""
    ev = events if chip is None else events[np.nonzero(chip_of_events(np.asarray(events.cpu() if torch.is_tensor(events) else events)) == chip)[0]]
    xp = torch if torch.is_tensor(ev) else np
    flags = ev[:, E_FLAGS]
    imm_b, imm_c = flags & 1, (flags & 2) >> 1
    ops = (ev[:, E_OP] | (ev[:, E_OPA] << 8) | (((1 - imm_b) * (ev[:, E_OPB] & 0xFF)) << 16) | (((1 - imm_c) * (ev[:, E_OPC] & 0xFF)) << 24)
           | ((flags & 3) << 32))
    b = xp.where(imm_b == 1, ev[:, E_OPB], ev[:, E_B])                   # an immediate operand travels as the value
    c = xp.where(imm_c == 1, ev[:, E_OPC], ev[:, E_C])
    cols = [ev[:, E_PC], ev[:, E_CLK], ops, ev[:, E_A], b, c, ev[:, E_A_PREV], ev[:, E_A_PTS], ev[:, E_B_PTS], ev[:, E_C_PTS], ev[:, E_NEXT_PC]]
    return xp.stack(cols, 1) if xp is np else torch.stack(cols, dim=1).contiguous()


MEM_TRACEGEN_CHIPS = ("LoadByte", "LoadHalf", "LoadWord", "LoadDouble", "LoadX0",           # api.RISCV_MEM_CHIPS: tables made on the device
                      "StoreByte", "StoreHalf", "StoreWord", "StoreDouble")


def pack_mem_events(events, chip=None):
    """The executor's 20-word instruction events -> `sp1hip_rv64_mem_event_t` records (include/sp1hip.h: 12 u64 words — pc, clk,
    ops, b, imm, a_prev, a_pts, b_pts, m_addr, m_pts, m_prev, m_new) for the load and store chips whose tables the device generates
    (api.tracegen_riscv_mem), in the events' order = the tables' row order. `events`: [n, 20] int64 (numpy or torch; all of a
    shard's events when `chip` names the chip to select, else already that chip's). An event is 96 bytes where the row it becomes
    is 156 (the Double chips) to 200 (StoreByte). Address, previous word and new word are the executor's records as they are."""
    ev = events if chip is None else events[np.nonzero(chip_of_events(np.asarray(events.cpu() if torch.is_tensor(events) else events)) == chip)[0]]
    ops = ev[:, E_OP] | (ev[:, E_OPA] << 8) | ((ev[:, E_OPB] & 0xFF) << 16)
    cols = [ev[:, E_PC], ev[:, E_CLK], ops, ev[:, E_B], ev[:, E_OPC], ev[:, E_A_PREV], ev[:, E_A_PTS], ev[:, E_B_PTS], ev[:, E_MADDR], ev[:, E_M_PTS],
            ev[:, E_M_PREV], ev[:, E_M_NEW]]
    return np.stack(cols, 1) if not torch.is_tensor(ev) else torch.stack(cols, dim=1).contiguous()


def core_device_tables(shard_events, heights, stream=None):
    """The tables of a core shard that the device makes itself: {name: api.ColMajor} for every chip of ALU_TRACEGEN_CHIPS +
    MEM_TRACEGEN_CHIPS with a non-zero entry in `heights` ({name: rows of its table, padding included}). `shard_events`: the
    shard's [n, 20] instruction events, numpy or torch; the records are packed where the events are (a host array is packed on
    the host and the 88- / 96-byte records are what crosses to the device), then api.tracegen_riscv_alu / _mem fill the tables."""
    from .. import api
    on_host = not (torch.is_tensor(shard_events) and shard_events.is_cuda)
    names = chip_of_events(np.asarray(shard_events.cpu() if torch.is_tensor(shard_events) else shard_events))
    out = {}
    for chips, pack, gen in ((ALU_TRACEGEN_CHIPS, pack_alu_events, api.tracegen_riscv_alu), (MEM_TRACEGEN_CHIPS, pack_mem_events, api.tracegen_riscv_mem)):
        for name in chips:
            if not heights.get(name):
                continue
            rows = np.nonzero(names == name)[0]
            packed = pack(shard_events[rows] if on_host else shard_events[torch.as_tensor(rows, device=shard_events.device)])
            if on_host:
                packed = torch.as_tensor(np.ascontiguousarray(packed)).cuda()
            out[name] = gen(name, packed, int(heights[name]), stream=stream)
    return out


REST_TRACEGEN_CHIPS = ("DivRem", "AluX0", "MemoryLocal", "Global")                          # core_device_tables_rest: made on the device too


def global_events_9(events11):
    """Global interaction events as eval_interactions yields them ([m, 11]: message[8], is_send, is_receive, kind; a torch tensor)
    -> the [m, 9] int32 form api.tracegen_riscv_global reads: message[8], is_receive | kind << 8."""
    ev = events11.to(torch.int64)
    return torch.cat([ev[:, :8], (ev[:, 9] | (ev[:, 10] << 8))[:, None]], dim=1).to(torch.int32)


def global_digest(table, count):
    """The digest a device-made Global table (api.ColMajor) accumulates to: its row count - 1's accumulation.cumulative_sum_x / _y,
    14 canonical words read back; the curve's start point when there is no event."""
    if not count:
        return [int(v) for xy in R.CURVE_CUMULATIVE_SUM_START for v in xy]
    lay = R.chip("Global")[0].layout
    cols = [lay["accumulation.cumulative_sum_" + axis] + j for axis in "xy" for j in range(7)]
    words = table.words.view(table.width, table.height)[cols, count - 1].cpu().numpy().view(np.uint32).astype(np.uint64)
    return [int(v) for v in words * np.uint64(pow(1 << 32, -1, P)) % np.uint64(P)]


def core_device_tables_rest(shard, heights, syscall_global_events=None, stream=None):
    """The DivRem, AluX0, MemoryLocal and Global tables of a core shard, made on the device: ({name: api.ColMajor} for each of them
    with a non-zero entry in `heights` ({name: rows of its table, padding included}), (global_count, digest[14])). `shard`: an
    ExecutedShard — DivRem and AluX0 come from its instruction events (pack_alu_events, packed where the events are: only the 88-byte
    records cross to the device), MemoryLocal from its 40-byte `local` records as they are. The MemoryLocal kernel also writes its
    rows' Global events; `syscall_global_events` ([m, 11] as eval_interactions yields them for SyscallCore, or None) are appended
    in the 9-word form, and api.tracegen_riscv_global makes the Global table from them: no host table is read. global_count is the
    number of events, the digest the last real row's accumulation.cumulative_sum_x / _y of the device table (canonical words; the
    curve's start point when there is no event) — the two public values the Global chip defines. MemoryBump, StateBump, SyscallInstrs
    and SyscallCore stay with the host tracer: a handful of rows per shard."""
    with torch.cuda.stream(stream or torch.cuda.current_stream()):     # the uploads and copies go where the kernels go
        return _core_device_tables_rest(shard, heights, syscall_global_events, stream)


def _core_device_tables_rest(shard, heights, syscall_global_events, stream):
    from .. import api
    events, out = shard.events, {}
    on_host = not (torch.is_tensor(events) and events.is_cuda)
    names = chip_of_events(np.asarray(events.cpu() if torch.is_tensor(events) else events))
    for name, gen in (("DivRem", api.tracegen_riscv_divrem), ("AluX0", api.tracegen_riscv_alu_x0)):
        if not heights.get(name):
            continue
        rows = np.nonzero(names == name)[0]
        packed = pack_alu_events(events[rows] if on_host else events[torch.as_tensor(rows, device=events.device)])
        if on_host:
            packed = torch.as_tensor(np.ascontiguousarray(packed)).cuda()
        out[name] = gen(packed, int(heights[name]), stream=stream)
    m = 0 if syscall_global_events is None else int(syscall_global_events.shape[0])
    _, count, digest = _local_and_global_tables(out, _on_device(shard.local, 5), m, stream, heights, fill=lambda tail: tail.copy_(
        global_events_9(torch.as_tensor(syscall_global_events)).to(tail.device)))
    return out, (count, digest)


def _on_device(records, words):
    """The executor's records (numpy or torch, anywhere) as a contiguous device tensor [n, words], uploaded as they are."""
    t = torch.as_tensor(np.ascontiguousarray(records) if isinstance(records, np.ndarray) else records).reshape(-1, words)
    return (t if t.is_cuda else t.cuda()).contiguous()


def _local_and_global_tables(made, local, extra, stream, heights=None, fill=None, pv=None):
    """What every device builder has in its middle: made["MemoryLocal"] from `local` (device int64 [n, 5]); the caller's `extra`
    events in the tail of MemoryLocal's Global events, written by fill(tail); made["Global"] from all of them; the Global table's
    count and digest, set in the public values `pv` if given. Returns (global events, count, digest). `heights`: None for pad32 of
    each table's rows, or {name: rows} — a table without an entry is not made (core_device_tables_rest)."""
    from .. import api
    n_local = int(local.shape[0])
    count = 2 * n_local + extra
    rows = lambda name, n: RT.pad32(n) if heights is None else int(heights.get(name) or 0)
    gev, digest = None, global_digest(None, 0)
    if heights is None or rows("MemoryLocal", n_local):
        made["MemoryLocal"], gev = api.tracegen_riscv_memory_local(local, rows("MemoryLocal", n_local), extra_global_events=extra, stream=stream)
    if heights is None or rows("Global", count):
        assert gev is not None or not n_local, "the Global table needs the MemoryLocal table's events"
        if gev is None:
            gev = torch.zeros((extra, api.GLOBAL_EVENT_WORDS), dtype=torch.int32, device="cuda")
        if extra:
            fill(gev[2 * n_local:])
        made["Global"] = api.tracegen_riscv_global(gev, rows("Global", count), stream=stream)
        digest = global_digest(made["Global"], count)
    if pv is not None:
        PVM.set_global(pv, count, digest)
    return gev, count, digest


def device_lookup_tables(machine, tables, publics, shard_events, program, pc_base, stream=None):
    """The Byte, Range and Program main tables of a shard counted ON THE DEVICE from the tables that are proved
    (api.LookupCounter): {"Byte", "Range", "Program": api.ColMajor}, word for word what Tracer.byte_range_tables and program_table
    count on the host. `machine`: the shard's [(AirProgram, InteractionProgram)]; `tables`: {name: (main ColMajor, prep ColMajor or
    None)} for every chip of the shard but Byte, Range and Program — device-made or staged, a chip without rows may be left out or
    have main None; `publics`: the shard's public values, canonical words (their sends are eval_public_values'); `shard_events`: the
    executed instructions, an [n, k] int64 matrix whose column 0 is the pc, numpy or a device tensor, or None for a shard that
    executes nothing; `program`: the transpiled instruction list (its length is what counts), `pc_base` its first pc. No host table
    is read."""
    from .. import api
    n_instructions = len(program)
    counter = api.LookupCounter(RT.pad32(n_instructions), stream=stream)
    for a, it in machine:
        if a.name in ("Byte", "Range", "Program"):
            continue
        main, prep = tables.get(a.name, (None, None))
        if main is not None and main.height:
            counter.add(it, main, prep)
    pv = np.asarray(publics.cpu() if torch.is_tensor(publics) else publics, dtype=np.int64)[:PV_WORDS]
    counter.add_row(PVM.program()[1], RT.to_monty_np(torch.as_tensor(pv)))
    if shard_events is not None and len(shard_events):
        counter.add_program_counters(shard_events, pc_base, n_instructions)
    return counter.finish()


def global_events_11(events9):
    """The inverse of global_events_9: [m, 9] int32 -> [m, 11] int64 (message[8], is_send, is_receive, kind), the form
    global_events_balance and the host tracer speak."""
    ev = events9.to(torch.int64)
    recv = ev[:, 8] & 1
    return torch.cat([ev[:, :8], (1 - recv)[:, None], recv[:, None], (ev[:, 8] >> 8)[:, None]], dim=1)


def preprocessed_tables(executor, device="cuda"):
    """{"Byte", "Program", "Range": int64 [rows, width]}: the preprocessed tables of every shard of the executor's program — what a
    proving key is made of, once per run (Tracer.byte_range_tables and program_table make the same three per shard)."""
    dev = torch.device(device)
    pc_base, program = executor.program()
    byte, rng = RT.byte_range_preprocessed(dev)
    return {"Program": RT.program_table(program, pc_base, dev)[0].prep, "Byte": byte, "Range": rng}


def device_core_shard(executor, shard, prep, prev=None, stream=None):
    """A provable core shard from the executor's records alone, every table made ON THE DEVICE: (machine, chips, publics, global
    events) with machine = [(AirProgram, InteractionProgram)] in chip-name order — the shard's whole shape cluster —, chips =
    [(air, it, main ColMajor, prep ColMajor or None)] in the same order, ready for api.ProvingKey.prove_shard, publics = the
    PROOF_MAX_NUM_PVS canonical words, global events = the int32 device tensor [count, 9] the Global table was made from (MemoryLocal's
    two per record, then SyscallCore's). `shard`: an ExecutedShard; `prep`: {"Byte", "Program", "Range": ColMajor}, the program's
    preprocessed tables (preprocessed_tables, made once per run); `prev`: the previous core shard's public values or None.

    The events and `local` are uploaded as they are; api.partition_rv64_events routes and packs them (one 116-byte readback: the 29
    counts are the tables' heights, pad32 of each); the instruction chips, DivRem, AluX0, SyscallInstrs, SyscallCore, StateBump and
    MemoryBump are made from views of the record arena, MemoryLocal from `local`, Global from the events the MemoryLocal and
    SyscallCore kernels write, Byte / Range / Program by device_lookup_tables; the chips of the shape cluster without rows stand at
    height zero. No EventTracer, no host table. MemoryBump's rows stand in the partition's order — by event, then slot A, B, C —
    where the host tracer's stand chip by chip."""
    from .. import api
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        events, local = _on_device(shard.events, EV_WORDS), _on_device(shard.local, 5)
        parts = api.partition_rv64_events(events, stream=stream)
        syscalls = parts.pop("SyscallCore")                  # made behind MemoryLocal: its Global events go into the tail of MemoryLocal's
        made = {name: api.tracegen_riscv_records(name, rec, RT.pad32(int(rec.shape[0])), stream=stream) for name, rec in parts.items() if rec.shape[0]}
        m, pv = int(syscalls.shape[0]), execution_public_values(shard, prev)
        gev, _, _ = _local_and_global_tables(made, local, m, stream, pv=pv, fill=lambda tail: made.update(
            SyscallCore=api.tracegen_riscv_syscall_core(syscalls, RT.pad32(m), global_events=tail, stream=stream)))
        publics = PVM.to_tensor(pv)
        pc_base, program = executor.program()
        machine, chips = _close_device_shard(made, prep, RT.smallest_cluster(set(made) | set(prep)), publics, RT.RunContext(program, pc_base), stream, events)
        return machine, chips, publics, gev


def _close_device_shard(made, prep, cluster, publics, ctx, stream, shard_events=None):
    """What every device builder ends with: the cluster's chips without rows at height zero, the Byte / Range / Program counts
    (device_lookup_tables; `shard_events`: a core shard's executed instructions, None for a shard that executes nothing), the chips
    in name order."""
    from .. import api
    names = sorted(cluster)
    machine = [R.chip(n) for n in names]
    for a, _ in machine:
        if a.name not in made and a.name not in prep:
            assert a.prep_width == 0, a.name
            made[a.name] = api.ColMajor(api.device_words(0), 0, a.main_width)
    made.update(device_lookup_tables(machine, {n: (t, prep.get(n)) for n, t in made.items()}, publics, shard_events, ctx.program, ctx.pc_base, stream=stream))
    return machine, [(a, it, made[a.name], prep.get(a.name)) for a, it in machine]


def _memory_global_records(addrs, recs, previous, which):
    """[n, 3] int64 { addr, value, timestamp } of a memory shard's address list and its (value, timestamp) records, with the host
    filler's two assertions (riscv_more_trace.memory_shard_from): the addresses increase strictly wherever a row is compared, and
    the chain does not end on the uncompared row of address 0."""
    addr = np.asarray(addrs, dtype=np.uint64).reshape(-1)
    n = int(addr.shape[0])
    rec = recs.astype(np.uint64) if isinstance(recs, np.ndarray) else np.array([[int(x) & ((1 << 64) - 1) for x in r] for r in recs], dtype=np.uint64)
    rec = rec.reshape(n, 2)
    if n:
        prev = np.concatenate([np.array([previous], dtype=np.uint64), addr[:-1]])
        comp = (prev != 0) | (np.arange(n) != 0)
        assert bool((addr[comp] > prev[comp]).all()), "addresses must increase strictly"
        assert bool(comp[-1]), "a memory shard whose only %s event is address 0 does not close its chain" % which
    return np.ascontiguousarray(np.concatenate([addr[:, None], rec], axis=1).view(np.int64))


def device_memory_shard(init_addrs, init_recs, fin_addrs, fin_recs, prep, ctx, previous_init=0, previous_fin=0, stream=None):
    """A provable memory shard from the run's address lists alone, every table made ON THE DEVICE: (machine, chips, publics, global
    events) in the shape of device_core_shard — machine = RT.MEMORY_CLUSTER in chip-name order, chips = [(air, it, main ColMajor, prep
    ColMajor or None)], publics = the PROOF_MAX_NUM_PVS canonical words, global events = the int32 device tensor [count, 9] the Global
    table was made from: MemoryGlobalInit's sends, then MemoryGlobalFinalize's receives. The arguments are memory_shard_from's:
    `init_addrs` / `fin_addrs` strictly increasing addresses, `init_recs` / `fin_recs` [n, 2] (value, timestamp) of each, `previous_init` /
    `previous_fin` the previous memory shard's last addresses, `ctx` the run's RunContext (program, final state); `prep`: {"Byte",
    "Program", "Range": ColMajor} (preprocessed_tables).

    The two lists are uploaded as [n, 3] records; api.tracegen_riscv_memory_global makes each chip's table and its Global events (a
    kind without events stands at height zero and its chain stands still), api.tracegen_riscv_global the Global table and — read back,
    14 words — the digest, device_lookup_tables the Byte / Range / Program counts. No Tracer, no host table."""
    from .. import api
    lists = (("MemoryGlobalInit", "init", init_addrs, init_recs, previous_init), ("MemoryGlobalFinalize", "finalize", fin_addrs, fin_recs, previous_fin))
    host = [_memory_global_records(a, r, int(p), which) for _, which, a, r, p in lists]
    pv = PVM.finalized_state(*ctx.final)
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        count = sum(int(h.shape[0]) for h in host)
        gev = torch.empty((count, api.GLOBAL_EVENT_WORDS), dtype=torch.int32, device="cuda")
        made, at = {}, 0
        for (name, which, a_list, _, previous), rec in zip(lists, host):
            n = int(rec.shape[0])
            PVM.put(pv, "previous_%s_addr" % which, PVM.addr_limbs(previous))
            PVM.put(pv, "last_%s_addr" % which, PVM.addr_limbs(int(rec[-1, 0]) if n else previous))
            PVM.put(pv, "global_%s_count" % which, n)
            if n == 0:
                continue
            made[name], ev = api.tracegen_riscv_memory_global(which, torch.from_numpy(rec).cuda(), RT.pad32(n), int(previous), stream=stream)
            gev[at:at + n] = ev
            at += n
        made["Global"] = api.tracegen_riscv_global(gev, RT.pad32(count), stream=stream)
        PVM.set_global(pv, count, global_digest(made["Global"], count))
        publics = PVM.to_tensor(pv)
        machine, chips = _close_device_shard(made, prep, RT.MEMORY_CLUSTER, publics, ctx, stream)
        return machine, chips, publics, gev


DEVICE_PRECOMPILE_KINDS = ("keccak", "secp256k1_add", "secp256k1_double")
DEVICE_SHA_KINDS = ("sha_extend", "sha_compress")             # their descriptors are api.SHA_DESCRIPTORS
DEVICE_WORD_KINDS = ("poseidon2", "uint256")                  # their descriptors are api.WORD_DESCRIPTORS


def _precompile_descriptor(kind):
    """(event words, syscall id, arg2 word, MemoryLocal segments) of a device-made precompile kind, from the table that has it."""
    from .. import api
    for table in (api.PRECOMPILE_DESCRIPTORS, api.SHA_DESCRIPTORS, api.WORD_DESCRIPTORS):
        if kind in table:
            return table[kind]
    raise KeyError("no device descriptor for a %r shard" % (kind,))


def device_precompile_shard(kind, events, prep, ctx, stream=None):
    """A provable precompile shard of `kind` (DEVICE_PRECOMPILE_KINDS, DEVICE_SHA_KINDS, DEVICE_WORD_KINDS) from the executor's event records
    alone ([n, 77 / 43 / 26 / 786 / 155 / 26 / 31] int64, numpy or torch), every table made ON THE DEVICE: (machine, chips, publics, global events) in the shape
    of device_core_shard. The wide tables come from api.tracegen_riscv_keccak / _keccak_control / _secp256k1_add / _double /
    _sha_extend / _sha_extend_control / _sha_compress / _sha_compress_control / _poseidon2 / _uint256_mul; SyscallPrecompile
    (api.tracegen_riscv_syscall_precompile) and the MemoryLocal records of the touched words (api.precompile_local_records, one
    record per word of each call) from the same records by api.PRECOMPILE_DESCRIPTORS[kind], api.SHA_DESCRIPTORS[kind] or api.WORD_DESCRIPTORS[kind]; MemoryLocal and Global as in a core
    shard — MemoryLocal's two events per record first, then SyscallPrecompile's receives —; the public values are the program's
    initial state with the Global fields set. No Tracer, no host table."""
    from .. import api
    words, syscall_id, arg2_word, segments = _precompile_descriptor(kind)
    chip, control, rows_per_call, _ = PRECOMPILES[kind]

    def wide(ev, n):
        made = {chip: api.tracegen_riscv_records(chip, ev, RT.pad32(rows_per_call * n), stream=stream)}
        if control:
            made[control] = api.tracegen_riscv_records(control, ev, RT.pad32(n), stream=stream)
        return made
    return _device_precompile_shard(events, words, wide, syscall_id, arg2_word, segments, prep, ctx, stream)


def _device_precompile_shard(events, words, wide, syscall_id, arg2_word, segments, prep, ctx, stream):
    """The body device_precompile_shard, device_family_shard and device_family_rest_shard share: the events uploaded as they are, the
    kind's wide tables (wide(events, n) -> {chip: ColMajor}), SyscallPrecompile into the tail of MemoryLocal's Global events — one
    `syscall_id` for all rows, or None for each event's own code (api.tracegen_riscv_syscall_precompile_coded) —, MemoryLocal from the
    touched words' records — `segments`: those of api.precompile_local_records, or a callback events -> records —, Global, the public
    values, the counted tables."""
    from .. import api
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        ev = _on_device(events, words)
        n = int(ev.shape[0])
        assert n, "a precompile shard has at least one call"
        made = wide(ev, n)
        if syscall_id is None:
            syscalls = lambda tail: api.tracegen_riscv_syscall_precompile_coded(ev, RT.pad32(n), api.FAMILY_CODE_WORD, arg2_word, global_events=tail, stream=stream)
        else:
            syscalls = lambda tail: api.tracegen_riscv_syscall_precompile(ev, RT.pad32(n), syscall_id, arg2_word, global_events=tail, stream=stream)
        pv = PVM.no_memory_events(PVM.initialized_state(ctx.pc_start))
        records = segments(ev) if callable(segments) else api.precompile_local_records(ev, segments, stream=stream)
        gev, _, _ = _local_and_global_tables(made, records, n, stream, pv=pv,
                                             fill=lambda tail: made.update(SyscallPrecompile=syscalls(tail)))
        publics = PVM.to_tensor(pv)
        machine, chips = _close_device_shard(made, prep, RT.smallest_cluster(set(made) | set(prep)), publics, ctx, stream)
        return machine, chips, publics, gev


DEVICE_KINDS = ("core", "memory") + DEVICE_PRECOMPILE_KINDS + DEVICE_SHA_KINDS
DEVICE_SHARD_KINDS = DEVICE_KINDS + DEVICE_WORD_KINDS        # every kind the executor records


def device_shard(executor, rec, prep, stream=None):
    """One shard of a run (`rec`: a ShardRecords of run_records, its kind one of DEVICE_SHARD_KINDS) made ON THE DEVICE by the builder of
    its kind — device_core_shard, device_memory_shard or device_precompile_shard: (machine, chips, publics, global events [count, 9])."""
    if rec.kind == "core":
        return device_core_shard(executor, rec.executed, prep, prev=rec.prev, stream=stream)
    if rec.kind == "memory":
        return device_memory_shard(rec.init_addrs, rec.init_recs, rec.fin_addrs, rec.fin_recs, prep, rec.ctx, previous_init=rec.previous_init,
                                   previous_fin=rec.previous_fin, stream=stream)
    if rec.kind in DEVICE_SHARD_KINDS:
        return device_precompile_shard(rec.kind, rec.events, prep, rec.ctx, stream=stream)
    raise ValueError("no device builder for a %r shard: device_shard makes %s" % (rec.kind, ", ".join(DEVICE_SHARD_KINDS)))


DEVICE_FAMILY_KINDS = tuple(FAMILIES)[:12]                   # the curve and Fp / Fp2 kinds; their descriptors are api.FAMILY_DESCRIPTORS


def device_family_shard(kind, events, prep, ctx, stream=None):
    """A provable precompile shard of a field / curve `kind` (DEVICE_FAMILY_KINDS) from the executor's family event records alone
    ([n, api.FAMILY_DESCRIPTORS[kind][0]] int64, numpy or torch), every table made ON THE DEVICE: (machine, chips, publics, global
    events) in the shape of device_precompile_shard. The chip's table comes from api.tracegen_riscv_field_chip; an Fp or Fp2AddSub
    shard mixes system calls, so its SyscallPrecompile rows take their ids from the events (the descriptor's syscall id is None)."""
    from .. import api
    if kind not in DEVICE_FAMILY_KINDS:
        raise ValueError("no device builder for a %r shard: device_family_shard makes %s" % (kind, ", ".join(DEVICE_FAMILY_KINDS)))
    words, syscall_id, arg2_word, segments = api.FAMILY_DESCRIPTORS[kind]
    wide = lambda ev, n: {FAMILIES[kind][1]: api.tracegen_riscv_field_chip(kind, ev, RT.pad32(n), stream=stream)}
    return _device_precompile_shard(events, words, wide, syscall_id, arg2_word, segments, prep, ctx, stream)


def device_shard_of(executor, rec, prep, stream=None):
    """device_shard for every kind with a device builder: DEVICE_SHARD_KINDS (device_shard) and DEVICE_FAMILY_KINDS
    (device_family_shard). The last three kinds (ed_add, ed_decompress, uint256_ops) raise ValueError here: device_shard_any, below,
    covers them too."""
    if rec.kind in DEVICE_FAMILY_KINDS:
        return device_family_shard(rec.kind, rec.events, prep, rec.ctx, stream=stream)
    if rec.kind in DEVICE_SHARD_KINDS:
        return device_shard(executor, rec, prep, stream=stream)
    raise ValueError("no device builder for a %r shard: device_shard_of makes %s" % (rec.kind, ", ".join(DEVICE_SHARD_KINDS + DEVICE_FAMILY_KINDS)))


DEVICE_FAMILY_REST_KINDS = ("ed_add", "ed_decompress", "uint256_ops")     # the last three FAMILIES; their descriptors are api.FAMILY_REST_DESCRIPTORS


def device_family_rest_shard(kind, events, prep, ctx, stream=None):
    """A provable precompile shard of `kind` (DEVICE_FAMILY_REST_KINDS) from the executor's family event records alone ([n, 44 / 24 /
    58] int64, numpy or torch), every table made ON THE DEVICE: (machine, chips, publics, global events) in the shape of
    device_precompile_shard. The chip's table comes from api.tracegen_riscv_ed_add / _ed_decompress / _uint256_ops; the touched words'
    records of ed_decompress and uint256_ops from api.precompile_touched_records (ed_add's are two plain segments); a uint256_ops shard
    mixes two system calls, so its SyscallPrecompile rows take their ids from the events."""
    from .. import api
    if kind not in DEVICE_FAMILY_REST_KINDS:
        raise ValueError("no device builder for a %r shard: device_family_rest_shard makes %s" % (kind, ", ".join(DEVICE_FAMILY_REST_KINDS)))
    words, syscall_id, arg2_word, local = api.FAMILY_REST_DESCRIPTORS[kind]
    chip = FAMILIES[kind][1]
    wide = lambda ev, n: {chip: api.tracegen_riscv_records(chip, ev, RT.pad32(n), stream=stream)}
    segments = local if isinstance(local, tuple) else (lambda ev: api.precompile_touched_records(ev, local, stream=stream))
    return _device_precompile_shard(events, words, wide, syscall_id, arg2_word, segments, prep, ctx, stream)


DEVICE_ANY_KINDS = DEVICE_SHARD_KINDS + DEVICE_FAMILY_KINDS + DEVICE_FAMILY_REST_KINDS       # every kind run_records yields


def device_shard_any(executor, rec, prep, stream=None):
    """device_shard for every kind of shard a run can have: DEVICE_SHARD_KINDS (device_shard), DEVICE_FAMILY_KINDS (device_family_shard)
    and DEVICE_FAMILY_REST_KINDS (device_family_rest_shard). Only an unknown kind raises ValueError."""
    if rec.kind in DEVICE_FAMILY_REST_KINDS:
        return device_family_rest_shard(rec.kind, rec.events, prep, rec.ctx, stream=stream)
    if rec.kind in DEVICE_FAMILY_KINDS + DEVICE_SHARD_KINDS:
        return device_shard_of(executor, rec, prep, stream=stream)
    raise ValueError("no device builder for a %r shard: device_shard_any makes %s" % (rec.kind, ", ".join(DEVICE_ANY_KINDS)))


def _constraints_of_row(air, row, publics):
    """The values of an AirProgram's constraints on one main row (canonical integers in and out; no preprocessed columns): the
    public values' own program on the public values, which are a host row to begin with."""
    from ..air import ADD, ASSERT_ZERO, CONST, LOAD_MAIN, MUL, NEG, PUBLIC, SUB
    vals, out = [], []
    for op, a, b in air.instrs:
        v = None
        if op == LOAD_MAIN:
            v = int(row[a])
        elif op == CONST:
            v = a
        elif op == PUBLIC:
            v = int(publics[a])
        elif op == ADD:
            v = (vals[a] + vals[b]) % P
        elif op == SUB:
            v = (vals[a] - vals[b]) % P
        elif op == MUL:
            v = vals[a] * vals[b] % P
        elif op == NEG:
            v = -vals[a] % P
        elif op == ASSERT_ZERO:
            out.append(vals[a])
        else:
            assert op > ASSERT_ZERO, "eval_public_values reads no preprocessed column"
        vals.append(v)
    return out


def check_device_shard(machine, chips, publics, cap=1 << 16, log_buckets=22, stream=None):
    """Every constraint on every row and every bus of one shard, checked where it is made (api.check_constraints,
    api.check_interactions): the reference's debug_constraints_all_chips / debug_interactions_with_all_chips under
    cfg(sp1_debug_constraints). machine, chips, publics: what device_shard_any returns (or a staged shard in the same shape: chips =
    [(air, it, main ColMajor, prep ColMajor or None)], publics = the canonical public values). eval_public_values joins as one more
    chip: its interactions over a one-row device table of the public values, its constraints on that row on the host. Returns
    (failing, imbalance) — failing = [(chip name, the first 8 failing constraint indices)] as machine_check.check_exact would name
    them, imbalance = {(kind, values...): discrepancy mod p}, {} for a balanced shard. Only the rows the findings name are copied to
    the host."""
    from .. import api
    assert [a.name for a, _ in machine] == [c[0].name for c in chips]
    pv = [int(v) for v in (publics.cpu().tolist() if torch.is_tensor(publics) else publics)]
    words = RT.to_monty_np(torch.as_tensor(np.asarray(pv, dtype=np.int64)))
    failing = [(r["name"], [int(k) for k in np.nonzero(r["fail_count"])[0][:8]]) for r in api.check_constraints(chips, words, stream=stream)
               if r["failing_rows"] or r["noncanonical"]]
    pv_air, pv_it = PVM.program()
    bad = [k for k, v in enumerate(_constraints_of_row(pv_air, pv[:PV_WORDS], pv)) if v]
    if bad:
        failing.append((pv_air.name, bad[:8]))
    row = api.ColMajor(api.to_device(words[:pv_it.main_width]), 1, pv_it.main_width)
    buses = api.check_interactions(list(chips) + [(pv_air, pv_it, row, None)], cap=cap, log_buckets=log_buckets, stream=stream)
    imbalance = buses["imbalance"]
    if not buses["balanced"] and not imbalance and not buses["truncated"]:
        # the verdict stands though no record names a culprit: only the second table has a non-zero bucket (pass 2 is keyed on the
        # first), or the discrepancies of the named messages cancel in the exact tally
        imbalance = {"unbalanced_buckets": buses["nonzero_buckets"]}
    if buses["truncated"]:
        imbalance = dict(imbalance, truncated=buses["records_wanted"])
    return failing, imbalance


def execution_public_values(sh, prev=None):
    """An execution shard's `PublicValues` as the tracing executor leaves them (tracing.rs postprocess L548-L562, executor.rs:L60
    finalize_public_values(true)) with the previous shard's state threaded in (`prev`: its words, None for the first shard); the
    Global chip's two fields are set once its table exists (EventTracer.finish)."""
    pv = PVM.set_state(PVM.blank(), sh.pc_start, sh.next_pc, sh.clk_start, sh.clk_end, sh.exit_code, True)
    PVM.put(pv, "committed_value_digest", PVM.digest_bytes(sh.committed_value_digest))
    PVM.put(pv, "deferred_proofs_digest", sh.deferred_proofs_digest)
    PVM.put(pv, "commit_syscall", sh.commit_syscall)
    PVM.put(pv, "commit_deferred_syscall", sh.commit_deferred_syscall)
    if prev is not None:
        for name in ("committed_value_digest", "deferred_proofs_digest", "exit_code", "commit_syscall", "commit_deferred_syscall"):
            PVM.put(pv, "prev_" + name, PVM.get(prev, name))
    return PVM.no_memory_events(pv)


def shard_tables(executor, shard, device="cpu", prev=None):
    """(machine, tables, public values) of one executed shard: machine = [(AirProgram, InteractionProgram)] in chip-name order —
    the shard's whole shape cluster —, tables = {name: (prep, main)} canonical int64 tensors on `device`, public values = the
    PROOF_MAX_NUM_PVS words of its ShardProof (`prev`: the previous shard's words, see EventTracer)."""
    return EventTracer(executor, shard, device, prev=prev).build()


def proof_order(kinds):
    """The order the shards of a run stand in inside a core proof, as indices into `kinds` (what `program_shards` yielded): the
    precompile shards first — they are in the program's INITIAL state (timestamp 1, pc = entry) —, the core shards in execution
    order, then the memory shards in the FINAL state (crates/prover/src/verify.rs:L160-L260 only accepts that chain)."""
    idx = range(len(kinds))
    return [i for i in idx if kinds[i] not in ("core", "memory")] + [i for i in idx if kinds[i] == "core"] + [i for i in idx if kinds[i] == "memory"]


ELEMENT_THRESHOLD, HEIGHT_THRESHOLD = (1 << 28) + (1 << 27), 1 << 22        # core/executor/src/opts.rs:L12-L14
# kind: (chip, control chip | None, rows per event, touched addresses) — air.rs:L473-L480, syscall_code.rs:L439-L479
PRECOMPILES = {"keccak": ("KeccakPermute", "KeccakPermuteControl", 24, 25), "poseidon2": ("Poseidon2", None, 1, 8),
               "sha_extend": ("ShaExtend", "ShaExtendControl", 48, 64), "sha_compress": ("ShaCompress", "ShaCompressControl", 80, 72),
               "uint256": ("Uint256MulMod", None, 1, 12), "secp256k1_add": ("Secp256k1AddAssign", None, 1, 16),
               "secp256k1_double": ("Secp256k1DoubleAssign", None, 1, 8),
               **{k: (FAMILIES[k][1], None, 1, t) for k, t in (("secp256r1_add", 16), ("secp256r1_double", 8), ("bn254_add", 16), ("bn254_double", 8),
                   ("bls12381_add", 24), ("bls12381_double", 12), ("bn254_fp", 8), ("bls12381_fp", 12), ("bn254_fp2_addsub", 16), ("bls12381_fp2_addsub", 24),
                   ("bn254_fp2_mul", 16), ("bls12381_fp2_mul", 24), ("ed_add", 16), ("ed_decompress", 8), ("uint256_ops", 20))}}


class SplitThresholds(Mapping):
    """split_thresholds' result: kind -> events per shard, each entry worked out when it is first asked for. A chip's cost is its
    width, and transcribing every precompile chip to learn it takes seconds, which a run without such calls need not spend; iterating
    (dict(thresholds), ==) works all of them out."""

    def __init__(self, program_rows):
        self.program_rows, self._known = program_rows, {}

    def __getitem__(self, kind):
        if kind not in self._known:
            if kind != "memory" and kind not in PRECOMPILES:
                raise KeyError(kind)
            cost = lambda name: (lambda a: a.main_width + a.prep_width)(R.chip(name)[0])
            trunc = lambda v: v // 32 * 32
            area = ELEMENT_THRESHOLD - (-(-self.program_rows // 32) * 32 * cost("Program") + (1 << 16) * cost("Byte") + (1 << 17) * cost("Range"))
            if kind == "memory":
                self._known[kind] = trunc(min(area // (cost("MemoryGlobalInit") + cost("Global")), HEIGHT_THRESHOLD) // 2)
            else:
                chip_name, control, rows, touched = PRECOMPILES[kind]
                per = rows * cost(chip_name) + (cost(control) if control else 0) + touched * cost("MemoryLocal") + 2 * touched * cost("Global")
                per += cost("SyscallPrecompile") + cost("Global")
                self._known[kind] = min(trunc(area // per), trunc(HEIGHT_THRESHOLD // max(rows, 2 * touched + 1)))
        return self._known[kind]

    def __iter__(self):
        return iter(list(PRECOMPILES) + ["memory"])

    def __len__(self):
        return len(PRECOMPILES) + 1


def split_thresholds(program_rows):
    """`SplitOpts::new` (core/executor/src/opts.rs:L186-L240): how many events of one system call, and how many memory
    initialise / finalise events, go into one shard — the trace area left beside the fixed tables divided by the cost of one event
    (its chip rows, control row, MemoryLocal / Global rows per touched address, SyscallPrecompile row: utils.rs:L117-L154),
    bounded by the height limit, rounded down to 32. A mapping over every kind of PRECOMPILES and "memory" (SplitThresholds)."""
    return SplitThresholds(program_rows)


@dataclasses.dataclass
class ShardRecords:
    """One shard of a run as run_records cuts it: the executor's records of its `kind` and the run's RunContext, no table. A core
    shard has `executed` (the ExecutedShard) and `prev` (the previous core shard's execution_public_values, None for the first); a
    precompile shard `events` (its chunk of the kind's int64 records, as the executor left them); a memory shard the address lists
    and the two chains' previous addresses — the arguments of riscv_more_trace.memory_shard_from and device_memory_shard."""
    kind: str
    ctx: RT.RunContext
    executed: ExecutedShard = None
    prev: list = None
    events: np.ndarray = None
    init_addrs: np.ndarray = None
    init_recs: np.ndarray = None
    fin_addrs: np.ndarray = None
    fin_recs: np.ndarray = None
    previous_init: int = 0
    previous_fin: int = 0


def run_records(executor, max_cycles, core_limit=None):
    """Every shard of a run as a ShardRecords, in the order the reference's controller emits them: the core shards as the program
    executes, then the precompile shards — every kind's calls of the whole run, cut at the `SplitOpts` thresholds (split_thresholds),
    the kinds in the order of PRECOMPILE_KINDS, then FAMILIES —, then the memory shards: MemoryGlobalInit / MemoryGlobalFinalize over
    every address the run touched. `core_limit`: only the first so many core shards are recorded and yielded (the rest of the program
    still runs, so every precompile and memory shard is there). No table is made and no device is touched: host_shard or
    device_shard makes a record's tables."""
    calls, n_core, prev, ctx, shard = {}, 0, None, None, None
    while not executor.halted:
        keep = core_limit is None or n_core < core_limit     # beyond the limit: executed (their precompile calls count), not recorded
        shard = executor.run_shard(max_cycles, record=keep)
        n_core += 1
        if ctx is None:                                      # what the shards without instructions take from the run (RunContext)
            pc_base, program = executor.program()
            ctx = RT.RunContext(program, pc_base, pc_start=shard.pc_start)
        for kind, events in shard.precompile_events().items():
            calls.setdefault(kind, []).append(events)
        if keep:
            yield ShardRecords("core", ctx, executed=shard, prev=prev)
        prev = execution_public_values(shard, prev)
    limit = split_thresholds(executor.program()[1].shape[0])    # (a kind's threshold is worked out when a call of that kind asks for it)
    for kind in PRECOMPILE_KINDS + tuple(FAMILIES):          # one chip per family kind; Fp / UINT256 kinds hold all their system calls' events
        if kind in calls:
            events = np.concatenate(calls[kind])
            for at in range(0, events.shape[0], limit[kind]):
                yield ShardRecords(kind, ctx, events=events[at:at + limit[kind]])
    # ---- the memory shards (prover/src/worker/controller/global.rs:L145-L300). Every touched address — registers with a timestamp,
    # memory words, hinted words — is finalised, and so is every word of the program's memory image, touched or not; every touched
    # address OUTSIDE the image is initialised (registers and fresh memory with 0, hinted words with their hint). The image's own
    # initialisation is the verifying key's `initial_global_cumulative_sum` (image_events / verifying_key_words below). The two
    # streams are merged by address and a shard is flushed when either buffer reaches the threshold: the finalise buffer, which
    # grows at every step, fills first — chunks of `memory` finalise events with the initialise events of their address range.
    gm = executor.global_memory()
    gm = gm[np.argsort(gm[:, 0].astype(np.uint64))]
    if gm.shape[0] == 0 or gm[0, 0] != 0:                  # register x0 opens the address chain whether or not the program read it
        gm = np.concatenate([np.zeros((1, 4), dtype=np.int64), gm])
    img = executor.memory_image()
    t_addr, i_addr = gm[:, 0].astype(np.uint64), img[:, 0].astype(np.uint64)
    outside = ~np.isin(t_addr, i_addr)
    init_addr, init_rec = t_addr[outside], np.stack([gm[outside, 1], np.zeros(int(outside.sum()), dtype=np.int64)], axis=1)
    untouched = ~np.isin(i_addr, t_addr)
    fin_addr = np.concatenate([t_addr, i_addr[untouched]])
    fin_rec = np.concatenate([gm[:, 2:4], np.stack([img[untouched, 1], np.zeros(int(untouched.sum()), dtype=np.int64)], axis=1)])
    order = np.argsort(fin_addr, kind="stable")
    fin_addr, fin_rec = fin_addr[order], fin_rec[order]
    previous_init = previous_fin = 0
    # the memory shards stand in the program's final state (update_finalized_state, worker/prover/core.rs:L370-L397)
    ctx.final = (shard.clk_end, shard.next_pc, shard.exit_code, shard.committed_value_digest, shard.deferred_proofs_digest)
    for at in range(0, fin_addr.shape[0], limit["memory"]):
        fa, fr = fin_addr[at:at + limit["memory"]], fin_rec[at:at + limit["memory"]]
        lo, hi = np.searchsorted(init_addr, fa[0], side="left"), np.searchsorted(init_addr, fa[-1], side="right")
        yield ShardRecords("memory", ctx, init_addrs=init_addr[lo:hi], init_recs=init_rec[lo:hi], fin_addrs=fa, fin_recs=fr,
                           previous_init=previous_init, previous_fin=previous_fin)
        previous_init = int(init_addr[hi - 1]) if hi > lo else previous_init
        previous_fin = int(fa[-1])


def host_shard(executor, rec, device="cpu"):
    """(machine, tables, publics, global events [m, 11]) of one ShardRecords by the host tracer, tables = {name: (prep, main)}
    canonical int64 tensors on `device`: a core shard through EventTracer, every other kind through the builder of its kind in
    riscv_more_trace."""
    from . import riscv_more_trace as MT
    if rec.kind == "core":
        tr = EventTracer(executor, rec.executed, device, prev=rec.prev)
        return (*tr.build(), tr.global_events)
    if rec.kind == "memory":
        return MT.memory_shard_from(rec.init_addrs, rec.init_recs, rec.fin_recs, device, previous_addr=rec.previous_init, ctx=rec.ctx,
                                    fin_addrs=rec.fin_addrs, previous_fin_addr=rec.previous_fin)

    def keccak(events, device, ctx):                         # clk, pointer, 25 x (previous timestamp, word read), 25 words written
        kk = torch.as_tensor(events, device=device)
        rd = kk[:, 2:52].reshape(-1, 25, 2)
        return MT.precompile_shard_from(kk[:, 0], kk[:, 1], rd[:, :, 1].contiguous(), rd[:, :, 0].contiguous(), device, ctx=ctx)

    def poseidon2(events, device, ctx):                      # clk, pointer, 8 x (previous timestamp, word read), 8 words written
        pp = torch.as_tensor(events, device=device)
        rd = pp[:, 2:18].reshape(-1, 8, 2)
        return MT.poseidon2_shard_from(pp[:, 0], pp[:, 1], rd[:, :, 1].contiguous(), rd[:, :, 0].contiguous(), pp[:, 18:26].contiguous(), device, ctx=ctx)
    builders = {"keccak": keccak, "poseidon2": poseidon2, "sha_extend": MT.sha_extend_shard_from, "sha_compress": MT.sha_compress_shard_from,
                "uint256": MT.uint256_shard_from, "secp256k1_add": MT.secp256k1_add_shard_from, "secp256k1_double": MT.secp256k1_double_shard_from,
                **{kind: functools.partial(MT.family_shard_from, kind) for kind in FAMILIES}}
    return builders[rec.kind](rec.events, device, ctx=rec.ctx)


def program_shards(executor, max_cycles, device="cpu", core_limit=None):
    """Every shard of a run traced on the host, in run_records' order: `(kind, machine, tables, publics, global events, ExecutedShard
    or None)` — host_shard of each record; the last slot holds a core shard's ExecutedShard. The global events of all shards cancel
    as a multiset: that is the statement the shards' septic-curve digests add up to. A caller that wants the records themselves, or
    shards made on the device (device_shard), iterates run_records."""
    for rec in run_records(executor, max_cycles, core_limit):
        yield (rec.kind, *host_shard(executor, rec, device), rec.executed)


def image_events(executor, device="cpu"):
    """The Global events the verifying key stands for: one SEND per word of the program's memory image, in the form MemoryGlobalInit
    would have sent it — [0, 0, address limbs, value limbs 0 / 1 with bytes 4 / 5 on top, value limb 3] at timestamp 0
    (`initial_global_cumulative_sum`, core/executor/src/program.rs:L170-L199). [m, 11] like every shard's events: with them
    appended, the events of a whole run cancel."""
    img = executor.memory_image()
    a, v = torch.as_tensor(img[:, 0], device=device), torch.as_tensor(img[:, 1], device=device)
    lim = lambda x, k: (x >> (16 * k)) & 0xFFFF
    cols = [torch.zeros_like(a), torch.zeros_like(a), lim(a, 0), lim(a, 1), lim(a, 2), lim(v, 0) + (((v >> 32) & 0xFF) << 16), lim(v, 1) + (((v >> 40) & 0xFF) << 16),
            lim(v, 3), torch.ones_like(a), torch.zeros_like(a), torch.full_like(a, R.MEMORY)]
    return torch.stack(cols, dim=1)


def verifying_key_words(executor, pc_start, device="cpu"):
    """What the transcript absorbs of the program besides the preprocessed commitment (`MachineVerifyingKey`: pc_start,
    initial_global_cumulative_sum): the entry point's three 16-bit limbs, then the septic digest x[7], y[7] of the memory image's
    initialisation — canonical integers. pc_start: the first shard's (the ELF's entry point)."""
    from . import septic as SE
    ev = image_events(executor, device)
    start = tuple(torch.tensor(v, dtype=torch.int64, device=device) for v in R.CURVE_CUMULATIVE_SUM_START)
    if ev.shape[0]:
        x, y, _, _ = SE.lift_x(ev[:, :8], ev[:, 10], ev[:, 9] == 1)
        cx, cy = SE.prefix_sums(start, x, y)
        digest = [int(t) for t in cx[-1]] + [int(t) for t in cy[-1]]
    else:
        digest = [int(t) for t in start[0]] + [int(t) for t in start[1]]
    return PVM.addr_limbs(pc_start) + digest


def global_events_balance(event_lists):
    """The cross-shard statement: over all shards, every Global message is sent exactly as often as it is received
    (events [n, 11] = message[8], is_send, is_receive, kind). Returns the messages that do not cancel."""
    ev = torch.cat([e.cpu() for e in event_lists]).numpy()
    if ev.shape[0] > (1 << 18):
        # a large run (millions of messages): first two independent 64-bit multiset fingerprints — sum of (send - receive) *
        # mix(message, kind) with wrap-around —, which are both zero when everything cancels; the exact tally below only otherwise
        u = ev.astype(np.uint64)
        sign = (ev[:, 8] - ev[:, 9]).astype(np.uint64)
        clean = True
        for seed in (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F):
            h = np.full(ev.shape[0], seed, dtype=np.uint64)
            for col in list(range(8)) + [10]:
                h = (h ^ u[:, col]) * np.uint64(0x100000001B3 | (seed & 0xFFFF0000))
                h ^= h >> np.uint64(29)
            clean &= int((h * sign).sum(dtype=np.uint64)) == 0
        if clean:
            return []
    tally = {}
    for row in ev:
        key = tuple(int(x) for x in row[:8]) + (int(row[10]),)
        tally[key] = tally.get(key, 0) + int(row[8]) - int(row[9])
    return {k: v for k, v in tally.items() if v}
