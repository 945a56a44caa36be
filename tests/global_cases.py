"""Cases for the RISC-V Global chip's trace generation (sp1_amd/csrc/septic.hpp, tracegen_global.hip), shared by
tests/test_tracegen_global_host.py (host form, no GPU) and tests/test_gpu_tracegen_global.py.

ONE event set: `events(n)` is a prefix of 32,800 distinct legal events — first the events whose words sit at the top of their
legal ranges (EDGE_EVENTS), then seeded random ones. Every (n_events, height) case of SIZES is a prefix of it, so the points and
the running sums of a case are prefixes of the full ones and the reference lift (`septic.py`, `Reference`) is computed once.

All messages are distinct. The scan of curve additions assumes that the incomplete addition never meets two points with the same
x; a send and a receive of one message are negatives of each other (same x), and a repeated event is a doubling. With distinct
messages an equal x is a Poseidon2 collision. What the table holds otherwise is not defined by these tests.

What the tests of this entry point reached before these cases (`EARLIER_LARGEST_N_EVENTS`, asserted by
test_tracegen_global_host.py::test_earlier_gpu_tests_stayed_below_every_scan_boundary): a few hundred events, one chunk-sum
workgroup, one finalize workgroup, and the scan's per = 1 regime only."""
import os
import subprocess
import tempfile

import numpy as np

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "septic_ops")
P = 0x7F000001
R1 = (1 << 32) % P
R_INV = pow(1 << 32, -1, P)
G_CHUNK, SCAN_LANES, WORKGROUP = 16, 1024, 256          # tracegen_global.hip: points per lane, lanes of the one scan workgroup
N_FULL = 32800
ROW_COLS, WIDTH = 213, 241                              # non-accumulation columns, all columns

# (n_events, height) -> what it reaches
SIZES = [(0, 16), (0, 4112),                                            # padding only, `events` null; finalize across workgroups without events
         (1, 16), (15, 16), (16, 16), (17, 32), (16, 48),               # chunk edges; a chunk of padding only after the last real one
         (4095, 4096), (4096, 4096), (4097, 4128),                      # chunk-sum and finalize across a 256-lane workgroup
         (16384, 16384), (16385, 16416),                                # n_chunks = 1024: slices of one; 1025: per = 2, live = 513, last slice of one
         (32785, 32800), (32800, 32800)]                                # n_chunks = 2050: per = 3, live = 684, last slice of one


def scan_shape(n_events):
    """(n_chunks, per, live, length of the last slice) of global_scan_totals_kernel for n_events, restated from its code."""
    n_chunks = -(-n_events // G_CHUNK)
    if n_chunks == 0:
        return 0, 0, 0, 0
    per = -(-n_chunks // SCAN_LANES)
    live = -(-n_chunks // per)
    return n_chunks, per, live, n_chunks - (live - 1) * per


# n_events of every call the earlier GPU tests of this entry point make: the (instruction counts, K, seed) of
# tests/test_gpu_tracegen_global.py's two tests and the program tests/riscv_core_row_cases.py executes (the CPU test named above
# regenerates the inputs and asserts these numbers). The largest, 654 events in a 672-row table, is 41 chunks: one lane of the scan
# in ten has a slice, per = 1, and neither the chunk-sum nor the finalize kernel leaves its first workgroup.
EARLIER_GENERATE_CASES = [({"Add": 4, "LoadWord": 6, "StoreWord": 6, "UType": 8, "Ecall": 6}, 2, 17, 86),
                          ({"Add": 40, "Addi": 40, "LoadByte": 60, "LoadDouble": 60, "StoreByte": 60, "StoreDouble": 60, "UType": 30, "Branch": 20}, 3, 17, 654),
                          ({"Add": 4, "Addi": 6, "LoadWord": 6, "StoreWord": 6, "UType": 8, "Branch": 4}, 2, 19, 84)]
EARLIER_EXECUTED_N_EVENTS = 27
EARLIER_LARGEST_N_EVENTS = 654

EDGE_WORDS_1_6 = [0, 1, P - 1, 0x7EFFFFFF]
EDGE_M0 = [0, 1, (1 << 24) - 1]
EDGE_M7 = [0, 0xFFFF]                                   # message[7] + offset 2^16 stays below 2^24
EDGE_KINDS = [0, 1, 126, 127, 128, 255]                 # kind 2^24 reaches p at 127 and passes it


def _edge_events():
    ev, i = [], 0
    for m0 in EDGE_M0:
        for m7 in EDGE_M7:
            for kind in EDGE_KINDS:
                for recv in (1, 0):
                    digits = (i * 57 + 5) % 4096                    # words 1..6 from the pool by the base-4 digits: every message differs
                    mid = [EDGE_WORDS_1_6[(digits >> (2 * k)) & 3] for k in range(6)]
                    ev.append([m0] + mid + [m7, recv | (kind << 8)])
                    i += 1
    for j, w in enumerate(EDGE_WORDS_1_6):                              # all six middle words the same edge word
        ev.append([EDGE_M0[j % 3]] + [w] * 6 + [EDGE_M7[j % 2], (j & 1) | (EDGE_KINDS[j + 2] << 8)])
    return ev


EDGE_EVENTS = _edge_events()
_CACHE = {}


def events(n=N_FULL):
    """[n, 9] uint32: message[8], is_receive | kind << 8."""
    if "all" not in _CACHE:
        rng = np.random.default_rng(20241)
        m = N_FULL - len(EDGE_EVENTS)
        rnd = np.zeros((m, 9), np.int64)
        rnd[:, 0] = rng.integers(0, 1 << 24, m)
        rnd[:, 1:7] = rng.integers(0, P, (m, 6))
        rnd[:, 7] = rng.integers(0, 1 << 16, m)
        rnd[:, 8] = rng.integers(0, 2, m) | (rng.integers(0, 64, m) << 8)
        ev = np.concatenate([np.array(EDGE_EVENTS, np.int64), rnd]).astype(np.uint32)
        assert ev.shape == (N_FULL, 9) and len(np.unique(ev[:, :8], axis=0)) == N_FULL, "messages must be distinct"
        _CACHE["all"] = ev
    return _CACHE["all"][:n]


def split(ev):
    """message [n, 8], is_receive [n], kind [n] as int64."""
    ev = np.asarray(ev, np.int64)
    return ev[:, :8], ev[:, 8] & 0xFF, (ev[:, 8] >> 8) & 0xFF


def from_monty(words):
    return np.asarray(words, np.uint64) * np.uint64(R_INV) % np.uint64(P)


def to_monty(vals):
    return np.asarray(vals, np.uint64) % np.uint64(P) * np.uint64(R1) % np.uint64(P)


# ---- tests/native/septic_ops
(OP_MUL, OP_FROB, OP_NORM_PARTS, OP_INV, OP_FP_SQRT, OP_SQRT, OP_CURVE_RHS, OP_EC_ADD, OP_PICK_ROOT, OP_FROB_TABLE) = range(10)
REC, RES = 32, 16


def run_ops(form, recs, timeout=120):
    """recs: [(op, k, a, b, c, d)] with canonical operands, 7-lists or shorter (zero-extended, trailing ones may be left out).
    Returns (canonical, raw) result words, int64 [n, 16] each: field elements are read from the first, flags from the second."""
    assert os.path.exists(EXE), "tests/native/septic_ops is not built: run __graft_entry__.build()"
    words = np.zeros((len(recs), REC), np.uint64)
    for i, (op, k, *ops) in enumerate(recs):
        words[i, 0], words[i, 1] = op, k
        for j, v in enumerate(ops):
            words[i, 2 + 7 * j:2 + 7 * j + len(v)] = to_monty(v)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.concatenate([np.array([len(recs)], np.uint32), words.astype(np.uint32).reshape(-1)]).tofile(fin)
        r = subprocess.run([EXE, form, "ops", fin, fout], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(fout, dtype="<u4").reshape(len(recs), RES)
    return from_monty(raw).astype(np.int64), raw.astype(np.int64)


def run_rows(form, ev, height, timeout=120):
    """the driver's rows mode: canonical int64 [height, 213] (row-major here)."""
    assert os.path.exists(EXE), "tests/native/septic_ops is not built: run __graft_entry__.build()"
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "ev.bin"), os.path.join(d, "out.bin")
        np.ascontiguousarray(ev, dtype=np.uint32).tofile(fin)
        r = subprocess.run([EXE, form, "rows", fin, str(height), fout], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(fout, dtype="<u4").reshape(ROW_COLS, height)
    assert int(raw.max(initial=0)) < P, "a word is not reduced (or a cell was never written)"
    return from_monty(raw).astype(np.int64).T.copy()


class Reference:
    """The host trace of the full event set on `device`, by sp1_amd/machines/septic.py exactly as riscv_trace.py's
    Tracer.global_chip uses it (lift_x, prefix_sums): lifted ONCE, `table(n, height)` assembles a prefix."""

    def __init__(self, ev, device):
        import torch
        from sp1_amd.machines import riscv as R
        from sp1_amd.machines import septic as SE
        self.torch, self.L, self.dev = torch, R.chip("Global")[0].layout, device
        I64 = torch.int64
        msg, recv, kind = (torch.tensor(a, dtype=I64, device=device) for a in split(ev))
        self.n = msg.shape[0]
        self.start = tuple(torch.tensor(v, dtype=I64, device=device) for v in R.CURVE_CUMULATIVE_SUM_START)
        self.dummy = tuple(torch.tensor(v, dtype=I64, device=device) for v in R.CURVE_WITNESS_DUMMY_POINT)
        rows = torch.zeros((self.n, WIDTH), dtype=I64, device=device)
        L = self.L

        def put(name, val):
            c = L[name]
            if val.dim() == 1:
                rows[:, c] = val
            else:
                rows[:, c:c + val.shape[1]] = val
        if self.n:
            x, y, off, perm = SE.lift_x(msg, kind, recv == 1)
            put("message", msg % P)
            put("kind", kind)
            put("message_0_16bit_limb", msg[:, 0] & 0xFFFF)
            put("message_0_8bit_limb", (msg[:, 0] >> 16) & 0xFF)
            put("interaction.x_coordinate", x)
            put("interaction.y_coordinate", y)
            put("interaction.offset", off)
            rc = torch.where(recv == 1, y[:, 6] - 1, P - y[:, 6] - 1)
            put("interaction.y6_byte_decomp", torch.stack([rc & 0xFF, (rc >> 8) & 0xFF, (rc >> 16) & 0xFF, rc >> 24], dim=1))
            put("is_real", torch.ones_like(recv))
            put("is_receive", recv)
            put("is_send", 1 - recv)
            put("index", torch.arange(self.n, device=device))
            put("interaction.permutation", perm)
            cx, cy = SE.prefix_sums(self.start, x, y)
            put("accumulation.initial_digest_x", torch.cat([self.start[0][None], cx[:-1]]))
            put("accumulation.initial_digest_y", torch.cat([self.start[1][None], cy[:-1]]))
            put("accumulation.cumulative_sum_x", cx)
            put("accumulation.cumulative_sum_y", cy)
        self.rows = rows
        pad = torch.zeros(WIDTH, dtype=I64, device=device)
        pad[L["interaction.x_coordinate"]:L["interaction.x_coordinate"] + 7] = self.dummy[0]
        pad[L["interaction.y_coordinate"]:L["interaction.y_coordinate"] + 7] = self.dummy[1]
        pad[L["interaction.permutation"]:L["interaction.permutation"] + 179] = SE.poseidon2_rows(torch.zeros((1, 16), dtype=I64, device=device))[0]
        sdx, sdy = SE.ec_add((self.start[0][None], self.start[1][None]), (self.dummy[0][None], self.dummy[1][None]))
        for nm, v in (("initial_digest_x", self.start[0]), ("initial_digest_y", self.start[1]), ("cumulative_sum_x", sdx[0]), ("cumulative_sum_y", sdy[0])):
            pad[L["accumulation." + nm]:L["accumulation." + nm] + 7] = v
        self.pad = pad

    def table(self, n, height):
        """canonical int64 [height, 241]: the first n events' rows, then padding rows."""
        assert n <= self.n and n <= height
        return self.torch.cat([self.rows[:n], self.pad[None, :].expand(height - n, WIDTH)])

    def words(self, n, height):
        """the column-major [241, height] Montgomery words the device table must equal, int32"""
        t = self.table(n, height)
        return ((t << 32) % P).to(self.torch.int32).t().contiguous()
