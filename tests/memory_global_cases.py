"""The cases of the MemoryGlobalInit / MemoryGlobalFinalize, SyscallPrecompile and precompile-record tests
(test_tracegen_memglobal_host.py on the CPU, test_gpu_tracegen_memglobal.py on the device): the record lists, the host tracer's
tables and Global events of each — made once and shared —, and the native program's runners.

MemoryGlobal. A `case` is "first" (address 0 with value 0 opens the list and previous = 0: the uncompared row) or "continuing"
(previous = 0x8000 != 0 at index 0). Every list that is long enough holds the neighbours 0x10000 -> 0x10008 (first differ in limb
0), 0x1FFF8 -> 0x20000 (limb 1), 0xFFFFFFF8 -> 0x100000000 (limb 2) and the top address 2^48 - 8; the values cycle through 0, 1,
2^32 - 1, 2^64 - 1, only byte 4, only byte 5 and mixed words; the timestamps through 0, 2^24 - 1, 2^24, 2^24 + 1, 2^40 and others.
SHAPES are the (records, height) pairs at which the read of record i - 1 crosses a wave's and a workgroup's edge. A first shard
of one record does not exist — its only row would be the uncompared one, which cannot close the chain (memory_shard_from asserts
it) —, so ("first", 1) is not a case; (0, 32) is the padding alone and has no host table: every row is zero."""
import os
import subprocess

import numpy as np
import torch

from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_more_trace as MT
from sp1_amd.machines import riscv_trace as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "riscv_memglobal_rows")
KINDS = ("init", "finalize")
CHIP = {"init": "MemoryGlobalInit", "finalize": "MemoryGlobalFinalize"}
CASES = ("first", "continuing")
SHAPES = [(0, 32), (1, 32), (32, 32), (33, 64), (64, 64), (65, 96), (256, 256), (257, 288), (300, 320)]
CASE_SHAPES = [(c, n, h) for c in CASES for n, h in SHAPES if not (c == "first" and n == 1)]
PREVIOUS = {"first": 0, "continuing": 0x8000}
M64 = (1 << 64) - 1
TOP = (1 << 48) - 8
NEIGHBOURS = [0x10000, 0x10008, 0x1FFF8, 0x20000, 0xFFFFFFF8, 0x100000000]
VALUES = [1, (1 << 32) - 1, M64, 0xFF << 32, 0xFF << 40, 0, 0xA1B2_C3D4_E5F6_0718, 0x0001_0000_FFFF_0000, 0x12 << 32, 0x8000_0000_0000_0000]
TIMESTAMPS = [0, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 1 << 40, 9, (5 << 24) + 1001, (1 << 40) + (1 << 24) - 1]


def addresses(case, n):
    """n strictly increasing 8-aligned addresses: the ones every list must hold first, then fillers that fall between no pair of
    neighbours — below 2^32 in steps of 0x1008 (so limbs 0 and 1 both move), above in steps of 2^33 + 8."""
    must = ([0] if case == "first" else []) + [TOP] + NEIGHBOURS
    fill = [0x30000 + 0x1008 * k for k in range(200)] + [0x2_0000_0000 + ((1 << 33) + 8) * k for k in range(200)]
    return sorted((must + fill)[:n])


def records(case, kind, n):
    """(addrs uint64 [n], recs int64 [n, 2] = (value, timestamp)) of a case; Init and Finalize carry other values and timestamps at
    the same addresses. Address 0 holds 0 (register x0)."""
    addrs = np.array(addresses(case, n), dtype=np.uint64)
    shift = 0 if kind == "init" else 3
    value = [0 if int(a) == 0 else VALUES[(i + shift) % len(VALUES)] for i, a in enumerate(addrs)]
    stamp = [TIMESTAMPS[(i + 2 * shift) % len(TIMESTAMPS)] for i in range(n)]
    recs = np.array([value, stamp], dtype=np.uint64).T.reshape(n, 2).view(np.int64)
    return addrs, np.ascontiguousarray(recs)


def records3(case, kind, n):
    """The same as the [n, 3] int64 records { addr, value, timestamp } the kernel and the native program read."""
    addrs, recs = records(case, kind, n)
    return np.ascontiguousarray(np.concatenate([addrs.view(np.int64)[:, None], recs], axis=1))


def reduce_global_events(ev11):
    ev11 = ev11.cpu().numpy().astype(np.int64)
    return np.concatenate([ev11[:, :8], (ev11[:, 9] | (ev11[:, 10] << 8))[:, None]], axis=1).astype(np.int32)


def montgomery_col_major(table):
    """int64 [height, width] canonical -> uint32 numpy [width, height] Montgomery words: what the device and the native program write."""
    return np.ascontiguousarray(RT.to_monty_np(table).T)


_HOST = {}


def host_shard(case, n):
    """memory_shard_from over the case's Init and Finalize lists: (machine, tables, publics, events [2 n, 11]), made once."""
    if (case, n) not in _HOST:
        (ia, ir), (fa, fr) = records(case, "init", n), records(case, "finalize", n)
        _HOST[(case, n)] = MT.memory_shard_from(ia, ir, fr, "cpu", previous_addr=PREVIOUS[case], fin_addrs=fa, previous_fin_addr=PREVIOUS[case])
    return _HOST[(case, n)]


def host_table(case, kind, n, height):
    """(the host filler's table as uint32 [30, height] Montgomery words, its Global events int32 [n, 9])."""
    if n == 0:
        return np.zeros((R.chip(CHIP[kind])[0].main_width, height), dtype=np.uint32), np.zeros((0, 9), dtype=np.int32)
    _, tables, _, gev = host_shard(case, n)
    main = tables[CHIP[kind]][1]
    assert main.shape[0] == height == RT.pad32(n)
    ev = reduce_global_events(gev)
    return montgomery_col_major(main), ev[:n] if kind == "init" else ev[n:]


def first_difference(name, want, got, n):
    """None when the two [width, height] word arrays are equal, else a line naming the first column and row that differ."""
    if want.shape != got.shape:
        return "%s: shape %s, want %s" % (name, got.shape, want.shape)
    bad = np.argwhere(want != got)
    if not len(bad):
        return None
    col, row = (int(v) for v in bad[0])
    key = max((k for k, v in R.chip(name)[0].layout.items() if v <= col), key=lambda k: R.chip(name)[0].layout[k])
    return "%s: %d words differ, first at column %d (%s), row %d (%s): got %#x, want %#x" % (
        name, len(bad), col, key, row, "live" if row < n else "padding", int(got[col, row]), int(want[col, row]))


# ---------------------------------------------------------------------------------------------------------- precompile events
PRECOMPILES = ("keccak", "secp256k1_add", "secp256k1_double")
PRECOMPILE_CHIP_ARGS = {"keccak": (77, 0x09, -1), "secp256k1_add": (43, 0x0A, 2), "secp256k1_double": (26, 0x0B, -1)}
# (ptr_word, count, pairs_word, final_word or None, final_clk_delta): the table of the header's comment, restated
SEGMENTS = {"keccak": ((1, 25, 2, 52, 1),), "secp256k1_add": ((1, 8, 3, 35, 1), (2, 8, 19, None, 0)), "secp256k1_double": ((1, 8, 2, 18, 0),)}
PRECOMPILE_COUNTS = {"keccak": (1, 2, 11), "secp256k1_add": (1, 33), "secp256k1_double": (1, 33)}
_EVENTS, _HOST_PRE = {}, {}


def precompile_events(kind, n):
    """n event records of `kind` as the executor leaves them, int64 [n, words]. Keccak: random states at pointers with a carry into
    the second limb and full upper limbs, clocks next to a 2^24 boundary, the words written computed by the host's permutation;
    secp256k1: multiples of G (tests/secp_cases.py, where the operand set's multiples of G begin)."""
    if (kind, n) in _EVENTS:
        return _EVENTS[(kind, n)]
    if kind == "keccak":
        gen = torch.Generator()
        gen.manual_seed(100 + n)
        clk = (6 << 24) - 8 * 40 + 1 + 8 * 40 * torch.arange(n)                      # the second call stands on the first cycle of a window
        addr = 0x20_0000 + 256 * torch.randperm(4 * n + 4, generator=gen)[:n]
        addr[0] = 0x0001_0002_FFF8                                                    # + 8 i carries into the second limb
        if n > 1:
            addr[1] = 0xFFFF_FFFF_0000                                                # both upper limbs full
        pre = torch.randint(RT.MIN64, (1 << 63) - 1, (n, 25), generator=gen, dtype=torch.int64)
        t_prev = torch.randint(1, (5 << 24) + 900, (n, 25), generator=gen, dtype=torch.int64)
        t_prev[0, 0], t_prev[0, 1] = clk[0] - 1, 1
        post = MT.keccak_round_tensors(pre)[1]
        ev = torch.cat([clk[:, None], addr[:, None], torch.stack([t_prev, pre], dim=2).reshape(n, 50), post], dim=1).numpy()
    else:
        import secp_cases as SC
        short = kind[len("secp256k1_"):]
        ev = SC.events(short, n, start={"add": 111, "double": 110}[short])
    assert ev.shape == (n, PRECOMPILE_CHIP_ARGS[kind][0]) and ev.dtype == np.int64
    _EVENTS[(kind, n)] = np.ascontiguousarray(ev)
    return _EVENTS[(kind, n)]


def host_precompile_shard(kind, n, ctx=None):
    """The host builder's shard of precompile_events(kind, n): (machine, tables, publics, events [2 words + n, 11]); made once for the
    default context."""
    if ctx is not None or (kind, n) not in _HOST_PRE:
        ev = precompile_events(kind, n)
        if kind == "keccak":
            t = torch.as_tensor(ev)
            rd = t[:, 2:52].reshape(-1, 25, 2)
            out = MT.precompile_shard_from(t[:, 0], t[:, 1], rd[:, :, 1].contiguous(), rd[:, :, 0].contiguous(), "cpu", ctx=ctx)
        else:
            out = (MT.secp256k1_add_shard_from if kind == "secp256k1_add" else MT.secp256k1_double_shard_from)(ev, "cpu", ctx=ctx)
        if ctx is not None:
            return out
        _HOST_PRE[(kind, n)] = out
    return _HOST_PRE[(kind, n)]


def local_records_of(table):
    """The [n, 5] int64 records { addr, initial clk, initial value, final clk, final value } a MemoryLocal host table's live rows
    stand for, read back from its columns (canonical values: limbs and clk halves put together again)."""
    lay = R.chip("MemoryLocal")[0].layout
    t = table.numpy().astype(np.uint64)
    limbs = lambda at, k: sum(t[:, at + j] << np.uint64(16 * j) for j in range(k))
    clk = lambda tag: (t[:, lay[tag + "_clk_high"]] << np.uint64(24)) | t[:, lay[tag + "_clk_low"]]
    cols = [limbs(lay["addr"], 3), clk("initial"), limbs(lay["initial_value"], 4), clk("final"), limbs(lay["final_value"], 4)]
    return np.stack(cols, axis=1).view(np.int64)


# ----------------------------------------------------------------------------------------------------------- the native program
def _write(tmp_path, tag, array):
    src, dst = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(array, dtype=np.int64).tobytes())
    return src, dst


def run_rows(chip, rec, height, tmp_path, args, timeout=120):
    """tests/native/riscv_memglobal_rows host rows: the table as uint32 numpy [width, height]. args: (previous_addr,) for the
    MemoryGlobal chips, (words_per_event, syscall_id, arg2_word) for SyscallPrecompile."""
    src, dst = _write(tmp_path, "%s_%d_%d" % (chip, len(rec), height), rec)
    subprocess.run([EXE, "host", "rows", chip, src, str(height), dst] + [str(a) for a in args], check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.uint32).reshape(R.chip(chip)[0].main_width, height)


def run_global(chip, rec, tmp_path, args=(), timeout=120):
    """... host global: the rows' Global events as int32 numpy [n, 9]."""
    src, dst = _write(tmp_path, "global_%s_%d" % (chip, len(rec)), rec)
    subprocess.run([EXE, "host", "global", chip, src, dst] + [str(a) for a in args], check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.int32).reshape(-1, 9)


def run_records(ev, segments, tmp_path, timeout=120):
    """... host records: the MemoryLocal records of the events as int64 numpy [n * sum of counts, 5]."""
    src, dst = _write(tmp_path, "records_%d_%d" % ev.shape, ev)
    segs = ["%d,%d,%d,%d,%d" % (p, c, q, -1 if f is None else f, d) for p, c, q, f, d in segments]
    subprocess.run([EXE, "host", "records", src, str(ev.shape[1]), dst] + segs, check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.int64).reshape(-1, 5)
