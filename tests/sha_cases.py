"""The cases of the SHA-256 trace-generation tests (test_tracegen_sha_host.py on the CPU, test_gpu_tracegen_sha.py on the device):
consistent SHA_EXTEND / SHA_COMPRESS event records written in Python integers — independent of the C++ —, the host builders'
tables of them (riscv_more_trace.sha_extend_shard_from / sha_compress_shard_from, made once and shared), ShaCompress's padding rule
restated for heights beyond the host builder's own, and the native program's runners.

The events. Event 0 is an ordinary call whose clock makes clk_low + 1 + r cross 2^24 inside the call (next_clk.is_overflow is 0 on
its first rows and 1 on the later ones); event 1's pointers stand at the top of the 48-bit range (both upper address limbs 0xFFFF);
event 2's w pointer carries from the first address limb into the second inside the call; SHA_COMPRESS's event 3 stands on the last
instruction slot of a 2^24 window (clk_low = 2^24 - 7: a call's three access times never leave its window, clocks being 1 mod 8).
The w / h words cycle through the edge values 0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFF0000, 0x0000FFFF and random ones; with `upper` (the default) every third word read has
non-zero upper 32 bits — the chips use the low half, the access columns the whole word —, and the words SHA_EXTEND overwrites
always have. The previous timestamp of a word's first access is, by the word's index mod 3, exactly one below the access time
(difference 0), in the same 2^24 window, or in an earlier window.

SHAPES are (calls, height) pairs that cross the 64-lane and 256-lane edges."""
import os
import random
import subprocess

import numpy as np
import torch

from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_more as M
from sp1_amd.machines import riscv_more_trace as MT
from sp1_amd.machines import riscv_trace as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "sha_rows")
KINDS = ("sha_extend", "sha_compress")
CHIPS = {"sha_extend": ("ShaExtend", "ShaExtendControl"), "sha_compress": ("ShaCompress", "ShaCompressControl")}
KIND_OF = {c: k for k, cs in CHIPS.items() for c in cs}
WORDS = {"sha_extend": 786, "sha_compress": 155}
ROWS_PER_CALL = {"ShaExtend": 48, "ShaExtendControl": 1, "ShaCompress": 80, "ShaCompressControl": 1}
SYSCALL = {"sha_extend": (M.SYS_SHA_EXTEND, -1), "sha_compress": (M.SYS_SHA_COMPRESS, 2)}       # (id, arg2 word)
QUAD = 0xFFFFFFFE
# (ptr_word, count, pairs_word, final_word | None | QUAD, final_clk_delta): the segments of the header's comment, restated
SEGMENTS = {"sha_extend": ((1, 64, 530, QUAD, 0),), "sha_compress": ((2, 8, 3, 147, 2), (1, 64, 19, None, 1))}
CONTROL_SHAPES = [(0, 32), (1, 32), (33, 64), (257, 288)]
SHAPES = {"ShaExtend": [(0, 32), (1, 64), (2, 96), (2, 128), (5, 256), (6, 288), (6, 512), (11, 544)],
          "ShaCompress": [(0, 96), (1, 96), (1, 512), (3, 256), (4, 320), (4, 512), (7, 576)],
          "ShaExtendControl": CONTROL_SHAPES, "ShaCompressControl": CONTROL_SHAPES}
CHIP_SHAPES = [(c, n, h) for c in SHAPES for n, h in SHAPES[c]]
SHARD_CALLS = (1, 6)
EDGE = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFF0000, 0x0000FFFF]
M32, M64, WINDOW = 0xFFFFFFFF, (1 << 64) - 1, 1 << 24
TOP = (1 << 48) - 4096


def _rotr(v, r):
    return ((v >> r) | (v << (32 - r))) & M32


def _word(rng, k, upper):
    """Memory word k of a call: its low half an edge value or random, its upper half non-zero on every third word when `upper`."""
    low = EDGE[k % len(EDGE)] if k % 2 == 0 else rng.getrandbits(32)
    return low | ((rng.getrandbits(32) | 1) << 32 if upper and k % 3 == 0 else 0)


def _previous(rng, k, t):
    """A previous timestamp for an access at time t, three ways by k mod 3: t - 1; in t's 2^24 window (unless t opens it); earlier."""
    start = t & ~(WINDOW - 1)
    if k % 3 == 0:
        return t - 1
    if k % 3 == 1 and t - start >= 2:
        return rng.randrange(start, t - 1)
    return ((t >> 24) - 1 - k % 2) * WINDOW + rng.randrange(WINDOW)


def _clk(e):
    """The clock of event e (= 1 mod 8, like every instruction's): event 0 has clk_low + 1 + r reach 2^24 at r = 22."""
    return (6 << 24) - 24 + 1 if e == 0 else (7 << 24) + 1 + 8 * 1000 * e


def _extend_event(rng, e, upper):
    clk = _clk(e)
    w_ptr = {1: TOP, 2: 0x0001_0002_FF00}.get(e, 0x20_0000 + 1024 * rng.randrange(1 << 12))
    mem = [_word(rng, k, upper) for k in range(16)] + [rng.getrandbits(64) for _ in range(48)]          # what the call finds
    initial, last, first = list(mem), [None] * 64, [None] * 64
    steps = []

    def access(k, t):
        if last[k] is None:
            first[k] = last[k] = _previous(rng, k, t)
        prev, last[k] = last[k], t
        return prev

    for r in range(48):
        i, t = 16 + r, clk + 1 + r
        words = []
        for off in (15, 2, 16, 7):
            words += [access(i - off, t), mem[i - off]]
        x, y = mem[i - 15] & M32, mem[i - 2] & M32
        s0 = _rotr(x, 7) ^ _rotr(x, 18) ^ (x >> 3)
        s1 = _rotr(y, 17) ^ _rotr(y, 19) ^ (y >> 10)
        new = ((mem[i - 16] & M32) + s0 + (mem[i - 7] & M32) + s1) & M32
        words += [access(i, t), mem[i], new]
        mem[i] = new
        steps += words
    around = []
    for k in range(64):
        around += [first[k], initial[k], last[k], mem[k]]
    return [clk, w_ptr] + steps + around


def _compress_event(rng, e, upper):
    clk = (8 << 24) - 7 if e == 3 else _clk(e) + 8 * 400
    w_ptr = {1: TOP, 2: 0x0001_0002_FF00}.get(e, 0x40_0000 + 1024 * rng.randrange(1 << 12))
    h_ptr = TOP - 64 if e == 1 else 0x80_0000 + 64 * rng.randrange(1 << 12)
    h = [_word(rng, q + e, upper) for q in range(8)]
    w = [_word(rng, t + 3 * e, upper) for t in range(64)]
    v = [x & M32 for x in h]
    for t in range(64):
        a, b, c, d, e_, f, g, hh = v
        t1 = (hh + (_rotr(e_, 6) ^ _rotr(e_, 11) ^ _rotr(e_, 25)) + ((e_ & f) ^ (~e_ & M32 & g)) + M.SHA_K[t] + (w[t] & M32)) & M32
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        v = [(t1 + t2) & M32, a, b, c, (d + t1) & M32, e_, f, g]
    out = [clk, w_ptr, h_ptr]
    for q in range(8):
        out += [_previous(rng, q, clk), h[q]]
    for t in range(64):
        out += [_previous(rng, t + 1, clk + 1), w[t]]
    return out + [((h[q] & M32) + v[q]) & M32 for q in range(8)]


_EVENTS, _TABLES, _SHARDS = {}, {}, {}


def events(kind, n, upper=True):
    """n consistent event records of `kind`, int64 [n, words]; the first n of any longer list."""
    if (kind, upper) not in _EVENTS or len(_EVENTS[(kind, upper)]) < n:
        rng = random.Random(2024 + KINDS.index(kind))
        make = _extend_event if kind == "sha_extend" else _compress_event
        rows = [make(rng, e, upper) for e in range(max(n, 33))]
        _EVENTS[(kind, upper)] = np.array(rows, dtype=np.uint64).view(np.int64).reshape(len(rows), WORDS[kind])
    return np.ascontiguousarray(_EVENTS[(kind, upper)][:n])


def shard_events(kind, n):
    """The events of the n-call shard the tests build whole (SHARD_CALLS). The one-call shard is also proved, so its words read are
    32-bit as the chips' constraints want them: a proof is of a table whose constraints vanish."""
    return events(kind, n, upper=n != 1)


def _builder(kind):
    return MT.sha_extend_shard_from if kind == "sha_extend" else MT.sha_compress_shard_from


def host_shard(kind, ev, key=None):
    """The host builder's shard of the events: (machine, tables, publics, global events [m, 11]); kept under `key`."""
    if key is None or key not in _SHARDS:
        out = _builder(kind)(ev, "cpu")
        if key is None:
            return out
        _SHARDS[key] = out
    return _SHARDS[key]


def host_chip_tables(kind, n, upper=True):
    """The host builder's two chip tables of events(kind, n) alone, canonical int64 [pad32(rows), width] — the builder runs as it
    is (its own assertions included: w[i] is the extension, the digest is the compression), and what it would hand on to close
    the shard is dropped: a 257-call shard's MemoryLocal and Global tables are not needed to compare two tables."""
    if (kind, n, upper) not in _TABLES:
        seen = {}

        def keep(tr, *args, **kwargs):
            seen.update({name: tr.tables[name].main for name in CHIPS[kind]})
        closing, MT._close_precompile_shard = MT._close_precompile_shard, keep
        try:
            _builder(kind)(events(kind, n, upper), "cpu")
        finally:
            MT._close_precompile_shard = closing
        _TABLES[(kind, n, upper)] = seen
    return _TABLES[(kind, n, upper)]


def compress_padding(first_row, height):
    """ShaCompress's padding rows first_row .. height - 1, restated: octet, octet_num, index and k by row mod 80, all else zero."""
    lay = R.chip("ShaCompress")[0].layout
    out = np.zeros((height - first_row, R.chip("ShaCompress")[0].main_width), dtype=np.int64)
    for i, row in enumerate(range(first_row, height)):
        j = row % 80
        out[i, lay["index"]] = j
        out[i, lay["octet"] + j % 8] = 1
        out[i, lay["octet_num"] + j // 8] = 1
        if 8 <= j < 72:
            out[i, lay["k"]], out[i, lay["k"] + 1] = M.SHA_K[j - 8] & 0xFFFF, M.SHA_K[j - 8] >> 16
    return out


def expected_table(chip, n, height, upper=True):
    """The table of `chip` over events(kind, n) at `height`, canonical int64 [height, width]: the host builder's rows, and behind its
    own height zero rows — for ShaCompress the restated padding."""
    width, live = R.chip(chip)[0].main_width, ROWS_PER_CALL[chip] * n
    assert live <= height
    if n == 0:
        return compress_padding(0, height) if chip == "ShaCompress" else np.zeros((height, width), dtype=np.int64)
    host = host_chip_tables(KIND_OF[chip], n, upper)[chip].numpy()
    assert host.shape == (RT.pad32(live), width)
    if height <= host.shape[0]:
        assert chip != "ShaCompress" or np.array_equal(host[height:], compress_padding(height, host.shape[0]))
        assert chip == "ShaCompress" or not host[height:].any()
        return host[:height]
    tail = compress_padding(host.shape[0], height) if chip == "ShaCompress" else np.zeros((height - host.shape[0], width), dtype=np.int64)
    return np.concatenate([host, tail])


def montgomery_col_major(table):
    """int64 [height, width] canonical -> uint32 numpy [width, height] Montgomery words: what the device and the native program write."""
    return np.ascontiguousarray(RT.to_monty_np(torch.as_tensor(np.ascontiguousarray(table))).T)


def first_difference(chip, want, got, live):
    """None when the two [width, height] word arrays are equal, else a line naming the first column and row that differ."""
    if want.shape != got.shape:
        return "%s: shape %s, want %s" % (chip, got.shape, want.shape)
    bad = np.argwhere(want != got)
    if not len(bad):
        return None
    col, row = (int(v) for v in bad[0])
    lay = R.chip(chip)[0].layout
    key = max((k for k, v in lay.items() if v <= col), key=lambda k: lay[k])
    return "%s: %d words differ, first at column %d (%s), row %d (%s): got %#x, want %#x" % (
        chip, len(bad), col, key, row, "live" if row < live else "padding", int(got[col, row]), int(want[col, row]))


# ----------------------------------------------------------------------------------------------------------- the native program
def _write(tmp_path, tag, array):
    src, dst = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(array, dtype=np.int64).tobytes())
    return src, dst


def run_rows(form, chip, ev, height, tmp_path, timeout=120):
    """tests/native/sha_rows FORM rows: the table as uint32 numpy [width, height]."""
    src, dst = _write(tmp_path, "%s_%d_%d" % (chip, len(ev), height), ev)
    subprocess.run([EXE, form, "rows", chip, src, str(height), dst], check=True, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.uint32).reshape(R.chip(chip)[0].main_width, height)


def run_records(ev, segments, tmp_path, check=True, timeout=120):
    """... host records: the MemoryLocal records of the events as int64 numpy [n * sum of counts, 5]."""
    src, dst = _write(tmp_path, "records_%d_%d" % ev.shape, ev)
    code = lambda f: -1 if f is None else -2 if f == QUAD else f
    segs = ["%d,%d,%d,%d,%d" % (p, c, q, code(f), d) for p, c, q, f, d in segments]
    done = subprocess.run([EXE, "host", "records", src, str(ev.shape[1]), dst] + segs, check=check, capture_output=True, timeout=timeout)
    return np.fromfile(dst, dtype=np.int64).reshape(-1, 5) if done.returncode == 0 else None
