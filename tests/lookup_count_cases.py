"""Shared by tests/test_lookup_counts_host.py (CPU) and tests/test_gpu_lookup_counts.py: the inputs of the byte-lookup count
(sp1hip_lookup_count_sends, sp1_amd/csrc/tg_lookup_counts.hpp) and what it must give.

Two kinds of input. The generated shard `riscv_trace.generate({every kind: 3}, K=5, seed=1)`, whose Byte and Range main tables are
the host tracer's count (Tracer.byte_range_tables) of every chip's byte sends and the public values'; and synthetic chips of one
byte send whose six columns ARE the message: [m0, m1, opcode, a, b, c] with multiplicity m0 + m1 — a variable opcode as Bitwise has,
a multiplicity that is a sum of flags as the load chips have. What a synthetic table must give is `model`, plain Python over its
rows, which shares nothing with the code under test."""
import functools
import os
import subprocess

import numpy as np
import torch

from sp1_amd import air
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_trace as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "lookup_counts")
P = 0x7F000001
BYTE_CELLS, RANGE_CELLS, STATUS_WORDS = 6 << 16, 1 << 17, 8
KINDS = ("Add", "Addi", "Sub", "Bitwise", "Lt", "Mul", "ShiftLeft", "ShiftRight", "Addw", "Subw", "UType", "LoadByte", "LoadHalf",
         "LoadWord", "LoadDouble", "StoreByte", "StoreHalf", "StoreWord", "StoreDouble", "Branch", "Jal", "Jalr")
HEIGHTS = (1, 63, 64, 65, 257)                # under a wave, a wave, one lane into the second, one row into the second workgroup
SEND = 1                                      # the byte send's interaction index in `message_chip` (a send of another kind stands first)


class Rejected(Exception):
    """The description was refused before anything was counted."""


def monty(a):
    """canonical integers (any array) -> Montgomery uint32 words."""
    return ((np.asarray(a).astype(np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def col_major(t):
    """canonical [rows, width] (torch int64 or numpy) -> column-major Montgomery words [width][rows]."""
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(monty(a).T)


def run(form, words, main, prep, tmp_path, timeout=120):
    """The native program over one chip: words = the interaction description, main / prep = column-major Montgomery [width][rows]
    (prep None for none). Returns (byte counts [6, 65536], range counts [131072], status [8]); raises Rejected."""
    main = np.ascontiguousarray(main, dtype=np.uint32)
    d, m, p, o = (str(tmp_path / n) for n in ("desc.bin", "main.bin", "prep.bin", "out.bin"))
    np.asarray(words, dtype=np.uint32).tofile(d)
    main.tofile(m)
    prep_width = 0
    if prep is not None:
        prep = np.ascontiguousarray(prep, dtype=np.uint32)
        assert prep.shape[1] == main.shape[1]
        prep.tofile(p)
        prep_width = prep.shape[0]
    r = subprocess.run([EXE, form, d, str(main.shape[0]), str(prep_width), str(main.shape[1]), m, p if prep is not None else "-", o],
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode == 3:
        raise Rejected(r.stderr.strip())
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = np.fromfile(o, dtype=np.uint32)
    assert out.size == BYTE_CELLS + RANGE_CELLS + STATUS_WORDS
    return out[:BYTE_CELLS].reshape(6, 1 << 16), out[BYTE_CELLS:BYTE_CELLS + RANGE_CELLS], out[BYTE_CELLS + RANGE_CELLS:]


# ---- the generated shard
@functools.lru_cache(maxsize=None)
def shard():
    """(machine {name: (air, interactions)}, tables {name: (prep, main)} canonical int64 padded, public values) on the CPU."""
    machine, tabs, publics = RT.generate({k: 3 for k in KINDS}, K=5, seed=1)
    return {a.name: (a, it) for a, it in machine}, tabs, publics


# every chip of the shard with rows, but the two tables that receive the byte messages (test_lookup_counts_host.py checks the list)
SENDERS = ("Add", "Addi", "Addw", "Bitwise", "Branch", "Global", "Jal", "Jalr", "LoadByte", "LoadDouble", "LoadHalf", "LoadWord", "Lt",
           "MemoryLocal", "Mul", "Program", "ShiftLeft", "ShiftRight", "StoreByte", "StoreDouble", "StoreHalf", "StoreWord", "Sub", "Subw",
           "UType")


def public_values_row():
    """(interaction words, the one-row table [160][1]) of the public values' sends."""
    from sp1_amd.machines import public_values as PVM
    _, _, publics = shard()
    return PVM.program()[1], PVM.row(publics)


def torch_tally(it, main, prep):
    """The byte sends of `it` over ALL rows of the canonical tables, tallied with torch: (byte [6, 65536], range [131072], the
    number of messages that are no row of the table they address). The rules are byte_range_tables' assertions as masks: a message
    that breaks one is counted in the third value and in no cell."""
    byte, rng, n_bad = torch.zeros(BYTE_CELLS, dtype=torch.int64), torch.zeros(RANGE_CELLS, dtype=torch.int64), 0
    for mult, vals, _ in RT.eval_interactions(it, main, prep, kinds=(R.BYTE,), sends_only=True):
        opc, a, x, y = (vals[:, i] for i in range(4))
        is_range = opc == R.B_RANGE
        r_ok = is_range & (x <= 16) & (a < (1 << x.clamp(max=16))) & (y == 0)
        xx, yy, o = x.clamp(max=255), y.clamp(max=255), opc.clamp(max=5)
        want = torch.stack([xx & yy, xx | yy, xx ^ yy, torch.zeros_like(xx), (xx < yy).to(torch.int64), xx >> 7], dim=1).gather(1, o[:, None])[:, 0]
        b_ok = ~is_range & (opc < 6) & (x < 256) & (y < 256) & (a == want) & ((opc != R.B_MSB) | (y == 0))
        r_ok, b_ok = r_ok & (mult < (1 << 16)), b_ok & (mult < (1 << 16))
        n_bad += int((~(r_ok | b_ok)).sum())
        rng.index_add_(0, ((1 << x[r_ok]) + a[r_ok]), mult[r_ok])
        byte.index_add_(0, opc[b_ok] * 65536 + x[b_ok] * 256 + y[b_ok], mult[b_ok])
    return byte.reshape(6, 1 << 16).numpy(), rng.numpy(), n_bad


# ---- synthetic chips
def message_chip(prep_columns=False):
    """Width 6: [m0, m1, opcode, a, b, c], one byte send [opcode, a, b, c] with multiplicity m0 + m1, between a send of another
    kind and a byte RECEIVE, both of which a count must pass over. prep_columns: b and c are read from a 2-column preprocessed table."""
    V = air.VCol
    it = air.InteractionProgram("Message", 6, 2 if prep_columns else 0)
    it.send(R.MEMORY, [V.main(3), V.main(4)], V.main(0))
    b, c = (V.prep(0), V.prep(1)) if prep_columns else (V.main(4), V.main(5))
    it.send(R.BYTE, [V.main(2), V.main(3), b, c], V.main(0) + V.main(1))
    it.receive(R.BYTE, [V.main(2), V.main(3), V.main(4), V.main(5)], V.main(1))
    return it


def weighted_chip():
    """Width 3: [flag, x, y], a range check of (x - y) / 8 + 1 to 13 bits with multiplicity 2 flag: constants, weights, an inverse."""
    V = air.VCol
    it = air.InteractionProgram("Weighted", 3)
    inv8 = pow(8, P - 2, P)
    it.send(R.BYTE, [V.const(R.B_RANGE), (V.main(1) + V.main(2) * (P - 1)) * inv8 + 1, V.const(13), V.const(0)], V.main(0) * 2)
    return it


def want_of(opcode, b, c):
    return [b & c, b | c, b ^ c, 0, int(b < c), b >> 7][opcode]


def model(rows):
    """rows of [m0, m1, opcode, a, b, c] canonical -> (byte [6, 65536], range [131072], [(row, reason)] of the bad messages)."""
    byte, rng, bad = np.zeros((6, 1 << 16), np.uint32), np.zeros(RANGE_CELLS, np.uint32), []
    for i, (m0, m1, op, a, b, c) in enumerate(rows):
        m = (m0 + m1) % P
        if m == 0:
            continue
        if m >= 1 << 16:
            bad.append((i, "multiplicity"))
        elif op == 6:
            if b > 16 or a >= 1 << b or c != 0:
                bad.append((i, "range"))
            else:
                rng[(1 << b) + a] += m
        elif op > 5 or b > 255 or c > 255:
            bad.append((i, "operand"))
        elif a != want_of(op, b, c) or (op == 5 and c != 0):
            bad.append((i, "result"))
        else:
            byte[op, b * 256 + c] += m
    return byte, rng, bad


GOOD = (1, 0, 6, 5, 8, 0)                      # range cell 256 + 5


def table_cases(h):
    """{name: rows} at height h: what every synthetic shape test runs."""
    junk = (0, 0, 9, 70000, 300, 300)          # multiplicity 0: anything may stand in a padding row
    return {
        "one_cell": [GOOD] * h,
        "distinct_cells": [(1, 0, 6, i, 16, 0) for i in range(h)],
        "two_flags": [(1, 1, 0, i & 0x0F, i & 0xFF, 0x0F) for i in range(h)],
        "skipped": [junk if i % 3 == 1 else (0, 1, 4, int((i & 0xFF) < 7), i & 0xFF, 7) for i in range(h)],
        # lanes that share a cell with DIFFERENT multiplicities: the combined add is a sum over the group, not m x lanes
        "mixed_multiplicities": [(1, i & 1, 6, 5, 8, 0) if i % 5 else (1, (i >> 1) & 1, 2, 0x0F ^ (i & 3), 0x0F, i & 3) for i in range(h)],
    }


# more rows than one pass of the count kernels' grid holds (2,048 workgroups of 256 rows), and a second pass that ends inside a
# workgroup: the grid stride itself
TALL = 2048 * 256 + 257


def tall_tables():
    """{name: (rows [TALL, 6] int64, want range counts [131072] int64)} — all range checks, built and tallied with numpy: every row
    on one cell; and runs of three rows per cell over all 65,536 16-bit cells with multiplicity 1, 2, 1, 2, ... down the rows, so
    that lanes of one wave share cells with different multiplicities and a wave holds more distinct cells than get combined."""
    i = np.arange(TALL, dtype=np.int64)
    one = np.tile(np.array(GOOD, dtype=np.int64), (TALL, 1))
    want_one = np.zeros(RANGE_CELLS, np.int64)
    want_one[256 + 5] = TALL
    a = (i // 3) & 0xFFFF
    mixed = np.stack([np.ones_like(i), i & 1, np.full_like(i, 6), a, np.full_like(i, 16), np.zeros_like(i)], axis=1)
    want_mixed = np.bincount((1 << 16) + a, weights=1 + (i & 1), minlength=RANGE_CELLS).astype(np.int64)
    return {"one_cell": (one, want_one), "mixed": (mixed, want_mixed)}


def tall_program_counters(n_instructions=1000, pc_base=0x200000):
    """(pcs [TALL] int64, want counts [n_instructions]): runs of five equal pcs (a wave holds 13 distinct ones), over the grid stride."""
    idx = (np.arange(TALL, dtype=np.int64) // 5) % n_instructions
    return pc_base + 4 * idx, np.bincount(idx, minlength=n_instructions).astype(np.int64)


def edge_rows():
    rows = [(1, 0, 6, 0, 0, 0), (1, 0, 6, 65535, 16, 0), (0, 1, 6, 0, 16, 0), (1, 0, 6, 1, 1, 0)]
    for op in range(5):                        # AND, OR, XOR, U8Range, LTU at both corners and across
        for b, c in ((0, 0), (255, 255), (0, 255), (255, 0)):
            rows.append((1, 0, op, want_of(op, b, c), b, c))
    rows += [(1, 0, 5, 0, 0x7F, 0), (1, 0, 5, 1, 0x80, 0), (1, 0, 5, 0, 0, 0), (1, 0, 5, 1, 255, 0)]
    return rows


BAD_ROWS = {                                   # each breaks one rule with multiplicity 1 (the last: with multiplicity p - 1)
    "a_is_2_pow_bits": (1, 0, 6, 256, 8, 0),
    "bits_17": (1, 0, 6, 0, 17, 0),
    "range_c_not_0": (1, 0, 6, 0, 8, 1),
    "operand_256": (1, 0, 0, 0, 256, 0),
    "wrong_and": (1, 0, 0, 2, 3, 5),
    "msb_with_c_1": (1, 0, 5, 1, 0x80, 1),
    "opcode_7": (1, 0, 7, 0, 0, 0),
    "multiplicity_p_minus_1": (P - 1, 0, 6, 5, 8, 0),
}


def bad_table(name, h=65, at=64):
    """h good rows with the bad one at row `at` (the first lane of the second wave)."""
    rows = [(1, 0, 2, (i & 0xFF) ^ 0x55, i & 0xFF, 0x55) for i in range(h)]
    rows[at] = BAD_ROWS[name]
    return rows


def malformed():
    """{name: (words, main width, prep width)} of descriptions that must be refused."""
    good = message_chip().to_array()
    V = air.VCol
    three = air.InteractionProgram("Three", 6)
    three.send(R.BYTE, [V.main(2), V.main(3), V.main(4)], V.main(0))
    prep = message_chip(prep_columns=True).to_array()
    return {"column_at_width": (good, 5, 0), "three_values": (three.to_array(), 6, 0), "truncated": (good[:-1], 6, 0),
            "truncated_in_header": (good[:2], 6, 0), "words_after_the_end": (np.append(good, np.uint32(0)), 6, 0),
            "prep_column_without_prep": (prep, 6, 0), "empty": (good[:0], 6, 0)}
