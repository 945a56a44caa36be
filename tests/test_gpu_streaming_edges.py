"""Edges (-m gpu) of the kernels that stream the base-field trace tables with 16-byte loads: a lane takes four consecutive rows of
a column, so what can go wrong is a height that is no multiple of four, a column whose base is not 16-byte aligned, a group of
fewer than four columns, a row chunk with a single row. Expected values come from the oracle (pyoracle) or from numpy integers,
never from the library.

Which case reaches which path (sp1_amd/csrc/col_dot.hpp, basefold.hip, gkr_kernels.hpp, jagged_kernels.hpp):

  gkr::open_columns_kernel (sp1hip_logup_gkr_prove, test_trace_openings)
    heights 4, 32, 256, shift 0        every column 16-byte aligned: the 16-byte loads, no tail
    heights 1, 3                       no whole row group: the one-row-per-lane tail alone
    heights 5, 31, 33, 255, 257,       odd columns start off a 16-byte boundary: the workgroups that hold one take the 4-byte
            1023, 1025                 loads; whole row groups and a tail of 1, 2 or 3 rows
    height 16385                       one row above a row chunk (16384): the second chunk is a tail of one row
    widths 1, 3, 5, 63, 65             last column group of 1, 2 or 3 columns; widths 4, 64 whole groups only
    shift 1                            the second chip's tables start one word into an allocation: heights 32 and 256 on the
                                       4-byte loads although they are multiples of four
    Omega                              a chip with zero rows next to chips with rows (its workgroups leave at once)
  eval_columns_partial_kernel, batch_kernel / batch_rows_kernel (sp1hip_mle_eval_columns, sp1hip_basefold_batch, test_eval_and_batch)
    lg 0, 1                            heights 1 and 2: the tail alone; batch_rows_kernel
    lg 2, 3, 5, 8, 10, shift 0         aligned: 16-byte loads; batch_kernel's steps of four columns and its remainder
                                       (total widths 1 + 3 + 4 + 5 + 63 + 64 + 65 = 205 = 51 steps + 1)
    lg 15                              two row chunks
    shift 1, 2, 3                      every tensor starts off a 16-byte boundary: the 4-byte loads, batch_rows_kernel
  the same two and jg_round01_tables (sp1hip_jagged_prove over stacked tables, test_jagged_rounds_0_and_1)
    heights = 0 mod 8, widths 1 .. 65  column slices of 1, 3, 4, 5, 63, 64 and 64 + 1 columns: whole steps of four and remainders of
                                       1, 2, 3; a zero-row table between tables with rows

The table updates of the zerocheck (zc_fix*), gkr::transition2_kernel, jg_fold_tables and jg_foldf_sum are as they were."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import kb_py  # noqa: E402
import pyoracle as orc  # noqa: E402
from kb_edges import EDGE_WORDS, R_INV  # noqa: E402
from sp1_amd.air import InteractionProgram, VCol  # noqa: E402
from test_gpu_jagged import test_jagged_proof_matches_oracle as _jagged_check  # noqa: E402

P = kb_py.P
WIDTHS = (1, 3, 4, 5, 63, 64, 65)


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _table(rng, h, w):
    """Stored-domain words: uniform, with the edge words (0, 1, p - 1, the Montgomery one, the largest 16-bit halves) in every column."""
    t = rng.integers(0, P, (h, w), dtype=np.uint64).astype(np.uint32)
    pool = np.array(EDGE_WORDS, dtype=np.uint32)
    mask = rng.random((h, w)) < 0.25
    t[mask] = pool[rng.integers(0, len(pool), int(mask.sum()))]
    return t


def _col_major_at(api, table, shift):
    """The table column-major on the device, its first word `shift` words into an allocation."""
    cm = api.ColMajor.from_row_major_host(table)
    if not shift:
        return cm
    buf = api.device_words(cm.words.numel() + shift)
    buf[shift:].copy_(cm.words)
    return api.ColMajor(buf[shift:], cm.height, cm.width)


# ------------------------------------------------------------------ gkr::open_columns_kernel

OPEN_CASES = [(1, 1, 0), (3, 3, 0), (4, 4, 0), (5, 5, 0), (31, 63, 0), (32, 64, 0), (33, 65, 0), (255, 1, 0), (256, 3, 0),
              (257, 4, 0), (1023, 5, 0), (1025, 63, 0), (16385, 5, 0), (32, 65, 1), (256, 5, 1)]


@pytest.mark.parametrize("rows,width,shift", OPEN_CASES)
def test_trace_openings(api, rows, width, shift):
    """Alpha sends column 0 of its main trace, Beta (the same table as its preprocessed trace, `shift` words into an allocation)
    receives it, Omega has no rows: proof bytes and transcript equal the dense oracle's, and the opened values are the tables'
    columns at the proof's point."""
    L = max(1, (rows - 1).bit_length())
    rng = np.random.default_rng(1000 * rows + width)
    t = _table(rng, rows, width)
    alpha = InteractionProgram("Alpha", width)
    alpha.send(11, [VCol.main(0)], VCol.const(1))
    beta = InteractionProgram("Beta", 1, prep_width=width)
    beta.receive(11, [VCol.prep(0)], VCol.const(1))
    omega = InteractionProgram("Omega", 2)
    omega.send(9, [VCol.main(0)], VCol.main(1))
    chips = [(alpha, t, None), (beta, np.ascontiguousarray(t[:, :1]), t), (omega, np.zeros((0, 2), np.uint32), None)]
    dev = [(alpha, _col_major_at(api, t, 0), None), (beta, _col_major_at(api, chips[1][1], shift), _col_major_at(api, t, shift)),
           (omega, None, None)]
    o_ch, g_ch = orc.Challenger(), api.DuplexChallenger()
    seed = orc.random_felts((9,), L)
    o_ch.observe(seed)
    g_ch.observe(seed)
    want = orc.gkr_prove(chips, L, o_ch)
    got = api.logup_gkr(dev, L, g_ch)
    assert got == want
    assert np.array_equal(g_ch.state(), o_ch.state())
    point, opened = api.parse_logup_gkr_proof(got)
    col_values = orc.padded_column_openings(t, L, point)
    assert np.array_equal(opened[0][1], col_values)
    assert np.array_equal(opened[1][1], col_values[:1]) and np.array_equal(opened[1][2], col_values)


# ------------------------------------------------------------------ eval_columns_partial_kernel, batch_kernel

def _batch_reference(cols, coeffs):
    """out[r][k] = sum_g coeff[g][k] * col_g[r] * 2^-32 mod p in numpy uint64, every product reduced before it is added."""
    cols = cols.astype(np.uint64)
    out = np.zeros((cols.shape[0], 4), np.uint64)
    for k in range(4):
        out[:, k] = ((cols * coeffs[:, k].astype(np.uint64)[None, :]) % np.uint64(P)).sum(axis=1) % np.uint64(P)
    return (out * np.uint64(R_INV) % np.uint64(P)).astype(np.uint32)


@pytest.mark.parametrize("lg,shift", [(0, 0), (1, 0), (2, 0), (3, 0), (5, 0), (8, 0), (10, 0), (15, 0), (2, 1), (5, 2), (8, 3), (10, 1)])
def test_eval_and_batch(api, lg, shift):
    """Seven tensors of widths 1 .. 65 and height 2^lg, each `shift` words into an allocation: their columns at a random point
    against the oracle's eval_mle, and their random linear combination against numpy integers."""
    rng = np.random.default_rng(77 * lg + shift)
    widths = WIDTHS if lg < 15 else (1, 3, 4, 5)
    tables = [_table(rng, 1 << lg, w) for w in widths]
    d_ts = [_col_major_at(api, t, shift) for t in tables]
    point = orc.random_felts((lg, 4), 5 + lg)
    got = api.BasefoldProver(1, 6, 4).evaluate_mles(d_ts, point)
    want = np.concatenate([orc.eval_mle(t, point) for t in tables])
    assert np.array_equal(got, want)
    tw = sum(widths)
    coeffs = _table(rng, tw, 4)
    out = api.device_words(4 << lg)
    api.check(api._L().sp1hip_basefold_batch(api._tensor_array(d_ts), len(d_ts), lg, api._dptr(api.to_device(coeffs)),
                                             api._dptr(out), api._stream_ptr()))
    assert np.array_equal(api.to_host(out, (4, 1 << lg)).T, _batch_reference(np.concatenate(tables, axis=1), coeffs))


# ------------------------------------------------------------------ jg_round01_tables and the stacked evaluations

def test_jagged_rounds_0_and_1(api, monkeypatch):
    """Every height a multiple of eight: rounds 0 and 1 of the jagged sumcheck come from one pass over the base words
    (jg_round01_tables), a lane walking its table's column slice four columns a step. Proof bytes equal the oracle's."""
    shapes = [[(256, 1), (8, 3), (1032, 4), (0, 2), (24, 5)], [(2048, 63), (512, 64), (264, 65)]]
    _jagged_check(api, monkeypatch, shapes, 11, 10, 8, "1")      # 2^10-row stacked columns, 8 per batch: 23 batches
