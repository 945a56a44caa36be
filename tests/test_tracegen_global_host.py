"""The Global chip's row function in its HOST form (sp1_amd/csrc/septic.hpp: global_row, what global_lift_kernel calls for its
lane, compiled for the CPU by tests/native/septic_ops.hip; no GPU is opened), on events whose words sit at the top of their legal
ranges and on random ones (tests/global_cases.py):

* every word of the 213 non-accumulation columns equals riscv_trace.py's Global table, padding rows included;
* every row passes tests/septic_model.py's `lift_check`, the lift rule restated in Python integers (Euler's criterion, roots
  verified by squaring, kb_py's Poseidon2) — a route that shares nothing with septic.py;
* sp1_amd/machines/septic.py, the reference of the GPU tests at sizes the integer model cannot reach, is itself pinned by the
  integer model: smul, sinv, ssqrt, ec_add, prefix_sums;
* the sizes of the GPU cases reach what global_cases.SIZES says of them, and the earlier GPU tests reached none of it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_cases as G  # noqa: E402
import septic_model as M  # noqa: E402

torch = pytest.importorskip("torch")
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402
from sp1_amd.machines import septic as SE  # noqa: E402
from sp1_amd.machines.recursion import P2_EXT, P2_OUT  # noqa: E402

P = M.P
N_MODEL = 280                                       # the integer model's share: at most 300 events
L = R.chip("Global")[0].layout
PERM = L["interaction.permutation"]


def tracer_table(ev):
    """riscv_trace.py's Global table of these events: Tracer.global_chip on a bare object (it uses the device and the table
    dictionary only); int64 [pad32(n), 241]."""
    class Bare:
        dev, tables = "cpu", {}
    msg, recv, kind = G.split(ev)
    ev11 = torch.tensor(np.concatenate([msg, (1 - recv)[:, None], recv[:, None], kind[:, None]], axis=1), dtype=torch.int64)
    bare = Bare()
    bare.tables = {}
    RT.Tracer.global_chip(bare, {}, ev11)
    return bare.tables["Global"].main


@pytest.fixture(scope="module")
def host_rows():
    ev = G.events(N_MODEL)
    want = tracer_table(ev).numpy()
    return ev, G.run_rows("host", ev, want.shape[0]), want


def test_earlier_gpu_tests_stayed_below_every_scan_boundary():
    """The largest n_events the GPU tests of sp1hip_tracegen_riscv_global reached before tests/global_cases.py, regenerated from
    their inputs: 654 events, 41 chunks — the scan at per = 1 with 41 of 1,024 lanes live, one workgroup in every other kernel."""
    is_real = L["is_real"]
    seen = []
    for counts, K, seed, want in G.EARLIER_GENERATE_CASES:
        _, tabs, _ = RT.generate(counts, K=K, seed=seed, device="cpu")
        main = tabs["Global"][1]
        n = int((main[:, is_real] == 1).sum())
        assert n == want
        seen.append((n, main.shape[0]))
    import riscv_core_row_cases as K
    _, _, tr, tabs, _ = K.executed()
    assert tr.global_events.shape[0] == G.EARLIER_EXECUTED_N_EVENTS
    seen.append((tr.global_events.shape[0], tabs["Global"].shape[0]))
    assert max(n for n, _ in seen) == G.EARLIER_LARGEST_N_EVENTS
    for n, height in seen:
        n_chunks, per, live, _ = G.scan_shape(n)
        assert per == 1 and live == n_chunks <= G.WORKGROUP                     # one chunk-sum workgroup, slices of one
        assert -(-height // G.G_CHUNK) <= G.WORKGROUP                           # one finalize workgroup
    assert G.EARLIER_LARGEST_N_EVENTS <= 4096 < 16384


def test_sizes_reach_what_they_claim():
    shape = {n: G.scan_shape(n) for n, _ in G.SIZES}
    assert shape[16384] == (1024, 1, 1024, 1) and shape[16385] == (1025, 2, 513, 1)
    assert shape[32785] == shape[32800] == (2050, 3, 684, 1)
    assert shape[4096][0] == 256 and shape[4097][0] == 257                     # the chunk-sum kernel's second workgroup
    assert -(-4112 // G.G_CHUNK) == 257 and -(-4128 // G.G_CHUNK) == 258       # the finalize kernel's second workgroup
    assert (16, 48) in G.SIZES and 48 // G.G_CHUNK == 3                         # a whole chunk of padding after the last real one
    assert all(n <= h for n, h in G.SIZES) and max(h for _, h in G.SIZES) == G.N_FULL
    ev = G.events()
    msg, recv, kind = G.split(ev)
    assert set(msg[:76, 0]) == set(G.EDGE_M0) and set(msg[:76, 7]) == set(G.EDGE_M7) and set(kind[:76]) == set(G.EDGE_KINDS)
    for w in range(1, 7):
        assert set(msg[:76, w]) == set(G.EDGE_WORDS_1_6)
    assert set(recv[:76]) == {0, 1} and msg[:, 0].max() < 1 << 24 and msg[:, 7].max() < 1 << 16 and msg[:, 1:7].max() < P
    assert ((kind[:76] << 24) >= P).any() and ((kind[:76] << 24) < P).any()


def test_host_rows_equal_the_tracer_table(host_rows):
    ev, got, want = host_rows
    assert want.shape[0] > N_MODEL                                              # padding rows are compared
    bad = np.argwhere(got != want[:, :G.ROW_COLS])
    assert bad.size == 0, ("first mismatch (row, column):", bad[0].tolist(), len(bad))


def test_host_rows_pass_the_integer_lift_rule(host_rows):
    ev, got, _ = host_rows
    msg, recv, kind = G.split(ev)
    xc, yc, oc, bc = L["interaction.x_coordinate"], L["interaction.y_coordinate"], L["interaction.offset"], L["interaction.y6_byte_decomp"]
    offsets = got[:N_MODEL, oc]
    # a root of the right-hand side at every offset below the stored one, from the code under test, verified by the model
    below = [(i, o) for i in range(N_MODEL) for o in range(int(offsets[i]))]
    recs = [(G.OP_SQRT, 0, M.curve_rhs(M.digest_x(msg[i], kind[i], o)[0])) for i, o in below]
    roots = {}
    if recs:
        can, raw = G.run_ops("host", recs)
        for j, (i, o) in enumerate(below):
            if raw[j, 0]:
                roots.setdefault(i, {})[o] = can[j, 1:8].tolist()
    for i in range(N_MODEL):
        row = {"x": got[i, xc:xc + 7].tolist(), "y": got[i, yc:yc + 7].tolist(), "offset": int(offsets[i]), "bytes": got[i, bc:bc + 4].tolist(),
               "perm_in": got[i, PERM + P2_EXT(0, 0):PERM + P2_EXT(0, 0) + 16].tolist(), "perm_out": got[i, PERM + P2_OUT(0):PERM + P2_OUT(0) + 16].tolist()}
        bad = M.lift_check((msg[i].tolist(), bool(recv[i]), int(kind[i])), row, roots.get(i))
        assert not bad, (i, ev[i].tolist(), bad)
        assert got[i, L["is_real"]] == 1 and got[i, L["is_receive"]] == recv[i] and got[i, L["is_send"]] == 1 - recv[i] and got[i, L["index"]] == i
        assert got[i, L["kind"]] == kind[i] and got[i, L["message"]:L["message"] + 8].tolist() == (msg[i] % P).tolist()
        assert got[i, L["message_0_16bit_limb"]] + (got[i, L["message_0_8bit_limb"]] << 16) == msg[i, 0]
    # the cases reach the first six offsets at least (about half of all events take offset 0)
    assert set(range(6)) <= set(offsets.tolist()), sorted(set(offsets.tolist()))


def test_padding_row_is_the_zero_permutation_and_the_dummy_point(host_rows):
    _, got, _ = host_rows
    import kb_py
    for row in got[N_MODEL:]:
        want = np.zeros(G.ROW_COLS, np.int64)
        want[L["interaction.x_coordinate"]:L["interaction.x_coordinate"] + 7] = M.DUMMY[0]
        want[L["interaction.y_coordinate"]:L["interaction.y_coordinate"] + 7] = M.DUMMY[1]
        perm = slice(PERM, PERM + 179)
        assert (np.delete(row, np.r_[perm]) == np.delete(want, np.r_[perm])).all()
        assert not row[PERM + P2_EXT(0, 0):PERM + P2_EXT(0, 0) + 16].any()
        assert row[PERM + P2_OUT(0):PERM + P2_OUT(0) + 16].tolist() == kb_py.permute([0] * 16)
    assert M.on_curve(M.DUMMY) and M.on_curve(M.START)
    assert (list(R.CURVE_WITNESS_DUMMY_POINT[0]), list(R.CURVE_WITNESS_DUMMY_POINT[1])) == M.DUMMY
    assert (list(R.CURVE_CUMULATIVE_SUM_START[0]), list(R.CURVE_CUMULATIVE_SUM_START[1])) == M.START


def test_host_rows_without_events_and_at_height_zero():
    got = G.run_rows("host", G.events(0), 3)
    assert got.shape == (3, G.ROW_COLS) and (got[0] == got[1]).all() and (got[0] == got[2]).all() and got[0, L["is_real"]] == 0
    assert G.run_rows("host", G.events(0), 0).shape == (0, G.ROW_COLS)


def test_septic_py_against_the_integer_model():
    """sp1_amd/machines/septic.py is what the GPU tests compare 32,800 rows with; here 200 elements and points of it are compared
    with Python integers."""
    rng = np.random.default_rng(4242)
    n = 200
    a = rng.integers(0, P, (n, 7))
    b = rng.integers(0, P, (n, 7))
    a[:4] = [[0] * 7, [1] + [0] * 6, [P - 1] * 7, [0, 1, 0, 0, 0, 0, 0]]
    b[:4] = [[P - 1] * 7, [P - 1] * 7, [P - 1] * 7, [0, 0, 0, 0, 0, 0, 1]]
    ta, tb = torch.tensor(a, dtype=torch.int64), torch.tensor(b, dtype=torch.int64)
    assert SE.smul(ta, tb).tolist() == [M.mul(x, y) for x, y in zip(a.tolist(), b.tolist())]
    assert SE.sinv(ta).tolist() == [M.inv(x) for x in a.tolist()]
    for k in (1, 3, 6):
        assert SE.frob(ta[:20], k).tolist() == [M.frob(x, k) for x in a[:20].tolist()]
    sq = np.concatenate([a[:100], np.array([M.mul(x, x) for x in b[:100].tolist()])])
    root, ok = SE.ssqrt(torch.tensor(sq, dtype=torch.int64))
    for x, r, flag in zip(sq.tolist(), root.tolist(), ok.tolist()):
        assert flag == M.is_square(x) and (not flag or M.mul(r, r) == x)
    assert 120 < sum(ok.tolist()) < 190
    assert SE.curve_rhs(ta).tolist() == [M.curve_rhs(x) for x in a.tolist()]
    # points: the lift of the first 200 events; sums by septic.py's scan against one addition after the other in integers
    ev = G.events(n)
    msg, recv, kind = (torch.tensor(v, dtype=torch.int64) for v in G.split(ev))
    x, y, _, _ = SE.lift_x(msg, kind, recv == 1)
    pts = list(zip(x.tolist(), y.tolist()))
    assert all(M.on_curve(p) for p in pts)
    sx, sy = SE.ec_add((x[:-1], y[:-1]), (x[1:], y[1:]))
    assert all(M.sum_holds(pts[i], pts[i + 1], (sx[i].tolist(), sy[i].tolist())) for i in range(n - 1))
    start = tuple(torch.tensor(v, dtype=torch.int64) for v in R.CURVE_CUMULATIVE_SUM_START)
    cx, cy = SE.prefix_sums(start, x, y)
    want = M.sequential_sum(pts)
    assert [(u, v) for u, v in zip(cx.tolist(), cy.tolist())] == want


def test_reference_assembly_equals_the_tracer_table():
    """global_cases.Reference, which lifts once and assembles prefixes for the GPU cases, against Tracer.global_chip, all 241
    columns, at a prefix shorter than what was lifted and with padding rows."""
    ev = G.events(100)
    ref = G.Reference(ev, "cpu")
    for n in (100, 37):
        want = tracer_table(ev[:n])
        assert (ref.table(n, want.shape[0]) == want).all()
    assert (ref.table(0, 32) == ref.pad[None, :]).all()
