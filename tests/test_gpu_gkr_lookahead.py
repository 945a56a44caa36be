"""GPU parity (-m gpu) of LogUp-GKR with up to four sumcheck rounds per flat pass (SP1HIP_GKR_LOOKAHEAD = 2 | 3 | 4,
sp1_amd/csrc/gkr_kernels.hpp: gkr_pass_deep): at every depth the proof bytes and the final transcript state equal the oracle's
(which materialises every layer densely, an independent algorithm) and the oracle's verifier accepts the proof. The round
polynomials are exact field elements, so the depth may not move a byte.

Shapes: every residue of a layer's row-variable count mod 3 and mod 4 and layers shorter than one deep pass (L = 1 .. 6); heights
111 / 37 / 37, whose cells are partly padding at every depth; and tables of several complete lane-blocked blocks with
SP1HIP_GKR_FLAT_SLOTS at 64 and 1024, where tiled two-round passes feed the deep flat passes inside one layer and an FV = 3 or 4
fold reads lane-blocked tables. The oracle's proof of a shape is made once and shared by the depths."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import pyoracle as orc  # noqa: E402
from gkr_chips import make_gkr_chips, make_gkr_wide_chips  # noqa: E402
from kb_edges import EdgeSource  # noqa: E402

DEPTHS = ["2", "3", "4"]
SMALL = [(1, 1, False, 2), (2, 2, False, 1), (4, 3, False, 2), (5, 4, True, 3), (3, 5, False, 1), (9, 6, True, 2), (37, 7, True, 3)]
LARGE = [(300, 10, True, 3), (1300, 12, True, 3)]


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _dev(api, chips):
    out = []
    for prog, main, prep in chips:
        d_main = api.ColMajor.from_row_major_host(main) if main.shape[0] else None
        d_prep = api.ColMajor.from_row_major_host(prep) if prep is not None and prep.shape[0] else None
        out.append((prog, d_main, d_prep))
    return out


def _seeded(L):
    o_ch = orc.Challenger()
    o_ch.observe(orc.random_felts((9,), L))
    return o_ch


_oracle = {}


def _case(key, make_chips, L):
    """(chips, oracle proof, oracle transcript state after it): once per shape, never changed."""
    if key not in _oracle:
        chips = make_chips()
        o_ch = _seeded(L)
        want = orc.gkr_prove(chips, L, o_ch)
        _oracle[key] = (chips, want, np.array(o_ch.state()))
    return _oracle[key]


def _check(api, chips, want, want_state, L):
    g_ch = api.DuplexChallenger()
    g_ch.observe(orc.random_felts((9,), L))
    got = api.logup_gkr(_dev(api, chips), L, g_ch)
    assert len(got) == len(want)
    assert got == want
    assert np.array_equal(g_ch.state(), want_state)
    assert orc.gkr_verify(chips, [c[1].shape[0] for c in chips], L, got, _seeded(L)) == 0


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("n_tuples,L,with_empty,dup", SMALL)
def test_every_depth_gives_the_oracles_bytes(api, monkeypatch, n_tuples, L, with_empty, dup, depth):
    monkeypatch.setenv("SP1HIP_GKR_LOOKAHEAD", depth)
    chips, want, state = _case((n_tuples, L, with_empty, dup), lambda: make_gkr_chips(n_tuples, 10 + L, with_empty, dup), L)
    if (n_tuples, L) == (37, 7):
        assert [c[1].shape[0] for c in chips] == [111, 37, 37, 0]
    _check(api, chips, want, state, L)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("flat_slots", ["64", "1024"])
@pytest.mark.parametrize("n_tuples,L,with_empty,dup", LARGE)
def test_tiled_passes_feed_deep_flat_passes(api, monkeypatch, n_tuples, L, with_empty, dup, flat_slots, depth):
    """Several complete lane-blocked blocks per table; the large passes of a layer stay tiled two-round passes and its tail turns
    flat, at a depth of 3 or 4 first behind a two-round fold and then behind its own."""
    monkeypatch.setenv("SP1HIP_GKR_LOOKAHEAD", depth)
    monkeypatch.setenv("SP1HIP_GKR_FLAT_SLOTS", flat_slots)
    chips, want, state = _case((n_tuples, L, with_empty, dup), lambda: make_gkr_chips(n_tuples, 10 + L, with_empty, dup), L)
    _check(api, chips, want, state, L)


@pytest.mark.parametrize("depth", ["3", "4"])
@pytest.mark.parametrize("n_tuples,L,with_empty,dup", LARGE)
def test_deep_folds_read_lane_blocked_tables(api, monkeypatch, n_tuples, L, with_empty, dup, depth):
    """The default flat size: every pass of these shapes is flat, so the deep folds read whole lane-blocked blocks of the level
    (FIRST) and of the folded tables."""
    monkeypatch.setenv("SP1HIP_GKR_LOOKAHEAD", depth)
    chips, want, state = _case((n_tuples, L, with_empty, dup), lambda: make_gkr_chips(n_tuples, 10 + L, with_empty, dup), L)
    _check(api, chips, want, state, L)


def test_edge_valued_tables_at_depth_four(api, monkeypatch):
    """Whole columns of p - 1 or 0x7effffff (tests/kb_edges.py) and two chips with wide interactions, as
    test_gkr_proof_of_edge_tables_matches_oracle, four rounds per pass."""
    monkeypatch.setenv("SP1HIP_GKR_LOOKAHEAD", "4")
    L = 7

    def make():
        src = EdgeSource(700 + L)
        return make_gkr_chips(37, 10 + L, True, 3, source=src) + make_gkr_wide_chips(37, 9, 10 + L, source=src)
    chips, want, state = _case("edge", make, L)
    assert [c[0].name for c in chips] == sorted(c[0].name for c in chips)
    _check(api, chips, want, state, L)


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_chip_of_zero_rows(api, monkeypatch, depth):
    """Omega has an interaction and no rows: no slot in any pass, the padding fraction in every layer's last fold."""
    monkeypatch.setenv("SP1HIP_GKR_LOOKAHEAD", depth)
    L = 6
    chips, want, state = _case("zero", lambda: make_gkr_chips(21, 40, True, 2), L)
    assert chips[-1][0].name == "Omega" and chips[-1][1].shape[0] == 0
    _check(api, chips, want, state, L)
