"""GPU parity (-m gpu) of LogUp-GKR on arbitrary tables of the real chips' interaction programs (tests/gkr_real.py): the 30 chips
of the core machine, the precompile chips with 106-value messages and thousands of interactions, the recursion machine's
preprocessed columns. Every chip is paired with its mirror, so the tables balance whatever they hold. For each case the proof
bytes and the final transcript state equal the dense oracle's (an independent algorithm; tests/test_gkr_real_host.py holds it
against the sparse oracle and an integer model), the oracle's verifier accepts the device's proof, and the opened column
evaluations are those of the tables at the proof's point. The oracle's proof of a case is made once and shared by the forms.

What each shape is chosen against is written at gkr_real.CASES and in DESIGN.md §11.0.4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gkr_real as GR  # noqa: E402
import pyoracle as orc  # noqa: E402


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


_device = {}


def _dev(api, name, chips):
    """The case's tables on the device, once; a chip and its mirror share them there too."""
    if name not in _device:
        tables, out = {}, []

        def put(t):
            if t is None or not t.shape[0] or not t.shape[1]:
                return None
            if id(t) not in tables:
                tables[id(t)] = api.ColMajor.from_row_major_host(t)
            return tables[id(t)]
        for prog, main, prep in chips:
            out.append((prog, put(main), put(prep)))
        _device[name] = out
    return _device[name]


_openings = {}


def _opening(name, table, L, point):
    """The columns of a table at the point, from the oracle: once per table and point (a mirror shares its chip's, and every form
    of a case ends at the same point)."""
    key = (name, id(table), point.tobytes())
    if key not in _openings:
        _openings[key] = orc.padded_column_openings(table, L, point)
    return _openings[key]


def _check(api, name):
    chips, L, want, want_state = GR.oracle_proof(name)
    g_ch = GR.seeded(api.DuplexChallenger(), L)
    got = api.logup_gkr(_dev(api, name, chips), L, g_ch)
    same = got == want                       # (not compared inside the assert: no diff of megabytes on a failure)
    assert same, "%s: first difference in %s" % (name, GR.first_difference(got, want))
    assert np.array_equal(g_ch.state(), want_state)
    assert orc.gkr_verify(chips, [c[1].shape[0] for c in chips], L, got, GR.seeded(orc.Challenger(), L)) == 0
    point, opened = api.parse_logup_gkr_proof(got)
    assert point.shape == (L, 4) and [o[0] for o in opened] == [c[0].name for c in chips]
    for (prog, main, prep), (_, o_main, o_prep) in zip(chips, opened):
        assert np.array_equal(o_main, _opening(name, main, L, point)), prog.name
        assert (o_prep is None) == (prep is None)
        if prep is not None:
            assert np.array_equal(o_prep, _opening(name, prep, L, point)), prog.name


@pytest.mark.parametrize("name", ["core-rand", "core-edge"])
def test_the_core_machine(api, name):
    """All 30 chips: 1,138 interactions, heights 0 .. 9 (every quad residue, the vector and the scalar loads of vcol_apply4), 255
    and 256 (a tile less a row, a tile)."""
    _check(api, name)


@pytest.mark.parametrize("name", ["k16", "k17", "k5"])
def test_interaction_counts_around_a_power_of_two(api, name):
    """16 interactions fill 2^4 with no padding interaction, 17 leave 15 padding interactions in 2^5, 5 is odd: the `real_pairs`
    edge of the host's interaction-variable rounds."""
    _check(api, name)


@pytest.mark.parametrize("depth,flat_slots", [("2", None), ("3", None), ("4", None), ("2", "64"), ("3", "64"), ("4", "64"), ("4", "0")])
def test_lane_blocked_levels(api, monkeypatch, depth, flat_slots):
    """Heights 513 .. 4,100: complete 512-entry blocks of a level plus an incomplete one at several levels, 474 interactions wide,
    at every depth of the flat passes, behind tiled passes (64) and with tiled passes only (0)."""
    monkeypatch.setenv("SP1HIP_GKR_LOOKAHEAD", depth)
    if flat_slots is not None:
        monkeypatch.setenv("SP1HIP_GKR_FLAT_SLOTS", flat_slots)
    _check(api, "blocks")


@pytest.mark.parametrize("name", ["wide-edge", "keccak-1030"])
def test_wide_messages(api, name):
    """106 and 105 live values (26 flushes and a tail of 2 or 1), 25 values of 16-term forms, 2,640 opened columns at 6 and at
    1,030 rows."""
    _check(api, name)


@pytest.mark.parametrize("name", ["bls-1", "bls-5", "curves"])
def test_many_interactions_on_few_rows(api, name):
    """3,396 interactions on one row (L = 1: first_layer_kernel and no tree) and on five (L = 3), 5,620 (13 interaction
    variables) on 37 and 130 rows."""
    _check(api, name)


def test_multi_term_and_constant_multiplicities(api):
    _check(api, "mults-edge")


@pytest.mark.parametrize("name", ["recursion-rand", "recursion-edge"])
def test_preprocessed_columns(api, name):
    _check(api, name)


@pytest.mark.parametrize("switch", ["SP1HIP_GKR_FUSED", "SP1HIP_HOST_SIMD"])
@pytest.mark.parametrize("name", ["core-rand", "core-edge", "wide-edge", "keccak-1030"])
def test_the_other_forms(api, monkeypatch, name, switch):
    """The level-by-level tree (first_layer_kernel + transition_kernel) and the scalar host rounds, at 10 and 11 interaction
    variables, on the core machine and on the wide messages."""
    monkeypatch.setenv(switch, "0")
    _check(api, name)
