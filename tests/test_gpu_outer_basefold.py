"""GPU checks (-m gpu) of the outer (BN254) BaseFold prover (sp1hip_outer_commit_mles_data / sp1hip_outer_basefold_prove)
against tests/outer_basefold_model.py, the hash-generic Python model whose protocol logic tests/test_outer_basefold_model.py
pins on the C++ oracle: proof bytes and final transcript state equal the model's; at the wrap parameters (94 queries,
22-bit grind, blowup 8) the model's VERIFIER accepts the bytes and rejects flipped ones.

A zero last coordinate of the evaluation point is HANDLED, exactly as sp1hip_basefold_prove handles it: the library's
extension inverse maps 0 to 0, so that round's one_val equals its zero_val (the reference would panic on the division)."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import outer_basefold_model as BM  # noqa: E402
import outer_model as M  # noqa: E402

P = BM.P
REF_WIDTHS = [[16, 10, 14], [20, 78, 34], [10, 10]]           # the reference BaseFold test's three commitment rounds


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _to_monty(a):
    return ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def _from_monty(a):
    rinv = pow(1 << 32, -1, P)
    return (np.asarray(a, dtype=np.uint64) % np.uint64(P) * np.uint64(rinv) % np.uint64(P)).astype(np.uint32)


def _rand_tables(rng, dim, round_widths):
    return [[rng.integers(0, P, (1 << dim, w), dtype=np.uint64).astype(np.uint32) for w in ws] for ws in round_widths]


def _rand_point(rng, dim):
    return rng.integers(0, P, (dim, 4), dtype=np.uint64).astype(np.uint32)


class Instance:
    """Commits canonical `tables` (per round: list of [2^dim][w] arrays) on the GPU and prepares the transcript."""

    def __init__(self, api, tables, point, lb):
        self.api, self.tables, self.point, self.lb = api, tables, np.asarray(point, np.uint32), lb
        self.dim = self.point.shape[0]
        self.prover = api.OuterBasefoldProver()
        self.d_mles = [[api.ColMajor.from_row_major_host(_to_monty(t)) for t in ts] for ts in tables]
        self.rounds, self.commits = [], []
        for ms in self.d_mles:
            commit, pd = self.prover.commit_mles(ms, lb)
            self.rounds.append(pd)
            self.commits.append(commit)
        self.ch = api.OuterChallenger()
        for c in self.commits:
            self.ch.observe_commitment(c)
        flat = [m for ms in self.d_mles for m in ms]
        self.claims_m = api.BasefoldProver().evaluate_mles(flat, _to_monty(self.point))
        self.claims = _from_monty(self.claims_m).tolist()

    def prove(self, nq, pow_bits):
        from sp1_amd._lib import FriConfig
        return self.prover.prove(_to_monty(self.point), self.rounds, self.claims_m, self.ch, FriConfig(self.lb, nq, pow_bits))

    def commits_canonical(self):
        return [M.from_words(c) for c in self.commits]

    def per_round_claims(self):
        out, k = [], 0
        for ts in self.tables:
            w = sum(t.shape[1] for t in ts)
            out.append(self.claims[k:k + w])
            k += w
        return out

    def model_start(self):
        ch = BM.OUTER.challenger()
        for c in self.commits_canonical():
            ch.observe_digest(c)
        return ch


def _check_against_model(api, tables, point, lb, nq, pow_bits):
    inst = Instance(api, tables, point, lb)
    m_rounds = [BM.CommittedRound(BM.OUTER, [t.tolist() for t in ts], lb) for ts in tables]
    assert inst.commits_canonical() == [r.commit for r in m_rounds]
    m_ch = inst.model_start()
    want = BM.basefold_prove(BM.OUTER, point.tolist(), m_rounds, inst.claims, m_ch, lb, nq, pow_bits)
    got = inst.prove(nq, pow_bits)
    assert len(got) == len(want)
    assert got == want, "outer BaseFold proof bytes differ from the model's"
    assert np.array_equal(inst.ch.state(), m_ch.ch.state()), "final transcript state differs from the model's"
    return inst, got


# every dim with every blowup and every round structure: the reference test's first two rounds, all three, a single width-1 mle
CASES = [(dim, lb, ws) for dim in (1, 2, 6, 9) for lb in (1, 2, 3) for ws in (REF_WIDTHS[:2], REF_WIDTHS, [[1]])]


@pytest.mark.parametrize("dim,lb,round_widths", CASES)
def test_proof_bytes_and_final_state_equal_the_model(api, dim, lb, round_widths):
    rng = np.random.default_rng(1000 * dim + 10 * lb + len(round_widths))
    _check_against_model(api, _rand_tables(rng, dim, round_widths), _rand_point(rng, dim), lb, 8, 8)


def test_across_the_tail_switch(api):
    """dim 12, blowup 8: the first fold tree has 2^14 leaves, so the layer kernels and the one-workgroup tail both run."""
    rng = np.random.default_rng(12)
    _check_against_model(api, _rand_tables(rng, 12, [[1]]), _rand_point(rng, 12), 3, 16, 8)


def test_wrap_parameters_verify_and_flips_are_rejected(api):
    dim, lb, nq, pow_bits = 14, 3, 94, 22
    rng = np.random.default_rng(14)
    tables = _rand_tables(rng, dim, [[3], [2, 2]])
    point = _rand_point(rng, dim)
    inst = Instance(api, tables, point, lb)
    blob = inst.prove(nq, pow_bits)
    assert len(blob) == inst.prover.proof_size(dim, inst.rounds, _cfg(lb, nq, pow_bits))

    def verify(b):
        return BM.basefold_verify(BM.OUTER, inst.commits_canonical(), point.tolist(), inst.per_round_claims(), b,
                                  inst.model_start(), lb, nq, pow_bits)

    assert verify(blob) == "ok"
    comp0 = 8 + 32 * dim + 8 + 40 * dim + 8                  # first component opening: u64 count, then its values
    bad = bytearray(blob)
    bad[comp0 + 8] ^= 1                                      # an opened value of query 0
    assert verify(bytes(bad)).split(":")[0] in ("Tcs", "QueryValueMismatch", "Parse")   # (Parse: the flip left the word >= p)
    path0 = comp0 + 8 + 4 * nq * 3 + 24 + 40 + 24            # first path digest of that opening
    bad = bytearray(blob)
    bad[path0 + 8 + 4] ^= 1                                  # a word of the digest (past its length prefix)
    assert verify(bytes(bad)).split(":")[0] in ("Tcs", "Parse")


def _cfg(lb, nq, pow_bits):
    from sp1_amd._lib import FriConfig
    return FriConfig(lb, nq, pow_bits)


@pytest.mark.parametrize("fill", ["zero", "p-1"])
def test_edge_data(api, fill):
    dim, lb = 4, 2
    v = 0 if fill == "zero" else P - 1
    tables = [[np.full((1 << dim, 3), v, np.uint32)], [np.full((1 << dim, 2), v, np.uint32)]]
    _check_against_model(api, tables, _rand_point(np.random.default_rng(5), dim), lb, 8, 8)


def test_zero_last_coordinate_is_handled_as_the_inner_prover_handles_it(api):
    dim, lb = 3, 1
    rng = np.random.default_rng(33)
    tables = _rand_tables(rng, dim, [[2, 1]])
    point = _rand_point(rng, dim)
    point[-1] = 0
    _, blob = _check_against_model(api, tables, point, lb, 8, 8)
    uni0 = struct.unpack_from("<8I", blob, 8)
    assert uni0[:4] == uni0[4:], "round 0: one_val == zero_val when the last coordinate is zero"
    # the inner entry point on the same input: succeeds, and its round 0 message has the same shape
    d = [api.ColMajor.from_row_major_host(_to_monty(t)) for t in tables[0]]
    inner = api.BasefoldProver(lb, 8, 8)
    commit, pd = inner.commit_mles(d)
    ch = api.DuplexChallenger()
    ch.observe(commit)
    claims = inner.evaluate_mles(d, _to_monty(point))
    iblob = inner.prove_trusted_mle_evaluations(_to_monty(point), [pd], claims, ch)
    iuni0 = struct.unpack_from("<8I", iblob, 8)
    assert iuni0[:4] == iuni0[4:]


def test_size_protocol_and_argument_errors(api):
    from sp1_amd import _lib
    lib = _lib.load()
    dim, lb, nq, pow_bits = 5, 2, 8, 8
    rng = np.random.default_rng(77)
    inst = Instance(api, _rand_tables(rng, dim, [[3, 2], [4]]), _rand_point(rng, dim), lb)
    cfg = _cfg(lb, nq, pow_bits)
    size = inst.prover.proof_size(dim, inst.rounds, cfg)
    handles = (C.c_void_p * 2)(*[pd.h for pd in inst.rounds])
    pt, cl = api._ext_array(_to_monty(inst.point)), api._ext_array(inst.claims_m)

    def call(dim_=dim, n_claims=9, cfg_=cfg, buf=None, cap=0, point=pt):
        n = C.c_size_t(cap)
        st = lib.sp1hip_outer_basefold_prove(point, dim_, handles, 2, cl, n_claims, cfg_, inst.ch.h, buf, C.byref(n), None)
        return st, n.value

    before = inst.ch.state()
    short = (C.c_uint8 * (size - 1))()
    assert call(buf=short, cap=size - 1) == (-6, size)
    assert call(buf=None, cap=0) == (-6, size)
    assert np.array_equal(inst.ch.state(), before), "a too-small buffer must leave the challenger untouched"
    big = (C.c_uint8 * (size + 64))()
    bad = -1                                                 # SP1HIP_ERROR_INVALID_ARGUMENT (-6: BUFFER_TOO_SMALL)
    assert call(n_claims=8, buf=big, cap=size + 64)[0] == bad and b"claim" in lib.sp1hip_last_error()
    assert call(cfg_=_cfg(lb + 1, nq, pow_bits), buf=big, cap=size + 64)[0] == bad and b"blowup" in lib.sp1hip_last_error()
    pt4 = api._ext_array(_to_monty(inst.point[:4]))
    assert call(dim_=4, buf=big, cap=size + 64, point=pt4)[0] == bad and b"dimension" in lib.sp1hip_last_error()
    pt22 = api._ext_array(np.zeros((22, 4), np.uint32))
    assert call(dim_=22, cfg_=_cfg(3, nq, pow_bits), buf=big, cap=size + 64, point=pt22)[0] == bad
    assert b"two-adicity" in lib.sp1hip_last_error()
    assert np.array_equal(inst.ch.state(), before)
    st, n = call(buf=big, cap=size + 64)
    assert st == 0 and n == size, "proof_size equals the written length"
    assert not np.array_equal(inst.ch.state(), before)


def test_commit_mles_data_gives_the_commitment_of_outer_commit_mles(api):
    rng = np.random.default_rng(8)
    tables = _rand_tables(rng, 7, [[5, 12, 1]])[0]
    d = [api.ColMajor.from_row_major_host(_to_monty(t)) for t in tables]
    want, _, _ = api.outer_commit_mles(d, 2)
    got, pd = api.OuterBasefoldProver().commit_mles(d, 2)
    assert np.array_equal(got, want) and np.array_equal(pd.commit, want)
