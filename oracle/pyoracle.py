"""ctypes binding of the CPU oracle (oracle/_build/liboracle.so) — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
All arrays are numpy uint32 in Montgomery form (R = 2^32) unless a name says canonical.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "liboracle.so")

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in os.listdir(_HERE) if f.endswith((".hpp", ".cpp", ".inc"))]
    stale = (not os.path.exists(_SO)) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", _HERE, "-s"] + (["-B"] if force else []))
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_SO)
        L.orc_two_adic_generator.restype = C.c_uint32
        L.orc_challenger_new.restype = C.c_void_p
        L.orc_challenger_clone.restype = C.c_void_p
        L.orc_challenger_clone.argtypes = [C.c_void_p]
        L.orc_challenger_free.argtypes = [C.c_void_p]
        L.orc_challenger_observe.argtypes = [C.c_void_p, u32p, C.c_size_t]
        L.orc_challenger_sample.argtypes = [C.c_void_p]
        L.orc_challenger_sample.restype = C.c_uint32
        L.orc_challenger_sample_ext.argtypes = [C.c_void_p, u32p]
        L.orc_challenger_sample_bits.argtypes = [C.c_void_p, C.c_int]
        L.orc_challenger_sample_bits.restype = C.c_uint32
        L.orc_challenger_grind.argtypes = [C.c_void_p, C.c_int]
        L.orc_challenger_grind.restype = C.c_uint32
        L.orc_challenger_check_witness.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
        L.orc_challenger_state.argtypes = [C.c_void_p, u32p]
        L.orc_merkle_commit.restype = C.c_void_p
        L.orc_merkle_commit.argtypes = [C.POINTER(u32p), C.POINTER(C.c_int), C.c_int, C.c_size_t, u32p]
        L.orc_merkle_free.argtypes = [C.c_void_p]
        L.orc_merkle_layers.argtypes = [C.c_void_p, u32p]
        L.orc_merkle_root.argtypes = [C.c_void_p, u32p]
        L.orc_merkle_paths.argtypes = [C.c_void_p, u64p, C.c_size_t, u32p]
        L.orc_merkle_verify.argtypes = [u32p, u64p, C.c_size_t, u32p, C.c_size_t, C.c_size_t, u32p, u32p]
        L.orc_commit_mles.restype = C.c_void_p
        L.orc_commit_mles.argtypes = [C.POINTER(u32p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, u32p]
        L.orc_pd_free.argtypes = [C.c_void_p]
        L.orc_pd_codeword.argtypes = [C.c_void_p, C.c_int, u32p]
        L.orc_pd_layers.argtypes = [C.c_void_p, u32p]
        L.orc_basefold_prove.restype = C.c_size_t
        L.orc_basefold_prove.argtypes = [u32p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(u32p),
                                         C.POINTER(C.c_int), u32p, C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t]
        L.orc_basefold_verify.argtypes = [u32p, C.c_int, u32p, C.c_int, u32p, C.POINTER(C.c_int),
                                          C.POINTER(C.c_uint8), C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.orc_interleave.restype = C.c_size_t
        L.orc_interleave.argtypes = [C.POINTER(u32p), u64p, C.POINTER(C.c_int), C.c_int, C.c_size_t, C.c_int,
                                     u32p, C.POINTER(C.c_int)]
        L.orc_jagged_commit_wrap.argtypes = [u32p, u64p, u64p, C.c_int, C.c_uint64, C.c_int, u32p]
        L.orc_jagged_commit.restype = C.c_void_p
        L.orc_jagged_commit.argtypes = [C.POINTER(u32p), u64p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_size_t,
                                        C.c_int, u32p]
        L.orc_jagged_round_free.argtypes = [C.c_void_p]
        L.orc_jagged_prove.restype = C.c_size_t
        L.orc_jagged_prove.argtypes = [u32p, C.c_int, C.c_int, C.POINTER(C.c_void_p), u32p, C.POINTER(C.c_int), C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t]
        L.orc_jagged_verify.argtypes = [u32p, C.c_int, u32p, C.c_int, u32p, C.POINTER(C.c_int), C.POINTER(C.c_uint8),
                                        C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.orc_partial_jagged_table.argtypes = [u64p, C.c_size_t, C.c_int, u32p, u32p, C.c_int, u32p]
        L.orc_full_jagged_eval.argtypes = [u64p, C.c_size_t, u32p, C.c_int, u32p, C.c_int, u32p, C.c_int, u32p]
        cpp = C.POINTER(C.c_char_p)
        L.orc_gkr_prove.restype = C.c_size_t
        L.orc_gkr_prove.argtypes = [C.c_int, cpp, C.POINTER(u32p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(u32p),
                                    C.POINTER(u32p), u64p, C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t]
        L.orc_gkr_verify.argtypes = [C.c_int, cpp, C.POINTER(u32p), C.POINTER(C.c_int), C.POINTER(C.c_int), u64p, C.c_int,
                                     C.POINTER(C.c_uint8), C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        ip = C.POINTER(C.c_int)
        L.orc_shard_prove.restype = C.c_size_t
        L.orc_shard_prove.argtypes = [C.c_int, cpp, C.POINTER(u32p), ip, ip, ip, ip, C.POINTER(u32p), C.POINTER(u32p),
                                      C.POINTER(u32p), u64p, u32p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t]
        L.orc_shard_verify.argtypes = [C.c_int, cpp, C.POINTER(u32p), ip, ip, ip, ip, C.POINTER(u32p), u32p, C.POINTER(C.c_uint8),
                                       C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.orc_gkr_verify_pv.argtypes = L.orc_gkr_verify.argtypes + [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, u32p, C.c_int]
        L.orc_shard_verify_pv.argtypes = L.orc_shard_verify.argtypes + [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int]
        L.orc_stage_seconds.argtypes = [C.POINTER(C.c_double)]
        L.orc_set_gkr_sparse.argtypes = [C.c_int]
        L.orc_set_zc_two_round_form.argtypes = [C.c_int]
        L.orc_set_zc_two_round_form.restype = None
        L.orc_set_threads.argtypes = [C.c_int]
        L.orc_set_threads.restype = None
        _lib = L
    return _lib


def _p(a):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(u32p)


def _arr(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


P = 0x7F000001


def to_monty(x):
    a = _arr(x).copy()
    lib().orc_to_monty(_p(a), C.c_size_t(a.size))
    return a


def from_monty(x):
    a = _arr(x).copy()
    lib().orc_from_monty(_p(a), C.c_size_t(a.size))
    return a


BB_P = 0x78000001


def bb_to_monty(x):
    return ((np.asarray(x, dtype=np.uint64) << np.uint64(32)) % np.uint64(BB_P)).astype(np.uint32)


def bb_from_monty(x):
    return (np.asarray(x, dtype=np.uint64) * np.uint64(pow(1 << 32, -1, BB_P)) % np.uint64(BB_P)).astype(np.uint32)


def bb_random_felts(shape, seed):
    """The documented generator (SplitMix64(seed) -> x mod p) over BabyBear, Montgomery form."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        idx = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(seed) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return bb_to_monty((z % np.uint64(BB_P)).astype(np.uint32)).reshape(shape)


def bb_commit_mles(mles, log_blowup, want_codewords=False, want_tree=False):
    """BabyBear `commit_mles` (RS encode + Poseidon2 Merkle commitment) on the CPU oracle: (commit[8], codewords | None, tree | None)."""
    mles = [_arr(m) for m in mles]
    log_n = mles[0].shape[0].bit_length() - 1
    N = 1 << (log_n + log_blowup)
    widths = (C.c_int * len(mles))(*[m.shape[1] for m in mles])
    commit = np.zeros(8, np.uint32)
    cws = [np.zeros((N, m.shape[1]), np.uint32) for m in mles] if want_codewords else None
    tree = np.zeros((2 * N - 1, 8), np.uint32) if want_tree else None
    L = lib()
    L.orc_bb_commit_mles.restype = None
    L.orc_bb_commit_mles(_ptr_array(mles), widths, len(mles), log_n, log_blowup, _p(commit),
                         _ptr_array(cws) if cws is not None else None, _p(tree) if tree is not None else None)
    return commit, cws, tree


def bb_rs_encode(m, log_blowup):
    """[n][w] row-major -> [n << log_blowup][w], rows bit-reversed (bb_commit.hpp rs_encode)."""
    m = _arr(m)
    log_n = m.shape[0].bit_length() - 1
    out = np.zeros((m.shape[0] << log_blowup, m.shape[1]), np.uint32)
    L = lib()
    L.orc_bb_rs_encode.restype = None
    L.orc_bb_rs_encode(_p(m), log_n, m.shape[1], log_blowup, _p(out))
    return out


def bb_merkle_commit(tensors):
    """Row-major tensors [h][w_k] of any content -> (tree [2 h - 1][8] leaf-first, root [8], commitment [8])."""
    tensors = [_arr(t) for t in tensors]
    h = tensors[0].shape[0]
    widths = (C.c_int * len(tensors))(*[t.shape[1] for t in tensors])
    tree, commit = np.zeros((2 * h - 1, 8), np.uint32), np.zeros(8, np.uint32)
    L = lib()
    L.orc_bb_merkle_commit.restype = None
    L.orc_bb_merkle_commit(_ptr_array(tensors), widths, len(tensors), C.c_size_t(h), _p(tree), _p(commit))
    return tree, tree[-1].copy(), commit


def bb_permute(states):
    s = np.ascontiguousarray(states, dtype=np.uint32).copy()
    L = lib()
    L.orc_bb_permute.restype = None
    L.orc_bb_permute(_p(s), C.c_size_t(s.size // 16))
    return s


def random_felts(shape, seed):
    """SplitMix64(seed) stream reduced mod p, returned in Montgomery form."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        idx = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(seed) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    canon = (z % np.uint64(P)).astype(np.uint32)
    return to_monty(canon).reshape(shape)


def permute(state):
    s = _arr(state).copy()
    lib().orc_permute(_p(s))
    return s


def hash_felts(xs):
    xs = _arr(xs)
    out = np.zeros(8, np.uint32)
    lib().orc_hash(_p(xs) if xs.size else None, C.c_size_t(xs.size), _p(out))
    return out


def compress(l, r):
    out = np.zeros(8, np.uint32)
    lib().orc_compress(_p(_arr(l)), _p(_arr(r)), _p(out))
    return out


def ext_mul(a, b):
    out = np.zeros(4, np.uint32)
    lib().orc_ext_mul(_p(_arr(a)), _p(_arr(b)), _p(out))
    return out


def ext_inv(a):
    out = np.zeros(4, np.uint32)
    lib().orc_ext_inv(_p(_arr(a)), _p(out))
    return out


def rs_encode(mle, log_blowup):
    """mle: [n][w] row-major -> [n << log_blowup][w], rows bit-reversed."""
    mle = _arr(mle)
    n, w = mle.shape
    log_n = n.bit_length() - 1
    assert 1 << log_n == n
    out = np.zeros((n << log_blowup, w), np.uint32)
    lib().orc_rs_encode(_p(mle), log_n, w, log_blowup, _p(out))
    return out


def fold_even_odd(cw, beta):
    cw = _arr(cw)
    N = cw.shape[0]
    out = np.zeros((N // 2, 4), np.uint32)
    lib().orc_fold_even_odd(_p(cw), N.bit_length() - 1, _p(_arr(beta)), _p(out))
    return out


def fold_mle(m, beta):
    m = _arr(m)
    n = m.shape[0]
    out = np.zeros((n // 2, 4), np.uint32)
    lib().orc_fold_mle(_p(m), n.bit_length() - 1, _p(_arr(beta)), _p(out))
    return out


def partial_lagrange(point):
    point = _arr(point).reshape(-1, 4)
    out = np.zeros((1 << point.shape[0], 4), np.uint32)
    lib().orc_partial_lagrange(_p(point), point.shape[0], _p(out))
    return out


def eval_mle(mle, point):
    mle = _arr(mle)
    n, w = mle.shape
    point = _arr(point).reshape(-1, 4)
    assert 1 << point.shape[0] == n
    out = np.zeros((w, 4), np.uint32)
    lib().orc_eval_mle(_p(mle), point.shape[0], w, _p(point), _p(out))
    return out


def _ptr_array(arrs):
    return (u32p * len(arrs))(*[_p(a) for a in arrs])


class MerkleTree:
    def __init__(self, tensors):
        self.tensors = [_arr(t) for t in tensors]
        self.height = self.tensors[0].shape[0]
        widths = (C.c_int * len(tensors))(*[t.shape[1] for t in self.tensors])
        self.commit = np.zeros(8, np.uint32)
        self.h = lib().orc_merkle_commit(_ptr_array(self.tensors), widths, len(tensors),
                                         C.c_size_t(self.height), _p(self.commit))
        self.log_height = self.height.bit_length() - 1

    def layers(self):
        out = np.zeros((2 * self.height - 1, 8), np.uint32)
        lib().orc_merkle_layers(self.h, _p(out))
        return out

    def root(self):
        out = np.zeros(8, np.uint32)
        lib().orc_merkle_root(self.h, _p(out))
        return out

    def paths(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.zeros((len(idx), self.log_height, 8), np.uint32)
        lib().orc_merkle_paths(self.h, idx.ctypes.data_as(u64p), C.c_size_t(len(idx)), _p(out))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_merkle_free(self.h)
            self.h = None


def merkle_verify(commit, idx, values, log_height, root, paths):
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    values = _arr(values)
    return lib().orc_merkle_verify(_p(_arr(commit)), idx.ctypes.data_as(u64p), C.c_size_t(len(idx)), _p(values),
                                   C.c_size_t(values.shape[1]), C.c_size_t(log_height), _p(_arr(root)),
                                   _p(_arr(paths)))


class Challenger:
    def __init__(self, h=None):
        self.h = h if h is not None else lib().orc_challenger_new()

    def clone(self):
        return Challenger(lib().orc_challenger_clone(self.h))

    def observe(self, xs):
        xs = _arr(xs).reshape(-1)
        lib().orc_challenger_observe(self.h, _p(xs), C.c_size_t(xs.size))

    def sample(self):
        return lib().orc_challenger_sample(self.h)

    def sample_ext(self):
        out = np.zeros(4, np.uint32)
        lib().orc_challenger_sample_ext(self.h, _p(out))
        return out

    def sample_point(self, n):
        return np.stack([self.sample_ext() for _ in range(n)]) if n else np.zeros((0, 4), np.uint32)

    def sample_bits(self, bits):
        return lib().orc_challenger_sample_bits(self.h, bits)

    def grind(self, bits):
        return lib().orc_challenger_grind(self.h, bits)

    def check_witness(self, bits, w):
        return bool(lib().orc_challenger_check_witness(self.h, bits, C.c_uint32(int(w))))

    def state(self):
        out = np.zeros(34, np.uint32)
        lib().orc_challenger_state(self.h, _p(out))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_challenger_free(self.h)
            self.h = None


class CommittedRound:
    """BasefoldProver::commit_mles on the CPU oracle for one commitment round."""

    def __init__(self, mles, log_blowup):
        self.mles = [_arr(m) for m in mles]
        n = self.mles[0].shape[0]
        self.log_n = n.bit_length() - 1
        self.log_blowup = log_blowup
        widths = (C.c_int * len(mles))(*[m.shape[1] for m in self.mles])
        self.commit = np.zeros(8, np.uint32)
        self.h = lib().orc_commit_mles(_ptr_array(self.mles), widths, len(mles), self.log_n, log_blowup,
                                       _p(self.commit))

    def codeword(self, k):
        out = np.zeros((1 << (self.log_n + self.log_blowup), self.mles[k].shape[1]), np.uint32)
        lib().orc_pd_codeword(self.h, k, _p(out))
        return out

    def layers(self):
        N = 1 << (self.log_n + self.log_blowup)
        out = np.zeros((2 * N - 1, 8), np.uint32)
        lib().orc_pd_layers(self.h, _p(out))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_pd_free(self.h)
            self.h = None


def basefold_prove(point, rounds, claims, challenger, log_blowup=2, num_queries=124, pow_bits=16):
    """rounds: list[CommittedRound]; claims: list (per round) of list (per mle) of [w][4] arrays."""
    point = _arr(point).reshape(-1, 4)
    mles, widths, per_round = [], [], []
    for r in rounds:
        per_round.append(len(r.mles))
        for m in r.mles:
            mles.append(m)
            widths.append(m.shape[1])
    flat_claims = _arr(np.concatenate([np.asarray(c, np.uint32).reshape(-1, 4) for rc in claims for c in rc]))
    pds = (C.c_void_p * len(rounds))(*[r.h for r in rounds])
    args = (_p(point), point.shape[0], len(rounds), (C.c_int * len(rounds))(*per_round), _ptr_array(mles),
            (C.c_int * len(widths))(*widths), _p(flat_claims), pds, log_blowup, num_queries, pow_bits)
    probe = challenger.clone()
    size = lib().orc_basefold_prove(*args, probe.h, None, C.c_size_t(0))
    buf = (C.c_uint8 * size)()
    got = lib().orc_basefold_prove(*args, challenger.h, buf, C.c_size_t(size))
    assert got == size
    return bytes(buf)


def basefold_verify(commitments, point, claims_per_round, blob, challenger, log_blowup=2, num_queries=124,
                    pow_bits=16):
    """claims_per_round: list (per round) of [total_cols][4] arrays. Returns 0 when the proof verifies."""
    point = _arr(point).reshape(-1, 4)
    commitments = _arr(np.stack(commitments))
    flat = _arr(np.concatenate([np.asarray(c, np.uint32).reshape(-1, 4) for c in claims_per_round]))
    counts = (C.c_int * len(claims_per_round))(*[np.asarray(c).reshape(-1, 4).shape[0] for c in claims_per_round])
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    return lib().orc_basefold_verify(_p(commitments), commitments.shape[0], _p(point), point.shape[0], _p(flat),
                                     counts, buf, C.c_size_t(len(blob)), log_blowup, num_queries, pow_bits,
                                     challenger.h)


def interleave(tables, batch_size, lsh):
    tables = [_arr(t) for t in tables]
    rows = (C.c_uint64 * len(tables))(*[t.shape[0] for t in tables])
    cols = (C.c_int * len(tables))(*[t.shape[1] for t in tables])
    nb = lib().orc_interleave(_ptr_array(tables), rows, cols, len(tables), C.c_size_t(batch_size), lsh, None, None)
    area = sum(t.size for t in tables)
    H = 1 << lsh
    padded = -(-area // H) * H
    out = np.zeros(max(padded, 1), np.uint32)
    widths = (C.c_int * nb)()
    lib().orc_interleave(_ptr_array(tables), rows, cols, len(tables), C.c_size_t(batch_size), lsh, _p(out), widths)
    res, o = [], 0
    for w in widths:
        res.append(out[o:o + H * w].reshape(H, w).copy())
        o += H * w
    return res


def jagged_commit_wrap(commit, rows, cols, num_added_vals, max_log_row_count):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    out = np.zeros(8, np.uint32)
    lib().orc_jagged_commit_wrap(_p(_arr(commit)), rows.ctypes.data_as(u64p), cols.ctypes.data_as(u64p), len(rows),
                                 C.c_uint64(num_added_vals), max_log_row_count, _p(out))
    return out


# ---- zerocheck ------------------------------------------------------------------------------------
class ZcChip:
    """One chip for the oracle's zerocheck: program ([n][3] u32), widths, traces (row-major, real rows
    only, Montgomery) and the trace-column evaluations at zeta (main then prep, [w][4])."""

    def __init__(self, prog, main_width, prep_width, num_constraints, main, prep=None, openings=None):
        self.prog = np.ascontiguousarray(prog, dtype=np.uint32).reshape(-1, 3)
        self.main_width, self.prep_width, self.num_constraints = main_width, prep_width, num_constraints
        self.main = _arr(main).reshape(-1, main_width) if main_width else np.zeros((0, 0), np.uint32)
        self.prep = _arr(prep).reshape(-1, prep_width) if prep_width else None
        self.real_rows = self.main.shape[0]
        self.openings = None if openings is None else _arr(openings).reshape(-1, 4)


def _zc_common(chips):
    n = len(chips)
    progs = _ptr_array([c.prog for c in chips])
    lens = (C.c_int * n)(*[c.prog.shape[0] for c in chips])
    mw = (C.c_int * n)(*[c.main_width for c in chips])
    pw = (C.c_int * n)(*[c.prep_width for c in chips])
    nc = (C.c_int * n)(*[c.num_constraints for c in chips])
    return n, progs, lens, mw, pw, nc


def zerocheck_prove(chips, max_log_row_count, zeta, alpha, gkr, publics, challenger, two_round_form=False):
    """two_round_form: restate the prover that takes rounds 0 and 1 from one pass over the base tables — the constraints' values on
    real rows are left out of round 1's node 0 as they are out of round 0's (kb_zerocheck.hpp). The same bytes on a satisfying
    trace; on any other table, what that prover gives (max_log_row_count >= 2; with one variable there is no second round)."""
    L = lib()
    L.orc_zerocheck_prove.restype = C.c_size_t
    n, progs, lens, mw, pw, nc = _zc_common(chips)
    mains = (u32p * n)(*[_p(c.main) if c.main.size else None for c in chips])
    preps = (u32p * n)(*[_p(c.prep) if c.prep is not None and c.prep.size else None for c in chips])
    rows = (C.c_uint64 * n)(*[c.real_rows for c in chips])
    openings = _arr(np.concatenate([c.openings for c in chips]))
    zeta, alpha, gkr, publics = _arr(zeta).reshape(-1, 4), _arr(alpha), _arr(gkr), _arr(publics).reshape(-1)
    args = [n, progs, lens, mw, pw, nc, mains, preps, rows, _p(openings), max_log_row_count, _p(zeta), _p(alpha), _p(gkr),
            _p(publics) if publics.size else None, int(publics.size)]
    probe = challenger.clone()
    L.orc_set_zc_two_round_form(1 if two_round_form else 0)
    try:
        size = L.orc_zerocheck_prove(*args, C.c_void_p(probe.h), None, C.c_size_t(0))
        buf = (C.c_uint8 * size)()
        got = L.orc_zerocheck_prove(*args, C.c_void_p(challenger.h), buf, C.c_size_t(size))
    finally:
        L.orc_set_zc_two_round_form(0)
    assert got == size
    return bytes(buf)


def zerocheck_verify(chips, heights, max_log_row_count, zeta, alpha, gkr, publics, blob, challenger):
    L = lib()
    n, progs, lens, mw, pw, nc = _zc_common(chips)
    hs = (C.c_uint64 * n)(*heights)
    openings = _arr(np.concatenate([c.openings for c in chips]))
    zeta, alpha, gkr, publics = _arr(zeta).reshape(-1, 4), _arr(alpha), _arr(gkr), _arr(publics).reshape(-1)
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    return L.orc_zerocheck_verify(n, progs, lens, mw, pw, nc, hs, _p(openings), max_log_row_count, _p(zeta), _p(alpha),
                                  _p(gkr), _p(publics) if publics.size else None, int(publics.size), buf,
                                  C.c_size_t(len(blob)), C.c_void_p(challenger.h))


def sumcheck_rounds_consistent(polys, claimed_sum, point, eval_):
    polys = _arr(polys)
    return lib().orc_sumcheck_rounds_consistent(_p(polys), polys.shape[0], polys.shape[1], _p(_arr(claimed_sum)),
                                                _p(_arr(point)), _p(_arr(eval_)))


def padded_column_openings(table, max_log_row_count, zeta):
    """Evaluations at zeta of every column of `table` zero-padded to 2^max_log_row_count rows."""
    t = _arr(table)
    full = np.zeros((1 << max_log_row_count, t.shape[1]), np.uint32)
    full[:t.shape[0]] = t
    return eval_mle(full, zeta) if t.shape[1] else np.zeros((0, 4), np.uint32)


# ---- jagged PCS evaluation proof -------------------------------------------------
class JaggedRound:
    """JaggedProver::commit_multilinears on the CPU oracle: tables = list of [rows_k][cols_k] row-major arrays
    (rows_k may be 0). Keeps the stacked batches + BaseFold data for the evaluation proof."""

    def __init__(self, tables, max_log_row_count, lsh, batch_size, log_blowup):
        self.tables = [_arr(t) for t in tables]
        rows = (C.c_uint64 * len(tables))(*[t.shape[0] for t in self.tables])
        cols = (C.c_int * len(tables))(*[t.shape[1] for t in self.tables])
        self.commit = np.zeros(8, np.uint32)
        self.h = lib().orc_jagged_commit(_ptr_array(self.tables), rows, cols, len(tables), max_log_row_count, lsh,
                                         C.c_size_t(batch_size), log_blowup, _p(self.commit))

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_jagged_round_free(self.h)
            self.h = None


def _claims_args(claims_per_round):
    flat = _arr(np.concatenate([np.asarray(c, np.uint32).reshape(-1, 4) for c in claims_per_round]))
    counts = (C.c_int * len(claims_per_round))(*[np.asarray(c).reshape(-1, 4).shape[0] for c in claims_per_round])
    return flat, counts


def jagged_prove(z_row, claims_per_round, rounds, lsh, challenger, log_blowup=2, num_queries=124, pow_bits=16):
    """JaggedProver::prove_trusted_evaluations -> bincode(JaggedPcsProof)."""
    z_row = _arr(z_row).reshape(-1, 4)
    flat, counts = _claims_args(claims_per_round)
    hs = (C.c_void_p * len(rounds))(*[r.h for r in rounds])
    args = (_p(z_row), z_row.shape[0], len(rounds), hs, _p(flat), counts, lsh, log_blowup, num_queries, pow_bits)
    scratch = challenger.clone()                      # sizing pass on a copy of the transcript
    n = lib().orc_jagged_prove(*args, scratch.h, None, 0)
    buf = (C.c_uint8 * n)()
    lib().orc_jagged_prove(*args, challenger.h, buf, n)
    return bytes(buf)


def jagged_verify(commitments, z_row, claims_per_round, blob, lsh, challenger, log_blowup=2, num_queries=124, pow_bits=16):
    """JaggedPcsVerifier::verify_trusted_evaluations; 0 = accepted."""
    z_row = _arr(z_row).reshape(-1, 4)
    commitments = _arr(np.stack(commitments))
    flat, counts = _claims_args(claims_per_round)
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    return lib().orc_jagged_verify(_p(commitments), commitments.shape[0], _p(z_row), z_row.shape[0], _p(flat), counts, buf,
                                   C.c_size_t(len(blob)), lsh, log_blowup, num_queries, pow_bits, challenger.h)


def partial_jagged_table(heights, max_log_row_count, z_row, z_col):
    heights = np.ascontiguousarray(heights, dtype=np.uint64)
    z_row, z_col = _arr(z_row).reshape(-1, 4), _arr(z_col).reshape(-1, 4)
    total = int(heights.sum())
    log_m = max(total - 1, 0).bit_length()
    out = np.zeros((1 << log_m, 4), np.uint32)
    lib().orc_partial_jagged_table(heights.ctypes.data_as(u64p), C.c_size_t(len(heights)), max_log_row_count, _p(z_row),
                                   _p(z_col), z_col.shape[0], _p(out))
    return out


def full_jagged_eval(heights, z_row, z_col, z_index):
    heights = np.ascontiguousarray(heights, dtype=np.uint64)
    z_row, z_col, z_index = (_arr(z).reshape(-1, 4) for z in (z_row, z_col, z_index))
    out = np.zeros(4, np.uint32)
    lib().orc_full_jagged_eval(heights.ctypes.data_as(u64p), C.c_size_t(len(heights)), _p(z_row), z_row.shape[0], _p(z_col),
                               z_col.shape[0], _p(z_index), z_index.shape[0], _p(out))
    return out


# ---- LogUp-GKR -------------------------------------------------------------------
def _gkr_chip_args(chips):
    """chips: [(InteractionProgram-like with .name/.main_width/.prep_width/.to_array(), main, prep or None)]."""
    n = len(chips)
    names = (C.c_char_p * n)(*[c[0].name.encode() for c in chips])
    progs = [np.ascontiguousarray(c[0].to_array(), dtype=np.uint32) for c in chips]
    mains = [_arr(c[1]) for c in chips]
    preps = [None if c[2] is None else _arr(c[2]) for c in chips]
    prog_ptrs = (u32p * n)(*[_p(a) for a in progs])
    main_ptrs = (u32p * n)(*[_p(a) if a.size else None for a in mains])
    prep_ptrs = (u32p * n)(*[None if a is None or not a.size else _p(a) for a in preps])
    mw = (C.c_int * n)(*[c[0].main_width for c in chips])
    pw = (C.c_int * n)(*[c[0].prep_width for c in chips])
    rows = (C.c_uint64 * n)(*[m.shape[0] for m in mains])
    keep = (progs, mains, preps)
    return n, names, prog_ptrs, mw, pw, main_ptrs, prep_ptrs, rows, keep


def gkr_prove(chips, max_log_row_count, challenger):
    """GkrProverImpl::prove_logup_gkr -> bincode(LogupGkrProof). Chips in name order."""
    n, names, progs, mw, pw, mains, preps, rows, keep = _gkr_chip_args(chips)
    scratch = challenger.clone()
    size = lib().orc_gkr_prove(n, names, progs, mw, pw, mains, preps, rows, max_log_row_count, scratch.h, None, 0)
    buf = (C.c_uint8 * size)()
    lib().orc_gkr_prove(n, names, progs, mw, pw, mains, preps, rows, max_log_row_count, challenger.h, buf, size)
    return bytes(buf)


def _pv_program_args(pv_program):
    """pv_program: None, or the machine's eval_public_values as (AirProgram over PUBLIC words, InteractionProgram over the row of
    public values, max interaction-kind arity, PROOF_MAX_NUM_PVS) — sp1_amd/machines/public_values.py."""
    if pv_program is None:
        return (None, 0, 0, None, 0), 0, 1, None
    air, it, max_arity, max_pvs = pv_program
    zc = np.ascontiguousarray(air.to_array(), dtype=np.uint32)
    gk = np.ascontiguousarray(it.to_array(), dtype=np.uint32)
    return (_p(zc), zc.shape[0], air.num_constraints, _p(gk), it.main_width), max_pvs, max_arity, (zc, gk)


def gkr_verify(chips, heights, max_log_row_count, blob, challenger, pv_program=None, publics=None):
    """LogUpGkrVerifier::verify_logup_gkr with the final interaction check; 0 = accepted. `pv_program` / `publics`: the
    machine's eval_public_values and the shard's public values (the cumulative sum the circuit output must have)."""
    n, names, progs, mw, pw, _, _, _, keep = _gkr_chip_args(chips)
    hs = (C.c_uint64 * n)(*heights)
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    (zc, zl, nc, gk, npv), _, max_arity, keep2 = _pv_program_args(pv_program)
    pv = _arr(publics).reshape(-1) if publics is not None else np.zeros(0, dtype=np.uint32)
    return lib().orc_gkr_verify_pv(n, names, progs, mw, pw, hs, max_log_row_count, buf, C.c_size_t(len(blob)), 1, -1, challenger.h,
                                   zc, zl, nc, gk, npv, max_arity, _p(pv) if pv.size else None, int(pv.size))


def gkr_verify_transcript_only(max_log_row_count, blob, beta_seed_dim, challenger):
    """Everything of verify_logup_gkr that does not need the machine's chips (used on the reference's real proof)."""
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    return lib().orc_gkr_verify(0, None, None, None, None, None, max_log_row_count, buf, C.c_size_t(len(blob)), 0,
                                beta_seed_dim, challenger.h)


# ---- whole shard proof ---------------------------------------------------------------------------------
def _shard_chip_args(chips):
    """chips: [(AirProgram, InteractionProgram, main row-major, prep row-major or None)] in name order."""
    n = len(chips)
    airs = [np.ascontiguousarray(c[0].to_array(), dtype=np.uint32) for c in chips]
    zc_ptrs = (u32p * n)(*[_p(a) for a in airs])
    zc_lens = (C.c_int * n)(*[a.shape[0] for a in airs])
    nc = (C.c_int * n)(*[c[0].num_constraints for c in chips])
    for c in chips:
        assert (c[0].main_width, c[0].prep_width) == (c[1].main_width, c[1].prep_width), "AIR / interaction widths differ"
    g = _gkr_chip_args([(c[1], c[2], c[3]) for c in chips])
    return n, g[1], zc_ptrs, zc_lens, g[3], g[4], nc, g[2], g[5], g[6], g[7], (airs, g[8])


def _check_publics(chips, n_publics):
    """A constraint program that reads public value i needs at least i + 1 of them (the C side indexes the array unchecked)."""
    need = 0
    for c in chips:
        for op, a, _ in c[0].instrs:
            if op == 3:                                     # PUBLIC idx
                need = max(need, a + 1)
    if need > n_publics:
        raise ValueError("the constraint programs read public value %d; only %d were passed" % (need - 1, n_publics))


def shard_prove(chips, publics, prep_round, L, lsh, batch, challenger, log_blowup=2, num_queries=124, pow_bits=16, capacity=None):
    """ShardProver::prove_shard_with_data -> bincode(ShardProof). prep_round: JaggedRound of the preprocessed traces."""
    n, names, zc, zl, mw, pw, nc, gk, mains, preps, rows, keep = _shard_chip_args(chips)
    pv = _arr(publics).reshape(-1)
    _check_publics(chips, pv.size)
    args = (n, names, zc, zl, mw, pw, nc, gk, mains, preps, rows, _p(pv) if pv.size else None, int(pv.size), prep_round.h, L,
            lsh, C.c_size_t(batch), log_blowup, num_queries, pow_bits)
    if capacity:                                             # ONE pass (the CPU baseline times this): a buffer that is surely large enough
        buf = (C.c_uint8 * capacity)()
        size = lib().orc_shard_prove(*args, challenger.h, buf, capacity)
        if size > capacity:
            raise ValueError("shard proof needs %d bytes" % size)
        return bytes(buf[:size]) if size < (1 << 16) else C.string_at(buf, size)
    scratch = challenger.clone()
    size = lib().orc_shard_prove(*args, scratch.h, None, 0)
    buf = (C.c_uint8 * size)()
    lib().orc_shard_prove(*args, challenger.h, buf, size)
    return bytes(buf)


def set_threads(n):
    """OpenMP threads of the oracle in this process (several oracle processes on one box: tests/test_multirank.py)."""
    lib().orc_set_threads(int(n))


def set_gkr_sparse(on):
    """LogUp-GKR formulation of shard_prove / gkr_prove: False = dense (independent of the GPU algorithm, small sizes only),
    True = real rows + closed-form padding (the reference's CPU shape; what the CPU baseline times)."""
    lib().orc_set_gkr_sparse(1 if on else 0)


def stage_seconds():
    """Wall seconds of the calling thread's last shard_prove: {commit, logup_gkr, zerocheck, evaluation_proof}."""
    out = (C.c_double * 4)()
    lib().orc_stage_seconds(out)
    return dict(zip(("commit", "logup_gkr", "zerocheck", "evaluation_proof"), list(out)))


def shard_verify(chips, prep_commit, blob, L, lsh, challenger, log_blowup=2, num_queries=124, pow_bits=16, pv_program=None):
    """ShardVerifier::verify_shard with every chip-dependent check; 0 = accepted. `pv_program`: the machine's
    eval_public_values (_pv_program_args) — the RISC-V machine has one, the recursion machine does not."""
    n, names, zc, zl, mw, pw, nc, gk, _, _, _, keep = _shard_chip_args(chips)
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    (pzc, pzl, pnc, pgk, npv), max_pvs, max_arity, keep2 = _pv_program_args(pv_program)
    return lib().orc_shard_verify_pv(n, names, zc, zl, mw, pw, nc, gk, _p(_arr(prep_commit)), buf, C.c_size_t(len(blob)), L, lsh,
                                     log_blowup, num_queries, pow_bits, 1, -1, challenger.h, pzc, pzl, pnc, pgk, npv, max_pvs, max_arity)


def shard_verify_transcript_only(prep_commit, blob, L, lsh, beta_seed_dim, challenger, log_blowup=2, num_queries=124, pow_bits=16):
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    return lib().orc_shard_verify(0, None, None, None, None, None, None, None, _p(_arr(prep_commit)), buf, C.c_size_t(len(blob)),
                                  L, lsh, log_blowup, num_queries, pow_bits, 0, beta_seed_dim, challenger.h)
