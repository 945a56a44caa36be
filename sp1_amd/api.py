"""Thin Python mirror of the reference's operator interfaces for the core-shard commit/open path,
calling the HIP backend through the C ABI (include/sp1hip.h). PyTorch is used only as the owner of
device memory (int32 tensors reinterpreted as u32 words) and for streams; every computation is a
hand-written gfx950 kernel inside libsp1hip.so. There is no CPU fallback.

Names follow the reference:
  DuplexChallenger                 slop_challenger::DuplexChallenger      (/root/reference/slop/crates/challenger/src/lib.rs:L25-L87)
  DftEncoder.encode_batch          CpuDftEncoder::encode_batch            (/root/reference/slop/crates/basefold-prover/src/encoder.rs:L22-L38)
  MerkleTcsProver.commit_tensors / prove_openings_at_indices / compute_openings_at_indices
                                   TensorCsProver / ComputeTcsOpenings    (/root/reference/slop/crates/merkle-tree/src/tcs.rs:L15-L47)
  BasefoldProver.commit_mles / prove_trusted_mle_evaluations
                                   BasefoldProver                         (/root/reference/slop/crates/basefold-prover/src/prover.rs:L78-L243)
Device layouts: base tensors column-major [height x width]; ext vectors SoA (see include/sp1hip.h).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import Ext, FriConfig, GkrChip, ShardChip, ShardParams, Table, Tensor, ZcChip, check

P = 0x7F000001


def _L():
    return _lib.load()


def _stream_ptr(stream=None):
    if stream is None:
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


def _dptr(t):
    return C.c_void_p(t.data_ptr())


def device_words(n, device=None):
    """Uninitialised device buffer of n u32 words."""
    return torch.empty(int(n), dtype=torch.int32, device=device or torch.device("cuda", torch.cuda.current_device()))


def to_device(a, device=None):
    """numpy uint32 array -> flat device word buffer (same memory order)."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    t = torch.from_numpy(a.view(np.int32).reshape(-1))
    return t.to(device or torch.device("cuda", torch.cuda.current_device()), non_blocking=False)


def to_host(t, shape=None):
    a = t.detach().cpu().numpy().view(np.uint32)
    return a.reshape(shape) if shape is not None else a


def _ext(x):
    e = Ext()
    for k in range(4):
        e.c[k] = int(x[k])
    return e


def _ext_array(xs):
    xs = np.asarray(xs, dtype=np.uint32).reshape(-1, 4)
    arr = (Ext * max(len(xs), 1))()
    for i, x in enumerate(xs):
        for k in range(4):
            arr[i].c[k] = int(x[k])
    return arr


class ColMajor:
    """A column-major [height x width] base-field tensor in device memory (Montgomery words)."""

    def __init__(self, words, height, width):
        assert words.numel() == height * width and words.dtype == torch.int32
        self.words, self.height, self.width = words, int(height), int(width)

    @staticmethod
    def from_row_major_host(a, stream=None):
        """Upload a row-major numpy [height][width] array and transpose it on the GPU."""
        a = np.ascontiguousarray(a, dtype=np.uint32)
        h, w = a.shape
        src = to_device(a)
        dst = device_words(h * w)
        check(_L().sp1hip_transpose_to_col_major(_dptr(dst), _dptr(src), h, w, _stream_ptr(stream)))
        return ColMajor(dst, h, w)

    def to_row_major_host(self, stream=None):
        dst = device_words(self.height * self.width)
        check(_L().sp1hip_transpose_to_row_major(_dptr(dst), _dptr(self.words), self.height, self.width,
                                                 _stream_ptr(stream)))
        return to_host(dst, (self.height, self.width))

    def as_tensor_struct(self):
        return Tensor(C.c_void_p(self.words.data_ptr()), self.width)


def stage_tables(host_tables, stream=None):
    """Row-major host traces -> column-major device tables, one call for the whole shard (sp1hip_stage_tables:
    chunked PCIe copies on a side stream overlapped with the on-GPU transposes; mirrors `device_main_tracegen`'s
    "copy host trace to device", /root/reference/sp1-gpu/crates/jagged_tracegen/src/lib.rs:L819-L835).
    `host_tables`: 2-D numpy uint32 arrays or CPU torch int32 tensors (pinned for the asynchronous path), Montgomery
    words. Returns a list of ColMajor; each keeps its host source alive (the copies are asynchronous)."""
    from ._lib import HostTable
    n = len(host_tables)
    arr = (HostTable * max(n, 1))()
    outs = (C.c_void_p * max(n, 1))()
    result = []
    for i, a in enumerate(host_tables):
        if isinstance(a, np.ndarray):
            assert a.dtype == np.uint32 and a.ndim == 2 and a.flags["C_CONTIGUOUS"], "row-major uint32 [rows][cols]"
            ptr, (h, w) = a.ctypes.data, a.shape
        else:
            assert a.dtype == torch.int32 and a.dim() == 2 and a.is_contiguous() and not a.is_cuda
            ptr, (h, w) = a.data_ptr(), a.shape
        dst = device_words(h * w)
        cm = ColMajor(dst, h, w)
        cm._host_source = a
        arr[i] = HostTable(C.c_void_p(ptr), h, w)
        outs[i] = C.c_void_p(dst.data_ptr())
        result.append(cm)
    check(_L().sp1hip_stage_tables(arr, n, outs, _stream_ptr(stream)))
    return result


def _tensor_array(tensors):
    arr = (Tensor * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.as_tensor_struct()
    return arr


class DuplexChallenger:
    def __init__(self, handle=None):
        if handle is None:
            handle = C.c_void_p()
            check(_L().sp1hip_challenger_new(C.byref(handle)))
        self.h = handle

    def clone(self):
        out = C.c_void_p()
        check(_L().sp1hip_challenger_clone(self.h, C.byref(out)))
        return DuplexChallenger(out)

    def observe(self, felts):
        a = np.ascontiguousarray(np.asarray(felts, dtype=np.uint32).reshape(-1))
        check(_L().sp1hip_challenger_observe(self.h, a.ctypes.data_as(_lib.u32p), a.size))

    def sample(self):
        out = C.c_uint32()
        check(_L().sp1hip_challenger_sample(self.h, C.byref(out)))
        return out.value

    def sample_ext_element(self):
        e = Ext()
        check(_L().sp1hip_challenger_sample_ext(self.h, C.byref(e)))
        return np.array(list(e.c), dtype=np.uint32)

    def sample_point(self, n):
        return np.stack([self.sample_ext_element() for _ in range(n)]) if n else np.zeros((0, 4), np.uint32)

    def sample_bits(self, bits):
        out = C.c_uint32()
        check(_L().sp1hip_challenger_sample_bits(self.h, bits, C.byref(out)))
        return out.value

    def check_witness(self, bits, witness):
        ok = C.c_int()
        check(_L().sp1hip_challenger_check_witness(self.h, bits, C.c_uint32(int(witness)), C.byref(ok)))
        return bool(ok.value)

    def inject_pow_witnesses(self, witnesses):
        """Canonical proof-of-work witnesses for the next grinds, in order (sp1hip_challenger_inject_pow_witnesses)."""
        w = (C.c_uint32 * max(len(witnesses), 1))(*[int(x) for x in witnesses])
        check(_L().sp1hip_challenger_inject_pow_witnesses(self.h, w, len(witnesses)))

    def grind(self, bits, stream=None):
        out = C.c_uint32()
        check(_L().sp1hip_challenger_grind(self.h, bits, C.byref(out), _stream_ptr(stream)))
        return out.value

    def state(self):
        out = np.zeros(34, np.uint32)
        check(_L().sp1hip_challenger_state(self.h, out.ctypes.data_as(_lib.u32p)))
        return out

    def __del__(self):
        if getattr(self, "h", None) and _L is not None:      # _L is None during interpreter shutdown
            try:
                _L().sp1hip_challenger_free(self.h)
            except TypeError:                    # interpreter shutdown: the module globals are already gone
                pass
            self.h = None


class DftEncoder:
    """Reed–Solomon encoder: zero-pad by 2^log_blowup, forward DFT, bit-reversed rows."""

    def __init__(self, log_blowup):
        self.log_blowup = int(log_blowup)

    def encode_batch(self, mles, stream=None):
        out = []
        for m in mles:
            lg_n = m.height.bit_length() - 1
            assert 1 << lg_n == m.height
            cw = device_words((m.height << self.log_blowup) * m.width)
            check(_L().sp1hip_rs_encode_batch(_dptr(cw), _dptr(m.words), lg_n, self.log_blowup, m.width,
                                              _stream_ptr(stream)))
            out.append(ColMajor(cw, m.height << self.log_blowup, m.width))
        return out


class TcsProverData:
    def __init__(self, tree, root, commit, log_height, total_width):
        self.tree, self.root, self.commit = tree, root, commit
        self.log_height, self.total_width = log_height, total_width


class MerkleTcsProver:
    """Poseidon2KoalaBear16Prover: Merkle tensor commitment over rows of column-major tensors."""

    def commit_tensors(self, tensors, stream=None):
        h = tensors[0].height
        lg = h.bit_length() - 1
        assert all(t.height == h for t in tensors) and 1 << lg == h
        tree = device_words((2 * h - 1) * 8)
        rc = device_words(16)
        check(_L().sp1hip_merkle_commit(_tensor_array(tensors), len(tensors), lg, _dptr(tree), _dptr(rc),
                                        _stream_ptr(stream)))
        rc_h = to_host(rc)
        data = TcsProverData(tree, rc_h[:8].copy(), rc_h[8:].copy(), lg, sum(t.width for t in tensors))
        return data.commit, data

    def _indices(self, indices):
        return to_device(np.asarray(indices, dtype=np.uint32))

    def prove_openings_at_indices(self, data, indices, stream=None):
        idx = self._indices(indices)
        paths = device_words(len(indices) * data.log_height * 8)
        none = (Tensor * 1)(Tensor(None, 0))
        check(_L().sp1hip_merkle_open(none, 1, data.log_height, _dptr(data.tree), _dptr(idx), len(indices), None,
                                      _dptr(paths), _stream_ptr(stream)))
        return dict(merkle_root=data.root, log_tensor_height=data.log_height, width=data.total_width,
                    paths=to_host(paths, (len(indices), data.log_height, 8)))

    def compute_openings_at_indices(self, tensors, indices, stream=None):
        idx = self._indices(indices)
        tw = sum(t.width for t in tensors)
        lg = tensors[0].height.bit_length() - 1
        vals = device_words(len(indices) * tw)
        check(_L().sp1hip_merkle_open(_tensor_array(tensors), len(tensors), lg, None, _dptr(idx), len(indices),
                                      _dptr(vals), None, _stream_ptr(stream)))
        return to_host(vals, (len(indices), tw))


class BasefoldProverData:
    def __init__(self, handle, mles, commit):
        self.h, self.mles, self.commit = handle, mles, commit

    def codeword(self, k):
        ptr, width, lg = C.c_void_p(), C.c_uint32(), C.c_int()
        check(_L().sp1hip_basefold_data_codeword(self.h, k, C.byref(ptr), C.byref(width), C.byref(lg)))
        n = (1 << lg.value) * width.value
        out = device_words(n)
        check(_L().sp1hip_memcpy_d2d_async(_dptr(out), ptr, n * 4, _stream_ptr()))
        return ColMajor(out, 1 << lg.value, width.value)

    def tree(self):
        ptr, lg = C.c_void_p(), C.c_int()
        check(_L().sp1hip_basefold_data_tree(self.h, C.byref(ptr), C.byref(lg)))
        n = ((2 << lg.value) - 1) * 8
        out = device_words(n)
        check(_L().sp1hip_memcpy_d2d_async(_dptr(out), ptr, n * 4, _stream_ptr()))
        return to_host(out, (n // 8, 8))

    def __del__(self):
        if getattr(self, "h", None):
            try:
                _L().sp1hip_basefold_data_free(self.h)
            except TypeError:                    # interpreter shutdown: the module globals are already gone
                pass
            self.h = None


class BasefoldProver:
    def __init__(self, log_blowup=2, num_queries=124, proof_of_work_bits=16):
        self.config = FriConfig(log_blowup, num_queries, proof_of_work_bits)

    def commit_mles(self, mles, stream=None):
        lg_n = mles[0].height.bit_length() - 1
        assert all(m.height == 1 << lg_n for m in mles)
        commit = np.zeros(8, np.uint32)
        handle = C.c_void_p()
        check(_L().sp1hip_commit_mles(_tensor_array(mles), len(mles), lg_n, self.config.log_blowup,
                                      commit.ctypes.data_as(_lib.u32p), C.byref(handle), _stream_ptr(stream)))
        return commit, BasefoldProverData(handle, list(mles), commit)

    def evaluate_mles(self, mles, point, stream=None):
        """Claims for `prove_trusted_mle_evaluations`: every column of every mle at `point` ([dim][4])."""
        point = np.asarray(point, dtype=np.uint32).reshape(-1, 4)
        dim = point.shape[0]
        eq = device_words(4 << dim)
        check(_L().sp1hip_partial_lagrange(_ext_array(point), dim, _dptr(eq), _stream_ptr(stream)))
        tw = sum(m.width for m in mles)
        out = device_words(tw * 4)
        check(_L().sp1hip_mle_eval_columns(_tensor_array(mles), len(mles), dim, _dptr(eq), _dptr(out),
                                           _stream_ptr(stream)))
        return to_host(out, (tw, 4))

    def prove_trusted_mle_evaluations(self, eval_point, prover_data, evaluation_claims, challenger, stream=None):
        """prover_data: list of BasefoldProverData (one per commitment round); evaluation_claims: [total][4]."""
        point = np.asarray(eval_point, dtype=np.uint32).reshape(-1, 4)
        claims = np.asarray(evaluation_claims, dtype=np.uint32).reshape(-1, 4)
        widths = (C.c_uint32 * len(prover_data))(*[sum(m.width for m in pd.mles) for pd in prover_data])
        size = _L().sp1hip_basefold_proof_size(point.shape[0], widths, len(prover_data), self.config)
        buf = (C.c_uint8 * size)()
        n = C.c_size_t(size)
        handles = (C.c_void_p * len(prover_data))(*[pd.h for pd in prover_data])
        check(_L().sp1hip_basefold_prove(_ext_array(point), point.shape[0], handles, len(prover_data),
                                         _ext_array(claims), claims.shape[0], self.config, challenger.h, buf,
                                         C.byref(n), _stream_ptr(stream)))
        return C.string_at(buf, n.value)        # (slicing a c_uint8 array would build a list of ints first: ~20 ms per MB)


class _BorrowedBasefoldData:
    """Non-owning view of the BaseFold data inside a stacked commitment (freed with its owner)."""

    def __init__(self, handle, commit, widths):
        self.h, self.commit = handle, commit
        self.mles = [_Width(w) for w in widths]


class _Width:
    def __init__(self, width):
        self.width = width


class _RawColMajor:
    """A ColMajor-like view over device memory owned elsewhere."""

    def __init__(self, ptr, height, width):
        self.ptr, self.height, self.width = ptr, height, width

    def as_tensor_struct(self):
        return Tensor(self.ptr, self.width)


class StackedData:
    """Owns the dense stacked buffer + BaseFold data of one commitment (StackedBasefoldProverData)."""

    def __init__(self, handle, commit, num_added_vals, log_stacking_height):
        self.h, self.commit, self.num_added_vals, self.lsh = handle, commit, num_added_vals, log_stacking_height
        bf, nb, dense, padded = C.c_void_p(), C.c_int(), C.c_void_p(), C.c_uint64()
        check(_L().sp1hip_stacked_data_info(handle, C.byref(bf), C.byref(nb), C.byref(dense), C.byref(padded)))
        self.padded_area = padded.value
        self.batches = []
        for k in range(nb.value):
            t = Tensor()
            check(_L().sp1hip_stacked_batch(handle, k, C.byref(t)))
            self.batches.append(_RawColMajor(t.d_data, 1 << log_stacking_height, t.width))
        self.basefold = _BorrowedBasefoldData(bf, commit, [t.width for t in self.batches])

    def __del__(self):
        if getattr(self, "h", None):
            try:
                _L().sp1hip_stacked_data_free(self.h)
            except TypeError:                    # interpreter shutdown: the module globals are already gone
                pass
            self.h = None


def _table_array(tables):
    arr = (Table * max(len(tables), 1))()
    for i, t in enumerate(tables):
        arr[i] = Table(C.c_void_p(t.words.data_ptr()) if t.height * t.width else None, t.height, t.width)
    return arr


class StackedPcsProver:
    def __init__(self, log_stacking_height, batch_size, log_blowup=2):
        self.lsh, self.batch_size, self.log_blowup = log_stacking_height, batch_size, log_blowup

    def commit_multilinears(self, tables, stream=None):
        commit = np.zeros(8, np.uint32)
        added, handle = C.c_uint64(), C.c_void_p()
        check(_L().sp1hip_stacked_commit(_table_array(tables), len(tables), self.lsh, self.batch_size, self.log_blowup,
                                         commit.ctypes.data_as(_lib.u32p), C.byref(added), C.byref(handle),
                                         _stream_ptr(stream)))
        return commit, StackedData(handle, commit, added.value, self.lsh), added.value


class JaggedProver:
    """JaggedProver::commit_multilinears over chip tables (zero-row tables are counted, not committed)."""

    def __init__(self, max_log_row_count, log_stacking_height, batch_size, log_blowup=2):
        self.max_log_row_count, self.lsh = max_log_row_count, log_stacking_height
        self.batch_size, self.log_blowup = batch_size, log_blowup

    def commit_multilinears(self, tables, stream=None):
        commit = np.zeros(8, np.uint32)
        handle = C.c_void_p()
        check(_L().sp1hip_jagged_commit(_table_array(tables), len(tables), self.max_log_row_count, self.lsh,
                                        self.batch_size, self.log_blowup, commit.ctypes.data_as(_lib.u32p),
                                        C.byref(handle), _stream_ptr(stream)))
        return commit, StackedData(handle, commit, None, self.lsh)

    def prove_trusted_evaluations(self, z_row, claims_per_round, rounds, challenger, num_queries=124, pow_bits=16,
                                  stream=None):
        """JaggedProver::prove_trusted_evaluations (/root/reference/slop/crates/jagged/src/prover.rs:L162-L328).
        rounds: the StackedData of every commitment round, in order; claims_per_round[r]: [n_cols_r][4] column
        evaluations at z_row of round r's tables. Returns bincode(JaggedPcsProof); advances the challenger."""
        z_row = np.ascontiguousarray(np.asarray(z_row, dtype=np.uint32).reshape(-1, 4))
        assert z_row.shape[0] == self.max_log_row_count
        cl = [np.asarray(c, dtype=np.uint32).reshape(-1, 4) for c in claims_per_round]
        flat = np.ascontiguousarray(np.concatenate(cl)) if cl else np.zeros((0, 4), np.uint32)
        counts = (C.c_size_t * len(rounds))(*[c.shape[0] for c in cl])
        hs = (C.c_void_p * len(rounds))(*[r.h for r in rounds])
        cfg = FriConfig(self.log_blowup, num_queries, pow_bits)
        n = C.c_size_t(0)
        args = [_ext_array(z_row), self.max_log_row_count, hs, len(rounds), _ext_array(flat) if flat.size else None, counts,
                cfg, challenger.h]
        st = _L().sp1hip_jagged_prove(*args, None, C.byref(n), _stream_ptr(stream))
        if st != _lib.ERROR_BUFFER_TOO_SMALL:                                   # anything but BUFFER_TOO_SMALL is a real error
            check(st)
            raise RuntimeError("size query unexpectedly succeeded")
        buf = (C.c_uint8 * n.value)()
        check(_L().sp1hip_jagged_prove(*args, buf, C.byref(n), _stream_ptr(stream)))
        return C.string_at(buf, n.value)        # (slicing a c_uint8 array would build a list of ints first: ~20 ms per MB)


class ZerocheckChip:
    """One chip for `zerocheck`: an `sp1_amd.air.AirProgram`, column-major device traces (real rows only)."""

    def __init__(self, air, main, prep=None):
        self.air, self.main, self.prep = air, main, prep
        self.program = np.ascontiguousarray(air.to_array(), dtype=np.uint32)
        self.real_rows = main.height if main is not None else 0


def zerocheck(chips, max_log_row_count, zeta, openings, alpha, gkr_batch, public_values, challenger, stream=None):
    """ShardProver::zerocheck on the GPU. openings: per chip main then preprocessed column evaluations
    at zeta, concatenated [total][4]. Returns the proof bytes (layout in include/sp1hip.h)."""
    arr = (ZcChip * len(chips))()
    for i, c in enumerate(chips):
        arr[i] = ZcChip(c.program.ctypes.data_as(_lib.u32p), c.program.shape[0], c.air.main_width, c.air.prep_width,
                        c.air.num_constraints,
                        C.c_void_p(c.main.words.data_ptr()) if c.real_rows and c.air.main_width else None,
                        C.c_void_p(c.prep.words.data_ptr()) if c.real_rows and c.prep is not None else None, c.real_rows)
    pv = np.ascontiguousarray(np.asarray(public_values, dtype=np.uint32).reshape(-1))
    zeta = np.asarray(zeta, dtype=np.uint32).reshape(-1, 4)
    n = C.c_size_t(0)
    args = [arr, len(chips), max_log_row_count, _ext_array(zeta), _ext_array(openings), _ext(alpha), _ext(gkr_batch),
            pv.ctypes.data_as(_lib.u32p) if pv.size else None, int(pv.size), challenger.h]
    st = _L().sp1hip_zerocheck_prove(*args, None, C.byref(n), _stream_ptr(stream))
    if st != _lib.ERROR_BUFFER_TOO_SMALL:                                       # anything but BUFFER_TOO_SMALL is a real error
        check(st)
        raise RuntimeError("size query unexpectedly succeeded")
    buf = (C.c_uint8 * n.value)()
    check(_L().sp1hip_zerocheck_prove(*args, buf, C.byref(n), _stream_ptr(stream)))
    return C.string_at(buf, n.value)        # (slicing a c_uint8 array would build a list of ints first: ~20 ms per MB)


def logup_gkr(chips, max_log_row_count, challenger, stream=None):
    """GkrProverImpl::prove_logup_gkr on the GPU. chips: [(sp1_amd.air.InteractionProgram, main ColMajor or None,
    prep ColMajor or None)] in name order. Returns bincode(LogupGkrProof); advances the challenger."""
    arr = (GkrChip * len(chips))()
    keep = []
    for i, (prog, main, prep) in enumerate(chips):
        words = np.ascontiguousarray(prog.to_array(), dtype=np.uint32)
        keep.append(words)
        rows = main.height if main is not None else (prep.height if prep is not None else 0)
        arr[i] = GkrChip(prog.name.encode(), words.ctypes.data_as(_lib.u32p), words.size, prog.main_width, prog.prep_width,
                         C.c_void_p(main.words.data_ptr()) if main is not None and rows and prog.main_width else None,
                         C.c_void_p(prep.words.data_ptr()) if prep is not None and rows and prog.prep_width else None, rows)
    n = C.c_size_t(0)
    st = _L().sp1hip_logup_gkr_prove(arr, len(chips), max_log_row_count, challenger.h, None, C.byref(n), _stream_ptr(stream))
    if st != _lib.ERROR_BUFFER_TOO_SMALL:
        check(st)
        raise RuntimeError("size query unexpectedly succeeded")
    buf = (C.c_uint8 * n.value)()
    check(_L().sp1hip_logup_gkr_prove(arr, len(chips), max_log_row_count, challenger.h, buf, C.byref(n), _stream_ptr(stream)))
    return C.string_at(buf, n.value)        # (slicing a c_uint8 array would build a list of ints first: ~20 ms per MB)


def _shard_chip_array(chips):
    arr = (ShardChip * len(chips))()
    keep = []
    for i, (air, inter, main, prep) in enumerate(chips):
        prog = np.ascontiguousarray(air.to_array(), dtype=np.uint32)
        words = np.ascontiguousarray(inter.to_array(), dtype=np.uint32)
        keep += [prog, words]
        rows = main.height if main is not None else 0
        arr[i] = ShardChip(inter.name.encode(), prog.ctypes.data_as(_lib.u32p), prog.shape[0], air.num_constraints,
                           words.ctypes.data_as(_lib.u32p), words.size, air.main_width, air.prep_width,
                           C.c_void_p(main.words.data_ptr()) if rows else None,
                           C.c_void_p(prep.words.data_ptr()) if prep is not None and rows and air.prep_width else None, rows)
    return arr, keep


def prove_shard(chips, public_values, preprocessed, max_log_row_count, log_stacking_height, batch_size, challenger,
                log_blowup=2, num_queries=124, pow_bits=16, stream=None):
    """ShardProver::prove_shard_with_data on the GPU (sp1hip_prove_shard). chips: [(AirProgram, InteractionProgram, main
    ColMajor or None, prep ColMajor or None)] in name order; preprocessed: the StackedData of the preprocessed round
    (JaggedProver.commit_multilinears over the preprocessed traces). Returns bincode(ShardProof)."""
    arr, keep = _shard_chip_array(chips)
    pv = np.ascontiguousarray(np.asarray(public_values, dtype=np.uint32).reshape(-1))
    params = ShardParams(max_log_row_count, log_stacking_height, batch_size, FriConfig(log_blowup, num_queries, pow_bits))
    args = [arr, len(chips), pv.ctypes.data_as(_lib.u32p) if pv.size else None, int(pv.size), preprocessed.h, params, challenger.h]
    # One call in the steady state: the calling thread's buffer of its previous proof is offered first; a shard that needs
    # more is answered with ERROR_BUFFER_TOO_SMALL and the size before any work (and before the transcript is touched).
    import threading
    me = threading.get_ident()
    buf = _PROOF_BUFS.get(me)
    for _ in range(2):
        n = C.c_size_t(len(buf) if buf is not None else 0)
        st = _L().sp1hip_prove_shard(*args, buf, C.byref(n), _stream_ptr(stream))
        if st != _lib.ERROR_BUFFER_TOO_SMALL:
            check(st)
            return C.string_at(buf, n.value)        # (slicing a c_uint8 array would build a list of ints first: ~20 ms per MB)
        buf = _PROOF_BUFS[me] = (C.c_uint8 * n.value)()
    check(st)


_PROOF_BUFS = {}     # thread id -> proof buffer (prove_shard)


# main-trace widths and events per row of the recursion chips with device trace generation (sp1hip_tracegen_recursion_*)
RECURSION_TRACEGEN = {"BaseAlu": ("base_alu", 3, 3, 1), "ExtAlu": ("ext_alu", 12, 12, 1), "Select": ("select", 5, 5, 1),
                      "MemoryVar": ("memory_var", 8, 4, 2), "PrefixSumChecks": ("prefix_sum_checks", 15, 20, 1),
                      "Poseidon2WideDeg3": ("poseidon2_wide", 179, 32, 1)}


def tracegen_recursion(chip, events, height, stream=None):
    """Main trace of a recursion chip generated on the device from its event array (`generate_trace_device`).
    events: [n_events][event_words] uint32 Montgomery words (numpy, or an int32 device tensor). Returns a ColMajor."""
    fn, width, event_words, _ = RECURSION_TRACEGEN[chip]
    if isinstance(events, np.ndarray):
        events = to_device(np.ascontiguousarray(events, dtype=np.uint32).reshape(-1, event_words))
    n = events.numel() // event_words
    out = device_words(int(height) * width)
    check(getattr(_L(), "sp1hip_tracegen_recursion_" + fn)(_dptr(out), int(height), _dptr(events) if n else None, n, _stream_ptr(stream)))
    return ColMajor(out, int(height), width)


def tracegen_riscv_global(events, height, stream=None):
    """`generate_trace_device` for the RISC-V Global chip (sp1hip_tracegen_riscv_global): events = device int32 tensor [n, 9]
    (message[8], is_receive | kind << 8); returns the column-major [241][height] table as a ColMajor."""
    n = int(events.shape[0])
    out = device_words(241 * height)
    check(_L().sp1hip_tracegen_riscv_global(_dptr(out), int(height), _dptr(events) if n else None, n, _stream_ptr(stream)))
    return ColMajor(out, int(height), 241)


RISCV_ALU_CHIPS = {"Add": 0, "Addi": 1, "Sub": 2, "Addw": 3, "Subw": 4, "Mul": 5, "ShiftRight": 6, "Branch": 7,    # SP1HIP_RV64_CHIP_*
                   "Bitwise": 8, "Lt": 9, "ShiftLeft": 10, "UType": 11, "Jal": 12, "Jalr": 13}
ALU_EVENT_WORDS = 11                                                                 # sp1hip_rv64_alu_event_t: 11 u64


def tracegen_riscv_alu(chip, events, height, stream=None):
    """`generate_trace_device` for one of the RISC-V instruction chips of RISCV_ALU_CHIPS (sp1hip_tracegen_riscv_alu): events = a
    device int64 tensor [n, 11] of sp1hip_rv64_alu_event_t records (riscv_exec.pack_alu_events); returns the column-major table
    [width][height] as a ColMajor."""
    return _tracegen_records("sp1hip_tracegen_riscv_alu", ALU_EVENT_WORDS, RISCV_ALU_CHIPS[chip], events, height, stream)


RISCV_MEM_CHIPS = {"LoadByte": 0, "LoadHalf": 1, "LoadWord": 2, "LoadDouble": 3, "LoadX0": 4,                     # SP1HIP_RV64_MEM_CHIP_*
                   "StoreByte": 5, "StoreHalf": 6, "StoreWord": 7, "StoreDouble": 8}
MEM_EVENT_WORDS = 12                                                                 # sp1hip_rv64_mem_event_t: 12 u64


def tracegen_riscv_mem(chip, events, height, stream=None):
    """`generate_trace_device` for one of the load and store chips of RISCV_MEM_CHIPS (sp1hip_tracegen_riscv_mem): events = a
    device int64 tensor [n, 12] of sp1hip_rv64_mem_event_t records (riscv_exec.pack_mem_events); returns the column-major table
    [width][height] as a ColMajor."""
    return _tracegen_records("sp1hip_tracegen_riscv_mem", MEM_EVENT_WORDS, RISCV_MEM_CHIPS[chip], events, height, stream)


def _n_records(records, words=None):
    """How many records a tracegen wrapper was handed, having checked them: an int64 tensor [n, words] (any width when `words` is
    None), on the device and contiguous unless it is empty."""
    n = int(records.shape[0])
    assert records.dtype == torch.int64 and (words is not None or records.dim() == 2)
    assert n == 0 or (records.is_cuda and records.is_contiguous() and (words is None or records.shape[1] == words))
    return n


def _tracegen_records(fn, words, kind, events, height, stream):
    """The body of every wrapper whose entry point makes one table from one stream of fixed-size records: `fn` the entry point
    (its width query is fn + "_width"), `words` the record's u64 words, `kind` the leading chip argument of both or None."""
    lead = () if kind is None else (kind,)
    width = getattr(_L(), fn + "_width")(*lead)
    n = _n_records(events, words)
    out = device_words(width * int(height))
    check(getattr(_L(), fn)(*lead, _dptr(out), int(height), _dptr(events) if n else None, n, _stream_ptr(stream)))
    return ColMajor(out, int(height), width)


def tracegen_riscv_divrem(events, height, stream=None):
    """`generate_trace_device` for the DivRem chip (sp1hip_tracegen_riscv_divrem): events = a device int64 tensor [n, 11] of
    sp1hip_rv64_alu_event_t records (riscv_exec.pack_alu_events(events, "DivRem")); returns the column-major [246][height] table as
    a ColMajor, rows >= n the reference's "0 / 1" padding row."""
    return tracegen_riscv_records("DivRem", events, height, stream)


def tracegen_riscv_alu_x0(events, height, stream=None):
    """The same for the AluX0 chip (sp1hip_tracegen_riscv_alu_x0; pack_alu_events(events, "AluX0")): column-major [34][height],
    zero padding rows."""
    return tracegen_riscv_records("AluX0", events, height, stream)


MEMORY_LOCAL_RECORD_WORDS, MEMORY_LOCAL_WIDTH, GLOBAL_EVENT_WORDS = 5, 20, 9


def _new_global_events(rows, extra, device, stream):
    """The tensor [rows + extra, 9] a chip's Global events go to: the kernel writes every word of the first `rows` rows, the `extra`
    rows behind them are the caller's to fill and are zero."""
    events = torch.empty((rows + extra, GLOBAL_EVENT_WORDS), dtype=torch.int32, device=device)
    if extra:
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            events[rows:].zero_()
    return events


def _global_events_ptr(global_events, n):
    """A `global_events` argument checked — None, or an int32 device tensor [n, 9] — as the pointer the entry point takes."""
    if global_events is None:
        return None
    assert global_events.dtype == torch.int32 and tuple(global_events.shape) == (n, GLOBAL_EVENT_WORDS) and global_events.is_contiguous()
    return _dptr(global_events) if n else None


def tracegen_riscv_memory_local(records, height, extra_global_events=0, stream=None):
    """`generate_trace_device` for the MemoryLocal chip (sp1hip_tracegen_riscv_memory_local): records = a device int64 tensor [n, 5]
    of the executor's local-memory records (riscv_exec.ExecutedShard.local: addr, initial clk, initial value, final clk, final
    value). Returns (the column-major [20][height] table as a ColMajor, the rows' Global events: an int32 device tensor
    [2 n + extra_global_events, 9] in the form tracegen_riscv_global reads, record i at rows 2 i and 2 i + 1; the
    `extra_global_events` rows behind them are the caller's to fill — SyscallCore's events — and are zero)."""
    n = _n_records(records, MEMORY_LOCAL_RECORD_WORDS)
    out = device_words(MEMORY_LOCAL_WIDTH * int(height))
    events = _new_global_events(2 * n, int(extra_global_events), out.device, stream)
    check(_L().sp1hip_tracegen_riscv_memory_local(_dptr(out), int(height), _dptr(records) if n else None, n, _dptr(events) if n else None,
                                                  _stream_ptr(stream)))
    return ColMajor(out, int(height), MEMORY_LOCAL_WIDTH), events


MEMORY_GLOBAL_RECORD_WORDS, MEMORY_GLOBAL_WIDTH = 3, 30
MEMORY_GLOBAL_KINDS = {"init": 0, "finalize": 1}


def tracegen_riscv_memory_global(kind, records, height, previous_addr, extra_global_events=0, stream=None):
    """`generate_trace_device` for the MemoryGlobalInit (kind "init") / MemoryGlobalFinalize ("finalize") chip
    (sp1hip_tracegen_riscv_memory_global): records = a device int64 tensor [n, 3] { addr, value, timestamp } in strictly increasing
    address order (not checked here: a list that does not increase makes a row whose constraints fail), previous_addr = the last
    address of the previous memory shard's chip (0 for the first). Returns (the column-major [30][height] table as a ColMajor, the
    rows' Global events: an int32 device tensor [n + extra_global_events, 9] in the form tracegen_riscv_global reads, record i at
    row i — Init sends at timestamp zero, Finalize receives at the record's; the `extra_global_events` rows behind them are the
    caller's to fill and are zero)."""
    n = _n_records(records, MEMORY_GLOBAL_RECORD_WORDS)
    out = device_words(MEMORY_GLOBAL_WIDTH * int(height))
    events = _new_global_events(n, int(extra_global_events), out.device, stream)
    check(_L().sp1hip_tracegen_riscv_memory_global(MEMORY_GLOBAL_KINDS[kind], _dptr(out), int(height), _dptr(records) if n else None, n,
                                                   int(previous_addr) & ((1 << 64) - 1), _dptr(events) if n else None, _stream_ptr(stream)))
    return ColMajor(out, int(height), MEMORY_GLOBAL_WIDTH), events


SYSCALL_PRECOMPILE_WIDTH = 10
# kind: (u64 words per event record, syscall id, the event word of the second pointer or -1, the segments of
# sp1hip_precompile_local_records: (ptr_word, count, pairs_word, final_word or None, final_clk_delta)) — what the host builders
# riscv_more_trace.precompile_shard_from / secp256k1_add_shard_from / secp256k1_double_shard_from hand _close_precompile_shard
PRECOMPILE_DESCRIPTORS = {"keccak": (77, 0x09, -1, ((1, 25, 2, 52, 1),)),
                          "secp256k1_add": (43, 0x0A, 2, ((1, 8, 3, 35, 1), (2, 8, 19, None, 0))),
                          "secp256k1_double": (26, 0x0B, -1, ((1, 8, 2, 18, 0),))}


def tracegen_riscv_syscall_precompile(events, height, syscall_id, arg2_word=-1, global_events=None, stream=None):
    """`generate_trace_device` for the SyscallPrecompile chip (sp1hip_tracegen_riscv_syscall_precompile): events = a device int64 tensor
    [n, words] of a precompile's event records as the executor leaves them (word 0 the clk, word 1 the first pointer, word
    `arg2_word` the second or -1). Returns the column-major [10][height] table as a ColMajor, one row per call. `global_events`: an
    int32 device tensor [n, 9] that receives the rows' Global events — receives of kind Syscall — in the form tracegen_riscv_global
    reads: the tail tracegen_riscv_memory_local leaves for them; or None."""
    n = _n_records(events)
    d_global_events = _global_events_ptr(global_events, n)
    out = device_words(SYSCALL_PRECOMPILE_WIDTH * int(height))
    check(_L().sp1hip_tracegen_riscv_syscall_precompile(_dptr(out), int(height), _dptr(events) if n else None, n, int(events.shape[1]), int(syscall_id),
                                                        int(arg2_word), d_global_events, _stream_ptr(stream)))
    return ColMajor(out, int(height), SYSCALL_PRECOMPILE_WIDTH)


def precompile_local_records(events, segments, stream=None):
    """The MemoryLocal records of the words a precompile's calls touched (sp1hip_precompile_local_records): events = a device int64
    tensor [n, words] of event records, segments = up to four (ptr_word, count, pairs_word, final_word or None, final_clk_delta) —
    PRECOMPILE_DESCRIPTORS has those of Keccak and secp256k1, SHA_DESCRIPTORS those of SHA-256 (final_word PRECOMPILE_QUAD_WORDS: the
    quad form). Returns a device int64 tensor [n * sum of counts, 5] { addr, initial
    clk, initial value, final clk, final value }, segment after segment, event by event inside each: what tracegen_riscv_memory_local
    reads."""
    n = int(events.shape[0])
    assert events.dtype == torch.int64 and events.dim() == 2 and (n == 0 or (events.is_cuda and events.is_contiguous()))
    flat = np.array([[p, c, q, 0xFFFFFFFF if f is None else f, d] for p, c, q, f, d in segments], dtype=np.uint32).reshape(-1)
    total = n * sum(int(s[1]) for s in segments)
    device = events.device if events.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        out = torch.empty((total, MEMORY_LOCAL_RECORD_WORDS), dtype=torch.int64, device=device)
    check(_L().sp1hip_precompile_local_records(_dptr(out) if total else None, total, _dptr(events) if n else None, n, int(events.shape[1]),
                                               flat.ctypes.data_as(C.POINTER(C.c_uint32)), len(segments), _stream_ptr(stream)))
    return out


RV64_EVENT_WORDS = 20                                                              # the executor's record (ExecutedShard.events)
RV64_BINS = tuple(RISCV_ALU_CHIPS) + tuple(RISCV_MEM_CHIPS) + ("DivRem", "AluX0", "SyscallInstrs", "SyscallCore", "StateBump", "MemoryBump")
RV64_BIN_WORDS = (ALU_EVENT_WORDS,) * 14 + (MEM_EVENT_WORDS,) * 9 + (ALU_EVENT_WORDS,) * 4 + (4, 4)    # u64 words of a bin's record


def partition_rv64_events(events, stream=None):
    """The stable partition of a core shard's executed instructions on the device (sp1hip_rv64_partition_count / _scatter): events = a
    device int64 tensor [n, 20], the executor's records as ExecutedShard.events holds them. Returns {bin name: int64 tensor [count,
    words]} for the 29 bins of RV64_BINS — the chips' record streams in execution order, ready for tracegen_riscv_alu / _mem / _divrem /
    _alu_x0 / _syscall_instrs / _syscall_core / _state_bump / _memory_bump — all views of one arena sized exactly. Between the two
    calls the 29 counts are read back (116 bytes): they decide the tables' heights."""
    n = int(events.shape[0])
    assert events.dtype == torch.int64 and (n == 0 or (events.is_cuda and events.shape[1] == RV64_EVENT_WORDS and events.is_contiguous()))
    L, sp = _L(), _stream_ptr(stream)
    device = events.device if n else torch.device("cuda", torch.cuda.current_device())
    if n == 0:
        return {name: torch.empty((0, w), dtype=torch.int64, device=device) for name, w in zip(RV64_BINS, RV64_BIN_WORDS)}
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        scratch = torch.empty(int(L.sp1hip_rv64_partition_scratch_bytes(n)) // 4, dtype=torch.int32, device=device)
        d_counts = torch.empty(32, dtype=torch.int32, device=device)
        check(L.sp1hip_rv64_partition_count(_dptr(events), n, _dptr(scratch), _dptr(d_counts), sp))
        counts = [int(c) for c in d_counts[:len(RV64_BINS)].cpu()]          # synchronises the stream
        total = sum(c * w for c, w in zip(counts, RV64_BIN_WORDS))
        arena = torch.empty(total, dtype=torch.int64, device=device)
        check(L.sp1hip_rv64_partition_scatter(_dptr(events), n, _dptr(scratch), _dptr(d_counts), _dptr(arena) if total else None, total, sp))
    out, at = {}, 0
    for name, c, w in zip(RV64_BINS, counts, RV64_BIN_WORDS):
        out[name] = arena[at:at + c * w].view(c, w)
        at += c * w
    return out


def tracegen_riscv_syscall_instrs(events, height, stream=None):
    """`generate_trace_device` for the SyscallInstrs chip (sp1hip_tracegen_riscv_syscall_instrs): events = a device int64 tensor [n, 11]
    of the ECALLs' sp1hip_rv64_alu_event_t records (bin "SyscallInstrs" of partition_rv64_events); returns the column-major
    [65][height] table as a ColMajor, zero padding rows."""
    return tracegen_riscv_records("SyscallInstrs", events, height, stream)


def tracegen_riscv_syscall_core(events, height, global_events=None, stream=None):
    """The same for the SyscallCore chip (bin "SyscallCore"): column-major [10][height]. `global_events`: an int32 device tensor
    [n, 9] that receives the rows' Global events in the form tracegen_riscv_global reads — the tail tracegen_riscv_memory_local leaves
    for them — or None."""
    width = _L().sp1hip_tracegen_riscv_syscall_core_width()
    n = _n_records(events, ALU_EVENT_WORDS)
    d_global_events = _global_events_ptr(global_events, n)
    out = device_words(width * int(height))
    check(_L().sp1hip_tracegen_riscv_syscall_core(_dptr(out), int(height), _dptr(events) if n else None, n, d_global_events, _stream_ptr(stream)))
    return ColMajor(out, int(height), width)


BUMP_RECORD_WORDS = 4                                                               # the StateBump / MemoryBump bins' records


def tracegen_riscv_state_bump(records, height, stream=None):
    """`generate_trace_device` for the StateBump chip (sp1hip_tracegen_riscv_state_bump): records = a device int64 tensor [n, 4] (clk, pc,
    next_pc, clock step | pc_carry << 32: bin "StateBump"); column-major [14][height], zero padding rows."""
    return tracegen_riscv_records("StateBump", records, height, stream)


def tracegen_riscv_memory_bump(records, height, stream=None):
    """The same for the MemoryBump chip (records: register, previous timestamp, value, window start — bin "MemoryBump"):
    column-major [15][height]."""
    return tracegen_riscv_records("MemoryBump", records, height, stream)


KECCAK_EVENT_WORDS = 77                                                            # SP1HIP_RV64_KECCAK_WORDS


def tracegen_riscv_keccak(events, height, stream=None):
    """`generate_trace_device` for the KeccakPermute chip (sp1hip_tracegen_riscv_keccak): events = a device int64 tensor [n, 77]
    of the executor's KECCAK_PERMUTE records (riscv_exec.ExecutedShard.keccak); 24 rows per event, height >= 24 n. Returns the
    column-major [2640][height] table as a ColMajor."""
    return tracegen_riscv_records("KeccakPermute", events, height, stream)


def tracegen_riscv_keccak_control(events, height, stream=None):
    """The same events' KeccakPermuteControl table (sp1hip_tracegen_riscv_keccak_control): one row per event, height >= n;
    column-major [634][height]."""
    return tracegen_riscv_records("KeccakPermuteControl", events, height, stream)


SECP_ADD_EVENT_WORDS, SECP_DOUBLE_EVENT_WORDS = 43, 26                              # SP1HIP_RV64_SECP_ADD_WORDS, _DOUBLE_WORDS


def tracegen_riscv_secp256k1_add(events, height, stream=None):
    """`generate_trace_device` for the Secp256k1AddAssign chip (sp1hip_tracegen_riscv_secp256k1_add): events = a device int64 tensor
    [n, 43] of the executor's SECP256K1_ADD records (riscv_exec.ExecutedShard.secp256k1_add); one row per event, height >= n,
    padding rows = the reference's dummy row. Returns the column-major [1599][height] table as a ColMajor."""
    return tracegen_riscv_records("Secp256k1AddAssign", events, height, stream)


def tracegen_riscv_secp256k1_double(events, height, stream=None):
    """The same for the Secp256k1DoubleAssign chip (sp1hip_tracegen_riscv_secp256k1_double): events int64 [n, 26]
    (ExecutedShard.secp256k1_double); column-major [1591][height]."""
    return tracegen_riscv_records("Secp256k1DoubleAssign", events, height, stream)


SHA_EXTEND_EVENT_WORDS, SHA_COMPRESS_EVENT_WORDS = 786, 155                        # SP1HIP_RV64_SHA_EXTEND_WORDS, _SHA_COMPRESS_WORDS
# final_word of a segment of sp1hip_precompile_local_records in the quad form: event words pairs_word + 4 i .. + 4 i + 3 hold word i's
# initial timestamp, initial value, final timestamp and final value (the words of one SHA_EXTEND call end at different timestamps)
PRECOMPILE_QUAD_WORDS = 0xFFFFFFFE
# the SHA-256 kinds in the shape of PRECOMPILE_DESCRIPTORS — what riscv_more_trace.sha_extend_shard_from / sha_compress_shard_from hand
# _close_precompile_shard: SHA_EXTEND's 64 words of w in the quad form; SHA_COMPRESS's 8 words of h (written at clk + 2), then its
# 64 words of w (read at clk + 1), arg2 = h_ptr
SHA_DESCRIPTORS = {"sha_extend": (SHA_EXTEND_EVENT_WORDS, 0x05, -1, ((1, 64, 530, PRECOMPILE_QUAD_WORDS, 0),)),
                   "sha_compress": (SHA_COMPRESS_EVENT_WORDS, 0x06, 2, ((2, 8, 3, 147, 2), (1, 64, 19, None, 1)))}


def tracegen_riscv_sha_extend(events, height, stream=None):
    """`generate_trace_device` for the ShaExtend chip (sp1hip_tracegen_riscv_sha_extend): events = a device int64 tensor [n, 786] of the
    executor's SHA_EXTEND records (riscv_exec.ExecutedShard.sha_extend); 48 rows per event, height >= 48 n, zero padding rows. Returns
    the column-major [128][height] table as a ColMajor."""
    return tracegen_riscv_records("ShaExtend", events, height, stream)


def tracegen_riscv_sha_extend_control(events, height, stream=None):
    """The same events' ShaExtendControl table (sp1hip_tracegen_riscv_sha_extend_control): one row per event, height >= n;
    column-major [18][height]."""
    return tracegen_riscv_records("ShaExtendControl", events, height, stream)


def tracegen_riscv_sha_compress(events, height, stream=None):
    """`generate_trace_device` for the ShaCompress chip (sp1hip_tracegen_riscv_sha_compress): events = a device int64 tensor [n, 155] of
    the executor's SHA_COMPRESS records (ExecutedShard.sha_compress); 80 rows per event, height >= 80 n. Padding rows keep octet,
    octet_num, index and k cycling by row mod 80 and are zero elsewhere. Returns the column-major [206][height] table as a ColMajor."""
    return tracegen_riscv_records("ShaCompress", events, height, stream)


def tracegen_riscv_sha_compress_control(events, height, stream=None):
    """The same events' ShaCompressControl table (sp1hip_tracegen_riscv_sha_compress_control): one row per event, height >= n;
    column-major [53][height]."""
    return tracegen_riscv_records("ShaCompressControl", events, height, stream)


POSEIDON2_EVENT_WORDS, UINT256_EVENT_WORDS = 26, 31                                # SP1HIP_RV64_POSEIDON2_WORDS, _UINT256_WORDS
# the POSEIDON2 and UINT256_MUL kinds in the shape of PRECOMPILE_DESCRIPTORS — what riscv_more_trace.poseidon2_shard_from /
# uint256_shard_from hand _close_precompile_shard: POSEIDON2's 8 words rewritten in place at clk; UINT256_MUL's 4 words of x (written at
# clk + 1), then the 8 words of y and the modulus (read at clk), arg2 = y_ptr
WORD_DESCRIPTORS = {"poseidon2": (POSEIDON2_EVENT_WORDS, 0x33, -1, ((1, 8, 2, 18, 0),)),
                    "uint256": (UINT256_EVENT_WORDS, 0x1D, 2, ((1, 4, 3, 27, 1), (2, 8, 11, None, 0)))}


def tracegen_riscv_poseidon2(events, height, stream=None):
    """`generate_trace_device` for the Poseidon2 chip (sp1hip_tracegen_riscv_poseidon2): events = a device int64 tensor [n, 26] of the
    executor's POSEIDON2 records (riscv_exec.ExecutedShard.poseidon2); one row per event, height >= n; a padding row is zero except for
    the permutation of the zero state. Returns the column-major [348][height] table as a ColMajor."""
    return tracegen_riscv_records("Poseidon2", events, height, stream)


def tracegen_riscv_uint256_mul(events, height, stream=None):
    """`generate_trace_device` for the Uint256MulMod chip (sp1hip_tracegen_riscv_uint256_mul): events = a device int64 tensor [n, 31] of
    the executor's UINT256_MUL records (ExecutedShard.uint256); one row per event, height >= n; a padding row is zero except for the
    witness offset. Returns the column-major [371][height] table as a ColMajor."""
    return tracegen_riscv_records("Uint256MulMod", events, height, stream)


FAMILY_CODE_WORD = 3                                                               # the system-call code's word of a family event
# kind: (SP1HIP_RV64_FAMILY_*, u64 words per operand, operands, syscall id or None) — the twelve field / curve precompile kinds of
# riscv_exec.FAMILIES with a device filler (sp1hip_tracegen_riscv_field_chip). None: the shard mixes system calls (Fp: ADD, SUB, MUL;
# Fp2: ADD, SUB) and each row's id is its event's own (tracegen_riscv_syscall_precompile_coded, word FAMILY_CODE_WORD)
FIELD_CHIP_KINDS = {"secp256r1_add": (0, 8, 2, 0x2C), "secp256r1_double": (1, 8, 1, 0x2D), "bn254_add": (2, 8, 2, 0x0E), "bn254_double": (3, 8, 1, 0x0F),
                    "bls12381_add": (4, 12, 2, 0x1E), "bls12381_double": (5, 12, 1, 0x1F), "bn254_fp": (6, 4, 2, None), "bls12381_fp": (7, 6, 2, None),
                    "bn254_fp2_addsub": (8, 8, 2, None), "bls12381_fp2_addsub": (9, 12, 2, None), "bn254_fp2_mul": (10, 8, 2, 0x2B),
                    "bls12381_fp2_mul": (11, 12, 2, 0x25)}


def _family_descriptor(nw, operands, syscall_id):
    """A family event is clk, arg1, arg2, code, `nw` (previous timestamp, word) pairs per operand, `nw` words written: two operands
    — x rewritten at clk + 1, y read at clk, arg2 = y's pointer — or one, rewritten in place at clk."""
    if operands == 2:
        return (4 + 5 * nw, syscall_id, 2, ((1, nw, 4, 4 + 4 * nw, 1), (2, nw, 4 + 2 * nw, None, 0)))
    return (4 + 3 * nw, syscall_id, -1, ((1, nw, 4, 4 + 2 * nw, 0),))


# the same kinds in the shape of PRECOMPILE_DESCRIPTORS — what riscv_more_trace.family_shard_from hands _close_precompile_shard
FAMILY_DESCRIPTORS = {kind: _family_descriptor(nw, operands, syscall_id) for kind, (_, nw, operands, syscall_id) in FIELD_CHIP_KINDS.items()}


def tracegen_riscv_field_chip(kind, events, height, stream=None):
    """`generate_trace_device` for the chip of a field / curve precompile kind of FIELD_CHIP_KINDS (sp1hip_tracegen_riscv_field_chip):
    events = a device int64 tensor [n, FAMILY_DESCRIPTORS[kind][0]] of the executor's records of that family
    (riscv_exec.ExecutedShard.precompile_events); one row per event, height >= n, padding rows = the reference's dummy row. The
    call's work buffer is allocated and released inside it, on the stream. Returns the column-major [width][height] table as a ColMajor."""
    if kind not in FIELD_CHIP_KINDS:
        raise ValueError("no device filler for a %r chip: tracegen_riscv_field_chip makes %s" % (kind, ", ".join(FIELD_CHIP_KINDS)))
    return _tracegen_records("sp1hip_tracegen_riscv_field_chip", FAMILY_DESCRIPTORS[kind][0], FIELD_CHIP_KINDS[kind][0], events, height, stream)


def tracegen_riscv_syscall_precompile_coded(events, height, code_word=FAMILY_CODE_WORD, arg2_word=-1, global_events=None, stream=None):
    """tracegen_riscv_syscall_precompile for a shard that mixes system calls (sp1hip_tracegen_riscv_syscall_precompile_coded): each
    row's syscall id is the low byte of its event's word `code_word`."""
    n = _n_records(events)
    d_global_events = _global_events_ptr(global_events, n)
    out = device_words(SYSCALL_PRECOMPILE_WIDTH * int(height))
    check(_L().sp1hip_tracegen_riscv_syscall_precompile_coded(_dptr(out), int(height), _dptr(events) if n else None, n, int(events.shape[1]), int(code_word),
                                                              int(arg2_word), d_global_events, _stream_ptr(stream)))
    return ColMajor(out, int(height), SYSCALL_PRECOMPILE_WIDTH)


ED_ADD_EVENT_WORDS, ED_DECOMPRESS_EVENT_WORDS, UINT256_OPS_EVENT_WORDS = 44, 24, 58     # FAMILY_WORDS of rv64_exec.cpp, families 12..14
# the last three kinds of riscv_exec.FAMILIES, which tracegen_riscv_field_chip does not make, in the shape of PRECOMPILE_DESCRIPTORS
# except for the last entry: the MemoryLocal segments of precompile_local_records (ed_add: _family_descriptor's), or the
# SP1HIP_RV64_FAMILY_* that precompile_touched_records takes (ed_decompress: 8 records per call; uint256_ops: 23, and each row's
# syscall id is its event's own: None). arg2 is word 2: ED_ADD's second pointer, ED_DECOMPRESS' sign bit, the carry calls' b pointer
FAMILY_REST_DESCRIPTORS = {"ed_add": _family_descriptor(8, 2, 0x07), "ed_decompress": (ED_DECOMPRESS_EVENT_WORDS, 0x08, 2, 13),
                           "uint256_ops": (UINT256_OPS_EVENT_WORDS, None, 2, 14)}
TOUCHED_RECORDS_PER_CALL = {13: 8, 14: 23}


def tracegen_riscv_ed_add(events, height, stream=None):
    """`generate_trace_device` for the EdAddAssign chip (sp1hip_tracegen_riscv_ed_add): events = a device int64 tensor [n, 44] of the
    executor's ED_ADD records (family "ed_add" of riscv_exec.ExecutedShard.precompile_events); one row per event, height >= n, padding
    rows = the reference's dummy row. The call's work buffer is allocated and released inside it, on the stream. Returns the
    column-major [1347][height] table as a ColMajor."""
    return tracegen_riscv_records("EdAddAssign", events, height, stream)


def tracegen_riscv_ed_decompress(events, height, stream=None):
    """The same for the EdDecompress chip (sp1hip_tracegen_riscv_ed_decompress): events int64 [n, 24] (family "ed_decompress");
    column-major [1123][height]."""
    return tracegen_riscv_records("EdDecompress", events, height, stream)


def tracegen_riscv_uint256_ops(events, height, stream=None):
    """The same for the Uint256Ops chip (sp1hip_tracegen_riscv_uint256_ops): events int64 [n, 58] (family "uint256_ops": UINT256_ADD_CARRY
    and UINT256_MUL_CARRY calls, told apart by the low byte of word 3); column-major [477][height]; a padding row is zero except for
    the witness offset."""
    return tracegen_riscv_records("Uint256Ops", events, height, stream)


def precompile_touched_records(events, family, stream=None):
    """The MemoryLocal records of the words the calls of an ed_decompress (family 13) or a uint256_ops (14) shard touched
    (sp1hip_precompile_touched_records): events = a device int64 tensor [n, 24 / 58]. Returns a device int64 tensor [n * 8 / 23, 5]
    { addr, initial clk, initial value, final clk, final value }, run after run, event by event inside each: what
    riscv_more_trace.family_shard_from hands _close_precompile_shard, and what tracegen_riscv_memory_local reads."""
    if family not in TOUCHED_RECORDS_PER_CALL:
        raise ValueError("precompile_touched_records makes the records of family 13 (ed_decompress) and 14 (uint256_ops), not of %r" % (family,))
    n = int(events.shape[0])
    words = FAMILY_REST_DESCRIPTORS["ed_decompress" if family == 13 else "uint256_ops"][0]
    assert events.dtype == torch.int64 and events.dim() == 2 and events.shape[1] == words and (n == 0 or (events.is_cuda and events.is_contiguous()))
    total = n * TOUCHED_RECORDS_PER_CALL[family]
    device = events.device if events.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        out = torch.empty((total, MEMORY_LOCAL_RECORD_WORDS), dtype=torch.int64, device=device)
    check(_L().sp1hip_precompile_touched_records(_dptr(out) if total else None, total, _dptr(events) if n else None, n, int(family), _stream_ptr(stream)))
    return out


# chip: (entry point, u64 words of a record, leading chip argument or None) — every chip whose table is made from its record stream
# alone, the wrappers above by chip name (MemoryLocal, MemoryGlobal*, SyscallCore and SyscallPrecompile also write Global events)
RISCV_TRACEGEN = {**{c: ("sp1hip_tracegen_riscv_alu", ALU_EVENT_WORDS, k) for c, k in RISCV_ALU_CHIPS.items()},
                  **{c: ("sp1hip_tracegen_riscv_mem", MEM_EVENT_WORDS, k) for c, k in RISCV_MEM_CHIPS.items()},
                  "DivRem": ("sp1hip_tracegen_riscv_divrem", ALU_EVENT_WORDS, None), "AluX0": ("sp1hip_tracegen_riscv_alu_x0", ALU_EVENT_WORDS, None),
                  "SyscallInstrs": ("sp1hip_tracegen_riscv_syscall_instrs", ALU_EVENT_WORDS, None),
                  "StateBump": ("sp1hip_tracegen_riscv_state_bump", BUMP_RECORD_WORDS, None),
                  "MemoryBump": ("sp1hip_tracegen_riscv_memory_bump", BUMP_RECORD_WORDS, None),
                  "KeccakPermute": ("sp1hip_tracegen_riscv_keccak", KECCAK_EVENT_WORDS, None),
                  "KeccakPermuteControl": ("sp1hip_tracegen_riscv_keccak_control", KECCAK_EVENT_WORDS, None),
                  "Secp256k1AddAssign": ("sp1hip_tracegen_riscv_secp256k1_add", SECP_ADD_EVENT_WORDS, None),
                  "Secp256k1DoubleAssign": ("sp1hip_tracegen_riscv_secp256k1_double", SECP_DOUBLE_EVENT_WORDS, None),
                  "ShaExtend": ("sp1hip_tracegen_riscv_sha_extend", SHA_EXTEND_EVENT_WORDS, None),
                  "ShaExtendControl": ("sp1hip_tracegen_riscv_sha_extend_control", SHA_EXTEND_EVENT_WORDS, None),
                  "ShaCompress": ("sp1hip_tracegen_riscv_sha_compress", SHA_COMPRESS_EVENT_WORDS, None),
                  "ShaCompressControl": ("sp1hip_tracegen_riscv_sha_compress_control", SHA_COMPRESS_EVENT_WORDS, None),
                  "Poseidon2": ("sp1hip_tracegen_riscv_poseidon2", POSEIDON2_EVENT_WORDS, None),
                  "Uint256MulMod": ("sp1hip_tracegen_riscv_uint256_mul", UINT256_EVENT_WORDS, None),
                  "EdAddAssign": ("sp1hip_tracegen_riscv_ed_add", ED_ADD_EVENT_WORDS, None),
                  "EdDecompress": ("sp1hip_tracegen_riscv_ed_decompress", ED_DECOMPRESS_EVENT_WORDS, None),
                  "Uint256Ops": ("sp1hip_tracegen_riscv_uint256_ops", UINT256_OPS_EVENT_WORDS, None)}


def tracegen_riscv_records(chip, records, height, stream=None):
    """The table of a chip of RISCV_TRACEGEN from its record stream (a device int64 tensor [n, words]): the wrapper of that chip."""
    return _tracegen_records(*RISCV_TRACEGEN[chip], records, height, stream)


class LookupCounter:
    """The Byte, Range and Program main tables of one shard — the multiplicities of the byte lookups every other table sends and
    of the executed pcs — counted on the device (sp1hip_lookup_count_sends / _program / _counts_finish): the reference's
    `generate_dependencies` of its Byte and Range chips over tables that are already in device memory. One u32 count buffer holds
    the three arrays back to back: [6][65536] Byte, [131072] Range, [program_height] Program; the calls enqueue on `stream`, and
    finish() converts the buffer to Montgomery words in place and hands out the three tables as views of it."""
    BYTE_CELLS, RANGE_CELLS, STATUS_WORDS = 6 << 16, 1 << 17, 8

    def __init__(self, program_height=0, stream=None):
        self.stream, self.program_height = stream, int(program_height)
        device = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):    # zeroed on the stream that counts
            self.counts = torch.zeros(self.BYTE_CELLS + self.RANGE_CELLS + self.program_height, dtype=torch.int32, device=device)
            self.status = torch.zeros(self.STATUS_WORDS, dtype=torch.int32, device=device)
        self.calls = []                                   # the name of every add, by tag: what an error message's "call" means
        self._keep = []                                   # inputs uploaded here stay alive until finish() has synchronised
        self.finished = False                             # finish() turns the counts into field elements: nothing may be added after

    def _open(self):
        if self.finished:
            raise RuntimeError("this LookupCounter is finished: its buffer holds Montgomery words, not counts")

    def _parts(self):
        b, r = self.BYTE_CELLS, self.BYTE_CELLS + self.RANGE_CELLS
        return self.counts[:b], self.counts[b:r], self.counts[r:]

    def add(self, interaction_program, main, prep=None):
        """Count the byte sends of a chip (air.InteractionProgram) over all rows of its tables (ColMajor; prep None for none)."""
        self._open()
        words = np.ascontiguousarray(interaction_program.to_array(), dtype=np.uint32)
        rows = main.height if main is not None else 0
        assert prep is None or prep.height == rows or rows == 0
        byte, rng, _ = self._parts()
        self.calls.append(interaction_program.name)
        check(_L().sp1hip_lookup_count_sends(words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size, main.width if main is not None else 0,
                                             prep.width if prep is not None else 0, _dptr(main.words) if main is not None and rows else None,
                                             _dptr(prep.words) if prep is not None and rows else None, rows, _dptr(byte), _dptr(rng),
                                             _dptr(self.status), len(self.calls) - 1, _stream_ptr(self.stream)))

    def add_row(self, interaction_program, row_words):
        """The same for one row given on the host (the public values' sends): Montgomery words, uploaded as a 1-row table."""
        row = np.ascontiguousarray(row_words, dtype=np.uint32).reshape(-1)
        table = ColMajor(to_device(row), 1, row.size)
        self._keep.append(table)
        self.add(interaction_program, table)

    def add_program_counters(self, events_or_pcs, pc_base, n_instructions):
        """Count executed pcs into the Program table: an int64 [n, k] matrix whose column 0 is the pc (the executor's [n, 20] events,
        the packed 11- / 12-word records) or a 1-D int64 array of pcs; numpy (uploaded) or a device tensor."""
        self._open()
        ev = events_or_pcs
        if not torch.is_tensor(ev):
            ev = torch.as_tensor(np.ascontiguousarray(ev, dtype=np.int64))
        assert ev.dtype == torch.int64 and ev.dim() in (1, 2) and int(n_instructions) <= self.program_height
        if not ev.is_cuda:
            ev = (ev if ev.dim() == 1 else ev[:, 0]).contiguous().to(self.counts.device)      # only the pcs cross
        n = int(ev.shape[0])
        stride = 1 if ev.dim() == 1 else int(ev.stride(0))
        assert n == 0 or (ev.dim() == 1 and ev.is_contiguous()) or ev.stride(1) == 1
        self._keep.append(ev)
        self.calls.append("Program")
        check(_L().sp1hip_lookup_count_program(_dptr(ev) if n else None, max(stride, 1), n, int(pc_base), int(n_instructions),
                                               _dptr(self._parts()[2]), _dptr(self.status), len(self.calls) - 1, _stream_ptr(self.stream)))

    def finish(self):
        """{"Byte": ColMajor 65536 x 6, "Range": ColMajor 131072 x 1, "Program": ColMajor program_height x 1}. Synchronises the
        stream; raises Sp1HipError naming the first bad message (its send and row, and the add it came from) if there was one. Once:
        the counter takes no further call, also after an error."""
        self._open()
        self.finished = True
        try:
            check(_L().sp1hip_lookup_counts_finish(_dptr(self.counts), self.counts.numel(), None, _dptr(self.status), _stream_ptr(self.stream)))
        except _lib.Sp1HipError as e:
            st = to_host(self.status)
            if int(st[1]) in (1, 2) and int(st[4]) < len(self.calls):
                e.args = ("%s (call %d is %s)" % (e.args[0], int(st[4]), self.calls[int(st[4])]),)
            raise
        finally:
            self._keep.clear()
        byte, rng, prog = self._parts()
        return {"Byte": ColMajor(byte, 1 << 16, 6), "Range": ColMajor(rng, 1 << 17, 1), "Program": ColMajor(prog, self.program_height, 1)}


def check_constraints(chips, public_values, stream=None):
    """Every constraint of every chip on every row, on the device (sp1hip_check_constraints: the reference's
    `debug_constraints_all_chips`, hypercube/src/debug.rs:L27-L125). chips: the [(AirProgram, InteractionProgram, main ColMajor or
    None, prep ColMajor or None)] of prove_shard; public_values: Montgomery words. No table is copied to the host: per chip one dict
    comes back — name, failing_rows, first_row (None when no row fails), fail_count (uint32 per constraint: the rows on which it is
    non-zero), noncanonical (stored words >= p), first_constraints (the indices non-zero on first_row, at most 64), first_row_main /
    first_row_prep (that row's Montgomery words), pieces / registers / lanes (how the program ran). Synchronises the stream."""
    arr, keep = _shard_chip_array(chips)
    pv = np.ascontiguousarray(np.asarray(public_values, dtype=np.uint32).reshape(-1))
    reports = np.zeros((max(len(chips), 1), _lib.CHECK_REPORT_WORDS), dtype=np.uint64)
    n = C.c_size_t(sum(a.num_constraints + a.main_width + a.prep_width for a, _, _, _ in chips))
    words = np.zeros(max(n.value, 1), dtype=np.uint32)
    check(_L().sp1hip_check_constraints(arr, len(chips), pv.ctypes.data_as(_lib.u32p) if pv.size else None, int(pv.size),
                                        reports.ctypes.data_as(C.POINTER(C.c_uint64)), words.ctypes.data_as(_lib.u32p), C.byref(n), _stream_ptr(stream)))
    out = []
    for (air, _, _, _), r in zip(chips, reports.tolist()):
        failing_rows, first_row, noncanonical, fc, row, pieces, registers, lanes, n_first = r[:9]
        failed = failing_rows != 0
        out.append({"name": air.name, "failing_rows": failing_rows, "first_row": first_row if failed else None,
                    "fail_count": words[fc:fc + air.num_constraints].copy(), "noncanonical": noncanonical,
                    "first_constraints": r[9:9 + n_first],
                    "first_row_main": words[row:row + air.main_width].copy() if failed else None,
                    "first_row_prep": words[row + air.main_width:row + air.main_width + air.prep_width].copy() if failed and air.prep_width else None,
                    "pieces": pieces, "registers": registers, "lanes": lanes})
    return out


def check_interactions(chips, cap=1 << 16, log_buckets=22, stream=None):
    """Do the sends and receives of the chips cancel, bus by bus (sp1hip_check_interactions: the reference's
    `debug_interactions_with_all_chips`, hypercube/src/lookup/debug.rs:L48-L200)? chips: the tuples of check_constraints, with the
    machine's eval_public_values appended by the caller as one more chip over a one-row table (riscv_exec.check_device_shard does).
    The device tallies signed multiplicities in two tables of 2^log_buckets buckets under two independent hashes and names, in at
    most `cap` records, the messages whose bucket of the first table does not cancel; this function fetches the rows those records
    name (and no other cell of any table), evaluates their messages with VCol.apply and sums them exactly. Returns {"balanced",
    "truncated", "messages", "nonzero_buckets", "records_wanted", "records" (uint32 [n, 4]: chip, interaction, row, canonical
    multiplicity), "imbalance": {(kind, values...): discrepancy mod p} over the keys that do not cancel}. When nothing was truncated
    the imbalance is the whole truth: balanced keys that merely share a bucket cancel in the exact tally and drop out."""
    arr = (ShardChip * max(len(chips), 1))()
    keep = []
    for i, (_, inter, main, prep) in enumerate(chips):         # the widths are the InteractionProgram's (eval_public_values' AirProgram has no columns)
        words = np.ascontiguousarray(inter.to_array(), dtype=np.uint32)
        keep.append(words)
        rows = main.height if main is not None else 0
        assert rows == 0 or (main.width == inter.main_width and (prep.width if prep is not None else 0) == inter.prep_width), inter.name
        arr[i] = ShardChip(inter.name.encode(), None, 0, 0, words.ctypes.data_as(_lib.u32p), words.size, inter.main_width, inter.prep_width,
                           C.c_void_p(main.words.data_ptr()) if rows and inter.main_width else None,
                           C.c_void_p(prep.words.data_ptr()) if prep is not None and rows and inter.prep_width else None, rows)
    report = np.zeros(_lib.CHECK_BUSES_WORDS, dtype=np.uint64)
    records = np.zeros((max(int(cap), 1), 4), dtype=np.uint32)
    check(_L().sp1hip_check_interactions(arr, len(chips), int(log_buckets), report.ctypes.data_as(C.POINTER(C.c_uint64)), records.ctypes.data_as(_lib.u32p), int(cap),
                                        _stream_ptr(stream)))
    messages, nonzero_a, nonzero_b, records_wanted, n_records, balanced, truncated = report.tolist()[:7]
    records = records[:n_records]
    tally = {}
    r_inv = pow(1 << 32, -1, P)
    for ci in np.unique(records[:, 0]):
        _, it, main, prep = chips[int(ci)]
        mine = records[records[:, 0] == ci]
        rows, where = np.unique(mine[:, 2], return_inverse=True)
        index = torch.as_tensor(rows.astype(np.int64), device=main.words.device)

        def fetch(t):                                          # the named rows of a column-major table, canonical, [n][width]
            if t is None or t.width == 0:
                return np.zeros((len(rows), 0), dtype=np.uint64)
            got = t.words.view(t.width, t.height).index_select(1, index).cpu().numpy().view(np.uint32).astype(np.uint64)
            return (got * np.uint64(r_inv) % np.uint64(P)).T

        main_rows, prep_rows = fetch(main), fetch(prep)
        both = [(1, x) for x in it.sends] + [(-1, x) for x in it.receives]
        for (_, k, _, m), w in zip(mine.tolist(), where.tolist()):
            sign, (kind, values, mult) = both[k]
            assert mult.apply(prep_rows[w], main_rows[w]) == m, "a record's multiplicity is not its row's"
            key = (kind,) + tuple(v.apply(prep_rows[w], main_rows[w]) for v in values)
            tally[key] = (tally.get(key, 0) + sign * m) % P
    return {"balanced": bool(balanced), "truncated": bool(truncated), "messages": messages, "nonzero_buckets": (nonzero_a, nonzero_b),
            "records_wanted": records_wanted,
            "records": records, "imbalance": {k: v for k, v in tally.items() if v}}


class ProvingKey:
    """`ProvingKey` of the AirProver slot: the preprocessed commitment round + the verifying key (sp1hip_setup).
    Keeps the preprocessed device tables alive."""

    def __init__(self, prep_tables, max_log_row_count, log_stacking_height, batch_size, pc_start=(0, 0, 0),
                 initial_global_cumulative_sum=(0,) * 14, enable_untrusted_programs=0, log_blowup=2, num_queries=124, pow_bits=16,
                 stream=None):
        self.tables = list(prep_tables)
        self.params = ShardParams(max_log_row_count, log_stacking_height, batch_size, FriConfig(log_blowup, num_queries, pow_bits))
        arr = _table_array(self.tables)
        pc = (C.c_uint32 * 3)(*[int(x) for x in pc_start])
        cum = (C.c_uint32 * 14)(*[int(x) for x in initial_global_cumulative_sum])
        h = C.c_void_p()
        check(_L().sp1hip_setup(arr, len(self.tables), pc, cum, int(enable_untrusted_programs), self.params, C.byref(h),
                                _stream_ptr(stream)))
        self.h = h
        vk = _lib.Vk()
        check(_L().sp1hip_pk_vk(self.h, C.byref(vk)))
        self.vk = vk
        self.preprocessed_commit = np.array(list(vk.preprocessed_commit), dtype=np.uint32)

    def observe_into(self, challenger):
        """MachineVerifyingKey::observe_into."""
        check(_L().sp1hip_vk_observe_into(C.byref(self.vk), challenger.h))

    def prove_shard(self, chips, public_values, pow_witnesses=(), stream=None):
        """AirProver::prove_shard_with_pk from the generated traces on -> bincode(ShardProof)."""
        arr, keep = _shard_chip_array(chips)
        pv = np.ascontiguousarray(np.asarray(public_values, dtype=np.uint32).reshape(-1))
        w = (C.c_uint32 * max(len(pow_witnesses), 1))(*[int(x) for x in pow_witnesses])
        args = [self.h, arr, len(chips), pv.ctypes.data_as(_lib.u32p) if pv.size else None, int(pv.size), w, len(pow_witnesses)]
        # one call in the steady state: the buffer of the previous proof of this key is offered first (the size depends on
        # the shard's shape only); a shard that needs more answers ERROR_BUFFER_TOO_SMALL with the size, before any work
        import threading
        bufs = self.__dict__.setdefault("_proof_bufs", {})            # per calling thread: two threads may prove with one key
        me = threading.get_ident()
        buf = bufs.get(me)
        for _ in range(2):
            n = C.c_size_t(len(buf) if buf is not None else 0)
            st = _L().sp1hip_prove_shard_with_pk(*args, buf, C.byref(n), _stream_ptr(stream))
            if st != _lib.ERROR_BUFFER_TOO_SMALL:
                check(st)
                return C.string_at(buf, n.value)
            buf = bufs[me] = (C.c_uint8 * n.value)()
        check(st)

    def __del__(self):
        if getattr(self, "h", None):
            try:
                _L().sp1hip_pk_free(self.h)
            except TypeError:                    # interpreter shutdown: the module globals are already gone
                pass
            self.h = None


def bb_commit_mles(mles, log_blowup, stream=None):
    """BabyBear `commit_mles` (sp1hip_bb_commit_mles): mles = ColMajor tensors of equal height 2^lg_n holding BabyBear Montgomery
    words. Returns (commitment [8] numpy, codewords [ColMajor], tree words as a device tensor [(2 N - 1) * 8])."""
    lg_n = mles[0].height.bit_length() - 1
    N = mles[0].height << log_blowup
    arr = (Tensor * len(mles))(*[m.as_tensor_struct() for m in mles])
    cws = [device_words(N * m.width) for m in mles]
    ptrs = (C.c_void_p * len(mles))(*[c.data_ptr() for c in cws])
    tree = device_words((2 * N - 1) * 8)
    commit = np.zeros(8, np.uint32)
    check(_L().sp1hip_bb_commit_mles(arr, len(mles), lg_n, log_blowup, ptrs, _dptr(tree), commit.ctypes.data_as(_lib.u32p), _stream_ptr(stream)))
    return commit, [ColMajor(c, N, m.width) for c, m in zip(cws, mles)], tree


def bb_rs_encode_batch(mle, log_blowup, stream=None):
    """BabyBear RS encode of one ColMajor tensor (sp1hip_bb_rs_encode_batch): every column's 2^lg_n coefficients -> its
    2^(lg_n + log_blowup) evaluations in bit-reversed row order, as a new ColMajor."""
    lg_n = mle.height.bit_length() - 1
    N = mle.height << log_blowup
    out = device_words(N * mle.width)
    check(_L().sp1hip_bb_rs_encode_batch(_dptr(out), _dptr(mle.words), lg_n, log_blowup, mle.width, _stream_ptr(stream)))
    return ColMajor(out, N, mle.width)


def bb_merkle_commit(tensors, stream=None):
    """BabyBear `commit_tensors` (sp1hip_bb_merkle_commit) over ColMajor tensors of equal power-of-two height, of any content.
    Returns (commitment [8] numpy, root [8] numpy, tree words as a device tensor [(2 h - 1) * 8], layers leaf-first)."""
    h = tensors[0].height
    tree = device_words((2 * h - 1) * 8)
    rc = device_words(16)
    check(_L().sp1hip_bb_merkle_commit(_tensor_array(tensors), len(tensors), h.bit_length() - 1, _dptr(tree), _dptr(rc), _stream_ptr(stream)))
    rc = to_host(rc)
    return rc[8:].copy(), rc[:8].copy(), tree


def bb_poseidon2_permute(states, stream=None):
    """[n, 16] numpy BabyBear Montgomery words -> permuted (sp1hip_bb_poseidon2_permute)."""
    d = to_device(np.ascontiguousarray(states, dtype=np.uint32).reshape(-1))
    check(_L().sp1hip_bb_poseidon2_permute(_dptr(d), d.numel() // 16, _stream_ptr(stream)))
    return to_host(d, (d.numel() // 16, 16))


class PinnedHost:
    """Pinned host words (sp1hip_malloc_host) holding one row-major table: what a host trace generator fills and
    `ProverPool.submit` uploads at full PCIe rate."""

    def __init__(self, table):
        table = np.ascontiguousarray(table, dtype=np.uint32)
        self.shape = table.shape
        p = C.c_void_p()
        check(_L().sp1hip_malloc_host(C.byref(p), max(table.nbytes, 4)))
        self.ptr = p
        if table.nbytes:
            C.memmove(p, table.ctypes.data, table.nbytes)

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                _L().sp1hip_free_host(self.ptr)
            except TypeError:                    # interpreter shutdown: the module globals are already gone
                pass
            self.ptr = None


class ProverPool:
    """N shard proofs in flight on one GPU (sp1hip_pool_*): `n_slots` prover slots (thread + stream each) plus a stager
    that uploads host traces of the next shards while the slots prove — the library-side `ProverSemaphore`."""

    def __init__(self, n_slots, device=None):
        import torch
        h = C.c_void_p()
        check(_L().sp1hip_pool_create(torch.cuda.current_device() if device is None else int(device), int(n_slots), C.byref(h)))
        self.h, self.n_slots, self._keep = h, int(n_slots), {}

    def submit(self, pk, chips, public_values=()):
        """chips: [(AirProgram, InteractionProgram, main, prep)] in name order; main is a ColMajor (resident in HBM), a
        PinnedHost (row-major host words the pool stages) or None; prep: the ColMajor the proving key was set up from."""
        arr = (_lib.PoolChip * len(chips))()
        keep = [chips, pk]
        for i, (air, inter, main, prep) in enumerate(chips):
            prog = np.ascontiguousarray(air.to_array(), dtype=np.uint32)
            words = np.ascontiguousarray(inter.to_array(), dtype=np.uint32)
            keep += [prog, words]
            if isinstance(main, PinnedHost):
                rows, h_main, d_main = main.shape[0], main.ptr, None
            else:
                rows = main.height if main is not None else 0
                h_main, d_main = None, (C.c_void_p(main.words.data_ptr()) if rows else None)
            arr[i] = _lib.PoolChip(inter.name.encode(), prog.ctypes.data_as(_lib.u32p), prog.shape[0], air.num_constraints,
                                   words.ctypes.data_as(_lib.u32p), words.size, air.main_width, air.prep_width, h_main, d_main,
                                   C.c_void_p(prep.words.data_ptr()) if prep is not None and rows and air.prep_width else None, rows)
        pv = np.ascontiguousarray(np.asarray(public_values, dtype=np.uint32).reshape(-1))
        keep += [arr, pv]
        t = C.c_uint64()
        check(_L().sp1hip_pool_submit(self.h, pk.h, arr, len(chips), pv.ctypes.data_as(_lib.u32p) if pv.size else None, int(pv.size),
                                      C.byref(t)))
        self._keep[t.value] = keep
        return t.value

    def wait(self, ticket, block=True):
        """-> (bincode(ShardProof), {"staging_ms", "queued_ms", "proving_ms", "slot"}); block=False returns None while the
        shard is in flight."""
        fn = _L().sp1hip_pool_wait if block else _L().sp1hip_pool_try_wait
        n, times = C.c_size_t(0), _lib.PoolTimes()
        st = fn(self.h, ticket, None, C.byref(n), C.byref(times))
        if st == _lib.ERROR_NOT_READY:
            return None
        if st != _lib.ERROR_BUFFER_TOO_SMALL:
            self._keep.pop(ticket, None)
            check(st)
            raise RuntimeError("size query unexpectedly succeeded")
        buf = (C.c_uint8 * n.value)()
        st = fn(self.h, ticket, buf, C.byref(n), C.byref(times))
        self._keep.pop(ticket, None)
        check(st)
        return C.string_at(buf, n.value), {"staging_ms": times.staging_ms, "queued_ms": times.queued_ms,
                                           "proving_ms": times.proving_ms, "slot": times.slot}

    def close(self):
        if getattr(self, "h", None):
            _L().sp1hip_pool_destroy(self.h)
            self.h = None
            self._keep.clear()

    def __del__(self):
        try:
            self.close()
        except TypeError:                        # interpreter shutdown: the module globals are already gone
            pass


def parse_logup_gkr_proof(blob):
    """The `logup_evaluations` of a bincode(LogupGkrProof): (point [L][4], [(name, main [w][4], prep [w][4] or None)])
    in Montgomery words — the zeta / openings that zerocheck consumes."""
    import struct
    o = 0

    def u64():
        nonlocal o
        v = struct.unpack_from("<Q", blob, o)[0]
        o += 8
        return v

    def exts(k):
        nonlocal o
        a = np.frombuffer(blob, dtype="<u4", count=4 * k, offset=o).astype(np.uint64)
        o += 16 * k
        return ((a << np.uint64(32)) % np.uint64(P)).astype(np.uint32).reshape(k, 4)

    for _ in range(2):                                     # circuit output
        exts(u64())
        o += 24
    for _ in range(u64()):                                 # round proofs
        exts(4)
        for _ in range(u64()):
            exts(u64())
        exts(1)
        exts(u64())
        exts(1)
    point = exts(u64())
    chips = []
    for _ in range(u64()):
        n = u64()
        name = blob[o:o + n].decode()
        o += n
        main = exts(u64())
        o += 16
        prep = None
        o += 1
        if blob[o - 1]:
            prep = exts(u64())
            o += 16
        chips.append((name, main, prep))
    assert o + 4 == len(blob)
    return point, chips


def parse_zerocheck_proof(blob):
    """Split the zerocheck output (layout in include/sp1hip.h) into the sumcheck point (Montgomery words,
    [dim][4]) and the per-chip opened values (one [w_prep + w_main][4] array per chip: preprocessed columns
    first, then main) — what the jagged evaluation proof takes as z_row and as its column claims."""
    import struct
    P_ = P
    o = 0

    def u64():
        nonlocal o
        v = struct.unpack_from("<Q", blob, o)[0]
        o += 8
        return v

    def exts(k):
        nonlocal o
        a = np.frombuffer(blob, dtype="<u4", count=4 * k, offset=o).astype(np.uint64)
        o += 16 * k
        return ((a << np.uint64(32)) % np.uint64(P_)).astype(np.uint32).reshape(k, 4)    # canonical -> Montgomery

    for _ in range(u64()):
        exts(u64())
    exts(1)
    point = exts(u64())
    exts(1)
    chips = []
    for _ in range(u64()):
        chips.append(exts(u64()))
    assert o == len(blob)
    return point, chips


# ---------------------------------------------------------------------------------------------------------- outer (BN254)
# The commitment layer and transcript of the wrap proof (`SP1OuterGlobalContext`, /root/reference/slop/crates/bn254/src/lib.rs):
# Poseidon2 over the BN254 scalar field, one BN254 element per Merkle digest, MultiField32Challenger. A BN254 value crosses the
# ABI as 8 little-endian u32 words in Montgomery form (R = 2^256).
OUTER_P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_OUTER_R = (1 << 256) % OUTER_P
_OUTER_R_INV = pow(1 << 256, -1, OUTER_P)


def outer_to_words(x):
    """Python int (or a sequence of them) -> uint32 array [..., 8] of Montgomery words."""
    if isinstance(x, (int, np.integer)):
        m = int(x) % OUTER_P * _OUTER_R % OUTER_P
        return np.array([(m >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
    return np.stack([outer_to_words(v) for v in x]) if len(x) else np.zeros((0, 8), np.uint32)


def outer_from_words(w):
    """uint32 array [..., 8] of Montgomery words -> Python int (or a nested list of them)."""
    w = np.asarray(w, dtype=np.uint32)
    if w.ndim == 1:
        m = sum(int(w[i]) << (32 * i) for i in range(8))
        return m * _OUTER_R_INV % OUTER_P
    return [outer_from_words(v) for v in w]


def outer_poseidon2_permute(states, stream=None):
    """Device batch of permutations: states = device words [n * 24] (n states of 3 x 8 Montgomery words), in place."""
    assert states.numel() % 24 == 0
    check(_L().sp1hip_outer_poseidon2_permute(_dptr(states), states.numel() // 24, _stream_ptr(stream)))
    return states


class OuterMerkleTcsProver:
    """Poseidon2Bn254 Merkle tensor commitment (the outer TCS prover): like MerkleTcsProver, one BN254 digest per node.
    Roots, commitments and paths are 8-word Montgomery arrays."""

    def commit_tensors(self, tensors, stream=None):
        h = tensors[0].height
        lg = h.bit_length() - 1
        assert all(t.height == h for t in tensors) and 1 << lg == h
        tree = device_words((2 * h - 1) * 8)
        rc = device_words(16)
        check(_L().sp1hip_outer_merkle_commit(_tensor_array(tensors), len(tensors), lg, _dptr(tree), _dptr(rc),
                                              _stream_ptr(stream)))
        rc_h = to_host(rc)
        data = TcsProverData(tree, rc_h[:8].copy(), rc_h[8:].copy(), lg, sum(t.width for t in tensors))
        return data.commit, data

    def prove_openings_at_indices(self, data, indices, stream=None):
        idx = to_device(np.asarray(indices, dtype=np.uint32))
        paths = device_words(max(len(indices) * data.log_height * 8, 1))
        none = (Tensor * 1)(Tensor(None, 0))
        check(_L().sp1hip_outer_merkle_open(none, 1, data.log_height, _dptr(data.tree), _dptr(idx), len(indices), None,
                                            _dptr(paths), _stream_ptr(stream)))
        return dict(merkle_root=data.root, log_tensor_height=data.log_height, width=data.total_width,
                    paths=to_host(paths)[:len(indices) * data.log_height * 8].reshape(len(indices), data.log_height, 8))

    def compute_openings_at_indices(self, tensors, indices, stream=None):
        idx = to_device(np.asarray(indices, dtype=np.uint32))
        tw = sum(t.width for t in tensors)
        lg = tensors[0].height.bit_length() - 1
        vals = device_words(len(indices) * tw)
        check(_L().sp1hip_outer_merkle_open(_tensor_array(tensors), len(tensors), lg, None, _dptr(idx), len(indices),
                                            _dptr(vals), None, _stream_ptr(stream)))
        return to_host(vals, (len(indices), tw))


def outer_commit_mles(mles, log_blowup=2, stream=None):
    """RS-encode every mle (the KoalaBear encoder of BasefoldProver.commit_mles) and commit the codewords with the outer tree.
    Returns (commitment words, codewords as ColMajor, TcsProverData)."""
    lg_n = mles[0].height.bit_length() - 1
    assert all(m.height == 1 << lg_n for m in mles)
    N = 1 << (lg_n + log_blowup)
    cws = [ColMajor(device_words(N * m.width), N, m.width) for m in mles]
    ptrs = (C.c_void_p * len(cws))(*[c.words.data_ptr() for c in cws])
    tree = device_words((2 * N - 1) * 8)
    commit = np.zeros(8, np.uint32)
    check(_L().sp1hip_outer_commit_mles(_tensor_array(mles), len(mles), lg_n, log_blowup, ptrs, _dptr(tree),
                                        commit.ctypes.data_as(_lib.u32p), _stream_ptr(stream)))
    return commit, cws, TcsProverData(tree, None, commit, lg_n + log_blowup, sum(m.width for m in mles))


class OuterBasefoldProverData:
    """Owns the codewords and the outer tree of one commitment round (sp1hip_outer_basefold_data_t)."""

    def __init__(self, handle, mles, commit):
        self.h, self.mles, self.commit = handle, mles, commit

    def __del__(self):
        if getattr(self, "h", None) and _L is not None:
            try:
                _L().sp1hip_outer_basefold_data_free(self.h)
            except TypeError:                    # interpreter shutdown: the module globals are already gone
                pass
            self.h = None


class OuterBasefoldProver:
    """BasefoldProver under the outer (BN254) configuration: Poseidon2-BN254 trees, the OuterChallenger transcript, proof bytes
    = bincode(BasefoldProof<SP1OuterGlobalContext>) with 40-byte digests (include/sp1hip.h)."""

    def commit_mles(self, mles, log_blowup, stream=None):
        """Returns (commitment: 8 Montgomery words, OuterBasefoldProverData)."""
        lg_n = mles[0].height.bit_length() - 1
        assert all(m.height == 1 << lg_n for m in mles)
        commit = np.zeros(8, np.uint32)
        handle = C.c_void_p()
        check(_L().sp1hip_outer_commit_mles_data(_tensor_array(mles), len(mles), lg_n, log_blowup,
                                                 commit.ctypes.data_as(_lib.u32p), C.byref(handle), _stream_ptr(stream)))
        return commit, OuterBasefoldProverData(handle, list(mles), commit)

    def proof_size(self, dim, rounds, config):
        widths = (C.c_uint32 * len(rounds))(*[sum(m.width for m in pd.mles) for pd in rounds])
        return _L().sp1hip_outer_basefold_proof_size(dim, widths, len(rounds), config)

    def prove(self, point, rounds, claims, challenger, config, stream=None):
        """point [dim][4], rounds: OuterBasefoldProverData per commitment round, claims [total width][4] (Montgomery words),
        challenger: OuterChallenger, config: FriConfig. Returns the proof bytes; the challenger advances only on success."""
        point = np.asarray(point, dtype=np.uint32).reshape(-1, 4)
        claims = np.asarray(claims, dtype=np.uint32).reshape(-1, 4)
        size = self.proof_size(point.shape[0], rounds, config)
        buf = (C.c_uint8 * size)()
        n = C.c_size_t(size)
        handles = (C.c_void_p * len(rounds))(*[pd.h for pd in rounds])
        check(_L().sp1hip_outer_basefold_prove(_ext_array(point), point.shape[0], handles, len(rounds), _ext_array(claims),
                                               claims.shape[0], config, challenger.h, buf, C.byref(n), _stream_ptr(stream)))
        return C.string_at(buf, n.value)


class OuterChallenger:
    """MultiField32Challenger<KoalaBear, Bn254Fr, Poseidon2Bn254, 3, 2> (host transcript, device grind). Observes and samples
    KoalaBear Montgomery words like DuplexChallenger; observe_commitment takes an 8-word BN254 digest."""

    def __init__(self, handle=None):
        if handle is None:
            handle = C.c_void_p()
            check(_L().sp1hip_outer_challenger_new(C.byref(handle)))
        self.h = handle

    def clone(self):
        out = C.c_void_p()
        check(_L().sp1hip_outer_challenger_clone(self.h, C.byref(out)))
        return OuterChallenger(out)

    def observe(self, felts):
        a = np.ascontiguousarray(np.asarray(felts, dtype=np.uint32).reshape(-1))
        check(_L().sp1hip_outer_challenger_observe(self.h, a.ctypes.data_as(_lib.u32p), a.size))

    def observe_commitment(self, digest):
        a = np.ascontiguousarray(np.asarray(digest, dtype=np.uint32).reshape(8))
        check(_L().sp1hip_outer_challenger_observe_commitment(self.h, a.ctypes.data_as(_lib.u32p)))

    def sample(self):
        out = C.c_uint32()
        check(_L().sp1hip_outer_challenger_sample(self.h, C.byref(out)))
        return out.value

    def sample_ext_element(self):
        e = Ext()
        check(_L().sp1hip_outer_challenger_sample_ext(self.h, C.byref(e)))
        return np.array(list(e.c), dtype=np.uint32)

    def sample_point(self, n):
        return np.stack([self.sample_ext_element() for _ in range(n)]) if n else np.zeros((0, 4), np.uint32)

    def sample_bits(self, bits):
        out = C.c_uint32()
        check(_L().sp1hip_outer_challenger_sample_bits(self.h, bits, C.byref(out)))
        return out.value

    def check_witness(self, bits, witness):
        ok = C.c_int()
        check(_L().sp1hip_outer_challenger_check_witness(self.h, bits, C.c_uint32(int(witness)), C.byref(ok)))
        return bool(ok.value)

    def grind(self, bits, stream=None):
        """The smallest witness (a Montgomery word), found on the device; the challenger ends as after check_witness."""
        out = C.c_uint32()
        check(_L().sp1hip_outer_challenger_grind(self.h, bits, C.byref(out), _stream_ptr(stream)))
        return out.value

    def state(self):
        out = np.zeros(50, np.uint32)
        check(_L().sp1hip_outer_challenger_state(self.h, out.ctypes.data_as(_lib.u32p)))
        return out

    def __del__(self):
        if getattr(self, "h", None) and _L is not None:
            try:
                _L().sp1hip_outer_challenger_free(self.h)
            except TypeError:                    # interpreter shutdown: the module globals are already gone
                pass
            self.h = None


class OuterStackedData:
    """Owns the dense stacked buffer and the outer BaseFold data of one outer commitment (sp1hip_outer_stacked_data_t).
    commit: the stacked commitment; jagged_commit, row_counts, column_counts (the two padding tables included): set when the
    handle came from OuterJaggedProver."""

    def __init__(self, handle, num_added_vals, log_stacking_height, jagged):
        self.h, self.num_added_vals, self.lsh = handle, num_added_vals, log_stacking_height
        bf, nb, dense, padded, nt = C.c_void_p(), C.c_int(), C.c_void_p(), C.c_uint64(), C.c_size_t()
        self.commit = np.zeros(8, np.uint32)
        check(_L().sp1hip_outer_stacked_data_info(handle, C.byref(bf), C.byref(nb), C.byref(dense), C.byref(padded),
                                                  self.commit.ctypes.data_as(_lib.u32p), None, C.byref(nt), None, None, 0))
        self.padded_area, self.basefold_handle = padded.value, bf
        self.jagged_commit, self.row_counts, self.column_counts = None, [], []
        if jagged:
            self.jagged_commit = np.zeros(8, np.uint32)
            rows, cols = (C.c_uint64 * nt.value)(), (C.c_uint64 * nt.value)()
            check(_L().sp1hip_outer_stacked_data_info(handle, None, None, None, None, None,
                                                      self.jagged_commit.ctypes.data_as(_lib.u32p), None, rows, cols, nt.value))
            self.row_counts, self.column_counts = list(rows), list(cols)
        self.batches = []
        for k in range(nb.value):
            t = Tensor()
            check(_L().sp1hip_outer_stacked_batch(handle, k, C.byref(t)))
            self.batches.append(_RawColMajor(t.d_data, 1 << log_stacking_height, t.width))

    def __del__(self):
        if getattr(self, "h", None) and _L is not None:
            try:
                _L().sp1hip_outer_stacked_data_free(self.h)
            except TypeError:                    # interpreter shutdown: the module globals are already gone
                pass
            self.h = None


class OuterStackedPcsProver:
    """StackedPcsProver under the outer (BN254) configuration."""

    def __init__(self, log_stacking_height, batch_size, log_blowup=3):
        self.lsh, self.batch_size, self.log_blowup = log_stacking_height, batch_size, log_blowup

    def commit_multilinears(self, tables, stream=None):
        commit = np.zeros(8, np.uint32)
        added, handle = C.c_uint64(), C.c_void_p()
        check(_L().sp1hip_outer_stacked_commit(_table_array(tables), len(tables), self.lsh, self.batch_size, self.log_blowup,
                                               commit.ctypes.data_as(_lib.u32p), C.byref(added), C.byref(handle),
                                               _stream_ptr(stream)))
        return commit, OuterStackedData(handle, added.value, self.lsh, False), added.value


class OuterJaggedProver:
    """JaggedProver under the outer (BN254) configuration: commit_multilinears over chip tables (zero-row tables are counted,
    not committed) and the whole evaluation proof, on an OuterChallenger."""

    def __init__(self, max_log_row_count, log_stacking_height, batch_size, log_blowup=3):
        self.max_log_row_count, self.lsh = max_log_row_count, log_stacking_height
        self.batch_size, self.log_blowup = batch_size, log_blowup

    def commit_multilinears(self, tables, stream=None):
        commit = np.zeros(8, np.uint32)
        handle = C.c_void_p()
        check(_L().sp1hip_outer_jagged_commit(_table_array(tables), len(tables), self.max_log_row_count, self.lsh,
                                              self.batch_size, self.log_blowup, commit.ctypes.data_as(_lib.u32p),
                                              C.byref(handle), _stream_ptr(stream)))
        return commit, OuterStackedData(handle, None, self.lsh, True)

    def _args(self, z_row, claims_per_round, rounds, challenger, num_queries, pow_bits):
        z_row = np.ascontiguousarray(np.asarray(z_row, dtype=np.uint32).reshape(-1, 4))
        assert z_row.shape[0] == self.max_log_row_count
        cl = [np.asarray(c, dtype=np.uint32).reshape(-1, 4) for c in claims_per_round]
        flat = np.ascontiguousarray(np.concatenate(cl)) if cl else np.zeros((0, 4), np.uint32)
        counts = (C.c_size_t * len(rounds))(*[c.shape[0] for c in cl])
        hs = (C.c_void_p * len(rounds))(*[r.h for r in rounds])
        cfg = FriConfig(self.log_blowup, num_queries, pow_bits)
        return [_ext_array(z_row), self.max_log_row_count, hs, len(rounds), _ext_array(flat) if flat.size else None, counts,
                cfg, challenger.h]

    def proof_size(self, rounds, num_queries, pow_bits):
        hs = (C.c_void_p * len(rounds))(*[r.h for r in rounds])
        return _L().sp1hip_outer_jagged_proof_size(hs, len(rounds), FriConfig(self.log_blowup, num_queries, pow_bits))

    def prove_trusted_evaluations(self, z_row, claims_per_round, rounds, challenger, num_queries=94, pow_bits=22, stream=None):
        """JaggedProver::prove_trusted_evaluations (/root/reference/slop/crates/jagged/src/prover.rs:L162-L328) under the outer
        configuration. rounds: the OuterStackedData of every commitment round, in order; claims_per_round[r]: [n_cols_r][4]
        column evaluations at z_row of round r's tables; challenger: an OuterChallenger, advanced on success only. Returns
        bincode(JaggedPcsProof<SP1OuterGlobalContext>)."""
        args = self._args(z_row, claims_per_round, rounds, challenger, num_queries, pow_bits)
        n = C.c_size_t(0)
        st = _L().sp1hip_outer_jagged_prove(*args, None, C.byref(n), _stream_ptr(stream))
        if st != _lib.ERROR_BUFFER_TOO_SMALL:                                   # anything but BUFFER_TOO_SMALL is a real error
            check(st)
            raise RuntimeError("size query unexpectedly succeeded")
        buf = (C.c_uint8 * n.value)()
        check(_L().sp1hip_outer_jagged_prove(*args, buf, C.byref(n), _stream_ptr(stream)))
        return C.string_at(buf, n.value)
