"""Edge-valued inputs (-m gpu) through the C ABI of the inner KoalaBear kernels: the delayed-reduction accumulators of
kb31.hpp at exactly the lengths their comments allow, folds and eq tables at challenges whose stored coordinates come from {0, R1, p - 1}, the RS-encode NTT on
columns that put a = 0 and b = p - 1 into one butterfly (the signed product's d = -(p - 1)), and Merkle trees over constant
tensors. Words are chosen in the stored (Montgomery) domain (tests/kb_edges.py): 0x7effffff and p - 1 = 0x7f000000 carry the
largest 16-bit halves. References: Python integers / oracle/kb_py.py / numpy uint64 with a reduction per term for small
shapes, the C++ oracle where it is the natural reference, closed forms (the encoding of a delta column is the powers of a
root of unity; the evaluation of a constant table is the constant) where neither is affordable."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import kb_py  # noqa: E402
import pyoracle as orc  # noqa: E402
from kb_edges import EDGE_WORDS, R1, R_INV  # noqa: E402

P = kb_py.P
V16 = 0x7EFFFFFF            # low half 0xffff under the largest high half
CHALLENGE_WORDS = (0, R1, P - 1)


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _ext_soa(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).T)     # [n][4] -> [4][n]


def _canon(words):
    """from_monty: numpy uint64 (a word times 2^-32 mod p is < 2^62)."""
    return np.asarray(words).astype(np.uint64) * np.uint64(R_INV) % np.uint64(P)


def _const_col_major(api, value, height, width):
    return api.ColMajor(torch.full((height * width,), int(value), dtype=torch.int32, device="cuda"), height, width)


# ------------------------------------------------------------------ sp1hip_basefold_batch at the 2^16-term bound

def _batch_reference(tables, coeffs):
    """out[r][k] = sum_g coeff[g][k] * col_g[r] * 2^-32 mod p: numpy uint64, every product reduced before it is added
    (a product is < 2^62; 2^16 reduced terms sum to < 2^47)."""
    cols = np.concatenate(tables, axis=1).astype(np.uint64)             # [rows][tw]
    out = np.zeros((cols.shape[0], 4), np.uint64)
    for k in range(4):
        out[:, k] = ((cols * coeffs[:, k].astype(np.uint64)[None, :]) % np.uint64(P)).sum(axis=1) % np.uint64(P)
    return (out * np.uint64(R_INV) % np.uint64(P)).astype(np.uint32)


@pytest.mark.parametrize("fill", ["v16", "p-1", "mixed"])
def test_batch_at_exactly_65536_columns(api, fill):
    """batch_kernel holds one DotAcc per row over ALL columns: 65536 columns is the stated limit of dot_add, and with
    coefficients p - 1 and words 0x7effffff the accumulators come within 2^-9 of dot_reduce64's 2^63. Three tensors, one of
    width 1; 128 rows = half a workgroup."""
    lg, widths = 7, (30000, 1, 35535)
    assert sum(widths) == 65536 and (1 << lg) % 256 != 0
    h = 1 << lg
    rng = np.random.default_rng(65536)
    if fill == "mixed":
        pool = np.array(EDGE_WORDS, dtype=np.uint32)
        tables = [pool[rng.integers(0, len(pool), (h, w))] for w in widths]
        tables[1][:] = P - 1
        coeffs = pool[rng.integers(0, len(pool), (65536, 4))]
    else:
        word = V16 if fill == "v16" else P - 1
        tables = [np.full((h, w), word, np.uint32) for w in widths]
        coeffs = np.full((65536, 4), P - 1, np.uint32)
    d_ts = [api.ColMajor.from_row_major_host(t) for t in tables]
    out = api.device_words(4 << lg)
    api.check(api._L().sp1hip_basefold_batch(api._tensor_array(d_ts), len(d_ts), lg, api._dptr(api.to_device(coeffs)),
                                             api._dptr(out), api._stream_ptr()))
    got = api.to_host(out, (4, h)).T
    want = _batch_reference(tables, coeffs)
    if fill != "mixed":         # ... and the closed form in Python integers: 65536 equal terms
        word = V16 if fill == "v16" else P - 1
        assert want[0].tolist() == [65536 * (P - 1) * word * R_INV % P] * 4
    assert np.array_equal(got, want)


def test_width_65537_is_refused_and_leaves_the_output_untouched(api):
    """Both `tw <= 65536` sites (sp1hip_basefold_batch and sp1hip_mle_eval_columns / evaluate_mles): the host check rejects
    the call before any launch."""
    lg = 3
    h = 1 << lg
    big, one = _const_col_major(api, P - 1, h, 65536), _const_col_major(api, P - 1, h, 1)
    coeffs = api.to_device(np.full((65537, 4), P - 1, np.uint32))
    sentinel = 0x5A5A5A5A
    L, s = api._L(), api._stream_ptr()
    out = torch.full((4 * h,), sentinel, dtype=torch.int32, device="cuda")
    st = L.sp1hip_basefold_batch(api._tensor_array([big, one]), 2, lg, api._dptr(coeffs), api._dptr(out), s)
    assert st != 0 and b"2^16 columns" in L.sp1hip_last_error()
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    eq = api.device_words(4 << lg)
    api.check(L.sp1hip_partial_lagrange(api._ext_array(np.full((lg, 4), R1, np.uint32)), lg, api._dptr(eq), s))
    evals = torch.full((65537 * 4,), sentinel, dtype=torch.int32, device="cuda")
    st = L.sp1hip_mle_eval_columns(api._tensor_array([big, one]), 2, lg, api._dptr(eq), api._dptr(evals), s)
    assert st != 0 and b"2^16 columns" in L.sp1hip_last_error()
    torch.cuda.synchronize()
    assert bool((evals == sentinel).all())
    with pytest.raises(api._lib.Sp1HipError):
        api.BasefoldProver().evaluate_mles([big, one], np.full((lg, 4), R1, np.uint32))
    # ... and 65536 columns pass through the same entry: a constant table evaluates to the constant
    claims = api.BasefoldProver().evaluate_mles([big], orc.random_felts((lg, 4), 5))
    assert claims.shape == (65536, 4) and np.array_equal(claims, np.tile(np.array([P - 1, 0, 0, 0], np.uint32), (65536, 1)))


# ------------------------------------------------------------------ evaluate_mles: constants and deltas

def _edge_point(dim, seed):
    """A point whose coordinates mix random extension elements with words from {0, 1 (stored R1), p - 1} and 0x7effffff."""
    pt = orc.random_felts((dim, 4), seed)
    rng = np.random.default_rng(seed)
    pool = np.array(CHALLENGE_WORDS + (V16,), dtype=np.uint32)
    for j in range(0, dim, 3):
        pt[j] = pool[rng.integers(0, len(pool), 4)]
    return pt


@pytest.mark.parametrize("lg", [20, 10, 5])
def test_evaluate_mles_of_constant_and_delta_tables(api, lg):
    """The evaluation of a constant table is the constant at ANY point (sum of eq = 1), whatever the unreduced sums did on
    the way; the evaluation of a delta table is the partial_lagrange entry of its row (times the word). 2^20 rows: 64
    chunks of EVAL_ROWS = 16384, 64 dot_add terms per lane; 2^10 and 2^5 rows leave the only workgroup partial (and at 2^5
    most lanes without a row)."""
    h = 1 << lg
    consts = [P - 1, V16, 0x7EFF0000, R1, 1, 0, (P + 1) // 2]
    rows = sorted({0, 1, h - 1, h // 2, h // 2 - 1, (h * 2) // 3, 255 % h, 256 % h, 16383 % h, 16384 % h})
    delta = np.zeros((h, len(rows) + 1), np.uint32)
    for c, r in enumerate(rows):
        delta[r, c] = P - 1 if c % 2 == 0 else V16
    delta[::2, len(rows)] = P - 1                                         # alternating p - 1 / 0: the sum of eq over even rows
    d_const = api.ColMajor(torch.tensor(consts, dtype=torch.int32, device="cuda").repeat_interleave(h), h, len(consts))
    d_delta = api.ColMajor.from_row_major_host(delta)
    for seed in (1, 2):
        pt = _edge_point(lg, 900 + 10 * lg + seed)
        claims = api.BasefoldProver().evaluate_mles([d_const, d_delta], pt)
        want_c = np.zeros((len(consts), 4), np.uint32)
        want_c[:, 0] = consts
        assert np.array_equal(claims[:len(consts)], want_c), (lg, seed)
        eq = _canon(orc.partial_lagrange(pt))                             # [h][4], canonical
        for c, r in enumerate(rows):
            w = (P - 1 if c % 2 == 0 else V16)                            # stored word: result = eq[r] * w (one Montgomery factor)
            want = [int(e) * w % P for e in eq[r]]                        # canonical eq times stored word = stored product
            assert claims[len(consts) + c].tolist() == want, (lg, seed, r)
        even = eq[::2].sum(axis=0) % np.uint64(P)
        assert claims[-1].tolist() == [int(e) * (P - 1) % P for e in even], (lg, seed)


# ------------------------------------------------------------------ folds, eq tables, fix_last_variable at {0, R1, p - 1}

def _edge_tables(n, width=4):
    """[n][width] tables: all p - 1, all 0, alternating 0 / p - 1 (both phases), all 0x7effffff."""
    alt = np.zeros((n, width), np.uint32)
    alt[1::2] = P - 1
    alt2 = np.zeros((n, width), np.uint32)
    alt2[0::2] = P - 1
    return [np.full((n, width), P - 1, np.uint32), np.zeros((n, width), np.uint32), alt, alt2, np.full((n, width), V16, np.uint32)]


def _edge_exts(limit=None):
    """Every extension element with coordinates in {0, R1, p - 1} (81), or a spread of `limit` of them."""
    allb = [np.array(t, np.uint32) for t in itertools.product(CHALLENGE_WORDS, repeat=4)]
    if limit is None or limit >= len(allb):
        return allb
    keep = [0, 1, 2, 27, 40, 54, 80, 79, 13, 26]                          # 0, x^3, (p - 1) x^3, 1, all ones, p - 1, all p - 1, ...
    return [allb[i] for i in keep[:limit]]


def test_partial_lagrange_at_edge_points(api):
    L, s = api._L(), api._stream_ptr()
    rng = np.random.default_rng(77)
    pool = np.array(CHALLENGE_WORDS, dtype=np.uint32)
    for dim in (0, 1, 2, 5, 13):
        pts = [np.tile(np.array(b, np.uint32), (dim, 1)) for b in _edge_exts(6)] + [pool[rng.integers(0, 3, (dim, 4))] for _ in range(4)]
        for pt in pts:
            out = api.device_words(4 << dim)
            api.check(L.sp1hip_partial_lagrange(api._ext_array(pt), dim, api._dptr(out), s))
            assert np.array_equal(api.to_host(out, (4, 1 << dim)).T, orc.partial_lagrange(pt)), (dim, pt[:1])
    # a boolean point selects one entry: the table is the stored one there and 0 elsewhere (Python integers)
    dim, index = 13, 0b1011001110001
    pt = np.zeros((dim, 4), np.uint32)
    for j in range(dim):
        pt[j, 0] = R1 if (index >> (dim - 1 - j)) & 1 else 0
    out = api.device_words(4 << dim)
    api.check(L.sp1hip_partial_lagrange(api._ext_array(pt), dim, api._dptr(out), s))
    want = np.zeros((1 << dim, 4), np.uint32)
    want[index, 0] = R1
    assert np.array_equal(api.to_host(out, (4, 1 << dim)).T, want)


@pytest.mark.parametrize("lg_n", [1, 2, 3, 10, 15])
def test_folds_at_edge_challenges_and_tables(api, lg_n):
    """sp1hip_fold_even_odd / sp1hip_fold_mle against the oracle, sp1hip_ext_fixed_at_zero against kb_py: tables of p - 1, 0,
    alternating 0 / p - 1 (e0 - e1 = -(p - 1) and its negative in every pair) and 0x7effffff; every challenge with
    stored coordinates in {0, R1, p - 1} at the small sizes, a spread of them at 2^10 and 2^15."""
    L, s = api._L(), api._stream_ptr()
    n = 1 << lg_n
    betas = _edge_exts(None if lg_n <= 3 else 10)
    for ti, cw in enumerate(_edge_tables(n)):
        d_cw = api.to_device(_ext_soa(cw))
        o1 = api.device_words(2 << lg_n)
        for beta in betas:
            api.check(L.sp1hip_fold_even_odd(api._dptr(d_cw), lg_n, api._ext(beta), api._dptr(o1), s))
            assert np.array_equal(api.to_host(o1, (4, n // 2)).T, orc.fold_even_odd(cw, beta)), (lg_n, ti, beta)
            api.check(L.sp1hip_fold_mle(api._dptr(d_cw), lg_n, api._ext(beta), api._dptr(o1), s))
            got = api.to_host(o1, (4, n // 2)).T
            assert np.array_equal(got, orc.fold_mle(cw, beta)), (lg_n, ti, beta)
            # out[i] = m[2i] + beta m[2i + 1] in Python integers on the first and last pair
            bc = [int(v) for v in _canon(beta)]
            for i in (0, n // 2 - 1):
                want = kb_py.ext_add(kb_py.ext_mul(bc, [int(v) for v in _canon(cw[2 * i + 1])]), [int(v) for v in _canon(cw[2 * i])])
                assert [int(v) for v in _canon(got[i])] == want, (lg_n, ti, beta)
        # fixed_at_zero = sum_i eq[i] * cw[2 i]; eq tables of edge points and constant eq tables of edge words
        eqs = [orc.partial_lagrange(np.tile(b, (lg_n - 1, 1))) for b in _edge_exts(4)]
        eqs += [np.full((n // 2, 4), P - 1, np.uint32), np.full((n // 2, 4), V16, np.uint32)]
        ce = _canon(cw)
        for eq in eqs:
            o4 = api.device_words(4)
            api.check(L.sp1hip_ext_fixed_at_zero(api._dptr(d_cw), lg_n, api._dptr(api.to_device(_ext_soa(eq))), api._dptr(o4), s))
            cq = _canon(eq)
            if (eq == eq[0]).all() and (cw[0::2] == cw[0]).all():         # constant x constant: n/2 equal terms
                acc = kb_py.ext_scale(kb_py.ext_mul([int(v) for v in cq[0]], [int(v) for v in ce[0]]), n // 2)
            else:
                acc = [0, 0, 0, 0]
                for i in range(n // 2):
                    if any(cq[i]) and any(ce[2 * i]):
                        acc = kb_py.ext_add(acc, kb_py.ext_mul([int(v) for v in cq[i]], [int(v) for v in ce[2 * i]]))
            assert [int(v) for v in _canon(api.to_host(o4))] == acc, (lg_n, ti)


@pytest.mark.parametrize("rows,width,pad", [(1000, 5, True), (1001, 3, True), (1, 2, True), (777, 4, False), (2, 1, False)])
def test_fix_last_variable_at_edge_challenges_and_tables(api, rows, width, pad):
    """out[i][c] = x + alpha (y - x), base input then the extension output fed back in, in Python integers (kb_py)."""
    L, s = api._L(), api._stream_ptr()
    alphas = _edge_exts(5)
    for ti, tab in enumerate(_edge_tables(rows, width)):
        d_in = api.ColMajor.from_row_major_host(tab)
        t = _canon(tab)
        padding = np.array([(P - 1, 0, V16)[c % 3] for c in range(width)], np.uint32)
        pv = [int(v) for v in _canon(padding)] if pad else [0] * width
        for ai, alpha in enumerate(alphas):
            out_rows = (rows + 1) // 2
            d_out = api.device_words(out_rows * width * 4)
            api.check(L.sp1hip_fix_last_variable(api._dptr(d_in.words), rows, width, 0, api._ext(alpha),
                                                 api._dptr(api.to_device(padding)) if pad else None, api._dptr(d_out), s))
            got = _canon(api.to_host(d_out)).reshape(width, 4, out_rows)
            al = [int(v) for v in _canon(alpha)]
            want = np.zeros((width, 4, out_rows), dtype=object)
            for c in range(width):
                for i in range(out_rows):
                    x = int(t[2 * i, c])
                    y = int(t[2 * i + 1, c]) if 2 * i + 1 < rows else pv[c]
                    want[c, :, i] = kb_py.ext_add(kb_py.ext_scale(al, (y - x) % P), kb_py.ext_from_base(x))
            assert np.array_equal(got.astype(object), want), (ti, ai)
            # second application on the extension table, with the next challenge of the list and extension padding
            beta = alphas[(ai + 1) % len(alphas)]
            out2 = (out_rows + 1) // 2
            pad2 = np.tile(np.array([P - 1, V16, 0, R1], np.uint32), width)
            d_out2 = api.device_words(out2 * width * 4)
            api.check(L.sp1hip_fix_last_variable(api._dptr(d_out), out_rows, width, 1, api._ext(beta),
                                                 api._dptr(api.to_device(pad2)) if pad else None, api._dptr(d_out2), s))
            got2 = _canon(api.to_host(d_out2)).reshape(width, 4, out2)
            be = [int(v) for v in _canon(beta)]
            p2 = _canon(pad2).reshape(width, 4) if pad else np.zeros((width, 4), dtype=object)
            want2 = np.zeros((width, 4, out2), dtype=object)
            for c in range(width):
                for i in range(out2):
                    x = [int(v) for v in want[c, :, 2 * i]]
                    y = [int(v) for v in want[c, :, 2 * i + 1]] if 2 * i + 1 < out_rows else [int(v) for v in p2[c]]
                    want2[c, :, i] = kb_py.ext_add(kb_py.ext_mul(be, kb_py.ext_sub(y, x)), x)
            assert np.array_equal(got2.astype(object), want2), (ti, ai)


# ------------------------------------------------------------------ DftEncoder.encode_batch

def _ntt_columns(lg_n):
    """[n][lg_n + 5+] stored words: all 0, all p - 1, 0 / p - 1 alternating at stride 2^k for every k < lg_n (a = 0 and
    b = p - 1 meet in one butterfly at the stage of that stride: the signed product's d = -(p - 1); the other phase gives
    d = p - 1), single non-zero words at index 0, n - 1 and the middle."""
    n = 1 << lg_n
    cols = [np.zeros(n, np.uint32), np.full(n, P - 1, np.uint32)]
    i = np.arange(n)
    for k in range(lg_n):
        cols.append(np.where((i >> k) & 1, P - 1, 0).astype(np.uint32))
        cols.append(np.where((i >> k) & 1, 0, P - 1).astype(np.uint32))
    for idx, w in ((0, P - 1), (n - 1, P - 1), (n // 2, V16), (n // 3, R1), (n - 1, 1)):
        d = np.zeros(n, np.uint32)
        d[idx] = w
        cols.append(d)
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("lg_n", list(range(0, 16)) + [17])
def test_rs_encode_of_edge_columns_matches_oracle(api, lg_n):
    m = _ntt_columns(lg_n)
    for lb in (1, 2):
        if lg_n <= 15 and lg_n + lb > 16:
            continue
        want = orc.rs_encode(m, lb)
        got = api.DftEncoder(lb).encode_batch([api.ColMajor.from_row_major_host(m)])[0]
        assert np.array_equal(got.to_row_major_host(), want), (lg_n, lb)


def _bit_reverse_indices(bits):
    rev = np.zeros(1, np.int64)
    for _ in range(bits):
        rev = np.concatenate([2 * rev, 2 * rev + 1])
    return rev


def _powers(g, count):
    """g^0 .. g^(count - 1) mod p (count a power of two), numpy uint64 by doubling."""
    pw = np.ones(1, np.uint64)
    step = g % P
    while len(pw) < count:
        pw = np.concatenate([pw, pw * np.uint64(step) % np.uint64(P)])
        step = step * step % P
    return pw


def _delta_codeword(lg_n, lb, index, word):
    """The encoding of the column with stored `word` at row `index` and 0 elsewhere: natural-order entry i is
    word * w^(i * index) with w = two_adic_generator(lg_n + lb) (canonical power, so the product stays a stored word); the
    output rows are bit-reversed."""
    lg_t = lg_n + lb
    w = kb_py.two_adic_generator(lg_t)
    nat = _powers(pow(w, index, P), 1 << lg_t) * np.uint64(word) % np.uint64(P)
    return nat[_bit_reverse_indices(lg_t)].astype(np.uint32)


@pytest.mark.parametrize("lg_n,lb", [(20, 2), (22, 2)])
def test_rs_encode_closed_forms_at_size(api, lg_n, lb):
    """Multi-pass plans at 2^22 and 2^24 points. The closed form's index convention (which root, which row order) is first
    established against the oracle at 2^3 .. 2^13 rows, then used at size: every row of the delta columns. The constant and
    alternating columns keep the checksums of test_baseline_config2_commit_properties: row 0 is the column sum, row 1
    the alternating sum."""
    enc = api.DftEncoder(lb)
    for small in (3, 8, 13):
        for index, word in ((0, P - 1), ((1 << small) - 1, V16), (5, R1)):
            col = np.zeros((1 << small, 1), np.uint32)
            col[index, 0] = word
            assert np.array_equal(orc.rs_encode(col, lb)[:, 0], _delta_codeword(small, lb, index, word)), (small, index)
    n = 1 << lg_n
    deltas = [(0, P - 1), (n - 1, P - 1), (n // 2, V16), (n // 3, P - 1), (1, V16)]
    m = torch.zeros((len(deltas) + 4, n), dtype=torch.int32, device="cuda")           # column-major: [col][row]
    for c, (index, word) in enumerate(deltas):
        m[c, index] = word
    c0 = len(deltas)
    m[c0] = P - 1                                                                      # all p - 1
    m[c0 + 1, 1::2] = P - 1                                                            # 0 / p - 1 at stride 1
    m[c0 + 2].view(-1, 2 << (lg_n // 2))[:, (1 << (lg_n // 2)):] = P - 1              # ... at stride 2^(lg_n / 2)
    m[c0 + 3, n // 2:] = P - 1                                                         # ... at stride n / 2
    cw = enc.encode_batch([api.ColMajor(m.reshape(-1), n, m.shape[0])])[0]
    out = cw.words.view(m.shape[0], n << lb)
    for c, (index, word) in enumerate(deltas):
        got = out[c].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, _delta_codeword(lg_n, lb, index, word)), (lg_n, index)
    cols = m[c0:].cpu().numpy().view(np.uint32).astype(np.uint64)                      # stored words: the DFT is linear
    total = cols.sum(axis=1) % P
    alt = (cols[:, 0::2].sum(axis=1) + (P - cols[:, 1::2].sum(axis=1) % P)) % P
    head = out[c0:, :2].cpu().numpy().view(np.uint32)
    assert head[:, 0].tolist() == total.tolist() and head[:, 1].tolist() == alt.tolist()


# ------------------------------------------------------------------ Merkle trees over constant tensors

@pytest.mark.parametrize("height,widths", [(1 << 10, [25] * 10), (1, [3]), (2, [8]), (256, [1]), (1 << 12, [7, 9, 16, 1]),
                                            (1 << 13, [32, 32, 32]), (64, [200])])
@pytest.mark.parametrize("word", [0, P - 1, V16])
def test_merkle_tree_of_constant_tensors(api, height, widths, word):
    """Every leaf absorbs the same edge word in every lane (the sponge's lazy ranges at their ends), every layer compresses
    two equal digests: the whole tree against the oracle."""
    ts = [np.full((height, w), word, np.uint32) for w in widths]
    want = orc.MerkleTree(ts)
    commit, data = api.MerkleTcsProver().commit_tensors([api.ColMajor.from_row_major_host(t) for t in ts])
    assert np.array_equal(commit, want.commit)
    assert np.array_equal(data.root, want.root())
    assert np.array_equal(api.to_host(data.tree, (2 * height - 1, 8)), want.layers())
