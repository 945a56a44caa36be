"""Edge values for the KoalaBear kernels, chosen in the STORED (Montgomery) domain, which is what a kernel sees: words whose
16-bit halves are 0 or 0xffff under the largest high half, the Montgomery one and its negative, the values around p / 2.
A uniform random word reaches about half of every range bound of sp1_amd/csrc/kb31.hpp; these reach them.

EdgeSource stands in for the numpy Generator of the hand-written trace generators (tests/gkr_chips.py, tests/zc_airs.py,
tests/test_gpu_jagged.py): a draw of field elements (`integers(0, P, ...)`) returns the canonical values whose stored words
come from the pool, column by column constant, alternating at a power-of-two stride, or picked per row; every other draw
(selectors, multiplicities, permutations) goes to an ordinary seeded Generator. Dependent columns are still computed by the
generators from what they drew, so constraints hold and buses balance."""
import numpy as np

P = 0x7F000001
R1 = (1 << 32) % P
R_INV = pow(1 << 32, -1, P)
EDGE_WORDS = [0, 1, 2, R1, P - R1, P - 2, P - 1, (P - 1) // 2, (P + 1) // 2, 0xFFFF, 0x10000, 0x00FFFFFF, 0x01000000, 0x7EFFFFFF,
              0x7EFF0000]
HEAVY_WORDS = [P - 1, 0x7EFFFFFF, 0x7EFF0000, P - 2]      # the largest 16-bit halves and the largest words
EDGE_CANONICAL = [w * R_INV % P for w in EDGE_WORDS]      # from_monty of the pool: what a generator of canonical values draws
HEAVY_CANONICAL = [w * R_INV % P for w in HEAVY_WORDS]


def from_monty_int(w):
    return int(w) * R_INV % P


class EdgeSource:
    """integers / permutation of numpy.random.Generator, with the field-element draws replaced by pool values."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.columns = 0

    def _column(self, rows):
        mode, self.columns = self.columns % 5, self.columns + 1
        pool = np.array(EDGE_CANONICAL, dtype=np.uint64)
        heavy = np.array(HEAVY_CANONICAL, dtype=np.uint64)
        pick = lambda src: src[int(self.rng.integers(0, len(src)))]
        if mode == 0:                                       # a whole column of one heavy word
            return np.full(rows, pick(heavy), dtype=np.uint64)
        if mode == 1:                                       # 0 / p - 1 (stored) alternating at a power-of-two stride
            stride = 1 << int(self.rng.integers(0, max(1, rows.bit_length())))
            return np.where((np.arange(rows) // stride) & 1, np.uint64(from_monty_int(P - 1)), np.uint64(0)).astype(np.uint64)
        if mode == 2:                                       # any pool word per row
            return pool[self.rng.integers(0, len(pool), rows)]
        if mode == 3:                                       # heavy words per row
            return heavy[self.rng.integers(0, len(heavy), rows)]
        return np.full(rows, pick(pool), dtype=np.uint64)   # a whole column of one pool word

    def integers(self, low, high=None, size=None, dtype=np.int64):
        if high != P or low != 0:
            return self.rng.integers(low, high, size, dtype=dtype)
        shape = (int(size),) if np.isscalar(size) else tuple(int(s) for s in size)
        rows, cols = shape[0], int(np.prod(shape[1:], dtype=np.int64))
        out = np.stack([self._column(rows) for _ in range(cols)], axis=1) if cols else np.zeros((rows, 0), np.uint64)
        return out.reshape(shape).astype(dtype)

    def permutation(self, n):
        return self.rng.permutation(n)
