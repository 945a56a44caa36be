"""Pure-Python model of the outer (BN254) commitment layer, written from the specification (Python ints, no library code):

  * Poseidon2 over the BN254 scalar field: width 3, x^5, external layer circ(2, 1, 1) once up front, 4 full rounds, 56
    partial rounds with the internal diagonal [1, 1, 2], 4 full rounds; constants from the Poseidon paper's Grain LFSR;
  * reduce_31: sum canonical(v_i) 2^(31 i) over <= 8 KoalaBear elements, the first least significant;
  * the sponge MultiField32PaddingFreeSponge<KB, Fr, Perm, 3, 16, 1>: 16-element blocks, chunk j of 8 overwrites lane j,
    one permutation per block, digest = lane 0; compress = permute([l, r, 0])[0];
  * the Merkle tensor commitment (leaf i = sponge over row i of all tensors, binary tree of compresses, commitment =
    compress(root, hash([log_height, width]))) and opening verification;
  * MultiField32Challenger<KB, Fr, Perm, 3, 2>.

KoalaBear words that cross the C ABI are Montgomery words (R = 2^32); BN254 values 8 LE u32 words, Montgomery (R = 2^256).
About 0.35 ms per permutation: keep model-compared sizes small."""
import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
KB_P = 0x7F000001
R256 = 1 << 256

KNOWN_ANSWER_IN = [0, 1, 2]
KNOWN_ANSWER_OUT = [0x0bb61d24daca55eebcb1929a82650f328134334da98ea4f847f760054f4a3033,
                    0x303b6f7c86d043bfcbcc80214f26a30277a15d3f74ca654992defe7ff8d03570,
                    0x1ed25194542b12eef8617361c3ba7c52e660b145994427cc86296242cf766ec8]


# ------------------------------------------------------------------------------------------------ constants
def _grain(n_values):
    # the 80-bit register as an int, bit 79 = the oldest bit; new bits enter at bit 0
    init = (1 << 78) | (0 << 74) | (254 << 62) | (3 << 50) | (8 << 40) | (56 << 30) | ((1 << 30) - 1)
    reg = init

    def bit():
        nonlocal reg
        b = ((reg >> 79) ^ (reg >> 66) ^ (reg >> 56) ^ (reg >> 41) ^ (reg >> 28) ^ (reg >> 17)) & 1
        reg = ((reg << 1) | b) & ((1 << 80) - 1)
        return b

    for _ in range(160):
        bit()
    vals = []
    while len(vals) < n_values:
        x, got = 0, 0
        while got < 254:
            first, second = bit(), bit()
            if first == 1:
                x = (x << 1) | second
                got += 1
        if x < P:
            vals.append(x)
    return vals


def round_constants():
    """[(c0, c1, c2)] per round, 64 rounds: 4 full, 56 partial (lanes 1, 2 zero), 4 full."""
    v = _grain(80)
    rounds = [tuple(v[3 * r:3 * r + 3]) for r in range(4)]
    rounds += [(v[12 + r], 0, 0) for r in range(56)]
    rounds += [tuple(v[68 + 3 * r:68 + 3 * r + 3]) for r in range(4)]
    return rounds


_RC = None


def _rc():
    global _RC
    if _RC is None:
        _RC = round_constants()
    return _RC


# ------------------------------------------------------------------------------------------------ permutation
def _external(x):
    s = x[0] + x[1] + x[2]
    return [(x[0] + s) % P, (x[1] + s) % P, (x[2] + s) % P]


def _internal(x):
    s = x[0] + x[1] + x[2]
    return [(x[0] + s) % P, (x[1] + s) % P, (2 * x[2] + s) % P]


def permute(state):
    """Canonical ints in, canonical ints out."""
    x = _external([int(v) % P for v in state])
    rc = _rc()
    for r in range(64):
        if r < 4 or r >= 60:
            x = [pow((x[i] + rc[r][i]) % P, 5, P) for i in range(3)]
            x = _external(x)
        else:
            x[0] = pow((x[0] + rc[r][0]) % P, 5, P)
            x = _internal(x)
    return x


# ------------------------------------------------------------------------------------------------ encodings
def to_words(x):
    """canonical int -> 8 LE u32 Montgomery words."""
    m = x * R256 % P
    return [(m >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_words(w):
    m = sum(int(w[i]) << (32 * i) for i in range(8))
    return m * pow(R256, -1, P) % P


def kb_to_monty(v):
    return (int(v) << 32) % KB_P


def kb_from_monty(m):
    return int(m) * pow(1 << 32, -1, KB_P) % KB_P


def reduce_31(canon):
    assert len(canon) <= 8
    return sum(int(v) << (31 * i) for i, v in enumerate(canon))


def split_32(x, n=4):
    """canonical BN254 int -> n canonical KoalaBear elements: the 64-bit chunks, each reduced mod p_KB."""
    return [((x >> (64 * k)) & ((1 << 64) - 1)) % KB_P for k in range(n)]


# ------------------------------------------------------------------------------------------------ sponge / tree
def hash_row(canon):
    """Digest (canonical int) of a row of canonical KoalaBear elements."""
    st = [0, 0, 0]
    for b in range(0, len(canon), 16):
        block = canon[b:b + 16]
        for j in range(0, len(block), 8):
            st[j // 8] = reduce_31(block[j:j + 8])
        st = permute(st)
    return st[0]


def compress(left, right):
    return permute([left, right, 0])[0]


def row_canon(tables, i):
    """Row i of the concatenated tables (each a numpy [height][width] array of Montgomery KB words), canonical."""
    out = []
    for t in tables:
        out += [kb_from_monty(v) for v in t[i]]
    return out


def merkle_tree(tables):
    """All layers leaf-first as lists of canonical ints, plus (root, commitment)."""
    h = tables[0].shape[0]
    lg = h.bit_length() - 1
    width = sum(t.shape[1] for t in tables)
    layers = [[hash_row(row_canon(tables, i)) for i in range(h)]]
    while len(layers[-1]) > 1:
        cur = layers[-1]
        layers.append([compress(cur[2 * k], cur[2 * k + 1]) for k in range(len(cur) // 2)])
    root = layers[-1][0]
    return layers, root, commitment(root, lg, width)


def commitment(root, lg_height, width):
    return compress(root, hash_row([lg_height, width]))


def tree_words(layers):
    """The device tree layout: every node's 8 Montgomery words, leaf layer first."""
    return np.array([to_words(x) for layer in layers for x in layer], dtype=np.uint32)


def verify_tensor_openings(commit, root, lg_height, width, indices, values, paths):
    """MerkleTreeTcs::verify_tensor_openings: values[q] (Montgomery KB words of row indices[q]) and sibling paths
    (canonical ints, [q][lg_height]) against root / commitment (canonical ints). Returns True when everything checks."""
    if commitment(root, lg_height, width) != commit:
        return False
    for q, idx in enumerate(indices):
        if len(values[q]) != width or len(paths[q]) != lg_height:
            return False
        node = hash_row([kb_from_monty(v) for v in values[q]])
        for k in range(lg_height):
            sib = paths[q][k]
            node = compress(sib, node) if (idx >> k) & 1 else compress(node, sib)
        if node != root:
            return False
    return True


# ------------------------------------------------------------------------------------------------ challenger
class Challenger:
    """MultiField32Challenger<KoalaBear, Bn254Fr, Perm, 3, 2>: observes / samples Montgomery KB words."""

    def __init__(self):
        self.sponge = [0, 0, 0]
        self.inp = []                   # canonical KB
        self.out = []                   # canonical KB, popped from the end

    def clone(self):
        c = Challenger()
        c.sponge, c.inp, c.out = list(self.sponge), list(self.inp), list(self.out)
        return c

    def _duplex(self):
        for i in range(0, len(self.inp), 8):
            self.sponge[i // 8] = reduce_31(self.inp[i:i + 8])
        self.inp = []
        self.sponge = permute(self.sponge)
        self.out = []
        for lane in self.sponge[:2]:
            self.out += split_32(lane, 4)

    def observe(self, m):
        self.out = []
        self.inp.append(kb_from_monty(m))
        if len(self.inp) == 16:
            self._duplex()

    def observe_many(self, ms):
        for m in ms:
            self.observe(m)

    def observe_commitment(self, x):
        """x: canonical BN254 int."""
        for v in split_32(x, 4):
            self.observe(kb_to_monty(v))

    def _sample_canon(self):
        if self.inp or not self.out:
            self._duplex()
        return self.out.pop()

    def sample(self):
        return kb_to_monty(self._sample_canon())

    def sample_ext(self):
        return [self.sample() for _ in range(4)]

    def sample_bits(self, bits):
        return self._sample_canon() & ((1 << bits) - 1)

    def check_witness(self, bits, w_monty):
        self.observe(w_monty)
        return self.sample_bits(bits) == 0

    def state(self):
        """The C ABI's 50-word dump: sponge [3][8] Montgomery words, n_in, input[16] (Montgomery KB, zero-padded), n_out,
        output[8] (Montgomery KB, zero-padded)."""
        out = []
        for x in self.sponge:
            out += to_words(x)
        out.append(len(self.inp))
        out += [kb_to_monty(v) for v in self.inp] + [0] * (16 - len(self.inp))
        out.append(len(self.out))
        out += [kb_to_monty(v) for v in self.out] + [0] * (8 - len(self.out))
        return np.array(out, dtype=np.uint32)
