"""
TEST INFRASTRUCTURE -- the sample definition of include/bsx.h ("attract over sampled initial conditions") restated in
Python ints and, for whole arrays of generator words, in numpy.  Nothing under boolsi_amd/ imports it.

    G      = 0x9E3779B97F4A7C15
    mix(z) : z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
    k0     = mix(seed + G)
    kb(b)  = mix(k0 + G * (b + 1))                     b = j >> 6
    A(b,a) = mix(kb(b) + G * (a + 1))                  a = 0 .. n_any-1, the order of any_nodes
    U(j)   = mix(kb(j >> 6) + G * (n_any + 1 + (j & 63)))

Sample j: 'any' node a has bit (j & 63) of A(j >> 6, a); variant number (U(j) * V) >> 64; flat index
I(j) = sum bit_a 2^a + variant 2^n_any.  The reference result of a sampled call is
WideRef(net, space).attract(sample_indices(space, seed, samples), ...) aggregated with wide_ref.aggregate.
"""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def key0(seed):
    return mix(seed + G)


def block_key(seed, b):
    return mix(key0(seed) + G * (b + 1))


def any_word(seed, b, a):
    """A(b, a)"""
    return mix(block_key(seed, b) + G * (a + 1))


def draw(seed, j, n_any):
    """U(j)"""
    return mix(block_key(seed, j >> 6) + G * (n_any + 1 + (j & 63)))


def variant_count(space):
    """V: the product of the variation radices (3 for 'any?', else 2)."""
    v = 1
    for _, rc in space.fixed_var.tolist():
        v *= 3 if rc == 3 else 2
    for _, _, rc in space.pert_var.tolist():
        v *= 3 if rc == 3 else 2
    return v


def sample(seed, j, n_any, V):
    """-> (bits of the 'any' nodes in their order, variant number) of sample j."""
    b, lane = j >> 6, j & 63
    return [(any_word(seed, b, a) >> lane) & 1 for a in range(n_any)], (draw(seed, j, n_any) * V) >> 64


def flat_index(seed, j, n_any, V):
    bits, variant = sample(seed, j, n_any, V)
    return sum(bit << a for a, bit in enumerate(bits)) | (variant << n_any)


def sample_indices(space, seed, samples):
    """Flat problem indices I(j) of the listed sample numbers."""
    n_any, V = len(space.any_nodes), variant_count(space)
    return [flat_index(seed, int(j), n_any, V) for j in samples]


def column_word(seed, j0, a, n_bits):
    """The 32-bit word of samples j0 .. j0 + 31 for 'any' ordinal a with n_bits valid bits, bit by bit from the definition."""
    return sum(((any_word(seed, (j0 + i) >> 6, a) >> ((j0 + i) & 63)) & 1) << i for i in range(n_bits))


# ---- whole arrays of generator words (for the statistics) ------------------------------------------------------------

def mix_np(z):
    z = z.astype(np.uint64)
    with np.errstate(over='ignore'):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def any_words_np(seed, n_blocks, n_any, first_block=0):
    """uint64[n_blocks, n_any]: A(first_block + b, a)."""
    with np.errstate(over='ignore'):
        b = np.arange(first_block + 1, first_block + n_blocks + 1, dtype=np.uint64)
        kb = mix_np(np.uint64(key0(seed)) + np.uint64(G) * b)
        a = np.arange(1, n_any + 1, dtype=np.uint64)
        return mix_np(kb[:, None] + np.uint64(G) * a[None, :])
