"""What the CPU and the GPU tests of sc_gkr_layers_eval_batch (GKRRoundSumcheck.evaluate_layers_batch) share: the inputs, the definition in
big integers, and the inequality each case rests on.

The definition.  Layer k of an instance is a list of non-zeros (index, v), index = z | x << dim | y << 2 dim, and
    W_k[z] = sum over the list of  v * A[x] * B[y]  mod p,     (A, B) = (f2, f3) for k = 0, (W_{k-1}, W_{k-1}) for k >= 1;
repeated indices add up, the list's order does not matter, a zero value is an ordinary term.  define_layer / define_layers compute exactly
that over python integers (canonical values, Montgomery form taken off and put on by oracle/cref.py's converters) -- nothing of the library.

The plans (sumcheck_amd/csrc/batch_shape.hpp, read here as the other *_cases.py modules read their limits):
    batch.gkr_eval_layers_one_block   dim <= MAX_DIM and every nnz <= MAX_NNZ_PER_CELL << dim, policy "batch" != 0
    batch.gkr_eval_cells              every other shape
The lanes.  A term's limb is below 2^32, so a lane of a cell that takes t terms stays below t * 2^32: 64 * 2^9 terms in one cell -- the
fullest state the one-block plan admits -- reach 2^47, the 70 000 terms of the cells plan's fullest case 2^49, both far below the 2^63
wide_fold_cell needs; the call refuses lists of 2^31 non-zeros and more, where the bound would no longer hold."""
import os
import re

import numpy as np

from oracle import cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cref.P
ONE_BLOCK, CELLS = "batch.gkr_eval_layers_one_block", "batch.gkr_eval_cells"
NAME = "sc_gkr_layers_eval_batch"


def _int(pattern):
    text = open(os.path.join(ROOT, "sumcheck_amd", "csrc", "batch_shape.hpp")).read()
    return int(re.search(pattern, text).group(1))


MAX_DIM = _int(r"constexpr int kGkrBatchMaxDim = (\d+);")
MAX_NNZ_PER_CELL = _int(r"constexpr uint64_t kGkrBatchMaxNnzPerCell = (\d+);")
assert (MAX_DIM, MAX_NNZ_PER_CELL) == (9, 64), "the cases below are written for these limits: 64 x 2^9 terms, dim 10 the first beyond"
assert MAX_NNZ_PER_CELL << MAX_DIM < 1 << 31 and 70000 < 1 << 31, "every list of the suite keeps a lane below 2^63"

ONE = cref.ints_to_mont([1])[0]
ZERO = cref.ints_to_mont([0])[0]
MINUS_ONE = cref.ints_to_mont([P - 1])[0]


def one_block_fits(dim, nnz_max):
    return dim <= MAX_DIM and nnz_max <= MAX_NNZ_PER_CELL << dim


def define_layer(idx, vals_int, dim, a_int, b_int):
    """the definition over python integers -> the 2^dim canonical values of the layer"""
    N = 1 << dim
    out = [0] * N
    for i, v in zip(idx, vals_int):
        i = int(i)
        z, x, y = i & (N - 1), (i >> dim) & (N - 1), (i >> (2 * dim)) & (N - 1)
        out[z] = (out[z] + v * a_int[x] * b_int[y]) % P
    return out


def define_layers(layers, f2, f3, dim):
    """layers: per layer (idx, vals) as the library takes them; f2, f3: (2^dim, 4) Montgomery limbs -> per layer the (2^dim, 4) table"""
    a, b = cref.mont_to_ints(f2), cref.mont_to_ints(f3)
    out = []
    for idx, vals in layers:
        w = define_layer(idx, cref.mont_to_ints(vals) if len(idx) else [], dim, a, b)
        out.append(cref.ints_to_mont(w))
        a = b = w
    return out


def sparse_terms(idx, vals_int, dim, a_of, b_of):
    """the definition where a table is too large to list (dim 21): {cell: value} over the list's terms only; a_of(x), b_of(y) give the
    canonical table entries"""
    N = 1 << dim
    out = {}
    for i, v in zip(idx, vals_int):
        i = int(i)
        z, x, y = i & (N - 1), (i >> dim) & (N - 1), (i >> (2 * dim)) & (N - 1)
        out[z] = (out.get(z, 0) + v * a_of(x) * b_of(y)) % P
    return out


def wiring(dim, seed, nnz, variant="random"):
    """(indices, values) of one layer: random (any order), repeated (every index about three times), zeros (half the values zero and kept in
    the list), edge (values from {0, 1, p - 1})"""
    rng = np.random.default_rng(seed)
    if variant == "repeated":
        pool = rng.integers(0, 1 << (3 * dim), size=max(nnz // 3, 1), dtype=np.uint64)
        idx = pool[rng.integers(0, pool.shape[0], size=nnz)]
    else:
        idx = rng.integers(0, 1 << (3 * dim), size=nnz, dtype=np.uint64)
    vals = cref.synth_table(seed, 1, nnz).copy() if nnz else np.zeros((0, 4), np.uint64)
    if variant == "zeros" and nnz:
        vals[::2] = 0
    if variant == "edge" and nnz:
        vals[:] = np.stack([ZERO, ONE, MINUS_ONE])[rng.integers(0, 3, size=nnz)]
    return np.ascontiguousarray(idx), vals


def edge_table(dim, seed):
    """2^dim entries from {0, 1, p - 1}"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([ZERO, ONE, MINUS_ONE])[rng.integers(0, 3, size=1 << dim)])


def one_cell(dim, nnz, z, seed):
    """nnz terms that all land in cell z, every factor p - 1: (p - 1)^3 = -1, so the cell is -nnz mod p and every limb of every term is one
    of p - 1's -- the fullest lanes a list of this length can produce"""
    rng = np.random.default_rng(seed)
    N = 1 << dim
    x, y = rng.integers(0, N, size=nnz, dtype=np.uint64), rng.integers(0, N, size=nnz, dtype=np.uint64)
    idx = np.ascontiguousarray(np.uint64(z) | (x << np.uint64(dim)) | (y << np.uint64(2 * dim)))
    vals = np.ascontiguousarray(np.repeat(MINUS_ONE[None, :], nnz, axis=0))
    table = np.ascontiguousarray(np.repeat(MINUS_ONE[None, :], N, axis=0))
    return idx, vals, table


def circuit(n, dim, n_layers, seed, nnzs, variant="repeated"):
    """n instances of n_layers layers: per instance (layers [(idx, vals)], f2, f3); nnzs[k]: layer k's non-zeros (every instance its own
    wiring)"""
    N = 1 << dim
    return [([wiring(dim, seed + 101 * i + 7 * k, nnzs[k], variant) for k in range(n_layers)], cref.synth_table(seed + 13 * i, 2, N), cref.synth_table(seed + 13 * i, 3, N))
            for i in range(n)]
