"""Seeded cases and fresh NumPy definitions for the sparse / pooling half of pycsou.linop.sampling (Pooling,
NNSampling, MappedDistanceMatrix, SparseLinearOperator; pycsou/linop/sampling.py:394-1058, base.py:121-137).
Shared by tests/golden/make_golden_sparse.py (the real reference runs on these inputs) and by the tests, which
regenerate the inputs instead of storing them.

Definitions written here, not taken from the reference: pooling by pad-and-reshape, unpooling by np.repeat,
nearest neighbours by brute force, the mean-scatter adjoint by np.bincount."""

import numpy as np
import scipy.sparse as sp

# ---------------------------------------------------------------- pooling
POOL_CASES = [((1,), (1,)), ((5,), (8,)), ((65,), (64,)),
              ((4, 6), (2, 3)), ((5, 7), (2, 3)), ((63, 65), (2, 2)), ((64, 64), (10, 20)), ((7, 300), (3, 70)),
              ((9, 4), (1, 4)),
              ((5, 6, 7), (2, 3, 4)), ((3, 4, 5, 6), (2, 2, 2, 4))]
POOL_GOLDEN = [((4, 6), (2, 3)), ((5, 7), (2, 3)), ((5, 6, 7), (2, 3, 4))]     # recorded from the reference
POOL_EXACT = [((64, 64), (2, 4)), ((63, 65), (2, 2)), ((70,), (64,)), ((5, 6, 7), (2, 1, 4)), ((3, 4, 5, 6), (2, 2, 2, 4)),
              ((3, 1100), (1, 512))]                                           # power-of-two blocks, integer data
MODES = ('mean', 'sum')


def tag(shape, block):
    return 'x'.join(map(str, shape)) + '_' + 'x'.join(map(str, block))


def make_vec(n, seed):
    return np.random.default_rng([11, int(seed), int(n)]).standard_normal(int(n))


def make_ints(n, seed):
    return np.random.default_rng([12, int(seed), int(n)]).integers(-3, 4, int(n)).astype(np.float64)


def pooled_shape(shape, block):
    return tuple(-(-n // b) for n, b in zip(shape, block))


def pool(x, shape, block, mode):
    """Pad with zeros to a multiple of the block, reshape to (m0, B0, m1, B1, ...), reduce the block axes; the
    mean divides by the full block size."""
    out = pooled_shape(shape, block)
    a = np.pad(np.asarray(x, dtype=np.float64).reshape(shape), [(0, m * b - n) for n, b, m in zip(shape, block, out)])
    a = a.reshape([v for m, b in zip(out, block) for v in (m, b)])
    s = a.sum(axis=tuple(range(1, 2 * len(shape), 2)))
    return (s / np.prod(block) if mode == 'mean' else s).ravel()


def unpool(y, shape, block):
    """Every cell receives the value of its block (both modes: the reference does not divide)."""
    a = np.asarray(y, dtype=np.float64).reshape(pooled_shape(shape, block))
    for ax, b in enumerate(block):
        a = np.repeat(a, b, axis=ax)
    return a[tuple(slice(0, n) for n in shape)].ravel()


def pool_matrices(shape, block, mode):
    """Dense forward and unpooling matrices from the definitions above."""
    n, m = int(np.prod(shape)), int(np.prod(pooled_shape(shape, block)))
    fwd = np.stack([pool(e, shape, block, mode) for e in np.eye(n)], axis=1)
    adj = np.stack([unpool(e, shape, block) for e in np.eye(m)], axis=1)
    return fwd, adj


# ---------------------------------------------------------------- nearest neighbours
def doctest_nn():
    """sampling.py:556-574."""
    rng = np.random.default_rng(seed=0)
    grid = np.stack(np.meshgrid(np.arange(6), np.arange(4)), axis=-1)
    samples = np.stack((5 * rng.random(size=6), 3 * rng.random(size=6)), axis=-1)
    return samples, grid


REPEAT_SAMPLES = np.array([0.1, 0.2, 2.9, 3.1, 0.05])[:, None]
REPEAT_GRID = np.arange(5.0)[:, None]
REPEAT_Y = np.array([1.0, 2.0, 3.0, 4.0, 6.0])
REPEAT_INDICES = np.array([0, 0, 3, 3, 0])
REPEAT_ADJOINT = np.array([3.0, 0.0, 0.0, 3.5, 0.0])


def mesh_case():
    """300 random 2-D samples on a (non-uniform) 17 x 19 mesh."""
    rng = np.random.default_rng(21)
    gx, gy = np.sort(rng.random(19)) * 4, np.sort(rng.random(17)) * 3
    grid = np.stack(np.meshgrid(gx, gy), axis=-1)
    samples = np.stack((4 * rng.random(300), 3 * rng.random(300)), axis=-1)
    return samples, grid


def brute_nn(samples, grid):
    g = grid.reshape(-1, grid.shape[-1])
    d = np.linalg.norm(samples[:, None, :] - g[None, :, :], axis=-1)
    return np.argmin(d, axis=1), np.min(d, axis=1)


def nn_adjoint(y, idx, size):
    """Mean of the samples that share a neighbour, 0 where there is none."""
    count = np.bincount(idx, minlength=size)
    total = np.bincount(idx, weights=y, minlength=size)
    return np.where(count > 0, total / np.maximum(count, 1), 0.0)


# ---------------------------------------------------------------- mapped distance matrices
SIGMA = 1 / 12


def gauss(x):
    return np.exp(-x ** 2 / (2 * SIGMA ** 2))


ZSIGMA = 1 / 3


def zonal_func(x):
    return np.exp(-np.abs(1 - x) / (ZSIGMA ** 2))


def doctest_mdm():
    """sampling.py:805-830: samples1, samples2, alpha, beta."""
    rng = np.random.default_rng(seed=1)
    samples1, samples2 = np.linspace(0, 2, 10), rng.random(size=3)
    alpha = rng.lognormal(size=samples2.size, sigma=0.5)
    beta = rng.lognormal(size=samples1.size, sigma=0.5)
    return samples1, samples2, alpha, beta


def radial_case():
    """Random 2-D points (no pair sits on max_distance): 200 samples against 40 knots, and the symmetric case."""
    rng = np.random.default_rng(31)
    return 2 * rng.random((200, 2)), 2 * rng.random((40, 2)), 3 * SIGMA


def sphere(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def zonal_case():
    rng = np.random.default_rng(32)
    return sphere(rng, 150), sphere(rng, 30), 3 * ZSIGMA


# ---------------------------------------------------------------- solver trajectories
LASSO_ITERS, LASSO_SAMPLES, LASSO_KNOTS = 40, 256, 64


def lasso_problem():
    """(a) 256 samples in [0, 2] against 64 knots, 5 active Gaussians, noisy data."""
    rng = np.random.default_rng(41)
    samples = np.sort(2 * rng.random(LASSO_SAMPLES))
    knots = np.sort(2 * rng.random(LASSO_KNOTS))
    alpha = np.zeros(LASSO_KNOTS)
    alpha[rng.choice(LASSO_KNOTS, 5, replace=False)] = rng.lognormal(size=5, sigma=0.5)
    noise = 0.01 * rng.standard_normal(LASSO_SAMPLES)
    return samples, knots, alpha, noise


POOL_PDS_SHAPE, POOL_PDS_BLOCK, POOL_PDS_ITERS, POOL_PDS_LAM = (24, 30), (2, 3), 30, 0.1


def forward_difference_matrix(shape):
    """The stacked 2-D forward-difference matrix [D_0; D_1] (last row / column of each difference zero)."""
    n0, n1 = shape

    def d(n):
        m = sp.diags([-np.ones(n), np.ones(n - 1)], [0, 1], shape=(n, n), format='lil')
        m[n - 1, n - 1] = 0.0
        return m.tocsr()

    D = sp.vstack([sp.kron(d(n0), sp.identity(n1)), sp.kron(sp.identity(n0), d(n1))]).tocsr()
    D.eliminate_zeros()
    D.sort_indices()
    return D


def pool_pds_data():
    """(b) a piecewise-constant 24 x 30 image, sum-pooled by (2, 3), plus noise."""
    rng = np.random.default_rng(42)
    img = np.zeros(POOL_PDS_SHAPE)
    img[4:14, 5:20] = 1.0
    img[10:20, 12:26] += 0.5
    y = pool(img.ravel(), POOL_PDS_SHAPE, POOL_PDS_BLOCK, 'sum')
    return y + 0.05 * rng.standard_normal(y.size)


# ---------------------------------------------------------------- CSR matrices for the kernel tests
def csr_from_lengths(lengths, ncols, seed, exact=False):
    """A CSR matrix with the given row lengths, distinct sorted columns per row.  ``exact``: weights in
    {+-1, +-0.5}, to be multiplied with integers in {-3..3}: every partial sum is exact in fp32 and fp64."""
    rng = np.random.default_rng([13, int(seed)])
    lengths = np.asarray(lengths, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    for r, n in enumerate(lengths):
        if n > ncols // 4:
            cols = np.sort(rng.permutation(ncols)[:n])
        else:
            cols = np.unique(rng.integers(0, ncols, 2 * int(n) + 8))[:n] if n else np.empty(0, dtype=np.int64)
            while cols.size < n:
                cols = np.unique(np.concatenate([cols, rng.integers(0, ncols, int(n))]))[:n]
        indices[indptr[r]:indptr[r + 1]] = cols
    if exact:
        data = rng.choice([1.0, -1.0, 0.5, -0.5], size=indices.size)
    else:
        data = rng.standard_normal(indices.size)
    return sp.csr_matrix((data, indices, indptr), shape=(lengths.size, int(ncols)))
