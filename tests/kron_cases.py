"""Seeded cases and fresh NumPy definitions for KroneckerProduct, KroneckerSum, KhatriRaoProduct, BlockOperator and
BlockDiagonalOperator (pycsou/linop/base.py:339-548, 715-989).  Shared by tests/golden/make_golden_kron.py (the real
reference runs on these inputs) and by the tests, which regenerate the inputs instead of storing them.

With linop1 = A (k x l) and linop2 = B (n x m), written here and not taken from the reference:
  KroneckerProduct(A, B)  = np.kron(B, A)                      (vec in C order: K x = (B X A^T).ravel())
  KroneckerSum(A, B)      = kron(I_m, A) + kron(B, I_l)        (square A and B)
  KhatriRaoProduct(A, B)  = [kron(B[:, c], A[:, c]) for c]     (columns)
  BlockOperator           = np.block
"""

import numpy as np
import scipy.sparse as sp

from tests.sparse_cases import forward_difference_matrix, make_ints, make_vec  # noqa: F401  (shared generators)


# ---------------------------------------------------------------- the definitions
def kron_matrix(A, B):
    return np.kron(B, A)


def ksum_matrix(A, B):
    return np.kron(np.eye(B.shape[0]), A) + np.kron(B, np.eye(A.shape[0]))


def khatri_rao_matrix(A, B):
    return np.stack([np.kron(B[:, c], A[:, c]) for c in range(A.shape[1])], axis=1)


def d2_matrix(n, step=1.0):
    """The second-difference matrix with one-sided second-order end rows (SecondDerivative with edge=True)."""
    M = np.zeros((n, n))
    for i in range(1, n - 1):
        M[i, i - 1:i + 2] = [1.0, -2.0, 1.0]
    M[0, :3] = [1.0, -2.0, 1.0]
    M[-1, -3:] = [1.0, -2.0, 1.0]
    return M / step ** 2


def d1_matrix(n, step=1.0):
    """The forward-difference matrix, last row zero (FirstDerivative with kind='forward')."""
    M = np.zeros((n, n))
    for i in range(n - 1):
        M[i, i:i + 2] = [-1.0, 1.0]
    return M / step


def conv_matrix(n, h, off):
    """Zero-padded 1-D convolution with the filter's origin at index ``off``: y[i] = sum_t h[t] x[i + off - t]."""
    M = np.zeros((n, n))
    for i in range(n):
        for t, v in enumerate(h):
            j = i + off - t
            if 0 <= j < n:
                M[i, j] = v
    return M


# ---------------------------------------------------------------- factors
def dense(shape, seed):
    return np.random.default_rng([21, int(seed)]).standard_normal(shape)


def sparse(shape, seed, density=0.4):
    """A CSR factor with an empty row and an empty column left in."""
    rng = np.random.default_rng([22, int(seed)])
    M = rng.standard_normal(shape) * (rng.random(shape) < density)
    M[shape[0] // 2, :] = 0.0
    M[:, shape[1] // 3] = 0.0
    return sp.csr_matrix(M)


def diag_values(n, seed):
    return np.random.default_rng([23, int(seed)]).standard_normal(n)


# pairs recorded from the reference: name -> (kind of linop1, kind of linop2); matrices by ``pair_matrices``
KRON_PAIRS = ('dense', 'sparse', 'deriv2', 'diag_dense')
DOCTEST_NV, DOCTEST_NH = 11, 21


def pair_matrices(name, square=False):
    """Dense matrices (A, B) of linop1 and linop2 of a recorded pair; ``square``: the KroneckerSum variant."""
    if name == 'dense':
        return (dense((5, 5), 0), dense((4, 4), 1)) if square else (dense((5, 7), 0), dense((4, 3), 1))
    if name == 'sparse':
        shapes = ((6, 6), (5, 5)) if square else ((6, 8), (5, 4))
        return sparse(shapes[0], 2).toarray(), sparse(shapes[1], 3).toarray()
    if name == 'deriv2':
        return d2_matrix(DOCTEST_NH), d2_matrix(DOCTEST_NV)
    if name == 'diag_dense':
        return np.diag(diag_values(6, 4)), dense((4, 4), 5) if square else dense((4, 3), 5)
    raise KeyError(name)


def build_pair(name, mod_base, mod_diff, square=False):
    """The two operators of a recorded pair from a package's ``linop.base`` / ``linop.diff`` modules (the
    reference's or this project's)."""
    A, B = pair_matrices(name, square)
    if name == 'dense':
        return mod_base.DenseLinearOperator(A), mod_base.DenseLinearOperator(B)
    if name == 'sparse':
        return mod_base.SparseLinearOperator(sp.csr_matrix(A)), mod_base.SparseLinearOperator(sp.csr_matrix(B))
    if name == 'deriv2':
        return mod_diff.SecondDerivative(size=DOCTEST_NH), mod_diff.SecondDerivative(size=DOCTEST_NV)
    return mod_base.DiagonalOperator(np.diag(A).copy()), mod_base.DenseLinearOperator(B)


def pair_inputs(A, B, seed=0):
    """(x, y) for the Kronecker operators of A (k x l) and B (n x m)."""
    return make_vec(B.shape[1] * A.shape[1], seed), make_vec(B.shape[0] * A.shape[0], seed + 1)


KR_DENSE = ((5, 7), (4, 7))            # A, B of the recorded dense Khatri-Rao pair (l = 7)
KR_DOCTEST_N = 11


def kr_dense_pair():
    return dense(KR_DENSE[0], 6), dense(KR_DENSE[1], 7)


# fused-kernel cases (k, n, l); the last two are the slab-crossing integer case and the one above the limit
KR_FUSED = [(1, 1, 1), (3, 2, 5), (5, 4, 7), (32, 32, 300), (33, 17, 257)]
KR_SLABS = (8, 6, 64 * 7 + 5)          # several column slabs (and, at 512 groups, one slab per workgroup)
KR_ABOVE = (33, 32, 130)               # k n = 1056 > 1024: the composed route


def make_int_matrix(shape, seed):
    """Weights in {+-1, +-0.5}: products with integers in {-3..3} sum exactly in fp32 and fp64."""
    return np.random.default_rng([24, int(seed)]).choice([1.0, -1.0, 0.5, -0.5], size=shape)


# ---------------------------------------------------------------- the solver trajectory
PDS_SHAPE, PDS_ITERS, PDS_LAM = (24, 30), 30, 0.05


def blur_matrix(n, sigma, half=3):
    """A dense Gaussian blur with zero boundary: row i holds exp(-(i - j)^2 / (2 sigma^2)), |i - j| <= half,
    normalised by the full kernel's sum."""
    t = np.arange(-half, half + 1)
    h = np.exp(-t ** 2 / (2.0 * sigma ** 2))
    return conv_matrix(n, h / h.sum(), half)


def pds_problem():
    """A piecewise-constant 24 x 30 image blurred by KroneckerProduct(A_h, B_v) (A_h along the rows' 30 samples,
    B_v along the 24 rows), plus noise: returns (A_h, B_v, data)."""
    rng = np.random.default_rng(51)
    n0, n1 = PDS_SHAPE
    img = np.zeros(PDS_SHAPE)
    img[4:14, 5:20] = 1.0
    img[10:20, 12:26] += 0.5
    Ah, Bv = blur_matrix(n1, 1.2), blur_matrix(n0, 0.8)
    y = (Bv @ img @ Ah.T).ravel() + 0.02 * rng.standard_normal(n0 * n1)
    return Ah, Bv, y


# ---------------------------------------------------------------- block layouts
def block_layout(mod_diff):
    """The reference doctest's 2 x 3 layout on an (Nv, Nh) = (11, 21) grid (base.py:371-379): second derivatives
    along both axes and scaled copies; returns (rows of operators, rows of dense matrices)."""
    nv, nh = DOCTEST_NV, DOCTEST_NH
    N = nv * nh
    D2h = mod_diff.SecondDerivative(size=N, shape=(nv, nh), axis=1)
    D2v = mod_diff.SecondDerivative(size=N, shape=(nv, nh), axis=0)
    Mh, Mv = np.kron(np.eye(nv), d2_matrix(nh)), np.kron(d2_matrix(nv), np.eye(nh))
    ops = [[D2v, 0.5 * D2v, -1 * D2h], [D2h, 2 * D2h, D2v]]
    mats = [[Mv, 0.5 * Mv, -Mh], [Mh, 2 * Mh, Mv]]
    return ops, mats
