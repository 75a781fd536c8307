"""Cases, references and bounds of the pseudo-inverse tests (tests/test_pinv_host.py, tests/test_gpu_pinv.py).

The contract of ``LinearOperator.pinv`` is ``scipy.sparse.linalg.cg`` on N x = b with N = A^T A + eps^2 I and
b = A^T y (PyLops 1.x ``NormalEquationsInversion`` only forwards to it).  ``cg_ref`` is that loop line by line in
NumPy; it also returns what SciPy does not: the residual norm after every iteration and the iteration count.

The error bound of the solver tests (``bound``).  CG stops with a recurrence residual ||r|| < tol = rtol ||b||
(atol = 0).  b = A^T y lies in the row space of A, which N maps into itself, so from x0 = 0 every iterate, every
residual and x* lie there too; on that subspace the eigenvalues of N are sigma_i^2 + eps^2 over the nonzero
singular values of A, hence

    ||x - x*|| = ||N^-1 r|| <= ||r|| / (sigma_min^2 + eps^2) < rtol ||A^T y|| / (sigma_min^2 + eps^2),

sigma_min the smallest nonzero singular value of A.  x* is the least-squares solution of the stacked
system [A; eps I] x = [y; 0] (``np.linalg.lstsq``: the minimum-norm one when eps = 0).  Nothing in the bound is
measured on the code under test.

The exact data of the one-launch tests (``exact_vectors``): entries in {-3..3}, eps2 = 1/4, alpha = beta = 1/2,
so every element the kernels form is a multiple of 1/8 below 8 and every summand a multiple of 1/64: all sums are
exact in fp64 in any order (``tests.scratch.assert_exact`` with bits = 53), and the per-system scalars are
single correctly rounded IEEE operations (a division, a square root) on exact operands.
"""

import numpy as np
import scipy.sparse as sp

from tests.views import conv1d_np, pycsou_offset, rounded

RTOL = 1e-5
CASES = ('tall', 'wide_eps', 'wide', 'sparse', 'conv1d', 'one', 'zero_rhs')
NORM_MAX = 10.0


def cg_ref(N, b, rtol=RTOL, atol=0.0, maxiter=None, x0=None):
    """``scipy.sparse.linalg.cg(N, b, x0, rtol=rtol, atol=atol, maxiter=maxiter)`` (SciPy 1.15, no
    preconditioner) for a dense matrix N: (x, info, iterations, [||r|| after each iteration])."""
    N = np.asarray(N)
    b = np.asarray(b, dtype=np.float64).ravel()
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64).ravel()
    bnrm2 = np.linalg.norm(b)
    atol = max(float(atol), float(rtol) * float(bnrm2))
    if bnrm2 == 0:
        return b, 0, 0, []
    n = len(b)
    if maxiter is None:
        maxiter = n * 10
    r = b - N.dot(x) if x.any() else b.copy()
    rho_prev, p = None, None
    hist, it = [], 0
    for iteration in range(maxiter):
        if np.linalg.norm(r) < atol:
            return x, 0, it, hist
        z = r
        rho_cur = np.dot(r, z)
        if iteration > 0:
            beta = rho_cur / rho_prev
            p *= beta
            p += z
        else:
            p = np.empty_like(r)
            p[:] = z[:]
        q = N.dot(p)
        alpha = rho_cur / np.dot(p, q)
        x += alpha * p
        r -= alpha * q
        rho_prev = rho_cur
        it += 1
        hist.append(float(np.linalg.norm(r)))
    return x, maxiter, it, hist


def _gauss(m, n, seed):
    """Gaussian entries of variance 1 / m, rounded to fp32 (the same matrix in both dtypes): ||A|| is about
    1 + sqrt(n / m), the condition number that of the unscaled matrix."""
    return rounded(np.random.default_rng([41, m, n, seed]).standard_normal((m, n)) / np.sqrt(m), np.float32)


def _rhs(m, seed, k=3):
    return rounded(np.random.default_rng([43, m, seed]).standard_normal((k, m)), np.float32)


def conv1d_matrix(n, taps):
    """The matrix of Convolve1D(n, taps) (zero boundary, pycsou's centring)."""
    eye = np.eye(n)
    return np.stack([conv1d_np(eye[j], np.asarray(taps, dtype=np.float64), pycsou_offset(len(taps)), 0)
                     for j in range(n)], axis=1)


def case(name):
    """{'A': dense fp64 matrix, 'eps', 'Y': (3, m) right-hand sides, 'kind': how make_op builds the operator}."""
    if name == 'tall':
        c = {'A': _gauss(48, 32, 0), 'eps': 0.0, 'Y': _rhs(48, 0), 'kind': 'dense'}
    elif name == 'wide_eps':
        c = {'A': _gauss(32, 48, 1), 'eps': 0.5, 'Y': _rhs(32, 1), 'kind': 'dense'}
    elif name == 'wide':
        c = {'A': _gauss(32, 48, 1), 'eps': 0.0, 'Y': _rhs(32, 2), 'kind': 'dense'}
    elif name == 'sparse':
        M = sp.random(60, 40, density=0.15, format='csr', random_state=np.random.default_rng([47, 60, 40]),
                      data_rvs=lambda k: rounded(np.random.default_rng([53, k]).standard_normal(k), np.float32))
        c = {'A': M.toarray(), 'eps': 0.25, 'Y': _rhs(60, 3), 'kind': 'sparse'}
    elif name == 'conv1d':
        c = {'A': conv1d_matrix(64, CONV_TAPS), 'eps': 0.1, 'Y': _rhs(64, 4), 'kind': 'conv1d'}
    elif name == 'one':
        c = {'A': np.array([[2.0]]), 'eps': 0.0, 'Y': np.array([[3.0], [-0.5], [1.25]]), 'kind': 'dense'}
    elif name == 'zero_rhs':
        Y = _rhs(48, 5)
        Y[1] = 0.0
        c = {'A': _gauss(48, 32, 0), 'eps': 0.0, 'Y': Y, 'kind': 'dense'}
    else:
        raise KeyError(name)
    c['name'] = name
    assert np.linalg.norm(c['A'], 2) <= NORM_MAX
    return c


CONV_TAPS = (0.25, 0.5, 0.25)


def make_op(c, dtype):
    """The device operator of a case in `dtype`."""
    from pycsou_amd.linop import Convolve1D, DenseLinearOperator, SparseLinearOperator
    if c['kind'] == 'dense':
        return DenseLinearOperator(c['A'].astype(dtype))
    if c['kind'] == 'sparse':
        return SparseLinearOperator(sp.csr_matrix(c['A'].astype(dtype)))
    return Convolve1D(c['A'].shape[1], np.asarray(CONV_TAPS), dtype=np.dtype(dtype).name)


def normal_system(c, j=0):
    """(N, b) of right-hand side j, dense fp64."""
    A = c['A']
    return A.T @ A + c['eps'] ** 2 * np.eye(A.shape[1]), A.T @ c['Y'][j]


def sigma_min(A):
    """The smallest nonzero singular value (NumPy's rank convention), 0 for a zero matrix."""
    s = np.linalg.svd(A, compute_uv=False)
    s = s[s > max(A.shape) * np.finfo(np.float64).eps * s[0]] if s.size and s[0] > 0 else s[:0]
    return float(s[-1]) if s.size else 0.0


def lam_min(c):
    """The smallest eigenvalue of N on the row space of A: sigma_min^2 + eps^2."""
    return sigma_min(c['A']) ** 2 + c['eps'] ** 2


def solution(c, j=0):
    """x* of right-hand side j: least squares on the stacked system [A; eps I] x = [y; 0]."""
    A, eps = c['A'], c['eps']
    n = A.shape[1]
    S = np.vstack([A, eps * np.eye(n)])
    return np.linalg.lstsq(S, np.concatenate([c['Y'][j], np.zeros(n)]), rcond=None)[0]


def bound(c, j=0, rtol=RTOL):
    """The module docstring's bound on ||x - x*|| for right-hand side j."""
    return rtol * float(np.linalg.norm(c['A'].T @ c['Y'][j])) / lam_min(c)


# ---------------------------------------------------------------- exact data of the one-launch tests

EPS2, ALPHA, BETA = 0.25, 0.5, 0.5
CAP = 1024                                    # PCS_CG_MAX_BLOCKS: asserted against the library by the tests
ONE_LAUNCH_N = (1, 63, 64, 65, 255, 256, 257, CAP * 256 + 1)
ONE_LAUNCH_NB = (1, 3)


def exact_vectors(n, nb):
    """x, r, p, q of shape (nb, n) with entries in {-3..3}; p has no zero and q the sign of p, so that
    pq_j = sum p (q + eps2 p) >= eps2 sum p^2 > 0 for every system."""
    rng = np.random.default_rng([59, n, nb])
    x, r, p, q = (rng.integers(-3, 4, (nb, n)).astype(np.float64) for _ in range(4))
    p[p == 0] = 1.0
    q = np.abs(q) * np.sign(p)
    return x, r, p, q


def dir_ref(r, p, beta=BETA, first=False):
    return r.copy() if first else beta * p + r


def dot_terms(p, q, eps2=EPS2):
    """The summands of pq_j."""
    return p * (q + eps2 * p)


def update_ref(x, r, p, q, alpha=ALPHA, eps2=EPS2):
    """(x', r', the summands of rho')."""
    rn = r - alpha * (q + eps2 * p)
    return x + alpha * p, rn, rn * rn
