"""Cases, the algorithm's oracle and the bounds of the device eigenvalue solver (``_ops.eigsh_restarted``,
``LinearOperator.eigenvals`` / ``singularvals``).

The reference of every case is the exact spectrum: ``numpy.linalg.eigvalsh`` of the dense fp64 symmetric matrix S
whose eigenvalues are sought -- the operator's own matrix for ``eigenvals``, the smaller Gram matrix for
``singularvals`` (singular values are compared through their squares).  ``spectral_ref`` is a NumPy restatement
of the thick-restart Lanczos of ``_ops.eigsh_restarted`` on a dense matrix: the algorithm's oracle, itself held
to the same bound as SciPy's ``eigsh`` (tests/test_spectral_host.py).

The bound on a computed eigenvalue ``theta`` of exact value ``lam``:

    |theta - lam| <= tol_eff max(|lam|, eps^(2/3)) + C eps_apply ||S||_2          tol_eff = tol or eps

The first term is the Ritz residual bound |theta - lam| <= ||r|| at the convergence criterion; ``eps_apply`` is the
epsilon of the dtype the operator computes in.  C is measured, not chosen: over every case and every ``which`` at
tol = 0, (|err| - first term) / (eps ||S||) came to at most RATIO_REF for ``spectral_ref`` and RATIO_SCIPY for
SciPy's ``eigsh`` (printed by test_spectral_host.py::test_measured_ratios, which also asserts that the constants
below still cover them); C is 8 x the larger, rounded up to a power of two.  The factor 8 covers the different
summation order of the device kernels and the stencil and CSR applications against a dense matvec.

ORTH_BOUND, the bar on ||V V^T - I||_max after 20 steps on ``sym_dense``, is set the same way: 8 x the figure of
``spectral_ref``'s own basis, ORTH_REF.

No case has a wanted eigenvalue of exact multiplicity except the breakdown cases (``conv1d_doc``, ``homothety``,
``zeros_sym``): ``separation`` states it on the exact spectrum.
"""

import functools

import numpy as np

from tests.views import conv1d_np, conv2d_np, pycsou_offset, rounded

EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
RATIO_REF, RATIO_SCIPY = 32.7, 42.8    # measured: see the module docstring (grad2d LM both)
C = 512.0                              # 8 x 42.8 = 342.4, rounded up to a power of two
ORTH_REF = 1.5e-15                     # measured: ||V V^T - I||_max of ref_basis(sym_dense, 20)
ORTH_BOUND = 8 * ORTH_REF
TOLS = (0.0, 1e-6)
WHICH_EIG = ('LM', 'LA', 'SA', 'BE')
GRAM_WHICH = {'LM': 'LA', 'SM': 'SA'}
BREAKDOWN_CASES = ('conv1d_doc', 'homothety', 'zeros_sym')

# name -> (kind, k, the values of `which`)
CASES = {
    'sym_dense': ('eig', 4, WHICH_EIG),
    'gauss_tall': ('svd', 3, ('LM', 'SM')),
    'gauss_wide': ('svd', 3, ('LM', 'SM')),
    'grad2d': ('svd', 6, ('LM', 'SM')),
    'grad2d_gram': ('eig', 6, ('LA', 'SA')),
    'conv1d_doc': ('svd', 3, ('LM',)),
    'homothety': ('eig', 3, WHICH_EIG),
    'zeros_sym': ('eig', 3, WHICH_EIG),
    'tiny': ('eig', 2, WHICH_EIG),
    'conv2d_f32': ('svd', 6, ('LM',)),
}
COMBOS = [(name, which) for name, (_, _, whiches) in CASES.items() for which in whiches]
GRAD_SHAPE, GRAD_STEPS = (40, 37), (1.0, 0.8)
CONV2D_SHAPE, CONV2D_PSF = (32, 24), (5, 3)


def doc_filter():
    """The half-zeroed 5-tap Hann window of the reference's doctest (core/linop.py:262-266)."""
    from scipy import signal
    filt = signal.windows.hann(5)
    filt[filt.size // 2:] = 0
    return filt


def conv2d_psf():
    h = np.random.default_rng([61, 5, 3]).uniform(0.1, 1.0, CONV2D_PSF)
    return rounded(h / h.sum(), np.float32)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The dense fp64 matrix A of the case's operator."""
    rng = np.random.default_rng([59, len(name)])
    if name == 'sym_dense':
        Q, _ = np.linalg.qr(rng.standard_normal((300, 300)))
        lam = np.concatenate([np.linspace(-3.0, -1.0, 150), np.linspace(0.05, 4.0, 150)])
        A = (Q * lam) @ Q.T
        return (A + A.T) / 2
    if name == 'gauss_tall':
        return rounded(rng.standard_normal((120, 80)) / np.sqrt(120), np.float32)
    if name == 'gauss_wide':
        return rounded(rng.standard_normal((80, 120)) / np.sqrt(120), np.float32)
    if name in ('grad2d', 'grad2d_gram'):
        from oracle import pylops1 as P
        g = P.Gradient(GRAD_SHAPE, sampling=list(GRAD_STEPS), edge=True, kind='forward')
        G = np.stack([g.matvec(e) for e in np.eye(int(np.prod(GRAD_SHAPE)))], axis=1)
        return G if name == 'grad2d' else G.T @ G
    if name == 'conv1d_doc':
        filt = doc_filter()
        eye = np.eye(30)
        return np.stack([conv1d_np(eye[j], filt, pycsou_offset(filt.size), 0) for j in range(30)], axis=1)
    if name == 'homothety':
        return 2.0 * np.eye(50)
    if name == 'zeros_sym':
        return np.zeros((40, 40))
    if name == 'tiny':
        B = rng.standard_normal((5, 5))
        return (B + B.T) / 2
    if name == 'conv2d_f32':
        n0, n1 = CONV2D_SHAPE
        h = conv2d_psf()
        eye = np.eye(n0 * n1)
        return np.stack([conv2d_np(eye[j].reshape(n0, n1), h, pycsou_offset(5), pycsou_offset(3)).ravel()
                         for j in range(n0 * n1)], axis=1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def sym(name):
    """S: the symmetric matrix whose eigenvalues the case asks for (the smaller Gram matrix of an svd case)."""
    A = matrix(name)
    if CASES[name][0] == 'eig':
        return A
    return A.T @ A if A.shape[0] >= A.shape[1] else A @ A.T


@functools.lru_cache(maxsize=None)
def spectrum(name):
    return np.linalg.eigvalsh(sym(name))


def eps_apply(name):
    return EPS32 if name == 'conv2d_f32' else EPS


def case_tol(name, tol):
    """conv2d_f32 runs at tol = 1e-4 whatever the sweep says (and for its largest values only: the smallest
    singular values of a blur are clustered at zero, thousands of restarts for the oracle and for ARPACK)."""
    return 1e-4 if name == 'conv2d_f32' else tol


def select(lam, k, which):
    """Ascending indices of the wanted values of the ascending spectrum `lam` (ARPACK's conventions)."""
    m = len(lam)
    if which == 'LA':
        idx = np.arange(m - k, m)
    elif which == 'SA':
        idx = np.arange(k)
    elif which == 'LM':
        idx = np.argsort(np.abs(lam), kind='stable')[m - k:]
    elif which == 'BE':
        idx = np.concatenate([np.arange(k // 2), np.arange(m - (k - k // 2), m)])
    else:
        raise KeyError(which)
    return np.sort(idx)


def gram_which(name, which):
    """`which` of the eigenproblem on S."""
    return which if CASES[name][0] == 'eig' else GRAM_WHICH[which]


def wanted(name, which):
    lam = spectrum(name)
    return lam[select(lam, CASES[name][1], gram_which(name, which))]


def first_term(name, which, tol):
    tol_eff = tol if tol else EPS
    return tol_eff * np.maximum(np.abs(wanted(name, which)), EPS ** (2.0 / 3.0))


def bound(name, which, tol, c=None):
    """Per wanted eigenvalue of S."""
    c = C if c is None else c
    return first_term(name, which, tol) + c * eps_apply(name) * max(float(np.abs(spectrum(name)).max()), 0.0)


def ratio(name, which, tol, got):
    """(|err| - first term) / (eps ||S||), the largest over the wanted values (0 for the zero matrix when exact)."""
    err = np.abs(np.sort(np.asarray(got, dtype=np.float64)) - wanted(name, which)) - first_term(name, which, tol)
    nrm = float(np.abs(spectrum(name)).max())
    if nrm == 0.0:
        return 0.0 if np.all(err <= 0) else float('inf')
    return float(np.max(err) / (EPS * nrm))


def separation(name, which, tol):
    """The smallest gap between a wanted value and any other eigenvalue, in units of the bound."""
    lam = spectrum(name)
    idx = select(lam, CASES[name][1], gram_which(name, which))
    bnd = bound(name, which, tol)
    worst = np.inf
    for j, i in enumerate(idx):
        others = np.delete(lam, i)
        worst = min(worst, float(np.min(np.abs(others - lam[i])) / bnd[j]))
    return worst


def make_op(name):
    """The device operator of a case."""
    import scipy.sparse as sp
    from pycsou_amd.linop import Convolve1D, Convolve2D, DenseLinearOperator, Gradient, HomothetyMap, \
        SparseLinearOperator
    if name in ('sym_dense', 'zeros_sym', 'tiny'):
        return DenseLinearOperator(matrix(name), is_symmetric=True)
    if name in ('gauss_tall', 'gauss_wide'):
        return DenseLinearOperator(matrix(name))
    if name == 'grad2d':
        return Gradient(GRAD_SHAPE, step=GRAD_STEPS, kind='forward')
    if name == 'grad2d_gram':
        return SparseLinearOperator(sp.csr_matrix(matrix(name)), is_symmetric=True)
    if name == 'conv1d_doc':
        return Convolve1D(size=30, filter=doc_filter())
    if name == 'homothety':
        return HomothetyMap(size=50, constant=2.0)
    if name == 'conv2d_f32':
        return Convolve2D(size=int(np.prod(CONV2D_SHAPE)), filter=conv2d_psf(), shape=CONV2D_SHAPE, dtype='float32')
    raise KeyError(name)


def public_call(op, name, which, **kw):
    """eigenvals / singularvals of the case through the public interface; eigenvalues of S back."""
    kind, k, _ = CASES[name]
    if kind == 'eig':
        return np.asarray(op.eigenvals(k, which=which, **kw), dtype=np.float64)
    return np.asarray(op.singularvals(k, which=which, **kw), dtype=np.float64) ** 2


# ---------------------------------------------------------------- the algorithm's oracle (NumPy)

def _cgs2(V, s, w, brk):
    """One step's orthogonalisation: (h1 + h2, beta, omega, row s + 1), beta = 0 on a breakdown."""
    Vs = V[:s + 1]
    before = float(w @ w)
    h1 = Vs @ w
    w = w - h1 @ Vs
    h2 = Vs @ w
    w = w - h2 @ Vs
    h3 = Vs @ w
    b = float(np.sqrt(w @ w))
    if b <= brk * np.sqrt(before):
        return h1 + h2, 0.0, 0.0, np.zeros_like(w)
    return h1 + h2, b, float(np.max(np.abs(h3)) / b), w / b


def ref_basis(S, steps, v0=None):
    """The basis after `steps` Lanczos steps with CGS2 on the dense matrix S, rows 0..steps."""
    n = S.shape[0]
    V = np.zeros((steps + 1, n))
    q = np.random.default_rng(0).standard_normal(n) if v0 is None else np.asarray(v0, dtype=np.float64)
    V[0] = q / np.linalg.norm(q)
    for s in range(steps):
        V[s + 1] = _cgs2(V, s, S @ V[s], 8.0 * EPS * np.sqrt(n))[3]
    return V


def spectral_ref(S, k, which, ncv=None, tol=0, maxiter=None, v0=None):
    """``_ops.eigsh_restarted`` restated in NumPy on the dense symmetric matrix S: (ascending values, restarts)."""
    from scipy.sparse.linalg import ArpackNoConvergence
    n = S.shape[0]
    assert 0 < k < n
    m = int(ncv) if ncv is not None else min(n, max(2 * k + 1, 20))
    assert k < m <= n
    rng = np.random.default_rng(0)
    q = rng.standard_normal(n) if v0 is None else np.asarray(v0, dtype=np.float64)
    V = np.zeros((m + 1, n))
    V[0] = q / np.linalg.norm(q)
    brk = 8.0 * EPS * np.sqrt(n)
    tol_eff = tol if tol else EPS
    maxiter = 10 * n if maxiter is None else maxiter
    H, beta = np.zeros((m, m)), np.zeros(m)
    j0, restarts = 0, 0
    while True:
        s = j0
        while s < m:
            c, beta[s], _, V[s + 1] = _cgs2(V, s, S @ V[s], brk)
            H[:s + 1, s] = c
            H[s, :s + 1] = c
            if beta[s] == 0.0 and s < m - 1:      # breakdown: a random row, orthogonalised twice, zero coupling
                b, V[s + 1] = _cgs2(V, s, rng.standard_normal(n), brk)[1::2]
                assert b > 0.0
            s += 1
        theta, Y = np.linalg.eigh(H)
        res = np.abs(beta[m - 1] * Y[m - 1])
        bar = np.maximum(tol_eff * np.maximum(EPS ** (2.0 / 3.0), np.abs(theta)), 8.0 * EPS * np.abs(theta).max())
        want = select(theta, k, which)
        conv = res[want] <= bar[want]
        if conv.all():
            return theta[want], restarts
        if restarts >= maxiter:
            raise ArpackNoConvergence(f'{int(conv.sum())} of {k} converged', theta[want][conv], None)
        keep = min(k + min(int(conv.sum()), (m - k) // 2), m - 1)
        idx = select(theta, keep, which)
        V[:keep] = Y[:, idx].T @ V[:m]
        V[keep] = V[m]
        H[:] = 0.0
        H[np.arange(keep), np.arange(keep)] = theta[idx]
        j0, restarts = keep, restarts + 1


# ---------------------------------------------------------------- the exact one-launch data

ONE_N = (1, 2, 255, 256, 257, 1000)
# s + 1: around the row-group size of pcs_orth_dots (8) and every size at which pcs_orth_update changes kernel
# (rows held in registers: 8, 16, 24; more: the second read)
ROWS = (1, 2, 7, 8, 9, 16, 17, 20, 24, 25, 41)
GROUP, TILE, CAP = 8, 512, 1024
BIG_N = CAP * TILE + 3                  # the grid-stride loop takes a second pass


def one_launch(n, rows, pad, seed=0):
    """(V (rows + 1, n + pad) with the row stride n + pad, w, h_in): V, w in {-3..3}, h_in multiples of 1/2 in
    [-2, 2]; the padding columns of V hold 7 (never read)."""
    rng = np.random.default_rng([67, n, rows, pad, seed])
    V = np.full((rows + 1, n + pad), 7.0)
    V[:, :n] = rng.integers(-3, 4, (rows + 1, n))
    w = rng.integers(-3, 4, n).astype(np.float64)
    h_in = rng.integers(-4, 5, rows + 1) / 2.0
    return V, w, h_in


def dots_ref(V, w, n, rows):
    return np.concatenate([V[:rows, :n] @ w, [w @ w]])


def update_ref(V, w, h_in, n, rows):
    wn = w - h_in[:rows] @ V[:rows, :n]
    return wn, dots_ref(V, wn, n, rows)
