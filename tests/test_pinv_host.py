"""CPU tier of the pseudo-inverse (pycsou/core/linop.py:323-440, 618-629; pycsou/linop/base.py:802-803): the NumPy
reference loop against SciPy's ``cg`` bit for bit, the derived error bound on SciPy's own result, the data
conditions of the exact one-launch cases, the new C-ABI entry points and their argument checks (they run before any
device call), and the shapes and types of the new operators.  No compute calls (no GPU here)."""

import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from tests import pinv_cases as C
from tests import scratch as S
from tests.cases import GOLDEN

NEW_SYMBOLS = ('pcs_cg_state_bytes', 'pcs_cg_nblocks', 'pcs_cg_init', 'pcs_cg_dir', 'pcs_cg_dot', 'pcs_cg_update')


def _scipy(N, b, **kw):
    count = [0]

    def cb(xk):
        count[0] += 1
    x, info = spla.cg(N, b, callback=cb, **kw)
    return x, info, count[0]


# ---------------------------------------------------------------- the reference loop is SciPy's
@pytest.mark.parametrize('name', C.CASES)
def test_cg_ref_is_scipy_cg_bit_for_bit(name):
    c = C.case(name)
    for j in range(c['Y'].shape[0]):
        N, b = C.normal_system(c, j)
        x, info, it = _scipy(N, b, rtol=C.RTOL)
        xr, infor, itr, hist = C.cg_ref(N, b, rtol=C.RTOL)
        print(f'PINV host {name} rhs {j}: {it} iterations, info {info}')
        assert np.array_equal(x, xr) and info == infor == 0 and it == itr == len(hist)
        assert it <= 10 * b.size
        if np.any(b):
            tol = C.RTOL * np.linalg.norm(b)
            assert hist[-1] < tol and all(h >= tol for h in hist[:-1])
        else:
            assert it == 0 and not np.any(x)


@pytest.mark.parametrize('name', [n for n in C.CASES if n != 'one'])      # a 1 x 1 system converges in one iteration
def test_cg_ref_is_scipy_cg_at_maxiter_3(name):
    c = C.case(name)
    N, b = C.normal_system(c, 0)
    x, info, it = _scipy(N, b, rtol=C.RTOL, maxiter=3)
    xr, infor, itr, hist = C.cg_ref(N, b, rtol=C.RTOL, maxiter=3)
    assert np.array_equal(x, xr) and info == infor == 3 and it == itr == 3 == len(hist)


def test_cg_ref_with_x0_and_atol():
    c = C.case('tall')
    N, b = C.normal_system(c, 0)
    x0 = np.linspace(-1.0, 1.0, b.size)
    x, info, it = _scipy(N, b, x0=x0, rtol=1e-8, atol=1e-3)
    xr, infor, itr, _ = C.cg_ref(N, b, rtol=1e-8, atol=1e-3, x0=x0)
    assert np.array_equal(x, xr) and info == infor == 0 and it == itr > 0
    xs = C.cg_ref(N, b)[0]
    assert C.cg_ref(N, b, x0=xs)[2] == 0 == _scipy(N, b, x0=xs, rtol=C.RTOL)[2]      # a converged start: 0 iterations


# ---------------------------------------------------------------- the derived bound
def _cg_f32(N, b, rtol=C.RTOL):
    """The same recurrence with every vector in fp32 and every scalar in fp64 (what the device does in fp32)."""
    f = np.float32
    N, b = N.astype(f), b.astype(f)
    x, r = np.zeros_like(b), b.copy()
    if not np.any(b):
        return x.astype(np.float64)
    tol = rtol * np.linalg.norm(b.astype(np.float64))
    rho, p = float(np.dot(r.astype(np.float64), r.astype(np.float64))), None
    for it in range(10 * b.size):
        if np.sqrt(rho) < tol:
            break
        p = r.copy() if it == 0 else f(beta) * p + r
        q = N @ p
        alpha = rho / float(np.dot(p.astype(np.float64), q.astype(np.float64)))
        x = x + f(alpha) * p
        r = r - f(alpha) * q
        rho_new = float(np.dot(r.astype(np.float64), r.astype(np.float64)))
        beta, rho = rho_new / rho, rho_new
    return x.astype(np.float64)


@pytest.mark.parametrize('name', C.CASES)
def test_bound_holds_for_scipy_and_for_an_fp32_run(name):
    c = C.case(name)
    for j in range(c['Y'].shape[0]):
        N, b = C.normal_system(c, j)
        xs, bnd = C.solution(c, j), C.bound(c, j)
        e64 = np.linalg.norm(spla.cg(N, b, rtol=C.RTOL)[0] - xs)
        e32 = np.linalg.norm(_cg_f32(N, b) - xs)
        print(f'PINV bound {name} rhs {j}: scipy {e64:.3e}, fp32 {e32:.3e}, bound {bnd:.3e}')
        assert e64 <= bnd and e32 <= bnd
        if not np.any(b):
            assert bnd == 0.0 and not np.any(xs)


def test_case_matrices_are_what_the_operators_apply():
    """The sparse case holds entries, the convolution matrix is the three taps on the diagonals."""
    c = C.case('conv1d')
    A = c['A']
    assert np.array_equal(np.diag(A), np.full(64, 0.5)) and np.array_equal(np.diag(A, 1), np.full(63, 0.25))
    assert np.array_equal(A, A.T) and np.count_nonzero(A) == 64 + 2 * 63
    s = C.case('sparse')['A']
    assert 0.1 < np.count_nonzero(s) / s.size < 0.2
    assert C.lam_min(C.case('wide')) == C.sigma_min(C.case('wide')['A']) ** 2 > 0
    assert np.linalg.matrix_rank(C.case('wide')['A']) == 32


# ---------------------------------------------------------------- the exact one-launch data
@pytest.mark.parametrize('nb', C.ONE_LAUNCH_NB)
@pytest.mark.parametrize('n', C.ONE_LAUNCH_N)
def test_exact_data_conditions(n, nb):
    x, r, p, q = C.exact_vectors(n, nb)
    for a in (x, r, p, q):
        assert a.shape == (nb, n) and np.abs(a).max() <= 3
    S.assert_exact(x, r, p, q, bits=24)                                   # the vectors: exact in fp32
    S.assert_exact(C.dir_ref(r, p), scale=0.5, bits=24)                   # p' = r + p / 2
    pq = C.dot_terms(p, q)
    S.assert_exact(pq, scale=0.25, bits=53)                               # summands of pq: multiples of 1/4
    assert np.all(pq.sum(axis=1) > 0)
    rho = 0.5 * pq.sum(axis=1)
    assert np.array_equal(rho / pq.sum(axis=1), np.full(nb, C.ALPHA))     # state.rho = pq / 2: alpha = 1/2 exactly
    xn, rn, rr = C.update_ref(x, r, p, q)
    S.assert_exact(xn, scale=0.5, bits=24)
    S.assert_exact(rn, scale=0.125, bits=24)                              # r' = r - (q + p / 4) / 2
    S.assert_exact(rr, scale=1.0 / 64, bits=53)                           # summands of rho'
    S.assert_exact(r * r, x * x, bits=53)                                 # pcs_cg_init's sums
    for a in (xn, rn, C.dir_ref(r, p)):                                   # and every element is exact in fp32
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------- the C ABI
def test_new_symbols_exported_abi_unchanged():
    from pycsou_amd import _lib, _ops
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pcs_abi_version() == 10 and _lib.ABI_VERSION == 10
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'pycsou_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert f'{name}(' in header
    assert f'#define PCS_CG_MAX_BLOCKS {C.CAP}' in header and _lib.PCS_CG_MAX_BLOCKS == C.CAP == _ops.CG_MAX_BLOCKS
    for name in ('cg_init', 'cg_dir', 'cg_dot', 'cg_update', 'cg_normal', 'cg_state', 'cg_partials'):
        assert callable(getattr(_ops, name))


def test_scratch_sizes():
    from pycsou_amd import _lib
    lib = _lib.load()
    assert [lib.pcs_cg_state_bytes(nb) for nb in (1, 3, 65535)] == [64, 192, 64 * 65535]
    assert lib.pcs_cg_state_bytes(0) == -1 == lib.pcs_cg_nblocks(-1, 1) and lib.pcs_cg_nblocks(5, 0) == -1
    sizes = {n: lib.pcs_cg_nblocks(n, 1) for n in (0, 1, 256, 257, C.CAP * 256, C.CAP * 256 + 1, 1 << 33)}
    assert sizes == {0: 1, 1: 1, 256: 1, 257: 2, C.CAP * 256: C.CAP, C.CAP * 256 + 1: C.CAP, 1 << 33: C.CAP}
    assert lib.pcs_cg_nblocks(257, 3) == 6 and lib.pcs_cg_nblocks(1 << 33, 65535) == C.CAP * 65535


X, R, P, Q, B, ST, PA, CT, HI = (0x100000 * k for k in range(1, 10))   # stand-in addresses: never dereferenced


def _call(lib, which, **over):
    from pycsou_amd import _lib
    kw = dict(dtype=_lib.PCS_F64, x=X, r=R, p=P, q=Q, b=B, n=100, nb=3, rtol=1e-5, atol=0.0, max_iter=10, eps2=0.25,
              state=ST, partials=PA, ctrl=CT, hist=HI, hist_len=24)
    kw.update(over)
    order = {'init': ('dtype', 'b', 'r', 'n', 'nb', 'rtol', 'atol', 'max_iter', 'state', 'partials', 'ctrl', 'hist',
                      'hist_len'),
             'dir': ('dtype', 'r', 'p', 'n', 'nb', 'state', 'ctrl'),
             'dot': ('dtype', 'p', 'q', 'n', 'nb', 'eps2', 'state', 'partials', 'ctrl'),
             'update': ('dtype', 'x', 'r', 'p', 'q', 'n', 'nb', 'eps2', 'state', 'partials', 'ctrl', 'hist')}[which]
    return getattr(lib, f'pcs_cg_{which}')(*[kw[k] for k in order], None)


COMMON_BAD = {'dtype': dict(dtype=2), 'dtype_neg': dict(dtype=-1), 'n_neg': dict(n=-1), 'nb0': dict(nb=0),
              'nb_neg': dict(nb=-2), 'state': dict(state=None), 'ctrl': dict(ctrl=None)}
INF, NAN = float('inf'), float('nan')
BAD = {
    'init': dict(COMMON_BAD, b=dict(b=None), r=dict(r=None), partials=dict(partials=None), hist=dict(hist=None),
                 hist_len=dict(hist_len=1), max_iter=dict(max_iter=-1), rtol_neg=dict(rtol=-1e-5), rtol_inf=dict(rtol=INF),
                 rtol_nan=dict(rtol=NAN), atol_neg=dict(atol=-1.0), atol_inf=dict(atol=INF), atol_nan=dict(atol=NAN)),
    'dir': dict(COMMON_BAD, r=dict(r=None), p=dict(p=None), alias=dict(p=R), alias_inside=dict(p=R + 8 * 299),
                alias_below=dict(r=P + 8 * 150)),
    'dot': dict(COMMON_BAD, p=dict(p=None), q=dict(q=None), partials=dict(partials=None), eps2_neg=dict(eps2=-0.25),
                eps2_inf=dict(eps2=INF), eps2_nan=dict(eps2=NAN), alias=dict(q=P), alias_inside=dict(q=P + 8 * 299)),
    'update': dict(COMMON_BAD, x=dict(x=None), r=dict(r=None), p=dict(p=None), q=dict(q=None),
                   partials=dict(partials=None), hist=dict(hist=None), eps2_neg=dict(eps2=-0.25), eps2_inf=dict(eps2=INF),
                   eps2_nan=dict(eps2=NAN), alias_xr=dict(r=X), alias_xp=dict(p=X), alias_xq=dict(q=X + 8 * 299),
                   alias_rp=dict(p=R), alias_rq=dict(q=R + 8), alias_pq=dict(q=P)),
}


@pytest.mark.parametrize('which,bad', [(w, b) for w in sorted(BAD) for b in sorted(BAD[w])])
def test_argument_checks(which, bad):
    """Every bad-argument case returns PCS_EINVAL before any device call (no GPU here)."""
    from pycsou_amd import _lib
    assert _call(_lib.load(), which, **BAD[which][bad]) == -1


@pytest.mark.parametrize('which', sorted(BAD))
def test_more_systems_than_grid_rows_is_unsupported(which):
    from pycsou_amd import _lib
    assert _call(_lib.load(), which, nb=65536, n=4) == -3
    assert _call(_lib.load(), which, nb=65536, n=4, dtype=7) == -1        # a bad argument is still reported first


# ---------------------------------------------------------------- shapes and types
def test_shapes_and_types_of_the_new_operators():
    from pycsou_amd.core.linop import LinOpPinv, SymmetricLinearOperator, UnitaryOperator
    from pycsou_amd.linop import DenseLinearOperator, KroneckerProduct
    A = DenseLinearOperator(C.case('tall')['A'])
    assert A.dagger.shape == A.H.shape == (32, 48) and isinstance(A.dagger, LinOpPinv) and isinstance(A.PinvOp, LinOpPinv)
    assert A.dagger.LinOp is A and A.dagger.eps == 0 and LinOpPinv(A, 0.5).eps == 0.5 and not A.dagger.is_symmetric
    Ad = A.dagger.H
    assert isinstance(Ad, LinOpPinv) and Ad.shape == (48, 32) and Ad.LinOp.shape == A.H.shape
    R, Cp = A.RowProjector, A.ColProjector
    assert isinstance(R, SymmetricLinearOperator) and R.is_symmetric and R.shape == (32, 32)
    assert isinstance(Cp, SymmetricLinearOperator) and Cp.is_symmetric and Cp.shape == (48, 48)
    S1 = DenseLinearOperator(np.eye(4), is_symmetric=True)
    S1d = S1.dagger
    assert S1d.is_symmetric and S1d.H is S1d
    B = DenseLinearOperator(np.ones((5, 3)))
    K = KroneckerProduct(DenseLinearOperator(np.ones((6, 4))), B).PinvOp
    assert isinstance(K, KroneckerProduct) and isinstance(K.linop1, LinOpPinv) and isinstance(K.linop2, LinOpPinv)
    assert K.shape == (12, 30) and K.linop1.shape == (4, 6) and K.linop2.shape == (3, 5)
    U = UnitaryOperator(size=7)
    assert U.cond() == 1 and U.dagger is not None and not isinstance(U.PinvOp, LinOpPinv)      # its overrides stay
    for name in ('pinv', 'todense', 'tosparse', 'cond'):
        assert callable(getattr(A, name))


def test_cond_refuses_large_operators():
    from pycsou_amd.linop.base import NullOperator
    with pytest.raises(NotImplementedError, match='2048'):
        NullOperator((2049, 3000)).cond()
