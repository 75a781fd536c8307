"""GPU tier of the func family: the threshold kernel (pcs_thresh_l1: L1Ball / LInftyNorm / SquaredL1Norm
prox, pycsou/math/prox.py:158-164, func/base.py:239-240, func/penalty.py:296-316) against the exact sort-based
restatement of tests/func_family_cases.py and against the reference's outputs in func_family.npz; the
element-wise KL / log-barrier / entropy prox kernels (func/loss.py:682, func/penalty.py:840, 921-922); every new
functional's prox, fenchel_prox and value; the solvers on the reference's trajectories; and the hipGraph-captured
generic loop against the eager one.

Bounds.  Threshold, fp64 against the exact restatement: 32 eps64 max|x| (a fixed-order tree sum of n <= 2^17
terms costs <= 17 eps S, plus the division and the subtraction, rounded up); fp32: eps32 max|x| (t is exact to
fp64, the only error is the final rounding of out); fp64 against the reference: 1e-11 max(1, max|x|) (brentq's
xtol 2e-12, x5).  KL / barrier fp64: relative 1e-11 (the reference itself loses ~eps x^2 / tau <= 2e-12 on
|x| <= 30); entropy fp64: relative 1e-12 (conditioning eps (1 + |x / tau|) ~ 1.6e-13, x6); fp32: 8 eps32.
"""

import numpy as np
import pytest
import torch

from tests import func_family_cases as C
from tests.cases import load, rel

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
_cache = {}


def golden():
    if 'g' not in _cache:
        _cache['g'] = load('func_family.npz')
    return _cache['g']


def fixture_slices():
    """{(family, n, kind, parameter): slice into thr_<family>} in the order make_golden_func.py wrote them."""
    if 'slices' not in _cache:
        off, out = {'l1ball': 0, 'linfty': 0, 'sql1': 0}, {}
        for n in C.FIXTURE_SIZES:
            for kind in C.KINDS:
                for name, par, a, b, mode in C.thresh_params(kind, n, C.make_x(kind, n)):
                    out[(name, n, kind, par)] = slice(off[name], off[name] + n)
                    off[name] += n
        _cache['slices'] = out
    return _cache['slices']


def dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


# ---------------------------------------------------------------- threshold kernel
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('kind', C.KINDS)
@pytest.mark.parametrize('n', C.SIZES)
def test_thresh_kernel_exact(n, kind, dtype):
    from pycsou_amd import _ops as O
    g = golden()
    x = C.make_x(kind, n)                      # fp32-representable: both dtypes run the same numbers
    xd = dev(x, dtype)
    mx = float(np.abs(x).max())
    bound = 32 * EPS64 * mx if dtype == np.float64 else EPS32 * mx
    t_out = torch.full((1,), -1.0, dtype=torch.float64, device='cuda')
    for name, par, a, b, mode in C.thresh_params(kind, n, x):
        t, exact = C.exact_prox(x, a, b, mode)
        out = O.thresh_l1(xd, a, b, mode, t_out).cpu().numpy()
        tg = float(t_out.item())
        assert out.dtype == dtype and np.all(np.isfinite(out))
        err, terr = float(np.max(np.abs(out.astype(np.float64) - exact))), abs(tg - t)
        print(f'{name} {par}: n={n} {kind} {np.dtype(dtype).name} |out-exact|={err:.3e} |t-exact|={terr:.3e} '
              f'bound={bound:.3e}')
        assert err <= bound, (name, par, err, bound)
        assert terr <= bound, (name, par, tg, t, bound)
        if name == 'l1ball' and par >= 1.0:    # inside the ball: x bitwise, t = 0
            assert tg == 0.0 and np.array_equal(out.view(np.uint8), np.ascontiguousarray(x, dtype).view(np.uint8))
        if mode == 'clip' and t == 0:
            assert not out.any()
        if dtype == np.float64 and n in C.FIXTURE_SIZES:
            ref = g['thr_' + name][fixture_slices()[(name, n, kind, par)]]
            assert np.max(np.abs(out - ref)) <= 1e-11 * max(1.0, mx), (name, par)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('mode,a,b', [('soft', 900.0, 0.0), ('clip', 3.0, 0.0), ('soft', 0.0, 0.25)])
def test_thresh_kernel_deterministic(mode, a, b, dtype):
    from pycsou_amd import _ops as O
    xd = dev(C.make_x('normal', 70001), dtype)
    t1 = torch.zeros(1, dtype=torch.float64, device='cuda')
    t2 = torch.zeros(1, dtype=torch.float64, device='cuda')
    o1 = O.thresh_l1(xd, a, b, mode, t1)
    o2 = O.thresh_l1(xd, a, b, mode, t2)
    assert torch.equal(o1, o2) and torch.equal(t1, t2) and float(t1) > 0


def test_thresh_in_place_and_no_t():
    from pycsou_amd import _lib as L, _ops as O
    x = C.make_x('normal', 4099)
    xd = dev(x)
    want = O.thresh_l1(xd, 40.0, 0.0, 'soft')
    L.check(L.gpu().pcs_thresh_l1(L.PCS_F64, L.ptr(xd), L.ptr(xd), xd.numel(), 40.0, 0.0, L.PCS_THRESH_SOFT, None,
                                  L.ptr(O._thresh_ws(xd)), L.stream()), 'pcs_thresh_l1')
    assert torch.equal(xd, want)


# ---------------------------------------------------------------- element-wise kernels
def _relerr(out, ref, floor=0.0):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return np.abs(out - ref) / np.maximum(np.abs(ref), floor if floor > 0 else np.finfo(np.float64).tiny)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('tau', C.KL_TAUS)
def test_kl_and_logbarrier_match_reference(tau, dtype):
    from pycsou_amd import _ops as O
    g = golden()
    x, y = C.kl_inputs()
    tol = 1e-11 if dtype == np.float64 else 8 * EPS32
    for name, out in (('kl', O.prox_kl(dev(x, dtype), dev(y, dtype), tau)),
                      ('logb', O.prox_logbarrier(dev(x, dtype), tau))):
        out = out.cpu().numpy()
        ref = g[f'{name}_prox_{tau}'].astype(dtype).astype(np.float64)
        zero = ref == 0
        assert np.array_equal(out[zero], ref[zero])          # y = 0, x <= tau: exactly 0, as in the reference
        e = float(_relerr(out[~zero], ref[~zero]).max())
        print(f'{name} tau={tau} {np.dtype(dtype).name}: max rel err {e:.3e} (tol {tol:.1e})')
        assert e <= tol, (name, e)
        assert np.all(out >= 0) and (name == 'kl' or np.all(out > 0))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('tau', C.KL_TAUS)
def test_kl_and_logbarrier_defining_equations(tau, dtype):
    """On x in [-1e6, 1e6] the prox is only checked against the quadratic it solves, out (out - x) = tau and
    out (out - x + tau) = tau y, evaluated in longdouble from the returned values: the residual is at most
    16 eps of the dtype relative to the magnitude of the equation's terms, out (|out| + |x| (+ tau)) + rhs."""
    from pycsou_amd import _ops as O
    rng = np.random.default_rng(31)
    x = np.concatenate([rng.uniform(-1e6, 1e6, 500), -10.0 ** rng.uniform(-3, 6, 250), 10.0 ** rng.uniform(-3, 6, 250),
                        [-1e6, 1e6, 0.0]]).astype(np.float32).astype(np.float64)
    y = np.tile([0.0, 1.0, 3.0, 50.0], x.size // 4 + 1)[:x.size]
    eps = EPS64 if dtype == np.float64 else EPS32
    xl, yl = x.astype(np.longdouble), y.astype(np.longdouble)
    p = O.prox_logbarrier(dev(x, dtype), tau).cpu().numpy().astype(np.longdouble)
    assert np.all(p > 0)
    res = np.abs(p * (p - xl) - tau) / (p * (p + np.abs(xl)) + tau)
    print(f'logb tau={tau} {np.dtype(dtype).name}: residual {float(res.max()):.3e} (16 eps = {16 * eps:.3e})')
    assert float(res.max()) <= 16 * eps
    p = O.prox_kl(dev(x, dtype), dev(y, dtype), tau).cpu().numpy().astype(np.longdouble)
    assert np.all(p >= 0)
    res = np.abs(p * (p - xl + tau) - tau * yl) / (p * (p + np.abs(xl) + tau) + tau * yl + np.finfo(np.float64).tiny)
    print(f'kl tau={tau} {np.dtype(dtype).name}: residual {float(res.max()):.3e}')
    assert float(res.max()) <= 16 * eps


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('tau', C.KL_TAUS)
def test_entropy_matches_reference(tau, dtype):
    from pycsou_amd import _ops as O
    x = C.entropy_inputs(tau)
    ref = golden()[f'ent_prox_{tau}']
    out = O.prox_entropy(dev(x, dtype), tau).cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(out)) and np.all(out >= 0)
    if dtype == np.float64:
        e = float(_relerr(out, ref).max())
        print(f'entropy tau={tau} fp64: max rel err {e:.3e} (tol 1e-12)')
        assert e <= 1e-12
    else:
        tol = 8 * EPS32 * (1 + np.abs(x / tau)) * np.abs(ref) + float(np.finfo(np.float32).tiny)
        e = np.abs(out - ref)
        print(f'entropy tau={tau} fp32: max err / tol {float((e / tol).max()):.3f}')
        assert np.all(e <= tol)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('tau', C.KL_TAUS)
def test_entropy_stays_finite_past_exp_overflow(tau, dtype):
    """x / tau in {800, 5000}: the reference's exp overflows; the log-domain form stays finite and solves
    p + tau ln p + tau = x to 16 eps of the dtype (relative to x); very negative x / tau underflows to 0."""
    from pycsou_amd import _ops as O
    x = np.array([800.0 * tau, 5000.0 * tau, -800.0 * tau, -5000.0 * tau]).astype(np.float32).astype(np.float64)
    p = O.prox_entropy(dev(x, dtype), tau).cpu().numpy().astype(np.longdouble)
    assert np.all(np.isfinite(p[:2])) and np.all(p[:2] > 0) and np.array_equal(p[2:], [0.0, 0.0])
    eps = EPS64 if dtype == np.float64 else EPS32
    res = np.abs(p[:2] + tau * np.log(p[:2]) + tau - x[:2]) / x[:2]
    print(f'entropy overflow tau={tau} {np.dtype(dtype).name}: residual {res.astype(float)}')
    assert np.all(res <= 16 * eps)


# ---------------------------------------------------------------- functionals
THRESH_FUNCS = ('l1ball', 'linfty', 'linfty3', 'sql1', 'sql1x2', 'l1ballloss', 'linftyloss', 'sql1loss')
CLOSED_FUNCS = ('l2ballloss', 'linftyballloss', 'consistency')
ELEMENT_FUNCS = {'logb': 1e-11, 'kl': 1e-11, 'entropy': 1e-12}


def _functionals(g):
    from pycsou_amd.func import loss, penalty as pen
    n = 65
    v, vp, d, yc = g['fn_v'], g['fn_vp'], g['fn_d'], g['fn_yc']
    return {
        'l1ball': (pen.L1Ball(dim=n, radius=4.0), v),
        'linfty': (pen.LInftyNorm(dim=n), v),
        'linfty3': (3.0 * pen.LInftyNorm(dim=n), v),
        'sql1': (pen.SquaredL1Norm(dim=n), v),
        'sql1x2': (2 * pen.SquaredL1Norm(dim=n), v),
        'logb': (pen.LogBarrier(dim=n), vp),
        'entropy': (pen.ShannonEntropy(dim=n), vp),
        'kl': (loss.KLDivergence(dim=n, data=yc), vp),
        'l2ballloss': (loss.L2BallLoss(dim=n, data=d, radius=3.0), v),
        'l1ballloss': (loss.L1BallLoss(dim=n, data=d, radius=4.0), v),
        'linftyballloss': (loss.LInftyBallLoss(dim=n, data=d, radius=0.8), v),
        'linftyloss': (loss.LInftyLoss(dim=n, data=d), v),
        'sql1loss': (loss.SquaredL1Loss(dim=n, data=d), v),
        'consistency': (loss.ConsistencyLoss(dim=n, data=d), v),
    }


@pytest.mark.parametrize('name', THRESH_FUNCS + CLOSED_FUNCS + tuple(ELEMENT_FUNCS))
def test_functional_matches_reference(name):
    """prox(., 0.7), fenchel_prox(., 1.3) and the value of each new functional against the reference, fp64, with the
    bound of its prox kernel: 1e-11 max(1, max|argument|) absolute for the threshold family (the argument of the
    inner prox: shifted by the data for a loss, divided by sigma and the result scaled by sigma for fenchel_prox),
    relative 1e-11 / 1e-12 of the prox value for the element-wise ones, 1e-13 for the closed forms and values."""
    g = golden()
    f, arg = _functionals(g)[name]
    sigma = 1.3
    out = f.prox(arg.copy(), tau=0.7)
    fen = f.fenchel_prox(arg.copy(), sigma=sigma)
    assert isinstance(out, np.ndarray) and isinstance(fen, np.ndarray) and out.dtype == np.float64
    ref_p, ref_f = g[f'fn_{name}_prox'], g[f'fn_{name}_fenchel']
    shift = np.abs(g['fn_d']).max() if name.endswith('loss') else 0.0
    if name in THRESH_FUNCS:
        assert np.max(np.abs(out - ref_p)) <= 1e-11 * max(1.0, np.abs(arg).max() + shift)
        assert np.max(np.abs(fen - ref_f)) <= sigma * 1e-11 * max(1.0, np.abs(arg).max() / sigma + shift)
    elif name in CLOSED_FUNCS:
        assert rel(out, ref_p) <= 1e-13 and rel(fen, ref_f) <= 1e-13
    else:
        tol = ELEMENT_FUNCS[name]
        assert np.all(np.abs(out - ref_p) <= tol * np.abs(ref_p))
        inner = np.abs(arg - ref_f)            # sigma * prox(arg / sigma, 1 / sigma)
        assert np.all(np.abs(fen - ref_f) <= tol * inner + 4 * EPS64 * np.abs(arg))
    val, ref_v = f(arg.copy()), float(g[f'fn_{name}_value'])
    assert val == ref_v if np.isinf(ref_v) else abs(val - ref_v) <= 1e-13 * abs(ref_v), (val, ref_v)
    # a torch tensor in gives a device tensor out
    t = f.prox(torch.from_numpy(arg), tau=0.7)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), out)


def test_indicator_values_and_quadratic_form():
    from pycsou_amd.func import loss, penalty as pen
    from pycsou_amd.linop.base import DenseLinearOperator
    g = golden()
    v, d, M = g['fn_v'], g['fn_d'], g['fn_M']
    assert pen.L1Ball(dim=65, radius=4.0)(v / np.abs(v).sum()) == float(g['fn_l1ball_value_inside']) == 0
    assert loss.ConsistencyLoss(dim=65, data=d)(d.copy()) == float(g['fn_consistency_value_at_data']) == 0
    Lop = DenseLinearOperator(M)
    Lop.lipschitz_cst = Lop.diff_lipschitz_cst = float(np.linalg.norm(M, 2))
    for name, q in (('quad', pen.QuadraticForm(dim=65)), ('quadL', pen.QuadraticForm(dim=65, linop=Lop))):
        assert abs(q(v) - float(g[f'fn_{name}_value'])) <= 1e-13 * abs(float(g[f'fn_{name}_value']))
        assert rel(q.gradient(v), g[f'fn_{name}_grad']) <= 1e-13
        assert q.diff_lipschitz_cst == float(g[f'fn_{name}_dlip'])


def test_reference_doctests():
    from pycsou_amd.func.penalty import L1Ball, SquaredL1Norm
    from pycsou_amd.math.prox import proj_l1_ball
    p = proj_l1_ball(np.linspace(-1, 1, 5), 2)
    assert isinstance(p, np.ndarray)
    np.testing.assert_allclose(p, [-0.75, -0.25, 0, 0.25, 0.75], rtol=0, atol=32 * EPS64)
    x1 = np.arange(10)
    ball = L1Ball(dim=10, radius=10)
    assert ball(x1) == np.inf and ball(x1 / 45.0) == 0
    assert abs(np.abs(ball.prox(x1, tau=1)).sum() - 10.0) <= 10 * 32 * EPS64
    np.testing.assert_array_equal(ball.prox(x1 / 45.0, tau=1), x1 / 45.0)
    s, r = SquaredL1Norm(dim=10, prox_computation='sort'), SquaredL1Norm(dim=10, prox_computation='root')
    assert s(x1) == 2025
    np.testing.assert_array_equal(s.prox(x1, tau=1), r.prox(x1, tau=1))
    assert not s.prox(np.zeros(10), tau=1).any()       # a zero input returns zeros


# ---------------------------------------------------------------- solvers on the reference's trajectories
def _apgd(G, g, tag):
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.linop.base import DenseLinearOperator
    from pycsou_amd.opt.proxalgs import APGD
    A, _, y = C.sparse_problem()
    Gop = DenseLinearOperator(A)
    Gop.lipschitz_cst = Gop.diff_lipschitz_cst = float(g['apgd_Glip'])
    F = (1 / 2) * SquaredL2Loss(dim=64, data=y) * Gop
    p = f'apgd_{tag}_'
    s = APGD(dim=128, F=F, G=G, acceleration='CD', max_iter=int(g[p + 'max_iter']), min_iter=int(g[p + 'min_iter']),
             accuracy_threshold=float(g[p + 'thr']), verbose=None)
    assert s.tau == float(g[p + 'tau'])
    est, _, diag = s.iterate()
    assert s.iter == int(g[p + 'n_iter'])
    assert rel(est['iterand'], g[p + 'x']) < 1e-9 and rel(est['past_aux'], g[p + 'past_aux']) < 1e-9
    np.testing.assert_allclose(diag['Relative Improvement'].to_numpy(float), g[p + 'diag'], rtol=1e-6)
    return est


@pytest.mark.parametrize('mode', ['fixed', 'stop'])
@pytest.mark.parametrize('r', [3, 6])
def test_apgd_l1ball_matches_reference(r, mode):
    """Constraint-form sparse recovery: 40 fixed iterations and the natural stop (31 / 121 iterations).  The
    projected iterate ('past_aux', the output of G.prox) lies in the ball."""
    from pycsou_amd.func.penalty import L1Ball
    est = _apgd(L1Ball(dim=128, radius=float(r)), golden(), f'l1ball{r}_{mode}')
    assert np.abs(est['past_aux']).sum() <= r * (1 + 1e-12)


@pytest.mark.parametrize('tag', ['linfty', 'sql1'])
def test_apgd_linfty_sql1_match_reference(tag):
    from pycsou_amd.func.penalty import LInftyNorm, SquaredL1Norm
    _apgd(0.5 * LInftyNorm(dim=128) if tag == 'linfty' else 0.02 * SquaredL1Norm(dim=128), golden(), tag)


def _poisson_tv(g, dtype=np.float64, engine=None):
    from pycsou_amd.func import KLDivergence, L21Norm, NonNegativeOrthant, ProxFuncHStack
    from pycsou_amd.linop import Convolve2D, Gradient, LinOpVStack
    from pycsou_amd.opt.proxalgs import CPS, PDS
    shape = tuple(int(s) for s in g['ptv_shape'])
    N = shape[0] * shape[1]
    Conv = Convolve2D(size=N, filter=g['ptv_psf'], shape=shape)
    Conv.lipschitz_cst = Conv.diff_lipschitz_cst = float(g['ptv_Clip'])
    D = Gradient(shape=shape, kind='forward')
    D.lipschitz_cst = D.diff_lipschitz_cst = float(g['ptv_Dlip'])
    H = ProxFuncHStack(KLDivergence(dim=N, data=g['ptv_y'].astype(dtype)),
                       0.3 * L21Norm(dim=2 * N, groups=np.tile(np.arange(N), 2)))
    K = LinOpVStack(Conv, D)
    kw = dict(dim=N, G=NonNegativeOrthant(dim=N), H=H, K=K, x0=np.zeros(N, dtype), z0=np.zeros(3 * N, dtype),
              max_iter=39, min_iter=39, accuracy_threshold=0.0, verbose=None)
    if engine is None:
        return CPS(**kw), K
    # ChambollePockSplitting (proxalgs.py:628-716) is PDS with F = 0 and rho = 1; PDS takes the engine choice
    return PDS(F=None, rho=1, engine=engine, **kw), K


def test_poisson_tv_cps_matches_reference():
    g = golden()
    cps, K = _poisson_tv(g)
    assert K.lipschitz_cst == pytest.approx(float(g['ptv_Klip']), rel=1e-15)
    assert (cps.tau, cps.sigma, cps.rho) == (float(g['ptv_tau']), float(g['ptv_sigma']), float(g['ptv_rho']))
    est, _, diag = cps.iterate()
    assert cps.iter == int(g['ptv_n_iter']) == 40
    assert rel(est['primal_variable'], g['ptv_x']) < 1e-9 and rel(est['dual_variable'], g['ptv_z']) < 1e-9
    np.testing.assert_allclose(diag['Relative Improvement (primal variable)'].to_numpy(float)[1:],
                               g['ptv_diag_primal'][1:], rtol=1e-7)
    np.testing.assert_allclose(diag['Relative Improvement (dual variable)'].to_numpy(float)[1:],
                               g['ptv_diag_dual'][1:], rtol=1e-7)
    assert np.all(est['primal_variable'] >= 0)


def test_poisson_tv_cps_fp32():
    """fp32 trajectory against the fp64 fixture: rel-L2 < 5e-5, the project's bound at this length."""
    g = golden()
    cps, _ = _poisson_tv(g, np.float32)
    est, _, _ = cps.iterate()
    assert est['primal_variable'].dtype == np.float32 and cps.iter == 40
    e = rel(est['primal_variable'], g['ptv_x'])
    print(f'poisson-tv fp32 rel-L2 {e:.3e}')
    assert e < 5e-5


def test_entropy_apgd_matches_reference():
    from pycsou_amd.func import ShannonEntropy, SquaredL2Loss
    from pycsou_amd.linop import Convolve2D
    from pycsou_amd.opt.proxalgs import APGD
    g = golden()
    shape = tuple(int(s) for s in g['ptv_shape'])
    N = shape[0] * shape[1]
    Conv = Convolve2D(size=N, filter=g['ptv_psf'], shape=shape)
    Conv.lipschitz_cst = Conv.diff_lipschitz_cst = 1.0
    F = (1 / 2) * SquaredL2Loss(dim=N, data=g['ent_apgd_y']) * Conv
    s = APGD(dim=N, F=F, G=0.5 * ShannonEntropy(dim=N), acceleration='CD', max_iter=29, min_iter=29,
             accuracy_threshold=0.0, verbose=None)
    assert s.tau == float(g['ent_apgd_tau'])
    est, _, diag = s.iterate()
    assert s.iter == int(g['ent_apgd_n_iter']) == 30
    assert rel(est['iterand'], g['ent_apgd_x']) < 1e-9
    np.testing.assert_allclose(diag['Relative Improvement'].to_numpy(float), g['ent_apgd_diag'], rtol=1e-6)


# ---------------------------------------------------------------- hipGraph-captured generic loop against eager
def _same_run(a, b):
    (pa, ea, da), (pb, eb, db) = a, b
    assert pa.iter == pb.iter
    for k in ea:
        x, y = ea[k], eb[k]
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y), k
    assert list(da.columns) == list(db.columns)
    for c in da.columns:
        np.testing.assert_array_equal(da[c].to_numpy(float), db[c].to_numpy(float))


def test_poisson_tv_graph_bitwise_eager(monkeypatch):
    runs = []
    for graph in (True, False):
        monkeypatch.setenv('PCS_GENERIC_GRAPH', '1' if graph else '0')
        cps, _ = _poisson_tv(golden(), engine='generic')
        est, _, diag = cps.iterate()
        runs.append((cps, est, diag))
    assert getattr(runs[0][0], '_graph_used', False) and not getattr(runs[1][0], '_graph_used', False)
    _same_run(*runs)


def test_l1ball_pds_graph_bitwise_eager(monkeypatch):
    """G = L1Ball on a 32 x 32 TV-denoising PDS, 11 iterations: the threshold kernel inside a captured chunk (no host
    sync in _prox, or the capture would fail and _graph_used stay false), bitwise the eager loop."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Ball, L21Norm
    from pycsou_amd.linop import Gradient
    from pycsou_amd.opt import PDS
    n = 32
    N = n * n
    img = np.zeros((n, n))
    img[n // 4:3 * n // 4, n // 3:2 * n // 3] = 1.0
    y = torch.from_numpy(img.ravel() + 0.1 * np.random.default_rng(11).standard_normal(N)).cuda()
    radius = 0.6 * float(np.abs(img).sum())
    runs = []
    for graph in (True, False):
        monkeypatch.setenv('PCS_GENERIC_GRAPH', '1' if graph else '0')
        K = Gradient(shape=(n, n), kind='forward')
        K.lipschitz_cst = K.diff_lipschitz_cst = float(np.sqrt(8.0))
        pds = PDS(dim=N, F=(1 / 2) * SquaredL2Loss(dim=N, data=y), G=L1Ball(dim=N, radius=radius),
                  H=0.1 * L21Norm(dim=2 * N, groups=np.tile(np.arange(N), 2)), K=K,
                  x0=torch.zeros(N, dtype=torch.float64, device='cuda'),
                  z0=torch.zeros(2 * N, dtype=torch.float64, device='cuda'), max_iter=10, min_iter=10,
                  accuracy_threshold=1e-3, verbose=None, engine='generic')
        est, _, diag = pds.iterate()
        runs.append((pds, est, diag))
    assert getattr(runs[0][0], '_graph_used', False) and not getattr(runs[1][0], '_graph_used', False)
    _same_run(*runs)
    assert runs[0][0].iter == 11
    x = runs[0][1]['primal_variable']
    # the iterate is a convex combination (rho) of projections onto the ball, starting inside it
    assert float(x.abs().sum()) <= radius * (1 + 1e-12)
