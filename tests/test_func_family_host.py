"""CPU tier of the func family (L1Ball / LInftyNorm / SquaredL1Norm, KLDivergence, LogBarrier,
ShannonEntropy, QuadraticForm and the ball / consistency losses): names, types and attributes as in
pycsou/func/penalty.py:248-417, 770-990, pycsou/func/loss.py:222-682 and pycsou/math/prox.py:117-164; the new
C-ABI entry points' argument checks (they run before any device call); the host-side bracket selection of
the threshold kernel against a NumPy evaluation of psi; and the fixture checked against the exact sort-based
restatement of tests/func_family_cases.py.  No compute calls (no GPU here)."""

import ctypes
import sys

import numpy as np
import pytest

from tests import func_family_cases as C
from tests.cases import load

PENALTY = ('L1Ball', 'LInftyNorm', 'SquaredL1Norm', 'LogBarrier', 'ShannonEntropy', 'QuadraticForm')
LOSS = ('KLDivergence', 'L1BallLoss', 'L2BallLoss', 'LInftyLoss', 'LInftyBallLoss', 'SquaredL1Loss',
        'ConsistencyLoss')
NEW_SYMBOLS = ('pcs_thresh_ws_bytes', 'pcs_thresh_l1', 'pcs_thresh_pick_host', 'pcs_prox_kl', 'pcs_prox_logbarrier',
               'pcs_prox_entropy')


def test_reference_names_import():
    import importlib
    for mod, names in (('func.penalty', PENALTY), ('func.loss', LOSS), ('math.prox', ('proj_l1_ball',))):
        m = importlib.import_module('pycsou_amd.' + mod)
        for name in names:
            assert callable(getattr(m, name)), (mod, name)
    from pycsou_amd import func
    for name in PENALTY + LOSS:
        assert hasattr(func, name), name


def test_reference_names_import_under_alias():
    import importlib
    import pycsou_amd
    saved = {k: v for k, v in sys.modules.items() if k == 'pycsou' or k.startswith('pycsou.')}
    try:
        pycsou_amd.install_alias('pycsou')
        for mod, names in (('func.penalty', PENALTY), ('func.loss', LOSS), ('math.prox', ('proj_l1_ball',))):
            m = importlib.import_module('pycsou.' + mod)
            for name in names:
                assert callable(getattr(m, name)), (mod, name)
        from pycsou.func.penalty import L1Ball  # noqa: F401
        from pycsou.func.loss import KLDivergence  # noqa: F401
    finally:
        for k in [k for k in sys.modules if k == 'pycsou' or k.startswith('pycsou.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_types_and_attributes_match_reference():
    from pycsou_amd.core.functional import (DifferentiableFunctional, ProxFuncPostComp, ProxFuncPreComp,
                                            ProximableFunctional)
    from pycsou_amd.func.base import IndicatorFunctional, LpNorm
    from pycsou_amd.func import loss, penalty
    from pycsou_amd.linop.base import DenseLinearOperator
    from pycsou_amd.math.prox import proj_l1_ball
    assert isinstance(penalty.LInftyNorm(5), LpNorm) and penalty.LInftyNorm(5).proj_lq_ball is proj_l1_ball
    assert isinstance(penalty.L1Ball(5, 2.0), IndicatorFunctional)
    s = penalty.SquaredL1Norm(5)
    assert isinstance(s, ProximableFunctional) and s.prox_computation == 'sort'
    assert penalty.SquaredL1Norm(5, prox_computation='root').prox_computation == 'root'
    two = 2 * penalty.SquaredL1Norm(5)
    assert isinstance(two, ProxFuncPostComp) and two.scale == 2
    for cls in (penalty.LogBarrier, penalty.ShannonEntropy):
        f = cls(7)
        assert isinstance(f, ProximableFunctional) and f.dim == 7 and f.shape == (1, 7)
    L = DenseLinearOperator(np.diag([1.0, 2.0, 3.0]))
    L.lipschitz_cst = L.diff_lipschitz_cst = 3.0
    q = penalty.QuadraticForm(3, linop=L)
    assert isinstance(q, DifferentiableFunctional)
    assert q.diff_lipschitz_cst == 2 * L.diff_lipschitz_cst and q.linop is L
    assert penalty.QuadraticForm(3).diff_lipschitz_cst == 2 and penalty.QuadraticForm(3).linop is None
    y = np.arange(4.0)
    kl = loss.KLDivergence(4, data=y)
    assert isinstance(kl, ProximableFunctional) and kl.data is y and kl.dim == 4
    for f in (loss.L1BallLoss(4, y, radius=2), loss.L2BallLoss(4, y), loss.LInftyBallLoss(4, y, 0.5),
              loss.LInftyLoss(4, y), loss.SquaredL1Loss(4, y, prox_computation='root')):
        assert isinstance(f, ProxFuncPreComp) and f.scale == 1 and np.array_equal(f.shift, -y)
    assert isinstance(loss.L1BallLoss(4, y).prox_func, IndicatorFunctional)
    assert isinstance(loss.LInftyLoss(4, y).prox_func, penalty.LInftyNorm)
    assert loss.SquaredL1Loss(4, y, prox_computation='root').prox_func.prox_computation == 'root'
    assert isinstance(loss.ConsistencyLoss(4, y), IndicatorFunctional)


def test_new_symbols_exported_abi_unchanged():
    from pycsou_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pcs_abi_version() == 10 and _lib.ABI_VERSION == 10
    assert lib.pcs_thresh_ws_bytes(70001) > 0 and lib.pcs_thresh_ws_bytes(1 << 40) >= lib.pcs_thresh_ws_bytes(70001)
    assert lib.pcs_thresh_ws_bytes(-1) == -1


X, Y, OUT, WS = 0x10000, 0x18000, 0x20000, 0x30000  # stand-in addresses: never dereferenced


@pytest.mark.parametrize('bad', ['dtype', 'n', 'x', 'out', 'ws', 'ws_align', 'a', 'b', 'ab', 'a_nan', 'mode'])
def test_thresh_argument_checks(bad):
    """Every bad-argument case returns PCS_EINVAL before any device call (no GPU here)."""
    from pycsou_amd import _lib
    lib = _lib.load()
    kw = dict(dtype=_lib.PCS_F64, x=X, out=OUT, n=8, a=1.0, b=0.0, mode=_lib.PCS_THRESH_SOFT, ws=WS)
    kw.update({'dtype': dict(dtype=2), 'n': dict(n=-1), 'x': dict(x=None), 'out': dict(out=None), 'ws': dict(ws=None),
               'ws_align': dict(ws=WS + 4), 'a': dict(a=-0.5), 'b': dict(b=-0.5), 'ab': dict(a=0.0, b=0.0),
               'a_nan': dict(a=float('nan')), 'mode': dict(mode=2)}[bad])
    rc = lib.pcs_thresh_l1(kw['dtype'], kw['x'], kw['out'], kw['n'], kw['a'], kw['b'], kw['mode'], None, kw['ws'], None)
    assert rc == -1


def test_n_zero_is_a_noop():
    from pycsou_amd import _lib
    lib = _lib.load()
    for dt in (_lib.PCS_F32, _lib.PCS_F64):
        for mode in (_lib.PCS_THRESH_SOFT, _lib.PCS_THRESH_CLIP):
            assert lib.pcs_thresh_l1(dt, X, OUT, 0, 1.0, 0.0, mode, None, WS, None) == 0
        assert lib.pcs_prox_kl(dt, X, Y, OUT, 0, 1.0, None) == 0
        assert lib.pcs_prox_logbarrier(dt, X, OUT, 0, 1.0, None) == 0
        assert lib.pcs_prox_entropy(dt, X, OUT, 0, 1.0, None) == 0


@pytest.mark.parametrize('fn', ['kl', 'logbarrier', 'entropy'])
@pytest.mark.parametrize('bad', ['dtype', 'n', 'x', 'out', 'y', 'tau0', 'tau_neg'])
def test_elementwise_argument_checks(fn, bad):
    from pycsou_amd import _lib
    lib = _lib.load()
    if bad == 'y' and fn != 'kl':
        return
    kw = dict(dtype=_lib.PCS_F32, x=X, y=Y, out=OUT, n=8, tau=1.0)
    kw.update({'dtype': dict(dtype=-1), 'n': dict(n=-1), 'x': dict(x=None), 'out': dict(out=None), 'y': dict(y=None),
               'tau0': dict(tau=0.0), 'tau_neg': dict(tau=-1.0)}[bad])
    if fn == 'kl':
        rc = lib.pcs_prox_kl(kw['dtype'], kw['x'], kw['y'], kw['out'], kw['n'], kw['tau'], None)
    else:
        rc = getattr(lib, 'pcs_prox_' + fn)(kw['dtype'], kw['x'], kw['out'], kw['n'], kw['tau'], None)
    assert rc == -1


# ---------------------------------------------------------------- bracket selection
def _key(v):
    return int(np.array([abs(v)], dtype=np.float64).view(np.uint64)[0])


def _val(k):
    return float(np.array([k], dtype=np.uint64).view(np.float64)[0])


def _pick(x, a, b, lo, hi):
    """pcs_thresh_pick_host on data x, next to the same selection from psi evaluated with NumPy."""
    from pycsou_amd import _lib
    lib = _lib.load()
    J = _lib.PCS_THRESH_PIVOTS
    piv = (ctypes.c_double * J)()
    assert lib.pcs_thresh_pick_host(_lib.PCS_F64, lo, hi, 0.0, None, a, b, piv, None) == J
    piv = np.array(piv[:])
    sums = np.array([np.maximum(np.abs(x) - p, 0.0).sum() for p in piv])
    br = (ctypes.c_uint64 * 2)()
    rc = lib.pcs_thresh_pick_host(_lib.PCS_F64, lo, hi, float(np.abs(x).sum()), _lib.dbls(sums), a, b, None, br)
    psi = sums - a - b * piv
    nonpos = np.flatnonzero(~(psi > 0))
    k = int(nonpos[0]) + 1 if nonpos.size else J + 1
    return rc, (br[0], br[1]), k, piv


@pytest.mark.parametrize('where,k_expect', [('first', 1), ('middle', 16), ('last', 32), ('tie', 16)])
def test_thresh_pick_host_brackets(where, k_expect):
    """x = (+h, -h, 0.5) over a bracket of 128 keys above 1.0 has psi(p) = 2 (r - p) with the root r placed by a:
    inside the first, a middle and the last bracket, and exactly on pivot 16 (psi = 0 there closes the bracket,
    so the tie lands on [pivot 15, pivot 16])."""
    from pycsou_amd import _lib
    J = _lib.PCS_THRESH_PIVOTS
    lo = _key(1.0)
    hi = lo + 128
    h = _val(hi)
    root = _val(lo + {'first': 2, 'middle': 62, 'last': 126, 'tie': 64}[where])
    x = np.array([h, -h, 0.5])
    rc, br, k, piv = _pick(x, 2 * (h - root), 0.0, lo, hi)
    assert rc == J and k == k_expect
    edges = np.concatenate([[1.0], piv, [h]])
    assert (_val(br[0]), _val(br[1])) == (edges[k - 1], edges[k])
    assert _val(br[0]) <= root <= _val(br[1])
    if where == 'tie':
        assert root == _val(br[1]) == piv[15]


def test_thresh_pick_host_inside_ball_and_slope():
    from pycsou_amd import _lib
    J = _lib.PCS_THRESH_PIVOTS
    x = np.array([3.0, -1.0, 0.25, 0.0])
    rc, br, _, _ = _pick(x, 4.25, 0.0, 0, _key(3.0))       # sum |x| == a: t = 0
    assert rc == 0 and br == (0, 0)
    rc, br, _, _ = _pick(x, 10.0, 0.5, 0, _key(3.0))
    assert rc == 0 and br == (0, 0)
    # b > 0 (the SquaredL1Norm form) from the full bracket, descended to two adjacent keys
    a, b = 0.0, 1.0 / (2 * 0.7)
    lo, hi = 0, _key(3.0)
    for _ in range(13):
        rc, (lo, hi), k, piv = _pick(x, a, b, lo, hi)
        assert rc == J
    assert hi - lo <= 1
    t = float(C.exact_threshold(x, a, b))
    assert _val(lo) <= t <= _val(hi)


# ---------------------------------------------------------------- fixture self-check
def _fixture_cases():
    for n in C.FIXTURE_SIZES:
        for kind in C.KINDS:
            x = C.make_x(kind, n)
            for case in C.thresh_params(kind, n, x):
                yield n, kind, x, case


def test_fixture_matches_exact_restatement():
    """Every threshold-family vector of func_family.npz against the sort-based restatement (longdouble sums):
    <= 1e-11 max(1, max|x|) where the reference runs brentq (xtol = 2e-12, rtol = 8.9e-16 on inputs of magnitude
    <= 8, x5 margin; the one 1e6 outlier scales the bound), <= 32 eps max|x| for the 'sort' vectors, which hold
    no brentq."""
    g = load('func_family.npz')
    eps = np.finfo(np.float64).eps
    off = {'l1ball': 0, 'linfty': 0, 'sql1': 0}
    count = 0
    for n, kind, x, (name, par, a, b, mode) in _fixture_cases():
        ref = g['thr_' + name][off[name]:off[name] + n]
        off[name] += n
        t, exact = C.exact_prox(x, a, b, mode)
        err = np.max(np.abs(ref - exact))
        mx = np.abs(x).max()
        bound = 32 * eps * mx if name == 'sql1' else 1e-11 * max(1.0, mx)
        assert err <= bound, (name, kind, n, par, err, bound)
        if name == 'l1ball' and par >= 1.0:
            assert t == 0 and np.array_equal(ref, x)   # inside the ball: the identity branch
        count += 1
    assert all(off[k] == g['thr_' + k].size for k in off) and count == 6 * 6 * 10 + 6
    # the 'root' computation (brentq on mu) gives the same prox
    o = 0
    for n in (63, 257):
        for kind in ('normal', 'mixed'):
            x = C.make_x(kind, n)
            for tau in C.TAUS:
                ref = g['thr_sql1_root'][o:o + n]
                o += n
                err = np.max(np.abs(ref - C.exact_prox(x, 0.0, 1.0 / (2 * tau), 'soft')[1]))
                assert err <= 1e-11 * max(1.0, np.abs(x).max()), (kind, n, tau, err)
    assert o == g['thr_sql1_root'].size


def test_fixture_is_arrays_only_and_small():
    import os
    from tests.cases import GOLDEN
    path = os.path.join(GOLDEN, 'func_family.npz')
    assert os.path.getsize(path) < 1_000_000
    g = load('func_family.npz')                         # allow_pickle=False: plain arrays
    assert int(g['apgd_l1ball3_stop_n_iter']) == 31 and int(g['apgd_l1ball6_stop_n_iter']) == 121
    assert (g['ptv_y'] == 0).any() and int(g['ptv_n_iter']) == 40
