"""Directional derivatives and Integration1D on the device (pcs_dirderiv_*, pcs_cumsum) against the PyLops 1.x
definitions of tests/diff_family_cases.py (fp64 NumPy over oracle.pylops1) and the reference's own outputs in
tests/golden/diff_family.npz (pycsou/linop/diff.py:380-774, 1071-1137).

Tolerances are those of tests/test_gpu_ops.py: rel-L2 1e-12 (fp64) and 2e-6 (fp32) against fp64 references.
fp32 scan lines stay <= 4099 for normal data (a sequential fp32 cumsum is 6.0e-7 from the fp64 sum there but
3.0e-6 at 70001); the long lines carry small integers, whose partial sums are exact in both dtypes in any
order, and are compared with array_equal -- the cases that catch a wrong carry between waves, segments or
launches.  pcs_cumsum supports out == x (every sample is read and written by the same thread): tested below.
"""

import functools

import numpy as np
import pytest
import torch

from tests import diff_family_cases as C
from tests.cases import load, rel

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-12, np.float32: 2e-6}
DTYPES = [np.float64, np.float32]


@functools.lru_cache(maxsize=None)
def golden():
    return load('diff_family.npz')


def dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def dot_gap(op, seed=5):
    """|<A x, y> - <x, A^T y>| / (||x|| ||y||) with every product on the device in fp64."""
    rng = np.random.default_rng(seed)
    x, y = dev(rng.standard_normal(op.shape[1])), dev(rng.standard_normal(op.shape[0]))
    gap = torch.abs(torch.dot(op(x), y) - torch.dot(x, op.adjoint(y)))
    return float(gap / (torch.linalg.vector_norm(x) * torch.linalg.vector_norm(y)))


# ---------------------------------------------------------------- first directional derivative
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(65,), (2, 17), (7, 9), (63, 65), (64, 64), (5, 6, 7), (16, 17, 18), (3, 4, 5, 6)])
def test_first_directional_derivative(shape, dtype):
    """Three kinds, both edge values, non-unit steps, field and constant directions, forward and adjoint; the
    1-D shape runs the fused kernel with two padded axes, the 4-D shape goes through the composition of
    Gradient, pcs_mul and adds."""
    from pycsou_amd.linop import FirstDirectionalDerivative
    x, y, st = C.make_x(shape, 0), C.make_x(shape, 1), C.steps(shape)
    for field in (True, False):
        v = C.make_dirs(shape, field)
        for kind in C.KINDS:
            for edge in C.EDGES:
                op = FirstDirectionalDerivative(shape=shape, directions=v, step=st, edge=edge, kind=kind,
                                                dtype=np.dtype(dtype).name)
                got, got_adj = op(x.astype(dtype)), op.adjoint(y.astype(dtype))
                assert got.dtype == dtype and got_adj.dtype == dtype
                assert rel(got, C.first_dir(x, v, shape, st, kind, edge)) < TOL[dtype], (field, kind, edge)
                assert rel(got_adj, C.first_dir(y, v, shape, st, kind, edge, adjoint=True)) < TOL[dtype], \
                    (field, kind, edge)
                if dtype == np.float64:
                    assert dot_gap(op) <= 1e-12


def test_first_directional_derivative_matches_reference_vectors():
    from pycsou_amd.linop import FirstDirectionalDerivative
    g = golden()
    for tag, shape, field, kind, edge in C.vector_cases():
        op = FirstDirectionalDerivative(shape=shape, directions=C.make_dirs(shape, field), step=C.steps(shape),
                                        edge=edge, kind=kind)
        assert rel(op(C.make_x(shape, 0)), g[f'd1_{tag}_fwd']) < 1e-12, tag
        assert rel(op.adjoint(C.make_x(shape, 1)), g[f'd1_{tag}_adj']) < 1e-12, tag
        assert dot_gap(op) <= 1e-12, tag


@pytest.mark.parametrize('dtype', DTYPES)
def test_axis_directions_equal_first_derivative_exactly(dtype):
    """The doctest diff.py:422-429 made exact: with v = e_k the sum is 1 a + 0 b, exact with or without FMA
    contraction, so the fused kernel returns FirstDerivative's bits."""
    from pycsou_amd.linop import FirstDerivative, FirstDirectionalDerivative
    from pycsou_amd.util.misc import peaks
    t = np.linspace(-2.5, 2.5, 100)
    Z = peaks(*np.meshgrid(t, t)).astype(dtype)
    for axis, direction in ((0, [1, 0]), (1, [0, 1])):
        Dop = FirstDirectionalDerivative(shape=Z.shape, directions=np.array(direction), kind='forward')
        D = FirstDerivative(size=Z.size, shape=Z.shape, axis=axis, kind='forward')
        a, b = Dop * Z.flatten(), D * Z.flatten()
        assert a.dtype == dtype and np.array_equal(a, b) and np.abs(b).max() > 0.1


# ---------------------------------------------------------------- second directional derivative
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(7, 9), (63, 65), (5, 6, 7), (5, 6, 5, 6)])
def test_second_directional_derivative(shape, dtype):
    """The 4-D shape applies the sign and the edge mask in the composition beyond 3-D."""
    from pycsou_amd.linop import SecondDirectionalDerivative
    g = golden()
    x, y, st = C.make_x(shape, 0), C.make_x(shape, 1), C.steps(shape)
    for field in (True, False):
        v = C.make_dirs(shape, field)
        for edge in C.EDGES:
            op = SecondDirectionalDerivative(shape=shape, directions=v, step=st, edge=edge, dtype=np.dtype(dtype).name)
            got, got_adj = op(x.astype(dtype)), op.adjoint(y.astype(dtype))
            assert rel(got, C.second_dir(x, v, shape, st, edge)) < TOL[dtype]
            assert rel(got_adj, C.second_dir(y, v, shape, st, edge, adjoint=True)) < TOL[dtype]
            assert not got[C.kill_mask(shape) == 0].any()
            if dtype == np.float64:
                assert dot_gap(op) <= 1e-12
                if shape in C.FIXTURE_SHAPES:
                    tag = 'x'.join(map(str, shape)) + f"_{'field' if field else 'const'}_{'edge' if edge else 'noedge'}"
                    assert rel(got, g[f'd2_{tag}_fwd']) < 1e-12 and rel(got_adj, g[f'd2_{tag}_adj']) < 1e-12


def test_second_directional_derivative_short_axis_is_zero():
    from pycsou_amd.linop import SecondDirectionalDerivative
    shape = (3, 9)
    op = SecondDirectionalDerivative(shape=shape, directions=C.make_dirs(shape, True))
    out = op(C.make_x(shape, 0))
    assert out.shape == (27,) and not out.any()
    assert not op.adjoint(C.make_x(shape, 1)).any()     # the mask zeroes the whole input


def test_directional_laplacian_weight_quirk():
    """diff.py:766-774: the first operator enters unweighted, weights[0] = 3 has no effect."""
    from pycsou_amd.linop import DirectionalLaplacian, SecondDirectionalDerivative
    g, shape = golden(), C.LAPLACIAN_SHAPE
    ops = [SecondDirectionalDerivative(shape=shape, directions=C.make_dirs(shape, True, seed=s), step=C.steps(shape))
           for s in (0, 1)]
    L = DirectionalLaplacian(ops, weights=C.LAPLACIAN_WEIGHTS)
    x, y = C.make_x(shape, 0), C.make_x(shape, 1)
    assert rel(L(x), g['lap_fwd']) < 1e-12 and rel(L.adjoint(y), g['lap_adj']) < 1e-12
    assert rel(L(x), ops[0](x) + C.LAPLACIAN_WEIGHTS[1] * ops[1](x)) < 1e-15
    assert dot_gap(L) <= 1e-12


def test_directional_gradient_stack():
    from pycsou_amd.linop import DirectionalGradient, FirstDirectionalDerivative
    shape = (7, 9)
    D1 = FirstDirectionalDerivative(shape, C.make_dirs(shape, True), step=C.steps(shape))
    D2 = FirstDirectionalDerivative(shape, C.make_dirs(shape, False), step=C.steps(shape), kind='forward')
    K = DirectionalGradient([D1, D2])
    x = C.make_x(shape, 0)
    assert np.array_equal(K(x), np.concatenate([D1(x), D2(x)]))
    assert dot_gap(K) <= 1e-12


# ---------------------------------------------------------------- Integration1D
INT_CASES = [((n,), 0) for n in (1, 2, 63, 64, 65, 255, 256, 257, 4099)] \
    + [((5, 6, 7), a) for a in range(3)] + [((3, 257), a) for a in range(2)] + [((257, 3), a) for a in range(2)]


@pytest.mark.parametrize('dtype', DTYPES)
def test_integration1d_normal_data(dtype):
    from pycsou_amd.linop import Integration1D
    g = golden()
    for shape, axis in INT_CASES:
        N = int(np.prod(shape))
        op = Integration1D(size=N, shape=shape, axis=axis, step=C.INT_STEP, dtype=np.dtype(dtype).name)
        x, y = C.make_x(shape, 0), C.make_x(shape, 1)
        got, got_adj = op(x.astype(dtype)), op.adjoint(y.astype(dtype))
        assert got.dtype == dtype
        assert rel(got, C.integ(x, shape, axis, C.INT_STEP)) < TOL[dtype], (shape, axis)
        assert rel(got_adj, C.integ(y, shape, axis, C.INT_STEP, adjoint=True)) < TOL[dtype], (shape, axis)
        if dtype == np.float64:
            assert dot_gap(op) <= 1e-12, (shape, axis)
    if dtype == np.float64:
        for tag, shape, axis in C.integ_cases():
            op = Integration1D(size=int(np.prod(shape)), shape=shape, axis=axis, step=C.INT_STEP)
            assert rel(op(C.make_x(shape, 0)), g[f'int_{tag}_fwd']) < 1e-12
            assert rel(op.adjoint(C.make_x(shape, 1)), g[f'int_{tag}_adj']) < 1e-12


def _int_data(shape, seed=3):
    return np.random.default_rng([seed] + list(shape)).integers(-3, 4, int(np.prod(shape))).astype(np.float64)


def _exact_cases():
    from pycsou_amd import _ops as O
    s, ss = O.CUMSUM_SPAN, O.CUMSUM_SPAN_STRIDED
    return [((70001,), 0), (((1 << 20) + 3,), 0), ((70001, 3), 0), ((3, 70001), 1), ((s + 1,), 0), ((2 * s + 1,), 0),
            ((ss + 1, 3), 0), ((2 * ss + 1, 3), 0), ((2, s + 1), 1)]


@pytest.mark.parametrize('dtype', DTYPES)
def test_integration1d_exact_on_integers(dtype):
    """Integer data in {-3..3}, step 0.5: every partial sum is exact in fp32 and fp64 in any order."""
    from pycsou_amd.linop import Integration1D
    for shape, axis in _exact_cases():
        x = _int_data(shape)
        op = Integration1D(size=x.size, shape=shape, axis=axis, step=0.5, dtype=np.dtype(dtype).name)
        a = x.reshape(shape)
        fwd = 0.5 * np.cumsum(a, axis=axis)
        adj = 0.5 * np.flip(np.cumsum(np.flip(a, axis), axis=axis), axis)
        assert np.abs(fwd).max() * 2 < 2 ** 24
        got, got_adj = op(x.astype(dtype)), op.adjoint(x.astype(dtype))
        assert got.dtype == dtype and np.array_equal(got, fwd.ravel()), (shape, axis)
        assert np.array_equal(got_adj, adj.ravel()), (shape, axis)


@pytest.mark.parametrize('dtype', DTYPES)
def test_cumsum_in_place(dtype):
    """out == x is supported: split and unsplit lines, both layouts, both directions."""
    from pycsou_amd import _ops as O
    for shape, axis in (((257,), 0), ((70001,), 0), ((70001, 3), 0), ((300, 5), 0), ((3, 4099), 1)):
        x = _int_data(shape, seed=4)
        a = x.reshape(shape)
        for reverse in (False, True):
            t = dev(x, dtype)
            out = O.cumsum(t, shape, axis, 0.5, reverse=reverse, out=t)
            assert out.data_ptr() == t.data_ptr()
            ref = 0.5 * (np.flip(np.cumsum(np.flip(a, axis), axis=axis), axis) if reverse else np.cumsum(a, axis=axis))
            assert np.array_equal(t.cpu().numpy(), ref.ravel().astype(dtype)), (shape, axis, reverse)
    t = dev(_int_data((257,)), dtype)
    with pytest.raises(ValueError):   # a strided view is not written as if it were dense
        O.cumsum(t, (257,), 0, 0.5, out=torch.empty(514, dtype=t.dtype, device=t.device)[::2])


# ---------------------------------------------------------------- solvers through the generic path
def _tv(dtype=np.float64):
    from pycsou_amd.func import L1Norm
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.linop import DirectionalGradient, FirstDirectionalDerivative
    from pycsou_amd.opt import PDS
    g = golden()
    shape = C.TV_SHAPE
    N = int(np.prod(shape))
    y, v, vp = C.tv_problem()
    name = np.dtype(dtype).name
    K = DirectionalGradient([FirstDirectionalDerivative(shape=shape, directions=v, dtype=name),
                             FirstDirectionalDerivative(shape=shape, directions=vp, dtype=name)])
    K.lipschitz_cst = K.diff_lipschitz_cst = float(g['tv_Klip'])
    return PDS(dim=N, F=(1 / 2) * SquaredL2Loss(dim=N, data=y.astype(dtype)), H=C.TV_LAM * L1Norm(dim=2 * N), K=K,
               x0=np.zeros(N, dtype), z0=np.zeros(2 * N, dtype), max_iter=C.TV_ITERS - 1, min_iter=C.TV_ITERS - 1,
               accuracy_threshold=0.0, verbose=None, engine='generic')


def test_directional_tv_pds_matches_reference():
    g = golden()
    pds = _tv()
    assert (pds.tau, pds.sigma, pds.rho) == pytest.approx((float(g['tv_tau']), float(g['tv_sigma']), float(g['tv_rho'])),
                                                          rel=1e-14)
    est, _, diag = pds.iterate()
    assert pds._engine is None and pds.iter == int(g['tv_n_iter']) == C.TV_ITERS
    e_x, e_z = rel(est['primal_variable'], g['tv_x']), rel(est['dual_variable'], g['tv_z'])
    print('directional TV fp64: rel x', e_x, 'rel z', e_z)
    assert e_x < 1e-9 and e_z < 1e-9
    np.testing.assert_allclose(diag['Relative Improvement (primal variable)'].to_numpy(float)[1:],
                               g['tv_diag_primal'][1:], rtol=1e-7)
    np.testing.assert_allclose(diag['Relative Improvement (dual variable)'].to_numpy(float)[1:],
                               g['tv_diag_dual'][1:], rtol=1e-7)


def test_directional_tv_pds_fp32():
    g = golden()
    est, _, _ = _tv(np.float32).iterate()
    assert est['primal_variable'].dtype == np.float32
    e_x, e_z = rel(est['primal_variable'], g['tv_x']), rel(est['dual_variable'], g['tv_z'])
    print('directional TV fp32: rel x', e_x, 'rel z', e_z)
    assert e_x < 5e-5 and e_z < 5e-5


def test_directional_tv_graph_bitwise_eager(monkeypatch):
    runs = []
    for graph in ('1', '0'):
        monkeypatch.setenv('PCS_GENERIC_GRAPH', graph)
        pds = _tv()
        est, _, diag = pds.iterate()
        runs.append((pds, est, diag))
    (pg, eg, dg), (pe, ee, de) = runs
    assert getattr(pg, '_graph_used', False) and not getattr(pe, '_graph_used', False)
    assert pg.iter == pe.iter
    for k in ('primal_variable', 'dual_variable'):
        assert np.array_equal(eg[k], ee[k]), k
    for c in dg.columns:
        np.testing.assert_array_equal(dg[c].to_numpy(float), de[c].to_numpy(float))


def test_integration_lasso_apgd_matches_reference():
    """The forward model of the demo at the bottom of pycsou/opt/mcmc.py: S = DownSampling(4) * MovingAverage1D(8),
    F = 1/2 ||y - S I a||^2, G = lam ||a||_1."""
    from pycsou_amd.func import L1Norm
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.linop import DownSampling, Integration1D, MovingAverage1D
    from pycsou_amd.opt.proxalgs import APGD
    g = golden()
    n = C.lasso_signal().size
    S = DownSampling(size=n, downsampling_factor=4) * MovingAverage1D(window_size=8, shape=(n,))
    Gop = S * Integration1D(size=n)
    Gop.lipschitz_cst = Gop.diff_lipschitz_cst = float(g['lasso_Glip'])
    F = (1 / 2) * SquaredL2Loss(dim=S.shape[0], data=g['lasso_y']) * Gop
    s = APGD(dim=n, F=F, G=float(g['lasso_lam']) * L1Norm(dim=n), acceleration='CD', beta=float(g['lasso_beta']),
             max_iter=C.LASSO_ITERS - 1, min_iter=C.LASSO_ITERS - 1, accuracy_threshold=0.0, verbose=None, engine=False)
    assert s.tau == pytest.approx(float(g['lasso_tau']), rel=1e-14)
    est, _, diag = s.iterate()
    assert s.iter == int(g['lasso_n_iter']) == C.LASSO_ITERS
    e_x, e_a = rel(est['iterand'], g['lasso_x']), rel(est['past_aux'], g['lasso_past_aux'])
    print('integration LASSO: rel iterand', e_x, 'rel past_aux', e_a)
    assert e_x < 1e-9 and e_a < 1e-9
    np.testing.assert_allclose(diag['Relative Improvement'].to_numpy(float), g['lasso_diag'], rtol=1e-6)
