"""GPU tier of the Green functions and of the matrix-free MappedDistanceMatrix (csrc/green_core.hpp, csrc/mdm.hip).

Section A, ``pcs_green_eval``: every class, k and dtype on the fixture's grid (0, the support edges, negative
values), at n in {1, 63, 64, 65, 1000}, held to C u (|phi| + |r phi'|).
Section B, ``pcs_mdm_apply`` one launch at a time: every operand inside a NaN-margined allocation (tests/views.py),
once 16-byte aligned and once at an element offset, ``partials`` in an exact-size buffer under both poison fills
(tests/scratch.py); margins intact, every one of the nrows outputs written and nothing else, results held to the
bound of tests/mdm_cases.py against the fixture.  The shape sweep (nrows across the form switch and a row tile,
ncols across a slab, dim 1..4, the plan's own split and a forced one) runs Matern(1), ord 2; the coverage sweep runs
every (class, k) with every ord and the zonal cases at one shape, forward and adjoint.
Section C, the operator: products against the fixture, the adjoint identity, symmetry, agreement with the dense
operator, Lipschitz constant, todense, one pinv solve and one APGD LASSO.

The largest observed error in units of u x bound per dtype is printed when the module's tests are done (a fixture
finaliser; every test holds its own to C = 32; DESIGN 5.7 records the numbers)."""

import numpy as np
import pytest
import torch

from tests import mdm_cases as C
from tests import scratch as S
from tests import views as V
from tests.cases import load

pytestmark = pytest.mark.gpu
DT = [np.float32, np.float64]
WORST = {}           # (section, dtype name) -> largest error in units of u x bound


@pytest.fixture(scope='module', autouse=True)
def report_worst():
    """Prints, after the module's tests, the largest ratios they observed (each already held to C by its test)."""
    yield
    for key in sorted(WORST):
        print(f'\nlargest error in units of u x bound, {key[0]} {key[1]}: {WORST[key]:.2f} (C = {C.C})')


def note(section, dtype, r):
    key = (section, np.dtype(dtype).name)
    WORST[key] = max(WORST.get(key, 0.0), float(r))
    return r


@pytest.fixture(scope='module')
def gold():
    return load('green_mdm.npz')


def green():
    import pycsou_amd.math.green as G
    return G


_bounds = {}


def shape_bound(dim, nc):
    """sum_k |x_k| (|phi| + d |phi'|) of the shape sweep's 130 rows against Q[:nc], computed once."""
    if (dim, nc) not in _bounds:
        P, Q, x, _ = C.points(dim)
        _bounds[dim, nc] = C.product_bound(C.make(green(), C.SHAPE_FUNC), P, Q[:nc], x[:nc], 'radial', 2.0)
    return _bounds[dim, nc]


def launch(spec, mode, ord, Ph, Qh, xh, dtype, plan, offset, fill='poison_a'):
    """One guarded pcs_mdm_apply: host arrays in, host result out, every guard checked."""
    from pycsou_amd import _lib as L
    lib = L.gpu()
    (nrows, dim), ncols = Ph.shape, Qh.shape[0]
    spg, ngroups = plan
    P, Q, x = (V.guarded(a.reshape(-1), offset, device='cuda', dtype=dtype) for a in (Ph, Qh, xh))
    for v in (P, Q, x):
        if v.numel():                     # an empty view reports no address of its own
            V.assert_misaligned(v, offset)
    out = V.assert_misaligned(V.guarded_out(nrows, dtype, offset, device='cuda'), offset)
    need = lib.pcs_mdm_partials_len(nrows, ncols, ngroups)
    assert need == (ngroups * nrows if ngroups > 1 else 0)
    ws = S.scratch(8 * need, fill, 'cuda') if need else None
    kind, k, p0, p1 = spec
    rc = lib.pcs_mdm_apply(L.dtcode(out), kind, k, p0, p1, L.PCS_MDM_RADIAL if mode == 'radial' else L.PCS_MDM_ZONAL,
                           float(ord), dim, L.ptr(P), nrows, L.ptr(Q), ncols, L.ptr(x), L.ptr(out), spg, ngroups,
                           L.ptr(ws), need, L.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    V.check_guards(P, Q, x, out)
    if ws is not None:
        S.check(ws)
        assert not bool(torch.isnan(ws).any()), 'a partial was never written'
    assert V.unwritten(out) == 0, f'{V.unwritten(out)} output element(s) never written'
    return out.cpu().numpy()


def forced(ncols):
    """One slab per group: 3 groups at 600 columns."""
    return 1, max(-(-ncols // 256), 1)


# ---------------------------------------------------------------- A: pcs_green_eval
@pytest.mark.parametrize('dtype', DT)
def test_green_eval(gold, dtype):
    from pycsou_amd import _ops as O
    G = green()
    u = C.U[dtype]
    for i, name in enumerate(C.FUNC_NAMES):
        f = C.make(G, name)
        with np.errstate(all='ignore'):
            bnd = C.entry_bound(f, C.EVAL_R, 'radial')
        for n in C.EVAL_N:
            r, ref, b = (np.resize(a, n) for a in (C.EVAL_R, gold['eval'][i], bnd))
            t = V.guarded(r, 1, device='cuda', dtype=dtype)
            out = V.guarded_out(n, dtype, 1, device='cuda')
            got = O.green_eval(f._device_spec(), t, out=out)
            torch.cuda.synchronize()
            V.check_guards(t, out)
            assert V.unwritten(out) == 0 or np.isnan(ref).any()
            ratio = note('green_eval', dtype, C.units(got.cpu().numpy(), ref, b, u))
            assert ratio <= C.C, (name, n, ratio)
        called = f(torch.as_tensor(C.EVAL_R).to(device='cuda', dtype=V.tdtype(dtype)))     # the class itself
        assert isinstance(called, torch.Tensor) and called.is_cuda and called.shape == (C.EVAL_R.size,)
        assert C.units(called.cpu().numpy(), gold['eval'][i], bnd, u) <= C.C


def test_green_eval_negative_arguments():
    G = green()
    t = torch.tensor([-0.5, 0.0, 0.5], dtype=torch.float64, device='cuda')
    assert G.CausalGreenIteratedDerivative(1)(t).tolist() == [0.0, 1.0, 1.0]              # the mask; 0 ** 0 = 1
    assert G.CausalGreenExponential(1, 1.5)(t).tolist()[:2] == [0.0, 1.0]
    s = G.SubGaussian(0.8, 0.5)(t)
    assert bool(torch.isnan(s[0])) and float(s[1]) == 1.0
    assert G.Wendland(0, 0.75)(torch.tensor([-0.75, 0.75, 1.0], device='cuda')).tolist() == [4.0, 0.0, 0.0]


# ---------------------------------------------------------------- B: pcs_mdm_apply, one launch at a time
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('dim', C.DIMS)
def test_shape_sweep(gold, dim, dtype):
    """nrows in {1, 4, 16 | 17, 63, 64, 65, 130} (column form | row form, one row tile and past it), ncols in {1,
    255, 256, 257, 600}: the plan's own split and one slab per group, aligned and offset operands."""
    from pycsou_amd import _ops as O
    assert (O.MDM_ROWS, O.MDM_SLAB, O.MDM_SMALL_ROWS) == (64, 256, 16)
    P, Q, x, _ = C.points(dim)
    spec = C.make(green(), C.SHAPE_FUNC)._device_spec()
    u = C.U[dtype]
    for b, nc in enumerate(C.NCOLS):
        ref, bnd = gold['shape'][C.DIMS.index(dim), b], shape_bound(dim, nc)
        for nr in C.NROWS:
            form, spg, ngroups, _ = O.mdm_plan(nr, nc)
            assert form == ('col' if nr <= 16 else 'row')
            runs = [((spg, ngroups), 0, 'poison_a'), ((spg, ngroups), 1, 'poison_b'),
                    (forced(nc), 0, 'poison_b'), (forced(nc), 1, 'poison_a')]
            for plan, offset, fill in runs:
                got = launch(spec, 'radial', 2.0, P[:nr], Q[:nc], x[:nc], dtype, plan, offset, fill)
                ratio = note('mdm_apply', dtype, C.units(got, ref[:nr], bnd[:nr], u))
                assert ratio <= C.C, (dim, nr, nc, plan, offset, ratio)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('mode', ['radial', 'zonal'])
def test_coverage_sweep(gold, mode, dtype):
    """Every (class, k) with every ord (radial) and the zonal cases at 65 x 257, forward and adjoint (257 x 65),
    offset operands, the plan's own split."""
    from pycsou_amd import _ops as O
    G = green()
    P, Q, x, y = C.sweep_inputs(mode)
    if mode == 'zonal':
        assert np.min(np.abs(P @ Q.T)) > 1e-3
    u = C.U[dtype]
    key = 'sweep' if mode == 'radial' else 'zonal'
    for _, name, o, idx in (c for c in C.sweep_cases() if c[0] == mode):
        f = C.make(G, name)
        for tag, A, B, v in (('fwd', P, Q, x), ('adj', Q, P, y)):
            with np.errstate(all='ignore'):
                bnd = C.product_bound(f, A, B, v, mode, o)
            got = launch(f._device_spec(), mode, o, A, B, v, dtype, O.mdm_plan(A.shape[0], B.shape[0])[1:3], 1)
            ratio = note('mdm_apply', dtype, C.units(got, gold[f'{key}_{tag}'][idx], bnd, u))
            assert ratio <= C.C, (mode, name, o, tag, ratio)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('mode', ['radial', 'zonal'])
def test_coverage_sweep_column_form(gold, mode, dtype):
    """The column form (nrows <= 16) with every class and ord and the zonal cases: the first 1, 7 and 16 rows of
    the sweep's forward product (row i depends on P_i alone), the plan's own split and one group."""
    from pycsou_amd import _ops as O
    G = green()
    P, Q, x, _ = C.sweep_inputs(mode)
    u = C.U[dtype]
    key = 'sweep' if mode == 'radial' else 'zonal'
    for _, name, o, idx in (c for c in C.sweep_cases() if c[0] == mode):
        f = C.make(G, name)
        with np.errstate(all='ignore'):
            bnd = C.product_bound(f, P[:16], Q, x, mode, o)
        for nr, plan in ((16, None), (7, (2, 1)), (1, None)):
            form, spg, ngroups, _ = O.mdm_plan(nr, Q.shape[0])
            assert form == 'col'
            got = launch(f._device_spec(), mode, o, P[:nr], Q, x, dtype, plan or (spg, ngroups), 1)
            ratio = note('mdm_apply', dtype, C.units(got, gold[f'{key}_fwd'][idx][:nr], bnd[:nr], u))
            assert ratio <= C.C, (mode, name, o, nr, ratio)


def test_wrapper_checks_and_in_place_evaluation():
    from pycsou_amd import _ops as O
    G = green()
    f = G.Matern(1, 0.5)
    P, Q, x, _ = C.sweep_inputs('radial')
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.array(a)).to(device='cuda', dtype=dt)  # noqa: E731
    Pd, Qd, xd = dev(P), dev(Q), dev(x)
    good = O.mdm_apply(f._device_spec(), 'radial', 2.0, Pd, Qd, xd, plan=(2, 1))
    out = torch.empty(P.shape[0], dtype=torch.float64, device='cuda')
    assert O.mdm_apply(f._device_spec(), 'radial', 2.0, Pd, Qd, xd, plan=(2, 1), out=out) is out and torch.equal(out, good)
    for bad in (torch.empty(P.shape[0] - 1, dtype=torch.float64, device='cuda'),
                torch.empty(P.shape[0], dtype=torch.float32, device='cuda'),
                torch.empty(2 * P.shape[0], dtype=torch.float64, device='cuda')[::2],
                torch.empty(P.shape[0], dtype=torch.float64)):
        with pytest.raises(ValueError):
            O.mdm_apply(f._device_spec(), 'radial', 2.0, Pd, Qd, xd, plan=(2, 1), out=bad)
    r = dev(C.EVAL_R)
    want = O.green_eval(f._device_spec(), r)
    assert O.green_eval(f._device_spec(), r, out=r) is not None and torch.equal(r, want)       # in place
    with pytest.raises(ValueError):                     # k = 2.5 has no device form: no silent truncation
        G.CausalGreenIteratedDerivative(2.5)(dev(C.EVAL_R))


@pytest.mark.parametrize('dtype', DT)
def test_two_calls_return_the_same_bits(dtype):
    from pycsou_amd import _ops as O
    P, Q, x, _ = C.points(3)
    spec = C.make(green(), 'wendland2')._device_spec()
    for nr in (4, 130):                                   # both forms
        for plan in (O.mdm_plan(nr, C.NQ)[1:3], forced(C.NQ), (3, 1)):      # the plan, one slab per group, one group
            a = launch(spec, 'radial', 2.0, P[:nr], Q, x, dtype, plan, 0, 'poison_a')
            b = launch(spec, 'radial', 2.0, P[:nr], Q, x, dtype, plan, 0, 'poison_b')
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (nr, plan)


@pytest.mark.parametrize('dtype', DT)
def test_empty_products(dtype):
    """ncols == 0 writes zeros (both forms); nrows == 0 writes nothing."""
    from pycsou_amd import _lib as L
    P, Q, x, _ = C.points(2)
    spec = C.make(green(), 'subgauss08')._device_spec()
    for nr in (3, 70):
        got = launch(spec, 'radial', 0.8, P[:nr], Q[:0], x[:0], dtype, (1, 1), 1)
        assert got.shape == (nr,) and not np.any(got) and not np.any(np.signbit(got))
    out = V.guarded_out(5, dtype, 1, device='cuda')
    q, xv = V.guarded(Q[:7].reshape(-1), 1, device='cuda', dtype=dtype), V.guarded(x[:7], 1, device='cuda', dtype=dtype)
    kind, k, p0, p1 = spec
    assert L.gpu().pcs_mdm_apply(L.dtcode(out), kind, k, p0, p1, L.PCS_MDM_RADIAL, 2.0, 2, None, 0, L.ptr(q), 7,
                                 L.ptr(xv), L.ptr(out), 1, 1, None, 0, L.stream()) == 0
    torch.cuda.synchronize()
    V.check_guards(out, q, xv)
    assert V.unwritten(out) == 5


# ---------------------------------------------------------------- C: the operator
def make_op(dtype, operator_type='dask', name=C.SHAPE_FUNC, symmetric=False, **kw):
    from pycsou_amd.linop.sampling import MappedDistanceMatrix
    P, Q, _, _ = C.sweep_inputs('radial')
    return MappedDistanceMatrix(samples1=P, samples2=None if symmetric else Q, function=C.make(green(), name),
                                operator_type=operator_type, dtype=dtype, **kw)


def sweep_ref(gold, name=C.SHAPE_FUNC, o=2.0):
    i, j = C.FUNC_NAMES.index(name), C.ORDS.index(o)
    return gold['sweep_fwd'][i, j], gold['sweep_adj'][i, j]


@pytest.mark.parametrize('dtype', DT)
def test_operator_products_and_adjoint_identity(gold, dtype):
    P, Q, x, y = C.sweep_inputs('radial')
    f = C.make(green(), C.SHAPE_FUNC)
    op = make_op(dtype)
    assert op.matrix_free and op.mat is None and op.is_dask and op.shape == C.SWEEP
    fwd, adj = op * x.astype(dtype), op.adjoint(y.astype(dtype))
    assert isinstance(fwd, np.ndarray) and fwd.dtype == dtype and fwd.shape == (C.SWEEP[0],) and adj.shape == (C.SWEEP[1],)
    bf, ba = C.product_bound(f, P, Q, x, 'radial', 2.0), C.product_bound(f, Q, P, y, 'radial', 2.0)
    rf, ra = sweep_ref(gold)
    u = C.U[dtype]
    assert note('operator', dtype, C.units(fwd, rf, bf, u)) <= C.C and note('operator', dtype, C.units(adj, ra, ba, u)) <= C.C
    lhs, rhs = float(np.dot(fwd.astype(np.float64), y)), float(np.dot(x, adj.astype(np.float64)))
    assert abs(lhs - rhs) <= C.C * u * (float(np.abs(y) @ bf) + float(np.abs(x) @ ba)), (lhs, rhs)
    t = torch.as_tensor(x).to(device='cuda', dtype=V.tdtype(dtype))          # a device tensor in, one out
    dev = op(t)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), fwd)
    assert set(op._partials) == {False} and op._partials[False].numel() == 2 * C.SWEEP[0]   # exactly partials_len


@pytest.mark.parametrize('dtype', DT)
def test_symmetric_operator(gold, dtype):
    P, _, _, y = C.sweep_inputs('radial')
    f = C.make(green(), C.SHAPE_FUNC)
    op = make_op(dtype, symmetric=True)
    assert op.matrix_free and op.is_symmetric and op.get_adjointOp() is op and op.shape == (C.SWEEP[0],) * 2
    got = op * y.astype(dtype)
    assert np.array_equal(got, op.adjoint(y.astype(dtype)))
    assert note('operator', dtype, C.units(got, gold['sym_fwd'], C.product_bound(f, P, P, y, 'radial', 2.0), C.U[dtype])) <= C.C


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('name,o', [('matern1', 2.0), ('wendland2', 0.8), ('subgauss15', 1.0)])
def test_agrees_with_the_dense_operator(name, o, dtype):
    P, Q, x, y = C.sweep_inputs('radial')
    f = C.make(green(), name)
    free, dense = make_op(dtype, name=name, ord=o), make_op(dtype, 'dense', name=name, ord=o)
    assert free.matrix_free and not dense.matrix_free and dense.is_dense and dense.mat.dtype == dtype
    u = C.U[dtype]
    assert C.units(free * x.astype(dtype), dense * x.astype(dtype), C.product_bound(f, P, Q, x, 'radial', o), u) <= C.C
    assert C.units(free.adjoint(y.astype(dtype)), dense.adjoint(y.astype(dtype)),
                   C.product_bound(f, Q, P, y, 'radial', o), u) <= C.C


def test_lipschitz_constant_agrees_with_the_dense_operator():
    """The Lanczos tolerance (core/linop.py, _lanczos_extreme, tol = 1e-9 on the eigenvalue of K^T K): a Ritz
    value lies below the eigenvalue by at most tol (relative) at the stop and the returned theta + r above it by at
    most sqrt(tol), so each norm lies in [1 - tol, 1 + sqrt(tol) / 2] times the exact one."""
    free, dense = make_op(np.float64), make_op(np.float64, 'dense')
    free.compute_lipschitz_cst()
    dense.compute_lipschitz_cst()
    exact = float(np.linalg.norm(dense.mat, 2))
    lo, hi = 1 - 1e-9, 1 + np.sqrt(1e-9) / 2
    print('Lipschitz constants: matrix-free', free.lipschitz_cst, 'dense', dense.lipschitz_cst, 'svd', exact)
    assert lo * exact <= free.lipschitz_cst <= hi * exact and lo * exact <= dense.lipschitz_cst <= hi * exact
    assert abs(free.lipschitz_cst - dense.lipschitz_cst) <= (hi - lo) * exact
    assert free.diff_lipschitz_cst == free.lipschitz_cst


@pytest.mark.parametrize('dtype', DT)
def test_todense(dtype):
    P, Q, _, _ = C.sweep_inputs('radial')
    f = C.make(green(), C.SHAPE_FUNC)
    D = make_op(dtype).todense()
    assert D.is_dense and D.mat.is_cuda and tuple(D.mat.shape) == C.SWEEP
    d = C.distances(P, Q, 'radial', 2.0)
    assert note('operator', dtype, C.units(D.mat.cpu().numpy(), f(d), C.entry_bound(f, d, 'radial'), C.U[dtype])) <= C.C


def test_pinv_solve():
    """130 x 40, Matern(0, 0.1), eps = 0.1, held to the bound of tests/pinv_cases.py."""
    from pycsou_amd.linop.sampling import MappedDistanceMatrix
    from tests import pinv_cases as PC
    P, Q, _, y = C.points(2)
    f = green().Matern(0, 0.1)
    op = MappedDistanceMatrix(samples1=P, samples2=Q[:40], function=f)
    assert op.matrix_free and op.shape == (130, 40)
    c = {'A': f(C.distances(P, Q[:40], 'radial', 2.0)), 'eps': 0.1, 'Y': y[None, :]}
    s = np.linalg.svd(c['A'], compute_uv=False)
    assert (s[0] ** 2 + 0.01) / (s[-1] ** 2 + 0.01) < 1e4          # the regularised normal matrix is well conditioned
    x = op.pinv(y, 0.1)
    err, bnd = float(np.linalg.norm(x - PC.solution(c))), PC.bound(c)
    print(f'matrix-free pinv: err {err:.3e} bound {bnd:.3e}')
    assert x.shape == (40,) and err <= bnd


def test_apgd_lasso_matches_the_dense_operator():
    from pycsou_amd.func import L1Norm
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.opt.proxalgs import APGD
    P, Q, x, _ = C.sweep_inputs('radial')
    n = Q.shape[0]
    truth = np.where(np.arange(n) % 16 == 0, x, 0.0)
    ops = {kind: make_op(np.float64, kind) for kind in ('dask', 'dense')}
    assert ops['dask'].matrix_free and not ops['dense'].matrix_free
    data, lip = ops['dense'].mat @ truth, float(np.linalg.norm(ops['dense'].mat, 2))
    out = {}
    for kind, Phi in ops.items():
        Phi.lipschitz_cst = Phi.diff_lipschitz_cst = lip
        F = (1 / 2) * SquaredL2Loss(dim=P.shape[0], data=data) * Phi
        s = APGD(dim=n, F=F, G=0.05 * L1Norm(dim=n), acceleration='CD', beta=lip ** 2, max_iter=19, min_iter=19,
                 accuracy_threshold=0.0, verbose=None, engine=False)
        out[kind], _, _ = s.iterate()
        assert s.iter == 20
    a, b = out['dask']['iterand'], out['dense']['iterand']
    rel = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    print('APGD LASSO, matrix-free against dense: rel', rel)
    assert np.count_nonzero(b) > 0 and rel <= 1e-10


