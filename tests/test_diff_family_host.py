"""CPU tier of the directional derivatives and Integration1D (pycsou/linop/diff.py:380-774, 1071-1137; peaks:
pycsou/util/misc.py:91-127): names, types, shapes and errors as in the reference; the closed-form norm of
Integration1D against dense SVD; the new C-ABI entry points' argument checks (they run before any device call);
and the fixture checked against the NumPy definitions of tests/diff_family_cases.py.  No compute calls (no GPU
here)."""

import os
import sys

import numpy as np
import pytest

from tests import diff_family_cases as C
from tests.cases import GOLDEN, load

NAMES = ('FirstDirectionalDerivative', 'SecondDirectionalDerivative', 'DirectionalGradient', 'DirectionalLaplacian',
         'Integration1D', 'peaks')
NEW_SYMBOLS = ('pcs_dirderiv_fwd', 'pcs_dirderiv_adj', 'pcs_cumsum', 'pcs_cumsum_ws_bytes')


def test_reference_names_import():
    import importlib
    for mod in ('pycsou_amd.linop.diff', 'pycsou_amd.linop'):
        m = importlib.import_module(mod)
        for name in NAMES:
            assert callable(getattr(m, name)), (mod, name)
    from pycsou_amd.util.misc import peaks  # noqa: F401


def test_reference_names_import_under_alias():
    import pycsou_amd
    saved = {k: v for k, v in sys.modules.items() if k == 'pycsou' or k.startswith('pycsou.')}
    try:
        pycsou_amd.install_alias('pycsou')
        from pycsou.linop.diff import (DirectionalGradient, DirectionalLaplacian,  # noqa: F401
                                       FirstDirectionalDerivative, Integration1D, SecondDirectionalDerivative)
        from pycsou.linop import Integration1D as I2, MovingAverage1D, DownSampling  # noqa: F401  (mcmc.py demo)
        from pycsou.util.misc import peaks
        assert I2 is Integration1D and callable(peaks)
    finally:
        for k in [k for k in sys.modules if k == 'pycsou' or k.startswith('pycsou.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_types_shapes_and_errors():
    from pycsou_amd.core.linop import LinearOperator, LinOpSum
    from pycsou_amd.linop import (DirectionalGradient, DirectionalLaplacian, FirstDirectionalDerivative,
                                  Integration1D, LinOpVStack, SecondDirectionalDerivative)
    shape, N = (7, 9), 63
    field = C.make_dirs(shape, True)
    for d in ([1, 0], field, field.reshape(2, 7, 9), field.ravel()):
        D = FirstDirectionalDerivative(shape=shape, directions=d)
        assert isinstance(D, LinearOperator) and D.shape == (N, N) and D.kind == 'centered' and D.edge is True
        assert D.dtype == np.float64 and D.is_field == (np.size(d) != 2)
    assert np.array_equal(FirstDirectionalDerivative(shape, [3, 4]).directions, [3.0, 4.0])  # not normalised
    for bad in ([1, 0, 0], np.ones((2, 62)), np.ones(N)):
        with pytest.raises(ValueError):
            FirstDirectionalDerivative(shape=shape, directions=bad)
        with pytest.raises(ValueError):
            SecondDirectionalDerivative(shape=shape, directions=bad)
    with pytest.raises(NotImplementedError):
        FirstDirectionalDerivative(shape=shape, directions=[1, 0], kind='central')
    D1, D2 = FirstDirectionalDerivative(shape, [1, 0]), FirstDirectionalDerivative(shape, field, dtype='float32')
    K = DirectionalGradient([D1, D2])
    assert isinstance(K, LinOpVStack) and K.shape == (2 * N, N) and K.linops[0] is D1 and K.linops[1] is D2
    S1, S2 = SecondDirectionalDerivative(shape, [1, 0]), SecondDirectionalDerivative(shape, field, step=(0.5, 2.0))
    assert S1.shape == (N, N) and S2.steps == [0.5, 2.0] and np.array_equal(S1.kill_edges, C.kill_mask(shape))
    L = DirectionalLaplacian([S1, S2], weights=[3, 0.5])
    assert isinstance(L, LinOpSum) and L.shape == (N, N) and L.LinOp1 is S1      # the first operator unweighted
    assert DirectionalLaplacian([S1]) is S1
    with pytest.raises(ValueError):
        DirectionalLaplacian([S1, S2], weights=[1.0])
    I = Integration1D(size=210, shape=(5, 6, 7), axis=1, step=0.5)
    assert isinstance(I, LinearOperator) and I.shape == (210, 210) and (I.axis, I.step) == (1, 0.5)
    assert Integration1D(size=9).dims == (9,) and Integration1D(size=9).dtype == np.float64
    with pytest.raises(ValueError):
        Integration1D(size=211, shape=(5, 6, 7))


@pytest.mark.parametrize('n', [1, 2, 5, 64, 257])
def test_integration_norm_is_exact(n):
    from pycsou_amd.linop import Integration1D
    I = Integration1D(size=3 * n, shape=(3, n), axis=1, step=0.5)
    I.compute_lipschitz_cst()
    exact = np.linalg.norm(0.5 * np.tril(np.ones((n, n))), 2)
    assert abs(I.lipschitz_cst - exact) <= 1e-12 * exact and I.diff_lipschitz_cst == I.lipschitz_cst


def test_new_symbols_exported_abi_unchanged():
    from pycsou_amd import _lib, _ops
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pcs_abi_version() == 10 and _lib.ABI_VERSION == 10
    assert (_ops.CUMSUM_SPAN, _ops.CUMSUM_SPAN_STRIDED) == (2048, 64)


X, V, OUT, WS = 0x10000, 0x18000, 0x20000, 0x30000  # stand-in addresses: never dereferenced


def _dirderiv(lib, which, **over):
    from pycsou_amd import _lib
    kw = dict(dtype=_lib.PCS_F64, x=X, v=V, field=0, out=OUT, ndim=2, dims=[7, 9], steps=[1.0, 1.0], kind=2, edge=1,
              scale=1.0, kill=0)
    kw.update(over)
    fn = lib.pcs_dirderiv_fwd if which == 'fwd' else lib.pcs_dirderiv_adj
    dims = None if kw['dims'] is None else _lib.i64s(kw['dims'])
    steps = None if kw['steps'] is None else _lib.dbls(kw['steps'])
    return fn(kw['dtype'], kw['x'], kw['v'], kw['field'], kw['out'], kw['ndim'], dims, steps, kw['kind'], kw['edge'],
              kw['scale'], kw['kill'], None)


@pytest.mark.parametrize('which', ['fwd', 'adj'])
@pytest.mark.parametrize('bad', ['dtype', 'x', 'v', 'out', 'dims', 'steps', 'ndim0', 'ndim4', 'dim_neg', 'kind_lo',
                                 'kind_hi', 'kill1', 'kill3', 'alias'])
def test_dirderiv_argument_checks(which, bad):
    """Every bad-argument case returns PCS_EINVAL before any device call (no GPU here)."""
    from pycsou_amd import _lib
    over = {'dtype': dict(dtype=2), 'x': dict(x=None), 'v': dict(v=None), 'out': dict(out=None), 'dims': dict(dims=None),
            'steps': dict(steps=None), 'ndim0': dict(ndim=0), 'ndim4': dict(ndim=4, dims=[2, 3, 4, 5], steps=[1.0] * 4),
            'dim_neg': dict(dims=[7, -1]), 'kind_lo': dict(kind=-1), 'kind_hi': dict(kind=3), 'kill1': dict(kill=1),
            'kill3': dict(kill=3), 'alias': dict(out=X)}[bad]
    assert _dirderiv(_lib.load(), which, **over) == -1


def _cumsum(lib, **over):
    from pycsou_amd import _lib
    kw = dict(dtype=_lib.PCS_F32, x=X, out=OUT, ndim=1, dims=[4099], axis=0, step=0.5, reverse=0, ws=WS)
    kw.update(over)
    dims = None if kw['dims'] is None else _lib.i64s(kw['dims'])
    return lib.pcs_cumsum(kw['dtype'], kw['x'], kw['out'], kw['ndim'], dims, kw['axis'], kw['step'], kw['reverse'],
                          kw['ws'], None)


@pytest.mark.parametrize('bad', ['dtype', 'x', 'out', 'dims', 'ndim0', 'ndim33', 'axis_lo', 'axis_hi', 'dim_neg', 'ws',
                                 'ws_align', 'ws_strided'])
def test_cumsum_argument_checks(bad):
    from pycsou_amd import _lib
    over = {'dtype': dict(dtype=2), 'x': dict(x=None), 'out': dict(out=None), 'dims': dict(dims=None),
            'ndim0': dict(ndim=0), 'ndim33': dict(ndim=33, dims=[1] * 33), 'axis_lo': dict(axis=-1),
            'axis_hi': dict(axis=1), 'dim_neg': dict(ndim=2, dims=[5, -2]), 'ws': dict(ws=None),
            'ws_align': dict(ws=WS + 4), 'ws_strided': dict(ndim=2, dims=[70001, 3], ws=None)}[bad]
    assert _cumsum(_lib.load(), **over) == -1


def test_cumsum_ws_bytes():
    from pycsou_amd import _lib
    lib = _lib.load()

    def ws(dims, axis):
        return int(lib.pcs_cumsum_ws_bytes(len(dims), _lib.i64s(dims), axis))

    assert ws([_lib.PCS_CUMSUM_SPAN], 0) == 0 and ws([_lib.PCS_CUMSUM_SPAN + 1], 0) == 16   # one / two segments
    assert ws([_lib.PCS_CUMSUM_SPAN_STRIDED, 3], 0) == 0 and ws([_lib.PCS_CUMSUM_SPAN_STRIDED + 1, 3], 0) == 48
    assert ws([4096, 4096], 1) == 0                                              # enough lines: never split
    for dims, axis in (([1], 0), ([1, 3], 0), ([3, 1], 1)):
        sizes = []
        for n in (1, 2, 63, 64, 65, 2048, 2049, 4097, 70001, 1 << 20, (1 << 20) + 3, (1 << 23) + 1, 1 << 24, 1 << 30,
                  1 << 40):
            d = list(dims)
            d[axis] = n
            sizes.append(ws(d, axis))
        assert all(0 <= a <= b <= _lib.PCS_CUMSUM_WS_MAX for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] % 8 == 0
    assert lib.pcs_cumsum_ws_bytes(1, None, 0) == -1 and ws([8], 1) == -1 and ws([8], -1) == -1
    assert ws([8, -1], 0) == -1 and lib.pcs_cumsum_ws_bytes(0, _lib.i64s([8]), 0) == -1
    assert ws([0, 5], 1) == 0


def test_zero_size_calls_are_noops():
    from pycsou_amd import _lib
    lib = _lib.load()
    for dt in (_lib.PCS_F32, _lib.PCS_F64):
        assert _cumsum(lib, dtype=dt, dims=[0], ws=None) == 0
        assert _cumsum(lib, dtype=dt, ndim=3, dims=[5, 0, 7], axis=2, ws=None) == 0
        for which in ('fwd', 'adj'):
            assert _dirderiv(lib, which, dtype=dt, dims=[0, 9]) == 0
            assert _dirderiv(lib, which, dtype=dt, ndim=3, dims=[4, 5, 0], steps=[1.0] * 3, field=1, kill=2) == 0


# ---------------------------------------------------------------- the fixture
def test_fixture_is_arrays_only_and_small():
    path = os.path.join(GOLDEN, 'diff_family.npz')
    assert os.path.getsize(path) < 1_000_000
    g = load('diff_family.npz')                 # allow_pickle=False: object arrays would raise
    assert all(a.dtype.kind in 'fiu' for a in g.values())


def _close(got, ref):
    assert np.max(np.abs(got - ref)) <= 16 * np.finfo(np.float64).eps * np.max(np.abs(ref))


def test_fixture_vectors_equal_the_definitions():
    g = load('diff_family.npz')
    for tag, shape, field, kind, edge in C.vector_cases():
        x, y, v = C.make_x(shape, 0), C.make_x(shape, 1), C.make_dirs(shape, field)
        _close(g[f'd1_{tag}_fwd'], C.first_dir(x, v, shape, C.steps(shape), kind, edge))
        _close(g[f'd1_{tag}_adj'], C.first_dir(y, v, shape, C.steps(shape), kind, edge, adjoint=True))
    for tag, shape, field, edge in C.second_cases():
        x, y, v = C.make_x(shape, 0), C.make_x(shape, 1), C.make_dirs(shape, field)
        fwd = g[f'd2_{tag}_fwd']
        _close(fwd, C.second_dir(x, v, shape, C.steps(shape), edge))
        _close(g[f'd2_{tag}_adj'], C.second_dir(y, v, shape, C.steps(shape), edge, adjoint=True))
        assert not fwd[C.kill_mask(shape) == 0].any() and fwd[C.kill_mask(shape) == 1].all()
    shape, (w0, w1) = C.LAPLACIAN_SHAPE, C.LAPLACIAN_WEIGHTS
    v0, v1 = C.make_dirs(shape, True, seed=0), C.make_dirs(shape, True, seed=1)
    for key, arg, adj in (('lap_fwd', C.make_x(shape, 0), False), ('lap_adj', C.make_x(shape, 1), True)):
        quirk = C.second_dir(arg, v0, shape, C.steps(shape), True, adjoint=adj) \
            + w1 * C.second_dir(arg, v1, shape, C.steps(shape), True, adjoint=adj)      # weights[0] = 3 is not applied
        _close(g[key], quirk)
    for tag, shape, axis in C.integ_cases():
        assert np.array_equal(g[f'int_{tag}_fwd'], C.integ(C.make_x(shape, 0), shape, axis, C.INT_STEP))
        assert np.array_equal(g[f'int_{tag}_adj'], C.integ(C.make_x(shape, 1), shape, axis, C.INT_STEP, adjoint=True))
        assert np.array_equal(g[f'int_{tag}_fwd'],
                              (C.INT_STEP * np.cumsum(C.make_x(shape, 0).reshape(shape), axis=axis)).ravel())


def test_peaks_matches_reference():
    from pycsou_amd.util.misc import peaks
    g = load('diff_family.npz')
    t = np.linspace(-2.5, 2.5, 25)
    got = peaks(*np.meshgrid(t, t))
    assert got.shape == (25, 25) and np.max(np.abs(got - g['peaks25'])) <= 16 * np.finfo(np.float64).eps * 8.1
    assert abs(peaks(0.0, 0.0) - (3 * np.exp(-1) - np.exp(-1) / 3)) < 1e-15
