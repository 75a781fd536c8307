"""CPU tier of the Green functions (pycsou/math/green.py) and of the matrix-free MappedDistanceMatrix
(pycsou/linop/sampling.py:772-1058): imports, constructor errors and attributes as in the reference, NumPy
evaluation against the fixture, the three new C-ABI entry points and their argument checks (they run before any
device call), the launch plan, the routing of MappedDistanceMatrix (with ``_ops.mdm_apply`` patched: no compute),
the fixture against this package's own host assembly, and the fp32 model of tests/mdm_cases.py against the bound
the GPU tests use.  No compute calls (no GPU here)."""

import os
import sys

import numpy as np
import pytest

from tests import mdm_cases as C
from tests.cases import GOLDEN, load

CLASSES = ('Matern', 'Wendland', 'CausalGreenIteratedDerivative', 'CausalGreenExponential', 'SubGaussian')
NEW_SYMBOLS = ('pcs_green_eval', 'pcs_mdm_apply', 'pcs_mdm_partials_len')


def green():
    import pycsou_amd.math.green as G
    return G


@pytest.fixture(scope='module')
def gold():
    return load('green_mdm.npz')


# ---------------------------------------------------------------- imports
def test_module_imports():
    G = green()
    for name in CLASSES:
        assert callable(getattr(G, name)), name
    assert tuple(c.__name__ for c in G.GREEN_CLASSES) == CLASSES


def test_module_imports_under_alias():
    import pycsou_amd
    saved = {k: v for k, v in sys.modules.items() if k == 'pycsou' or k.startswith('pycsou.')}
    try:
        pycsou_amd.install_alias('pycsou')
        from pycsou.math.green import (CausalGreenExponential, CausalGreenIteratedDerivative, Matern,  # noqa: F401
                                       SubGaussian, Wendland)
        assert Matern is green().Matern and SubGaussian is green().SubGaussian
    finally:
        for k in [k for k in sys.modules if k == 'pycsou' or k.startswith('pycsou.')]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---------------------------------------------------------------- constructors, attributes, errors
def test_constructor_errors_and_attributes():
    G = green()
    for cls in (G.Matern, G.Wendland):
        for k in (-1, 4, 1.5, 'a'):
            with pytest.raises(TypeError):
                cls(k)
        f = cls(2)
        assert f.k == 2 and f.epsilon == 1.
        f = cls(3, epsilon=0.25)
        assert f.k == 3 and f.epsilon == 0.25
    assert G.Matern(1, 0.5).support() == 1.5 and G.Matern(1, 0.5).support(2) == 1.0 and G.Matern(0).support(sigmas=4) == 4.
    w = G.Wendland(2, 0.75)
    assert w.support == 0.75 and isinstance(w.support, float)        # the instance attribute shadows the method
    for alpha in (0, -1.0):
        with pytest.raises(TypeError):
            G.CausalGreenExponential(1, alpha)
    e = G.CausalGreenExponential(3)
    assert e.k == 3 and e.alpha == 1
    assert G.CausalGreenExponential(2, alpha=1.5).alpha == 1.5 and G.CausalGreenIteratedDerivative(4).k == 4
    for alpha in (0, 2, -0.5, 2.5):
        with pytest.raises(TypeError):
            G.SubGaussian(alpha)
    s = G.SubGaussian(0.8)
    assert s.alpha == 0.8 and s.epsilon == 1.
    assert G.SubGaussian(1.5, epsilon=0.5).epsilon == 0.5


def test_device_specs():
    from pycsou_amd import _lib
    G = green()
    assert G.Matern(2, 0.5)._device_spec() == (_lib.PCS_GREEN_MATERN, 2, 0.5, 0.0)
    assert G.Wendland(3, 0.75)._device_spec() == (_lib.PCS_GREEN_WENDLAND, 3, 0.75, 0.0)
    assert G.SubGaussian(0.8, 0.5)._device_spec() == (_lib.PCS_GREEN_SUBGAUSSIAN, 0, 0.8, 0.5)
    assert G.CausalGreenIteratedDerivative(4)._device_spec() == (_lib.PCS_GREEN_CAUSAL_ITER, 4, 0.0, 0.0)
    assert G.CausalGreenExponential(2, 1.5)._device_spec() == (_lib.PCS_GREEN_CAUSAL_EXP, 2, 1.5, 0.0)
    assert (_lib.PCS_GREEN_MATERN, _lib.PCS_GREEN_WENDLAND, _lib.PCS_GREEN_SUBGAUSSIAN, _lib.PCS_GREEN_CAUSAL_ITER,
            _lib.PCS_GREEN_CAUSAL_EXP) == (0, 1, 2, 3, 4)


def test_negative_arguments_and_scalars():
    G = green()
    neg = np.array([-0.5, -0.0, 0.0, 0.5])
    assert np.array_equal(G.CausalGreenIteratedDerivative(1)(neg), [0, 1, 1, 1])          # 0 ** 0 = 1
    assert np.array_equal(G.CausalGreenIteratedDerivative(2)(neg), [0, 0, 0, 0.5])
    assert np.array_equal(G.CausalGreenExponential(1, 1.5)(neg)[:3], [0, 1, 1])
    with np.errstate(invalid='ignore'):
        s = G.SubGaussian(0.8, 0.5)(neg)
        assert np.isnan(s[0]) and s[2] == 1.0 and np.isnan(G.SubGaussian(0.8, 0.5)(-0.5))
    assert G.Matern(1, 0.5)(np.array([-0.25]))[0] == (1 - np.sqrt(3) * 0.5) * np.exp(np.sqrt(3) * 0.5)
    assert G.Wendland(0, 0.75)(np.array([-0.75, 0.75, 1.0])).tolist() == [4.0, 0.0, 0.0]
    for f in (G.Matern(2, 0.5), G.Wendland(1, 0.75), G.SubGaussian(1.5, 0.5), G.CausalGreenExponential(2, 1.5)):
        v = f(0.3)
        assert np.ndim(v) == 0 and float(v) == float(f(np.array([0.3]))[0])
        assert f(np.ones(3, dtype=np.float32)).dtype == np.float32


def test_cpu_tensor_in_cpu_tensor_out():
    import torch
    G = green()
    for dt in (torch.float32, torch.float64):
        t = torch.tensor([-0.5, 0.0, 0.3, 0.75], dtype=dt)
        for f in (G.Matern(2, 0.5), G.Wendland(1, 0.75), G.SubGaussian(0.8, 0.5), G.CausalGreenExponential(2, 1.5)):
            v = f(t)
            assert isinstance(v, torch.Tensor) and not v.is_cuda and v.dtype == dt and v.shape == t.shape
            with np.errstate(invalid='ignore'):
                assert np.array_equal(v.numpy(), np.asarray(f(t.numpy())).astype(v.numpy().dtype), equal_nan=True)


def test_parameters_without_a_device_form():
    """The reference's constructors accept any k for the causal classes and any epsilon: such instances work on
    the host as there and are never handed to the device as something else."""
    G = green()
    ok = (G.Matern(2, 0.5), G.Wendland(0), G.SubGaussian(0.8, 0.5), G.CausalGreenIteratedDerivative(1),
          G.CausalGreenExponential(np.int64(4), 1.5))
    bad = (G.CausalGreenIteratedDerivative(2.5), G.CausalGreenIteratedDerivative(0), G.CausalGreenExponential(1.5, 1.5),
           G.CausalGreenExponential(0), G.CausalGreenIteratedDerivative(True), G.Matern(1, 0.0), G.Matern(1, -1.0),
           G.Wendland(2, float('inf')), G.Wendland(2, float('nan')), G.SubGaussian(0.8, 0.0), G.SubGaussian(0.8, -1.0))
    assert all(f._device_ok() for f in ok) and not any(f._device_ok() for f in bad)
    from pycsou_amd import _lib
    lib = _lib.load()
    for f in ok + bad:              # _device_ok() is what the library accepts (an empty evaluation: no device call)
        kind, k, p0, p1 = f._device_spec() if f._device_ok() else (0, 0, 0.0, 0.0)
        if f._device_ok():
            assert lib.pcs_green_eval(_lib.PCS_F64, kind, k, p0, p1, None, None, 0, None) == 0
    x = np.array([0.25, 4.0])
    assert np.array_equal(G.CausalGreenIteratedDerivative(2.5)(x), x ** 1.5)
    for f in bad[:4]:
        op = _mdm_op(function=f)
        assert op.matrix_free is False and op.mat is not None and not op.is_dask
    P, Q, _, _ = C.sweep_inputs('radial')
    d = np.linalg.norm(P[:20, None, :] - Q[None, :30, :], axis=-1)
    assert np.array_equal(_mdm_op(function=bad[0]).mat, d ** 1.5)


def test_numpy_evaluation_equals_the_reference(gold):
    G = green()
    assert gold['eval'].shape == (len(C.FUNC_NAMES), C.EVAL_R.size)
    assert np.any(C.EVAL_R == 0) and np.any(C.EVAL_R < 0) and np.any(C.EVAL_R == 0.75) and np.any(C.EVAL_R == 0.5)
    for i, name in enumerate(C.FUNC_NAMES):
        with np.errstate(invalid='ignore'):
            got = C.make(G, name)(C.EVAL_R)
        np.testing.assert_allclose(got, gold['eval'][i], rtol=1e-14, atol=1e-15, equal_nan=True, err_msg=name)
    assert np.isnan(gold['eval'][C.FUNC_NAMES.index('subgauss08')][C.EVAL_R < 0]).all()
    assert not np.isnan(gold['eval'][:8]).any()


# ---------------------------------------------------------------- the fixture
def test_fixture_is_arrays_only_and_small(gold):
    path = os.path.join(GOLDEN, 'green_mdm.npz')
    assert os.path.getsize(path) < 300_000
    assert all(a.dtype.kind in 'fiu' for a in gold.values())      # allow_pickle=False: object arrays would raise
    assert gold['sweep_fwd'].shape == (len(C.FUNC_NAMES), len(C.ORDS), C.SWEEP[0])
    assert gold['sweep_adj'].shape == (len(C.FUNC_NAMES), len(C.ORDS), C.SWEEP[1])
    assert gold['zonal_fwd'].shape == (len(C.ZONAL_FUNCS), C.SWEEP[0])
    assert gold['shape'].shape == (len(C.DIMS), len(C.NCOLS), C.NP)


def _host_op(name, mode, ord, **kw):
    """This package's own host assembly ('dense': no device work at construction)."""
    from pycsou_amd.linop.sampling import MappedDistanceMatrix
    P, Q, x, y = C.sweep_inputs(mode)
    return MappedDistanceMatrix(samples1=P, samples2=Q, function=C.make(green(), name), mode=mode, ord=ord,
                                operator_type='dense', **kw), x, y


@pytest.mark.parametrize('mode', ['radial', 'zonal'])
def test_fixture_equals_the_host_assembly(gold, mode):
    for _, name, o, idx in (c for c in C.sweep_cases() if c[0] == mode):
        op, x, y = _host_op(name, mode, o)
        key = 'sweep' if mode == 'radial' else 'zonal'
        np.testing.assert_allclose(op.mat @ x, gold[f'{key}_fwd'][idx], rtol=1e-12, atol=1e-13, err_msg=f'{name} {o}')
        np.testing.assert_allclose(op.mat.T @ y, gold[f'{key}_adj'][idx], rtol=1e-12, atol=1e-13, err_msg=f'{name} {o}')


# ---------------------------------------------------------------- the C ABI
def test_new_symbols_exported_abi_unchanged():
    from pycsou_amd import _lib, _ops
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pcs_abi_version() == 10 and _lib.ABI_VERSION == 10
    for name in ('mdm_plan', 'mdm_apply', 'green_eval'):
        assert callable(getattr(_ops, name))
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'pycsou_hip.h')).read()
    for name in NEW_SYMBOLS[:2]:
        assert f'int {name}(' in header
    assert 'int64_t pcs_mdm_partials_len(' in header
    for macro, val in (('PCS_GREEN_MATERN', 0), ('PCS_GREEN_WENDLAND', 1), ('PCS_GREEN_SUBGAUSSIAN', 2),
                       ('PCS_GREEN_CAUSAL_ITER', 3), ('PCS_GREEN_CAUSAL_EXP', 4), ('PCS_MDM_RADIAL', 0),
                       ('PCS_MDM_ZONAL', 1), ('PCS_MDM_MAX_DIM', 4), ('PCS_MDM_ROWS', 64), ('PCS_MDM_SLAB', 256),
                       ('PCS_MDM_SMALL_ROWS', 16), ('PCS_MDM_MAX_GROUPS', 1024)):
        assert f'#define {macro} {val}' in header and getattr(_lib, macro) == val


PP, QQ, X, OUT, PA, RR = (0x100000 * k for k in range(1, 7))  # stand-in addresses: never dereferenced


def _mdm(lib, **over):
    from pycsou_amd import _lib
    kw = dict(dtype=_lib.PCS_F32, kind=_lib.PCS_GREEN_MATERN, k=1, p0=0.5, p1=0.0, mode=_lib.PCS_MDM_RADIAL, ord=2.0,
              dim=2, P=PP, nrows=100, Q=QQ, ncols=700, x=X, out=OUT, spg=1, ngroups=3, partials=PA, partials_len=300)
    kw.update(over)
    return lib.pcs_mdm_apply(*[kw[k] for k in ('dtype', 'kind', 'k', 'p0', 'p1', 'mode', 'ord', 'dim', 'P', 'nrows', 'Q',
                                               'ncols', 'x', 'out', 'spg', 'ngroups', 'partials', 'partials_len')], None)


def _kinds():
    from pycsou_amd import _lib
    return _lib


PARAM_BAD = {
    'kind5': dict(kind=5), 'kind_neg': dict(kind=-1),
    'matern_k4': dict(k=4), 'matern_k_neg': dict(k=-1), 'matern_eps0': dict(p0=0.0), 'matern_eps_neg': dict(p0=-0.5),
    'matern_eps_nan': dict(p0=float('nan')),
    'wendland_k4': dict(kind=1, k=4), 'wendland_eps0': dict(kind=1, p0=0.0),
    'subgauss_alpha0': dict(kind=2, p0=0.0, p1=0.5), 'subgauss_alpha2': dict(kind=2, p0=2.0, p1=0.5),
    'subgauss_alpha_neg': dict(kind=2, p0=-0.8, p1=0.5), 'subgauss_eps0': dict(kind=2, p0=0.8, p1=0.0),
    'subgauss_alpha_nan': dict(kind=2, p0=float('nan'), p1=0.5),
    'iter_k0': dict(kind=3, k=0), 'iter_k_neg': dict(kind=3, k=-2),
    'cexp_k0': dict(kind=4, k=0, p0=1.5), 'cexp_alpha0': dict(kind=4, k=1, p0=0.0), 'cexp_alpha_neg': dict(kind=4, k=1, p0=-1.0),
}
MDM_BAD = dict(PARAM_BAD, **{
    'dtype': dict(dtype=2), 'dtype_neg': dict(dtype=-1), 'mode2': dict(mode=2), 'mode_neg': dict(mode=-1),
    'ord0': dict(ord=0.0), 'ord_neg': dict(ord=-1.0), 'ord_nan': dict(ord=float('nan')),
    'dim0': dict(dim=0), 'dim5': dict(dim=5), 'nrows_neg': dict(nrows=-1), 'ncols_neg': dict(ncols=-1),
    'nrows_2p31': dict(nrows=1 << 31), 'ncols_2p31': dict(ncols=1 << 31),
    'spg0': dict(spg=0), 'ngroups0': dict(ngroups=0), 'ngroups_neg': dict(ngroups=-1), 'plan_short': dict(ngroups=2),
    'plan_long': dict(ngroups=4), 'plan_spg2': dict(spg=2), 'plan_one_group': dict(ngroups=1),
    'too_many_groups': dict(ncols=256 * 1025, ngroups=1025, partials_len=1025 * 100),
    'partials': dict(partials=None), 'partials_align': dict(partials=PA + 4), 'partials_short': dict(partials_len=299),
    'partials_len_neg': dict(partials_len=-1),
    'P': dict(P=None), 'Q': dict(Q=None), 'x': dict(x=None), 'out': dict(out=None),
    'alias_P': dict(out=PP), 'alias_P_tail': dict(out=PP + 4 * 199), 'alias_Q': dict(out=QQ + 8), 'alias_x': dict(out=X),
    'alias_x_tail': dict(x=OUT + 4 * 99), 'alias_partials': dict(out=PA + 8), 'alias_partials_Q': dict(partials=QQ + 8),
    'col_form_partials': dict(nrows=4, partials=None), 'col_form_plan': dict(nrows=4, ngroups=2),
})


@pytest.mark.parametrize('bad', sorted(MDM_BAD))
def test_mdm_apply_argument_checks(bad):
    """Every bad-argument case returns PCS_EINVAL before any device call (no GPU here)."""
    from pycsou_amd import _lib
    assert _mdm(_lib.load(), **MDM_BAD[bad]) == -1


def test_mdm_apply_zonal_ignores_ord_and_empty_rows_are_a_no_op():
    """nrows == 0 returns PCS_OK without a launch (there is no device here to launch on): with a radial ord that
    is valid, with a zonal ord of any value, with null arrays and without a workspace."""
    from pycsou_amd import _lib
    lib = _lib.load()
    assert _mdm(lib, nrows=0, partials_len=0) == 0
    assert _mdm(lib, nrows=0, mode=_lib.PCS_MDM_ZONAL, ord=-1.0) == 0
    assert _mdm(lib, nrows=0, mode=_lib.PCS_MDM_ZONAL, ord=float('nan'), P=None, out=None, Q=None, x=None) == 0
    assert _mdm(lib, nrows=0, ncols=0, ngroups=1, partials=None, partials_len=0) == 0
    assert _mdm(lib, nrows=0, ord=0.0) == -1                        # the checks still come first


def _eval(lib, **over):
    from pycsou_amd import _lib
    kw = dict(dtype=_lib.PCS_F64, kind=_lib.PCS_GREEN_MATERN, k=1, p0=0.5, p1=0.0, r=RR, out=OUT, n=100)
    kw.update(over)
    return lib.pcs_green_eval(*[kw[k] for k in ('dtype', 'kind', 'k', 'p0', 'p1', 'r', 'out', 'n')], None)


EVAL_BAD = dict(PARAM_BAD, **{'dtype': dict(dtype=2), 'dtype_neg': dict(dtype=-1), 'n_neg': dict(n=-1), 'r': dict(r=None),
                              'out': dict(out=None), 'alias_shifted': dict(out=RR + 8), 'alias_tail': dict(r=OUT + 8 * 99)})


@pytest.mark.parametrize('bad', sorted(EVAL_BAD))
def test_green_eval_argument_checks(bad):
    from pycsou_amd import _lib
    assert _eval(_lib.load(), **EVAL_BAD[bad]) == -1


def test_green_eval_empty_is_a_no_op():
    from pycsou_amd import _lib
    lib = _lib.load()
    assert _eval(lib, n=0) == 0 and _eval(lib, n=0, r=None, out=None) == 0 and _eval(lib, n=0, k=4) == -1


def test_partials_len():
    from pycsou_amd import _lib
    lib = _lib.load()
    assert lib.pcs_mdm_partials_len(100, 700, 3) == 300 and lib.pcs_mdm_partials_len(100, 700, 1) == 0
    assert lib.pcs_mdm_partials_len(0, 700, 3) == 0 and lib.pcs_mdm_partials_len(4, 0, 1) == 0
    assert lib.pcs_mdm_partials_len((1 << 31) - 1, 5, 1024) == 1024 * ((1 << 31) - 1)
    for bad in ((-1, 5, 1), (5, -1, 1), (5, 5, 0), (5, 5, 1025), (1 << 31, 5, 1), (5, 1 << 31, 1)):
        assert lib.pcs_mdm_partials_len(*bad) == -1, bad


# ---------------------------------------------------------------- the plan
PLAN_ROWS = (0, 1, 4, 16, 17, 63, 64, 65, 130, 1000, 4096, 64 * 1023, 64 * 1023 + 1, 64 * 1024, 65536, 1 << 20)
PLAN_COLS = (0, 1, 255, 256, 257, 600, 4096, 65536, 256 * 1024, 256 * 1025, 1 << 24)


def test_mdm_plan_properties():
    from pycsou_amd import _lib, _ops as O
    lib = _lib.load()
    assert (O.MDM_ROWS, O.MDM_SLAB, O.MDM_SMALL_ROWS, O.MDM_MAX_GROUPS, O.MDM_FILL) == (64, 256, 16, 1024, 1024)
    for nrows in PLAN_ROWS:
        for ncols in PLAN_COLS:
            form, spg, ngroups, need = O.mdm_plan(nrows, ncols)
            nslabs = max(-(-ncols // O.MDM_SLAB), 1)
            assert form == ('col' if nrows <= 16 else 'row'), (nrows, ncols)
            assert spg >= 1 and 1 <= ngroups <= O.MDM_MAX_GROUPS
            assert ngroups == -(-nslabs // spg) and (ngroups - 1) * spg < nslabs <= ngroups * spg   # tiles every slab
            tiles = 1 if form == 'col' else -(-nrows // O.MDM_ROWS)
            if tiles >= O.MDM_FILL:
                assert ngroups == 1                                   # the row tiles alone fill the device
            else:
                most = min(-(-O.MDM_FILL // tiles), O.MDM_MAX_GROUPS)   # groups that fill, capped
                assert ngroups <= most                                # the smallest split that fills: no more
                # ... and no fewer, unless the slabs run out or one slab less per group would pass `most`
                assert tiles * ngroups >= O.MDM_FILL or ngroups == O.MDM_MAX_GROUPS or spg == 1 or \
                    -(-nslabs // (spg - 1)) > most
            assert need == lib.pcs_mdm_partials_len(nrows, ncols, ngroups) == (ngroups * nrows if ngroups > 1 else 0)
            # the library accepts the plan: the plan is checked before the empty product returns
            assert _mdm(lib, nrows=0, ncols=ncols, spg=spg, ngroups=ngroups, partials_len=0) == 0
            assert _mdm(lib, nrows=0, ncols=ncols, spg=spg, ngroups=ngroups + 1, partials_len=0) == -1
    assert O.mdm_plan(65536, 4) == ('row', 1, 1, 0) and O.mdm_plan(4, 65536)[:3] == ('col', 1, 256)
    assert O.mdm_plan(65536, 65536) == ('row', 256, 1, 0) and O.mdm_plan(130, 600) == ('row', 1, 3, 390)
    assert O.mdm_plan(4096, 65536) == ('row', 16, 16, 16 * 4096)
    with pytest.raises(ValueError):
        O.mdm_plan(-1, 5)


# ---------------------------------------------------------------- routing
@pytest.fixture
def calls(monkeypatch):
    """``_ops.mdm_apply`` replaced by a recorder: routing is checked with no compute."""
    from pycsou_amd import _ops as O
    seen = []
    monkeypatch.setattr(O, 'mdm_apply', lambda *a, **k: seen.append((a, k)) or 'patched')
    return seen


def _mdm_op(**kw):
    from pycsou_amd.linop.sampling import MappedDistanceMatrix
    P, Q, _, _ = C.sweep_inputs('radial')
    args = dict(samples1=P[:20], samples2=Q[:30], function=green().Matern(1, 0.5))
    args.update(kw)
    return MappedDistanceMatrix(**args)


def test_recognised_function_with_dask_is_matrix_free(calls):
    G = green()
    for f in (G.Matern(1, 0.5), G.Wendland(2, 0.75), G.SubGaussian(0.8, 0.5), G.CausalGreenIteratedDerivative(2),
              G.CausalGreenExponential(2, 1.5)):
        for dtype in (np.float32, np.float64, 'float32'):
            op = _mdm_op(function=f, dtype=dtype, max_distance=0.1, eps=0.5, chunks=7)      # the three are ignored
            assert op.matrix_free is True and op.mat is None and op.shape == (20, 30)
            assert op.is_dask and op.is_explicit and not op.is_dense and not op.is_sparse and not op.is_symmetric
            assert op._spec == f._device_spec() and op.function is f
    assert _mdm_op().operator_type == 'dask'                         # the default
    sym = _mdm_op(samples2=None)
    assert sym.matrix_free and sym.is_symmetric and sym.shape == (20, 20) and sym.get_adjointOp() is sym
    one_d = _mdm_op(samples1=np.arange(5.), samples2=np.arange(7.))
    assert one_d.matrix_free and one_d.samples1.shape == (5, 1) and one_d.shape == (5, 7)
    assert _mdm_op(mode='zonal').matrix_free
    assert calls == []                                              # construction computes nothing


def test_everything_else_takes_the_host_route(calls):
    from pycsou_amd.linop.base import ExplicitLinearOperator
    G = green()
    f = G.Matern(1, 0.5)
    P5 = np.random.default_rng(5).random((12, 5))
    others = {
        'lambda': _mdm_op(function=lambda d: np.exp(-d)),
        'wrapped': _mdm_op(function=lambda d: f(d)),
        'dense': _mdm_op(operator_type='dense'),
        'sparse': _mdm_op(operator_type='sparse', max_distance=0.3, verbose=0),
        'dim5': _mdm_op(samples1=P5, samples2=P5[:7]),
        'float16': _mdm_op(dtype=np.float16),
    }
    for name, op in others.items():
        assert op.matrix_free is False and op.mat is not None and not op.is_dask and op.is_explicit, name
        assert isinstance(op, ExplicitLinearOperator) and op.is_sparse == (name == 'sparse') and op.is_dense != op.is_sparse
    assert others['float16'].mat.dtype == np.float16 and others['dim5'].shape == (12, 7)
    P, Q, _, _ = C.sweep_inputs('radial')
    ref = f(np.linalg.norm(P[:20, None, :] - Q[None, :30, :], axis=-1))
    assert np.array_equal(others['dense'].mat, ref) and np.array_equal(others['wrapped'].mat, ref)
    assert calls == []


def test_unknown_operator_type_still_raises():
    with pytest.raises(ValueError):
        _mdm_op(operator_type='chunks')
    with pytest.raises(ValueError):
        _mdm_op(operator_type='sparse')          # needs max_distance
    with pytest.raises(ValueError):
        _mdm_op(mode='planar')


# ---------------------------------------------------------------- the model and the bound
def test_fp32_model_stays_within_half_the_bound(gold):
    """The fp32 NumPy model of the kernels' formulas against the fixture, in units of u times the bound: at most
    C / 2 = 16 on every case of the sweep, zonal and causal cases included (forward and adjoint)."""
    G = green()
    worst = {}
    for mode, name, o, idx in C.sweep_cases():
        P, Q, x, y = C.sweep_inputs(mode)
        func = C.make(G, name)
        key = 'sweep' if mode == 'radial' else 'zonal'
        with np.errstate(all='ignore'):
            rf = C.units(C.model(func, P, Q, x, mode, o), gold[f'{key}_fwd'][idx], C.product_bound(func, P, Q, x, mode, o),
                         C.U[np.float32])
            ra = C.units(C.model(func, Q, P, y, mode, o), gold[f'{key}_adj'][idx], C.product_bound(func, Q, P, y, mode, o),
                         C.U[np.float32])
        worst[mode, name, o] = max(rf, ra)
    top = max(worst, key=worst.get)
    print('fp32 model, worst case in units of u x bound:', top, round(worst[top], 2))
    assert worst[top] <= C.C / 2, (top, worst[top])
    assert max(v for (m, *_), v in worst.items() if m == 'radial') > 0.25      # the bound is not slack by orders
