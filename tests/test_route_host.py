"""Where every 2-D problem of the element-wise matrix (tests/pointwise.py) is routed, decided on the host: the
solver is built without a GPU, its spec's step arguments are filled by the engines' own builder
(engine.step_args) with fake 16-byte-aligned addresses for the buffers that problem's engine holds, and the
engines' route functions (engine.route_stencil2d, nm_fused_route, forward_normal) take the decision -- only
planning entry points of the library are called, nothing is launched or dereferenced.  Asserted is what
tests/test_gpu_step_pointwise.py::_check_route asserts on a built engine: the kernel path of the case's `path`
column, `march`, `nm_fused` and the final `fkind`.

The case's environment switches are set for the call; PCS_NO_MARCH is read once per process and must be unset,
as in tests/test_host_dispatch.py."""

import ctypes
import itertools
import os

import pytest

from tests import pointwise as PW


def _paths():
    from pycsou_amd import _lib as L
    return {'TILE': L.PCS_PATH_TILE, 'MARCH': L.PCS_PATH_MARCH, 'NMARCH': L.PCS_PATH_NMARCH, 'PT': L.PCS_PATH_PT,
            'SMARCH': L.PCS_PATH_SMARCH, 'SMARCH_NX': L.PCS_PATH_SMARCH_NX, 'NM64': L.PCS_PATH_NM64,
            'stencil_tile': 'stencil_tile'}


def _fake(a, *fields):
    """Distinct fake device addresses on the 16-byte grid for `fields` of the argument struct `a`."""
    for name in fields:
        setattr(a, name, 0x100000 * next(_fake.count))


_fake.count = itertools.count(1)


def _route(spec, dtype, tau, sigma, rho):
    """(engine class, path, Route or None, the final arguments) of a spec, as the engine constructors decide."""
    from pycsou_amd import _lib as L
    from pycsou_amd.opt import engine as E
    lib = L.load()
    cls = E.engine_class(spec)
    fk = spec['fkind']
    a = E.step_args(spec, dtype, tau, sigma, rho, with_k=cls is not E.PDS2DEngine)
    a.fkind = fk
    _fake(a, 'x', 'xn', 'z', 'zn', 'partials')
    sep = spec['conv'].separable(rtol=E.sep_rtol(dtype)) if 'conv' in spec else None
    if cls is E.PDS2DMaskEngine:
        a.mkind = L.PCS_M_L1LOSS
        _fake(a, 'ym', 'zm', 'zmn')
        assert lib.pcs_pds2d_supported(ctypes.byref(a)) == 1
        return cls, int(lib.pcs_pds2d_path(ctypes.byref(a))), None, a
    if cls is E.PDS2DEngine:
        if fk in (L.PCS_F_DENOISE, L.PCS_F_SEPCONV):
            _fake(a, 'y')
        if fk == L.PCS_F_SEPCONV and sep is not None:
            a.half = sep[2]
            _fake(a, 'taps0', 'taps1')
            if E.forward_normal(sep[2], dtype):
                _fake(a, 'cty', 'ntaps')
        elif fk == L.PCS_F_SEPCONV:
            a.fkind = L.PCS_F_GRADBUF
            _fake(a, 'gbuf')
        return cls, int(lib.pcs_pds2d_path(ctypes.byref(a))), None, a
    assert cls is E.PDS2DStencilEngine
    if fk == L.PCS_F_DENOISE:
        _fake(a, 'y')
    elif fk == L.PCS_F_GRADBUF:
        _fake(a, 'gbuf')
        if sep is not None and sep[2] <= 7 and E.stencil_march_on():
            a.fkind, a.half = L.PCS_F_SEPCONV, sep[2]
            _fake(a, 'y', 'taps0', 'taps1', 'cty', 'ntaps')
    r = E.route_stencil2d(lib, a)
    if not r.march:
        assert r.fkind == fk and not r.nm_fused
        return cls, 'stencil_tile', r, None
    a = E.with_fields(a, fkind=r.fkind, **dict.fromkeys(r.drop))
    assert lib.pcs_pds2d_supported(ctypes.byref(a)) == 1
    return cls, int(lib.pcs_pds2d_path(ctypes.byref(a))), r, a


@pytest.mark.parametrize('ik', PW.MATRIX, ids=PW.case_id)
def test_route(ik, monkeypatch):
    import torch
    from pycsou_amd import _lib as L
    from pycsou_amd.opt import engine as E
    assert 'PCS_NO_MARCH' not in os.environ  # read once: this process must never have seen it
    for k in ('PCS_NM64', 'PCS_NMARCH_GEN', 'PCS_SM_FWD', 'PCS_NMARCH', 'PCS_STENCIL_MARCH'):
        monkeypatch.delenv(k, raising=False)
    c, p = PW.case_problem(ik)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    s = PW.build_solver(p, 1, c.engine)
    spec = s._fused_spec()
    dtype = s._compute_dtype()
    assert dtype == (torch.float32 if c.dtype == 'f32' else torch.float64)
    cls, path, r, a = _route(spec, dtype, s.tau, s.sigma, s.rho)
    assert path == _paths()[c.path], (c.path, path)
    if a is not None:
        assert a.dtype == (L.PCS_F32 if c.dtype == 'f32' else L.PCS_F64)
    fkind = r.fkind if r is not None else a.fkind
    if c.row == 'masked':
        assert cls is E.PDS2DMaskEngine and a.mkind == L.PCS_M_L1LOSS
    elif c.engine == 'stencil':
        assert cls is E.PDS2DStencilEngine
        assert r.march == (c.path != 'stencil_tile')
        if p['l0'] and r.march:  # separable PSF: N x inside the one launch, or into the buffer first
            assert fkind == L.PCS_F_SEPCONV and a.cty
            assert r.nm_fused == (c.path in ('NMARCH', 'NM64')), (c.path, r.nm_fused)
            assert bool(a.ntaps) == r.nm_fused
    else:
        assert cls is E.PDS2DEngine
        if c.path == 'NMARCH':
            assert a.cty and a.ntaps
        if c.path == 'MARCH':
            assert not a.cty
    if p['q']:
        assert fkind == L.PCS_F_GRADBUF
