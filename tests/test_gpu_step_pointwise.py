"""One and two iterations of every fused 2-D step kernel from a generic state, compared element by element
with the fp64 oracle (tests/pointwise.py: inputs, oracle, derived rounding bound c eps M, comparator;
tests/test_step_pointwise_cpu.py proves what they rely on).

Unlike the 12-iteration relative-L2 tests of these kernels, the start (x0, z0) is not zero, so N x, K^T z and
the (1 - rho) terms act from the first iteration and the first diagnostics row is a number; the PSF taps
are about 1 / len each and not symmetric, so every tap and every edge-table entry of N = Conv^T Conv is
far above the bound; every element is checked, so one wrong value at a strip seam, a segment seam or a
corner fails; and prox_G (Segment(0.25, 0.75) / nonneg) and the dual projection bind on 15-60 % of the
elements, both outcomes inside every wave.  nit = 1 reads buffer parity 0 and nit = 2 both parities, with
the deferred finalization of the diagnostics in between.

Every case asserts the kernel path it is about (pcs_pds2d_path on the engine's arguments, the engine's
march / nm_fused flags), so a routing change cannot move it to another kernel unnoticed.  The matrix is
tests/pointwise.py CONFIGS.  Each case prints its worst error in units of eps M (DESIGN.md records them)."""

import ctypes

import numpy as np
import pytest

from tests import pointwise as PW

pytestmark = pytest.mark.gpu


def _paths():
    from pycsou_amd import _lib as L
    return {'TILE': L.PCS_PATH_TILE, 'MARCH': L.PCS_PATH_MARCH, 'NMARCH': L.PCS_PATH_NMARCH, 'PT': L.PCS_PATH_PT,
            'SMARCH': L.PCS_PATH_SMARCH, 'SMARCH_NX': L.PCS_PATH_SMARCH_NX, 'NM64': L.PCS_PATH_NM64,
            'stencil_tile': 'stencil_tile'}


def _check_route(c, p, eng):
    from pycsou_amd import _lib as L
    from pycsou_amd.opt.engine import PDS2DEngine, PDS2DMaskEngine, PDS2DStencilEngine
    path = PW.engine_path(eng)
    assert path == _paths()[c.path], (c.path, path)
    assert eng.args.dtype == (L.PCS_F32 if c.dtype == 'f32' else L.PCS_F64)
    if c.row == 'masked':
        assert isinstance(eng, PDS2DMaskEngine) and eng.args.mkind == L.PCS_M_L1LOSS
    elif c.engine == 'stencil':
        assert isinstance(eng, PDS2DStencilEngine)
        assert eng.march == (c.path != 'stencil_tile')
        if p['l0'] and eng.march:  # separable PSF: N x inside the one launch, or into the buffer first
            assert eng.fkind == L.PCS_F_SEPCONV and eng.cty is not None
            assert eng.nm_fused == (c.path in ('NMARCH', 'NM64')), (c.path, eng.nm_fused)
    else:
        assert type(eng) is PDS2DEngine
        if c.path == 'NMARCH':
            assert eng.args.cty and eng.args.ntaps
        if c.path == 'MARCH':
            assert not eng.args.cty
    if p['q']:
        assert eng.fkind == L.PCS_F_GRADBUF and eng.plans[0] is not None and eng.plans[1] is not None


def _check(tag, p, nit, s, est, diag):
    """x, z and the diagnostics of a finished run against the oracle; prints the ratios."""
    xr, zr, dr, _ = PW.oracle_steps(p, nit)
    assert s.iter == nit
    x, z = est['primal_variable'], est['dual_variable']
    assert x.dtype == p['dtype'] and z.dtype == p['dtype']
    b = PW.bound(p, nit)
    m, shape = p['m'], p['shape']
    rx = PW.compare(x, xr, b['x'], shape, 'x', diag=diag, diag_ref=dr, dtype=p['dtype'])
    rz = PW.compare(z[m:], zr[m:], b['z'], shape, 'z')
    if m:  # the masked dual block, in the order of the sampled pixels
        rz = max(rz, PW.compare(z[:m], zr[:m], b['z'], (1, m), 'z_m'))
    print(f'POINTWISE {tag} nit={nit} c={b["x"].c} x={rx:.2f} z={rz:.2f}')


@pytest.mark.parametrize('ik', PW.MATRIX, ids=PW.case_id)
def test_steps_elementwise(ik, monkeypatch):
    c, p = PW.case_problem(ik)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    for nit in (1, 2):
        s = PW.build_solver(p, nit, c.engine)
        est, _, diag = s.iterate()
        assert s._engine is not None, 'the fused engine must take this problem'
        _check_route(c, p, s._engine)
        _check(PW.case_id(ik), p, nit, s, est, diag)


@pytest.mark.parametrize('bands', [0, 1])
def test_run_loop_from_c(bands, monkeypatch):
    """pcs_pds2d_run (chunks launched from C, deferred finalization; single launch per iteration and the
    band-paired schedule) on the forward normal-operator march, three iterations."""
    import pycsou_amd.opt.engine as E
    from pycsou_amd import _lib as L
    monkeypatch.setenv('PCS_RUN_BANDS', str(bands))
    monkeypatch.setattr(E, 'NATIVE_MIN_PIXELS', 1)
    monkeypatch.setattr(E, 'DEFER_FIN', True)
    p = PW.make_problem(PW.A, 'forward', 'l21', 'sep15', 'segment', lam=PW.LAM, seed=77, dtype=np.float32)
    s = PW.build_solver(p, 3, 'fused')
    est, _, diag = s.iterate()
    eng = s._engine
    assert eng is not None and eng.native and eng.defer
    assert PW.engine_path(eng) == L.PCS_PATH_NMARCH
    out = (ctypes.c_int64 * 6)()
    assert eng.lib.pcs_pds2d_run_plan(ctypes.byref(eng.args), -1, 0, out) == 0
    assert int(out[0]) == bands, 'the schedule under test did not engage'
    _check(f'run-bands{bands}-forward-sep15-l21-segment-150x200', p, 3, s, est, diag)
