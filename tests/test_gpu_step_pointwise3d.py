"""One and two iterations of every route of the fused 3-D PDS engine from a generic state, compared element
by element with the fp64 oracle (tests/pointwise3d.py: inputs, oracle, derived rounding bound c eps M, the
matrix; tests/test_step_pointwise3d_cpu.py proves what they rely on).

Unlike the relative-L2 tests of these kernels, the start (x0, z0) is not zero, so K^T z, the (1 - rho) terms
and the z ring prologue at every plane-segment seam carry data from the first iteration and the first
diagnostics row is a number; the taps differ per axis, are about 1 / len each and not symmetric; the steps
differ per axis on most routes; prox_G (Segment(0.25, 0.75) / nonneg) and the dual projection bind inside
every wave; and every voxel of x and of the three components of z is checked.  nit = 1 reads buffer parity 0
and nit = 2 both parities.

Every case asserts the route it is about (the engine's kkind, fkind, ata, fold, fused0, sep2 and the launch
arguments' gkind / hkind / edge) and that its launch has at least two plane segments, so a routing change
cannot move it to another kernel unnoticed.  Each case prints its worst error in units of eps M (DESIGN.md
records them)."""

import numpy as np
import pytest
import torch

from tests import pointwise3d as PW

pytestmark = pytest.mark.gpu


def _check_route(c, p, eng):
    from pycsou_amd import _lib as L
    from pycsou_amd.opt.engine3d import PDS3DEngine
    assert isinstance(eng, PDS3DEngine)
    fname, ata, fold, fused0, sep2 = PW.ROUTES[c.route]
    a = eng.args[0]
    assert a.dtype == (L.PCS_F32 if c.dtype == 'f32' else L.PCS_F64)
    assert eng.kkind == {'forward': L.PCS_FORWARD, 'backward': L.PCS_BACKWARD, 'centered': L.PCS_CENTERED}[c.kind]
    assert a.kkind == eng.kkind
    assert eng.fkind == getattr(L, 'PCS_F_' + fname), (c.route, eng.fkind)
    assert a.fkind == (L.PCS_F_CONV0 if fold else eng.fkind), (c.route, a.fkind)
    got = (eng.ata, eng.fold, getattr(eng, 'fused0', None), getattr(eng, 'sep2', None))
    assert got == (ata, fold, fused0, sep2), (c.route, got)
    assert a.gkind == {'': L.PCS_G_NULL, 'nonneg': L.PCS_G_NONNEG, 'segment': L.PCS_G_SEGMENT}[p['gname']]
    assert a.hkind == (L.PCS_H_L21 if p['hname'] == 'l21' else L.PCS_H_L1)
    assert a.edge == int(c.edge)
    assert (a.step0, a.step1, a.step2) == tuple(c.steps)
    if p['gname'] == 'segment':
        assert (a.seg_a, a.seg_b) == PW.SEG
    t1, tw = PW.update_tile(c.kind, p['dtype'])
    tiles = -(-c.shape[1] // t1) * -(-c.shape[2] // tw)
    assert eng.nblocks >= 2 * tiles and eng.nblocks % tiles == 0, (eng.nblocks, tiles)


def _oracle(p):
    """{nit: (x, z, diag)} for nit = 1, 2 from one oracle run of two iterations."""
    first = {}
    x, z, d, _ = PW.oracle_steps(p, 2, first=first)
    d1 = {'primal': d['primal'][:1], 'dual': d['dual'][:1]}
    return {1: (first['x'], first['z'], d1), 2: (x, z, d)}


def _check(tag, p, nit, ref, n, x, z, diag):
    """x, z and the diagnostics of a finished run against the oracle; prints the ratios."""
    xr, zr, dr = ref
    assert n == nit
    b = PW.bound(p, nit)
    rx = PW.compare(x, xr, b['x'], p['shape'], 'x', diag=diag, diag_ref=dr, dtype=p['dtype'])
    rz = PW.compare(z, zr, b['z'], p['shape'], 'z')  # all three components, the worst one named
    print(f'POINTWISE3D {tag} nit={nit} c={b["x"].c} x={rx:.2f} z={rz:.2f}')


@pytest.mark.parametrize('ik', PW.MATRIX, ids=PW.case_id)
def test_steps_elementwise(ik, monkeypatch):
    c, p = PW.case_problem(ik)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    ref = _oracle(p)
    for nit in (1, 2):
        s = PW.build_solver(p, nit)
        est, _, diag = s.iterate()
        assert s._engine is not None, 'the fused engine must take this problem'
        _check_route(c, p, s._engine)
        x, z = est['primal_variable'], est['dual_variable']
        assert x.dtype == p['dtype'] and z.dtype == p['dtype']
        _check(PW.case_id(ik), p, nit, ref[nit], s.iter, x, z, diag)


SB = (30, 20, 132)  # taps 3 x 15 x 6: x halo 3 planes, boundary bands of 4; 3 slabs of 10 planes are banded
SLABS = {
    'forward-blur': (SB, 'forward', 'sep3x15x6', np.float32, 'l21'),
    'centered-blur': (SB, 'centered', 'sep3x15x6', np.float64, 'l1'),
    'backward-denoise': (PW.VB, 'backward', 'denoise', np.float32, 'l21'),
}


@pytest.mark.parametrize('name', list(SLABS))
def test_slabs_from_a_generic_state(name):
    """Plane slabs in one process (world 2 and 3) from a non-zero (x0, z0) with G = Segment and steps
    (2, 0.5, 1), two iterations: the halos of x0 and z0 carry data from the first iteration.  x and z are
    bitwise the single-GPU engine's, which is checked element-wise against the oracle here.  The blur
    problems at world 3 take the banded schedule (boundary bands, then the interior)."""
    from pycsou_amd.opt.engine3d import PDS3DEngine
    from pycsou_amd.parallel import run_local
    shape, kind, fk, dtype, hname = SLABS[name]
    p = PW.make_problem(shape, kind, hname, fk, 'segment', steps=PW.NU, lam=PW.LAM, seed=500 + len(name), dtype=dtype)
    nit = 2
    pds = PW.build_solver(p, nit)
    spec = pds._fused_spec()
    assert spec is not None and spec.get('ndim') == 3
    dt = pds._compute_dtype()
    run = (pds.max_iter, pds.min_iter, pds.accuracy_threshold)
    one = PDS3DEngine(spec, dt, pds.tau, pds.sigma, pds.rho, pds.x0, pds.z0)
    n1, x1, z1, h1 = one.run(*run)
    diag = {'primal': h1[:, 0], 'dual': h1[:, 1]}
    _check(f'slab-{name}-single', p, nit, _oracle(p)[nit], n1, x1.cpu().numpy(), z1.cpu().numpy(), diag)
    for world in (2, 3):
        slabs = [PDS3DEngine(spec, dt, pds.tau, pds.sigma, pds.rho, pds.x0, pds.z0, rank=r, world=world)
                 for r in range(world)]
        split = world == 3 and fk.startswith('sep')
        if split:
            assert all(s.banded for s in slabs) and slabs[0].hx == 3 and slabs[0].band == 4
        res = run_local(slabs, *run, split=split)
        assert all(r[0] == n1 for r in res)
        x2 = torch.cat([r[1] for r in res])
        z2 = torch.cat([torch.cat([r[2].view(3, -1)[k] for r in res]) for k in range(3)])
        assert torch.equal(x2, x1), (world, (x2 - x1).abs().max().item())
        assert torch.equal(z2, z1), (world, (z2 - z1).abs().max().item())
        np.testing.assert_allclose(res[0][3], h1, rtol=1e-3 if dtype == np.float32 else 1e-9)
