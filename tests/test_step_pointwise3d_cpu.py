"""What the element-wise one-step GPU tests of the 3-D kernels (tests/test_gpu_step_pointwise3d.py) rely on,
proved without a GPU: the derived bound holds for a plain fp32 evaluation of the same step, the inputs of
every case of the matrix make prox_G and the dual projection bind on both sides, and the comparator fails on
each of the kernel mistakes the norm-based 3-D tests cannot see -- while their criterion passes the localised
ones."""

import numpy as np
import pytest

from tests import pointwise3d as PW
from tests.cases import rel

VB = PW.VB


def _problem(kind='forward', fk='sep7x15x4', hname='l21', gname='segment', edge=True, steps=PW.NU, seed=3):
    return PW.make_problem(VB, kind, hname, fk, gname, edge=edge, steps=steps, lam=PW.LAM, seed=seed,
                           dtype=np.float32)


@pytest.fixture(scope='module')
def base():
    """The (17, 9, 132) forward case with a 7 x 15 x 4 blur, steps (2, 0.5, 1), lam L21 and G = Segment, and
    its fp64 one-step reference."""
    p = _problem()
    x, z, d, _ = PW.oracle_steps(p, 1)
    return p, x, z, d


@pytest.mark.parametrize('name,kw', [('blur', {}), ('denoise', dict(kind='backward', fk='denoise', hname='l1')),
                                     ('noedge', dict(kind='centered', fk='sep4x7x15', gname='', edge=False))])
@pytest.mark.parametrize('nit', [1, 2])
def test_fp32_restatement_within_bound(nit, name, kw):
    """The oracle itself in np.float32 (NumPy's operation order, no FMA) against the fp64 oracle: inside
    nit c eps M with c = 2 (l0 + l1 + l2) + 16 (68 for both blurs here) or 16, and above 0."""
    p = _problem(**kw)
    xr, zr, dr, _ = PW.oracle_steps(p, nit)
    x, z, d, _ = PW.oracle_steps(p, nit, dtype=np.float32)
    assert x.dtype == np.float32 and z.dtype == np.float32
    b = PW.bound(p, nit)
    assert b['x'].c == (16 if name == 'denoise' else 68) and b['z'].c == b['x'].c
    rx = PW.compare(x, xr, b['x'], VB, 'x', diag=d, diag_ref=dr, dtype=np.float32)
    rz = PW.compare(z, zr, b['z'], VB, 'z')
    print(f'fp32 restatement {name} nit={nit}: x {rx:.2f} z {rz:.2f} eps*M (c = {b["x"].c})')
    assert 0 < rx and 0 < rz  # fp32 arithmetic did run


@pytest.mark.parametrize('ik', PW.MATRIX, ids=PW.case_id)
def test_input_conditions(ik):
    """Every case of the GPU matrix, at iteration 1 on the oracle's side: prox_G clips at least 10 % of the
    voxels at each bound it has, the Fenchel prox projects between 10 % and 90 % of the dual entries, and
    both diagnostics of row 0 are finite and positive."""
    c, p = PW.case_problem(ik)
    _, _, d, s = PW.oracle_steps(p, 1)
    if p['gname'] in ('nonneg', 'segment'):
        assert s['low'] >= 0.10, s
    if p['gname'] == 'segment':
        assert s['high'] >= 0.10, s
    assert 0.10 <= s['dual'] <= 0.90, s
    assert np.isfinite(d['primal'][0]) and np.isfinite(d['dual'][0]) and d['primal'][0] > 0 and d['dual'][0] > 0


def test_matrix_layout():
    """23 configurations, two H each; every route of ROUTES occurs; every shape has at least two plane
    segments' worth of planes (plan3: segments of >= 8 planes, at most ceil(n0 / 8) of them)."""
    assert len(PW.CONFIGS) == 23 and len(PW.MATRIX) == 46
    assert {c.route for c in PW.CONFIGS} == set(PW.ROUTES)
    assert len({PW.case_id(ik) for ik in PW.MATRIX}) == 46
    assert all(-(-c.shape[0] // 8) >= 2 for c in PW.CONFIGS)
    # VG32 / VG64 hold a k_pds3d_gen tile of each of the four code forms (pds3d.hip: row_int, col_int)
    for shape, dtype in ((PW.VG32, np.float32), (PW.VG64, np.float64)):
        t1, tw = PW.update_tile('centered', dtype)
        forms = {(r1 - 1 >= 2 and r1 + t1 <= shape[1] - 3, c2 - 4 >= 2 and c2 + tw + 3 <= shape[2] - 3)
                 for r1 in range(0, shape[1], t1) for c2 in range(0, shape[2], tw)}
        assert len(forms) == 4, (shape, forms)
        assert any(c.shape == shape and c.kind != 'forward' and c.dtype == ('f32' if dtype == np.float32 else 'f64')
                   for c in PW.CONFIGS)
    for g in ('', 'nonneg', 'segment'):  # every G kind meets both H
        assert {c.hs[k] for c in PW.CONFIGS for k in range(2) if c.g[k] == g} == {'l1', 'l21'}


def _fails(got, ref, bound, name='x'):
    with pytest.raises(AssertionError, match='eps\\*M'):
        PW.compare(got, ref, bound, VB, name)


def _mistake(base, name='x', **changes):
    """The comparator fails on `name` of the one-step oracle run of the base problem with `changes`."""
    p, x, z, _ = base
    q = dict(p)
    q.update(changes)
    xq, zq, _, _ = PW.oracle_steps(q, 1)
    _fails({'x': x, 'z': z}[name], {'x': xq, 'z': zq}[name], PW.bound(p)[name], name)


def test_detects_swapped_steps(base):
    s0, s1, s2 = base[0]['steps']
    assert s1 != s2
    _mistake(base, steps=(s0, s2, s1))  # tau and sigma depend on the steps symmetrically: only K changes
    _mistake(base, 'z', steps=(s0, s2, s1))


def test_detects_swapped_inplane_taps(base):
    p = base[0]
    _mistake(base, t1=p['t2'], t2=p['t1'])


def test_detects_dropped_outer_tap(base):
    t0 = base[0]['t0'].copy()
    t0[0] = 0.0
    _mistake(base, t0=t0)


def test_detects_reversed_taps(base):
    _mistake(base, t2=base[0]['t2'][::-1].copy())


@pytest.mark.parametrize('which', [0, 1])
def test_detects_moved_segment_bound(base, which):
    seg = list(PW.SEG)
    seg[which] += 1e-3
    _mistake(base, seg=tuple(seg))


def test_detects_flipped_edge():
    p = _problem(kind='centered')
    x, z, d, _ = PW.oracle_steps(p, 1)
    _mistake((p, x, z, d), edge=False)
    _mistake((p, x, z, d), 'z', edge=False)


def test_detects_l21_over_two_components(base):
    p, x, z, _ = base
    xq, zq, _, _ = PW.oracle_steps(p, 1, l21_comps=2)
    _fails(z, zq, PW.bound(p)['z'], 'z')


def _stale_plane(p, plane=6, comp=0):
    """z0 of one component zeroed on one plane: a ring slot that was never loaded."""
    z0 = p['z0'].copy()
    z0.reshape(3, *p['shape'])[comp, plane] = 0.0
    return z0


def test_detects_stale_z_plane(base):
    p, x, z, _ = base
    q = dict(p, z0=_stale_plane(p))
    xq, zq, _, _ = PW.oracle_steps(q, 1)
    with pytest.raises(AssertionError, match='plane [567], row'):  # K^T z of a forward K reaches one plane back
        PW.compare(x, xq, PW.bound(p)['x'], VB, 'x')
    _fails(z, zq, PW.bound(p)['z'], 'z')


def _single_voxel(p, x):
    """x with one voxel inside the segment (where prox_G passes the error on) off by 20 c eps Mx."""
    b = PW.bound(p)['x']
    n0, n1, n2 = VB
    v = x.reshape(VB)
    r = int(np.flatnonzero((v[6, :, 128] > PW.SEG[0]) & (v[6, :, 128] < PW.SEG[1]))[0])
    xq = x.copy()
    xq[(6 * n1 + r) * n2 + 128] += 20 * b.c * b.unit
    return xq, r


def test_detects_single_voxel_at_a_tile_seam(base):
    p, x, z, _ = base
    xq, r = _single_voxel(p, x)
    with pytest.raises(AssertionError, match=f'plane 6, row {r}, col 128.*component 0.*eps\\*M'):
        PW.compare(xq, x, PW.bound(p)['x'], VB, 'x')
    zq = z.copy()
    b = PW.bound(p)['z']
    zq[2 * p['N'] + (16 * VB[1] + 8) * VB[2] + 131] -= 20 * b.c * b.unit
    with pytest.raises(AssertionError, match='plane 16, row 8, col 131.*component 2'):
        PW.compare(zq, z, b, VB, 'z')


def test_norm_criterion_passes_localised_mistakes(base):
    """The gap this closes.  rel(...) < 5e-5, the criterion of every other 3-D test, passes (a) the single
    voxel off by 20 times the element-wise bar, and (b) the never-loaded z plane on the state those tests
    start from: with z0 = 0 the slot holds what it should have loaded, the first iteration is exact, and
    nothing of the mistake is left to see -- while on this module's state the same two mistakes fail the
    comparator (test_detects_single_voxel_at_a_tile_seam, test_detects_stale_z_plane).  What the zero start
    hides is the slot's first use: a plane of z that K^T never saw in any of 8-20 iterations moves the norm
    by 2e-2 to 1e-1 (measured on a 20 x 24 x 36 Gaussian-blur problem of those tests' kind) and is seen."""
    p, x, z, _ = base
    xq, _ = _single_voxel(p, x)
    assert np.max(np.abs(xq - x)) > PW.bound(p)['x'].tol
    assert rel(xq, x) < 5e-5
    zero = dict(p, x0=np.zeros(p['N']), z0=np.zeros(3 * p['N']))
    x0, z0, _, _ = PW.oracle_steps(zero, 1)
    xs, zs, _, _ = PW.oracle_steps(dict(zero, z0=_stale_plane(zero)), 1)
    assert rel(xs, x0) < 5e-5 and rel(zs, z0) < 5e-5
