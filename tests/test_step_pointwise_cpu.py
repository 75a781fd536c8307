"""What the element-wise one-step GPU tests (tests/test_gpu_step_pointwise.py) rely on, proved without a GPU:
the derived bound holds for a plain fp32 evaluation of the same step, the inputs of every case of the matrix
make prox_G and the dual projection bind on both sides, and the comparator fails on each of the kernel
mistakes the norm-based tests cannot see -- while their criterion passes one of them."""

import numpy as np
import pytest

from tests import pointwise as PW
from tests.cases import rel

A = PW.A


def _sep_case(gname, hname='l21', seed=3):
    return PW.make_problem(A, 'forward', hname, 'sep15', gname, lam=PW.LAM, seed=seed, dtype=np.float32)


@pytest.fixture(scope='module')
def base():
    """The (150, 200) separable forward case with G = Segment and its fp64 one-step reference."""
    p = _sep_case('segment')
    x, z, d, _ = PW.oracle_steps(p, 1)
    return p, x, z, d


@pytest.mark.parametrize('gname', ['', 'segment'])
@pytest.mark.parametrize('nit', [1, 2])
def test_fp32_restatement_within_bound(nit, gname):
    """The oracle itself in np.float32 (NumPy's operation order, no FMA) against the fp64 oracle: inside
    c eps M with c = 76.  Measured worst element, in units of eps M: x 0.56 (nit 1) / 0.64 (nit 2) with G none,
    0.23 / 0.23 with the segment (it clips the largest values); z 0.09 / 0.08 and 0.08 / 0.07 (Mz is the more
    conservative of the two magnitudes).  That is about c / 100: roundings add like a random walk, and the
    partial sums of 15 positive taps of about 1 / 15 each stay far below M."""
    p = _sep_case(gname)
    xr, zr, dr, _ = PW.oracle_steps(p, nit)
    x, z, d, _ = PW.oracle_steps(p, nit, dtype=np.float32)
    assert x.dtype == np.float32 and z.dtype == np.float32
    b = PW.bound(p, nit)
    assert b['x'].c == 76
    rx = PW.compare(x, xr, b['x'], A, 'x', diag=d, diag_ref=dr, dtype=np.float32)
    rz = PW.compare(z, zr, b['z'], A, 'z')
    print(f'fp32 restatement nit={nit} G={gname or "none"}: x {rx:.2f} z {rz:.2f} eps*M (c = {b["x"].c})')
    assert 0 < rx and 0 < rz  # fp32 arithmetic did run


@pytest.mark.parametrize('ik', PW.MATRIX, ids=PW.case_id)
def test_input_conditions(ik):
    """Every case of the GPU matrix, at iteration 1 on the oracle's side: prox_G clips at least 10 % of the
    pixels at each bound it has, and the Fenchel prox projects between 10 % and 90 % of the dual entries."""
    c, p = PW.case_problem(ik)
    _, _, d, s = PW.oracle_steps(p, 1)
    if p['gname'] in ('nonneg', 'segment'):
        assert s['low'] >= 0.10, s
    if p['gname'] == 'segment':
        assert s['high'] >= 0.10, s
    assert 0.10 <= s['dual'] <= 0.90, s
    assert np.isfinite(d['primal'][0]) and np.isfinite(d['dual'][0]) and d['primal'][0] > 0 and d['dual'][0] > 0


def _fails(got, ref, bound, name='x'):
    with pytest.raises(AssertionError, match='eps\\*M'):
        PW.compare(got, ref, bound, A, name)


def test_detects_dropped_outer_tap(base):
    p, x, z, _ = base
    q = dict(p)
    t0 = p['t0'].copy()
    t0[0] = 0.0
    q['psf'] = np.outer(t0, p['t1'])
    xq, zq, _, _ = PW.oracle_steps(q, 1)
    _fails(x, xq, PW.bound(p)['x'])


def test_detects_reversed_taps(base):
    p, x, z, _ = base
    q = dict(p)
    q['psf'] = np.outer(p['t0'], p['t1'][::-1])
    xq, zq, _, _ = PW.oracle_steps(q, 1)
    _fails(x, xq, PW.bound(p)['x'])


def _dense_grad(p, t0, t1, interior_row=None):
    """grad F(v) = N v - Conv^T y from the dense 1-D matrices (tests/test_host.py builds C^T C so):
    Conv X = C0 X C1^T, N X = (C0^T C0) X (C1^T C1).  `interior_row`: that row of the vertical N takes the
    interior window (no edge-table correction), the mistake of a kernel that mis-indexes its E table."""
    n0, n1 = p['shape']
    C0, C1 = PW.dense_conv1d(n0, t0), PW.dense_conv1d(n1, t1)
    N0, N1 = C0.T @ C0, C1.T @ C1
    if interior_row is not None:
        pad = 2 * len(t0)
        Cb = PW.dense_conv1d(n0 + 2 * pad, t0)
        N0 = N0.copy()
        N0[interior_row] = (Cb.T @ Cb)[interior_row + pad, pad:pad + n0]
    cty = C0.T @ p['y'].reshape(n0, n1) @ C1
    return lambda v: (N0 @ v.reshape(n0, n1) @ N1 - cty).ravel()


@pytest.mark.parametrize('row', [0, 3, 6])
def test_detects_interior_window_on_an_edge_row(base, row):
    p, x, z, _ = base
    xd, zd, _, _ = PW.oracle_steps(p, 1, grad=_dense_grad(p, p['t0'], p['t1']))
    assert np.max(np.abs(xd - x)) < 1e-13  # the dense form is the oracle's operator
    xq, zq, _, _ = PW.oracle_steps(p, 1, grad=_dense_grad(p, p['t0'], p['t1'], interior_row=row))
    _fails(x, xq, PW.bound(p)['x'])


def test_detects_single_pixel_at_a_strip_seam(base):
    p, x, z, _ = base
    n1 = A[1]
    b = PW.bound(p)
    xq = x.copy()
    i = int(np.flatnonzero((x.reshape(A)[:, 64] > PW.SEG[0]) & (x.reshape(A)[:, 64] < PW.SEG[1]))[0])
    xq[i * n1 + 64] += 1e-4
    assert rel(xq, x) < 5e-5  # a whole-image norm does not see it
    with pytest.raises(AssertionError, match=f'row {i}, col 64.*col % 64 = 0'):
        PW.compare(xq, x, b['x'], A, 'x')
    zq = z.copy()
    zq[A[0] * n1 + 5 * n1 + 64] += 4e-4
    with pytest.raises(AssertionError, match='row 5, col 64.*component 1'):
        PW.compare(zq, z, b['z'], A, 'z')


def test_detects_ignored_upper_bound(base):
    p, x, z, _ = base
    q = dict(p)
    q['seg'] = (PW.SEG[0], np.inf)
    xq, zq, _, _ = PW.oracle_steps(q, 1)
    _fails(x, xq, PW.bound(p)['x'])


def test_legacy_criterion_is_blind_to_an_edge_row():
    """The gap this closes: the Gaussian taps of tests/test_gpu_march.py (sigma 1.7 / 2.3, 15 taps), a start
    from zero, 12 iterations and rel < 5e-5 -- row 6 of the vertical normal operator computed with the
    interior window passes."""
    from oracle import pycsou_ref as OR
    n0, n1 = A
    rng = np.random.default_rng(0)
    r = np.arange(15) - 7
    t0, t1 = np.exp(-0.5 * (r / 1.7) ** 2), np.exp(-0.5 * (r / 2.3) ** 2)
    t0, t1 = t0 / t0.sum(), t1 / t1.sum()
    p = PW.make_problem(A, 'forward', 'l21', 'sep15', '', lam=0.05, seed=0, dtype=np.float32)
    p.update(psf=np.outer(t0, t1), t0=t0, t1=t1, x0=np.zeros(n0 * n1), z0=np.zeros(2 * n0 * n1),
             y=OR.phantom(A, seed=0).ravel() + 0.05 * rng.standard_normal(n0 * n1))
    x, z, d, _ = PW.oracle_steps(p, 12, grad=_dense_grad(p, t0, t1))
    xq, zq, dq, _ = PW.oracle_steps(p, 12, grad=_dense_grad(p, t0, t1, interior_row=6))
    assert np.max(np.abs(xq - x)) > 0
    assert rel(xq, x) < 5e-5 and rel(zq, z) < 5e-5, (rel(xq, x), rel(zq, z))
    np.testing.assert_allclose(dq['primal'][1:], d['primal'][1:], rtol=1e-3)
    # ... and with the equal-weight taps of this module one step shows it (test_detects_interior_window_...)
