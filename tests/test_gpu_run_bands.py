"""The band-paired run loop (pcs_pds2d_run with PCS_RUN_BANDS=1: every iteration as two row-band launches,
T B | B T | T B ..., csrc/pds.hip) against the single launch per iteration (PCS_RUN_BANDS=0) on the fp32
normal-operator marches with a 15 x 15 separable PSF (tier 7): forward and centred K, L21 and L1.

Shapes: 160 x 128, the smallest the march takes with two strips and a non-empty band on each side of the
split row m = 80; 208 x 192, where m = 112 is off the segment grid, there are three strips, and the edge
bands of the vertical normal operator lie within 7 rows of both image edges and next to the band boundary.
Counts: 5 and 6 iterations (both launch orders; the run ends on either parity), 33 (crosses the engine's
32-iteration chunk), and a natural stop at a threshold the single-launch run reaches in under 40 iterations.

Asserted: x and z bitwise equal, the same iteration count, and every diagnostics row equal to P * 2^-52
relative, P the number of per-workgroup partials of the paired run -- the two schedules add the same fp32-derived
fp64 partials in a different order, each sum within (P - 1) * 2^-53 relative of the exact one (all terms are
non-negative), which the square root halves and the quotient of two sums doubles.  The paired loop run twice is
bitwise identical, diagnostics included."""

import ctypes

import numpy as np
import pytest
import torch

import pycsou_amd.opt.engine as E
from pycsou_amd import _lib as L

pytestmark = pytest.mark.gpu


def _build(n0, n1, kind, hname):
    import bench
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm, L21Norm
    from pycsou_amd.linop.conv import Convolve2D
    from pycsou_amd.linop.diff import Gradient
    from pycsou_amd.opt.proxalgs import PDS
    dtype, N = torch.float32, n0 * n1
    xs = torch.as_tensor(bench.phantom((n0, n1), 16, 3).ravel()).to('cuda', dtype)
    C = Convolve2D(size=N, filter=bench.gaussian_psf(15, 2.0), shape=(n0, n1))
    K = Gradient(shape=(n0, n1), kind=kind)
    C.lipschitz_cst = C.diff_lipschitz_cst = 1.0  # nonnegative PSF of unit sum
    K.lipschitz_cst = K.diff_lipschitz_cst = float(np.sqrt(8.0))  # a bound for every Gradient kind
    g = torch.Generator(device='cuda').manual_seed(4)
    y = C(xs) + 0.01 * torch.randn(N, generator=g, device='cuda', dtype=dtype)
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y) * C
    H = 0.05 * (L21Norm(dim=2 * N, groups=np.tile(np.arange(N), 2)) if hname == 'l21' else L1Norm(dim=2 * N))
    return PDS(dim=N, F=F, H=H, K=K, x0=torch.zeros(N, dtype=dtype, device='cuda'),
               z0=torch.zeros(2 * N, dtype=dtype, device='cuda'), verbose=None)


def _run(pds, bands, max_iter, min_iter, thr, monkeypatch):
    from pycsou_amd import _ops as O
    monkeypatch.setenv('PCS_RUN_BANDS', '1' if bands else '0')
    monkeypatch.setattr(E, 'NATIVE_MIN_PIXELS', 1)  # chunks launched from C (pcs_pds2d_run) at any size
    monkeypatch.setattr(E, 'DEFER_FIN', True)
    spec = pds._fused_spec()
    assert spec is not None
    dtype = torch.float32
    eng = E.engine_class(spec)(spec, dtype, pds.tau, pds.sigma, pds.rho, O.to_dev(pds.x0, dtype),
                               O.to_dev(pds.z0, dtype))
    assert eng.native and eng.defer
    assert eng.lib.pcs_pds2d_path(ctypes.byref(eng.args)) == L.PCS_PATH_NMARCH
    out = (ctypes.c_int64 * 6)()
    assert eng.lib.pcs_pds2d_run_plan(ctypes.byref(eng.args), -1, 0, out) == 0
    assert int(out[0]) == int(bands), 'the schedule under test did not engage'
    if bands:
        assert eng.run_nblocks == int(out[2]) + int(out[3]) and int(out[2]) > 0 and int(out[3]) > 0
    else:
        assert eng.run_nblocks == eng.nblocks
    n, x, z, h = eng.run(max_iter, min_iter, thr)
    torch.cuda.synchronize()
    return n, x.clone(), z.clone(), np.array(h, copy=True), eng.run_nblocks


def _same(a, b, tag):
    (na, xa, za, ha, pa), (nb, xb, zb, hb, _) = a, b
    assert na == nb, (tag, na, nb)
    assert torch.equal(xa, xb) and torch.equal(za, zb), tag
    assert ha.shape == hb.shape == (na, 2) and not np.isnan(ha).any() and not np.isnan(hb).any(), tag
    fin = np.isfinite(hb)  # iteration 0 starts from zero iterates: its relative improvements are inf
    assert np.array_equal(ha[~fin], hb[~fin]) and fin[1:].all(), tag
    err = np.max(np.abs(ha[fin] - hb[fin]) / np.abs(hb[fin]))
    print(f'{tag}: n={na} partials={pa} max rel diagnostics difference {err:.3e} (bound {pa * 2.0 ** -52:.3e})')
    assert err <= pa * 2.0 ** -52, (tag, err)


@pytest.mark.parametrize('hname', ['l21', 'l1'])
@pytest.mark.parametrize('kind', ['forward', 'centered'])
@pytest.mark.parametrize('shape', [(160, 128), (208, 192)])
def test_paired_run_matches_single_launch(shape, kind, hname, monkeypatch):
    pds = _build(shape[0], shape[1], kind, hname)
    single33 = None
    for count in (5, 6, 33):
        one = _run(pds, False, count - 1, count - 1, 0.0, monkeypatch)
        two = _run(pds, True, count - 1, count - 1, 0.0, monkeypatch)
        assert one[0] == count
        _same(two, one, f'{shape} {kind} {hname} count {count}')
        if count == 33:
            single33 = one
    # natural stop: the threshold just above the single-launch run's primal improvement of iteration 20
    rp = single33[3][:, 0]
    thr = float(rp[20]) * (1 + 1e-9)
    k_ref = int(np.argmax(rp <= thr))
    one = _run(pds, False, 500, 0, thr, monkeypatch)
    two = _run(pds, True, 500, 0, thr, monkeypatch)
    assert one[0] == k_ref + 1 < 40, (one[0], k_ref)
    _same(two, one, f'{shape} {kind} {hname} natural stop')


@pytest.mark.parametrize('kind', ['forward', 'centered'])
def test_paired_run_is_reproducible(kind, monkeypatch):
    pds = _build(208, 192, kind, 'l21')
    a = _run(pds, True, 32, 32, 0.0, monkeypatch)
    b = _run(pds, True, 32, 32, 0.0, monkeypatch)
    assert a[0] == b[0] == 33
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert np.array_equal(a[3], b[3])
