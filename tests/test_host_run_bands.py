"""Planning of the band-paired run loop (pcs_pds2d_run, csrc/pds.hip) on the host: nothing is launched and
the fake device addresses are never dereferenced.  Iteration i runs the row bands T = [0, m) and B = [m, rows)
as two launches, T first when i is even and B first when odd; m lies on the 16-row step grid; an iteration
leaves the partials of both launches; the schedule is off unless PCS_RUN_BANDS asks for it (1: any problem that
runs as row bands, auto: the size rule); and the size rule pairs the 4096^2 fp32 problem (448 MiB in seven
arrays, 224 MiB per band) but neither 2048^2 fp32 (224 MiB: resident as a whole) nor 4096^2 fp64 (448 MiB per
band)."""

import ctypes

import pytest

from pycsou_amd import _lib


def _args(n0, n1, dtype, kkind=None):
    a = _lib.PdsArgs()
    a.dtype, a.fkind, a.hkind, a.gkind = dtype, _lib.PCS_F_SEPCONV, _lib.PCS_H_L21, _lib.PCS_G_NULL
    a.kkind = _lib.PCS_K_GRAD_FORWARD if kkind is None else kkind
    a.half = 7
    a.n0 = a.rows = n0
    a.n1 = n1
    a.sigma = a.step0 = a.step1 = 1.0
    for f in ('x', 'xn', 'z', 'zn', 'y', 'partials', 'taps0', 'taps1', 'cty', 'ntaps'):
        setattr(a, f, 0x10000)
    return a


def _plan(lib, a, mode, i):
    out = (ctypes.c_int64 * 6)()
    assert lib.pcs_pds2d_run_plan(ctypes.byref(a), mode, i, out) == 0
    return [int(v) for v in out]


def test_size_rule(monkeypatch):
    monkeypatch.setenv('PCS_RUN_BANDS', 'auto')
    lib = _lib.load()
    on = _args(4096, 4096, _lib.PCS_F32)
    cen = _args(4096, 4096, _lib.PCS_F32, _lib.PCS_K_GRAD_CENTERED)
    for mode in (2, -1):  # the rule itself, and PCS_RUN_BANDS=auto
        assert _plan(lib, on, mode, 0)[0] == 1
        assert _plan(lib, cen, mode, 0)[0] == 1
        for a in (_args(2048, 2048, _lib.PCS_F32), _args(4096, 4096, _lib.PCS_F64)):
            assert lib.pcs_pds2d_supported(ctypes.byref(a)) == 1
            assert _plan(lib, a, mode, 0)[0] == 0
            assert lib.pcs_pds2d_run_nblocks(ctypes.byref(a), mode) == lib.pcs_pds2d_nblocks(ctypes.byref(a))
            assert _plan(lib, a, 1, 0)[0] == 1  # forced: any problem that runs as row bands


def test_environment_switch(monkeypatch):
    lib = _lib.load()
    big, small = _args(4096, 4096, _lib.PCS_F32), _args(160, 128, _lib.PCS_F32)
    monkeypatch.delenv('PCS_RUN_BANDS', raising=False)  # unset: the single launch (the A/B of DESIGN.md)
    assert _plan(lib, big, -1, 0)[0] == 0 and _plan(lib, small, -1, 0)[0] == 0
    monkeypatch.setenv('PCS_RUN_BANDS', '0')
    assert _plan(lib, big, -1, 0)[0] == 0 and _plan(lib, small, -1, 0)[0] == 0
    assert lib.pcs_pds2d_run_nblocks(ctypes.byref(big), -1) == lib.pcs_pds2d_nblocks(ctypes.byref(big))
    monkeypatch.setenv('PCS_RUN_BANDS', '1')
    assert _plan(lib, big, -1, 0)[0] == 1 and _plan(lib, small, -1, 0)[0] == 1
    # slabs with halos, the masked block and CONV2D keep the single launch
    slab = _args(4096, 4096, _lib.PCS_F32)
    slab.row0, slab.rows, slab.halo_x, slab.halo_y, slab.halo_z = 1024, 2048, 15, 8, 1
    assert _plan(lib, slab, -1, 0)[0] == 0


@pytest.mark.parametrize('shape', [(4096, 4096), (160, 128), (208, 192)])
def test_band_order_split_and_counts(shape, monkeypatch):
    monkeypatch.delenv('PCS_RUN_BANDS', raising=False)
    lib = _lib.load()
    n0, n1 = shape
    a = _args(n0, n1, _lib.PCS_F32)
    for i in range(6):
        paired, m, nt, nb, lo, hi = _plan(lib, a, 1, i)
        assert paired == 1
        assert m % 16 == 0 and 0 < m < n0 and abs(m - n0 / 2) <= 8
        assert (lo, hi) == ((0, m) if i % 2 == 0 else (m, n0)), i  # T B | B T | T B ...
        assert nt == lib.pcs_pds2d_nblocks_bands(ctypes.byref(a), 0, m, m, m) > 0
        assert nb == lib.pcs_pds2d_nblocks_bands(ctypes.byref(a), m, n0, n0, n0) > 0
        assert lib.pcs_pds2d_run_nblocks(ctypes.byref(a), 1) == nt + nb
    assert lib.pcs_pds2d_run_nblocks(ctypes.byref(a), 0) == lib.pcs_pds2d_nblocks(ctypes.byref(a))
    if shape == (4096, 4096):
        assert _plan(lib, a, 1, 0)[1] == 2048
    if shape == (208, 192):
        assert _plan(lib, a, 1, 0)[1] == 112
