"""The device loop control every solver engine shares (pycsou_amd/opt/_loop.py) on the GPU: the layout of
the control block (pcs::Ctrl, csrc/pds_ctrl.hpp) behind LoopControl's named fields; that growing the device
history in the middle of a run -- which replaces the buffer a captured chunk points at and rewrites
Ctrl::hist_len -- changes nothing a run computes, in every loop that grows it; and that the host's lagging
view of the stop decision (poll) ends the generic loop on the same iterate whatever the lag.

The loop under test is the reference's `while` of pycsou/core/solver.py:55-76 with the diagnostics of
pycsou/opt/proxalgs.py:366-394 / 604-622, evaluated on the device.  Shapes are the smallest each engine
takes, not the benchmark's."""

import numpy as np
import pytest
import torch

import pycsou_amd.opt._loop as LP
import pycsou_amd.opt.engine as E
import pycsou_amd.opt.proxalgs as PA

pytestmark = pytest.mark.gpu

N_FIXED = 40  # max_iter = min_iter: 41 iterations (solver.py:65-66)
SMALL_CHUNK = 8  # HIST_CHUNK of the patched runs: the history grows 8 -> 16 -> 32 -> 41 rows


def test_ctrl_layout_and_reserve():
    from pycsou_amd import _lib as L
    C = LP.LoopControl
    # sizeof(pcs::Ctrl) is 48 (static_assert in csrc/pds_ctrl.hpp); pcs_ctrl_bytes() is what a caller allocates for
    # it, 64 (csrc/pds.hip): the block LoopControl holds is exactly that and covers every named field
    assert int(L.gpu().pcs_ctrl_bytes()) == 64
    ctl = C(torch.device('cuda'))
    assert ctl.ctrl.numel() * 8 == 64 >= 48 >= 8 * (C.THR + 1)
    total = ctl.start(max_iter=7, min_iter=3, thr=0.5, has_dual=True, up_front=2)
    assert total == 8 and ctl.replaced
    H = ctl.hist.numel()
    assert H == 2 * 2 + 2
    torch.cuda.synchronize()
    f = ctl.ctrl.view(torch.int32).tolist()
    assert [f[i] for i in (C.IT, C.STOPPED, C.MIN_ITER, C.MAX_ITER, C.HAS_DUAL, C.HIST_LEN)] == [0, 0, 3, 7, 1, H]
    assert ctl.ctrl[C.THR].item() == 0.5
    assert ctl.iterations() == 0 and not ctl.stopped() and ctl.rows(0).shape == (0, 2)
    ctl.hist[:4] = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64, device='cuda')
    assert not ctl.reserve(2) and ctl.hist.numel() == H  # fits: the same buffer
    assert ctl.reserve(5)  # past the end: 2 rows -> max(2 * 2, 5) = 5 rows
    assert ctl.hist.numel() == 2 * 5 + 2
    torch.cuda.synchronize()
    f = ctl.ctrl.view(torch.int32).tolist()
    assert f[C.HIST_LEN] == ctl.hist.numel()
    assert [f[i] for i in (C.IT, C.STOPPED, C.MIN_ITER, C.MAX_ITER, C.HAS_DUAL)] == [0, 0, 3, 7, 1]
    assert ctl.ctrl[C.THR].item() == 0.5
    h = ctl.hist.cpu().numpy()
    np.testing.assert_array_equal(h[:4], [1.0, 2.0, 3.0, 4.0])
    assert np.isnan(h[4:]).all()
    np.testing.assert_array_equal(ctl.rows(2), [[1.0, 2.0], [3.0, 4.0]])
    assert ctl.reserve(100) and ctl.hist.numel() == 2 * 8 + 2  # never past the loop's total
    assert not ctl.reserve(100)
    assert ctl.start(7, 3, 0.5, True, up_front=2) == 8 and not ctl.replaced  # large enough: kept


# ---- growth does not change a run: (n, x, z or past_aux, hist (n, 2), hist.numel() at the end) of each loop
def _fused_pds(pds, dtype, small):
    from pycsou_amd import _ops as O
    spec = pds._fused_spec()
    assert spec is not None
    eng = E.engine_class(spec)(spec, dtype, pds.tau, pds.sigma, pds.rho, O.to_dev(pds.x0, dtype),
                               O.to_dev(pds.z0, dtype), **({'chunk': 4} if small else {}))
    n, x, z, h = eng.run(N_FIXED, N_FIXED, 0.0)
    torch.cuda.synchronize()
    return n, x.clone(), z.clone(), np.array(h), eng.hist.numel(), eng


def _pds2d(small, monkeypatch):
    import bench
    out = _fused_pds(bench.build_denoise(128, torch.float32, lipschitz='analytic'), torch.float32, small)
    assert type(out[-1]) is E.PDS2DEngine and not out[-1].native
    return out[:5]


def _pds2d_native(small, monkeypatch):
    import bench
    monkeypatch.setattr(E, 'NATIVE_MIN_PIXELS', 0)
    out = _fused_pds(bench.build_denoise(128, torch.float32, lipschitz='analytic'), torch.float32, small)
    assert type(out[-1]) is E.PDS2DEngine and out[-1].native
    return out[:5]


def _stencil(small, monkeypatch):
    import bench
    out = _fused_pds(bench.build_denoise_k(128, torch.float32, 'lap', lipschitz='analytic'), torch.float32, small)
    assert type(out[-1]) is E.PDS2DStencilEngine
    return out[:5]


def _mask(small, monkeypatch):
    from tests.test_gpu_defer import _cps
    out = _fused_pds(_cps(128, torch.float32), torch.float32, small)
    assert type(out[-1]) is E.PDS2DMaskEngine
    return out[:5]


def _pds3d(small, monkeypatch):
    from pycsou_amd.opt.engine3d import PDS3DEngine
    from tests.cases import pds_case
    from tests.test_gpu_pds import build
    out = _fused_pds(build(pds_case('denoise3d_l1_fwd_16'), np.float32), torch.float32, small)
    assert type(out[-1]) is PDS3DEngine and out[-1].world == 1
    return out[:5]


def _apgd2d(small, monkeypatch):
    from tests.apgd2d_cases import case
    apgd = case((128, 128)).solver('l1', 'CD', np.float32, N_FIXED, N_FIXED, 0.0, engine='fused')
    if small:
        apgd.ENGINE_CHUNK = 4
    it, _, _ = apgd.iterate()
    eng = apgd._engine
    assert type(eng) is E.APGD2DEngine
    return apgd.iter, it['iterand'], it['past_aux'], eng.ctl.rows(apgd.iter), eng.hist.numel()


def _spy_loops(monkeypatch):
    """The _DeviceLoop objects the generic paths build, in order."""
    made = []

    class Spy(PA._DeviceLoop):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(PA, '_DeviceLoop', Spy)
    return made


def _generic_pds(small, monkeypatch):
    from tests.test_gpu_generic_graph import _problem
    monkeypatch.setenv('PCS_GENERIC_GRAPH', '0')
    made = _spy_loops(monkeypatch)
    pds = _problem('l21_labels', 32, torch.float32, N_FIXED, N_FIXED, 0.0)
    it, _, _ = pds.iterate()
    assert not pds._graph_used and len(made) == 1
    return pds.iter, it['primal_variable'], it['dual_variable'], made[0].rows(pds.iter), made[0].hist.numel()


def _generic_apgd(small, monkeypatch):
    from tests.apgd2d_cases import case
    made = _spy_loops(monkeypatch)
    apgd = case((32, 32)).solver('l1', 'CD', np.float32, N_FIXED, N_FIXED, 0.0, engine=False)
    it, _, _ = apgd.iterate()
    assert apgd._engine is None and len(made) == 1
    return apgd.iter, it['iterand'], it['past_aux'], made[0].rows(apgd.iter), made[0].hist.numel()


LOOPS = {'pds2d_graph': _pds2d, 'pds2d_native': _pds2d_native, 'stencil': _stencil, 'mask': _mask, 'apgd2d': _apgd2d,
         'pds3d': _pds3d, 'generic_pds': _generic_pds, 'generic_apgd': _generic_apgd}


@pytest.mark.parametrize('name', list(LOOPS))
def test_history_growth_does_not_change_a_run(name, monkeypatch):
    n0, x0, z0, h0, _ = LOOPS[name](False, monkeypatch)
    monkeypatch.setattr(LP, 'HIST_CHUNK', SMALL_CHUNK)
    n1, x1, z1, h1, numel = LOOPS[name](True, monkeypatch)
    assert n0 == n1 == N_FIXED + 1
    assert torch.equal(torch.as_tensor(x0), torch.as_tensor(x1))
    assert torch.equal(torch.as_tensor(z0), torch.as_tensor(z1))
    print(name, 'hist numel', numel, 'rows', h1.shape, 'nan', int(np.isnan(h1).sum()))
    assert h0.shape == h1.shape == (n0, 2)
    assert np.array_equal(h0, h1)
    assert not np.isnan(h1).any()
    assert 2 * SMALL_CHUNK + 2 < numel <= 2 * (N_FIXED + 1) + 2  # it started at SMALL_CHUNK rows and grew


# ---- poll: the host's view of the stop lags, the result does not depend on the lag
def test_poll_lag_does_not_change_the_stop(monkeypatch):
    from tests.test_gpu_generic_graph import _problem
    monkeypatch.setenv('PCS_GENERIC_GRAPH', '0')
    pds = _problem('l21_labels', 32, torch.float64, N_FIXED, N_FIXED, 0.0)
    pds.iterate()
    rp = pds.diagnostics['Relative Improvement (primal variable)'].to_numpy(float)
    thr = float(rp[20]) * (1 + 1e-9)  # just above the primal improvement of iteration 20
    n_ref = int(np.argmax((rp <= thr) & (np.arange(rp.size) >= 3))) + 1  # the first iteration past min_iter there
    assert 4 <= n_ref <= 21
    out = {}
    for lag in (0, 3):
        monkeypatch.setattr(PA.PDS, 'LOOP_LAG', lag)
        made = _spy_loops(monkeypatch)
        p = _problem('l21_labels', 32, torch.float64, 500, 3, thr)
        it, _, diag = p.iterate()
        assert made[0].lag == lag
        out[lag] = (p.iter, it['primal_variable'], it['dual_variable'], diag.to_numpy(float))
    assert out[0][0] == out[3][0] == n_ref
    assert torch.equal(out[0][1], out[3][1]) and torch.equal(out[0][2], out[3][2])
    assert np.array_equal(out[0][3], out[3][3])
