"""One and two launches of the fused APGD kernel (pcs_apgd2d_step / pcs_apgd2d_run, the NrmApgd policy of
csrc/sep_nrm.hpp) from a generic state, compared element by element with the fp64 oracle
(tests/pointwise_apgd.py: inputs, oracle, derived rounding bound nit c eps M, matrix;
tests/test_apgd_pointwise_cpu.py proves what they rely on).

Unlike the 6-iteration relative-L2 tests of this kernel (tests/test_gpu_apgd2d.py), x, aux and y are
independent non-zero draws, the momentum coefficient is given (0.61, then -0.35) so a (w - aux) acts at full
weight from the first launch, the PSF taps are about 1 / len each and not symmetric, every prox binds on a
third to a half of the pixels, every element of x' and aux' is checked, and the first history row is a number.
The shapes are the kernel's geometry: fewer rows than the ring prologue, ragged and exact strips and steps,
one, two and three row segments.  Every case asserts that the fused engine took it, with the half width and
the task count (strips x row segments) it is about.  The public API from a non-zero x0 is held to the same
element-wise bar on both of its paths, the fused engine and engine=False (k_apgd_step and the correlation
kernels).  Each case prints its worst error in units of eps M (DESIGN.md 2.3 records them)."""

import ctypes
import functools

import numpy as np
import pytest

from tests import pointwise_apgd as PA

pytestmark = pytest.mark.gpu


def _engine(i, nit=1):
    """(case, problem, solver, engine) of case i: the solver built and run through the public API, its engine
    checked for route and geometry."""
    import torch
    from pycsou_amd import _lib as L
    from pycsou_amd.opt.engine import APGD2DEngine
    c, p = PA.case_problem(i)
    s = PA.build_solver(p, nit)
    s.iterate()
    eng = s._engine
    assert type(eng) is APGD2DEngine, 'the fused engine must take this problem'
    assert eng.args.half == p['half'] and eng.args.dtype == (L.PCS_F32 if c.dtype == 'f32' else L.PCS_F64)
    assert (eng.args.n0, eng.args.n1) == c.shape and eng.args.tau == c.tau
    nstrips, nseg = PA.geometry(c)
    assert int(eng.lib.pcs_apgd2d_nblocks(ctypes.byref(eng.args))) == nstrips * nseg == eng.nblocks
    assert eng.dtype == (torch.float32 if c.dtype == 'f32' else torch.float64)
    return c, p, s, eng


def _load_state(p, eng, max_iter):
    """A fresh loop of the engine with X[0] = x, AUX[0] = aux and NaN in the other parity."""
    import torch
    eng.start(max_iter, max_iter, 0.0)
    dev = eng.X[0].device
    x = torch.as_tensor(p['x'].astype(p['dtype']), device=dev)
    aux = torch.as_tensor(p['aux'].astype(p['dtype']), device=dev)
    eng.X[0].copy_(x)
    eng.AUX[0].copy_(aux)
    eng.X[1].fill_(float('nan'))
    eng.AUX[1].fill_(float('nan'))
    return x, aux


def _bits(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('i', PA.MATRIX, ids=PA.case_id)
def test_one_launch_from_a_generic_state(i):
    """pcs_apgd2d_step once with a = 0.61 on (x, aux): X[1], AUX[1] and history row 0 against the oracle, the
    inputs untouched, Ctrl.it == 1."""
    import torch
    from pycsou_amd import _lib as L
    c, p, s, eng = _engine(i)
    x, aux = _load_state(p, eng, 10)
    eng.args.hist = eng.hist.data_ptr()
    L.check(eng.lib.pcs_apgd2d_step(ctypes.byref(eng.args), PA.A0, L.stream()), 'pcs_apgd2d_step')
    torch.cuda.synchronize()
    u = PA.case_oracle(i)[0]
    b = PA.bound(p, [(p['x'], p['aux'], PA.A0)])
    rx = PA.compare(eng.X[1].cpu().numpy(), u.x, b['x'], c.shape, 'x', hist=eng.ctl.rows(1)[:, 0], hist_ref=[u.metric],
                    dtype=p['dtype'])
    ra = PA.compare(eng.AUX[1].cpu().numpy(), u.aux, b['aux'], c.shape, 'aux')
    assert _same_bits(eng.X[0], x) and _same_bits(eng.AUX[0], aux)
    assert eng.ctl.iterations() == 1 and not eng.ctl.stopped()
    print(f'POINTWISE apgd-step-{PA.case_id(i)} nit=1 c={b["x"].c} x={rx:.2f} aux={ra:.2f}')


@pytest.mark.parametrize('i', PA.MATRIX, ids=PA.case_id)
def test_two_launches_through_the_run_loop(i):
    """pcs_apgd2d_run with a = (0.61, -0.35): the second launch reads parity 1 -- its aux is the first one's w --
    and writes parity 0; both history rows."""
    import torch
    c, p, s, eng = _engine(i)
    _load_state(p, eng, 10)
    co = [PA.A0, PA.A1]
    eng.launch(co)
    torch.cuda.synchronize()
    ups = PA.case_oracle(i)
    states = PA.run_states(p, co, ups)
    b1, b2 = PA.bound(p, states[:1]), PA.bound(p, states)
    # parity 1 still holds the first launch's outputs
    PA.compare(eng.X[1].cpu().numpy(), ups[0].x, b1['x'], c.shape, 'x after launch 1')
    PA.compare(eng.AUX[1].cpu().numpy(), ups[0].aux, b1['aux'], c.shape, 'aux after launch 1')
    rx = PA.compare(eng.X[0].cpu().numpy(), ups[1].x, b2['x'], c.shape, 'x', hist=eng.ctl.rows(2)[:, 0],
                    hist_ref=[u.metric for u in ups], dtype=p['dtype'])
    ra = PA.compare(eng.AUX[0].cpu().numpy(), ups[1].aux, b2['aux'], c.shape, 'aux')
    assert eng.ctl.iterations() == 2 and not eng.ctl.stopped()
    print(f'POINTWISE apgd-run-{PA.case_id(i)} nit=2 c={b2["x"].c} x={rx:.2f} aux={ra:.2f}')


@pytest.mark.parametrize('i', PA.MATRIX, ids=PA.case_id)
def test_a_launch_after_the_stop_stores_nothing(i):
    """max_iter = min_iter = 1: the second launch sets the stop flag; two more launches leave all four buffers,
    the history and Ctrl.it as they are, bit for bit."""
    import torch
    c, p, s, eng = _engine(i)
    _load_state(p, eng, 1)
    eng.launch([PA.A0, PA.A1])
    torch.cuda.synchronize()
    assert eng.ctl.iterations() == 2 and eng.ctl.stopped()
    bufs = eng.X + eng.AUX + [eng.hist]
    snap = [t.clone() for t in bufs]
    assert all(bool(torch.isfinite(t).all()) for t in bufs[:4])
    eng.launch([0.3, -0.2])
    torch.cuda.synchronize()
    for k, (t, t0) in enumerate(zip(bufs, snap)):
        assert _same_bits(t, t0), f'buffer {k} changed after the stop'
    assert eng.ctl.iterations() == 2 and eng.ctl.stopped()


@functools.lru_cache(maxsize=None)
def _api_oracle(i, acc):
    """OR.apgd from x0 = x for 1, 2 and 3 iterations ('CD' with d = 2: a = 0, 0, 1/3), computed once."""
    _, p = PA.case_problem(i)
    return [PA.oracle_api(p, acc, 2.0, nit) for nit in (1, 2, 3)]


@pytest.mark.parametrize('acc', ['BT', 'CD', None])
@pytest.mark.parametrize('i', PA.MATRIX, ids=PA.case_id)
def test_public_api_from_a_nonzero_start(i, acc):
    """APGD.iterate() for nit = 1, 2, 3 from x0 = x on the fused engine and with engine=False: iterand and
    past_aux element-wise, past_t exactly, every diagnostics row."""
    from pycsou_amd.opt.engine import APGD2DEngine
    c, p = PA.case_problem(i)
    refs = _api_oracle(i, acc)
    coeffs, _ = PA.ref_coeffs(acc, 2.0, 3)
    # the state each iteration starts from: (x0, 0), then the oracle's after 1 and 2 iterations
    states = [(p['x'], np.zeros(p['N']), coeffs[0])] + [(refs[k][0], refs[k][1], coeffs[k + 1]) for k in (0, 1)]
    worst = {}
    for engine in (None, False):
        for nit in (1, 2, 3):
            xr, auxr, tr, hr = refs[nit - 1]
            s = PA.build_solver(p, nit, acc=acc, d=2.0, engine=engine)
            est, conv, diag = s.iterate()
            if engine is None:
                assert type(s._engine) is APGD2DEngine and s._engine.args.half == p['half']
                assert s._engine.nblocks == int(np.prod(PA.geometry(c)))
            else:
                assert s._engine is None
            assert conv is True and s.iter == nit
            assert est['iterand'].dtype == p['dtype'] and est['past_aux'].dtype == p['dtype']
            assert est['past_t'] == tr, (est['past_t'], tr)
            np.testing.assert_array_equal(diag['Iter'].to_numpy(), np.arange(nit))
            b = PA.bound(p, states[:nit])
            rx = PA.compare(est['iterand'], xr, b['x'], c.shape, 'x', hist=diag[PA.H_COL].to_numpy(float), hist_ref=hr,
                            dtype=p['dtype'])
            ra = PA.compare(est['past_aux'], auxr, b['aux'], c.shape, 'aux')
            worst[engine, nit] = (rx, ra)
    for engine, name in ((None, 'fused'), (False, 'eager')):
        print(f'POINTWISE apgd-api-{name}-{acc}-{PA.case_id(i)} nit=1/2/3 c={PA.chain(p)} x='
              + '/'.join(f'{worst[engine, n][0]:.2f}' for n in (1, 2, 3)) + ' aux='
              + '/'.join(f'{worst[engine, n][1]:.2f}' for n in (1, 2, 3)))
