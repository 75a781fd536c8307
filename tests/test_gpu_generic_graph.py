"""The generic (operator-by-operator) PDS loop as hipGraph chunks against the same loop launched
eagerly (PCS_GENERIC_GRAPH=0): the captured chunks issue the same kernels in the same order, so
x, z, the iteration count and every diagnostics row are bitwise equal -- for fixed counts that end
inside a chunk, natural stops, both dtypes, a general-label L21Norm, a ProxFuncHStack H and a
primal-only problem; the verbose lines match too.  An FFT-path K (Convolve2D with a 33 x 33 PSF: rocFFT between
the pad and crop kernels) is bitwise the eager loop too, and whether it ran inside the capture is pinned to what
an MI355X does (FFT_K_GRAPH_USED).  A capture that raises on the host, and an out-of-memory error while the ring
is allocated, fall back to the eager loop with the same bits, and the next problem captures again.

Reference: the loop of pycsou/core/solver.py:55-76 with PrimalDualSplitting.update_iterand,
pycsou/opt/proxalgs.py:343-355; L21Norm labels pycsou/func/penalty.py:525-560, ProxFuncHStack
pycsou/func/base.py:21-89.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# observed on an MI355X: rocFFT's launches are captured like any other, the chunks replay
FFT_K_GRAPH_USED = True


def _problem(name, n, dtype, max_iter, min_iter, thr, verbose=None):
    from pycsou_amd.func import L1Norm, ProxFuncHStack
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L21Norm
    from pycsou_amd.linop import Gradient
    from pycsou_amd.opt import PDS
    N = n * n
    rng = np.random.default_rng(11)
    img = np.zeros((n, n))
    img[n // 4:3 * n // 4, n // 3:2 * n // 3] = 1.0
    npdt = np.float32 if dtype == torch.float32 else np.float64
    y = torch.from_numpy((img.ravel() + 0.1 * rng.standard_normal(N)).astype(npdt)).cuda()
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y)
    if name == 'primal_only':
        return PDS(dim=N, F=F, G=0.05 * L1Norm(dim=N), x0=torch.zeros(N, dtype=dtype, device='cuda'),
                   max_iter=max_iter, min_iter=min_iter, accuracy_threshold=thr, verbose=verbose, engine='generic')
    if name == 'fft_k':
        from pycsou_amd.linop import Convolve2D
        from tests.views import fft_psf
        K = Convolve2D(N, fft_psf(), (n, n))    # non-negative taps of unit sum: ||K|| <= 1
        K.lipschitz_cst = K.diff_lipschitz_cst = 1.0
        assert K.plan(dtype, False) is None, 'wider than the direct tiers: the FFT path'
        return PDS(dim=N, F=F, H=0.1 * L1Norm(dim=N), K=K, x0=torch.zeros(N, dtype=dtype, device='cuda'),
                   z0=torch.zeros(N, dtype=dtype, device='cuda'), max_iter=max_iter, min_iter=min_iter,
                   accuracy_threshold=thr, verbose=verbose, engine='generic')
    K = Gradient(shape=(n, n), kind='forward')
    K.lipschitz_cst = K.diff_lipschitz_cst = float(np.sqrt(8.0))
    if name == 'no_capture':
        K = _NoCapture(K)
    if name == 'l21_labels':
        lab = np.arange(N) // 2
        H = 0.1 * L21Norm(dim=2 * N, groups=np.concatenate([lab, lab]))
    else:
        H = ProxFuncHStack(0.1 * L1Norm(dim=N), 0.1 * L1Norm(dim=N))
    return PDS(dim=N, F=F, H=H, K=K, x0=torch.zeros(N, dtype=dtype, device='cuda'),
               z0=torch.zeros(2 * N, dtype=dtype, device='cuda'), max_iter=max_iter, min_iter=min_iter,
               accuracy_threshold=thr, verbose=verbose, engine='generic')


def _NoCapture(inner):
    """A LinearOperator that delegates to `inner` and raises on the host from _apply while the stream is capturing."""
    from pycsou_amd.core.linop import LinearOperator

    class NoCapture(LinearOperator):
        def __init__(self, op):
            super().__init__(shape=op.shape, dtype=op.dtype, lipschitz_cst=op.lipschitz_cst)
            self.op, self.refused = op, 0

        def _apply(self, t):
            if torch.cuda.is_current_stream_capturing():
                self.refused += 1
                raise RuntimeError('this operator does not run under stream capture')
            return self.op._apply(t)

        def _adj(self, t):
            return self.op._adj(t)
    return NoCapture(inner)


def _run(monkeypatch, graph, *args, **kw):
    monkeypatch.setenv('PCS_GENERIC_GRAPH', '1' if graph else '0')
    pds = _problem(*args, **kw)
    est, _, diag = pds.iterate()
    return pds, est, diag


def _same(a, b):
    (pa, ea, da), (pb, eb, db) = a, b
    assert pa.iter == pb.iter
    for k in ea:
        if ea[k] is None:
            assert eb[k] is None
        else:
            assert torch.equal(ea[k], eb[k]), k
    assert list(da.columns) == list(db.columns)
    for c in da.columns:
        np.testing.assert_array_equal(da[c].to_numpy(float), db[c].to_numpy(float))


@pytest.mark.parametrize('name,dtype', [('l21_labels', torch.float32), ('l21_labels', torch.float64),
                                        ('stack_h', torch.float32), ('primal_only', torch.float64),
                                        ('fft_k', torch.float64)])
@pytest.mark.parametrize('stop', ['fixed_11', 'fixed_16', 'natural'])
def test_generic_graph_bitwise_eager(monkeypatch, name, dtype, stop):
    n = 32 if name == 'fft_k' else 64
    if stop == 'natural':
        args = (name, n, dtype, 500, 3, 2e-3)
    else:  # max_iter = min_iter = m runs m + 1 iterations (solver.py:65-66): 11 ends inside a chunk of 4
        m = int(stop.split('_')[1]) - 1
        args = (name, n, dtype, m, m, 1e-3)
    g = _run(monkeypatch, True, *args)
    e = _run(monkeypatch, False, *args)
    if name == 'fft_k':  # bitwise the eager loop either way; whether rocFFT ran inside the capture is pinned
        assert g[0]._graph_used is FFT_K_GRAPH_USED and e[0]._graph_used is False
    else:
        assert getattr(g[0], '_graph_used', False) and not getattr(e[0], '_graph_used', False)
    _same(g, e)
    if stop == 'natural':
        assert 3 < g[0].iter < 500
    else:
        assert g[0].iter == int(stop.split('_')[1])


def test_generic_graph_verbose_lines(monkeypatch, capsys):
    _run(monkeypatch, True, 'l21_labels', 32, torch.float64, 500, 3, 1e-3, verbose=5)
    out_g = capsys.readouterr().out
    _run(monkeypatch, False, 'l21_labels', 32, torch.float64, 500, 3, 1e-3, verbose=5)
    out_e = capsys.readouterr().out
    assert out_g == out_e and out_g.count('\n') >= 2


def test_generic_graph_capture_failure_falls_back(monkeypatch):
    """A K that raises on the host under stream capture: _iterate_generic_graph returns None and the eager loop
    runs -- same x, z, count and diagnostics as PCS_GENERIC_GRAPH=0 -- and an ordinary problem afterwards in the
    same process captures again."""
    args = ('no_capture', 32, torch.float64, 10, 10, 1e-3)
    g = _run(monkeypatch, True, *args)
    assert g[0]._graph_used is False and g[0].K.refused == 1
    e = _run(monkeypatch, False, *args)
    assert e[0]._graph_used is False and e[0].K.refused == 0
    _same(g, e)
    assert g[0].iter == 11
    plain = ('stack_h', 32, torch.float64, 10, 10, 1e-3)
    g2 = _run(monkeypatch, True, *plain)
    e2 = _run(monkeypatch, False, *plain)
    assert g2[0]._graph_used is True and e2[0]._graph_used is False
    _same(g2, e2)
    _same(g2, g)    # the wrapper delegates: the same problem


def test_generic_graph_out_of_memory_falls_back(monkeypatch):
    """torch.cuda.OutOfMemoryError from the first allocation inside _iterate_generic_graph (the history, the
    state ring, the pinned pair: all inside its try) falls back to the eager loop.  Nothing is exhausted: the
    first torch.empty_like inside the method is made to raise."""
    from pycsou_amd.opt import PDS
    args = ('stack_h', 32, torch.float64, 10, 10, 1e-3)
    e = _run(monkeypatch, False, *args)
    armed = {'on': False, 'raised': 0}
    real_empty_like, real_iter = torch.empty_like, PDS._iterate_generic_graph

    def empty_like(*a, **kw):
        if armed['on']:
            armed['on'] = False
            armed['raised'] += 1
            raise torch.cuda.OutOfMemoryError('planted: out of memory')
        return real_empty_like(*a, **kw)

    def iterate_graph(self, state):
        armed['on'] = True
        try:
            return real_iter(self, state)
        finally:
            armed['on'] = False

    monkeypatch.setattr(torch, 'empty_like', empty_like)
    monkeypatch.setattr(PDS, '_iterate_generic_graph', iterate_graph)
    g = _run(monkeypatch, True, *args)
    assert armed['raised'] == 1 and g[0]._graph_used is False
    _same(g, e)
    monkeypatch.setattr(PDS, '_iterate_generic_graph', real_iter)
    g3 = _run(monkeypatch, True, *args)
    assert g3[0]._graph_used is True
    _same(g3, e)
