"""Golden fixtures for the directional derivatives and ``Integration1D`` of ``pycsou.linop.diff``, from the
REAL reference code imported as in ``make_golden.py`` (same stand-in modules, nothing copied).

Build container only:  ``python tests/golden/make_golden_diff_family.py``  ->  ``tests/golden/diff_family.npz``
(arrays only).  Inputs come from ``tests/diff_family_cases.py``, which the tests regenerate.

The stubbed ``pylops`` module is filled with restatements written here on top of ``oracle.pylops1`` --
``FirstDirectionalDerivative`` = sum o diag o ``Gradient``, ``SecondDirectionalDerivative`` = ``-D^T D``,
``CausalIntegration`` = cumsum / flipped cumsum, ``Smoothing1D`` from the oracle -- and the reference's OWN
``FirstDirectionalDerivative`` / ``SecondDirectionalDerivative`` (kill-edge mask, ``pycsou/linop/diff.py:596-606``),
``DirectionalGradient`` (``LinOpVStack``), ``DirectionalLaplacian`` (weight quirk, ``diff.py:766-774``),
``Integration1D``, ``DownSampling``, ``MovingAverage1D``, ``PDS`` and ``APGD`` produce the vectors.

Asserted before saving: the doctest ``diff.py:422-429`` and a dot test
``|<A x, y> - <x, A^T y>| <= 1e-12 ||x|| ||y||`` for every restated operator.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)


def main():
    from make_golden import import_reference
    from oracle import pylops1 as P
    from tests import diff_family_cases as C
    R = import_reference()
    pylops = sys.modules['pylops']

    class FirstDir(P._Op):
        """PyLops 1.x FirstDirectionalDerivative: Sum(dims=(ndim, N), dir=0) * Diagonal(v.ravel()) * Gradient."""

        def __init__(self, dims, v, sampling=1, edge=False, dtype='float64', kind='centered'):
            self.dims, self.nd, self.N = tuple(dims), len(dims), int(np.prod(dims))
            super().__init__((self.N, self.N), dtype)
            self.G = P.Gradient(self.dims, sampling=sampling, edge=edge, dtype=dtype, kind=kind)
            v = np.asarray(v, dtype=np.float64)
            if v.ndim == 1:  # one direction: PyLops repeats it over the entries
                v = np.repeat(v, self.N)
            self.v = v.ravel()
            assert self.v.size == self.nd * self.N

        def matvec(self, x):
            return np.sum((self.v * self.G.matvec(x)).reshape(self.nd, self.N), axis=0)

        def rmatvec(self, y):
            return self.G.rmatvec(self.v * np.tile(y, self.nd))

    class SecondDir(P._Op):
        """PyLops 1.x SecondDirectionalDerivative: -Dv^T Dv with the centred first directional derivative."""

        def __init__(self, dims, v, sampling=1, edge=False, dtype='float64'):
            self.D = FirstDir(dims, v, sampling=sampling, edge=edge, dtype=dtype, kind='centered')
            super().__init__(self.D.shape, dtype)

        def matvec(self, x):
            return -self.D.rmatvec(self.D.matvec(x))

        rmatvec = matvec

    class CausalIntegration(P._Op):
        """PyLops 1.x CausalIntegration with halfcurrent=False: sampling * cumsum along dir."""

        def __init__(self, N, dims=None, dir=-1, sampling=1, halfcurrent=True, dtype='float64'):
            assert not halfcurrent
            super().__init__((N, N), dtype)
            self.dims, self.dir, self.sampling = ((N,) if dims is None else tuple(dims)), dir, sampling

        def matvec(self, x):
            return (self.sampling * np.cumsum(np.reshape(x, self.dims), axis=self.dir)).ravel()

        def rmatvec(self, y):
            y = np.flip(np.reshape(y, self.dims), self.dir)
            return (self.sampling * np.flip(np.cumsum(y, axis=self.dir), self.dir)).ravel()

    pylops.FirstDerivative = lambda N, dims=None, dir=0, sampling=1., edge=False, dtype='float64', kind='centered': \
        P.FirstDerivative(N, dims=dims, dir=dir, sampling=sampling, edge=edge, dtype=dtype, kind=kind)
    pylops.Gradient = lambda dims, sampling=1, edge=False, dtype='float64', kind='centered': \
        P.Gradient(dims, sampling=sampling, edge=edge, dtype=dtype, kind=kind)
    pylops.FirstDirectionalDerivative = FirstDir
    pylops.SecondDirectionalDerivative = SecondDir
    pylops.CausalIntegration = CausalIntegration
    pylops.Smoothing1D = P.Smoothing1D
    from pycsou.linop import diff as rdiff, conv as rconv, sampling as rsamp
    from pycsou.util.misc import peaks
    pen, loss = R.penalty, R.loss
    out = {}

    def dot_test(A, seed):
        rng = np.random.default_rng(seed)
        x, y = rng.standard_normal(A.shape[1]), rng.standard_normal(A.shape[0])
        gap = abs(np.dot(A.matvec(x), y) - np.dot(x, A.rmatvec(y)))
        assert gap <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y), (type(A).__name__, gap)

    # ---- the doctest diff.py:422-429
    x = np.linspace(-2.5, 2.5, 100)
    X, Y = np.meshgrid(x, x)
    Z = peaks(X, Y)
    Dop = rdiff.FirstDirectionalDerivative(shape=Z.shape, directions=np.array([1, 0]), kind='forward')
    D = rdiff.FirstDerivative(size=Z.size, shape=Z.shape, kind='forward')
    assert np.allclose(Dop * Z.flatten(), D * Z.flatten())

    # ---- (a) forward and adjoint vectors
    worst = 0.0
    for tag, shape, field, kind, edge in C.vector_cases():
        xv, yv, v = C.make_x(shape, 0), C.make_x(shape, 1), C.make_dirs(shape, field)
        dot_test(FirstDir(shape, v, sampling=C.steps(shape), edge=edge, kind=kind), 1)
        A = rdiff.FirstDirectionalDerivative(shape=shape, directions=v, step=C.steps(shape), edge=edge, kind=kind)
        out[f'd1_{tag}_fwd'], out[f'd1_{tag}_adj'] = A(xv), A.adjoint(yv)
        for key, adj, arg in ((f'd1_{tag}_fwd', False, xv), (f'd1_{tag}_adj', True, yv)):
            ref = C.first_dir(arg, v, shape, C.steps(shape), kind, edge, adjoint=adj)
            worst = max(worst, np.max(np.abs(out[key] - ref)) / np.max(np.abs(ref)))
    for tag, shape, field, edge in C.second_cases():
        xv, yv, v = C.make_x(shape, 0), C.make_x(shape, 1), C.make_dirs(shape, field)
        dot_test(SecondDir(shape, v, sampling=C.steps(shape), edge=edge), 2)
        A = rdiff.SecondDirectionalDerivative(shape=shape, directions=v, step=C.steps(shape), edge=edge)
        out[f'd2_{tag}_fwd'], out[f'd2_{tag}_adj'] = A(xv), A.adjoint(yv)
        for key, adj, arg in ((f'd2_{tag}_fwd', False, xv), (f'd2_{tag}_adj', True, yv)):
            ref = C.second_dir(arg, v, shape, C.steps(shape), edge, adjoint=adj)
            worst = max(worst, np.max(np.abs(out[key] - ref)) / max(np.max(np.abs(ref)), 1e-300))
    print('directional vectors vs the NumPy definitions, worst scaled error', worst)
    shape = C.LAPLACIAN_SHAPE
    ops = [rdiff.SecondDirectionalDerivative(shape=shape, directions=C.make_dirs(shape, True, seed=s), step=C.steps(shape))
           for s in (0, 1)]
    Lq = rdiff.DirectionalLaplacian(ops, weights=C.LAPLACIAN_WEIGHTS)
    out['lap_fwd'], out['lap_adj'] = Lq(C.make_x(shape, 0)), Lq.adjoint(C.make_x(shape, 1))
    for tag, shape, axis in C.integ_cases():
        N = int(np.prod(shape))
        dot_test(CausalIntegration(N, dims=shape, dir=axis, sampling=C.INT_STEP, halfcurrent=False), 3)
        A = rdiff.Integration1D(size=N, shape=shape, axis=axis, step=C.INT_STEP)
        out[f'int_{tag}_fwd'], out[f'int_{tag}_adj'] = A(C.make_x(shape, 0)), A.adjoint(C.make_x(shape, 1))

    # ---- (b) peaks on a 25 x 25 grid
    g = np.linspace(-2.5, 2.5, 25)
    out['peaks25'] = peaks(*np.meshgrid(g, g))

    # ---- (c) directional-TV denoising: PDS(F = 1/2 ||x - y||^2, K = [D_v; D_vperp], H = lam ||.||_1)
    shape = C.TV_SHAPE
    N = int(np.prod(shape))
    y, v, vp = C.tv_problem()
    Dv = rdiff.FirstDirectionalDerivative(shape=shape, directions=v)
    Dp = rdiff.FirstDirectionalDerivative(shape=shape, directions=vp)
    K = rdiff.DirectionalGradient([Dv, Dp])
    dense = np.stack([K(e) for e in np.eye(N)], axis=1)
    Klip = float(np.linalg.norm(dense, 2))
    K.lipschitz_cst = K.diff_lipschitz_cst = Klip
    pds = R.proxalgs.PDS(dim=N, F=(1 / 2) * loss.SquaredL2Loss(dim=N, data=y), H=C.TV_LAM * pen.L1Norm(dim=2 * N), K=K,
                         x0=np.zeros(N), z0=np.zeros(2 * N), max_iter=C.TV_ITERS - 1, min_iter=C.TV_ITERS - 1,
                         accuracy_threshold=0.0, verbose=None)
    est, _, diag = pds.iterate()
    assert pds.iter == C.TV_ITERS and np.all(np.isfinite(est['primal_variable']))
    for k, val in dict(Klip=Klip, x=est['primal_variable'], z=est['dual_variable'], n_iter=pds.iter, tau=pds.tau,
                       sigma=pds.sigma, rho=pds.rho,
                       diag_primal=diag['Relative Improvement (primal variable)'].to_numpy(float),
                       diag_dual=diag['Relative Improvement (dual variable)'].to_numpy(float)).items():
        out[f'tv_{k}'] = np.asarray(val)
    print('directional TV: ||K|| =', Klip, 'last metric', out['tv_diag_primal'][-1])

    # ---- (d) the forward model of the demo at the bottom of pycsou/opt/mcmc.py as a LASSO
    sig = C.lasso_signal()
    n = sig.size
    S = rsamp.DownSampling(size=n, downsampling_factor=4) * rconv.MovingAverage1D(window_size=8, shape=(n,))
    Iop = rdiff.Integration1D(size=n)
    Gop = S * Iop
    yl = S(sig) + C.lasso_noise(S.shape[0])
    Gd = np.stack([Gop(e) for e in np.eye(n)], axis=1)
    Glip = float(np.linalg.norm(Gd, 2))
    Gop.lipschitz_cst = Gop.diff_lipschitz_cst = Glip
    F = (1 / 2) * loss.SquaredL2Loss(dim=S.shape[0], data=yl) * Gop
    lam = 0.1 * float(np.max(np.abs(F.gradient(0 * sig))))
    apgd = R.proxalgs.APGD(dim=n, F=F, G=lam * pen.L1Norm(dim=n), acceleration='CD', beta=Glip ** 2,
                           max_iter=C.LASSO_ITERS - 1, min_iter=C.LASSO_ITERS - 1, accuracy_threshold=0.0, verbose=None)
    est, _, diag = apgd.iterate()
    assert apgd.iter == C.LASSO_ITERS and np.all(np.isfinite(est['iterand']))
    for k, val in dict(y=yl, Glip=Glip, lam=lam, beta=Glip ** 2, tau=apgd.tau, x=est['iterand'],
                       past_aux=est['past_aux'], n_iter=apgd.iter,
                       diag=diag['Relative Improvement'].to_numpy(float)).items():
        out[f'lasso_{k}'] = np.asarray(val)
    print('integration LASSO: ||S I|| =', Glip, 'lam', lam, 'nonzeros', int(np.count_nonzero(est['iterand'])))

    path = os.path.join(HERE, 'diff_family.npz')
    np.savez_compressed(path, **out)
    print('diff_family.npz', len(out), 'arrays,', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
