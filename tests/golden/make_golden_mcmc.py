"""Golden fixtures for the PMYULA sampler and the P-square estimator, from the REAL reference code imported as in
``make_golden.py`` (same stand-in modules, ``numba.njit`` the identity; nothing copied).

Build container only:  ``python tests/golden/make_golden_mcmc.py``  ->  ``tests/golden/mcmc.npz`` (arrays only).
Inputs come from ``tests/mcmc_cases.py``, which the tests regenerate.

``PMYULA.update_iterand`` draws from an undefined module global ``rng`` (``pycsou/opt/mcmc.py:112``); it runs once
that global is injected, ``mcmc.rng = np.random.default_rng(seed)``, which is what the constructor's unused
``self.rng`` evidently intends.  The stubbed ``pylops`` gets ``CausalIntegration`` (restated here: cumsum) and the
oracle's ``Smoothing1D`` so that the reference's own ``Integration1D`` / ``MovingAverage1D`` / ``DownSampling``
build the demo's forward model.

Sensitivity measurement: every chain is re-run with its data-fidelity products formed by a dense matrix whose
columns (A x) and rows (A^T r) are summed in a permuted order -- the size of change a different reduction tree
makes -- for ``N_PERM`` permutations; the largest deviation of every output is stored as ``<problem>_dev_<output>``
and the device tests allow 8 times that.

Asserted before saving: the P-square doctest value, ``count == 33`` for the dense problem, that every P-square
stream fired both update branches (and, unless it is monotone, both end replacements; a monotone stream fires
its own end on every sample), that the float64 restatement of ``tests/mcmc_cases.py`` equals the reference bit
for bit, and that every result is finite.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

N_PERM = 8


def main():
    from make_golden import import_reference
    from oracle import pylops1 as P
    from tests import mcmc_cases as C
    R = import_reference()
    pylops = sys.modules['pylops']

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

    pylops.CausalIntegration = CausalIntegration
    pylops.Smoothing1D = P.Smoothing1D
    from pycsou.linop import diff as rdiff, conv as rconv, sampling as rsamp
    from pycsou.opt import mcmc as rmcmc
    from pycsou.util import stats as rstats
    pen, loss, Dense = R.penalty, R.loss, R.lbase.DenseLinearOperator
    out = {}

    # ---------------- P-square: doctest, streams ----------------
    rng = np.random.default_rng(0)
    p2 = rstats.P2Algorithm(pvalue=0.95)
    for _ in range(1000):
        p2.add_sample(rng.standard_normal())
    assert p2.q.shape == (1,) and f'{p2.q[0]:.8f}' == f'{C.DOCTEST_Q:.8f}', p2.q
    out['doctest_q'] = np.asarray(p2.q, dtype=np.float64)

    for kind in C.STREAMS:
        s = C.stream(kind)
        states, est = C.restated_states(s, C.P2_PVALUES, np.float64)
        ref = [rstats.P2Algorithm(pvalue=p) for p in C.P2_PVALUES]
        for t, row in enumerate(s, start=1):
            for r in ref:
                r.add_sample(row.copy())
            if t in C.P2_CHECKPOINTS:
                h, p = C.device_layout([r.marker_heights for r in ref], [r.marker_positions for r in ref], np.float64)
                assert np.all(np.isfinite(h))
                assert C.same_bits(h, states[t][0]) and C.same_bits(p, states[t][1]), (kind, t)
                out[f'p2_{kind}_{t}_heights'], out[f'p2_{kind}_{t}_pos'] = h, p
        for e in est:
            f = e.fired
            assert f['parabolic'] > 0 and f['linear'] > 0, (kind, e.pvalue, f)
            if kind == 'ascending':
                assert f['high'] > 0 and f['low'] == 0, (kind, f)
            elif kind == 'descending':  # the constant column takes the upper replacement (s >= q[4]) every time
                assert f['low'] > 0 and f['high'] == C.P2_SAMPLES - 5, (kind, f)
            else:
                assert f['low'] > 0 and f['high'] > 0, (kind, e.pvalue, f)
        print('p2', kind, [e.fired for e in est])

    # ---------------- chains ----------------
    def run(F, G, dim, kw, x0=None, linops=None, tau=None):
        kw = dict(kw)
        seed = kw.pop('seed')
        kw.pop('tau', None)
        rmcmc.rng = np.random.default_rng(seed)
        s = rmcmc.PMYULA(dim=dim, F=F, G=G, x0=x0, tau=tau, verbose=None, seed=seed, linops=linops,
                         accuracy_threshold=1e-5, **kw)
        est, _, diag = s.iterate()
        res = {'mcmc_sample': est['mcmc_sample'], 'count': s.count, 'n_iter': s.iter, 'gamma': s.gamma,
               'tau': np.nan if s.tau is None else s.tau, 'beta': s.beta,
               'diag_iter': diag['Iter'].to_numpy(float),
               'diag_rel': diag['Relative Improvement (MMSE)'].to_numpy(float),
               'diag_nb': diag['Nb of samples'].to_numpy(float)}
        if linops is None:
            assert list(est) == ['mcmc_sample', 'mmse', 'std', 'quantiles', 'pvalues']
            res.update(mmse=est['mmse'], std=est['std'], quantiles=np.stack(est['quantiles']))
        else:
            res.update(mmse=est['mmse_raw'], std=est['std_raw'], quantiles=np.stack(est['quantiles_raw']),
                       mmse_linops=est['mmse_linops'][0], std_linops=est['std_linops'][0],
                       quantiles_linops=np.stack(est['quantiles_linops'][0]))
        return {k: np.asarray(v, dtype=np.float64) for k, v in res.items()}

    def permuted(M, lip, seed):
        """Dense operator of M whose products sum the columns / rows in a permuted order."""
        rng = np.random.default_rng([51, seed])
        pc, pr = rng.permutation(M.shape[1]), rng.permutation(M.shape[0])
        Mc, Mr = np.ascontiguousarray(M[:, pc]), np.ascontiguousarray(M[pr, :])

        class Permuted(Dense):
            def __call__(self, x):
                return Mc @ np.asarray(x)[pc]

            def adjoint(self, y):
                return Mr.T @ np.asarray(y)[pr]

        op = Permuted(M)
        op.lipschitz_cst = op.diff_lipschitz_cst = lip
        return op

    def record(name, base, variants):
        for k, v in base.items():
            assert np.all(np.isfinite(v) | (k in ('diag_rel', 'tau'))), (name, k)
            out[f'{name}_{k}'] = v
        for k in base:
            if k in ('count', 'n_iter', 'gamma', 'tau', 'beta', 'diag_iter', 'diag_nb') or k.startswith('quantiles'):
                continue
            fin = np.isfinite(base[k])
            dev = max(float(np.max(np.abs(v[k][fin] - base[k][fin]), initial=0.0)) for v in variants)
            for v in variants:
                assert np.array_equal(np.isfinite(v[k]), fin), (name, k)
            out[f'{name}_dev_{k}'] = np.asarray(dev)
            print(f'  {name} {k}: largest deviation over {len(variants)} permuted runs {dev:.3e} '
                  f'(scale {float(np.max(np.abs(base[k][fin]))):.3e})')

    A, y, x0 = C.dense_problem()
    Alip = float(np.linalg.norm(A, 2))

    def dense_F(op):
        return (1 / 2) * loss.SquaredL2Loss(dim=A.shape[0], data=y) * op

    Aop = Dense(A)
    Aop.lipschitz_cst = Aop.diff_lipschitz_cst = Alip
    dim = A.shape[1]
    base = run(dense_F(Aop), C.DENSE_LAM * pen.L1Norm(dim=dim), dim, C.DENSE)
    assert int(base['count']) == C.DENSE_COUNT and int(base['n_iter']) == C.DENSE['max_iter'] + 1
    beta = float(base['beta'])
    assert np.isclose(base['tau'], 2 / beta) and np.isclose(base['gamma'], base['tau'] / (beta * base['tau'] + 1))
    record('dense_l1', base, [run(dense_F(permuted(A, Alip, s)), C.DENSE_LAM * pen.L1Norm(dim=dim), dim, C.DENSE)
                              for s in range(N_PERM)])
    base = run(dense_F(Aop), None, dim, C.DENSE, x0=x0)
    assert int(base['count']) == C.DENSE_COUNT and np.isnan(base['tau']) and np.isclose(base['gamma'], 1 / beta)
    record('dense_null', base, [run(dense_F(permuted(A, Alip, s)), None, dim, C.DENSE, x0=x0) for s in range(N_PERM)])

    # the demo at the bottom of mcmc.py at N = 8
    sig = C.demo_signal()
    n = sig.size
    S = rsamp.DownSampling(size=n, downsampling_factor=4) * rconv.MovingAverage1D(window_size=8, shape=(n,))
    Iop = rdiff.Integration1D(size=n)
    Gop = S * Iop
    Gd = np.stack([Gop(e) for e in np.eye(n)], axis=1)
    Glip = float(np.linalg.norm(Gd, 2))
    Gop.lipschitz_cst = Gop.diff_lipschitz_cst = Glip
    Iop.lipschitz_cst = Iop.diff_lipschitz_cst = float(np.linalg.norm(np.tril(np.ones((n, n))), 2))
    yd = S(sig) + C.demo_noise(S.shape[0])

    def demo_F(op):
        return (1 / 2) * loss.SquaredL2Loss(dim=S.shape[0], data=yd) * op

    Gball = pen.L2Ball(dim=n, radius=C.DEMO_RADIUS)
    apgd = R.proxalgs.APGD(dim=n, F=demo_F(Gop), G=Gball, min_iter=100, max_iter=1e4, accuracy_threshold=1e-4,
                           verbose=None)
    est, _, _ = apgd.iterate()
    xd0 = est['iterand'] + 0.05 * np.random.default_rng(44).standard_normal(n)
    base = run(demo_F(Gop), Gball, n, C.DEMO, x0=xd0, linops=(Iop,), tau=C.DEMO['tau'])
    assert int(base['count']) == 50
    out['demo_y'], out['demo_x0'], out['demo_Glip'] = yd, xd0, np.asarray(Glip)
    record('demo', base, [run(demo_F(permuted(Gd, Glip, s)), Gball, n, C.DEMO, x0=xd0, linops=(Iop,),
                              tau=C.DEMO['tau']) for s in range(N_PERM)])

    path = os.path.join(HERE, 'mcmc.npz')
    np.savez_compressed(path, **out)
    print('mcmc.npz', len(out), 'arrays,', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 500_000


if __name__ == '__main__':
    main()
