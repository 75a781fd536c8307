"""Golden fixtures for the rest of ``pycsou.func``: the L1-ball family, KL, log barrier, entropy, from the
REAL reference code imported as in ``make_golden.py`` (same stand-in modules, nothing copied).

Build container only:  ``python tests/golden/make_golden_func.py``  ->  ``tests/golden/func_family.npz``
(arrays only).

The reference's own ``proj_l1_ball`` (``pycsou/math/prox.py:117-164``), ``SquaredL1Norm`` / ``L1Ball`` /
``LInftyNorm`` / ``LogBarrier`` / ``ShannonEntropy`` / ``QuadraticForm`` (``pycsou/func/penalty.py:248-417,
770-990``), ``KLDivergence`` and the ball / consistency losses (``pycsou/func/loss.py:222-682``), ``APGD`` and
``CPS`` (``pycsou/opt/proxalgs.py``) produce the vectors, on the inputs of ``tests/func_family_cases.py``
(which the tests regenerate; only the outputs are stored).  PyLops arithmetic comes from ``oracle.pylops1``
as in ``make_golden_stacks.py``.

(a) prox vectors, (b) APGD with G = L1Ball / LInftyNorm / SquaredL1Norm, (c) Poisson-TV CPS with a KL data
term, (d) APGD with an entropy penalty.  The natural-stop runs must not sit on the stopping threshold: the
last metric value above it has to exceed it by more than 1 % (asserted below).
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
    from oracle.pycsou_ref import gaussian_psf, phantom
    from tests import func_family_cases as C
    R = import_reference()
    pylops = sys.modules['pylops']
    pylops.Gradient = lambda dims, sampling=1, edge=False, dtype='float64', kind='centered': \
        P.Gradient(dims, sampling=sampling, edge=edge, dtype=dtype, kind=kind)
    from pycsou.linop import diff as rdiff
    lb, fb, pen, loss, mprox = R.lbase, R.fbase, R.penalty, R.loss, R.mprox
    out = {}

    # ---- (a) threshold family: one concatenated array per family, cases in the order of the loops
    fam = {'l1ball': [], 'linfty': [], 'sql1': [], 'sql1_root': []}
    worst = 0.0
    for n in C.FIXTURE_SIZES:
        for kind in C.KINDS:
            x = C.make_x(kind, n)
            for name, par, a, b, mode in C.thresh_params(kind, n, x):
                if name == 'l1ball':
                    y = pen.L1Ball(dim=n, radius=a).prox(x.copy(), tau=1.0)
                    assert np.array_equal(y, mprox.proj_l1_ball(x.copy(), radius=a))
                elif name == 'linfty':
                    y = pen.LInftyNorm(dim=n).prox(x.copy(), tau=par)
                else:
                    y = pen.SquaredL1Norm(dim=n, prox_computation='sort').prox(x.copy(), tau=par)
                fam[name].append(np.asarray(y, dtype=np.float64))
                worst = max(worst, np.max(np.abs(y - C.exact_prox(x, a, b, mode)[1])) / max(1.0, np.abs(x).max()))
    # the 'root' computation (brentq on mu, [FirstOrd] Lemma 6.70) on the generic kinds
    for n in (63, 257):
        for kind in ('normal', 'mixed'):
            x = C.make_x(kind, n)
            for tau in C.TAUS:
                fam['sql1_root'].append(pen.SquaredL1Norm(dim=n, prox_computation='root').prox(x.copy(), tau=tau))
    for k, v in fam.items():
        out['thr_' + k] = np.concatenate(v)
    print('threshold family vs exact restatement, worst scaled error', worst)

    # ---- (a) element-wise
    xk, yk = C.kl_inputs()
    for tau in C.KL_TAUS:
        out[f'kl_prox_{tau}'] = loss.KLDivergence(dim=xk.size, data=yk).prox(xk.copy(), tau=tau)
        out[f'logb_prox_{tau}'] = pen.LogBarrier(dim=xk.size).prox(xk.copy(), tau=tau)
        xe = C.entropy_inputs(tau)
        out[f'ent_prox_{tau}'] = pen.ShannonEntropy(dim=xe.size).prox(xe.copy(), tau=tau)
        assert np.all(np.isfinite(out[f'ent_prox_{tau}']))

    # ---- (a) functionals: prox, fenchel_prox and value at one vector
    n = 65
    rng = np.random.default_rng(5)
    v = C.make_x('normal', n) * 2.0
    vp = np.abs(v) + 0.05                       # positive: finite KL / barrier / entropy values
    d = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    yc = rng.poisson(3.0, n).astype(np.float64)
    M = rng.standard_normal((n, n))
    M = M @ M.T / n + np.eye(n)
    out.update(fn_v=v, fn_vp=vp, fn_d=d, fn_yc=yc, fn_M=M)
    Lop = lb.DenseLinearOperator(M)
    Lop.lipschitz_cst = Lop.diff_lipschitz_cst = float(np.linalg.norm(M, 2))
    funcs = {
        'l1ball': (pen.L1Ball(dim=n, radius=4.0), v),
        'linfty': (pen.LInftyNorm(dim=n), v),
        'linfty3': (3.0 * pen.LInftyNorm(dim=n), v),
        'sql1': (pen.SquaredL1Norm(dim=n), v),
        'sql1x2': (2 * pen.SquaredL1Norm(dim=n), v),
        'logb': (pen.LogBarrier(dim=n), vp),
        'entropy': (pen.ShannonEntropy(dim=n), vp),
        'kl': (loss.KLDivergence(dim=n, data=yc), vp),
        'l2ballloss': (loss.L2BallLoss(dim=n, data=d, radius=3.0), v),
        'l1ballloss': (loss.L1BallLoss(dim=n, data=d, radius=4.0), v),
        'linftyballloss': (loss.LInftyBallLoss(dim=n, data=d, radius=0.8), v),
        'linftyloss': (loss.LInftyLoss(dim=n, data=d), v),
        'sql1loss': (loss.SquaredL1Loss(dim=n, data=d), v),
        'consistency': (loss.ConsistencyLoss(dim=n, data=d), v),
    }
    for name, (f, arg) in funcs.items():
        out[f'fn_{name}_prox'] = np.asarray(f.prox(arg.copy(), tau=0.7), dtype=np.float64)
        out[f'fn_{name}_fenchel'] = np.asarray(f.fenchel_prox(arg.copy(), sigma=1.3), dtype=np.float64)
        out[f'fn_{name}_value'] = np.array(float(f(arg.copy())))
    out['fn_consistency_value_at_data'] = np.array(float(funcs['consistency'][0](d.copy())))
    out['fn_l1ball_value_inside'] = np.array(float(funcs['l1ball'][0](v / np.abs(v).sum())))
    for name, q in (('quad', pen.QuadraticForm(dim=n)), ('quadL', pen.QuadraticForm(dim=n, linop=Lop))):
        out[f'fn_{name}_value'] = np.array(float(q(v)))
        out[f'fn_{name}_grad'] = q.gradient(v)
        out[f'fn_{name}_dlip'] = np.array(float(q.diff_lipschitz_cst))

    # ---- (b) APGD, F = 1/2 ||A x - y||^2, G = L1Ball(r) / 0.5 LInftyNorm / 0.02 SquaredL1Norm
    A, xs, y = C.sparse_problem()
    Glip = float(np.linalg.norm(A, 2))

    def apgd(G, niter, thr, mi, tag):
        Gop = lb.DenseLinearOperator(A)
        Gop.lipschitz_cst = Gop.diff_lipschitz_cst = Glip
        F = (1 / 2) * loss.SquaredL2Loss(dim=64, data=y) * Gop
        s = R.proxalgs.APGD(dim=128, F=F, G=G, acceleration='CD', max_iter=niter - 1, min_iter=mi,
                            accuracy_threshold=thr, verbose=None)
        est, _, diag = s.iterate()
        dg = diag['Relative Improvement'].to_numpy(float)
        if thr > 0:  # natural stop: not decided by the last bits of the projection
            above = dg[1:][dg[1:] > thr]
            assert s.iter < niter and above[-1] > 1.01 * thr, (tag, s.iter, above[-1] / thr)
            print(tag, 'stops after', s.iter, 'iterations; last metric above the threshold / threshold =',
                  above[-1] / thr)
        assert np.all(np.isfinite(est['iterand']))
        for k, val in dict(x=est['iterand'], past_aux=est['past_aux'], n_iter=s.iter, tau=s.tau, diag=dg,
                           max_iter=niter - 1, min_iter=mi, thr=thr).items():
            out[f'apgd_{tag}_{k}'] = np.asarray(val)

    out['apgd_Glip'] = np.array(Glip)
    for r in (3, 6):
        apgd(pen.L1Ball(dim=128, radius=float(r)), 40, 0.0, 39, f'l1ball{r}_fixed')
        apgd(pen.L1Ball(dim=128, radius=float(r)), 500, 1e-4, 10, f'l1ball{r}_stop')
    apgd(0.5 * pen.LInftyNorm(dim=128), 30, 0.0, 29, 'linfty')
    apgd(0.02 * pen.SquaredL1Norm(dim=128), 30, 0.0, 29, 'sql1')

    # ---- (c) Poisson-TV: CPS, K = [Conv; Gradient], H = KL(y) (+) 0.3 L21, G = NonNegativeOrthant
    shape = (24, 20)
    N = shape[0] * shape[1]
    psf = gaussian_psf(5, 1.0)
    img = 12.0 * phantom(shape, n_rect=6, seed=2)
    PyLop = lb.PyLopLinearOperator
    Conv = PyLop(P.Convolve2D(N, psf, shape, offset=tuple(P.pycsou_offset(s) for s in psf.shape)))
    Conv.lipschitz_cst = Conv.diff_lipschitz_cst = 1.0
    yp = np.random.default_rng(9).poisson(Conv(img.ravel()).clip(0)).astype(np.float64)
    assert (yp == 0).any() and (yp > 0).any()
    D = rdiff.Gradient(shape=shape, kind='forward')
    D.lipschitz_cst = D.diff_lipschitz_cst = float(np.sqrt(8.0))
    H = fb.ProxFuncHStack(loss.KLDivergence(dim=N, data=yp), 0.3 * pen.L21Norm(dim=2 * N, groups=np.tile(np.arange(N), 2)))
    K = lb.LinOpVStack(Conv, D)
    cps = R.proxalgs.CPS(dim=N, G=pen.NonNegativeOrthant(dim=N), H=H, K=K, max_iter=39, min_iter=39,
                         accuracy_threshold=0.0, verbose=None)
    est, _, diag = cps.iterate()
    assert np.all(np.isfinite(est['primal_variable'])) and cps.iter == 40
    for k, val in dict(psf=psf, y=yp, shape=np.array(shape), x=est['primal_variable'], z=est['dual_variable'],
                       n_iter=cps.iter, tau=cps.tau, sigma=cps.sigma, rho=cps.rho, Klip=K.lipschitz_cst,
                       Clip=Conv.lipschitz_cst, Dlip=D.lipschitz_cst,
                       diag_primal=diag['Relative Improvement (primal variable)'].to_numpy(float),
                       diag_dual=diag['Relative Improvement (dual variable)'].to_numpy(float)).items():
        out[f'ptv_{k}'] = np.asarray(val)
    print('poisson-tv cps', cps.iter, 'iterations, zeros in y:', int((yp == 0).sum()))

    # ---- (d) entropy APGD on the same blur: F = 1/2 ||C x - y||^2, G = 0.5 ShannonEntropy
    # (the image at its count scale: at unit scale the entropy term's curvature makes the run converge to the
    # rounding floor in 30 iterations, and a metric of 1e-15 cannot be compared to rtol 1e-6)
    ye = Conv(img.ravel()) + 0.1 * np.random.default_rng(10).standard_normal(N)
    F = (1 / 2) * loss.SquaredL2Loss(dim=N, data=ye) * Conv
    s = R.proxalgs.APGD(dim=N, F=F, G=0.5 * pen.ShannonEntropy(dim=N), acceleration='CD', max_iter=29, min_iter=29,
                        accuracy_threshold=0.0, verbose=None)
    est, _, diag = s.iterate()
    assert np.all(np.isfinite(est['iterand'])) and s.iter == 30
    assert diag['Relative Improvement'].to_numpy(float)[-1] > 1e-9, 'the metric reached the rounding floor'
    for k, val in dict(y=ye, x=est['iterand'], n_iter=s.iter, tau=s.tau,
                       diag=diag['Relative Improvement'].to_numpy(float)).items():
        out[f'ent_apgd_{k}'] = np.asarray(val)

    path = os.path.join(HERE, 'func_family.npz')
    np.savez_compressed(path, **out)
    print('func_family.npz', len(out), 'arrays,', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
