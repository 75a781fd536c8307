"""Golden fixture of the Green functions (``pycsou/math/green.py``) and of ``MappedDistanceMatrix`` built on them
(``pycsou/linop/sampling.py:772-1058``), from the REAL reference code imported as in ``make_golden.py`` (same
stand-in modules, nothing copied).

Build container only:  ``python tests/golden/make_golden_green.py``  ->  ``tests/golden/green_mdm.npz`` (arrays
only, under 300 KB).  Inputs and the layout of the stacked arrays come from ``tests/mdm_cases.py``, which the tests
regenerate.  Every product is the reference's own dense operator (``operator_type='dense'``) in fp64, applied to x
and adjoint-applied to y; the function values are the reference's own classes on ``EVAL_R``.

Asserted before saving: the reference's constructor errors and attributes that the host test pins (``TypeError``
for k = 4, for alpha = 0 and alpha = 2; ``Wendland(...).support`` the float epsilon; ``Matern.support(2)``), the mask
of the causal functions at a negative argument, NaN of ``SubGaussian`` there, and 0 ** 0 = 1.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)


def raises(f, *a):
    try:
        f(*a)
    except TypeError:
        return True
    return False


def main():
    from make_golden import import_reference
    from tests import mdm_cases as C
    import_reference()
    from pycsou.linop import sampling as rsamp
    from pycsou.math import green as G

    assert raises(G.Matern, 4) and raises(G.Wendland, -1) and raises(G.CausalGreenExponential, 1, 0)
    assert raises(G.SubGaussian, 0) and raises(G.SubGaussian, 2)
    assert G.Wendland(2, 0.75).support == 0.75 and G.Matern(1, 0.5).support(2) == 1.0
    neg = np.array([-0.5, 0.0, 0.5])
    assert np.array_equal(G.CausalGreenIteratedDerivative(1)(neg), [0, 1, 1])
    assert np.array_equal(G.CausalGreenExponential(1, 1.5)(neg)[:2], [0, 1])
    with np.errstate(invalid='ignore'):
        assert np.isnan(G.SubGaussian(0.8, 0.5)(neg)[0])

    out = {}
    with np.errstate(invalid='ignore'):
        out['eval'] = np.stack([np.asarray(C.make(G, f)(C.EVAL_R), dtype=np.float64) for f in C.FUNC_NAMES])

    def dense(func, P, Q, mode, ord):
        op = rsamp.MappedDistanceMatrix(samples1=P, samples2=Q, function=func, mode=mode, ord=ord,
                                        operator_type='dense', verbose=0, n_jobs=1)
        assert isinstance(op.mat, np.ndarray) and op.mat.dtype == np.float64
        return op

    P, Q, x, y = C.sweep_inputs('radial')
    fwd = np.empty((len(C.FUNC_NAMES), len(C.ORDS), P.shape[0]))
    adj = np.empty((len(C.FUNC_NAMES), len(C.ORDS), Q.shape[0]))
    for i, f in enumerate(C.FUNC_NAMES):
        for j, o in enumerate(C.ORDS):
            op = dense(C.make(G, f), P, Q, 'radial', o)
            fwd[i, j], adj[i, j] = op * x, op.adjoint(y)
    out['sweep_fwd'], out['sweep_adj'] = fwd, adj

    P, Q, x, y = C.sweep_inputs('zonal')
    ops = [dense(C.make(G, f), P, Q, 'zonal', 2.) for f in C.ZONAL_FUNCS]
    out['zonal_fwd'], out['zonal_adj'] = np.stack([op * x for op in ops]), np.stack([op.adjoint(y) for op in ops])

    shape = np.empty((len(C.DIMS), len(C.NCOLS), C.NP))
    for a, dim in enumerate(C.DIMS):
        P, Q, x, _ = C.points(dim)
        for b, nc in enumerate(C.NCOLS):
            shape[a, b] = dense(C.make(G, C.SHAPE_FUNC), P, Q[:nc], 'radial', 2.) * x[:nc]
    out['shape'] = shape

    P, _, _, y = C.sweep_inputs('radial')
    sym = dense(C.make(G, C.SHAPE_FUNC), P, None, 'radial', 2.)
    assert sym.is_symmetric
    out['sym_fwd'] = sym * y

    assert all(np.all(np.isfinite(v)) for k, v in out.items() if k != 'eval')
    path = os.path.join(HERE, 'green_mdm.npz')
    np.savez_compressed(path, **out)
    print('green_mdm.npz', {k: v.shape for k, v in out.items()}, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 300_000


if __name__ == '__main__':
    main()
