"""Golden fixtures for ``Pooling``, ``NNSampling``, ``GeneralisedVandermonde``, ``MappedDistanceMatrix`` and
``SparseLinearOperator`` (``pycsou/linop/sampling.py:394-1058``, ``pycsou/linop/base.py:121-137``), from the REAL
reference code imported as in ``make_golden.py`` (same stand-in modules, nothing copied).

Build container only:  ``python tests/golden/make_golden_sparse.py``  ->  ``tests/golden/sparse_family.npz``
(arrays only).  Inputs come from ``tests/sparse_cases.py``, which the tests regenerate.

Two stand-ins are defined here for what the reference delegates to packages that are absent or have moved on:
``block_reduce`` (scikit-image) restated with NumPy -- pad with ``cval`` to a multiple of the block, view as
blocks, apply ``func`` over the block axes -- and assigned to the reference module's ``block_reduce``; and a
``cKDTree`` subclass whose ``query`` maps the removed ``n_jobs`` keyword to ``workers``.  With them the
reference's OWN ``Pooling``, ``NNSampling``, ``MappedDistanceMatrix`` (sparse through joblib, and dense),
``GeneralisedVandermonde``, ``SparseLinearOperator``, ``APGD`` and ``PDS`` produce the vectors.

Asserted before saving: the reference's doctests (Pooling (4,6)/(2,3) in both modes; the NNSampling indices
``[15 13 12 18 16 5]`` and its adjoint; the sparse and dense MappedDistanceMatrix products; the Vandermonde
matrix; a SparseLinearOperator product), finite iterates, and nonzeros in the LASSO solution.
"""

import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)


def block_reduce(image, block_size, func=np.sum, cval=0, func_kwargs=None):
    """scikit-image's block_reduce restated: pad with ``cval`` up to a multiple of ``block_size``, then apply
    ``func`` over the axes of each block."""
    image = np.asarray(image)
    pad = [(0, (-n) % b) for n, b in zip(image.shape, block_size)]
    image = np.pad(image, pad, mode='constant', constant_values=cval)
    view = image.reshape([v for n, b in zip(image.shape, block_size) for v in (n // b, b)])
    return func(view, axis=tuple(range(1, 2 * image.ndim, 2)), **(func_kwargs or {}))


def main():
    from make_golden import import_reference
    from scipy.spatial import cKDTree
    from tests import sparse_cases as C
    R = import_reference()
    from pycsou.linop import sampling as rsamp

    class Tree(cKDTree):
        def query(self, x, k=1, eps=0, p=2, distance_upper_bound=np.inf, n_jobs=None, workers=1):
            return super().query(x, k=k, eps=eps, p=p, distance_upper_bound=distance_upper_bound,
                                 workers=workers if n_jobs is None else n_jobs)

    rsamp.block_reduce = block_reduce
    rsamp.cKDTree = Tree
    pen, loss, lbase = R.penalty, R.loss, R.lbase
    out = {}

    # ---- doctests
    x = np.arange(24).reshape(4, 6)
    Pm = rsamp.Pooling(shape=x.shape, block_size=(2, 3), pooling_func='mean')
    assert np.array_equal((Pm * x.flatten()).reshape(Pm.output_shape), [[4, 7], [16, 19]])
    assert np.array_equal(Pm.adjoint(Pm * x.flatten()).reshape(x.shape), np.repeat(np.repeat([[4, 7], [16, 19]], 2, 0), 3, 1))
    Ps = rsamp.Pooling(shape=x.shape, block_size=(2, 3), pooling_func='sum')
    assert np.array_equal((Ps * x.flatten()).reshape(Ps.output_shape), [[24, 42], [96, 114]])
    assert np.array_equal(Ps.adjoint(Ps * x.flatten()).reshape(x.shape),
                          np.repeat(np.repeat([[24, 42], [96, 114]], 2, 0), 3, 1))

    samples, grid = C.doctest_nn()
    NN = rsamp.NNSampling(samples=samples, grid=grid)
    assert np.array_equal(NN * x.flatten(), [15, 13, 12, 18, 16, 5]) and NN.shape == (12, 24)
    nn_adj = NN.adjoint((NN * x.flatten()).astype(float))
    assert np.array_equal(nn_adj.reshape(x.shape), [[0, 0, 0, 0, 0, 5], [0] * 6, [12, 13, 0, 15, 16, 0], [18, 0, 0, 0, 0, 0]])
    out['nn_doctest_indices'], out['nn_doctest_adjoint'] = NN.nn_indices, nn_adj

    s1, s2, alpha, beta = C.doctest_mdm()
    kw = dict(function=C.gauss, verbose=0, n_jobs=1)
    M1 = rsamp.MappedDistanceMatrix(samples1=s1, samples2=s2, max_distance=3 * C.SIGMA, operator_type='sparse', **kw)
    M2 = rsamp.MappedDistanceMatrix(samples1=s1, samples2=None, max_distance=3 * C.SIGMA, operator_type='sparse', **kw)
    M3 = rsamp.MappedDistanceMatrix(samples1=s1, samples2=s2, operator_type='dense', **kw)
    assert sp.issparse(M1.mat) and isinstance(M3.mat, np.ndarray) and M1.mat.shape == (10, 3) and M2.mat.shape == (10, 10)
    assert np.allclose(M1 * alpha, [0.27995783, 0.8060865, 0.37589858, 0.09274313, 1.19684992, 0.24525208, 0, 0, 0, 0],
                       rtol=1e-7, atol=0)
    assert np.allclose(M2 * beta, [0.80274037, 1.39329178, 1.27124579, 1.22168244, 1.08494933, 1.36310926, 0.7558366,
                                   0.96398702, 0.85066284, 1.37152693], rtol=1e-7, atol=0)
    assert np.allclose(M3 * alpha, [2.79957838e-01, 8.07329704e-01, 3.77792488e-01, 9.75090904e-02, 1.19686859e+00,
                                    2.45252084e-01, 4.10080770e-05, 5.59512490e-12, 6.22922262e-22, 5.65902486e-35],
                       rtol=1e-8, atol=0)
    assert np.allclose(M3.mat[2], [7.21186665e-001, 9.84802612e-009, 1.51504434e-003], rtol=1e-8, atol=0)
    out['mdm_doctest_sparse'], out['mdm_doctest_sym'], out['mdm_doctest_dense'] = M1 * alpha, M2 * beta, M3 * alpha
    out['mdm_doctest_dense_mat'] = M3.mat
    out['mdm_doctest_sparse_adj'] = M1.adjoint(beta)

    V = rsamp.GeneralisedVandermonde(funcs=[lambda t: t ** 2, lambda t: t ** 3], samples=np.arange(10))
    assert np.array_equal(V.mat, np.stack([np.arange(10.) ** 2, np.arange(10.) ** 3], axis=-1))
    assert np.allclose(V * np.ones(2), np.arange(10) ** 2 + np.arange(10) ** 3)
    out['vandermonde_mat'] = V.mat

    S = lbase.SparseLinearOperator(sp.csr_matrix(np.arange(12.).reshape(3, 4) % 5))
    assert S.is_sparse and not S.is_dense
    assert np.array_equal(S * np.arange(4.), (np.arange(12.).reshape(3, 4) % 5) @ np.arange(4.))

    # ---- pooling, ragged shapes included
    for shape, block in C.POOL_GOLDEN:
        n, m = int(np.prod(shape)), int(np.prod(C.pooled_shape(shape, block)))
        for mode in C.MODES:
            P = rsamp.Pooling(shape=shape, block_size=block, pooling_func=mode)
            assert P.output_shape == C.pooled_shape(shape, block)
            out[f'pool_{C.tag(shape, block)}_{mode}_fwd'] = P(C.make_vec(n, 0))
            out[f'pool_{C.tag(shape, block)}_{mode}_adj'] = P.adjoint(C.make_vec(m, 1))
    top_right = rsamp.Pooling(shape=(5, 7), block_size=(2, 3), pooling_func='mean')(np.arange(35.)).reshape(3, 3)[0, 2]
    assert abs(top_right - 19 / 6) < 1e-15, top_right          # (6 + 13) / 6: the full block size divides

    # ---- nearest neighbours with repeats
    NR = rsamp.NNSampling(samples=C.REPEAT_SAMPLES, grid=C.REPEAT_GRID)
    assert np.array_equal(NR.nn_indices, C.REPEAT_INDICES) and np.array_equal(NR.adjoint(C.REPEAT_Y), C.REPEAT_ADJOINT)
    out['nn_repeat_indices'], out['nn_repeat_adjoint'] = NR.nn_indices, NR.adjoint(C.REPEAT_Y)
    samples, grid = C.mesh_case()
    NM = rsamp.NNSampling(samples=samples, grid=grid)
    out['nn_mesh_indices'] = NM.nn_indices
    out['nn_mesh_adjoint'] = NM.adjoint(C.make_vec(300, 2))

    # ---- mapped distance matrices, stored as CSR arrays
    def put_csr(key, m):
        m = m.tocsr()
        m.sort_indices()
        out[f'{key}_indptr'], out[f'{key}_indices'], out[f'{key}_data'] = m.indptr, m.indices, m.data

    a, b, dmax = C.radial_case()
    put_csr('mdm_radial', rsamp.MappedDistanceMatrix(samples1=a, samples2=b, max_distance=dmax, operator_type='sparse',
                                                     **kw).mat)
    put_csr('mdm_radial_sym', rsamp.MappedDistanceMatrix(samples1=b, samples2=None, max_distance=dmax,
                                                         operator_type='sparse', **kw).mat)
    out['mdm_radial_dense'] = rsamp.MappedDistanceMatrix(samples1=a, samples2=b, operator_type='dense', **kw).mat
    out['mdm_radial_dense_ord1'] = rsamp.MappedDistanceMatrix(samples1=a, samples2=b, operator_type='dense', ord=1., **kw).mat
    a, b, dmax = C.zonal_case()
    zkw = dict(function=C.zonal_func, mode='zonal', verbose=0, n_jobs=1)
    put_csr('mdm_zonal', rsamp.MappedDistanceMatrix(samples1=a, samples2=b, max_distance=dmax, operator_type='sparse',
                                                    **zkw).mat)
    out['mdm_zonal_dense'] = rsamp.MappedDistanceMatrix(samples1=a, samples2=b, operator_type='dense', **zkw).mat

    # ---- (a) APGD LASSO with a sparse Gaussian MappedDistanceMatrix
    samples, knots, alpha0, noise = C.lasso_problem()
    Phi = rsamp.MappedDistanceMatrix(samples1=samples, samples2=knots, max_distance=3 * C.SIGMA, operator_type='sparse',
                                     **kw)
    Plip = float(np.linalg.norm(Phi.mat.toarray(), 2))
    Phi.lipschitz_cst = Phi.diff_lipschitz_cst = Plip
    y = Phi(alpha0) + noise
    F = (1 / 2) * loss.SquaredL2Loss(dim=y.size, data=y) * Phi
    lam = 0.1 * float(np.max(np.abs(F.gradient(0 * alpha0))))
    apgd = R.proxalgs.APGD(dim=alpha0.size, F=F, G=lam * pen.L1Norm(dim=alpha0.size), acceleration='CD', beta=Plip ** 2,
                           max_iter=C.LASSO_ITERS - 1, min_iter=C.LASSO_ITERS - 1, accuracy_threshold=0.0, verbose=None)
    est, _, diag = apgd.iterate()
    assert apgd.iter == C.LASSO_ITERS and np.all(np.isfinite(est['iterand'])) and np.count_nonzero(est['iterand']) > 0
    for k, val in dict(y=y, lip=Plip, lam=lam, beta=Plip ** 2, tau=apgd.tau, x=est['iterand'], past_aux=est['past_aux'],
                       n_iter=apgd.iter, diag=diag['Relative Improvement'].to_numpy(float)).items():
        out[f'lasso_{k}'] = np.asarray(val)
    print('sparse LASSO: ||Phi|| =', Plip, 'lam', lam, 'nonzeros', int(np.count_nonzero(est['iterand'])), 'nnz(Phi)',
          Phi.mat.nnz)

    # ---- (b) PDS: F = 1/2 ||y - P x||^2, K = sparse forward differences, H = lam ||.||_1
    shape, block = C.POOL_PDS_SHAPE, C.POOL_PDS_BLOCK
    N = int(np.prod(shape))
    yp = C.pool_pds_data()
    P = rsamp.Pooling(shape=shape, block_size=block, pooling_func='sum')
    Pd, _ = C.pool_matrices(shape, block, 'sum')
    assert np.array_equal(np.stack([P(e) for e in np.eye(N)], axis=1), Pd)
    P.lipschitz_cst = P.diff_lipschitz_cst = float(np.linalg.norm(Pd, 2))
    D = C.forward_difference_matrix(shape)
    K = lbase.SparseLinearOperator(D)
    K.lipschitz_cst = K.diff_lipschitz_cst = float(np.linalg.norm(D.toarray(), 2))
    pds = R.proxalgs.PDS(dim=N, F=(1 / 2) * loss.SquaredL2Loss(dim=yp.size, data=yp) * P,
                         H=C.POOL_PDS_LAM * pen.L1Norm(dim=2 * N), K=K, x0=np.zeros(N), z0=np.zeros(2 * N),
                         max_iter=C.POOL_PDS_ITERS - 1, min_iter=C.POOL_PDS_ITERS - 1, accuracy_threshold=0.0,
                         verbose=None)
    est, _, diag = pds.iterate()
    assert pds.iter == C.POOL_PDS_ITERS and np.all(np.isfinite(est['primal_variable']))
    assert np.all(np.isfinite(est['dual_variable']))
    for k, val in dict(Plip=P.lipschitz_cst, Klip=K.lipschitz_cst, x=est['primal_variable'], z=est['dual_variable'],
                       n_iter=pds.iter, tau=pds.tau, sigma=pds.sigma, rho=pds.rho,
                       diag_primal=diag['Relative Improvement (primal variable)'].to_numpy(float),
                       diag_dual=diag['Relative Improvement (dual variable)'].to_numpy(float)).items():
        out[f'pds_{k}'] = np.asarray(val)
    print('pooling PDS: ||P|| =', P.lipschitz_cst, '||K|| =', K.lipschitz_cst, 'last metric', out['pds_diag_primal'][-1])

    path = os.path.join(HERE, 'sparse_family.npz')
    np.savez_compressed(path, **out)
    print('sparse_family.npz', len(out), 'arrays,', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
