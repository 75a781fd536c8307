"""Golden fixtures for ``KroneckerProduct``, ``KroneckerSum`` and ``KhatriRaoProduct`` (``pycsou/linop/base.py:715-989``)
from the REAL reference code imported as in ``make_golden.py`` (same stand-in modules, nothing copied).

Build container only:  ``python tests/golden/make_golden_kron.py``  ->  ``tests/golden/kron_family.npz`` (arrays
only).  Inputs come from ``tests/kron_cases.py``, which the tests regenerate.

The stubbed ``pylops`` module is filled with ``FirstDerivative`` / ``SecondDerivative`` from ``oracle.pylops1``, as in
``make_golden_diff_family.py``; the reference's OWN ``KroneckerProduct``, ``KroneckerSum``, ``KhatriRaoProduct``,
``DenseLinearOperator``, ``SparseLinearOperator``, ``DiagonalOperator``, ``SecondDerivative`` and ``PDS`` produce the
vectors.  ``BlockOperator`` / ``BlockDiagonalOperator`` go through ``pylops.Block`` / ``pylops.BlockDiag``, which the
stand-ins do not have: no fixture for them (the tests use ``np.block``).

Asserted before saving: the doctests ``base.py:724-732`` (Kronecker product of two second derivatives against
``apply_along_axis``) and ``base.py:898-907`` (Khatri-Rao of two second derivatives, shape ``(121,)`` and the dense
formula, with ``todense().mat`` restated as the second-difference matrix of ``kron_cases``), the dense Khatri-Rao
branch's 2-D output shape, and finite iterates.  The sparse Khatri-Rao branch is broken under the installed SciPy
(forward: 0-d object array) and is not recorded.
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
    from tests import kron_cases as C
    R = import_reference()
    pylops = sys.modules['pylops']
    pylops.FirstDerivative = lambda N, dims=None, dir=0, sampling=1., edge=False, dtype='float64', kind='centered': \
        P.FirstDerivative(N, dims=dims, dir=dir, sampling=sampling, edge=edge, dtype=dtype, kind=kind)
    pylops.SecondDerivative = lambda N, dims=None, dir=0, sampling=1., edge=False, dtype='float64': \
        P.SecondDerivative(N, dims=dims, dir=dir, sampling=sampling, edge=edge, dtype=dtype)
    from pycsou.linop import diff as rdiff
    lbase, pen, loss = R.lbase, R.penalty, R.loss
    out = {}

    # ---- the doctests
    Nv, Nh = C.DOCTEST_NV, C.DOCTEST_NH
    D2h, D2v = rdiff.SecondDerivative(size=Nh), rdiff.SecondDerivative(size=Nv)
    Dkron = lbase.KroneckerProduct(D2h, D2v)
    x = np.zeros((Nv, Nh))
    x[Nv // 2, Nh // 2] = 1
    assert np.allclose(Dkron(x.flatten()), D2v.apply_along_axis(
        D2h.apply_along_axis(x.transpose(), axis=0).transpose(), axis=0).flatten())
    n = C.KR_DOCTEST_N
    D1, D2 = rdiff.SecondDerivative(size=n), rdiff.SecondDerivative(size=n)
    Dkrao = lbase.KhatriRaoProduct(D1, D2)
    xa = np.arange(n)
    M = C.d2_matrix(n)
    assert np.allclose(np.stack([D1(e) for e in np.eye(n)], axis=1), M)           # todense().mat
    assert Dkrao(xa).shape == (n * n,) and np.allclose(Dkrao(xa), ((M * xa[None, :]) @ M.transpose()).flatten())
    ya = C.make_vec(n * n, 9)
    out['kr_doctest_fwd'], out['kr_doctest_adj'] = np.asarray(Dkrao(xa), dtype=np.float64), Dkrao.adjoint(ya)
    assert out['kr_doctest_adj'].shape == (n,)

    # ---- Kronecker product and sum: forward and adjoint of every recorded pair
    for name in C.KRON_PAIRS:
        for tag, cls, square in (('kron', lbase.KroneckerProduct, False), ('ksum', lbase.KroneckerSum, True)):
            A, B = C.pair_matrices(name, square)
            op = cls(*C.build_pair(name, lbase, rdiff, square))
            xv, yv = C.pair_inputs(A, B)
            assert op.shape == (B.shape[0] * A.shape[0], B.shape[1] * A.shape[1])
            out[f'{tag}_{name}_fwd'], out[f'{tag}_{name}_adj'] = op(xv), op.adjoint(yv)

    # ---- Khatri-Rao, the dense pair with l = 7: the forward output is 2-D
    A, B = C.kr_dense_pair()
    op = lbase.KhatriRaoProduct(lbase.DenseLinearOperator(A), lbase.DenseLinearOperator(B))
    xv, yv = C.make_vec(A.shape[1], 0), C.make_vec(A.shape[0] * B.shape[0], 1)
    out['kr_dense_fwd'], out['kr_dense_adj'] = op(xv), op.adjoint(yv)
    assert out['kr_dense_fwd'].shape == (B.shape[0], A.shape[0]) and out['kr_dense_adj'].shape == (A.shape[1],)

    # ---- PDS: F = 1/2 ||y - (A_h (x) B_v) x||^2, K the sparse stacked forward differences, H = lam ||.||_1
    Ah, Bv, y = C.pds_problem()
    shape = C.PDS_SHAPE
    N = int(np.prod(shape))
    Alip, Blip = float(np.linalg.norm(Ah, 2)), float(np.linalg.norm(Bv, 2))
    opA, opB = lbase.DenseLinearOperator(Ah), lbase.DenseLinearOperator(Bv)
    opA.lipschitz_cst = opA.diff_lipschitz_cst = Alip
    opB.lipschitz_cst = opB.diff_lipschitz_cst = Blip
    G = lbase.KroneckerProduct(opA, opB)
    assert G.lipschitz_cst == Alip * Blip
    Dm = C.forward_difference_matrix(shape)
    K = lbase.SparseLinearOperator(Dm)
    Klip = float(np.linalg.norm(Dm.toarray(), 2))
    K.lipschitz_cst = K.diff_lipschitz_cst = Klip
    pds = R.proxalgs.PDS(dim=N, F=(1 / 2) * loss.SquaredL2Loss(dim=N, data=y) * G, H=C.PDS_LAM * pen.L1Norm(dim=2 * N),
                         K=K, x0=np.zeros(N), z0=np.zeros(2 * N), max_iter=C.PDS_ITERS - 1, min_iter=C.PDS_ITERS - 1,
                         accuracy_threshold=0.0, verbose=None)
    est, _, diag = pds.iterate()
    assert pds.iter == C.PDS_ITERS and np.all(np.isfinite(est['primal_variable']))
    for k, val in dict(Alip=Alip, Blip=Blip, Klip=Klip, x=est['primal_variable'], z=est['dual_variable'],
                       n_iter=pds.iter, tau=pds.tau, sigma=pds.sigma, rho=pds.rho,
                       diag_primal=diag['Relative Improvement (primal variable)'].to_numpy(float),
                       diag_dual=diag['Relative Improvement (dual variable)'].to_numpy(float)).items():
        out[f'pds_{k}'] = np.asarray(val)
    print('Kronecker PDS: ||G|| =', Alip * Blip, '||K|| =', Klip, 'last metric', out['pds_diag_primal'][-1])

    path = os.path.join(HERE, 'kron_family.npz')
    np.savez_compressed(path, **out)
    print('kron_family.npz', len(out), 'arrays,', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
