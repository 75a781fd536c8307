"""pcs_csr_spmm, the fused Khatri-Rao kernels pcs_khatri_rao_fwd / pcs_khatri_rao_adj, LinearOperator._apply_cols and
the operators on them (KroneckerProduct, KroneckerSum, KhatriRaoProduct, BlockOperator, BlockDiagonalOperator) on the
device, against SciPy, the NumPy definitions of tests/kron_cases.py and the reference's own outputs in
tests/golden/kron_family.npz (pycsou/linop/base.py:339-548, 715-989).

Tolerances are those of tests/test_gpu_ops.py and tests/test_gpu_sparse.py: rel-L2 1e-12 (fp64) and 2e-6 (fp32)
against fp64 references.  fp32 cases with ordinary data keep every summed length <= 4099 terms; longer sums carry
integers in {-3..3} against weights in {+-1, +-0.5}, so every partial sum is exact in both dtypes in any order, and
are compared with array_equal -- the cases that catch a wrong lane, slab, chunk or carry."""

import functools

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import torch

from tests import kron_cases as C
from tests import sparse_cases as SC
from tests.cases import load, rel

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-12, np.float32: 2e-6}
DTYPES = [np.float64, np.float32]


@functools.lru_cache(maxsize=None)
def golden():
    return load('kron_family.npz')


def dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return t.cpu().numpy()


def dot_gap(op, seed=5):
    """|<A x, y> - <x, A^T y>| / (||x|| ||y||) with every product on the device in fp64."""
    rng = np.random.default_rng(seed)
    x, y = dev(rng.standard_normal(op.shape[1])), dev(rng.standard_normal(op.shape[0]))
    gap = torch.abs(torch.dot(op._apply(x).reshape(-1), y) - torch.dot(x, op._adj(y).reshape(-1)))
    return float(gap / (torch.linalg.vector_norm(x) * torch.linalg.vector_norm(y)))


@functools.lru_cache(maxsize=None)
def mixed_matrix():
    """Row lengths 0, 1, 2, 63, 64, 65, 257 and 4099 (the last one a long row of two chunks) in one matrix."""
    return SC.csr_from_lengths([0, 1, 2, 63, 64, 65, 257, 4099], 5000, 2)


# ---------------------------------------------------------------- pcs_csr_spmm
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nb', [1, 2, 63, 64, 65, 130])
def test_spmm_axis0(nb, dtype):
    from pycsou_amd import _ops as O
    A = mixed_matrix()
    D = O.DeviceCSR(A, O.torch_dtype(dtype))
    X = C.make_vec(A.shape[1] * nb, 0).reshape(A.shape[1], nb)
    ref = A @ X
    got = O.spmm(D, dev(X, dtype), 0)
    assert got.shape == (A.shape[0], nb) and got.is_contiguous() and not host(got)[0].any()
    assert rel(host(got), ref) < TOL[dtype]
    assert torch.equal(got, O.spmm(D, dev(X, dtype), 0))                              # same bits twice
    start = C.make_vec(A.shape[0] * nb, 1).reshape(A.shape[0], nb).astype(dtype)
    acc = [O.spmm(D, dev(X, dtype), 0, out=dev(start, dtype), accumulate=True) for _ in range(2)]
    assert rel(host(acc[0]), ref + start.astype(np.float64)) < TOL[dtype] and torch.equal(acc[0], acc[1])
    if nb == 1:
        assert torch.equal(got.reshape(-1), O.spmv(D, dev(X.ravel(), dtype)))         # the bits of pcs_csr_spmv


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nb', [1, 3, 65])
def test_spmm_axis1(nb, dtype):
    from pycsou_amd import _ops as O
    A = mixed_matrix()
    D = O.DeviceCSR(A, O.torch_dtype(dtype))
    X = C.make_vec(nb * A.shape[1], 2).reshape(nb, A.shape[1])
    ref = (A @ X.T).T
    Xd = dev(X, dtype)
    got = O.spmm(D, Xd, 1)
    assert got.shape == (nb, A.shape[0]) and got.is_contiguous() and rel(host(got), ref) < TOL[dtype]
    assert torch.equal(got, O.spmm(D, Xd, 1))
    for b in range(nb):                                                               # every batch row: pcs_csr_spmv's bits
        assert torch.equal(got[b], O.spmv(D, Xd[b])), b
    start = C.make_vec(nb * A.shape[0], 3).reshape(nb, A.shape[0]).astype(dtype)
    acc = O.spmm(D, Xd, 1, out=dev(start, dtype), accumulate=True)
    assert rel(host(acc), ref + start.astype(np.float64)) < TOL[dtype]
    with pytest.raises(ValueError):
        O.spmm(D, Xd[:, :-1].contiguous(), 1)
    with pytest.raises(ValueError):
        O.spmm(D, Xd, 1, accumulate=True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_spmm_long_rows_exact(dtype):
    """A three-chunk row between short ones, and the transpose of a tall thin matrix (three rows of about 47000
    entries) with a batch: integer data, every sum exact, both layouts."""
    from pycsou_amd import _ops as O
    K = O.SPMV_CHUNK
    A = SC.csr_from_lengths([3, 2 * K + 1, 0, 70], 3 * K, 4, exact=True)
    D = O.DeviceCSR(A, O.torch_dtype(dtype))
    assert D.nchunks == 3 and D.nlong == 1
    for nb in (1, 3):
        X1 = C.make_ints(nb * A.shape[1], 0).reshape(nb, A.shape[1])
        out = torch.full((nb, A.shape[0]), float('nan'), dtype=O.torch_dtype(dtype), device='cuda')
        assert np.array_equal(host(O.spmm(D, dev(X1, dtype), 1, out=out)), (A @ X1.T).T), nb
        X0 = np.ascontiguousarray(X1.T)
        out = torch.full((A.shape[0], nb), float('nan'), dtype=O.torch_dtype(dtype), device='cuda')
        assert np.array_equal(host(O.spmm(D, dev(X0, dtype), 0, out=out)), A @ X0), nb
    start = C.make_ints(3 * A.shape[0], 5).reshape(3, A.shape[0])
    got = O.spmm(D, dev(X1, dtype), 1, out=dev(start, dtype), accumulate=True)
    assert np.array_equal(host(got), (A @ X1.T).T + start)
    rng = np.random.default_rng(7)
    dense = rng.choice([0.0, 1.0, -1.0, 0.5, -0.5], size=(70001, 3), p=[1 / 3, 1 / 6, 1 / 6, 1 / 6, 1 / 6])
    Dt = O.DeviceCSR(sp.csr_matrix(dense).T.tocsr(), O.torch_dtype(dtype))
    assert Dt.nlong == 3
    Y = C.make_ints(3 * 70001, 1).reshape(3, 70001)
    got = O.spmm(Dt, dev(Y, dtype), 1)
    assert np.array_equal(host(got), Y @ dense) and torch.equal(got[2], O.spmv(Dt, dev(Y[2], dtype)))


# ---------------------------------------------------------------- the fused Khatri-Rao kernels
def _kr_ops(A, B):
    from pycsou_amd.linop import DenseLinearOperator, KhatriRaoProduct
    return KhatriRaoProduct(DenseLinearOperator(A), DenseLinearOperator(B))


def _kr_kernels(A, B, x, y, dtype):
    """The two fused kernels themselves (whatever route the operator takes), each run twice: same bits."""
    from pycsou_amd import _ops as O
    (k, l), n = A.shape, B.shape[0]
    Ad, Bd = dev(A, dtype), dev(B, dtype)
    ws = torch.full((O.kr_fwd_plan(k, n, l)[2],), float('nan'), dtype=torch.float64, device='cuda')
    fwd = [O.khatri_rao_fwd(Ad, Bd, dev(x, dtype), ws) for _ in range(2)]
    adj = [O.khatri_rao_adj(Ad, Bd, dev(y, dtype)) for _ in range(2)]
    assert fwd[0].shape == (n, k) and adj[0].shape == (l,)
    assert torch.equal(fwd[0], fwd[1]) and torch.equal(adj[0], adj[1])
    return host(fwd[0]), host(adj[0])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('knl', C.KR_FUSED, ids=['x'.join(map(str, s)) for s in C.KR_FUSED])
def test_khatri_rao_fused(knl, dtype):
    k, n, l = knl
    A, B = C.dense((k, l), 10), C.dense((n, l), 11)
    x, y = C.make_vec(l, 0), C.make_vec(n * k, 1)
    op = _kr_ops(A, B)
    assert op._route(dtype) == 'fused' and op._route(dtype, adjoint=True) in ('fused', 'torch')
    M = C.khatri_rao_matrix(A, B)
    for fwd, adj in (_kr_kernels(A, B, x, y, dtype), (op(x.astype(dtype)), op.adjoint(y.astype(dtype)))):
        assert fwd.shape == (n, k) and adj.shape == (l,) and fwd.dtype == dtype and adj.dtype == dtype
        assert rel(fwd.ravel(), M @ x) < TOL[dtype] and rel(adj, M.T @ y) < TOL[dtype]
    assert np.array_equal(fwd, op(x.astype(dtype))) and np.array_equal(adj, op.adjoint(y.astype(dtype)))
    if dtype == np.float64:
        assert dot_gap(op) <= 1e-12
        rng = np.random.default_rng(5)                       # and of the kernel pair itself
        u, v = rng.standard_normal(l), rng.standard_normal(n * k)
        f, a = _kr_kernels(A, B, u, v, dtype)
        assert abs(np.dot(f.ravel(), v) - np.dot(u, a)) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(v)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('knl', [C.KR_SLABS, (3, 2, 64 * 513 + 3)], ids=['slabs', 'two_slabs_per_group'])
def test_khatri_rao_fused_across_slabs_exact(knl, dtype):
    """l over several column slabs, and over more slabs than workgroups (two per group): integer data."""
    from pycsou_amd import _ops as O
    k, n, l = knl
    spg, ngroups, _ = O.kr_fwd_plan(k, n, l)
    assert (spg, ngroups) == ((1, 8) if l < 1000 else (2, 257))
    A, B = C.make_int_matrix((k, l), 0), C.make_int_matrix((n, l), 1)
    x, y = C.make_ints(l, 2), C.make_ints(n * k, 3)
    fwd, adj = _kr_kernels(A, B, x, y, dtype)
    assert fwd.dtype == dtype and np.array_equal(fwd, (B * x[None, :]) @ A.T)
    assert adj.dtype == dtype and np.array_equal(adj, np.sum((y.reshape(n, k) @ A) * B, axis=0))


@pytest.mark.parametrize('dtype', DTYPES)
def test_khatri_rao_above_the_fused_limit_composes(dtype):
    k, n, l = C.KR_ABOVE
    A, B = C.dense((k, l), 12), C.dense((n, l), 13)
    x, y = C.make_vec(l, 0), C.make_vec(n * k, 1)
    op = _kr_ops(A, B)
    assert op._route(dtype) == 'torch' == op._route(dtype, adjoint=True)
    M = C.khatri_rao_matrix(A, B)
    fwd, adj = op(x.astype(dtype)), op.adjoint(y.astype(dtype))
    assert fwd.shape == (n, k) and adj.shape == (l,)
    assert rel(fwd.ravel(), M @ x) < TOL[dtype] and rel(adj, M.T @ y) < TOL[dtype]
    if dtype == np.float64:
        assert dot_gap(op) <= 1e-12


# ---------------------------------------------------------------- factors of every kind
def factor(kind, shape, seed):
    """(operator, dense matrix) of one factor; the square kinds use shape[1]."""
    from pycsou_amd import linop as L
    n = shape[1]
    if kind == 'dense':
        M = C.dense(shape, seed)
        return L.DenseLinearOperator(M), M
    if kind == 'sparse':
        M = C.sparse(shape, seed)
        return L.SparseLinearOperator(M), M.toarray()
    if kind == 'd2':
        return L.SecondDerivative(size=n), C.d2_matrix(n)
    if kind == 'd1':
        return L.FirstDerivative(size=n, kind='forward', step=0.5), C.d1_matrix(n, 0.5)
    if kind == 'conv':
        op = L.Convolve1D(size=n, filter=np.array([0.25, 0.5, 1.0, -0.5, 0.125]))
        return op, np.stack([op(e) for e in np.eye(n)], axis=1)         # the 1-D operator's own columns
    if kind == 'diag':
        d = C.diag_values(n, seed)
        return L.DiagonalOperator(d), np.diag(d)
    if kind == 'identity':
        return L.IdentityOperator(n), np.eye(n)
    if kind == 'homothety':
        return L.HomothetyMap(n, -1.5), -1.5 * np.eye(n)
    if kind == 'null':
        return L.NullOperator((shape[0], n)), np.zeros((shape[0], n))
    raise KeyError(kind)


def wrapped(kind, n, seed):
    """The algebra wrappers over square factors: (operator, dense matrix)."""
    from pycsou_amd import linop as L
    from pycsou_amd.core.linop import SymmetricLinearOperator
    a, Ma = factor('dense', (n, n), seed)
    s, Ms = factor('sparse', (n, n), seed + 1)
    if kind == 'adjoint':
        return s.H, Ms.T
    if kind == 'transpose':
        return a.T, Ma.T
    if kind == 'sum':
        return a + s, Ma + Ms
    if kind == 'sum_identity':
        return L.IdentityOperator(n) + s, np.eye(n) + Ms
    if kind == 'comp':
        return s * a, Ms @ Ma
    if kind == 'symmetric':
        return SymmetricLinearOperator(a.H * a), Ma.T @ Ma
    if kind == 'poly':
        return L.PolynomialLinearOperator(s, [0.5, -1.0, 0.25]), 0.5 * np.eye(n) - Ms + 0.25 * Ms @ Ms
    if kind == 'kron':
        (p, Mp), (q, Mq) = factor('d1', (3, 3), 0), factor('sparse', (n // 3, n // 3), seed)
        return L.KroneckerProduct(p, q), C.kron_matrix(Mp, Mq)
    if kind == 'ksum':
        (p, Mp), (q, Mq) = factor('dense', (3, 3), seed), factor('sparse', (n // 3, n // 3), seed)
        return L.KroneckerSum(p, q), C.ksum_matrix(Mp, Mq)
    if kind in ('khatri_rao_sparse', 'khatri_rao_dense'):
        which = 'sparse' if kind.endswith('sparse') else 'dense'
        (p, Mp), (q, Mq) = factor(which, (4, n), seed), factor(which, (3, n), seed + 1)
        return L.KhatriRaoProduct(p, q), C.khatri_rao_matrix(Mp, Mq)
    raise KeyError(kind)


# ---------------------------------------------------------------- _apply_cols: every override equals the column loop
BITWISE = {'sparse': (1,), 'd1': (0, 1), 'd2': (0, 1), 'identity': (0, 1), 'homothety': (0, 1), 'null': (0, 1)}
FACTORS = ['dense', 'sparse', 'd1', 'd2', 'conv', 'diag', 'identity', 'homothety', 'null']
WRAPPERS = ['adjoint', 'transpose', 'sum', 'sum_identity', 'comp', 'symmetric', 'poly', 'kron', 'ksum', 'khatri_rao_sparse',
            'khatri_rao_dense']


def _check_cols(op, M, other, dtype, bitwise=()):
    from pycsou_amd.core.linop import LinearOperator
    for adjoint in (False, True):
        Md = M.T if adjoint else M
        for axis in (0, 1):
            shape = (Md.shape[1], other) if axis == 0 else (other, Md.shape[1])
            T = C.make_vec(shape[0] * shape[1], axis).reshape(shape)
            ref = Md @ T if axis == 0 else T @ Md.T
            Td = dev(T, dtype)
            got = op._apply_cols(Td, axis, adjoint)
            loop = LinearOperator._apply_cols(op, Td, axis, adjoint)
            assert got.shape == ref.shape == loop.shape and got.is_contiguous() and loop.is_contiguous()
            assert torch.equal(Td, dev(T, dtype))                                    # the input is left alone
            if not M.any():
                assert not host(got).any() and not host(loop).any()
                continue
            assert rel(host(loop), ref) < TOL[dtype] and rel(host(got), ref) < TOL[dtype], (adjoint, axis)
            assert rel(host(got), host(loop)) < TOL[dtype], (adjoint, axis)
            if axis in bitwise:
                assert torch.equal(got, loop), (adjoint, axis)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', FACTORS)
def test_apply_cols_of_factors_equals_the_column_loop(kind, dtype):
    """A (7 x 9) array: the operator acts on the 7 (axis 0) or the 9 (axis 1); the other length is 9 or 7."""
    for axis_len, other in ((7, 9), (9, 7)):
        op, M = factor(kind, (5, axis_len), 3)
        _check_cols(op, M, other, dtype, BITWISE.get(kind, ()))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['d1', 'd2', 'conv'])
def test_apply_cols_of_stencils_64_by_65(kind, dtype):
    for axis_len, other in ((64, 65), (65, 64)):
        op, M = factor(kind, (axis_len, axis_len), 3)
        _check_cols(op, M, other, dtype, BITWISE.get(kind, ()))


def test_apply_cols_of_nd_stencils_keeps_the_column_loop():
    from pycsou_amd import linop as L
    op = L.SecondDerivative(size=12, shape=(3, 4), axis=1)
    M = np.kron(np.eye(3), C.d2_matrix(4))
    _check_cols(op, M, 5, np.float64, (0, 1))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', WRAPPERS)
def test_apply_cols_of_wrappers_equals_the_column_loop(kind, dtype):
    op, M = wrapped(kind, 12, 4)
    _check_cols(op, M, 7, dtype)


# ---------------------------------------------------------------- the operators
def _check_operator(op, M, dtype, two_d=None):
    x, y = C.make_vec(M.shape[1], 0), C.make_vec(M.shape[0], 1)
    fwd, adj = op(x.astype(dtype)), op.adjoint(y.astype(dtype))
    assert fwd.dtype == dtype and adj.dtype == dtype and adj.shape == (M.shape[1],)
    assert fwd.shape == ((M.shape[0],) if two_d is None else two_d)
    if M.any():
        assert rel(fwd.ravel(), M @ x) < TOL[dtype] and rel(adj, M.T @ y) < TOL[dtype]
    else:
        assert not fwd.any() and not adj.any()
    assert np.array_equal(fwd, op(x.astype(dtype))) and np.array_equal(adj, op.adjoint(y.astype(dtype)))
    if dtype == np.float64:
        assert dot_gap(op) <= 1e-12


KRON_PAIRINGS = [('dense', 'dense'), ('sparse', 'sparse'), ('d2', 'd2'), ('diag', 'dense'), ('dense', 'sparse'),
                 ('sparse', 'd1'), ('conv', 'diag'), ('identity', 'sparse'), ('homothety', 'dense'), ('d1', 'null')]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('pair', KRON_PAIRINGS, ids=['_'.join(p) for p in KRON_PAIRINGS])
def test_kronecker_product_against_definition(pair, dtype):
    from pycsou_amd.linop import KroneckerProduct
    (a, Ma), (b, Mb) = factor(pair[0], (5, 7), 0), factor(pair[1], (4, 6), 1)
    _check_operator(KroneckerProduct(a, b), C.kron_matrix(Ma, Mb), dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('pair', KRON_PAIRINGS, ids=['_'.join(p) for p in KRON_PAIRINGS])
def test_kronecker_sum_against_definition(pair, dtype):
    from pycsou_amd.linop import KroneckerSum
    (a, Ma), (b, Mb) = factor(pair[0], (7, 7), 0), factor(pair[1], (6, 6), 1)
    _check_operator(KroneckerSum(a, b), C.ksum_matrix(Ma, Mb), dtype)


KR_PAIRINGS = [('dense', 'dense'), ('sparse', 'sparse'), ('d2', 'd2'), ('diag', 'dense'), ('dense', 'sparse'),
               ('sparse', 'd1'), ('conv', 'dense'), ('identity', 'sparse')]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('pair', KR_PAIRINGS, ids=['_'.join(p) for p in KR_PAIRINGS])
def test_khatri_rao_against_definition(pair, dtype):
    from pycsou_amd.linop import KhatriRaoProduct
    (a, Ma), (b, Mb) = factor(pair[0], (5, 11), 0), factor(pair[1], (4, 11), 1)
    op = KhatriRaoProduct(a, b)
    assert op._route() == {('dense', 'dense'): 'fused', ('sparse', 'sparse'): 'csr'}.get(pair, 'generic')
    two_d = (Mb.shape[0], Ma.shape[0]) if op._route() in ('fused', 'csr') else None   # the explicit pairs: (n, k)
    _check_operator(op, C.khatri_rao_matrix(Ma, Mb), dtype, two_d)


def test_operators_match_the_reference_fixture():
    import pycsou_amd.linop.base as B
    import pycsou_amd.linop.diff as D
    g = golden()
    for name in C.KRON_PAIRS:
        for tag, cls, square in (('kron', B.KroneckerProduct, False), ('ksum', B.KroneckerSum, True)):
            Am, Bm = C.pair_matrices(name, square)
            op = cls(*C.build_pair(name, B, D, square))
            x, y = C.pair_inputs(Am, Bm)
            assert rel(op(x), g[f'{tag}_{name}_fwd']) < 1e-12 and rel(op.adjoint(y), g[f'{tag}_{name}_adj']) < 1e-12, (tag, name)
    Am, Bm = C.kr_dense_pair()
    op = B.KhatriRaoProduct(B.DenseLinearOperator(Am), B.DenseLinearOperator(Bm))
    fwd, adj = op(C.make_vec(7, 0)), op.adjoint(C.make_vec(20, 1))
    assert fwd.shape == g['kr_dense_fwd'].shape == (4, 5) and rel(fwd, g['kr_dense_fwd']) < 1e-12
    assert adj.shape == (7,) and rel(adj, g['kr_dense_adj']) < 1e-12
    n = C.KR_DOCTEST_N
    Dk = B.KhatriRaoProduct(D.SecondDerivative(size=n), D.SecondDerivative(size=n))
    x = np.arange(n)
    assert Dk(x).shape == (n * n,) and rel(Dk(x), g['kr_doctest_fwd']) < 1e-12
    assert np.allclose(Dk(x), ((C.d2_matrix(n) * x[None, :]) @ C.d2_matrix(n).T).flatten())       # base.py:903-907
    assert rel(Dk.adjoint(C.make_vec(n * n, 9)), g['kr_doctest_adj']) < 1e-12
    Nv, Nh = C.DOCTEST_NV, C.DOCTEST_NH                                                            # base.py:724-732
    Dkron = B.KroneckerProduct(D.SecondDerivative(size=Nh), D.SecondDerivative(size=Nv))
    img = np.zeros((Nv, Nh))
    img[Nv // 2, Nh // 2] = 1
    assert np.allclose(Dkron(img.flatten()), (C.d2_matrix(Nv) @ img @ C.d2_matrix(Nh).T).flatten())


def test_kronecker_product_lipschitz_constant():
    from pycsou_amd.linop import KroneckerProduct
    for pair in (('dense', 'sparse'), ('d2', 'dense'), ('sparse', 'd1')):
        (a, Ma), (b, Mb) = factor(pair[0], (5, 7), 0), factor(pair[1], (4, 6), 1)
        K = KroneckerProduct(a, b)
        K.compute_lipschitz_cst()
        exact = np.linalg.norm(C.kron_matrix(Ma, Mb), 2)
        assert abs(K.lipschitz_cst - exact) <= 1e-8 * exact and K.diff_lipschitz_cst == K.lipschitz_cst, pair


@pytest.mark.parametrize('dtype', DTYPES)
def test_block_operators_against_np_block(dtype):
    import pycsou_amd.linop.base as B
    import pycsou_amd.linop.diff as D
    ops, mats = C.block_layout(D)
    _check_operator(B.BlockOperator(ops), np.block(mats), dtype)
    Nv, Nh = C.DOCTEST_NV, C.DOCTEST_NH
    if dtype == np.float64:                                                                         # base.py:365-371
        Dblock = B.BlockOperator(ops)
        img = np.zeros((Nv, Nh))
        img[Nv // 2, Nh // 2] = 1
        z = np.tile(img, (3, 1)).flatten()
        D2v, D2h = ops[0][0], ops[1][0]
        assert np.allclose(Dblock(z), np.concatenate(((D2v + 0.5 * D2v + -1 * D2h)(img.flatten()),
                                                      (D2h + 2 * D2h + D2v)(img.flatten()))))
    diag_ops, diag_mats = [ops[0][0], ops[0][1], ops[0][2]], [mats[0][0], mats[0][1], mats[0][2]]    # base.py:996-999
    _check_operator(B.BlockDiagonalOperator(*diag_ops), scipy.linalg.block_diag(*diag_mats), dtype)
    (a, Ma), (b, Mb), (c, Mc) = factor('dense', (3, 4), 0), factor('sparse', (5, 4), 1), factor('d1', (6, 6), 2)
    Dg = B.BlockDiagonalOperator(a, b, c)
    _check_operator(Dg, scipy.linalg.block_diag(Ma, Mb, Mc), dtype)
    if dtype == np.float64:
        Dg.compute_lipschitz_cst()
        exact = max(np.linalg.norm(m, 2) for m in (Ma, Mb, Mc))
        assert abs(Dg.lipschitz_cst - exact) <= 1e-8 * exact


# ---------------------------------------------------------------- solvers through the generic path
def _kron_pds():
    from pycsou_amd.func import L1Norm
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.linop import DenseLinearOperator, KroneckerProduct, SparseLinearOperator
    from pycsou_amd.opt import PDS
    g = golden()
    Ah, Bv, y = C.pds_problem()
    N = y.size
    a, b = DenseLinearOperator(Ah), DenseLinearOperator(Bv)
    a.lipschitz_cst = a.diff_lipschitz_cst = float(g['pds_Alip'])
    b.lipschitz_cst = b.diff_lipschitz_cst = float(g['pds_Blip'])
    G = KroneckerProduct(a, b)
    assert G.lipschitz_cst == float(g['pds_Alip']) * float(g['pds_Blip'])
    K = SparseLinearOperator(C.forward_difference_matrix(C.PDS_SHAPE))
    K.lipschitz_cst = K.diff_lipschitz_cst = float(g['pds_Klip'])
    return PDS(dim=N, F=(1 / 2) * SquaredL2Loss(dim=N, data=y) * G, H=C.PDS_LAM * L1Norm(dim=2 * N), K=K,
               x0=np.zeros(N), z0=np.zeros(2 * N), max_iter=C.PDS_ITERS - 1, min_iter=C.PDS_ITERS - 1,
               accuracy_threshold=0.0, verbose=None, engine='generic')


def test_kronecker_pds_matches_reference():
    """F = 1/2 ||y - (A_h (x) B_v) x||^2 on a 24 x 30 image, K the sparse stacked forward differences, H = lam ||.||_1."""
    g = golden()
    pds = _kron_pds()
    assert (pds.tau, pds.sigma, pds.rho) == pytest.approx((float(g['pds_tau']), float(g['pds_sigma']), float(g['pds_rho'])),
                                                          rel=1e-14)
    est, _, diag = pds.iterate()
    assert pds._engine is None and pds.iter == int(g['pds_n_iter']) == C.PDS_ITERS
    e_x, e_z = rel(est['primal_variable'], g['pds_x']), rel(est['dual_variable'], g['pds_z'])
    print('Kronecker PDS fp64: rel x', e_x, 'rel z', e_z)
    assert e_x < 1e-9 and e_z < 1e-9
    np.testing.assert_allclose(diag['Relative Improvement (primal variable)'].to_numpy(float)[1:],
                               g['pds_diag_primal'][1:], rtol=1e-6)
    np.testing.assert_allclose(diag['Relative Improvement (dual variable)'].to_numpy(float)[1:],
                               g['pds_diag_dual'][1:], rtol=1e-6)


def test_kronecker_pds_graph_bitwise_eager(monkeypatch):
    """The captured loop returns the eager loop's bits."""
    runs = []
    for graph in ('1', '0'):
        monkeypatch.setenv('PCS_GENERIC_GRAPH', graph)
        pds = _kron_pds()
        est, _, diag = pds.iterate()
        runs.append((pds, est, diag))
    (pg, eg, dg), (pe, ee, de) = runs
    assert getattr(pg, '_graph_used', False) and not getattr(pe, '_graph_used', False)
    assert pg.iter == pe.iter
    for k in ('primal_variable', 'dual_variable'):
        assert np.array_equal(eg[k], ee[k]), k
    for c in dg.columns:
        np.testing.assert_array_equal(dg[c].to_numpy(float), de[c].to_numpy(float))


@pytest.mark.parametrize('which', ['ksum', 'khatri_rao', 'block', 'block_diag'])
def test_other_operators_under_graph_capture(which, monkeypatch):
    """Each of the other four as K of a small PDS: the captured generic loop is used and returns the eager bits."""
    from pycsou_amd.func import L1Norm
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd import linop as L
    from pycsou_amd.opt import PDS

    def build():
        (a, Ma), (s, Ms) = factor('dense', (6, 6), 0), factor('sparse', (5, 5), 1)
        if which == 'ksum':
            K, M = L.KroneckerSum(a, s), C.ksum_matrix(Ma, Ms)
        elif which == 'khatri_rao':
            (p, Mp), (q, Mq) = factor('dense', (5, 30), 2), factor('dense', (4, 30), 3)
            K, M = L.KhatriRaoProduct(p, q), C.khatri_rao_matrix(Mp, Mq)
        elif which == 'block':
            K, M = L.BlockOperator([[a, L.IdentityOperator(6)], [L.NullOperator((5, 6)), factor('sparse', (5, 6), 4)[0]]]), None
        else:
            K, M = L.BlockDiagonalOperator(a, s), None
        K.lipschitz_cst = K.diff_lipschitz_cst = 10.0 if M is None else float(np.linalg.norm(M, 2))
        n = K.shape[1]
        return PDS(dim=n, F=(1 / 2) * SquaredL2Loss(dim=n, data=C.make_vec(n, 6)), H=0.1 * L1Norm(dim=K.shape[0]), K=K,
                   x0=np.zeros(n), z0=np.zeros(K.shape[0]), max_iter=11, min_iter=11, accuracy_threshold=0.0,
                   verbose=None, engine='generic')

    runs = []
    for graph in ('1', '0'):
        monkeypatch.setenv('PCS_GENERIC_GRAPH', graph)
        pds = build()
        est, _, _ = pds.iterate()
        runs.append((pds, est))
    (pg, eg), (pe, ee) = runs
    assert getattr(pg, '_graph_used', False) and not getattr(pe, '_graph_used', False) and pg.iter == pe.iter
    for k in ('primal_variable', 'dual_variable'):
        assert np.all(np.isfinite(eg[k])) and np.array_equal(eg[k], ee[k]), k
