"""CPU tier of KroneckerProduct, KroneckerSum, KhatriRaoProduct, BlockOperator and BlockDiagonalOperator
(pycsou/linop/base.py:339-548, 715-989): names, shapes, dtypes, Lipschitz constants and errors as in the reference,
the new C-ABI entry points and their argument checks (they run before any device call), the launch and workspace
plans of pcs_csr_spmm and pcs_khatri_rao_fwd, the host CSR assembly of the sparse Khatri-Rao matrix, and the
fixture against the NumPy definitions of tests/kron_cases.py.  No compute calls (no GPU here)."""

import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import kron_cases as C
from tests.cases import GOLDEN, load

NAMES = ('KroneckerProduct', 'KroneckerSum', 'KhatriRaoProduct', 'BlockOperator', 'BlockDiagonalOperator')
NEW_SYMBOLS = ('pcs_csr_spmm', 'pcs_khatri_rao_fwd', 'pcs_khatri_rao_adj')


def test_reference_names_import():
    import importlib
    for mod in ('pycsou_amd.linop.base', 'pycsou_amd.linop'):
        m = importlib.import_module(mod)
        for name in NAMES:
            assert callable(getattr(m, name)), (mod, name)
    import pycsou_amd.linop.base as B
    assert 'out of scope' not in B.__doc__


def test_reference_names_import_under_alias():
    import pycsou_amd
    saved = {k: v for k, v in sys.modules.items() if k == 'pycsou' or k.startswith('pycsou.')}
    try:
        pycsou_amd.install_alias('pycsou')
        from pycsou.linop.base import (BlockDiagonalOperator, BlockOperator, KhatriRaoProduct,  # noqa: F401
                                       KroneckerProduct, KroneckerSum)
        from pycsou.linop import KroneckerProduct as K2
        import pycsou_amd.linop.base as B
        assert K2 is KroneckerProduct is B.KroneckerProduct and KhatriRaoProduct is pycsou_amd.linop.KhatriRaoProduct
    finally:
        for k in [k for k in sys.modules if k == 'pycsou' or k.startswith('pycsou.')]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---------------------------------------------------------------- constructors, attributes, errors
def _ops():
    import pycsou_amd.linop.base as B
    import pycsou_amd.linop.diff as D
    return B, D


def test_kronecker_product_attributes():
    from pycsou_amd.core.linop import LinearOperator
    B, D = _ops()
    for name in C.KRON_PAIRS:
        Am, Bm = C.pair_matrices(name)
        a, b = C.build_pair(name, B, D)
        K = B.KroneckerProduct(a, b)
        assert isinstance(K, LinearOperator) and K.linop1 is a and K.linop2 is b
        assert K.shape == (Bm.shape[0] * Am.shape[0], Bm.shape[1] * Am.shape[1]) and K.dtype == a.dtype
    a, b = B.DenseLinearOperator(C.dense((5, 7), 0).astype(np.float32)), B.DenseLinearOperator(C.dense((4, 3), 1))
    K = B.KroneckerProduct(a, b)
    assert K.dtype == np.float32 and K.lipschitz_cst == np.inf and K.shape == (20, 21)
    a.lipschitz_cst, b.lipschitz_cst = 2.0, 3.5
    assert B.KroneckerProduct(a, b).lipschitz_cst == 7.0 == B.KroneckerProduct(a, b).diff_lipschitz_cst
    assert B.KroneckerProduct(B.NullOperator((3, 3)), b).lipschitz_cst == 0          # 0 * finite
    assert B.KroneckerProduct(B.NullOperator((3, 3)), B.DenseLinearOperator(np.eye(2))).lipschitz_cst == np.inf


def test_kronecker_product_lipschitz_is_the_product_of_exact_norms():
    """compute_lipschitz_cst fills in the factors' constants (closed forms for the stencils: no device call) and
    multiplies them: ||A (x) B|| = ||A|| ||B||."""
    B, D = _ops()
    a, b = D.SecondDerivative(size=C.DOCTEST_NH), D.SecondDerivative(size=C.DOCTEST_NV)
    K = B.KroneckerProduct(a, b)
    assert K.lipschitz_cst == np.inf
    K.compute_lipschitz_cst()
    exact = np.linalg.norm(C.kron_matrix(C.d2_matrix(C.DOCTEST_NH), C.d2_matrix(C.DOCTEST_NV)), 2)
    assert abs(K.lipschitz_cst - exact) <= 1e-12 * exact and K.diff_lipschitz_cst == K.lipschitz_cst
    assert a.lipschitz_cst != np.inf and b.lipschitz_cst != np.inf
    a.lipschitz_cst = 100.0                                   # a constant that is already there is kept
    K.compute_lipschitz_cst()
    assert K.lipschitz_cst == 100.0 * b.lipschitz_cst


def test_kronecker_sum_attributes_and_errors():
    B, D = _ops()
    a, b = B.DenseLinearOperator(np.eye(5)), B.DenseLinearOperator(np.eye(4))
    a.lipschitz_cst, b.lipschitz_cst = 1.0, 2.0
    S = B.KroneckerSum(a, b)
    assert S.shape == (20, 20) and S.lipschitz_cst == 3.0 and S.dtype == np.float64
    assert B.KroneckerSum(D.SecondDerivative(size=21), D.SecondDerivative(size=11)).lipschitz_cst == np.inf
    for bad in ((B.DenseLinearOperator(np.ones((5, 7))), b), (a, B.DenseLinearOperator(np.ones((4, 3)))),
                (B.DenseLinearOperator(np.ones((4, 5))), B.DenseLinearOperator(np.ones((5, 4))))):
        with pytest.raises(ValueError):
            B.KroneckerSum(*bad)


def test_khatri_rao_attributes_routes_and_errors():
    from pycsou_amd import _ops as O
    B, D = _ops()
    Am, Bm = C.kr_dense_pair()
    a, b = B.DenseLinearOperator(Am), B.DenseLinearOperator(Bm)
    K = B.KhatriRaoProduct(a, b)
    assert K.shape == (20, 7) and K.dtype == np.float64 and K.lipschitz_cst == np.inf and K._route() == 'fused'
    a.lipschitz_cst, b.lipschitz_cst = 2.0, 3.0
    assert B.KhatriRaoProduct(a, b).lipschitz_cst == 6.0
    with pytest.raises(ValueError, match='Invalid shapes.'):
        B.KhatriRaoProduct(a, B.DenseLinearOperator(np.ones((4, 6))))
    mk = lambda k, n, l=9: B.KhatriRaoProduct(B.DenseLinearOperator(np.ones((k, l))), B.DenseLinearOperator(np.ones((n, l))))
    assert (O.KR_MAX_NK, O.KR_MAX_ROWS, O.KR_SLAB, O.KR_MAX_GROUPS) == (1024, 120, 64, 512)
    assert mk(32, 32)._route() == 'fused' and mk(33, 32)._route() == 'torch' == mk(*C.KR_ABOVE[:2])._route()
    assert mk(8, 112)._route() == 'fused' and mk(8, 113)._route() == 'torch'       # k + n past 120 at k n <= 1024
    assert mk(1, 119)._route() == 'fused' and mk(1, 120)._route() == 'torch'
    # the adjoint's measured boundary: k n <= 256 in both dtypes, up to 32 x 32 in fp64
    import torch
    routes = {(k, n): [O.kr_route(k, n, dt, adj) for dt in (np.float32, torch.float64) for adj in (False, True)]
              for k, n in ((16, 16), (32, 8), (32, 16), (32, 32), (64, 16), (100, 10), (33, 32))}
    assert routes[(16, 16)] == routes[(32, 8)] == ['fused'] * 4
    assert routes[(32, 16)] == routes[(32, 32)] == ['fused', 'torch', 'fused', 'fused']
    assert routes[(64, 16)] == routes[(100, 10)] == ['fused', 'torch', 'fused', 'torch']
    assert routes[(33, 32)] == ['torch'] * 4
    assert mk(32, 32)._route(np.float32, adjoint=True) == 'torch' and mk(32, 32)._route(np.float64, adjoint=True) == 'fused'
    s = lambda shape, seed: B.SparseLinearOperator(C.sparse(shape, seed))
    assert B.KhatriRaoProduct(s((5, 7), 0), s((4, 7), 1))._route() == 'csr'
    assert B.KhatriRaoProduct(a, s((4, 7), 1))._route() == 'generic'
    assert B.KhatriRaoProduct(D.SecondDerivative(size=11), D.SecondDerivative(size=11))._route() == 'generic'
    aH = B.DenseLinearOperator(np.ascontiguousarray(Am.T)).H
    assert aH.shape == a.shape and B.KhatriRaoProduct(aH, b)._route() == 'generic'    # a wrapper holds no matrix of its own
    assert 'broken' in B.KhatriRaoProduct.__doc__ and '2-D' in B.KhatriRaoProduct.__doc__


def test_block_operators_attributes_and_errors():
    from pycsou_amd.core.linop import LinearOperator
    B, D = _ops()
    ops, mats = C.block_layout(D)
    Bop = B.BlockOperator(ops, n_jobs=4)
    N = C.DOCTEST_NV * C.DOCTEST_NH
    assert isinstance(Bop, LinearOperator) and Bop.shape == (2 * N, 3 * N) == np.block(mats).shape
    with pytest.raises(ValueError):
        B.BlockOperator([[ops[0][0], ops[0][1]], [ops[1][0]]])                      # ragged rows
    with pytest.raises(ValueError):
        B.BlockOperator([[ops[0][0], B.NullOperator((5, N))]])                      # rows of one block row differ
    with pytest.raises(ValueError):
        B.BlockOperator([[ops[0][0]], [B.NullOperator((N, 5))]])                    # columns of one block column differ
    with pytest.raises(ValueError):
        B.BlockOperator([])
    a, b, c = B.DenseLinearOperator(np.ones((3, 4))), B.IdentityOperator(5), B.HomothetyMap(2, 0.5)
    Dg = B.BlockDiagonalOperator(a, b, c, n_jobs=2)
    assert Dg.shape == (10, 11) and Dg.lipschitz_cst == np.inf and not Dg.is_symmetric
    a.lipschitz_cst = 3.0
    assert B.BlockDiagonalOperator(a, b, c).lipschitz_cst == 3.0
    assert B.BlockDiagonalOperator(b, c).lipschitz_cst == 1 and B.BlockDiagonalOperator(b, c).is_symmetric
    with pytest.raises(ValueError):
        B.BlockDiagonalOperator()


# ---------------------------------------------------------------- the C ABI
def test_new_symbols_exported_abi_unchanged():
    from pycsou_amd import _lib, _ops
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pcs_abi_version() == 10 and _lib.ABI_VERSION == 10
    for name in ('spmm', 'spmm_plan', 'khatri_rao_fwd', 'khatri_rao_adj', 'kr_fwd_plan', 'kr_fused_ok', 'kr_route'):
        assert callable(getattr(_ops, name))
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'pycsou_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert f'int {name}(' in header
    for macro, val in (('PCS_KR_SLAB', 64), ('PCS_KR_MAX_NK', 1024), ('PCS_KR_MAX_ROWS', 120), ('PCS_KR_MAX_GROUPS', 512)):
        assert f'#define {macro} {val}' in header and getattr(_lib, macro) == val


RP, CI, VA, X, OUT, CR, CS, LR, LF, PA, BB = (0x100000 * k for k in range(1, 12))  # stand-in addresses: never dereferenced


def _spmm(lib, **over):
    from pycsou_amd import _lib
    kw = dict(dtype=_lib.PCS_F64, axis=0, accumulate=0, nrows=3, ncols=7, nnz=4, rowptr=RP, colind=CI, vals=VA, x=X,
              out=OUT, nb=5, lanes=4, nchunks=0, chunk_row=None, chunk_start=None, nlong=0, long_row=None,
              long_first=None, partials=None, partials_len=0)
    kw.update(over)
    return lib.pcs_csr_spmm(*[kw[k] for k in ('dtype', 'axis', 'accumulate', 'nrows', 'ncols', 'nnz', 'rowptr', 'colind',
                                              'vals', 'x', 'out', 'nb', 'lanes', 'nchunks', 'chunk_row', 'chunk_start',
                                              'nlong', 'long_row', 'long_first', 'partials', 'partials_len')], None)


LONG = dict(axis=1, nnz=10000, nchunks=3, chunk_row=CR, chunk_start=CS, nlong=1, long_row=LR, long_first=LF, partials=PA,
            partials_len=15)
SPMM_BAD = {
    'dtype': dict(dtype=2), 'dtype_neg': dict(dtype=-1), 'axis2': dict(axis=2), 'axis_neg': dict(axis=-1),
    'accumulate2': dict(accumulate=2), 'nrows_neg': dict(nrows=-1), 'ncols_neg': dict(ncols=-1), 'nnz_neg': dict(nnz=-1),
    'nb_neg': dict(nb=-1), 'ncols_2p31': dict(ncols=1 << 31), 'nb_huge': dict(nb=1 << 41), 'rowptr': dict(rowptr=None),
    'colind': dict(colind=None), 'vals': dict(vals=None), 'x': dict(x=None), 'out': dict(out=None),
    'lanes0': dict(lanes=0), 'lanes3': dict(lanes=3), 'lanes128': dict(lanes=128), 'alias': dict(out=X),
    'alias_inside': dict(out=X + 8 * 30), 'alias_tail': dict(x=OUT + 8 * 14), 'alias_axis1': dict(axis=1, out=X + 8 * 34),
    'nchunks_neg': dict(nchunks=-1), 'nlong_neg': dict(nlong=-1), 'partials_len_neg': dict(partials_len=-1),
    'chunks_without_rows': dict(LONG, nlong=0), 'rows_without_chunks': dict(LONG, nchunks=0),
    'more_rows_than_chunks': dict(LONG, nlong=4), 'too_many_chunks': dict(LONG, nchunks=4),
    'chunk_row': dict(LONG, chunk_row=None), 'chunk_start': dict(LONG, chunk_start=None),
    'long_row': dict(LONG, long_row=None), 'long_first': dict(LONG, long_first=None),
    'partials': dict(LONG, partials=None), 'partials_align': dict(LONG, partials=PA + 4),
    'partials_short_for_nb': dict(LONG, partials_len=14), 'partials_short_nb1_axis0': dict(LONG, axis=0, nb=1, partials_len=2),
    'entries_without_columns': dict(ncols=0), 'entries_without_rows': dict(nrows=0),
}


@pytest.mark.parametrize('bad', sorted(SPMM_BAD))
def test_spmm_argument_checks(bad):
    """Every bad-argument case returns PCS_EINVAL before any device call (no GPU here)."""
    from pycsou_amd import _lib
    assert _spmm(_lib.load(), **SPMM_BAD[bad]) == -1


def _kr(lib, which, **over):
    from pycsou_amd import _lib
    kw = dict(dtype=_lib.PCS_F32, A=VA, B=BB, x=X, out=OUT, k=5, n=4, l=200, spg=1, ngroups=4, partials=PA,
              partials_len=80)
    kw.update(over)
    if which == 'fwd':
        return lib.pcs_khatri_rao_fwd(*[kw[k] for k in ('dtype', 'A', 'B', 'x', 'out', 'k', 'n', 'l', 'spg', 'ngroups',
                                                        'partials', 'partials_len')], None)
    return lib.pcs_khatri_rao_adj(*[kw[k] for k in ('dtype', 'A', 'B', 'x', 'out', 'k', 'n', 'l')], None)


KR_BAD_BOTH = {
    'dtype': dict(dtype=2), 'dtype_neg': dict(dtype=-1), 'k_neg': dict(k=-1), 'n_neg': dict(n=-1), 'l_neg': dict(l=-1),
    'A': dict(A=None), 'B': dict(B=None), 'x_or_Y': dict(x=None), 'out': dict(out=None),
    'nk_past_limit': dict(k=33, n=32), 'rows_past_limit': dict(k=8, n=113), 'alias_A': dict(out=VA), 'alias_B': dict(out=BB + 16),
    'alias_x_or_Y': dict(out=X),
}
KR_BAD_FWD = {
    'spg0': dict(spg=0), 'ngroups_neg': dict(ngroups=-1), 'plan_short': dict(ngroups=3), 'plan_long': dict(ngroups=5),
    'plan_spg2': dict(spg=2), 'too_many_groups': dict(l=64 * 513, ngroups=513, partials_len=513 * 20),
    'partials': dict(partials=None), 'partials_align': dict(partials=PA + 4), 'partials_short': dict(partials_len=79),
    'partials_len_neg': dict(partials_len=-1), 'alias_partials': dict(out=PA + 8),
}


@pytest.mark.parametrize('which', ['fwd', 'adj'])
@pytest.mark.parametrize('bad', sorted(KR_BAD_BOTH))
def test_khatri_rao_argument_checks(which, bad):
    from pycsou_amd import _lib
    assert _kr(_lib.load(), which, **KR_BAD_BOTH[bad]) == -1


@pytest.mark.parametrize('bad', sorted(KR_BAD_FWD))
def test_khatri_rao_forward_plan_checks(bad):
    from pycsou_amd import _lib
    assert _kr(_lib.load(), 'fwd', **KR_BAD_FWD[bad]) == -1


def test_zero_size_calls_are_noops():
    from pycsou_amd import _lib
    lib = _lib.load()
    for dt in (_lib.PCS_F32, _lib.PCS_F64):
        for axis in (0, 1):
            assert _spmm(lib, dtype=dt, axis=axis, nrows=0, ncols=0, nnz=0, colind=None, vals=None, x=None, out=None) == 0
            assert _spmm(lib, dtype=dt, axis=axis, nb=0, x=None, out=None) == 0
        assert _kr(lib, 'fwd', dtype=dt, k=0, ngroups=4, partials=None, partials_len=0, A=None, out=None) == 0
        assert _kr(lib, 'adj', dtype=dt, l=0, A=None, B=None, out=None) == 0


# ---------------------------------------------------------------- launch and workspace plans
class _Csr:
    def __init__(self, shape, nchunks):
        self.shape, self.nchunks = shape, nchunks


def test_spmm_plan():
    from pycsou_amd import _ops as O
    A = _Csr((8, 5000), 2)
    widths = {nb: O.spmm_plan(A, 0, nb) for nb in (2, 3, 63, 64, 65, 130)}
    assert [widths[nb]['width'] for nb in (2, 3, 63, 64, 65, 130)] == [2, 4, 64, 64, 64, 64]
    assert [widths[nb]['col_tiles'] for nb in (2, 3, 63, 64, 65, 130)] == [1, 1, 1, 1, 2, 3]
    assert all(p['family'] == 'cols' and p['partials'] == 0 for p in widths.values())
    for axis in (0, 1):                          # one column or row: the vector product, pcs_csr_spmv's own plan
        assert O.spmm_plan(A, axis, 1) == {'family': 'rows', 'width': 0, 'col_tiles': 0, 'partials': 2}
    assert [O.spmm_plan(A, 1, nb)['partials'] for nb in (0, 3, 65)] == [0, 6, 130]
    assert O.spmm_plan(_Csr((8, 50), 0), 1, 65) == {'family': 'rows', 'width': 0, 'col_tiles': 0, 'partials': 0}
    with pytest.raises(ValueError):
        O.spmm_plan(A, 2, 4)
    with pytest.raises(ValueError):
        O.spmm_plan(A, 0, -1)


def test_khatri_rao_forward_plan():
    from pycsou_amd import _ops as O
    S, G = O.KR_SLAB, O.KR_MAX_GROUPS
    assert O.kr_fwd_plan(5, 4, 0) == (1, 0, 1) and O.kr_fwd_plan(5, 4, 1) == (1, 1, 20) == O.kr_fwd_plan(5, 4, S)
    assert O.kr_fwd_plan(5, 4, S + 1) == (1, 2, 40) and O.kr_fwd_plan(*C.KR_SLABS) == (1, 8, 8 * 48)
    assert O.kr_fwd_plan(32, 32, S * G) == (1, G, G * 1024) and O.kr_fwd_plan(32, 32, S * G + 1) == (2, G // 2 + 1, (G // 2 + 1) * 1024)
    for l in (1, 63, 64, 65, 300, 10 ** 5, S * G * 3 + 7):
        spg, ngroups, ws = O.kr_fwd_plan(3, 2, l)
        nslabs = -(-l // S)
        assert ngroups <= G and (ngroups - 1) * spg < nslabs <= ngroups * spg and ws == 6 * ngroups    # the groups tile the slabs
    assert [O.kr_fused_ok(k, n) for k, n in ((1, 1), (32, 32), (33, 32), (8, 112), (8, 113), (0, 4), (1024, 1))] \
        == [True, True, False, True, False, False, False]


# ---------------------------------------------------------------- host assembly of the sparse Khatri-Rao matrix
@pytest.mark.parametrize('shapes', [((5, 7), (4, 7)), ((1, 3), (1, 3)), ((6, 1), (3, 1)), ((9, 40), (7, 40))])
def test_khatri_rao_csr_equals_the_definition(shapes):
    from pycsou_amd.linop.base import khatri_rao_csr
    A, B = C.sparse(shapes[0], 0), C.sparse(shapes[1], 1)
    for a, b in ((A, B), (A.tocsc(), B.tocoo())):
        M = khatri_rao_csr(a, b)
        assert sp.isspmatrix_csr(M) and M.has_sorted_indices and M.shape == (shapes[0][0] * shapes[1][0], shapes[0][1])
        assert np.array_equal(M.toarray(), C.khatri_rao_matrix(A.toarray(), B.toarray()))
        assert M.nnz == int(np.sum(np.diff(A.tocsc().indptr) * np.diff(B.tocsc().indptr)))
    E = khatri_rao_csr(sp.csr_matrix((3, shapes[1][1])), B)
    assert E.nnz == 0 and E.shape == (3 * shapes[1][0], shapes[1][1])
    with pytest.raises(ValueError, match='Invalid shapes.'):
        khatri_rao_csr(sp.csr_matrix((3, shapes[1][1] + 1)), B)


def test_khatri_rao_uploads_the_assembled_matrix_and_its_transpose(monkeypatch):
    from pycsou_amd import _ops as O
    from pycsou_amd.linop import KhatriRaoProduct, SparseLinearOperator
    A, B = C.sparse((5, 7), 0), C.sparse((4, 7), 1)
    op = KhatriRaoProduct(SparseLinearOperator(A), SparseLinearOperator(B))
    made = []
    monkeypatch.setattr(O, 'DeviceCSR', lambda h, dtype: made.append(h) or h)       # record the host matrix, no upload
    f, t = op._matrix(np.float64, False), op._matrix(np.float64, True)
    ref = C.khatri_rao_matrix(A.toarray(), B.toarray())
    assert np.array_equal(f.toarray(), ref) and np.array_equal(t.toarray(), ref.T) and t.has_sorted_indices
    assert op._matrix(np.float64, True) is t and len(made) == 2                     # cached


# ---------------------------------------------------------------- the fixture
def test_fixture_is_arrays_only_and_small():
    path = os.path.join(GOLDEN, 'kron_family.npz')
    assert os.path.getsize(path) < 1_000_000
    g = load('kron_family.npz')                 # allow_pickle=False: object arrays would raise
    assert all(a.dtype.kind in 'fiu' for a in g.values())


def _close(a, ref):
    return np.max(np.abs(a - ref)) <= 64 * np.finfo(np.float64).eps * max(np.max(np.abs(ref)), 1e-300)


def test_fixture_equals_the_definitions():
    """Every recorded vector against the dense definitions: pins kron(B, A), not kron(A, B)."""
    g = load('kron_family.npz')
    for name in C.KRON_PAIRS:
        for tag, matrix, square in (('kron', C.kron_matrix, False), ('ksum', C.ksum_matrix, True)):
            A, B = C.pair_matrices(name, square)
            x, y = C.pair_inputs(A, B)
            M = matrix(A, B)
            assert _close(g[f'{tag}_{name}_fwd'], M @ x) and _close(g[f'{tag}_{name}_adj'], M.T @ y), (tag, name)
    A, B = C.pair_matrices('dense')
    x, _ = C.pair_inputs(A, B)
    assert not _close(g['kron_dense_fwd'], np.kron(A, B) @ x)                      # the other ordering is another operator
    A, B = C.kr_dense_pair()
    M = C.khatri_rao_matrix(A, B)
    assert g['kr_dense_fwd'].shape == (4, 5) and g['kr_dense_adj'].shape == (7,)
    assert _close(g['kr_dense_fwd'].ravel(), M @ C.make_vec(7, 0)) and _close(g['kr_dense_adj'], M.T @ C.make_vec(20, 1))
    n = C.KR_DOCTEST_N
    M = C.khatri_rao_matrix(C.d2_matrix(n), C.d2_matrix(n))
    assert g['kr_doctest_fwd'].shape == (n * n,) and _close(g['kr_doctest_fwd'], M @ np.arange(n))
    assert _close(g['kr_doctest_adj'], M.T @ C.make_vec(n * n, 9))
    assert int(g['pds_n_iter']) == C.PDS_ITERS and np.all(np.isfinite(g['pds_x'])) and g['pds_x'].shape == (24 * 30,)
    Ah, Bv, _ = C.pds_problem()
    assert abs(float(g['pds_Alip']) - np.linalg.norm(Ah, 2)) < 1e-14 and abs(float(g['pds_Blip']) - np.linalg.norm(Bv, 2)) < 1e-14


def test_block_definitions_are_consistent():
    """np.block of the layout's matrices is what the reference's doctest (base.py:365-371) computes."""
    _, D = _ops()
    _, mats = C.block_layout(D)
    nv, nh = C.DOCTEST_NV, C.DOCTEST_NH
    x = np.zeros((nv, nh))
    x[nv // 2, nh // 2] = 1
    z = np.tile(x, (3, 1)).flatten()
    Mv, Mh = mats[0][0], mats[1][0]
    want = np.concatenate([(Mv + 0.5 * Mv - Mh) @ x.ravel(), (Mh + 2 * Mh + Mv) @ x.ravel()])
    assert np.allclose(np.block(mats) @ z, want, rtol=1e-14, atol=1e-14)


def test_fused_selectors_leave_these_operators_to_the_generic_path():
    from pycsou_amd.func import L1Norm
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.linop import DenseLinearOperator, KroneckerProduct, SparseLinearOperator
    from pycsou_amd.opt.engine import match_apgd2d, match_masked_stencil2d, match_pds2d, match_stencil2d
    from pycsou_amd.opt.engine3d import match_pds3d
    Ah, Bv, y = C.pds_problem()
    N = y.size
    G = KroneckerProduct(DenseLinearOperator(Ah), DenseLinearOperator(Bv))
    K = SparseLinearOperator(C.forward_difference_matrix(C.PDS_SHAPE))
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y) * G
    H = C.PDS_LAM * L1Norm(dim=2 * N)
    for match in (match_pds2d, match_stencil2d, match_masked_stencil2d, match_pds3d):
        assert match(F, None, H, K, True) is None, match.__name__
    assert match_apgd2d(F, 0.1 * L1Norm(dim=N)) is None
