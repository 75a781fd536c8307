"""Basic linear operators (mirrors the hot-path part of ``pycsou/linop/base.py``).

``DiagonalOperator`` / ``IdentityOperator`` / ``NullOperator`` / ``HomothetyMap``
(``base.py:551-633``) are the defaults PDS inserts for missing K / F terms and the
scalar factors of the algebra; ``DenseLinearOperator`` (``base.py:102-118``) backs the
LASSO problem (C1); ``LinOpStack`` / ``LinOpVStack`` / ``LinOpHStack`` (``base.py:159-302``)
build stacked K operators (notebook cell [62]: ``K = LinOpVStack(Gop, D)``);
``PolynomialLinearOperator`` (``base.py:636-700``) backs ``GeneralisedLaplacian``;
``SparseLinearOperator`` (``base.py:121-137``) holds a SciPy sparse matrix and applies it and its
transpose with the CSR kernel ``pcs_csr_spmv`` (``csrc/spmv.hip``).  ``KroneckerProduct`` / ``KroneckerSum`` /
``KhatriRaoProduct`` (``base.py:715-989``) act through the device-side ``LinearOperator._apply_cols`` (an operator
along one axis of a matrix: ``torch.matmul``, ``pcs_csr_spmm``, one stencil launch, or a column loop on the
device) and, for two dense factors, the fused ``pcs_khatri_rao_*`` kernels (``csrc/khatri_rao.hip``);
``BlockOperator`` / ``BlockDiagonalOperator`` (``base.py:339-548``) are stacks of the blocks.
"""

from numbers import Number

import numpy as np
import scipy.sparse as sparse
import torch

from .. import _ops as O
from ..core.linop import LinearOperator
from ..core.map import DiffMapStack


class ExplicitLinearOperator(LinearOperator):
    """Operator given by an explicit matrix held in HBM (``base.py:57-99``): a dense array, or anything
    ``scipy.sparse.issparse`` accepts.  A sparse matrix stays in ``.mat`` as given; its CSR form with sorted
    indices, and on the first adjoint the CSR of its transpose (``mat.T.tocsr()``, sorted), are built once on the
    host and cached on the device per dtype, with their long-row chunk lists and workspaces."""

    def __init__(self, array, is_symmetric=False):
        is_sparse = sparse.issparse(array)
        if isinstance(array, torch.Tensor):
            dt = np.float32 if array.dtype == torch.float32 else np.float64
        elif isinstance(array, np.ndarray) or is_sparse:
            dt = array.dtype
        else:
            raise TypeError('Invalid input type.')
        super().__init__(shape=tuple(array.shape), dtype=dt, is_explicit=True, is_dask=False, is_dense=not is_sparse,
                         is_sparse=is_sparse, is_symmetric=is_symmetric)
        self.mat = array
        self._dev = {}
        self._host_csr = {}

    def _csr(self, dtype, transposed):
        """The device CSR of ``mat`` (or of its transpose) in ``dtype``."""
        A = self._dev.get((dtype, transposed))
        if A is None:
            h = self._host_csr.get(transposed)
            if h is None:
                h = (self.mat.T if transposed else self.mat).tocsr()
                if not h.has_sorted_indices:
                    h = h.sorted_indices()      # a copy: ``mat`` is the caller's
                self._host_csr[transposed] = h
            A = self._dev[(dtype, transposed)] = O.DeviceCSR(h, dtype)
        return A


    def _m(self, dtype):
        m = self._dev.get(dtype)
        if m is None:
            m = torch.as_tensor(np.asarray(self.mat) if not isinstance(self.mat, torch.Tensor) else self.mat)
            m = m.to(device=O.device(), dtype=dtype).contiguous()
            self._dev[dtype] = m
        return m

    def _apply(self, t):
        if self.is_sparse:
            return O.spmv(self._csr(t.dtype, False), t)
        return torch.mv(self._m(t.dtype), t)

    def _adj(self, t):
        if self.is_sparse:
            return O.spmv(self._csr(t.dtype, True), t)
        return torch.mv(self._m(t.dtype).T, t)

    def _apply_cols(self, T, axis, adjoint=False):
        if self.is_sparse:
            return O.spmm(self._csr(T.dtype, adjoint), T, axis)
        M = self._m(T.dtype)
        if axis == 0:
            return torch.matmul(M.T if adjoint else M, T)
        return torch.matmul(T, M if adjoint else M.T)

    def _apply_cols_acc(self, T, axis, adjoint, acc):
        if self.is_sparse:
            if acc.data_ptr() == T.data_ptr():      # an identity term handed its input on: do not write into it
                return O.add(acc, O.spmm(self._csr(T.dtype, adjoint), T, axis))
            return O.spmm(self._csr(T.dtype, adjoint), T, axis, out=acc, accumulate=True)
        M = self._m(T.dtype)
        if axis == 0:
            return torch.addmm(acc, M.T if adjoint else M, T)
        return torch.addmm(acc, T, M if adjoint else M.T)


class DenseLinearOperator(ExplicitLinearOperator):
    """``base.py:102-118``."""

    def __init__(self, ndarray, is_symmetric=False):
        super().__init__(array=ndarray, is_symmetric=is_symmetric)


class SparseLinearOperator(ExplicitLinearOperator):
    """``base.py:121-137``: the operator of a SciPy sparse matrix (``is_sparse=True``, ``is_dense=False``)."""

    def __init__(self, spmatrix, is_symmetric=False):
        super().__init__(array=spmatrix, is_symmetric=is_symmetric)


class DiagonalOperator(LinearOperator):
    """``base.py:551-579``."""

    def __init__(self, diag):
        self.diag = np.asarray(diag).reshape(-1)
        super().__init__(shape=(self.diag.size, self.diag.size), dtype=self.diag.dtype, is_explicit=False,
                         is_dense=False, is_sparse=False, is_dask=False,
                         is_symmetric=bool(np.all(np.isreal(self.diag))))
        self.lipschitz_cst = self.diff_lipschitz_cst = np.max(diag)
        self._dev = {}

    def _d(self, dtype):
        d = self._dev.get(dtype)
        if d is None:
            d = torch.as_tensor(self.diag).to(device=O.device(), dtype=dtype)
            self._dev[dtype] = d
        return d

    def _apply(self, t):
        if isinstance(t, Number):
            return float(self.diag[0]) * t
        if self.diag.size == 1:
            return O.scale(t, float(self.diag[0]))
        return O.mul(t, self._d(t.dtype))

    def _adj(self, t):
        return self._apply(t)

    def _apply_cols(self, T, axis, adjoint=False):
        if self.diag.size == 1:
            return O.scale(T, float(self.diag[0]))
        d = self._d(T.dtype)
        return T * (d[:, None] if axis == 0 else d[None, :])

    def __call__(self, x):
        if self.shape[1] == 1 and not O.is_array(x):
            return float(self.diag[0]) * x
        return LinearOperator.__call__(self, x)


class IdentityOperator(DiagonalOperator):
    """``base.py:582-598``."""

    def __init__(self, size, dtype=None):
        super().__init__(np.ones(shape=(size,), dtype=dtype))
        self.lipschitz_cst = self.diff_lipschitz_cst = 1

    def _apply(self, t):
        return t

    def _adj(self, t):
        return t

    def _apply_cols(self, T, axis, adjoint=False):
        return T


class NullOperator(LinearOperator):
    """``base.py:601-622``."""

    def __init__(self, shape, dtype=np.float64):
        super().__init__(shape=shape, dtype=dtype, is_explicit=False, is_dense=False, is_sparse=False,
                         is_dask=False, is_symmetric=shape[0] == shape[1])
        self.lipschitz_cst = self.diff_lipschitz_cst = 0

    def _apply(self, t):
        return torch.zeros(self.shape[0], dtype=t.dtype, device=t.device)

    def _adj(self, t):
        return torch.zeros(self.shape[1], dtype=t.dtype, device=t.device)

    def _apply_cols(self, T, axis, adjoint=False):
        n = self.shape[1] if adjoint else self.shape[0]
        shape = (n, T.shape[1]) if axis == 0 else (T.shape[0], n)
        return torch.zeros(shape, dtype=T.dtype, device=T.device)

    def eigenvals(self, k, which='LM', **kwargs):
        return np.zeros(shape=(k,), dtype=self.dtype)

    def singularvals(self, k, which='LM', **kwargs):
        return np.zeros(shape=(k,), dtype=self.dtype)


class HomothetyMap(DiagonalOperator):
    """``x -> constant * x`` (``base.py:625-633``); ``jacobianT`` is the constant."""

    def __init__(self, size, constant):
        self.cst = constant
        super().__init__(diag=constant)
        self.shape = (size, size)
        self.lipschitz_cst = self.diff_lipschitz_cst = constant

    def _jacT(self, t=None):
        return self.cst

    def jacobianT(self, arg=None):
        return self.cst


class LinOpStack(LinearOperator, DiffMapStack):
    """Vertical (``axis=0``) / horizontal (``axis=1``) stack of linear operators
    (``base.py:159-256``): ``V x = (L_1 x, ..., L_k x)``, ``V^* y = sum_i L_i^* y_i``;
    ``H (x_1, ..., x_k) = sum_i L_i x_i``, ``H^* y = (L_1^* y, ..., L_k^* y)``.  Sums are
    accumulated in block order (``result = 0; result += ...``) as the reference does."""

    def __init__(self, *linops, axis, n_jobs=1, joblib_backend='loky'):
        DiffMapStack.__init__(self, *linops, axis=axis, n_jobs=n_jobs, joblib_backend=joblib_backend)
        self.linops = self.maps
        self.is_explicit_list = [op.is_explicit for op in self.linops]
        self.is_dense_list = [op.is_dense for op in self.linops]
        self.is_sparse_list = [op.is_sparse for op in self.linops]
        self.is_dask_list = [op.is_dask for op in self.linops]
        self.is_symmetric_list = [op.is_symmetric for op in self.linops]
        LinearOperator.__init__(self, shape=self.shape, is_explicit=bool(np.prod(self.is_explicit_list).astype(bool)),
                                is_dense=bool(np.prod(self.is_dense_list).astype(bool)),
                                is_sparse=bool(np.prod(self.is_sparse_list).astype(bool)),
                                is_dask=bool(np.prod(self.is_dask_list).astype(bool)),
                                is_symmetric=bool(np.prod(self.is_symmetric_list).astype(bool)),
                                lipschitz_cst=self.lipschitz_cst)
        dts = {op.dtype for op in self.linops}
        self.dtype = dts.pop() if len(dts) == 1 else None

    def _adj(self, t):
        from ..core.map import _cat
        if self.axis == 0:
            o = _sections([op.shape[0] for op in self.linops])
            result = None
            for i, op in enumerate(self.linops):
                r = op._adj(t[o[i]:o[i + 1]])
                result = r if result is None else O.add(result, r)
            return result
        return _cat([op._adj(t) for op in self.linops], t)


def _sections(sizes):
    return [0] + [int(s) for s in np.cumsum(sizes)]


class LinOpVStack(LinOpStack):
    """``LinOpStack(*linops, axis=0)`` (``base.py:259-279``)."""

    def __init__(self, *linops, n_jobs=1, joblib_backend='loky'):
        super().__init__(*linops, axis=0, n_jobs=n_jobs, joblib_backend=joblib_backend)


class LinOpHStack(LinOpStack):
    """``LinOpStack(*linops, axis=1)`` (``base.py:282-302``)."""

    def __init__(self, *linops, n_jobs=1, joblib_backend='loky'):
        super().__init__(*linops, axis=1, n_jobs=n_jobs, joblib_backend=joblib_backend)


class PolynomialLinearOperator(LinearOperator):
    """``P(L) = a_0 I + a_1 L + ... + a_N L^N`` for a square ``L`` (``base.py:636-700``):
    ``y = a_0 x; z = x; y += a_i (z = L z)`` in the reference's order; the adjoint uses
    ``L^*`` (or ``P(L)`` itself when ``L`` is symmetric)."""

    def __init__(self, LinOp, coeffs):
        self.coeffs = np.asarray(coeffs).astype(LinOp.dtype if LinOp.dtype is not None else np.float64)
        if LinOp.shape[0] != LinOp.shape[1]:
            raise ValueError('Input linear operator must be square.')
        self.Linop = LinOp
        super().__init__(shape=LinOp.shape, dtype=LinOp.dtype, is_explicit=LinOp.is_explicit,
                         is_dense=LinOp.is_dense, is_sparse=LinOp.is_sparse, is_dask=LinOp.is_dask,
                         is_symmetric=LinOp.is_symmetric)

    def _poly(self, t, step):
        z = t
        y = O.scale(t, float(self.coeffs[0]))
        for c in self.coeffs[1:]:
            z = step(z)
            y = O.axpby(y, z, 1.0, float(c))
        return y

    def _apply(self, t):
        return self._poly(t, self.Linop._apply)

    def _adj(self, t):
        if self.is_symmetric:
            return self._apply(t)
        return self._poly(t, self.Linop._adj)

    def _apply_cols(self, T, axis, adjoint=False):
        adjoint = adjoint and not self.is_symmetric
        return self._poly(T, lambda Z: self.Linop._apply_cols(Z, axis, adjoint))


class KroneckerProduct(LinearOperator):
    r"""Kronecker product of ``linop1`` = A (k x l) and ``linop2`` = B (n x m) (``base.py:715-803``):
    ``K x = vec(B X A^T)`` with ``X = x.reshape(m, l)`` and ``K^* y = vec(B^* Y A)`` with ``Y = y.reshape(n, k)``
    (C order), i.e. the matrix ``np.kron(B, A)``, of shape ``(n k, m l)``.  Both factors act through
    ``_apply_cols``: one ``torch.matmul`` / ``pcs_csr_spmm`` / stencil launch per factor where it has a batched
    form.  ``lipschitz_cst`` is the product of the factors' constants (``inf`` until they have one);
    ``compute_lipschitz_cst`` computes the missing ones and multiplies: ``||A (x) B|| = ||A|| ||B||`` exactly."""

    def __init__(self, linop1, linop2):
        self.linop1, self.linop2 = linop1, linop2
        super().__init__(shape=(linop2.shape[0] * linop1.shape[0], linop2.shape[1] * linop1.shape[1]),
                         dtype=linop1.dtype, lipschitz_cst=_lip_product(linop1, linop2))

    def _apply_cols(self, T, axis, adjoint=False):
        A, B = self.linop1, self.linop2
        (k, l), (n, m) = (A.shape, B.shape) if not adjoint else (A.shape[::-1], B.shape[::-1])
        if axis == 1:
            nb = T.shape[0]
            Z = A._apply_cols(T.reshape(nb * m, l), 1, adjoint)
            return B._apply_mid(Z.reshape(nb, m, k), adjoint).reshape(nb, n * k)
        nb = T.shape[1]
        Z = B._apply_cols(T.reshape(m, l * nb), 0, adjoint)
        return A._apply_mid(Z.reshape(n, l, nb), adjoint).reshape(n * k, nb)

    def _apply(self, t):
        return self._apply_cols(t.reshape(1, -1), 1).reshape(-1)

    def _adj(self, t):
        return self._apply_cols(t.reshape(1, -1), 1, adjoint=True).reshape(-1)

    def compute_lipschitz_cst(self, **kwargs):
        for op in (self.linop1, self.linop2):
            if op.lipschitz_cst == np.inf:
                op.compute_lipschitz_cst(**kwargs)
        self.lipschitz_cst = self.diff_lipschitz_cst = float(self.linop1.lipschitz_cst * self.linop2.lipschitz_cst)

    @property
    def PinvOp(self):
        """``(A (x) B)^+ = A^+ (x) B^+`` (``base.py:802-803``): each factor's pseudo-inverse solves all the lines
        of the reshaped vector as one batch (``LinOpPinv._apply_cols``)."""
        return KroneckerProduct(self.linop1.PinvOp, self.linop2.PinvOp)


def _lip_product(op1, op2):
    a, b = op1.lipschitz_cst, op2.lipschitz_cst
    return np.inf if np.inf in (a, b) else a * b


class KroneckerSum(LinearOperator):
    r"""Kronecker sum of two square operators ``linop1`` = A (l x l) and ``linop2`` = B (m x m)
    (``base.py:806-886``): ``S x = vec(X A^T + B X)`` with ``X = x.reshape(m, l)``, the matrix
    ``kron(I_m, A) + kron(B, I_l)``.  The reference does not check the shapes; anything but two square factors is
    a ``ValueError`` here.  The second term is accumulated into the first where the factor can
    (``pcs_csr_spmm`` with ``accumulate``, ``torch.addmm``).  ``lipschitz_cst`` starts as the sum of the factors'
    constants, as in the reference; ``compute_lipschitz_cst`` is the inherited device Lanczos."""

    def __init__(self, linop1, linop2):
        if linop1.shape[0] != linop1.shape[1] or linop2.shape[0] != linop2.shape[1]:
            raise ValueError('KroneckerSum is defined for two square operators.')
        self.linop1, self.linop2 = linop1, linop2
        super().__init__(shape=(linop2.shape[0] * linop1.shape[0], linop2.shape[1] * linop1.shape[1]),
                         dtype=linop1.dtype, lipschitz_cst=linop1.lipschitz_cst + linop2.lipschitz_cst)

    def _apply_cols(self, T, axis, adjoint=False):
        A, B = self.linop1, self.linop2
        l, m = A.shape[0], B.shape[0]
        if axis == 1:
            nb = T.shape[0]
            first = A._apply_cols(T.reshape(nb * m, l), 1, adjoint)
            if nb == 1:
                return B._apply_cols_acc(T.reshape(m, l), 0, adjoint, first).reshape(1, m * l)
            return O.add(first.reshape(nb, m * l), B._apply_mid(T.reshape(nb, m, l), adjoint).reshape(nb, m * l))
        nb = T.shape[1]
        first = B._apply_cols(T.reshape(m, l * nb), 0, adjoint)
        return O.add(first.reshape(m * l, nb), A._apply_mid(T.reshape(m, l, nb), adjoint).reshape(m * l, nb))

    def _apply(self, t):
        return self._apply_cols(t.reshape(1, -1), 1).reshape(-1)

    def _adj(self, t):
        return self._apply_cols(t.reshape(1, -1), 1, adjoint=True).reshape(-1)


def khatri_rao_csr(A, B):
    """The Khatri-Rao matrix of two SciPy sparse factors A (k x l) and B (n x l) as CSR with sorted indices:
    column c is ``kron(B[:, c], A[:, c])`` (row ``j k + i`` holds ``B[j, c] A[i, c]``), ``nnz(A_c) nnz(B_c)``
    entries, assembled on the host without the dense matrix."""
    A, B = sparse.csc_matrix(A), sparse.csc_matrix(B)
    (k, l), n = A.shape, B.shape[0]
    if B.shape[1] != l:
        raise ValueError('Invalid shapes.')
    na, nb = np.diff(A.indptr).astype(np.int64), np.diff(B.indptr).astype(np.int64)
    per_col = na * nb
    total = int(per_col.sum())
    col = np.repeat(np.arange(l, dtype=np.int64), per_col)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(per_col) - per_col, per_col)
    # entry (q, p) of column c pairs the q-th entry of B_c with the p-th entry of A_c
    q, p = within // np.maximum(na[col], 1), within % np.maximum(na[col], 1)
    ia, ib = A.indptr[col] + p, B.indptr[col] + q
    rows = B.indices[ib].astype(np.int64) * k + A.indices[ia]
    data = np.asarray(B.data)[ib] * np.asarray(A.data)[ia]
    M = sparse.coo_matrix((data, (rows, col)), shape=(n * k, l)).tocsr()
    M.sort_indices()
    return M


class KhatriRaoProduct(LinearOperator):
    r"""Khatri-Rao (column-wise Kronecker) product of ``linop1`` = A (k x l) and ``linop2`` = B (n x l)
    (``base.py:889-989``): column ``c`` of the matrix is ``np.kron(B[:, c], A[:, c])``; ``K x = vec(B diag(x) A^T)``
    and ``K^* y = diag(B^* Y A)`` with ``Y = y.reshape(n, k)``; shape ``(n k, l)``.

    Output shapes are the reference's: with two dense factors ``__call__`` returns the **2-D** array
    ``(B * x) A^T`` of shape ``(n, k)``; every other pair returns the flat ``(n k,)`` vector; ``adjoint`` returns
    ``(l,)``.  With two sparse factors the reference's branch is broken under current SciPy (forward: a 0-d object
    array, adjoint: shape ``(1, l)``); that pair returns the values and shapes of the dense branch here (forward
    ``(n, k)``, adjoint ``(l,)``).

    Routes: a dense pair runs the fused kernels ``pcs_khatri_rao_fwd`` / ``pcs_khatri_rao_adj`` while
    ``k n <= KR_MAX_NK`` and ``k + n <= KR_MAX_ROWS`` (the LDS and register budget derived in
    ``csrc/khatri_rao.hip``) and, for the adjoint, inside the measured boundary of ``_ops.kr_route``; the ``torch``
    composition ``mm(B * x, A^T)`` / ``sum(mm(Y, A) * B, 0)`` beyond; a
    sparse pair assembles the Khatri-Rao matrix itself as CSR once on the host (``khatri_rao_csr``) and applies it
    and its transpose with ``pcs_csr_spmv``; any other pair takes the reference's route through ``diag(x)`` and the
    diagonal of ``B^* Y A``, on the device via ``_apply_cols``."""

    def __init__(self, linop1, linop2):
        if linop1.shape[1] != linop2.shape[1]:
            raise ValueError('Invalid shapes.')
        self.linop1, self.linop2 = linop1, linop2
        super().__init__(shape=(linop2.shape[0] * linop1.shape[0], linop2.shape[1]), dtype=linop1.dtype,
                         lipschitz_cst=_lip_product(linop1, linop2))
        both = isinstance(linop1, ExplicitLinearOperator) and isinstance(linop2, ExplicitLinearOperator)
        self._dense_pair = both and linop1.is_dense and linop2.is_dense
        self._sparse_pair = both and linop1.is_sparse and linop2.is_sparse
        self._csr, self._ws = {}, {}
        self._host = {}

    def _route(self, dtype=torch.float64, adjoint=False):
        """'fused', 'torch', 'csr' or 'generic'."""
        if self._dense_pair:
            return O.kr_route(self.linop1.shape[0], self.linop2.shape[0], dtype, adjoint)
        return 'csr' if self._sparse_pair else 'generic'

    def _matrix(self, dtype, transposed):
        A = self._csr.get((dtype, transposed))
        if A is None:
            h = self._host.get(False)
            if h is None:
                h = self._host[False] = khatri_rao_csr(self.linop1.mat, self.linop2.mat)
            if transposed:
                h = self._host.get(True)
                if h is None:
                    h = self._host[False].T.tocsr()
                    h.sort_indices()
                    self._host[True] = h
            A = self._csr[(dtype, transposed)] = O.DeviceCSR(h, dtype)
        return A

    def _workspace(self, dtype):
        ws = self._ws.get(dtype)
        if ws is None:
            need = O.kr_fwd_plan(self.linop1.shape[0], self.linop2.shape[0], self.shape[1])[2]
            ws = self._ws[dtype] = torch.empty(need, dtype=torch.float64, device=O.device())
        return ws

    def _apply(self, t):
        A, B, route = self.linop1, self.linop2, self._route(t.dtype)
        if route == 'fused':
            return O.khatri_rao_fwd(A._m(t.dtype), B._m(t.dtype), t, self._workspace(t.dtype)).reshape(-1)
        if route == 'torch':
            return torch.mm(B._m(t.dtype) * t[None, :], A._m(t.dtype).T).reshape(-1)
        if route == 'csr':
            return O.spmv(self._matrix(t.dtype, False), t)
        Z = A._apply_cols(torch.diag(t), 0)                       # (k, l): A diag(x)
        return B._apply_cols(Z.T.contiguous(), 0).reshape(-1)     # (n, k): B diag(x) A^T

    def _adj(self, t):
        A, B, route = self.linop1, self.linop2, self._route(t.dtype, adjoint=True)
        k, n = A.shape[0], B.shape[0]
        if route == 'fused':
            return O.khatri_rao_adj(A._m(t.dtype), B._m(t.dtype), t.contiguous())
        if route == 'torch':
            return torch.sum(torch.mm(t.reshape(n, k), A._m(t.dtype)) * B._m(t.dtype), dim=0)
        if route == 'csr':
            return O.spmv(self._matrix(t.dtype, True), t)
        Z = A._apply_cols(t.reshape(n, k), 1, adjoint=True)       # (n, l): Y A
        return torch.diagonal(B._apply_cols(Z, 0, adjoint=True)).contiguous()   # diag(B^* Y A)

    def _apply_cols(self, T, axis, adjoint=False):
        if self._sparse_pair:                # the assembled CSR matrix: one batched product
            return O.spmm(self._matrix(T.dtype, adjoint), T, axis)
        return LinearOperator._apply_cols(self, T, axis, adjoint)

    def __call__(self, x):
        out = LinearOperator.__call__(self, x)
        if self._dense_pair or self._sparse_pair:
            return out.reshape(self.linop2.shape[0], self.linop1.shape[0])
        return out


def BlockOperator(linops, n_jobs=1):
    """``base.py:339-450``: the operator of a rectangular layout of blocks ``[[A, B], [C, D]]``, a vertical stack
    of horizontal stacks.  ``n_jobs`` is accepted and ignored.  All rows must have equal length and blocks of
    compatible shapes, else ``ValueError``."""
    rows = [list(r) for r in linops]
    if not rows or not rows[0] or len({len(r) for r in rows}) != 1:
        raise ValueError('BlockOperator: every row of blocks must have the same, non-zero length.')
    for r in rows:
        if len({op.shape[0] for op in r}) != 1:
            raise ValueError('BlockOperator: the blocks of a row must have equal numbers of rows.')
    for col in zip(*rows):
        if len({op.shape[1] for op in col}) != 1:
            raise ValueError('BlockOperator: the blocks of a column must have equal numbers of columns.')
    return LinOpVStack(*[LinOpHStack(*r) for r in rows])


class BlockDiagonalOperator(LinearOperator):
    """``base.py:453-548``: ``diag(L_1, ..., L_k)``: each operator acts on its own slice of the input and the
    results are concatenated.  ``n_jobs`` is accepted and ignored.  ``lipschitz_cst`` is the maximum of the
    blocks' constants (``inf`` until every block has one)."""

    def __init__(self, *linops, n_jobs=1):
        if not linops:
            raise ValueError('BlockDiagonalOperator needs at least one operator.')
        self.linops, self.n_jobs = list(linops), n_jobs
        self._rows = _sections([op.shape[0] for op in linops])
        self._cols = _sections([op.shape[1] for op in linops])
        dts = {op.dtype for op in linops}
        super().__init__(shape=(self._rows[-1], self._cols[-1]), dtype=dts.pop() if len(dts) == 1 else None,
                         is_symmetric=all(op.is_symmetric for op in linops),
                         lipschitz_cst=max(op.lipschitz_cst for op in linops))

    def _apply(self, t):
        from ..core.map import _cat
        o = self._cols
        return _cat([op._apply(t[o[i]:o[i + 1]]) for i, op in enumerate(self.linops)], t)

    def _adj(self, t):
        from ..core.map import _cat
        o = self._rows
        return _cat([op._adj(t[o[i]:o[i + 1]]) for i, op in enumerate(self.linops)], t)

    def compute_lipschitz_cst(self, **kwargs):
        for op in self.linops:
            if op.lipschitz_cst == np.inf:
                op.compute_lipschitz_cst(**kwargs)
        self.lipschitz_cst = self.diff_lipschitz_cst = float(max(op.lipschitz_cst for op in self.linops))
