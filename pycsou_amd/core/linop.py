"""Linear operators (mirrors ``pycsou/core/linop.py``).

``LinearOperator`` keeps the reference contract: ``__call__``/``matvec`` and
``adjoint``, ``.H`` (``AdjointLinearOperator`` unless symmetric), ``jacobianT`` = the
adjoint operator, ``lipschitz_cst`` (= ``diff_lipschitz_cst``), sum / composition
algebra (``linop.py:442-553``).  Subclasses implement the device-level ``_apply`` and
``_adj`` on flat tensors.

``compute_lipschitz_cst`` replaces ARPACK ``svds``/``eigsh`` (``linop.py:279-321``,
host loop of tens to hundreds of operator applications) by a device Lanczos iteration
on ``K^T K`` in O(1) vectors: every operator application and the recurrence stay on the
GPU, only the small tridiagonal eigenproblem runs on the host every few steps.

``eigenvals`` / ``singularvals`` (``linop.py:208-219``) replace ARPACK ``eigsh`` / ``svds`` on ``SciOp`` by a
thick-restart Lanczos whose basis, re-orthogonalisation (``csrc/orth.hip``) and operator applications stay on the
device (``_ops.eigsh_restarted``); what it does not serve -- ``which='SM'`` of ``eigenvals``, non-symmetric
operators, other keyword arguments -- still goes to SciPy.

``pinv`` / ``PinvOp`` / ``dagger`` / ``LinOpPinv`` (``linop.py:397-440, 618-629``) replace PyLops'
``NormalEquationsInversion`` (SciPy ``cg`` on the normal equations) by batched conjugate gradients on the device
(``_ops.cg_normal``, ``csrc/cg.hip``); ``todense`` / ``tosparse`` / ``cond`` (``linop.py:323-395``) go through the
dense matrix, which stays on the device.
"""

import warnings
from numbers import Number

import numpy as np
import torch

from .. import _ops as O
from .map import DifferentiableMap, DiffMapComp, DiffMapSum, Map, MapComp, MapSum


def _lanczos_extreme(apply, n, sym=False, tol=1e-9, max_steps=5000, check_every=10, seed=0, device=None):
    """Largest eigenvalue of a PSD Gram operator (or largest |eigenvalue| of a symmetric one) by
    plain Lanczos in fp64 with O(1) memory: three vectors of ``n`` (q_prev, q, w) plus what
    ``apply`` allocates, no re-orthogonalisation (the extreme Ritz value converges regardless;
    lost orthogonality only duplicates it).  The recurrence coefficients stay on the device
    (no host sync per step); every ``check_every`` steps the tridiagonal matrix T is copied to
    the host and its extreme eigenpair (theta, s) computed, with the residual of the Ritz pair
    r = beta_k |s_k| = ||A y - theta y|| (y the Ritz vector; no extra operator application).
    The run stops when r <= tol |theta|, when theta moved by at most ``tol`` (relative) since
    the previous check, or on an invariant subspace (beta ~ 0).

    Returns theta + r when the residual test or stagnation stopped the run (some eigenvalue lies
    within r of the Ritz value; a Ritz value never exceeds the extreme eigenvalue, so the value
    stays on the high side of theta, which keeps tau sigma ||K||^2 <= 1 on the safe side even
    without re-orthogonalisation), and theta itself on an invariant subspace (r = 0: theta is an
    eigenvalue of A).  A stagnated theta is accepted only while its residual is small too
    (r <= sqrt(tol) |theta|, so theta + r over-estimates by at most that much): otherwise the run
    goes on to the residual test or ``max_steps`` (ADVICE r5 -- a loose bound would shrink tau and
    sigma below the reference's svds-based step sizes); a run that ends with a residual above that
    warns.  The
    structured operators of the path (Gradient, derivatives, separable / 1-D convolutions) do not
    come here: their norms are exact (linop/_spectral.py).
    """
    from scipy.linalg import eigh_tridiagonal, eigvalsh_tridiagonal
    dev = O.device() if device is None else device
    g = torch.Generator(device='cpu').manual_seed(seed)
    q = torch.randn(n, generator=g, dtype=torch.float64).to(dev)
    q /= torch.linalg.vector_norm(q)
    q_prev = torch.zeros_like(q)
    steps = max(1, min(int(max_steps), 10 * n + 10))
    alphas = torch.zeros(steps, dtype=torch.float64, device=dev)
    betas = torch.zeros(steps, dtype=torch.float64, device=dev)
    b_prev = torch.zeros((), dtype=torch.float64, device=dev)
    theta, resid, prev = 0.0, 0.0, None
    for j in range(steps):
        w = apply(q).to(torch.float64)
        a = torch.dot(w, q)
        w -= a * q
        w -= b_prev * q_prev
        b = torch.linalg.vector_norm(w)
        alphas[j], betas[j] = a, b
        q_prev, q, b_prev = q, w / b, b
        if (j + 1) % check_every and j + 1 < steps:
            continue
        al = alphas[:j + 1].cpu().numpy()
        be = betas[:j + 1].cpu().numpy()
        scale = max(np.max(np.abs(al[np.isfinite(al)]), initial=0.0), 1e-300)
        bad = np.nonzero(~np.isfinite(be) | (be <= 1e-13 * scale))[0]
        k = int(bad[0]) + 1 if bad.size else j + 1  # T of size k: alphas[:k], betas[:k-1]
        if k > 1:
            # the extreme eigenvalue, then its eigenvector alone (O(k) per check, not the O(k^2)
            # of a full eigendecomposition of T)
            i = k - 1
            if sym:
                ends = eigvalsh_tridiagonal(al[:k], be[:k - 1], select='i', select_range=(0, 0)), \
                    eigvalsh_tridiagonal(al[:k], be[:k - 1], select='i', select_range=(k - 1, k - 1))
                i = 0 if abs(ends[0][0]) > abs(ends[1][0]) else k - 1
            ev, S = eigh_tridiagonal(al[:k], be[:k - 1], select='i', select_range=(i, i))
            theta = float(abs(ev[0])) if sym else float(ev[0])
            # residual of the Ritz pair: the next beta times the last component of its vector
            resid = 0.0 if bad.size else float(abs(be[k - 1] * S[-1, 0]))
        else:
            theta, resid = (float(abs(al[0])) if sym else float(al[0])), (0.0 if bad.size else float(abs(be[0])))
        if bad.size:
            return theta
        if resid <= tol * abs(theta):
            return theta + resid
        loose = resid > np.sqrt(tol) * abs(theta)
        if prev is not None and abs(theta - prev) <= tol * abs(theta) and not loose:
            return theta + resid
        prev = theta
    if resid > np.sqrt(tol) * abs(theta):
        warnings.warn(f'Lanczos: {steps} steps left the Ritz residual at {resid / max(abs(theta), 1e-300):.2e} of '
                      f'theta; the returned bound theta + r may over-estimate the norm by that much')
    return theta + resid


class LinearOperator(DifferentiableMap):
    """Base class for linear operators (``pycsou/core/linop.py:21-485``)."""

    def __init__(self, shape, dtype=None, is_explicit=False, is_dense=False, is_sparse=False, is_dask=False,
                 is_symmetric=False, lipschitz_cst=np.inf):
        DifferentiableMap.__init__(self, shape=shape, is_linear=True, lipschitz_cst=lipschitz_cst,
                                   diff_lipschitz_cst=lipschitz_cst)
        self.dtype = dtype
        self.is_explicit = is_explicit
        self.is_dense = is_dense
        self.is_sparse = is_sparse
        self.is_dask = is_dask
        self.is_symmetric = is_symmetric
        self.is_square = shape[0] == shape[1]

    # -- device layer
    def _adj(self, t):
        raise NotImplementedError

    def _jacT(self, t=None):
        return self.get_adjointOp()

    def _apply_cols(self, T, axis, adjoint=False):
        """The operator (or its adjoint) along ``axis`` of a contiguous 2-D device tensor: a contiguous result
        with that axis replaced by the range dimension (the device counterpart of ``Map.apply_along_axis``).
        The default is a loop over the lines on the device -- slice, ``_apply`` / ``_adj``, stack -- with no host
        copy and no synchronisation; operators with a batched form override it."""
        f = self._adj if adjoint else self._apply
        n_out = self.shape[1] if adjoint else self.shape[0]
        if axis == 0:
            if T.shape[1] == 0:
                return torch.empty((n_out, 0), dtype=T.dtype, device=T.device)
            return torch.stack([f(T[:, j].contiguous()) for j in range(T.shape[1])], dim=1).contiguous()
        if T.shape[0] == 0:
            return torch.empty((0, n_out), dtype=T.dtype, device=T.device)
        return torch.stack([f(T[i]) for i in range(T.shape[0])], dim=0)

    def _apply_cols_acc(self, T, axis, adjoint, acc):
        """``acc + _apply_cols(T, axis, adjoint)``; ``acc`` may be overwritten with the result."""
        return O.add(acc, self._apply_cols(T, axis, adjoint))

    def _apply_mid(self, T, adjoint=False):
        """Along the middle axis of a contiguous (a, p, b) device tensor, through ``_apply_cols``."""
        a, p, b = T.shape
        if b == 1:
            return self._apply_cols(T.reshape(a, p), 1, adjoint).reshape(a, -1, 1)
        if a == 1:
            return self._apply_cols(T.reshape(p, b), 0, adjoint).reshape(1, -1, b)
        Z = self._apply_cols(T.permute(1, 0, 2).reshape(p, a * b), 0, adjoint)
        return Z.reshape(-1, a, b).permute(1, 0, 2).contiguous()

    # -- public layer
    def matvec(self, x):
        return self.__call__(x)

    def adjoint(self, y):
        if isinstance(y, Number):
            y = np.asarray([y], dtype=float)
        return O.like(self._adj(O.to_dev(y)), y)

    def transpose(self, y):
        return self.adjoint(y)  # real operators only

    def jacobianT(self, arg=None):
        return self.get_adjointOp()

    def get_adjointOp(self):
        return self if self.is_symmetric else AdjointLinearOperator(self)

    @property
    def H(self):
        return self.get_adjointOp()

    def get_transposeOp(self):
        return TransposeLinearOperator(self)

    @property
    def T(self):
        return self.get_transposeOp()

    @property
    def RangeGram(self):
        return SymmetricLinearOperator(self * self.H)

    @property
    def DomainGram(self):
        return SymmetricLinearOperator(self.H * self)

    # -- spectral helpers
    def _compute_dtype(self):
        return O.torch_dtype(self.dtype)

    def tosciop(self):
        import scipy.sparse.linalg as spls
        return spls.LinearOperator(dtype=np.float64, shape=self.shape, matvec=lambda v: self.matvec(v),
                                   rmatvec=lambda v: self.adjoint(v))

    @property
    def SciOp(self):
        return self.tosciop()

    _SPECTRAL_KW = ('tol', 'ncv', 'maxiter', 'v0')

    def _device_spectral(self, n, k, kwargs, vectors_kw):
        """The keyword arguments of ``_ops.eigsh_restarted`` when the device Lanczos serves this call, else None
        (SciPy's path): only ``tol``, ``ncv``, ``maxiter``, ``v0`` and a false ``vectors_kw`` are understood, and
        the basis must fit the kernels' limit."""
        if any(key not in self._SPECTRAL_KW + (vectors_kw,) for key in kwargs) or kwargs.get(vectors_kw, False):
            return None
        kw = {key: kwargs[key] for key in self._SPECTRAL_KW if key in kwargs}
        if isinstance(k, (int, np.integer)) and O.spectral_ncv(n, max(int(k), 0), kw.get('ncv')) > O.ORTH_MAX_M:
            return None
        return kw

    def eigenvals(self, k, which='LM', **kwargs):
        """``linop.py:208-213``.  A symmetric operator with ``which`` in LM / LA / SA / BE runs the thick-restart
        Lanczos on the device (``_ops.eigsh_restarted``: ``tol``, ``ncv``, ``maxiter`` and ``v0`` as ``eigsh``
        takes them, ascending values back); ``which='SM'`` (no shift-invert on the device), any other keyword
        argument, ``ncv`` above 256 and non-symmetric operators (complex eigenvalues) take SciPy's ARPACK wrappers
        through ``SciOp``."""
        import scipy.sparse.linalg as spls
        if self.is_symmetric:
            kw = self._device_spectral(self.shape[1], k, kwargs, 'return_eigenvectors') \
                if which in O.SPECTRAL_WHICH else None
            if kw is not None:
                n, cdt = self.shape[1], self._compute_dtype()
                if not 0 < k < n:
                    raise ValueError(f'k must satisfy 0 < k < {n}, got k = {k}')
                return O.eigsh_restarted(lambda v: self._apply(v.to(cdt)).to(torch.float64), n, k, which, **kw)
            return spls.eigsh(A=self.SciOp, k=k, which=which, return_eigenvectors=False, **kwargs)
        if self.is_square:
            return spls.eigs(A=self.SciOp, k=k, which=which, return_eigenvectors=False, **kwargs)
        raise NotImplementedError('The function eigenvals is only for square linear operator. For non square linear '
                                  'operators, use the method singularvals.')

    def singularvals(self, k, which='LM', **kwargs):
        """``linop.py:215-219``.  ``which`` LM / SM: the device Lanczos on the smaller Gram operator (A^T A or
        A A^T, as ``svds`` does), LA / SA there, and the roots of its eigenvalues, ascending; ``tol`` is that of
        the Gram eigenproblem.  Other keyword arguments than ``tol``, ``ncv``, ``maxiter``, ``v0``: SciPy's
        ``svds`` through ``SciOp``."""
        import scipy.sparse.linalg as spls
        kw = self._device_spectral(min(self.shape), k, kwargs, 'return_singular_vectors') \
            if which in ('LM', 'SM') else None
        if kw is None:
            return spls.svds(A=self.SciOp, k=k, which=which, return_singular_vectors=False, **kwargs)
        n, cdt = min(self.shape), self._compute_dtype()
        if not 1 <= k < n:
            raise ValueError(f'k must satisfy 1 <= k < min(shape) = {n}, got k = {k}')
        if self.shape[0] >= self.shape[1]:
            gram = lambda v: self._adj(self._apply(v.to(cdt))).to(torch.float64)    # noqa: E731
        else:
            gram = lambda v: self._apply(self._adj(v.to(cdt))).to(torch.float64)    # noqa: E731
        theta = O.eigsh_restarted(gram, n, k, 'LA' if which == 'LM' else 'SA', **kw)
        return np.sqrt(np.maximum(theta, 0.0))

    def compute_lipschitz_cst(self, tol=1e-9, max_steps=5000, **kwargs):
        """Operator norm ``||K||_2`` (``pycsou/core/linop.py:279-321``: ARPACK ``svds`` / ``eigsh``
        with k=1) by device Lanczos on ``K^T K`` (or ``|eig|`` if symmetric) in bounded memory
        (a few vectors of the domain size, whatever the operator's size).  Other ARPACK keyword
        arguments are accepted and ignored; ``tol`` is the relative residual (or change of the
        estimate between checks) at which the iteration stops; the value is accurate to about
        ``tol`` relative (see _lanczos_extreme).  Structured operators override this with their
        exact norms (linop/_spectral.py)."""
        if self.is_symmetric:
            lam = _lanczos_extreme(lambda v: self._apply(v), self.shape[1], sym=True, tol=tol, max_steps=max_steps)
            self.lipschitz_cst = float(abs(lam))
        else:
            lam = _lanczos_extreme(lambda v: self._adj(self._apply(v)), self.shape[1], tol=tol, max_steps=max_steps)
            self.lipschitz_cst = float(np.sqrt(max(lam, 0.0)))
        self.diff_lipschitz_cst = self.lipschitz_cst

    # -- explicit forms, condition number, pseudo-inverse (linop.py:323-440)
    TODENSE_BLOCK = 1024    # identity columns per _apply_cols call of todense
    COND_MAX = 2048         # largest min(shape) cond() takes

    def todense(self, dtype=None):
        """The operator as a ``DenseLinearOperator`` whose matrix stays on the device (``linop.py:323-334``):
        ``_apply_cols`` on blocks of at most ``TODENSE_BLOCK`` columns of the identity, in the operator's
        compute dtype unless ``dtype`` (a torch dtype) says otherwise."""
        from ..linop.base import DenseLinearOperator
        dt = self._compute_dtype() if dtype is None else dtype
        m, n = self.shape
        dev = O.device()
        M = torch.empty((m, n), dtype=dt, device=dev)
        for c0 in range(0, n, self.TODENSE_BLOCK):
            k = min(self.TODENSE_BLOCK, n - c0)
            E = torch.zeros((n, k), dtype=dt, device=dev)
            E[c0:c0 + k] = torch.eye(k, dtype=dt, device=dev)
            M[:, c0:c0 + k] = self._apply_cols(E, 0)
        return DenseLinearOperator(M, is_symmetric=self.is_symmetric)

    def tosparse(self):
        """``linop.py:336-347``: the CSR matrix of ``todense()``."""
        import scipy.sparse as sp
        from ..linop.base import SparseLinearOperator
        return SparseLinearOperator(sp.csr_matrix(self.todense().mat.cpu().numpy()), is_symmetric=self.is_symmetric)

    def cond(self, **kwargs):
        """Condition number (``linop.py:381-395``): largest over smallest nonzero singular value (those above
        ``max(shape) eps sigma_max``, NumPy's rank convention), from ``torch.linalg.svdvals`` of the fp64
        ``todense()``.  The dense route serves ``min(shape) <= COND_MAX``; PyLops' keyword arguments are accepted
        and ignored."""
        if min(self.shape) > self.COND_MAX:
            raise NotImplementedError(f'cond() forms the dense matrix and serves min(shape) <= {self.COND_MAX}, '
                                      f'got shape {self.shape}')
        s = torch.linalg.svdvals(self.todense(dtype=torch.float64).mat).cpu().numpy()
        if s.size == 0 or not s[0] > 0:
            return float('inf')
        s = s[s > max(self.shape) * np.finfo(np.float64).eps * s[0]]
        return float(s[0] / s[-1])

    def pinv(self, y, eps=0, **kwargs):
        """Pseudo-inverse at ``y`` (``linop.py:397-420``): conjugate gradients on the normal equations
        ``(A^T A + eps^2 I) x = A^T y`` on the device (``_ops.cg_normal``) with the semantics of
        ``scipy.sparse.linalg.cg``, which PyLops' ``NormalEquationsInversion`` hands its keyword arguments to:
        ``rtol`` (or ``tol``), ``atol``, ``maxiter`` and ``x0`` are honoured, any other is accepted and ignored."""
        if isinstance(y, Number):
            y = np.asarray([y], dtype=float)
        t = O.to_dev(y)
        kwargs = dict(kwargs)
        x0 = kwargs.pop('x0', None)
        x0 = None if x0 is None else O.to_dev(x0, t.dtype)
        return O.like(LinOpPinv(self, eps).solve(t.reshape(1, -1), x0=x0, **kwargs)[0].reshape(-1), y)

    @property
    def PinvOp(self):
        return LinOpPinv(self)

    @property
    def dagger(self):
        return self.PinvOp

    @property
    def RowProjector(self):
        return SymmetricLinearOperator(self.dagger * self)

    @property
    def ColProjector(self):
        return SymmetricLinearOperator(self * self.dagger)

    # -- algebra (linop.py:442-485)
    def __add__(self, other):
        if isinstance(other, LinearOperator):
            return LinOpSum(self, other)
        if isinstance(other, DifferentiableMap):
            return DiffMapSum(self, other)
        if isinstance(other, Map):
            return MapSum(self, other)
        raise NotImplementedError

    def __mul__(self, other):
        if isinstance(other, Number):
            from ..linop.base import HomothetyMap
            other = HomothetyMap(constant=other, size=self.shape[1])
        if O.is_array(other):
            return self(other)
        if isinstance(other, LinearOperator):
            return LinOpComp(self, other)
        if isinstance(other, DifferentiableMap):
            return DiffMapComp(self, other)
        if isinstance(other, Map):
            return MapComp(self, other)
        raise NotImplementedError

    def __rmul__(self, other):
        if isinstance(other, Number):
            from ..linop.base import HomothetyMap
            other = HomothetyMap(constant=other, size=self.shape[0])
        if isinstance(other, LinearOperator):
            return LinOpComp(other, self)
        if isinstance(other, DifferentiableMap):
            return DiffMapComp(other, self)
        if isinstance(other, Map):
            return MapComp(other, self)
        raise NotImplementedError


class AdjointLinearOperator(LinearOperator):
    """``linop.py:488-506``."""

    def __init__(self, LinOp):
        super().__init__(shape=(LinOp.shape[1], LinOp.shape[0]), dtype=LinOp.dtype, is_explicit=LinOp.is_explicit,
                         is_dask=LinOp.is_dask, is_dense=LinOp.is_dense, is_sparse=LinOp.is_sparse,
                         is_symmetric=LinOp.is_symmetric)
        self.Linop = LinOp

    def _apply(self, t):
        return self.Linop._adj(t)

    def _adj(self, t):
        return self.Linop._apply(t)

    def _apply_cols(self, T, axis, adjoint=False):
        return self.Linop._apply_cols(T, axis, not adjoint)

    def compute_lipschitz_cst(self, **kwargs):
        if self.Linop.lipschitz_cst != np.inf:
            self.lipschitz_cst = self.Linop.lipschitz_cst
        else:
            LinearOperator.compute_lipschitz_cst(self, **kwargs)


class TransposeLinearOperator(AdjointLinearOperator):
    """``linop.py:509-521`` (real operators: transpose == adjoint)."""


class LinOpSum(LinearOperator, DiffMapSum):
    """``linop.py:524-537``."""

    def __init__(self, LinOp1, LinOp2, dtype=None):
        dtype = LinOp1.dtype if LinOp1.dtype is LinOp2.dtype else dtype
        DiffMapSum.__init__(self, map1=LinOp1, map2=LinOp2)
        LinearOperator.__init__(self, shape=self.shape, dtype=dtype, is_explicit=LinOp1.is_explicit & LinOp2.is_explicit,
                                is_dask=LinOp1.is_dask & LinOp2.is_dask, is_dense=LinOp1.is_dense & LinOp2.is_dense,
                                is_sparse=LinOp1.is_sparse & LinOp2.is_sparse,
                                is_symmetric=LinOp1.is_symmetric & LinOp2.is_symmetric,
                                lipschitz_cst=self.lipschitz_cst)
        self.LinOp1, self.LinOp2 = LinOp1, LinOp2

    def _apply(self, t):
        return O.add(self.LinOp1._apply(t), self.LinOp2._apply(t))

    def _adj(self, t):
        return O.add(self.LinOp1._adj(t), self.LinOp2._adj(t))

    def _apply_cols(self, T, axis, adjoint=False):
        return self.LinOp2._apply_cols_acc(T, axis, adjoint, self.LinOp1._apply_cols(T, axis, adjoint))


class LinOpComp(LinearOperator, DiffMapComp):
    """``linop.py:540-553``."""

    def __init__(self, LinOp1, LinOp2, dtype=None):
        dtype = LinOp1.dtype if LinOp1.dtype is LinOp2.dtype else dtype
        DiffMapComp.__init__(self, map1=LinOp1, map2=LinOp2)
        LinearOperator.__init__(self, shape=self.shape, dtype=dtype, is_explicit=LinOp1.is_explicit & LinOp2.is_explicit,
                                is_dask=LinOp1.is_dask & LinOp2.is_dask, is_dense=LinOp1.is_dense & LinOp2.is_dense,
                                is_sparse=LinOp1.is_sparse & LinOp2.is_sparse,
                                is_symmetric=LinOp1.is_symmetric & LinOp2.is_symmetric,
                                lipschitz_cst=self.lipschitz_cst)
        self.LinOp1, self.LinOp2 = LinOp1, LinOp2

    def _apply(self, t):
        return self.LinOp1._apply(self.LinOp2._apply(t))

    def _adj(self, t):
        return self.LinOp2._adj(self.LinOp1._adj(t))

    def _apply_cols(self, T, axis, adjoint=False):
        if adjoint:
            return self.LinOp2._apply_cols(self.LinOp1._apply_cols(T, axis, True), axis, True)
        return self.LinOp1._apply_cols(self.LinOp2._apply_cols(T, axis), axis)

    def _jacT(self, t=None):
        return self.get_adjointOp()

    def _factors(self):
        out = []
        for op in (self.LinOp1, self.LinOp2):
            out.extend(op._factors() if isinstance(op, LinOpComp) else [op])
        return out

    def compute_lipschitz_cst(self, **kwargs):
        """A composition of Convolve1D along distinct axes of one shape (the reference's only 3-D
        blur, pycsou/linop/conv.py:20-164) is a Kronecker product: its norm is the product of the
        factors' exact norms.  Anything else: the device Lanczos."""
        from ..linop.conv import Convolve1DOp
        f = self._factors()
        if all(isinstance(o, Convolve1DOp) for o in f) and len({o.dims for o in f}) == 1 \
                and len({o.axis for o in f}) == len(f):
            self.lipschitz_cst = self.diff_lipschitz_cst = float(np.sqrt(np.prod([o.norm2() for o in f])))
            return
        LinearOperator.compute_lipschitz_cst(self, **kwargs)


class SymmetricLinearOperator(LinearOperator):
    """``linop.py:556-571``."""

    def __init__(self, LinOp):
        if LinOp.shape[0] != LinOp.shape[1]:
            raise TypeError('The input linear operator is not symmetric.')
        super().__init__(shape=LinOp.shape, dtype=LinOp.dtype, is_explicit=LinOp.is_explicit, is_dask=LinOp.is_dask,
                         is_dense=LinOp.is_dense, is_sparse=LinOp.is_sparse, is_symmetric=True,
                         lipschitz_cst=LinOp.lipschitz_cst)
        self.LinOp = LinOp

    def _apply(self, t):
        return self.LinOp._apply(t)

    def _adj(self, t):
        return self.LinOp._apply(t)

    def _apply_cols(self, T, axis, adjoint=False):
        return self.LinOp._apply_cols(T, axis)


class UnitaryOperator(LinearOperator):
    """``linop.py:574-615``."""

    def __init__(self, size, dtype=None, is_explicit=False, is_dense=False, is_sparse=False, is_dask=False,
                 is_symmetric=False):
        super().__init__(shape=(size, size), dtype=dtype, is_explicit=is_explicit, is_dense=is_dense,
                         is_sparse=is_sparse, is_dask=is_dask, is_symmetric=is_symmetric)
        self.size = size
        self.lipschitz_cst = self.diff_lipschitz_cst = 1

    def compute_lipschitz_cst(self, **kwargs):
        self.lipschitz_cst = self.diff_lipschitz_cst = 1

    def singularvals(self, k, which='LM', **kwargs):
        if k > min(self.shape):
            raise ValueError('The number of singular values must not exceed the smallest dimension size.')
        return np.ones(shape=(k,))

    def eigenvals(self, k, which='LM', **kwargs):
        return self.singularvals(k=k)

    def pinv(self, y, eps=0, **kwargs):
        return self.adjoint(y)

    @property
    def PinvOp(self):
        return self.H

    def cond(self, **kwargs):
        return 1


class LinOpPinv(LinearOperator):
    """Pseudo-inverse of ``LinOp`` with Tikhonov damping ``eps`` as an operator (``linop.py:618-629``): applying
    it solves ``(A^T A + eps^2 I) x = A^T y`` by conjugate gradients on the device (``_ops.cg_normal``; SciPy's
    ``cg`` defaults: x0 = 0, rtol = 1e-5, maxiter = 10 n).  ``_apply_cols`` solves all the lines of a matrix as
    one batch -- what ``KroneckerProduct.PinvOp`` runs on -- and the adjoint is the pseudo-inverse of ``LinOp.H``.
    ``last``: iteration count and ``CGInfo`` of the most recent solve.  A system whose ``p . N p`` is not
    positive (a breakdown, where SciPy would return inf / NaN) stops where it is, with a warning."""

    def __init__(self, LinOp, eps=0):
        self.LinOp = LinOp
        self.eps = eps
        super().__init__(shape=LinOp.H.shape, dtype=LinOp.dtype, is_explicit=False, is_dense=False, is_dask=False,
                         is_symmetric=LinOp.is_symmetric)
        self._plans = {}
        self._adjoint = None
        self.last = None

    def solve(self, Y, x0=None, **kwargs):
        """The rows of the (nb, m) device tensor ``Y``: (X, iterations, CGInfo); ``kwargs`` as ``pinv`` takes."""
        rtol = kwargs.get('rtol', kwargs.get('tol', 1e-5))
        opts = {k: kwargs[k] for k in ('chunk', 'use_graph') if k in kwargs}
        X, it, info = O.cg_normal(self.LinOp, Y, self.eps, rtol=rtol, atol=kwargs.get('atol', 0.0),
                                  maxiter=kwargs.get('maxiter'), x0=x0, plans=self._plans, **opts)
        if info.breakdown.any():
            warnings.warn(f'pinv: conjugate gradients broke down (p . N p not positive) in '
                          f'{int(info.breakdown.sum())} of {len(info.breakdown)} system(s); their iterates are '
                          f'returned as they stood')
        self.last = (it, info)
        return X, it, info

    def _apply(self, t):
        return self.solve(t.reshape(1, -1))[0].reshape(-1)

    def _adj(self, t):
        return self.get_adjointOp()._apply(t)

    def get_adjointOp(self):
        if self.is_symmetric:
            return self
        if self._adjoint is None:
            self._adjoint = LinOpPinv(self.LinOp.H, self.eps)
            self._adjoint._adjoint = self
        return self._adjoint

    def _apply_cols(self, T, axis, adjoint=False):
        if adjoint and not self.is_symmetric:
            return self.get_adjointOp()._apply_cols(T, axis)
        if axis == 1:
            return self.solve(T)[0]
        return self.solve(T.t().contiguous())[0].t().contiguous()
