"""Finite-difference operators on the GPU (``pycsou/linop/diff.py`` hot-path subset).

``FirstDerivative`` (``diff.py:24-130``), ``Gradient`` (``diff.py:777-882``) and
``Laplacian`` (``diff.py:885-957``) keep the reference signatures and defaults and the
PyLops 1.x arithmetic they delegate to (forward / backward / 3-point centred stencils,
one-sided ends with ``edge=True``, ``Gradient`` = stacked ``[D_0 x; D_1 x; ...]``,
adjoint = accumulated ``sum_k D_k^T z_k``).  Matvec and adjoint are the gfx950 kernels
``pcs_deriv1_*``, ``pcs_grad_*``, ``pcs_lap_*``.

``FirstDirectionalDerivative`` / ``SecondDirectionalDerivative`` / ``DirectionalGradient`` /
``DirectionalLaplacian`` (``diff.py:380-774``) run the fused ``pcs_dirderiv_*`` kernels and
``Integration1D`` (``diff.py:1071-1137``) the scan ``pcs_cumsum``.
"""

from numbers import Number

import numpy as np
import torch

from .. import _ops as O
from ..core.linop import LinearOperator
from ..util.misc import peaks  # noqa: F401  -- the reference's doctests of this module use it
from . import _spectral as S


def _steps(step, nd):
    if isinstance(step, Number):
        return [float(step)] * nd
    step = [float(s) for s in step]
    if len(step) != nd:
        raise ValueError('step must be a float or one value per axis')
    return step


class _DiffOp(LinearOperator):
    def __init__(self, shape, size, dtype):
        super().__init__(shape=shape, dtype=np.dtype(dtype), is_explicit=False, lipschitz_cst=np.inf)
        self._size = size


class FirstDerivativeOp(_DiffOp):
    """``pylops.FirstDerivative`` restated on the GPU."""

    def __init__(self, size, shape=None, axis=0, step=1.0, edge=True, dtype='float64', kind='forward'):
        if kind not in ('forward', 'centered', 'backward'):
            raise NotImplementedError('kind must be forward, centered, or backward')
        dims = (size,) if shape is None else tuple(int(s) for s in shape)
        if int(np.prod(dims)) != size:
            raise ValueError('shape and size are not compatible')
        if not 1 <= len(dims) <= 32:
            raise NotImplementedError('FirstDerivative supports 1-D to 32-D arrays')
        super().__init__((size, size), size, dtype)
        self.dims, self.axis, self.step, self.edge, self.kind = dims, int(axis), float(step), bool(edge), kind

    def _apply(self, t):
        return O.deriv1(t, self.dims, self.axis, self.step, self.kind, self.edge)

    def _adj(self, t):
        return O.deriv1(t, self.dims, self.axis, self.step, self.kind, self.edge, adjoint=True)

    def _apply_cols(self, T, axis, adjoint=False):
        if len(self.dims) != 1:
            return LinearOperator._apply_cols(self, T, axis, adjoint)
        return O.deriv1(T, tuple(T.shape), axis, self.step, self.kind, self.edge, adjoint=adjoint)

    def compute_lipschitz_cst(self, **kwargs):
        """Exact ||D|| = sqrt(lambda_max(D_1^T D_1)) of the 1-D stencil along the axis (K = I (x) D_1 (x) I;
        linop/_spectral.py), in place of the reference's ARPACK svds (pycsou/core/linop.py:279-321)."""
        self.lipschitz_cst = self.diff_lipschitz_cst = float(
            np.sqrt(S.deriv1_norm2(self.dims[self.axis], self.kind, self.edge, self.step)))


def FirstDerivative(size, shape=None, axis=0, step=1.0, edge=True, dtype='float64', kind='forward'):
    """``pycsou/linop/diff.py:24-130``."""
    return FirstDerivativeOp(size, shape=shape, axis=axis, step=step, edge=edge, dtype=dtype, kind=kind)


class GradientOp(_DiffOp):
    """``pylops.Gradient`` = ``VStack([FirstDerivative(dir=k)])`` on the GPU."""

    def __init__(self, shape, step=1.0, edge=True, dtype='float64', kind='centered'):
        if kind not in ('forward', 'centered', 'backward'):
            raise NotImplementedError('kind must be forward, centered, or backward')
        dims = tuple(int(s) for s in shape)
        if not 1 <= len(dims) <= 32:
            raise NotImplementedError('Gradient supports 1-D to 32-D arrays')
        N = int(np.prod(dims))
        super().__init__((len(dims) * N, N), N, dtype)
        self.dims, self.steps, self.edge, self.kind = dims, _steps(step, len(dims)), bool(edge), kind

    def _apply(self, t):
        return O.grad_fwd(t, self.dims, self.steps, self.kind, self.edge)

    def _adj(self, t):
        return O.grad_adj(t, self.dims, self.steps, self.kind, self.edge)

    def compute_lipschitz_cst(self, **kwargs):
        """Exact ||K||: K^T K = sum_k I (x) D_k^T D_k (x) I is a Kronecker sum, so ||K||^2 = sum_k
        lambda_max(D_k^T D_k) over the 1-D stencils of the axes (linop/_spectral.py; forward /
        backward: 4 sin^2(pi (n-1) / 2n) / h^2 per axis), in place of the reference's ARPACK svds
        (pycsou/core/linop.py:279-321)."""
        self.lipschitz_cst = self.diff_lipschitz_cst = float(np.sqrt(sum(
            S.deriv1_norm2(n, self.kind, self.edge, h) for n, h in zip(self.dims, self.steps))))


def Gradient(shape, step=1., edge=True, dtype='float64', kind='centered'):
    """``pycsou/linop/diff.py:777-882``."""
    return GradientOp(shape, step=step, edge=edge, dtype=dtype, kind=kind)


class LaplacianOp(_DiffOp):
    """``pylops.Laplacian`` (2-D): ``w0 * D2_0 + w1 * D2_1`` on the GPU."""

    def __init__(self, shape, weights=(1, 1), step=1., edge=True, dtype='float64'):
        dims = tuple(int(s) for s in shape)
        if len(dims) != 2:
            raise NotImplementedError('Laplacian is 2-D in the reference (pycsou/linop/diff.py:885)')
        N = int(np.prod(dims))
        super().__init__((N, N), N, dtype)
        self.dims, self.weights, self.steps, self.edge = dims, tuple(float(w) for w in weights), _steps(step, 2), bool(edge)

    def _apply(self, t):
        return O.lap(t, self.dims, self.weights, self.steps, self.edge)

    def _adj(self, t):
        return O.lap(t, self.dims, self.weights, self.steps, self.edge, adjoint=True)


def Laplacian(shape, weights=(1, 1), step=1., edge=True, dtype='float64'):
    """``pycsou/linop/diff.py:885-957``."""
    return LaplacianOp(shape, weights=weights, step=step, edge=edge, dtype=dtype)


class SecondDerivativeOp(_DiffOp):
    """``pylops.SecondDerivative`` restated on the GPU (``pcs_deriv2_*``)."""

    def __init__(self, size, shape=None, axis=0, step=1.0, edge=True, dtype='float64'):
        dims = (size,) if shape is None else tuple(int(s) for s in shape)
        if int(np.prod(dims)) != size:
            raise ValueError('shape and size are not compatible')
        if not 1 <= len(dims) <= 32:
            raise NotImplementedError('SecondDerivative supports 1-D to 32-D arrays')
        super().__init__((size, size), size, dtype)
        self.dims, self.axis, self.step, self.edge = dims, int(axis), float(step), bool(edge)

    def _apply(self, t):
        return O.deriv2(t, self.dims, self.axis, self.step, self.edge)

    def _adj(self, t):
        return O.deriv2(t, self.dims, self.axis, self.step, self.edge, adjoint=True)

    def _apply_cols(self, T, axis, adjoint=False):
        if len(self.dims) != 1:
            return LinearOperator._apply_cols(self, T, axis, adjoint)
        return O.deriv2(T, tuple(T.shape), axis, self.step, self.edge, adjoint=adjoint)

    def compute_lipschitz_cst(self, **kwargs):
        """Exact ||D2|| of the 1-D second-difference stencil along the axis (linop/_spectral.py)."""
        self.lipschitz_cst = self.diff_lipschitz_cst = float(
            np.sqrt(S.deriv2_norm2(self.dims[self.axis], self.edge, self.step)))


def SecondDerivative(size, shape=None, axis=0, step=1.0, edge=True, dtype='float64'):
    """``pycsou/linop/diff.py:133-219``."""
    return SecondDerivativeOp(size, shape=shape, axis=axis, step=step, edge=edge, dtype=dtype)


def _kill_edges(Dgen, shape, axis, order, kind):
    from .base import DiagonalOperator
    k = np.ones(shape=Dgen.shape[0]) if shape is None else np.ones(shape=shape)
    if axis > 0:
        k = np.swapaxes(k, axis, 0)
    if kind == 'forward':
        k[-order:] = 0
    elif kind == 'backward':
        k[:order] = 0
    elif kind == 'centered':
        k[-order:] = 0
        k[:order] = 0
    if axis > 0:
        k = np.swapaxes(k, 0, axis)
    return DiagonalOperator(k.reshape(-1)) * Dgen


def GeneralisedDerivative(size, shape=None, axis=0, step=1.0, edge=True, dtype='float64', kind_op='iterated',
                          kind_diff='centered', **kwargs):
    """``pycsou/linop/diff.py:222-377``: ``D^N`` ('iterated'), ``(a^2 I - D2)^N`` ('sobolev'),
    ``(a I + D)^N`` ('exponential') or ``P(D)`` ('polynomial'), with the unreliable edge samples
    zeroed by a diagonal mask."""
    from .base import IdentityOperator, PolynomialLinearOperator
    D = FirstDerivative(size=size, shape=shape, axis=axis, step=step, edge=edge, dtype=dtype, kind=kind_diff)
    D.is_symmetric = False
    D2 = SecondDerivative(size=size, shape=shape, axis=axis, step=step, edge=edge, dtype=dtype)
    if kind_op == 'iterated':
        N = kwargs['order']
        Dgen, order = D ** N, N
    elif kind_op == 'sobolev':
        I = IdentityOperator(size=size)
        N = kwargs['order']
        Dgen, order = ((kwargs['constant'] ** 2) * I - D2) ** N, 2 * N
    elif kind_op == 'exponential':
        I = IdentityOperator(size=size)
        N = kwargs['order']
        Dgen, order = (kwargs['constant'] * I + D) ** N, N
    elif kind_op == 'polynomial':
        coeffs = kwargs['coeffs']
        Dgen, order = PolynomialLinearOperator(LinOp=D, coeffs=coeffs), len(coeffs) - 1
    else:
        raise NotImplementedError(
            'Supported generalised derivative types are: iterated, sobolev, exponential, polynomial.')
    return _kill_edges(Dgen, shape, axis, order, kind_diff)


def GeneralisedLaplacian(shape=None, step=1., edge=True, dtype='float64', kind='iterated', **kwargs):
    """``pycsou/linop/diff.py:960-1068``: ``Delta^N`` ('iterated'), ``(a^2 I - Delta)^N``
    ('sobolev') or ``P(Delta)`` ('polynomial') of the 2-D ``Laplacian``, with ``order`` edge samples
    zeroed along every axis."""
    from .base import DiagonalOperator, IdentityOperator, PolynomialLinearOperator
    Delta = Laplacian(shape=shape, step=step, edge=edge, dtype=dtype)
    Delta.is_symmetric = True
    if kind == 'iterated':
        N = kwargs['order']
        Dgen, order = Delta ** N, 2 * N
    elif kind == 'sobolev':
        I = IdentityOperator(size=shape[0] * shape[1])
        N = kwargs['order']
        Dgen, order = ((kwargs['constant'] ** 2) * I - Delta) ** N, 2 * N
    elif kind == 'polynomial':
        coeffs = kwargs['coeffs']
        Dgen, order = PolynomialLinearOperator(LinOp=Delta, coeffs=coeffs), 2 * (len(coeffs) - 1)
    else:
        raise NotImplementedError('Supported generalised derivative types are: iterated, sobolev, polynomial.')
    k = np.ones(shape=shape)
    for ax in range(len(shape)):
        k = np.swapaxes(k, ax, 0)
        k[-order:] = 0
        k[:order] = 0
        k = np.swapaxes(k, 0, ax)
    return DiagonalOperator(k.reshape(-1)) * Dgen


def _interior_mask(dims, width):
    """1 where a sample lies at least ``width`` samples from both ends of every axis, else 0 (flat float64): the
    coordinate test of ``killed()`` in csrc/stencil.hip.  An axis shorter than ``2 * width`` leaves nothing."""
    m = np.ones(dims)
    for ax, n in enumerate(dims):
        i = np.arange(n)
        inside = ((i >= width) & (i < n - width)).astype(np.float64)
        m *= inside.reshape([n if a == ax else 1 for a in range(len(dims))])
    return m.reshape(-1)


def _directions(directions, dims):
    """``directions`` as PyLops ravels it: one direction (``ndim`` values) or a field of ``ndim * N`` values in
    [k][p] order, given as ``(ndim, N)`` or ``(ndim, *shape)``.  Returns (flat float64 array, is_field)."""
    v = np.asarray(directions, dtype=np.float64).reshape(-1)
    nd, N = len(dims), int(np.prod(dims))
    if v.size == nd:
        return v, False
    if v.size == nd * N:
        return v, True
    raise ValueError(f'directions must hold {nd} values (one direction) or {nd} x {N} values (one per entry)')


class FirstDirectionalDerivativeOp(_DiffOp):
    """``pylops.FirstDirectionalDerivative`` (1.x: ``Sum(axis 0) * Diagonal(v) * Gradient``) on the GPU:
    ``y = (v_0 . D_0 x + v_1 . D_1 x) + v_2 . D_2 x``, adjoint ``sum_k D_k^T (v_k . y)`` in axis order.  One fused
    launch each way for 1-D to 3-D shapes (``pcs_dirderiv_*``); beyond 3-D the composition of ``Gradient``,
    ``pcs_mul`` and adds.  ``directions`` is used as given (no normalisation) and held on the device in the
    operator's dtype."""

    def __init__(self, shape, directions, step=1., edge=True, dtype='float64', kind='centered'):
        if kind not in ('forward', 'centered', 'backward'):
            raise NotImplementedError('kind must be forward, centered, or backward')
        dims = tuple(int(s) for s in shape)
        if not 1 <= len(dims) <= 32:
            raise NotImplementedError('FirstDirectionalDerivative supports 1-D to 32-D arrays')
        N = int(np.prod(dims))
        super().__init__((N, N), N, dtype)
        self.dims, self.steps, self.edge, self.kind = dims, _steps(step, len(dims)), bool(edge), kind
        self.directions, self.is_field = _directions(directions, dims)
        self._v = {}

    def _dev(self, dtype):
        v = self._v.get(dtype)
        if v is None:
            v = torch.as_tensor(self.directions).to(device=O.device(), dtype=dtype)
            if len(self.dims) > 3 and not self.is_field:  # the composition multiplies whole blocks
                v = v.repeat_interleave(self._size)
            self._v[dtype] = v
        return v

    def _edge_mask(self, dtype, width):
        m = self._v.get((dtype, width))
        if m is None:
            m = torch.as_tensor(_interior_mask(self.dims, width)).to(device=O.device(), dtype=dtype)
            self._v[(dtype, width)] = m
        return m

    def _finish(self, out, scale, kill):
        """``scale`` and the edge width of the fused kernels, for the composition beyond 3-D."""
        if kill:
            out = O.mul(out, self._edge_mask(out.dtype, kill))
        return out if scale == 1.0 else O.scale(out, float(scale))

    def _apply(self, t, scale=1.0, kill=0):
        v = self._dev(t.dtype)
        if len(self.dims) <= 3:
            return O.dirderiv(t, v, self.is_field, self.dims, self.steps, self.kind, self.edge, scale=scale, kill=kill)
        g = O.mul(O.grad_fwd(t, self.dims, self.steps, self.kind, self.edge), v)
        N, acc = self._size, None
        for k in range(len(self.dims)):
            acc = g[:N] if acc is None else O.add(acc, g[k * N:(k + 1) * N])
        return self._finish(acc, scale, kill)

    def _adj(self, t, scale=1.0, kill=0):
        v = self._dev(t.dtype)
        if len(self.dims) <= 3:
            return O.dirderiv(t, v, self.is_field, self.dims, self.steps, self.kind, self.edge, adjoint=True,
                              scale=scale, kill=kill)
        out = O.grad_adj(O.mul(t.repeat(len(self.dims)), v), self.dims, self.steps, self.kind, self.edge)
        return self._finish(out, scale, kill)


def FirstDirectionalDerivative(shape, directions, step=1., edge=True, dtype='float64', kind='centered'):
    """``pycsou/linop/diff.py:380-486``."""
    return FirstDirectionalDerivativeOp(shape, directions, step=step, edge=edge, dtype=dtype, kind=kind)


class SecondDirectionalDerivativeOp(_DiffOp):
    """``KillEdgeOp * pylops.SecondDirectionalDerivative`` (``diff.py:596-606``; PyLops 1.x: ``-Dv^T Dv`` with
    ``Dv`` the centred first directional derivative): the mask zeroes the first two and last two samples
    along every axis.  Forward: two launches and one temporary (``pcs_dirderiv_fwd``, then
    ``pcs_dirderiv_adj`` with ``scale = -1, kill = 2``); the adjoint ``-Dv^T Dv (mask . y)`` masks its input
    with one more launch."""

    def __init__(self, shape, directions, step=1., edge=True, dtype='float64'):
        self.Dv = FirstDirectionalDerivativeOp(shape, directions, step=step, edge=edge, dtype=dtype, kind='centered')
        N = self.Dv._size
        super().__init__((N, N), N, dtype)
        self.dims, self.steps, self.edge = self.Dv.dims, self.Dv.steps, self.Dv.edge
        self.kill_edges = _interior_mask(self.dims, 2)

    def _apply(self, t):
        return self.Dv._adj(self.Dv._apply(t), scale=-1.0, kill=2)

    def _adj(self, t):
        return self.Dv._adj(self.Dv._apply(O.mul(t, self.Dv._edge_mask(t.dtype, 2))), scale=-1.0)


def SecondDirectionalDerivative(shape, directions, step=1., edge=True, dtype='float64'):
    """``pycsou/linop/diff.py:489-606``."""
    return SecondDirectionalDerivativeOp(shape, directions, step=step, edge=edge, dtype=dtype)


def DirectionalGradient(first_directional_derivatives):
    """``pycsou/linop/diff.py:609-688``: ``LinOpVStack`` of first directional derivatives."""
    from .base import LinOpVStack
    return LinOpVStack(*first_directional_derivatives)


def DirectionalLaplacian(second_directional_derivatives, weights=None):
    """``pycsou/linop/diff.py:691-774``, as written there: the sum starts from the first operator *unweighted*
    and adds ``weights[i] * op_i`` for ``i >= 1``, so ``weights[0]`` has no effect (only its presence counts
    towards the length check)."""
    ops = list(second_directional_derivatives)
    if weights is not None and len(weights) != len(ops):
        raise ValueError(f'{len(weights)} weights were given for {len(ops)} operators')
    total = ops[0]
    for k, op in enumerate(ops[1:], start=1):
        total = total + (1.0 if weights is None else weights[k]) * op
    return total


class Integration1DOp(_DiffOp):
    """``pylops.CausalIntegration(..., halfcurrent=False)`` on the GPU (``pcs_cumsum``):
    ``y[i] = step * sum_{j <= i} x[j]`` along ``axis``; adjoint ``step * sum_{j >= i} y[j]``."""

    def __init__(self, size, shape=None, axis=0, step=1., dtype='float64'):
        dims = (size,) if shape is None else tuple(int(s) for s in shape)
        if int(np.prod(dims)) != size:
            raise ValueError('shape and size are not compatible')
        if not 1 <= len(dims) <= 32:
            raise NotImplementedError('Integration1D supports 1-D to 32-D arrays')
        if not -len(dims) <= int(axis) < len(dims):
            raise ValueError('axis is out of range')
        super().__init__((size, size), size, dtype)
        self.dims, self.axis, self.step = dims, int(axis) % len(dims), float(step)

    def _apply(self, t):
        return O.cumsum(t, self.dims, self.axis, self.step)

    def _adj(self, t):
        return O.cumsum(t, self.dims, self.axis, self.step, reverse=True)

    def compute_lipschitz_cst(self, **kwargs):
        """Exact ``||step * L|| = step / (2 sin(pi / (4n + 2)))`` for the integrated axis of length n
        (linop/_spectral.py), in place of the reference's ARPACK svds."""
        self.lipschitz_cst = self.diff_lipschitz_cst = S.integration_norm(self.dims[self.axis], self.step)


def Integration1D(size, shape=None, axis=0, step=1., dtype='float64'):
    """``pycsou/linop/diff.py:1071-1137``."""
    return Integration1DOp(size, shape=shape, axis=axis, step=step, dtype=dtype)
