"""Green functions of common pseudo-differential operators (``pycsou/math/green.py``), written from their
closed forms:

    Matern(k, eps)                      S_{k+1/2}(r) = exp(-s r / eps) p_k(s r / eps),  s = sqrt(2 k + 1),  k in 0..3
    Wendland(k, eps)                    (1 - r / eps)_+^(2 k + 2) q_k(r / eps),  k in 0..3  (support [0, eps))
    SubGaussian(alpha, eps)             exp(-r^alpha / eps),  alpha in (0, 2)
    CausalGreenIteratedDerivative(k)    t^(k - 1) [t >= 0]
    CausalGreenExponential(k, alpha)    t^(k - 1) exp(-alpha t) [t >= 0],  alpha > 0

Calling an instance returns the kind it was given: a Python number or a NumPy array is evaluated with NumPy on
the host (what the host assembly of the dense and sparse ``MappedDistanceMatrix`` and of ``GeneralisedVandermonde``
calls; no GPU involved), a torch device tensor is evaluated on the device by ``pcs_green_eval``
(``csrc/green_core.hpp``).  Constants enter as Python floats, so a float32 array stays float32 on the host.

``_device_spec()`` is ``(kind, k, p0, p1)``, the four numbers the device kernels take; the matrix-free
``MappedDistanceMatrix`` recognises a function by ``isinstance`` of ``GREEN_CLASSES`` and nothing else.
``_device_ok()`` says whether those four numbers describe the instance exactly: the reference's constructors accept
any ``k`` for the causal classes (2.5, 0) and any ``epsilon``; such an instance works on the host as in the
reference, keeps ``MappedDistanceMatrix`` on its host assembly and raises ``ValueError`` for a device tensor.  A CPU
torch tensor is evaluated with the host formulas and comes back as a CPU tensor of its dtype.
"""

import math

import numpy as np
import torch

from .. import _lib as L
from .. import _ops as O

_ORDERS = (0, 1, 2, 3)
MAX_CAUSAL_K = 1 << 20          # kGreenMaxCausalK of csrc/green_core.hpp


def _power(x, m):
    """``x ** m`` for an integer ``m >= 0`` as NumPy evaluates it (``0 ** 0 = 1``)."""
    return x ** m


def _positive(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and 0 < v < math.inf


def _whole(k, lo, hi):
    return isinstance(k, (int, np.integer)) and not isinstance(k, bool) and lo <= k <= hi


class _Green:
    def __call__(self, r):
        if isinstance(r, torch.Tensor):
            if r.is_cuda:
                if not self._device_ok():
                    raise ValueError(f'{type(self).__name__}: these parameters have no device form (an integer k in '
                                     f'the range of the class and positive finite parameters); evaluate a NumPy array')
                return O.green_eval(self._device_spec(), r)
            with np.errstate(all='ignore'):      # a CPU tensor: the host formulas, a CPU tensor back
                return torch.as_tensor(np.asarray(self._host(r.detach().numpy()))).to(r.dtype)
        return self._host(r)

    def _device_ok(self):
        """Whether ``_device_spec()`` describes this function exactly (what ``pcs_green_eval`` accepts)."""
        raise NotImplementedError


class Matern(_Green):
    """Matern function of half-integer smoothness ``k + 1/2`` and spread ``epsilon``."""

    def __init__(self, k, epsilon=1.):
        if k not in _ORDERS:
            raise TypeError('Parameter k must be one of [0,1,2,3].')
        self.k = k
        self.epsilon = epsilon

    def _host(self, r):
        eps, k = self.epsilon, self.k
        if k == 0:
            return np.exp(-r / eps)
        s = math.sqrt(2 * k + 1)
        decay = np.exp(-s * r / eps)
        if k == 1:
            return (1 + s * r / eps) * decay
        if k == 2:
            return (1 + s * r / eps + (5 * r ** 2) / (3 * eps ** 2)) * decay
        return (1 + s * r / eps + (42 * r ** 2) / (15 * eps ** 2) + (7 * s * r ** 3) / (15 * eps ** 3)) * decay

    def support(self, sigmas=3):
        """Effective support from the Gaussian the function approaches: ``sigmas * epsilon``."""
        return sigmas * self.epsilon

    def _device_ok(self):
        return _whole(self.k, 0, 3) and _positive(self.epsilon)

    def _device_spec(self):
        return L.PCS_GREEN_MATERN, int(self.k), float(self.epsilon), 0.0


class Wendland(_Green):
    """Wendland function of order ``k``, supported on ``[0, epsilon)``.  As in the reference, the instance
    attribute ``support`` (the float ``epsilon``) shadows the method of that name."""

    def __init__(self, k, epsilon=1.):
        if k not in _ORDERS:
            raise TypeError('Parameter k must be one of [0,1,2,3].')
        self.k = k
        self.epsilon = epsilon
        self.support = epsilon

    def _host(self, r):
        eps, k = self.epsilon, self.k
        t = np.clip(1 - r / eps, a_min=0, a_max=None)
        if k == 0:
            return t ** 2
        if k == 1:
            return (t ** 4) * (1 + 4 * r / eps)
        if k == 2:
            return (t ** 6) * (1 + 6 * r / eps + 35 * r ** 2 / (3 * eps ** 2))
        return (t ** 8) * (1 + 8 * r / eps + 25 * r ** 2 / (eps ** 2) + 32 * r ** 3 / (eps ** 3))

    def support(self):
        return self.support

    def _device_ok(self):
        return _whole(self.k, 0, 3) and _positive(self.epsilon)

    def _device_spec(self):
        return L.PCS_GREEN_WENDLAND, int(self.k), float(self.epsilon), 0.0


class CausalGreenIteratedDerivative(_Green):
    """Causal Green function of the iterated derivative ``D^k``: ``t_+^(k - 1)``."""

    def __init__(self, k):
        self.k = k

    def _host(self, x):
        return _power(x, self.k - 1) * (x >= 0)

    def _device_ok(self):
        return _whole(self.k, 1, MAX_CAUSAL_K)

    def _device_spec(self):
        return L.PCS_GREEN_CAUSAL_ITER, int(self.k), 0.0, 0.0


class CausalGreenExponential(_Green):
    """Causal Green function of ``(D + alpha Id)^k``: ``t_+^(k - 1) exp(-alpha t)``."""

    def __init__(self, k, alpha=1):
        if alpha <= 0:
            raise TypeError('Parameter alpha must be strictly positive.')
        self.k = k
        self.alpha = alpha

    def _host(self, x):
        return _power(x, self.k - 1) * np.exp(-self.alpha * x) * (x >= 0)

    def _device_ok(self):
        return _whole(self.k, 1, MAX_CAUSAL_K) and _positive(self.alpha)

    def _device_spec(self):
        return L.PCS_GREEN_CAUSAL_EXP, int(self.k), float(self.alpha), 0.0


class SubGaussian(_Green):
    """Sub-Gaussian function ``exp(-r^alpha / epsilon)``, ``alpha`` in (0, 2)."""

    def __init__(self, alpha, epsilon=1.):
        if (alpha <= 0) or (alpha >= 2):
            raise TypeError('Parameter alpha must be in (0,2).')
        self.alpha = alpha
        self.epsilon = epsilon

    def _host(self, r):
        return np.exp(-np.power(r, self.alpha) / self.epsilon)      # a negative argument is NaN, Python numbers too

    def _device_ok(self):
        return _positive(self.alpha) and self.alpha < 2 and _positive(self.epsilon)

    def _device_spec(self):
        return L.PCS_GREEN_SUBGAUSSIAN, 0, float(self.alpha), float(self.epsilon)


GREEN_CLASSES = (Matern, Wendland, CausalGreenIteratedDerivative, CausalGreenExponential, SubGaussian)
