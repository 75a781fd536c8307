"""Losses (``pycsou/func/loss.py`` hot-path subset).

``SquaredL2Loss(dim, data) = SquaredL2Norm(dim).shifter(-data)`` (``loss.py:165-219``,
through ``DifferentiableLoss``, ``loss.py:72-120``); ``(1/2) * SquaredL2Loss(...) * Op``
therefore has ``gradient(x) = Op^T((2*(Op x - y))*0.5)`` and ``diff_lipschitz_cst =
||Op||^2``, exactly as in the reference.
"""

import numpy as np
import torch

from .. import _ops as O
from ..core.functional import ProxFuncPreComp, ProximableFunctional
from .base import IndicatorFunctional
from .penalty import L1Ball, L1Norm, L2Ball, L2Norm, LInftyBall, LInftyNorm, SquaredL1Norm, SquaredL2Norm


def _neg(data):
    if isinstance(data, torch.Tensor):
        return -data
    return -np.asarray(data)


def ProximableLoss(func, data):
    """``loss.py:20-69``."""
    return ProxFuncPreComp(func, scale=1, shift=_neg(data))


def DifferentiableLoss(func, data):
    """``loss.py:72-120``."""
    return func.shifter(shift=_neg(data))


def L2Loss(dim, data):
    """``loss.py:123-162``."""
    return ProximableLoss(L2Norm(dim=dim), data=data)


def SquaredL2Loss(dim, data):
    """``loss.py:165-219``."""
    return DifferentiableLoss(SquaredL2Norm(dim=dim), data=data)


def L1Loss(dim, data):
    """``loss.py:280-326``."""
    return ProximableLoss(L1Norm(dim=dim), data=data)


def L2BallLoss(dim, data, radius=1):
    """``loss.py:222-277``."""
    return ProximableLoss(L2Ball(dim=dim, radius=radius), data=data)


def SquaredL1Loss(dim, data, prox_computation='sort'):
    """``loss.py:329-368``."""
    return ProximableLoss(SquaredL1Norm(dim=dim, prox_computation=prox_computation), data=data)


def L1BallLoss(dim, data, radius=1):
    """``loss.py:371-426``."""
    return ProximableLoss(L1Ball(dim=dim, radius=radius), data=data)


def LInftyLoss(dim, data):
    """``loss.py:429-475``."""
    return ProximableLoss(LInftyNorm(dim=dim), data=data)


def LInftyBallLoss(dim, data, radius=1):
    """``loss.py:478-533``."""
    return ProximableLoss(LInftyBall(dim=dim, radius=radius), data=data)


class _DeviceData:
    """``data`` as a flat device tensor, one copy per dtype."""

    def __init__(self, data):
        self.data = data
        self._dev = {}

    def __call__(self, like):
        d = self._dev.get(like.dtype)
        if d is None:
            d = self._dev[like.dtype] = O.to_dev(self.data, like.dtype)
        return d


def ConsistencyLoss(dim, data):
    """``loss.py:536-587``: indicator of ``{data}``; the projection returns the data."""
    dev = _DeviceData(data)
    return IndicatorFunctional(dim=dim, condition_func=lambda t: bool(torch.allclose(t, dev(t))),
                               projection_func=lambda t: dev(t).clone())


class KLDivergence(ProximableFunctional):
    """Generalised Kullback-Leibler divergence ``sum y log(y / x) - y + x`` (``loss.py:590-682``);
    ``prox = (x - tau + sqrt((x - tau)^2 + 4 tau y)) / 2`` is one kernel (``pcs_prox_kl``)."""

    def __init__(self, dim, data):
        super().__init__(dim=dim, data=None, is_differentiable=False, is_linear=False)
        self.data = data
        self._dev = _DeviceData(data)

    def _apply(self, t):
        # loss.py:659-664: y log(y / x) where x, y > 0; 0 where x == 0 <= y; +inf elsewhere
        x, y = t.double(), self._dev(t).double()
        pos = (x > 0) & (y > 0)
        z = torch.full_like(x, float('inf'))
        z[pos] = y[pos] * torch.log(y[pos] / x[pos])
        z[(x == 0) & (y >= 0)] = 0
        return float(torch.sum(z - y + x))

    def _prox(self, t, tau):
        return O.prox_kl(t, self._dev(t), tau)
