"""Streaming statistics (mirrors ``pycsou/util/stats.py``).

``P2Algorithm`` is the P-square estimator of one quantile per pixel.  The reference updates the five markers of
every pixel in a Numba loop; here the update is one element-wise kernel (``pcs_p2_update``) over a
structure-of-arrays state on the device, following ``stats.py:97-132`` operation for operation.
"""

import numpy as np
import torch

from .. import _ops as O


class P2Algorithm:
    """``stats.py:6-94``: same attributes and behaviour.  ``add_sample`` takes a float, a NumPy array or a torch
    tensor; ``q``, ``marker_heights`` and ``marker_positions`` come back as NumPy or torch, whichever went in."""

    def __init__(self, pvalue):
        self.pvalue = pvalue
        self._state = None
        self._torch = False
        self._count = 0
        self._k = 0
        des, inc = O.p2_desired((pvalue,))
        self._des0, self._inc0 = des[0], inc[0]

    @classmethod
    def _view(cls, state, k, torch_out):
        """Estimator k of a shared device state (PMYULA keeps all its p-values in one)."""
        self = cls(state.pvalues[k])
        self._state, self._k, self._torch, self._count = state, k, torch_out, state.count
        return self

    @property
    def count(self):
        return self._count

    @property
    def desired_marker_positions(self):
        return self._des0 if self._state is None else self._state.desired[self._k]

    @property
    def increments(self):
        return self._inc0

    def add_sample(self, sample):
        self._torch = isinstance(sample, torch.Tensor)
        x = O.to_dev(sample)
        if self._state is None:
            self._state = O.P2State((self.pvalue,), x.numel(), x.dtype, x.device)
        elif x.dtype != self._state.heights.dtype:
            x = x.to(self._state.heights.dtype)
        self._state.add(x)
        self._count = self._state.count

    def _out(self, t):
        return t if self._torch else t.detach().cpu().numpy()

    @property
    def marker_heights(self):
        """(n, min(count, 5)) heights, ascending along axis 1; None before the first sample."""
        if self._state is None:
            return None
        return self._out(self._state.heights[self._k, :min(self._count, 5)].t().contiguous())

    @property
    def marker_positions(self):
        """(n, 5) integer positions; None before the fifth sample."""
        if self._state is None or self._count < 5:
            return None
        return self._out(self._state.positions(self._k))

    @property
    def q(self):
        """The quantile estimate, shape (n,); None until the sixth sample."""
        if self._state is None or self._count <= 5:
            return None
        return self._out(self._state.quantile(self._k).clone())
