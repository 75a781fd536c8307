"""Inputs, parameters and the exact restatement shared by the func-family tests and by
``tests/golden/make_golden_func.py`` (which runs the reference on the same inputs).

The threshold family -- ``L1Ball`` (``pycsou/math/prox.py:158-164``), ``LInftyNorm`` (``func/base.py:239-240``
with ``proj_l1_ball``), ``SquaredL1Norm`` (``func/penalty.py:296-316``) -- is one problem:
``t = 0`` if ``sum|x| <= a``, else the root of ``sum max(|x| - t, 0) = a + b t``.  ``exact_threshold`` solves
it by sorting, with every sum in ``longdouble``: the yardstick for the device kernel.
"""

import numpy as np

SIZES = (1, 2, 63, 64, 65, 257, 4099, 70001)
FIXTURE_SIZES = (1, 2, 63, 64, 65, 257)          # the sizes whose reference outputs func_family.npz holds
KINDS = ('normal', 'quant', 'zeros', 'equal', 'outlier', 'mixed')
RADII = (0.01, 0.5, 0.999, 1.0, 2.0)             # times ||x||_1
TAUS = (0.05, 1.0, 7.0)


def make_x(kind, n):
    """fp64 input of one data kind; every value is exactly representable in fp32 as well, so the fp32
    tests run the same numbers."""
    rng = np.random.default_rng([7, n, KINDS.index(kind)])
    if kind == 'normal':
        x = rng.standard_normal(n)
    elif kind == 'quant':          # multiples of 1/4: many ties, sums exact in any order
        x = rng.integers(-12, 13, n) / 4.0
        x[0] = 1.25
    elif kind == 'zeros':          # 90 % zeros
        x = rng.standard_normal(n) * (rng.uniform(size=n) < 0.1)
        x[0] = 0.7
    elif kind == 'equal':
        x = np.full(n, 0.75)
    elif kind == 'outlier':        # one element of 1e6 among O(1) values
        x = rng.uniform(-1, 1, n)
        x[n // 2] = 1e6
    elif kind == 'mixed':          # both signs, magnitudes over seven decades
        x = 10.0 ** rng.uniform(-6, 1, n) * rng.choice([-1.0, 1.0], n)
    else:
        raise ValueError(kind)
    return x.astype(np.float32).astype(np.float64)


def thresh_params(kind, n, x):
    """[(family, parameter, a, b, mode)] for one input.  The radius equal to ||x||_1 is kept for the quantised
    kind at n <= 257 only: there sum|x| is exact in every summation order, so every implementation takes the
    identity branch."""
    l1 = float(np.sum(np.abs(x)))
    out = []
    for f in RADII:
        if f == 1.0 and not (kind == 'quant' and n <= 257):
            continue
        out.append(('l1ball', f, f * l1, 0.0, 'soft'))
    for tau in TAUS:
        out.append(('linfty', tau, tau, 0.0, 'clip'))
    for tau in TAUS:
        out.append(('sql1', tau, 0.0, 1.0 / (2.0 * tau), 'soft'))
    return out


def exact_threshold(x, a, b):
    """t of the module docstring by a descending sort and longdouble prefix sums: the largest k with
    |x|_(k) > (S_k - a) / (k + b) gives t = (S_k - a) / (k + b)."""
    ax = np.sort(np.abs(np.asarray(x, dtype=np.longdouble)))[::-1]
    a, b = np.longdouble(a), np.longdouble(b)
    if ax.sum() <= a:
        return np.longdouble(0)
    s = np.cumsum(ax)
    tk = (s - a) / (np.arange(1, ax.size + 1, dtype=np.longdouble) + b)
    k = np.flatnonzero(ax > tk).max()
    return tk[k]


def exact_apply(x, t, mode):
    """The soft threshold / clip at t in longdouble, rounded once to fp64.  t = 0: x itself (soft) or zeros."""
    xl = np.asarray(x, dtype=np.longdouble)
    if mode == 'soft':
        if t == 0:
            return np.asarray(x, dtype=np.float64).copy()
        return (np.sign(xl) * np.maximum(np.abs(xl) - t, 0)).astype(np.float64)
    return np.clip(xl, -t, t).astype(np.float64)


def exact_prox(x, a, b, mode):
    t = exact_threshold(x, a, b)
    return float(t), exact_apply(x, t, mode)


# ---------------------------------------------------------------- element-wise inputs
KL_TAUS = (0.1, 1.0, 4.0)


def kl_inputs():
    """x in [-30, 30] (fp32-representable) and y cycling over {0, 1, 3, 50}."""
    rng = np.random.default_rng(21)
    x = np.concatenate([rng.uniform(-30, 30, 396), [-30.0, 30.0, 0.0, 0.1]]).astype(np.float32).astype(np.float64)
    y = np.tile([0.0, 1.0, 3.0, 50.0], x.size // 4)
    return x, y


def entropy_inputs(tau):
    """x with x / tau over [-700, 700] (fp32-representable x)."""
    rng = np.random.default_rng(22)
    r = np.concatenate([rng.uniform(-700, 700, 250), np.linspace(-3, 3, 46), [-700.0, 700.0, 0.0, 1.0]])
    x = (r * tau).astype(np.float32).astype(np.float64)
    return x[np.abs(x / tau) <= 700.0]


# ---------------------------------------------------------------- solver problems
def sparse_problem():
    """A (64 x 128, default_rng(3)), a 6-sparse +-1 truth and y = A x*."""
    rng = np.random.default_rng(3)
    A = rng.standard_normal((64, 128))
    xs = np.zeros(128)
    xs[rng.choice(128, 6, replace=False)] = rng.choice([-1.0, 1.0], 6)
    return A, xs, A @ xs
