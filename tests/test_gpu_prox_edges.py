"""The standalone kernels of csrc/prox.hip beyond the fp64 n = 200 fixture: fp32 and fp64, element by element
against the oracle/pycsou_ref.py function evaluated in fp64 on the same (dtype-rounded) inputs, at
n = 1, 255, 257 (one thread, one short of and one past a 256-thread workgroup) and 2^21 + 257 (past the
8192-workgroup cap of grid_for: a second grid-stride trip for the last 257 elements).

Tolerance of the element-wise maps: 4 eps(dtype) M absolute, M the largest magnitude among the operands
(scalar factors are at most 1 in magnitude, so no term exceeds it) -- each map has at most four roundings
on operands no larger than M, each at most eps M / 2, doubled for the sums of up to three such terms.  The
fp64-accumulated sums: 1e-9 relative, as tests/test_gpu_ops.py::test_reductions.  Gathers are exact.
Scalars are fp32-representable, so the kernel's cast of them is exact.

L21 data holds all-zero groups (the result is 0, not NaN: tau / 0 = inf -> factor 0) and groups whose norm is
exactly tau (the factor is 0 up to its rounding); label vectors are not sorted and their values not contiguous."""

import numpy as np
import pytest

from oracle import pycsou_ref as OR

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 257, (1 << 21) + 257]
DTYPES = [np.float32, np.float64]
both = pytest.mark.parametrize('dtype,n', [(d, n) for d in DTYPES for n in SIZES],
                               ids=lambda v: str(v) if isinstance(v, int) else np.dtype(v).name)


def _data(n, dtype, seed, scale=1.0):
    """fp64 array of `dtype` values."""
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(dtype).astype(np.float64)


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.asarray(a, dtype=dtype)).cuda()


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _close(got, ref, dtype, *operands):
    got, ref = _host(got), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    M = max(float(np.max(np.abs(o))) for o in operands)
    tol = 4.0 * float(np.finfo(dtype).eps) * M
    err = np.abs(got - ref)
    i = int(np.argmax(err))
    assert np.isfinite(got).all() and err[i] <= tol, (i, got[i], ref[i], err[i], tol)


@both
@pytest.mark.parametrize('branch', ['inside', 'outside'])
def test_prox_l2(dtype, n, branch):
    from pycsou_amd import _ops as O
    x = _data(n, dtype, 1)
    nrm = float(np.linalg.norm(x))
    tau = float(np.float32(2.0 * nrm if branch == 'inside' else 0.3 * nrm))  # ||x|| / tau <= 1 | > 1
    assert (nrm / tau <= 1) == (branch == 'inside')
    _close(O.prox_l2(_dev(x, dtype), tau), OR.prox_l2(x.copy(), tau), dtype, x)


@both
def test_prox_sql2(dtype, n):
    from pycsou_amd import _ops as O
    x = _data(n, dtype, 2)
    _close(O.prox_sql2(_dev(x, dtype), 0.375), OR.prox_sql2(x, 0.375), dtype, x)


@both
def test_fenchel_l1(dtype, n):
    from pycsou_amd import _ops as O
    w = _data(n, dtype, 3)
    sigma, lam = 0.5, 0.75  # projects |w| > 0.75: about 45 % of N(0, 1)
    ref = OR.fenchel_prox(OR.postcomp(OR.prox_l1, lam), w.copy(), sigma)
    assert n == 1 or 0.2 < np.mean(np.abs(w) > lam) < 0.8
    _close(O.fenchel_l1(_dev(w, dtype), sigma, lam), ref, dtype, w)


def _special_groups(x2, tau):
    """x2: [members, groups] view.  Every 7th group all zero; the next one of norm exactly tau (members
    0.6 tau and 0.8 tau, exact for tau = 1.25: 0.75 and 1.0), where it has two members."""
    x2[:, 0::7] = 0.0
    if x2.shape[0] >= 2:
        x2[:, 1::7] = 0.0
        x2[0, 1::7], x2[1, 1::7] = 0.6 * tau, 0.8 * tau


@both
@pytest.mark.parametrize('d', [2, 3])
def test_prox_l21_pixel(dtype, n, d):
    from pycsou_amd import _ops as O
    tau = 1.25
    x = _data(d * n, dtype, 4 + d)
    _special_groups(x.reshape(d, n), tau)
    ref = OR.prox_l21_pixel(x, tau, d)
    assert np.all(ref.reshape(d, n)[:, 0::7] == 0) and np.all(ref.reshape(d, n)[:, 1::7] == 0)
    _close(O.prox_l21_pixel(_dev(x, dtype), tau, d), ref, dtype, x)


GROUPS = {'short': list(range(1, 33)), 'long': [33, 64, 65, 1000, 5, 1], 'one': None}


def _labels(n, kind, seed):
    """Unsorted labels with non-contiguous values: groups of the lengths of GROUPS[kind] in turn (the last cut
    at n; 'one': a single group), their elements scattered over the vector."""
    rng = np.random.default_rng(seed)
    if kind == 'one':
        return np.full(n, 41, dtype=np.int64)
    pat = np.asarray(GROUPS[kind])
    reps = int(np.ceil(n / pat.sum())) + 1
    lens = np.tile(pat, reps)
    g = np.repeat(np.arange(lens.size), lens)[:n]
    names = rng.permutation(g.max() + 1) * 3 + 5  # group k is called names[k]
    return names[g][rng.permutation(n)] if n > 1 else names[g]


def _group_data(n, dtype, kind, tau, seed):
    from pycsou_amd.func.penalty import L21Norm
    labels = _labels(n, kind, seed)
    x = _data(n, dtype, seed + 1)
    ids, inv = np.unique(labels, return_inverse=True)
    order, off, maxlen = L21Norm._csr_host(inv, ids.size)
    for g in range(0, ids.size if ids.size > 1 else 0, 5):  # all-zero groups (not the only group)
        x[order[off[g]:off[g + 1]]] = 0.0
    for g in range(1, ids.size, 5):  # norm exactly tau
        mem = order[off[g]:off[g + 1]]
        if mem.size >= 2:
            x[mem] = 0.0
            x[mem[0]], x[mem[-1]] = 0.6 * tau, 0.8 * tau
    return labels, x, inv.astype(np.int32), ids.size, order, off, maxlen


@both
@pytest.mark.parametrize('kind', ['short', 'long', 'one'])
def test_prox_l21_groups(dtype, n, kind):
    """Group lengths <= 32: one thread per group; longer (33, 64, 65, 1000, everything): one wave per group."""
    from pycsou_amd import _ops as O
    tau = 1.25
    labels, x, inv, ng, order, off, maxlen = _group_data(n, dtype, kind, tau, 20)
    assert (maxlen <= 32) == (kind == 'short' or n <= 32)
    if kind == 'long' and n > 2000:
        assert {33, 64, 65, 1000} <= set(np.diff(off).tolist())
    assert n < 3 or kind == 'one' or np.any(np.diff(labels) < 0), 'labels must not be sorted'
    ref = OR.prox_l21(x, tau, labels)
    assert np.isfinite(ref).all()
    got = O.prox_l21_groups(_dev(x, dtype), tau, _dev(inv, np.int32), ng, _dev(order, np.int32), _dev(off, np.int64),
                            maxlen)
    _close(got, ref, dtype, x)


@both
@pytest.mark.parametrize('kind', ['short', 'long'])
def test_prox_l21_labels(dtype, n, kind):
    from pycsou_amd import _ops as O
    tau = 1.25
    labels, x, inv, ng, _, _, _ = _group_data(n, dtype, kind, tau, 30)
    _close(O.prox_l21_labels(_dev(x, dtype), tau, _dev(inv, np.int32), ng), OR.prox_l21(x, tau, labels), dtype, x)


@both
def test_projections(dtype, n):
    from pycsou_amd import _ops as O
    x = _data(n, dtype, 40)
    xd = _dev(x, dtype)
    np.testing.assert_array_equal(_host(O.proj_nonneg(xd)), OR.proj_nonnegative_orthant(x.copy()))
    np.testing.assert_array_equal(_host(O.proj_segment(xd, -0.25, 0.5)), OR.proj_segment(x.copy(), -0.25, 0.5))
    if n > 200:
        assert np.mean(x < -0.25) > 0.2 and np.mean(x > 0.5) > 0.2


@both
def test_vector_algebra(dtype, n):
    from pycsou_amd import _ops as O
    x, y, w = _data(n, dtype, 50), _data(n, dtype, 51), _data(n, dtype, 52)
    xd, yd, wd = _dev(x, dtype), _dev(y, dtype), _dev(w, dtype)
    a, b = 0.75, -0.375
    _close(O.axpby(xd, yd, a, b), a * x + b * y, dtype, x, y)
    _close(O.axpby(xd, None, a, 0.0), a * x, dtype, x)
    _close(O.sub2(xd, yd, wd, a, b), (x - a * y) - b * w, dtype, x, y, w)
    _close(O.mul(xd, yd), y * x, dtype, x * y)


@both
def test_rel_sums(dtype, n):
    import torch

    from pycsou_amd import _ops as O
    old, new = _data(n, dtype, 60), _data(n, dtype, 61)
    out = torch.full((2,), float('nan'), dtype=torch.float64, device='cuda')
    O.rel_sums(_dev(old, dtype), _dev(new, dtype), out)
    np.testing.assert_allclose(_host(out), [np.sum((old - new) ** 2), np.sum(old ** 2)], rtol=1e-9)


@both
def test_gathers(dtype, n):
    from pycsou_amd import _ops as O
    rng = np.random.default_rng(70)
    src = _data(max(1, n // 3 + 2), dtype, 71)
    idx = rng.integers(0, src.size, n).astype(np.int32)
    np.testing.assert_array_equal(_host(O.gather(_dev(src, dtype), _dev(idx, np.int32))), src[idx])
    inv = np.where(rng.random(n) < 0.3, -1, idx).astype(np.int32)
    ref = np.where(inv >= 0, src[np.maximum(inv, 0)], 0.0)
    np.testing.assert_array_equal(_host(O.gather_or_zero(_dev(src, dtype), _dev(inv, np.int32))), ref)
