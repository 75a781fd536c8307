"""Tensor-level wrappers over the C ABI + the array boundary of the public API.

Public pycsou-style methods accept NumPy arrays or torch tensors and return the same
kind they were given (NumPy in -> NumPy out, as in the reference; torch in -> device
tensor out).  Everything in between is a contiguous 1-D device tensor handled by the
gfx950 kernels.
"""

from numbers import Number

import ctypes

import numpy as np
import torch

from . import _lib as L

_ws_cache = {}


# ---------------------------------------------------------------- array boundary

def device():
    return torch.device('cuda', torch.cuda.current_device())


def torch_dtype(dtype, default=torch.float64):
    if dtype is None:
        return default
    if isinstance(dtype, torch.dtype):
        return dtype
    d = np.dtype(dtype)
    if d == np.float32:
        return torch.float32
    return torch.float64


def to_dev(x, dtype=None):
    """Contiguous flat device tensor (float32/float64) from NumPy / torch / scalar."""
    L.gpu()
    if isinstance(x, torch.Tensor):
        t = x
        if dtype is None and t.dtype not in (torch.float32, torch.float64):
            dtype = torch.float64
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        if not t.is_cuda:
            t = t.to(device())
        return t.reshape(-1).contiguous()
    a = np.asarray(x)
    if dtype is None:
        dtype = torch.float32 if a.dtype == np.float32 else torch.float64
    return torch.as_tensor(np.ascontiguousarray(a).reshape(-1)).to(device=device(), dtype=dtype)


def like(out, ref):
    """Return `out` (device tensor) as the array kind of `ref`."""
    if isinstance(ref, torch.Tensor):
        return out
    return out.detach().cpu().numpy()


def numel(x):
    return int(x.numel()) if isinstance(x, torch.Tensor) else int(np.size(x))


def is_array(x):
    return isinstance(x, (np.ndarray, torch.Tensor))


def empty_like(t):
    return torch.empty_like(t)


# ---------------------------------------------------------------- elementwise / algebra

def axpby(x, y, a, b, out=None):
    """out = a*x + b*y  (y may be None)."""
    lib = L.gpu()
    out = torch.empty_like(x) if out is None else out
    L.check(lib.pcs_axpby(L.dtcode(x), L.ptr(x), L.ptr(y), L.ptr(out), x.numel(), float(a), float(b),
                          L.stream()), 'pcs_axpby')
    return out


def scale(x, a):
    return axpby(x, None, a, 0.0)


def add(x, y):
    return axpby(x, y, 1.0, 1.0)


def mul(x, d):
    """d * x elementwise (pcs_mul)."""
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_mul(L.dtcode(x), L.ptr(x), L.ptr(d), L.ptr(out), x.numel(), L.stream()), 'pcs_mul')
    return out


def rel_sums(old, new, out):
    """out[0], out[1] = sum (old - new)^2, sum old^2 (fp64, fixed order) into a device slice."""
    lib = L.gpu()
    L.check(lib.pcs_rel_sums(L.dtcode(old), L.ptr(old), L.ptr(new), old.numel(), L.ptr(out), L.ptr(_ws(old)),
                             L.stream()), 'pcs_rel_sums')
    return out


def sub2(x, y, w, a, b):
    """(x - a*y) - b*w  (proxalgs.py:348)."""
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_sub2(L.dtcode(x), L.ptr(x), L.ptr(y), L.ptr(w), L.ptr(out), x.numel(), float(a), float(b),
                         L.stream()), 'pcs_sub2')
    return out


def _cached_ws(device, kind, nbytes):
    """A float64 workspace of exactly `nbytes` bytes (the size the C ABI advertises: what a C caller allocates
    is what these wrappers run on), one per (device, kind, size) and never replaced, so that a captured loop
    replays with the buffer it was captured with."""
    key = (device, kind, int(nbytes))
    ws = _ws_cache.get(key)
    if ws is None:
        ws = _ws_cache[key] = torch.empty(-(-int(nbytes) // 8), dtype=torch.float64, device=device)
    return ws


def _ws(t):
    return _cached_ws(t.device, 'reduce', L.gpu().pcs_reduce_ws_bytes())


def reduce_dev(kind, x, y=None, out=None):
    """Deterministic fp64 reduction into a 1-element device tensor.
    kind: 0 sum x^2, 1 sum |x|, 2 sum (x-y)^2, 3 sum x*y."""
    lib = L.gpu()
    out = torch.empty(1, dtype=torch.float64, device=x.device) if out is None else out
    L.check(lib.pcs_reduce(L.dtcode(x), int(kind), L.ptr(x), L.ptr(y), x.numel(), L.ptr(out), L.ptr(_ws(x)),
                           L.stream()), 'pcs_reduce')
    return out


def apgd_step(x, g, aux, tau, a, gkind, lam=1.0, seg=(0.0, 1.0), sums=None):
    """Fused APGD update (``pcs_apgd_step``): returns (x', x_t, sums) with sums[0..1] =
    ||x - x'||^2, ||x||^2 on the device."""
    lib = L.gpu()
    xn, auxn = torch.empty_like(x), torch.empty_like(x)
    sums = torch.empty(2, dtype=torch.float64, device=x.device) if sums is None else sums
    L.check(lib.pcs_apgd_step(L.dtcode(x), L.ptr(x), L.ptr(g), L.ptr(aux), L.ptr(xn), L.ptr(auxn), x.numel(),
                              float(tau), float(a), int(gkind), float(lam), float(seg[0]), float(seg[1]), L.ptr(sums),
                              L.ptr(_ws(x)), L.stream()), 'pcs_apgd_step')
    return xn, auxn, sums


def myula_step(x, g, tau, gamma, p=None, gk=None, z=None, seed=0, it=0, stream_id=0, out=None):
    """One Langevin step (``pcs_myula_step``).  ``p``: G.prox(x, tau) as a buffer; else ``gk`` = (kind, lam, seg)
    of ``engine.apgd_g_kind`` for a prox formed in the kernel; neither: the G-null form.  ``z``: the normals, or
    None for in-kernel Philox noise keyed by (seed, it, stream_id)."""
    lib = L.gpu()
    out = torch.empty_like(x) if out is None else out
    mode, kind, lam, seg = L.PCS_MYULA_P_NONE, 0, 1.0, (0.0, 1.0)
    if p is not None:
        mode = L.PCS_MYULA_P_BUF
    elif gk is not None:
        mode, (kind, lam, seg) = L.PCS_MYULA_P_KIND, gk
    for t in (g, p, z):
        if t is not None and (t.dtype != x.dtype or t.numel() != x.numel() or not _dense_on(x.device, t)):
            raise ValueError('myula_step: every buffer must be a contiguous tensor of the dtype, size and GPU of x')
    L.check(lib.pcs_myula_step(L.dtcode(x), L.ptr(x), L.ptr(g), L.ptr(p), L.ptr(z), L.ptr(out), x.numel(),
                               float(tau if tau is not None else 0.0), float(gamma), mode, int(kind), float(lam),
                               float(seg[0]), float(seg[1]), int(seed) & (2 ** 64 - 1), int(it) & 0xffffffff,
                               int(stream_id) & 0xffffffff, L.stream()), 'pcs_myula_step')
    return out


def mcmc_normal(n, dtype, seed, it, stream_id=0):
    """The n normals ``pcs_myula_step`` generates for (seed, it, stream_id), as a device tensor."""
    lib = L.gpu()
    out = torch.empty(int(n), dtype=dtype, device=device())
    L.check(lib.pcs_mcmc_normal(L.dtcode(out), L.ptr(out), out.numel(), int(seed) & (2 ** 64 - 1),
                                int(it) & 0xffffffff, int(stream_id) & 0xffffffff, L.stream()), 'pcs_mcmc_normal')
    return out


def mcmc_philox(nblocks, seed, it, stream_id=0):
    """Raw Philox words of blocks 0..nblocks-1 (4 per block) as an int32 device tensor (bit patterns)."""
    lib = L.gpu()
    out = torch.empty(4 * int(nblocks), dtype=torch.int32, device=device())
    L.check(lib.pcs_mcmc_philox(L.ptr(out), int(nblocks), int(seed) & (2 ** 64 - 1), int(it) & 0xffffffff,
                                int(stream_id) & 0xffffffff, L.stream()), 'pcs_mcmc_philox')
    return out


class P2State:
    """Device state of K P-square estimators over n pixels (layout of ``pcs_p2_update``): ``heights`` (K, 5, n)
    in ``dtype``, ``pos`` (K, 3, n) int32 for markers 1..3, and on the host the sample count and the desired
    positions, accumulated by repeated addition as ``P2Algorithm.add_sample`` does."""

    def __init__(self, pvalues, n, dtype, dev=None):
        self.pvalues = tuple(float(p) for p in pvalues)
        self.K, self.n, self.count = len(self.pvalues), int(n), 0
        if self.K > L.PCS_P2_MAX_K:
            raise ValueError(f'at most {L.PCS_P2_MAX_K} p-values per state, got {self.K}')
        dev = device() if dev is None else dev
        self.heights = torch.zeros((max(self.K, 1), 5, self.n), dtype=dtype, device=dev)
        self.pos = torch.zeros((max(self.K, 1), 3, self.n), dtype=torch.int32, device=dev)
        self.desired, self.increments = p2_desired(self.pvalues)

    def advance(self):
        """Count one more sample; returns the desired positions to pass with it."""
        self.count += 1
        if self.count > 5:
            self.desired += self.increments  # stats.py:91
        return self.desired

    def add(self, x):
        """``pcs_p2_update`` with the sample ``x`` (device tensor of n elements)."""
        lib = L.gpu()
        if x.dtype != self.heights.dtype or x.numel() != self.n or not _dense_on(self.heights.device, x):
            raise ValueError('P2State.add: the sample must be a contiguous tensor of the state\'s dtype, size and GPU')
        des = np.ascontiguousarray(self.advance())
        L.check(lib.pcs_p2_update(L.dtcode(x), L.ptr(x), L.ptr(self.heights), L.ptr(self.pos), self.n, self.K,
                                  self.count, des.ctypes.data_as(L._pdbl), L.stream()), 'pcs_p2_update')

    def quantile(self, k):
        """Marker 2 of estimator k (``P2Algorithm.q``): None before the sixth sample."""
        return None if self.count <= 5 else self.heights[k, 2]

    def positions(self, k):
        """(n, 5) marker positions of estimator k as the reference keeps them, None before the fifth sample."""
        if self.count < 5:
            return None
        p = self.pos[k].to(torch.int64)
        ends = torch.ones(self.n, dtype=torch.int64, device=p.device)
        return torch.stack([ends, p[0], p[1], p[2], ends * self.count], dim=1)


def p2_desired(pvalues):
    """Initial desired marker positions and their increments, (K, 5) float64 each (stats.py:67-68)."""
    des = np.array([[1, 1 + 2 * p, 1 + 4 * p, 3 + 2 * p, 5] for p in pvalues], dtype=np.float64).reshape(-1, 5)
    inc = np.array([[0, p / 2, p, (p + 1) / 2, 1] for p in pvalues], dtype=np.float64).reshape(-1, 5)
    return des, inc


def mcmc_accumulate(x, total, total_sq, state, sums):
    """One retained sample (``pcs_mcmc_accumulate``): ``total += x``, ``total_sq += x * x``, the P2 ``state``
    takes x, and ``sums[0..1]`` (float64 device slice) = sum x^2, sum total_old^2."""
    lib = L.gpu()
    for t in (total, total_sq):
        if t.dtype != x.dtype or t.numel() != x.numel() or not _dense_on(x.device, t):
            raise ValueError('mcmc_accumulate: the sums must be contiguous tensors of the dtype, size and GPU of x')
    if state.n != x.numel() or state.heights.dtype != x.dtype or not _dense_on(x.device, x, state.heights, sums):
        raise ValueError('mcmc_accumulate: the P2 state does not match the sample')
    des = np.ascontiguousarray(state.advance())
    L.check(lib.pcs_mcmc_accumulate(L.dtcode(x), L.ptr(x), L.ptr(total), L.ptr(total_sq), L.ptr(state.heights),
                                    L.ptr(state.pos), x.numel(), state.K, state.count, des.ctypes.data_as(L._pdbl),
                                    L.ptr(sums), L.ptr(_ws(x)), L.stream()), 'pcs_mcmc_accumulate')


def sumsq(x):
    return float(reduce_dev(0, x).item())


def norm(x):
    return float(np.sqrt(sumsq(x)))


# ---------------------------------------------------------------- prox

def prox_l1(x, tau):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_prox_l1(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), float(tau), L.stream()), 'pcs_prox_l1')
    return out


def fenchel_l1(w, sigma, lam):
    lib = L.gpu()
    out = torch.empty_like(w)
    L.check(lib.pcs_fenchel_l1(L.dtcode(w), L.ptr(w), L.ptr(out), w.numel(), float(sigma), float(lam), L.stream()),
            'pcs_fenchel_l1')
    return out


def prox_l21_pixel(x, tau, d):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_prox_l21_pixel(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel() // d, int(d), float(tau),
                                   L.stream()), 'pcs_prox_l21_pixel')
    return out


def fenchel_l21_pixel(w, sigma, lam, d):
    lib = L.gpu()
    out = torch.empty_like(w)
    L.check(lib.pcs_fenchel_l21_pixel(L.dtcode(w), L.ptr(w), L.ptr(out), w.numel() // d, int(d), float(sigma),
                                      float(lam), L.stream()), 'pcs_fenchel_l21_pixel')
    return out


def prox_l21_labels(x, tau, gid, ngroups):
    lib = L.gpu()
    out = torch.empty_like(x)
    ws = torch.empty(int(ngroups), dtype=torch.float64, device=x.device)
    L.check(lib.pcs_prox_l21_labels(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), L.ptr(gid), int(ngroups),
                                    float(tau), L.ptr(ws), L.stream()), 'pcs_prox_l21_labels')
    return out


def prox_l21_groups(x, tau, gid, ngroups, order, off, maxlen):
    """L21Norm.prox over general labels with deterministic group sums (pcs_prox_l21_groups)."""
    lib = L.gpu()
    out = torch.empty_like(x)
    ws = torch.empty(int(ngroups), dtype=torch.float64, device=x.device)
    L.check(lib.pcs_prox_l21_groups(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), L.ptr(gid), int(ngroups),
                                    L.ptr(order), L.ptr(off), int(maxlen), float(tau), L.ptr(ws), L.stream()),
            'pcs_prox_l21_groups')
    return out


def prox_l2(x, tau):
    lib = L.gpu()
    ss = reduce_dev(0, x)
    out = torch.empty_like(x)
    L.check(lib.pcs_prox_l2(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), float(tau), L.ptr(ss), L.stream()),
            'pcs_prox_l2')
    return out


def prox_sql2(x, tau):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_prox_sql2(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), float(tau), L.stream()),
            'pcs_prox_sql2')
    return out


def proj_nonneg(x):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_proj_nonneg(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), L.stream()), 'pcs_proj_nonneg')
    return out


def proj_segment(x, a, b):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_proj_segment(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), float(a), float(b), L.stream()),
            'pcs_proj_segment')
    return out


def _thresh_ws(t):
    """Workspace of pcs_thresh_l1 for the elements of `t`: pcs_thresh_ws_bytes(n) bytes (it does not grow past
    the kernel's block cap, so there are at most that many sizes), cached like ``_ws``."""
    return _cached_ws(t.device, 'thresh', L.gpu().pcs_thresh_ws_bytes(t.numel()))


def thresh_l1(x, a, b, mode, t_out=None):
    """One global threshold (``pcs_thresh_l1``): ``t = 0`` if ``sum|x| <= a``, else the root of
    ``sum max(|x| - t, 0) = a + b t``; mode 'soft' -> ``sign(x) max(|x| - t, 0)``, 'clip' ->
    ``clip(x, -t, t)``.  ``t_out``: a 1-element float64 device tensor that receives t.  No host sync."""
    lib = L.gpu()
    out = torch.empty_like(x)
    code = {'soft': L.PCS_THRESH_SOFT, 'clip': L.PCS_THRESH_CLIP}[mode]
    L.check(lib.pcs_thresh_l1(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), float(a), float(b), code, L.ptr(t_out),
                              L.ptr(_thresh_ws(x)), L.stream()), 'pcs_thresh_l1')
    return out


def prox_kl(x, y, tau):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_prox_kl(L.dtcode(x), L.ptr(x), L.ptr(y), L.ptr(out), x.numel(), float(tau), L.stream()),
            'pcs_prox_kl')
    return out


def prox_logbarrier(x, tau):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_prox_logbarrier(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), float(tau), L.stream()),
            'pcs_prox_logbarrier')
    return out


def prox_entropy(x, tau):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_prox_entropy(L.dtcode(x), L.ptr(x), L.ptr(out), x.numel(), float(tau), L.stream()),
            'pcs_prox_entropy')
    return out


# ---------------------------------------------------------------- operators

def grad_fwd(x, dims, steps, kind, edge):
    lib = L.gpu()
    out = torch.empty(len(dims) * x.numel(), dtype=x.dtype, device=x.device)
    L.check(lib.pcs_grad_fwd(L.dtcode(x), L.ptr(x), L.ptr(out), len(dims), L.i64s(dims), L.dbls(steps),
                             L.KINDS[kind], int(bool(edge)), L.stream()), 'pcs_grad_fwd')
    return out


def grad_adj(z, dims, steps, kind, edge):
    lib = L.gpu()
    out = torch.empty(z.numel() // len(dims), dtype=z.dtype, device=z.device)
    L.check(lib.pcs_grad_adj(L.dtcode(z), L.ptr(z), L.ptr(out), len(dims), L.i64s(dims), L.dbls(steps),
                             L.KINDS[kind], int(bool(edge)), L.stream()), 'pcs_grad_adj')
    return out


def deriv1(x, dims, axis, step, kind, edge, adjoint=False):
    lib = L.gpu()
    out = torch.empty_like(x)
    fn = lib.pcs_deriv1_adj if adjoint else lib.pcs_deriv1_fwd
    L.check(fn(L.dtcode(x), L.ptr(x), L.ptr(out), len(dims), L.i64s(dims), int(axis), float(step), L.KINDS[kind],
               int(bool(edge)), L.stream()), 'pcs_deriv1')
    return out


def deriv2(x, dims, axis, step, edge, adjoint=False):
    lib = L.gpu()
    out = torch.empty_like(x)
    fn = lib.pcs_deriv2_adj if adjoint else lib.pcs_deriv2_fwd
    L.check(fn(L.dtcode(x), L.ptr(x), L.ptr(out), len(dims), L.i64s(dims), int(axis), float(step), int(bool(edge)),
               L.stream()), 'pcs_deriv2')
    return out


def _dense_on(device, *tensors):
    """The kernels take raw pointers: every tensor contiguous and on `device`, a GPU."""
    return device.type == 'cuda' and all(t.is_contiguous() and t.device == device for t in tensors)


def dirderiv(x, v, v_is_field, dims, steps, kind, edge, adjoint=False, scale=1.0, kill=0):
    """Fused directional derivative ``scale * sum_k v_k . D_k x`` or its adjoint ``scale * sum_k D_k^T (v_k . y)``
    (``pcs_dirderiv_*``, 1-D to 3-D); ``v``: device tensor of ``ndim`` scalars or ``ndim * N`` values in [k][p]
    order; ``kill`` (0 or 2) zeroes that many samples at both ends of every axis of the output."""
    lib = L.gpu()
    if v.dtype != x.dtype or v.numel() != (len(dims) * x.numel() if v_is_field else len(dims)):
        raise ValueError('dirderiv: directions must have the dtype of x and ndim or ndim * N values')
    if int(np.prod(dims)) != x.numel() or not _dense_on(x.device, x, v):
        raise ValueError('dirderiv: x and directions must be contiguous tensors on one GPU, x of prod(dims) elements')
    out = torch.empty_like(x)
    fn = lib.pcs_dirderiv_adj if adjoint else lib.pcs_dirderiv_fwd
    L.check(fn(L.dtcode(x), L.ptr(x), L.ptr(v), int(bool(v_is_field)), L.ptr(out), len(dims), L.i64s(dims),
               L.dbls(steps), L.KINDS[kind], int(bool(edge)), float(scale), int(kill), L.stream()), 'pcs_dirderiv')
    return out


# shortest segment of a line that pcs_cumsum splits (contiguous axis / strided axis): lines of SPAN + 1 and
# 2 SPAN + 1 samples are the first with two and three segments
CUMSUM_SPAN, CUMSUM_SPAN_STRIDED = L.PCS_CUMSUM_SPAN, L.PCS_CUMSUM_SPAN_STRIDED


def _cumsum_ws(t, nbytes):
    """Workspace of pcs_cumsum: the `nbytes` pcs_cumsum_ws_bytes returns for the call (bounded for any shape by
    PCS_CUMSUM_WS_MAX), cached like ``_ws``; None when the call needs none."""
    return _cached_ws(t.device, 'cumsum', nbytes) if nbytes > 0 else None


def cumsum(x, dims, axis, step, reverse=False, out=None):
    """``step * cumsum(x, axis)`` of a C-order array of shape ``dims`` (``pcs_cumsum``), or with ``reverse`` the
    sum from the far end of the axis (the adjoint).  ``out`` may be ``x`` itself."""
    lib = L.gpu()
    out = torch.empty_like(x) if out is None else out
    d = L.i64s(dims)
    need = int(lib.pcs_cumsum_ws_bytes(len(dims), d, int(axis)))
    if need < 0 or need > L.PCS_CUMSUM_WS_MAX or int(np.prod(dims)) != x.numel() or out.numel() != x.numel() \
            or out.dtype != x.dtype or not _dense_on(x.device, x, out):
        raise ValueError('cumsum: shape, axis and tensors do not agree (x and out: contiguous, same dtype, one GPU)')
    L.check(lib.pcs_cumsum(L.dtcode(x), L.ptr(x), L.ptr(out), len(dims), d, int(axis), float(step),
                           int(bool(reverse)), L.ptr(_cumsum_ws(x, need)), L.stream()), 'pcs_cumsum')
    return out


def gather(x, idx):
    """x[idx] (idx: int32 device tensor)."""
    lib = L.gpu()
    out = torch.empty(idx.numel(), dtype=x.dtype, device=x.device)
    L.check(lib.pcs_gather(L.dtcode(x), L.ptr(x), L.ptr(idx), L.ptr(out), idx.numel(), L.stream()), 'pcs_gather')
    return out


def gather_or_zero(y, inv):
    """out[p] = y[inv[p]] if inv[p] >= 0 else 0 (inv: int32 device tensor)."""
    lib = L.gpu()
    out = torch.empty(inv.numel(), dtype=y.dtype, device=y.device)
    L.check(lib.pcs_gather_or_zero(L.dtcode(y), L.ptr(y), L.ptr(inv), L.ptr(out), inv.numel(), L.stream()),
            'pcs_gather_or_zero')
    return out


# pcs_csr_spmv: a row of more than SPMV_LONG_ROW entries is cut into chunks of SPMV_CHUNK entries (rows of
# LONG_ROW + 1 and 2 CHUNK + 1 entries are the first with two and three chunks)
SPMV_LONG_ROW, SPMV_CHUNK = L.PCS_SPMV_LONG_ROW, L.PCS_SPMV_CHUNK


def spmv_lanes(nnz, nrows):
    """Lanes per row of pcs_csr_spmv: the smallest power of two >= nnz / nrows, at most a wave."""
    mean = nnz / max(int(nrows), 1)
    lanes = 1
    while lanes < 64 and lanes < mean:
        lanes *= 2
    return lanes


def spmv_plan(rowptr):
    """Chunk lists of pcs_csr_spmv for a CSR row-pointer array: (chunk_row, chunk_start, long_row, long_first),
    int64 NumPy arrays.  Rows of more than SPMV_LONG_ROW entries, in row order, each cut into chunks of SPMV_CHUNK
    entries in entry order."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    length = np.diff(rowptr)
    long_row = np.flatnonzero(length > SPMV_LONG_ROW).astype(np.int64)
    per_row = -(-length[long_row] // SPMV_CHUNK)
    long_first = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int64)
    chunk_row = np.repeat(long_row, per_row)
    within = np.arange(int(long_first[-1]), dtype=np.int64) - np.repeat(long_first[:-1], per_row)
    chunk_start = rowptr[chunk_row] + within * SPMV_CHUNK
    return chunk_row, chunk_start.astype(np.int64), long_row, long_first


class DeviceCSR:
    """A fixed SciPy sparse matrix as the device arrays of pcs_csr_spmv in one dtype: int64 row pointers, int32
    column indices, values, the chunk lists of its long rows and their partials workspace.  Everything is
    validated and built once on the host, so a captured loop replays with the buffers it was captured with."""

    def __init__(self, mat, dtype):
        import scipy.sparse as sp
        L.gpu()
        m = sp.csr_matrix(mat)
        nrows, ncols = m.shape
        if ncols >= 2 ** 31:
            raise NotImplementedError('pcs_csr_spmv indexes columns with int32 (ncols < 2^31)')
        rowptr, colind = np.asarray(m.indptr, dtype=np.int64), np.asarray(m.indices, dtype=np.int64)
        nnz = int(rowptr[-1])
        if rowptr.size != nrows + 1 or rowptr[0] != 0 or np.any(np.diff(rowptr) < 0) or colind.size < nnz \
                or m.data.size < nnz or (nnz and (colind[:nnz].min() < 0 or colind[:nnz].max() >= ncols)):
            raise ValueError('DeviceCSR: inconsistent CSR arrays')
        self.shape, self.nnz, self.dtype = (int(nrows), int(ncols)), nnz, dtype
        self.lanes = spmv_lanes(nnz, nrows)
        dev = device()
        plan = spmv_plan(rowptr)
        self.rowptr = torch.as_tensor(rowptr).to(dev)
        self.colind = torch.as_tensor(colind[:nnz].astype(np.int32)).to(dev)
        self.vals = torch.as_tensor(np.asarray(m.data[:nnz]).real.astype(np.float64)).to(device=dev, dtype=dtype)
        self.chunk_row, self.chunk_start, self.long_row, self.long_first = (torch.as_tensor(a).to(dev) for a in plan)
        self.nchunks, self.nlong = int(plan[0].size), int(plan[2].size)
        self.partials = torch.empty(max(self.nchunks, 1), dtype=torch.float64, device=dev)


def spmv(A, x, out=None, lanes=None):
    """``A x`` for a ``DeviceCSR`` (``pcs_csr_spmv``); ``lanes`` overrides the matrix's lanes per row."""
    lib = L.gpu()
    nrows, ncols = A.shape
    out = torch.empty(nrows, dtype=A.dtype, device=x.device) if out is None else out
    if x.dtype != A.dtype or out.dtype != A.dtype or x.numel() != ncols or out.numel() != nrows \
            or not _dense_on(A.vals.device, x, out):
        raise ValueError(f'spmv: x and out must be contiguous {A.dtype} tensors of {ncols} and {nrows} elements on '
                         f'{A.vals.device}')
    L.check(lib.pcs_csr_spmv(L.dtcode(x), nrows, ncols, A.nnz, L.ptr(A.rowptr), L.ptr(A.colind), L.ptr(A.vals),
                             L.ptr(x), L.ptr(out), A.lanes if lanes is None else int(lanes), A.nchunks,
                             L.ptr(A.chunk_row), L.ptr(A.chunk_start), A.nlong, L.ptr(A.long_row),
                             L.ptr(A.long_first), L.ptr(A.partials), L.stream()), 'pcs_csr_spmv')
    return out


def spmm_plan(A, axis, nb):
    """Launch and workspace plan of pcs_csr_spmm for a ``DeviceCSR``-like ``A`` (``shape``, ``nchunks``): the
    kernel family ('cols': lanes across the nb columns, entries in order; 'rows': the pcs_csr_spmv scheme with
    the batch on grid y), the lanes across the columns, and the doubles of the partials workspace."""
    nb = int(nb)
    if axis not in (0, 1) or nb < 0:
        raise ValueError('spmm: axis is 0 or 1 and nb >= 0')
    if axis == 0 and nb > 1:
        width = 1
        while width < 64 and width < nb:
            width *= 2
        return {'family': 'cols', 'width': width, 'col_tiles': -(-nb // width), 'partials': 0}
    return {'family': 'rows', 'width': 0, 'col_tiles': 0, 'partials': nb * int(A.nchunks)}


def spmm(A, X, axis, out=None, accumulate=False):
    """``A X`` (axis 0, ``X`` of shape (ncols, nb)) or ``X A^T`` (axis 1, ``X`` of shape (nb, ncols)) for a
    ``DeviceCSR`` and a contiguous 2-D tensor (``pcs_csr_spmm``); ``accumulate`` adds the product to ``out``.  The
    partials workspace of the long rows is kept on ``A`` per batch size, so a captured loop replays with it."""
    lib = L.gpu()
    nrows, ncols = A.shape
    if X.dim() != 2 or axis not in (0, 1) or X.shape[axis] != ncols or X.dtype != A.dtype:
        raise ValueError(f'spmm: X must be a 2-D {A.dtype} tensor with {ncols} entries along axis {axis}')
    nb = int(X.shape[1 - axis])
    shape = (nrows, nb) if axis == 0 else (nb, nrows)
    if out is None:
        if accumulate:
            raise ValueError('spmm: accumulate needs out')
        out = torch.empty(shape, dtype=A.dtype, device=X.device)
    if tuple(out.shape) != shape or out.dtype != A.dtype or not _dense_on(A.vals.device, X, out):
        raise ValueError(f'spmm: X and out must be contiguous {A.dtype} tensors on {A.vals.device}, out of shape {shape}')
    need = spmm_plan(A, axis, nb)['partials']
    ws = A.partials
    if need > ws.numel():
        cache = A.__dict__.setdefault('spmm_partials', {})
        ws = cache.get(nb)
        if ws is None:
            ws = cache[nb] = torch.empty(need, dtype=torch.float64, device=A.vals.device)
    L.check(lib.pcs_csr_spmm(L.dtcode(X), int(axis), int(bool(accumulate)), nrows, ncols, A.nnz, L.ptr(A.rowptr),
                             L.ptr(A.colind), L.ptr(A.vals), L.ptr(X), L.ptr(out), nb, A.lanes, A.nchunks,
                             L.ptr(A.chunk_row), L.ptr(A.chunk_start), A.nlong, L.ptr(A.long_row),
                             L.ptr(A.long_first), L.ptr(ws), ws.numel(), L.stream()), 'pcs_csr_spmm')
    return out


# pcs_khatri_rao_*: the fused pair serves k n <= KR_MAX_NK and k + n <= KR_MAX_ROWS (derived in csrc/khatri_rao.hip)
KR_SLAB, KR_MAX_NK, KR_MAX_ROWS, KR_MAX_GROUPS = L.PCS_KR_SLAB, L.PCS_KR_MAX_NK, L.PCS_KR_MAX_ROWS, L.PCS_KR_MAX_GROUPS


def kr_fused_ok(k, n):
    """Whether the fused Khatri-Rao kernels serve factors of k and n rows."""
    return 1 <= k and 1 <= n and k * n <= KR_MAX_NK and k + n <= KR_MAX_ROWS


# Measured on an MI355X (profiles/kron_bench.jsonl): the fused forward beats mm(B * x, A^T) in every
# class it serves; the fused adjoint beats sum(mm(Y, A) * B, 0) up to k n = 256 in both dtypes and, in fp64, up to
# 32 x 32; with more rows in one factor (64 x 16, 100 x 10) and for 32 x 32 in fp32 the composition is faster.
KR_ADJ_FUSED_MAX_NK, KR_ADJ_FUSED_MAX_SIDE_F64 = 256, 32


def kr_route(k, n, dtype, adjoint):
    """'fused' or 'torch' for a dense Khatri-Rao pair of k and n rows: the derived limit first, then the measured
    boundary of the adjoint."""
    if not kr_fused_ok(k, n):
        return 'torch'
    if not adjoint or k * n <= KR_ADJ_FUSED_MAX_NK:
        return 'fused'
    if torch_dtype(dtype) == torch.float64 and max(k, n) <= KR_ADJ_FUSED_MAX_SIDE_F64:
        return 'fused'
    return 'torch'


def kr_fwd_plan(k, n, l):
    """Launch and workspace plan of pcs_khatri_rao_fwd: (slabs per workgroup, workgroups, doubles of partials).
    The l columns make ceil(l / KR_SLAB) slabs; at most KR_MAX_GROUPS workgroups share them in runs of ``spg``."""
    nslabs = -(-int(l) // KR_SLAB)
    spg = max(1, -(-nslabs // KR_MAX_GROUPS))
    ngroups = -(-nslabs // spg)
    return spg, ngroups, max(ngroups * int(k) * int(n), 1)


def khatri_rao_fwd(A, B, x, ws, out=None):
    """``(B * x) A^T`` (shape (n, k)) for dense row-major device matrices A (k, l) and B (n, l); ``ws``: the
    float64 partials workspace of ``kr_fwd_plan``."""
    lib = L.gpu()
    (k, l), n = A.shape, B.shape[0]
    if B.shape[1] != l or x.numel() != l or not (A.dtype == B.dtype == x.dtype) or not _dense_on(A.device, A, B, x, ws):
        raise ValueError('khatri_rao_fwd: A (k, l), B (n, l) and x (l) must be contiguous tensors of one dtype on one GPU')
    spg, ngroups, _ = kr_fwd_plan(k, n, l)
    out = torch.empty((n, k), dtype=A.dtype, device=A.device) if out is None else out
    L.check(lib.pcs_khatri_rao_fwd(L.dtcode(A), L.ptr(A), L.ptr(B), L.ptr(x), L.ptr(out), k, n, l, spg, ngroups,
                                   L.ptr(ws), ws.numel(), L.stream()), 'pcs_khatri_rao_fwd')
    return out


def khatri_rao_adj(A, B, Y, out=None):
    """``out[c] = B[:, c]^T Y A[:, c]`` for dense row-major device matrices A (k, l), B (n, l) and Y of n k values."""
    lib = L.gpu()
    (k, l), n = A.shape, B.shape[0]
    if B.shape[1] != l or Y.numel() != n * k or not (A.dtype == B.dtype == Y.dtype) or not _dense_on(A.device, A, B, Y):
        raise ValueError('khatri_rao_adj: A (k, l), B (n, l) and Y (n k) must be contiguous tensors of one dtype on one GPU')
    out = torch.empty(l, dtype=A.dtype, device=A.device) if out is None else out
    L.check(lib.pcs_khatri_rao_adj(L.dtcode(A), L.ptr(A), L.ptr(B), L.ptr(Y), L.ptr(out), k, n, l, L.stream()),
            'pcs_khatri_rao_adj')
    return out


# pcs_green_eval / pcs_mdm_apply (csrc/mdm.hip)
MDM_MAX_DIM, MDM_ROWS, MDM_SLAB, MDM_SMALL_ROWS, MDM_MAX_GROUPS = (L.PCS_MDM_MAX_DIM, L.PCS_MDM_ROWS, L.PCS_MDM_SLAB,
                                                                   L.PCS_MDM_SMALL_ROWS, L.PCS_MDM_MAX_GROUPS)
# Workgroups that fill the device for the plan below: 4 per CU of the 256 CUs.  A 256-thread workgroup puts one wave
# on each SIMD of a CU; the kernels do arithmetic on registers and LDS broadcasts with no global load in the inner
# loop, and the derivation stopped at two waves per SIMD (512 workgroups).  Measured (profiles/mdm_bench.jsonl, DESIGN
# 5.7): the 4096 x 65536 fp32 product on 512 workgroups ran at 0.60 of the pair rate that 1024 workgroups reach, so
# the plan asks for four waves per SIMD, which every kernel's register count admits (fp64: 3 to 4).
MDM_FILL = 4 * 256
MDM_MODES = {'radial': L.PCS_MDM_RADIAL, 'zonal': L.PCS_MDM_ZONAL}


def mdm_plan(nrows, ncols):
    """Launch plan of pcs_mdm_apply: ``(form, spg, ngroups, doubles of partials)``.  ``form`` is ``'col'`` for
    ``nrows <= MDM_SMALL_ROWS`` and ``'row'`` otherwise.  The ``max(ceil(ncols / MDM_SLAB), 1)`` slabs go to one
    group when the row tiles alone (``ceil(nrows / MDM_ROWS)``, 1 in the column form) number ``MDM_FILL`` or more;
    otherwise to the fewest groups that bring tiles x groups to ``MDM_FILL``, never less than one slab per group
    and never more than ``MDM_MAX_GROUPS`` groups.  Pure Python."""
    nrows, ncols = int(nrows), int(ncols)
    if nrows < 0 or ncols < 0:
        raise ValueError('mdm_plan: negative size')
    form = 'col' if nrows <= MDM_SMALL_ROWS else 'row'
    tiles = 1 if form == 'col' else -(-nrows // MDM_ROWS)
    nslabs = max(-(-ncols // MDM_SLAB), 1)
    want = 1 if tiles >= MDM_FILL else min(-(-MDM_FILL // tiles), nslabs, MDM_MAX_GROUPS)
    spg = -(-nslabs // want)
    ngroups = -(-nslabs // spg)
    return form, spg, ngroups, (ngroups * nrows if ngroups > 1 else 0)


def green_eval(spec, r, out=None):
    """``phi(r)`` element-wise for a float32 / float64 device tensor; ``spec``: a Green function's ``_device_spec()``."""
    lib = L.gpu()
    kind, k, p0, p1 = spec
    rc = r.contiguous()
    out = torch.empty_like(rc) if out is None else out
    if not _dense_on(rc.device, rc, out) or out.dtype != rc.dtype or out.numel() != rc.numel():
        raise ValueError('green_eval: r and out must be contiguous tensors of one dtype on one GPU')
    L.check(lib.pcs_green_eval(L.dtcode(rc), int(kind), int(k), float(p0), float(p1), L.ptr(rc), L.ptr(out), rc.numel(),
                               L.stream()), 'pcs_green_eval')
    return out.reshape(r.shape)


def mdm_apply(spec, mode, ord, P, Q, x, ws=None, plan=None, out=None):
    """``out[i] = sum_j phi(d(P_i, Q_j)) x[j]`` for device point sets P (nrows, dim) and Q (ncols, dim) and a vector
    x of ncols values, all of one dtype; ``spec`` is a Green function's ``_device_spec()``, ``mode`` ``'radial'``
    (``ord``-norm) or ``'zonal'``.  ``plan``: ``(spg, ngroups)``, by default that of ``mdm_plan``; ``ws``: the float64
    partials workspace of at least ``pcs_mdm_partials_len`` doubles (not needed for one group)."""
    lib = L.gpu()
    kind, k, p0, p1 = spec
    if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1] or x.numel() != Q.shape[0] or \
            not (P.dtype == Q.dtype == x.dtype) or not _dense_on(P.device, P, Q, x):
        raise ValueError('mdm_apply: P (nrows, dim), Q (ncols, dim) and x (ncols) must be contiguous tensors of one '
                         'dtype on one GPU')
    (nrows, dim), ncols = P.shape, Q.shape[0]
    spg, ngroups = mdm_plan(nrows, ncols)[1:3] if plan is None else plan
    need = ngroups * nrows if ngroups > 1 else 0
    if need and (ws is None or ws.dtype != torch.float64 or ws.numel() < need or not _dense_on(P.device, ws)):
        raise ValueError(f'mdm_apply: the plan needs a float64 workspace of {need} doubles on {P.device}')
    out = torch.empty(nrows, dtype=P.dtype, device=P.device) if out is None else out
    if out.dtype != P.dtype or out.numel() != nrows or not _dense_on(P.device, out):
        raise ValueError(f'mdm_apply: out must be a contiguous {P.dtype} tensor of {nrows} values on {P.device}')
    L.check(lib.pcs_mdm_apply(L.dtcode(P), int(kind), int(k), float(p0), float(p1), MDM_MODES[mode], float(ord), dim,
                              L.ptr(P), nrows, L.ptr(Q), ncols, L.ptr(x), L.ptr(out), int(spg), int(ngroups),
                              L.ptr(ws) if need else None, ws.numel() if need else 0, L.stream()), 'pcs_mdm_apply')
    return out


def _pool_call(fn, name, x, dims, block, scale, n_out):
    dims, block = [int(d) for d in dims], [int(b) for b in block]
    if len(dims) != len(block) or not 1 <= len(dims) <= 3:
        raise ValueError(f'{name}: 1 to 3 axes with one block size each')
    if not _dense_on(x.device, x):
        raise ValueError(f'{name}: the input must be a contiguous tensor on a GPU')
    out = torch.empty(n_out, dtype=x.dtype, device=x.device)
    L.check(fn(L.dtcode(x), L.ptr(x), L.ptr(out), len(dims), L.i64s(dims), L.i64s(block), float(scale), L.stream()),
            name)
    return out


def pooled_shape(dims, block):
    return tuple(-(-int(d) // int(b)) for d, b in zip(dims, block))


def pool(x, dims, block, scale=1.0):
    """``scale`` times the block sums of a C-order array of shape ``dims`` (1 to 3 axes), ragged blocks zero
    padded (``pcs_pool_fwd``)."""
    if x.numel() != int(np.prod(dims)):
        raise ValueError('pool: x must have prod(dims) elements')
    n_out = int(np.prod(pooled_shape(dims, block)))
    return _pool_call(L.gpu().pcs_pool_fwd, 'pcs_pool_fwd', x, dims, block, scale, n_out)


def unpool(y, dims, block, scale=1.0):
    """``out[p] = scale * y[block of p]`` for the unpooled shape ``dims`` (``pcs_pool_adj``)."""
    if y.numel() != int(np.prod(pooled_shape(dims, block))):
        raise ValueError('unpool: y must have one element per block')
    return _pool_call(L.gpu().pcs_pool_adj, 'pcs_pool_adj', y, dims, block, scale, int(np.prod(dims)))


def lap(x, dims, weights, steps, edge, adjoint=False):
    lib = L.gpu()
    out = torch.empty_like(x)
    fn = lib.pcs_lap_adj if adjoint else lib.pcs_lap_fwd
    L.check(fn(L.dtcode(x), L.ptr(x), L.ptr(out), L.i64s(dims), L.dbls(weights), L.dbls(steps), int(bool(edge)),
               L.stream()), 'pcs_lap')
    return out


def conv2d(x, dims, psf_dev, kh, kw, off0, off1, b=None, beta=0.0):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_conv2d(L.dtcode(x), L.ptr(x), L.ptr(out), int(dims[0]), int(dims[1]), L.ptr(psf_dev), int(kh),
                           int(kw), int(off0), int(off1), L.ptr(b), float(beta), L.stream()), 'pcs_conv2d')
    return out


def conv2d_plan(psf, off0, off1, adjoint, dtype):
    """Packed correlation window of a PSF for pcs_conv2d_planned (host pack, one device copy):
    returns (tier, device tensor) or None if the PSF is larger than the kernel's tiers."""
    lib = L.load()
    h = np.ascontiguousarray(np.asarray(psf, dtype=np.float64))
    kh, kw = h.shape
    tier = int(lib.pcs_conv2d_plan_tier(kh, kw, int(off0), int(off1)))
    if tier < 0:
        return None
    code = L.PCS_F32 if dtype == torch.float32 else L.PCS_F64
    nbytes = int(lib.pcs_conv2d_plan_bytes(code, kh, kw, int(off0), int(off1)))
    host = np.empty(nbytes // (4 if code == L.PCS_F32 else 8), dtype=np.float32 if code == L.PCS_F32 else np.float64)
    L.check(lib.pcs_conv2d_plan_pack(code, h.ctypes.data_as(L._pdbl), kh, kw, int(off0), int(off1), int(adjoint),
                                     host.ctypes.data), 'pcs_conv2d_plan_pack')
    return tier, torch.as_tensor(host).to(device=device())


def conv2d_planned(x, dims, plan, b=None, beta=0.0, out=None):
    lib = L.gpu()
    tier, w = plan
    out = torch.empty_like(x) if out is None else out
    L.check(lib.pcs_conv2d_planned(L.dtcode(x), L.ptr(x), L.ptr(out), int(dims[0]), int(dims[1]), L.ptr(w), int(tier),
                                   L.ptr(b), float(beta), L.stream()), 'pcs_conv2d_planned')
    return out


class FFTConv2D:
    """An FFT-domain Convolve2D plan (pcs_fftconv2d_*: rocFFT R2C / C2R on the zero-padded grid,
    PSF spectrum formed once) for one (dtype, image shape, PSF); freed with the object."""

    def __init__(self, psf, dims, off0, off1, dtype):
        lib = L.gpu()
        self._lib = lib
        h = np.ascontiguousarray(np.asarray(psf, dtype=np.float64))
        kh, kw = h.shape
        code = L.PCS_F32 if dtype == torch.float32 else L.PCS_F64
        handle = ctypes.c_void_p()
        L.check(lib.pcs_fftconv2d_create(code, int(dims[0]), int(dims[1]), h.ctypes.data_as(L._pdbl), kh, kw,
                                         int(off0), int(off1), ctypes.byref(handle)), 'pcs_fftconv2d_create')
        self.handle, self.dims, self.dtype = handle, tuple(dims), dtype

    def apply(self, x, adjoint=False, b=None, beta=0.0, out=None):
        """Conv x (+ beta b) or Conv^T x into a new (or the given) device vector."""
        if x.dtype != self.dtype:
            raise ValueError('FFTConv2D: dtype mismatch')
        out = torch.empty_like(x) if out is None else out
        n = self.dims[0] * self.dims[1]
        dev = torch.device('cuda', torch.cuda.current_device())
        for name, t in (('x', x), ('out', out), ('b', b)):
            if t is None:
                continue
            # the kernels read / write n0*n1 elements through raw pointers: validate before the call
            if not isinstance(t, torch.Tensor) or t.dtype != self.dtype or t.numel() != n or not t.is_contiguous() \
                    or t.device != dev:
                raise ValueError(f'FFTConv2D.apply: {name} must be a contiguous {self.dtype} tensor of {n} elements '
                                 f'on {dev} (got {getattr(t, "dtype", type(t))}, '
                                 f'{getattr(t, "numel", lambda: "?")()} elements on {getattr(t, "device", "?")})')
        L.check(self._lib.pcs_fftconv2d_apply(self.handle, L.ptr(x), L.ptr(out), int(bool(adjoint)), L.ptr(b),
                                              float(beta), L.stream()), 'pcs_fftconv2d_apply')
        return out

    def __del__(self):
        if getattr(self, 'handle', None):
            self._lib.pcs_fftconv2d_destroy(self.handle)
            self.handle = None


def conv1d(x, dims, axis, taps_dev, k, off):
    lib = L.gpu()
    out = torch.empty_like(x)
    L.check(lib.pcs_conv1d(L.dtcode(x), L.ptr(x), L.ptr(out), len(dims), L.i64s(dims), int(axis), L.ptr(taps_dev),
                           int(k), int(off), L.stream()), 'pcs_conv1d')
    return out


def scalar(x):
    return isinstance(x, Number)


# ---------------------------------------------------------------- pseudo-inverse: batched CG on the normal equations

# pcs_cg_*: most workgroups per system (the grid-stride loop takes a second pass from CG_MAX_BLOCKS * 256 + 1
# elements), most systems per launch, iterations per captured chunk
CG_MAX_BLOCKS, CG_MAX_NB, CG_CHUNK = L.PCS_CG_MAX_BLOCKS, L.PCS_CG_MAX_NB, 8
CG_RHO, CG_PQ, CG_ALPHA, CG_BETA, CG_TOL, CG_BNRM, CG_ACTIVE, CG_BREAKDOWN = range(8)   # doubles of one system's state


def cg_state(nb, dev):
    """The state block of `nb` systems, (nb, 8) float64 at exactly pcs_cg_state_bytes(nb) bytes."""
    return torch.empty(int(L.gpu().pcs_cg_state_bytes(int(nb))) // 8, dtype=torch.float64, device=dev).view(int(nb), 8)


def cg_partials(n, nb, dev):
    """The per-workgroup partial sums of `nb` systems of `n` unknowns: pcs_cg_nblocks(n, nb) doubles."""
    return torch.empty(int(L.gpu().pcs_cg_nblocks(int(n), int(nb))), dtype=torch.float64, device=dev)


def _cg_rows(name, first, *more):
    """(n, nb) of contiguous (nb, n) tensors of one dtype on one GPU."""
    if first.dim() != 2 or any(t.shape != first.shape or t.dtype != first.dtype for t in more) \
            or not _dense_on(first.device, first, *more):
        raise ValueError(f'{name}: the vectors must be contiguous (nb, n) tensors of one shape and dtype on one GPU')
    return int(first.shape[1]), int(first.shape[0])


def cg_init(B, R, rtol, atol, max_iter, state, partials, ctrl, hist):
    """``pcs_cg_init``: with ``R`` the initial residual, ||b_j||, tol_j, rho_j and active_j of every system and
    the loop control."""
    n, nb = _cg_rows('cg_init', B, R)
    L.check(L.gpu().pcs_cg_init(L.dtcode(B), L.ptr(B), L.ptr(R), n, nb, float(rtol), float(atol), int(max_iter),
                                L.ptr(state), L.ptr(partials), L.ptr(ctrl), L.ptr(hist), int(hist.numel()),
                                L.stream()), 'pcs_cg_init')


def cg_dir(R, P, state, ctrl):
    """``pcs_cg_dir``: P_j = beta_j P_j + R_j (P_j = R_j on iteration 0)."""
    n, nb = _cg_rows('cg_dir', R, P)
    L.check(L.gpu().pcs_cg_dir(L.dtcode(R), L.ptr(R), L.ptr(P), n, nb, L.ptr(state), L.ptr(ctrl), L.stream()),
            'pcs_cg_dir')


def cg_dot(P, Q, eps2, state, partials, ctrl):
    """``pcs_cg_dot``: pq_j = sum P_j (Q_j + eps2 P_j) and alpha_j = rho_j / pq_j."""
    n, nb = _cg_rows('cg_dot', P, Q)
    L.check(L.gpu().pcs_cg_dot(L.dtcode(P), L.ptr(P), L.ptr(Q), n, nb, float(eps2), L.ptr(state), L.ptr(partials),
                               L.ptr(ctrl), L.stream()), 'pcs_cg_dot')


def cg_update(X, R, P, Q, eps2, state, partials, ctrl, hist):
    """``pcs_cg_update``: X_j += alpha_j P_j, R_j -= alpha_j (Q_j + eps2 P_j), then rho, beta, the stop test, the
    iteration count and one history row."""
    n, nb = _cg_rows('cg_update', X, R, P, Q)
    L.check(L.gpu().pcs_cg_update(L.dtcode(X), L.ptr(X), L.ptr(R), L.ptr(P), L.ptr(Q), n, nb, float(eps2),
                                  L.ptr(state), L.ptr(partials), L.ptr(ctrl), L.ptr(hist), L.stream()),
            'pcs_cg_update')


class CGInfo:
    """What a solve leaves beside X: per-system ``rnorm`` (||r_j||), ``active`` and ``breakdown`` (NumPy arrays)
    and ``hist``, one row per iteration: (max_j ||r_j|| / ||b_j||, active systems after it)."""

    def __init__(self, rnorm, active, breakdown, hist):
        self.rnorm, self.active, self.breakdown, self.hist = rnorm, active, breakdown, hist


class CGNormal:
    """The buffers and the captured chunk of CG on ``(A^T A + eps^2 I) x = A^T y`` for one operator, batch size,
    dtype and eps (1 <= nb <= CG_MAX_NB).  One iteration is ``pcs_cg_dir``, ``Q = A^T (A P)`` through
    ``_apply_cols``, ``pcs_cg_dot``, ``pcs_cg_update``; ``chunk`` iterations are captured into one hipGraph
    (eager launches when the capture fails or ``use_graph`` is off) and the stop decision is read back
    asynchronously, one chunk behind -- the iterations issued past the stop write nothing."""

    def __init__(self, op, nb, dtype, eps, chunk=CG_CHUNK, use_graph=True):
        from .opt._loop import LoopControl
        dev = device()
        self.op, self.nb, self.n, self.dtype = op, int(nb), int(op.shape[1]), dtype
        self.eps2, self.chunk, self.use_graph = float(eps) ** 2, max(1, int(chunk)), bool(use_graph)
        self.X, self.R, self.P = (torch.zeros((self.nb, self.n), dtype=dtype, device=dev) for _ in range(3))
        self.state, self.partials = cg_state(self.nb, dev), cg_partials(self.n, self.nb, dev)
        self.ctl = LoopControl(dev)
        self.graph = None

    def adjoint(self, Y):
        """A^T on the rows of Y; a single row goes through ``_adj`` (no line loop, no stacking copy)."""
        if self.nb == 1:
            return self.op._adj(Y.reshape(-1)).reshape(1, -1).contiguous()
        return self.op._apply_cols(Y, 1, adjoint=True).contiguous()

    def normal(self, P):
        """A^T (A P) on the rows of P, never P's own storage."""
        Q = self.adjoint(self.op._apply(P.reshape(-1)).reshape(1, -1) if self.nb == 1 else self.op._apply_cols(P, 1))
        return Q.clone() if Q.data_ptr() == P.data_ptr() else Q

    def _iteration(self):
        cg_dir(self.R, self.P, self.state, self.ctl.ctrl)
        Q = self.normal(self.P)
        cg_dot(self.P, Q, self.eps2, self.state, self.partials, self.ctl.ctrl)
        cg_update(self.X, self.R, self.P, Q, self.eps2, self.state, self.partials, self.ctl.ctrl, self.ctl.hist)

    def _chunk(self):
        for _ in range(self.chunk):
            self._iteration()

    def solve(self, Y, rtol=1e-5, atol=0.0, maxiter=None, x0=None):
        """X (a new (nb, n) tensor), the iteration count and a CGInfo for the rows of ``Y`` (nb, m)."""
        from .opt._loop import capture_agreed
        if Y.dim() != 2 or Y.shape != (self.nb, self.op.shape[0]) or Y.dtype != self.dtype:
            raise ValueError(f'CGNormal.solve: Y must be a ({self.nb}, {self.op.shape[0]}) {self.dtype} tensor')
        maxiter = min(10 * self.n if maxiter is None else int(maxiter), 2 ** 31 - 2)
        B = self.adjoint(Y.contiguous())
        if x0 is None:
            self.X.zero_()
            self.R.copy_(B)
        else:
            self.X.copy_(x0.reshape(self.nb, self.n))
            self.R.copy_(B - (self.normal(self.X) + self.eps2 * self.X))      # scipy: r = b - matvec(x)
        ctl = self.ctl
        ctl.start(maxiter, 0, 0.0, False, chunk=self.chunk)
        if ctl.replaced:
            self.graph = None
        cg_init(B, self.R, rtol, atol, maxiter, self.state, self.partials, ctl.ctrl, ctl.hist)
        issued = 0
        if maxiter > 0:
            self._iteration()       # eager: whatever the operator builds on first use is built outside a capture
            issued = 1
            ctl.read_async()
        while issued < maxiter:
            if ctl.reserve(issued + self.chunk + 2):
                self.graph = None   # the captured chunk holds the history pointer
            if self.use_graph and self.graph is None:
                if ctl.poll(lag=0, drain=True) is not None:     # a capture synchronises anyway: already done?
                    break
                self.graph = capture_agreed(self._chunk)
                self.use_graph = self.graph is not None
            if self.graph is not None:
                self.graph.replay()
            else:
                self._chunk()
            issued += self.chunk
            ctl.read_async()
            if ctl.poll(lag=1) is not None:     # one chunk in flight behind the one whose control is read
                break
        torch.cuda.synchronize()
        it = ctl.iterations()
        st = self.state.cpu().numpy()
        if x0 is not None and np.any(st[:, CG_BNRM] == 0):                  # scipy: `if bnrm2 == 0: return b`
            self.X[torch.as_tensor(st[:, CG_BNRM] == 0).to(self.X.device)] = 0
        info = CGInfo(np.sqrt(st[:, CG_RHO]), st[:, CG_ACTIVE] != 0, st[:, CG_BREAKDOWN] != 0, ctl.rows(it).copy())
        return self.X.clone(), it, info


def cg_normal(op, Y, eps, rtol=1e-5, atol=0.0, maxiter=None, x0=None, chunk=CG_CHUNK, use_graph=True, plans=None):
    """``(A^T A + eps^2 I) X_j = A^T Y_j`` for the rows of the (nb, m) device tensor ``Y`` by conjugate gradients
    with SciPy's ``cg`` semantics (x0 = 0 unless given, stop when ||r|| < max(atol, rtol ||b||), maxiter = 10 n):
    returns X (nb, n), the iteration count (the most over the batch) and a CGInfo.  ``plans``: a dict in which
    the CGNormal of each (batch size, dtype, chunk, use_graph) is kept for the next call.  A batch of more than
    CG_MAX_NB systems is solved in slices."""
    Y = Y.contiguous()
    nb = int(Y.shape[0])
    if nb == 0:
        return torch.empty((0, op.shape[1]), dtype=Y.dtype, device=Y.device), 0, \
            CGInfo(np.zeros(0), np.zeros(0, bool), np.zeros(0, bool), np.zeros((0, 2)))
    plans = {} if plans is None else plans
    parts = []
    for s in range(0, nb, CG_MAX_NB):
        Ys = Y[s:s + CG_MAX_NB]
        key = (int(Ys.shape[0]), Y.dtype, int(chunk), bool(use_graph))
        plan = plans.get(key)
        if plan is None:
            plan = plans[key] = CGNormal(op, Ys.shape[0], Y.dtype, eps, chunk, use_graph)
        xs = None if x0 is None else x0.reshape(nb, -1)[s:s + CG_MAX_NB]
        parts.append(plan.solve(Ys, rtol, atol, maxiter, xs))
    if len(parts) == 1:
        return parts[0]
    info = CGInfo(*(np.concatenate([getattr(p[2], f) for p in parts]) for f in ('rnorm', 'active', 'breakdown')),
                  parts[int(np.argmax([p[1] for p in parts]))][2].hist)
    return torch.cat([p[0] for p in parts]), max(p[1] for p in parts), info


# ---------------------------------------------------------------- eigenvalues: thick-restart Lanczos with CGS2

# pcs_orth_*: largest basis (m), rows per group of pcs_orth_dots, most workgroups over the columns, their tile
ORTH_MAX_M, ORTH_GROUP, ORTH_MAX_BLOCKS, ORTH_TILE = L.PCS_ORTH_MAX_M, L.PCS_ORTH_GROUP, L.PCS_ORTH_MAX_BLOCKS, \
    L.PCS_ORTH_TILE
SPECTRAL_WHICH = ('LM', 'LA', 'SA', 'BE')
_EPS = float(np.finfo(np.float64).eps)


def orth_state(m, dev):
    """The state of a basis of `m` vectors: H (m x m), beta[m], omega[m], the breakdown index -- m m + 2 m + 1
    float64 at exactly pcs_orth_state_bytes(m) bytes."""
    return torch.empty(int(L.check_size(L.gpu().pcs_orth_state_bytes(int(m)), 'pcs_orth_state_bytes')) // 8,
                       dtype=torch.float64, device=dev)


def orth_partials(n, rows, dev):
    """The per-workgroup partial sums of a step against `rows` basis rows: pcs_orth_nblocks(n, rows) doubles."""
    return torch.empty(int(L.check_size(L.gpu().pcs_orth_nblocks(int(n), int(rows)), 'pcs_orth_nblocks')),
                       dtype=torch.float64, device=dev)


def _orth_basis(name, V, w):
    """(ldv, n) of a basis (rows, n) with unit column stride and the contiguous vector w, fp64 on one GPU."""
    if V.dim() != 2 or w.dim() != 1 or V.dtype != torch.float64 or w.dtype != torch.float64 or not V.is_cuda \
            or w.device != V.device or w.shape[0] != V.shape[1] or (V.shape[1] > 1 and V.stride(1) != 1) \
            or not w.is_contiguous():
        raise ValueError(f'{name}: V must be a (rows, n) float64 GPU tensor with unit column stride and w a '
                         f'contiguous float64 vector of n elements on the same GPU')
    return int(V.stride(0)) if V.shape[0] > 1 else max(int(V.stride(0)), int(V.shape[1])), int(V.shape[1])


def orth_state_init(state, m):
    L.check(L.gpu().pcs_orth_state_init(L.ptr(state), int(m), L.stream()), 'pcs_orth_state_init')


def orth_dots(V, s, w, h, partials):
    """``pcs_orth_dots``: h[i] = <V_i, w> for i <= s, h[s+1] = <w, w>."""
    ldv, n = _orth_basis('orth_dots', V, w)
    L.check(L.gpu().pcs_orth_dots(L.ptr(V), ldv, int(s), L.ptr(w), n, L.ptr(h), L.ptr(partials), L.stream()),
            'pcs_orth_dots')


def orth_update(V, s, w, h_in, h_out, partials):
    """``pcs_orth_update``: w -= sum_i h_in[i] V_i, then h_out as ``orth_dots`` of the new w."""
    ldv, n = _orth_basis('orth_update', V, w)
    L.check(L.gpu().pcs_orth_update(L.ptr(V), ldv, int(s), L.ptr(w), n, L.ptr(h_in), L.ptr(h_out), L.ptr(partials),
                                    L.stream()), 'pcs_orth_update')


def orth_commit(V, s, m, w, h1, h2, h3, brk, state):
    """``pcs_orth_commit``: column s of H, beta_s, omega_s, the breakdown index and row s + 1 of V."""
    ldv, n = _orth_basis('orth_commit', V, w)
    L.check(L.gpu().pcs_orth_commit(L.ptr(V), ldv, int(s), int(m), L.ptr(w), n, L.ptr(h1), L.ptr(h2), L.ptr(h3),
                                    float(brk), L.ptr(state), L.stream()), 'pcs_orth_commit')


class _OrthHip:
    """Basis, step and restart of ``eigsh_restarted`` on the pcs_orth_* kernels."""

    def __init__(self, n, m, dev):
        self.n, self.m, self.dev = n, m, dev
        ldv = n + (n & 1)                                      # even stride: every row starts 16-byte aligned
        self.V = torch.zeros((m + 1, ldv), dtype=torch.float64, device=dev)[:, :n]
        self.w = torch.empty(n, dtype=torch.float64, device=dev)
        self.h = [torch.empty(m + 1, dtype=torch.float64, device=dev) for _ in range(3)]
        self.partials = orth_partials(n, m, dev)
        self.state, self.fill_state = orth_state(m, dev), orth_state(m, dev)
        self.brk = 8.0 * _EPS * np.sqrt(n)

    def begin(self):
        orth_state_init(self.state, self.m)

    def _step(self, s, state):
        h1, h2, h3 = self.h
        orth_dots(self.V, s, self.w, h1, self.partials)
        orth_update(self.V, s, self.w, h1, h2, self.partials)
        orth_update(self.V, s, self.w, h2, h3, self.partials)
        orth_commit(self.V, s, self.m, self.w, h1, h2, h3, self.brk, state)

    def step(self, s, w):
        self.w.copy_(w.reshape(-1))
        self._step(s, self.state)

    def read(self):
        m = self.m
        st = self.state.cpu().numpy()
        return st[:m * m].reshape(m, m), st[m * m:m * m + m], st[m * m + m:m * m + 2 * m], int(st[-1])

    def fill(self, row, vec):
        """Row `row` = `vec` orthogonalised twice against the rows before it and normalised (same kernels)."""
        orth_state_init(self.fill_state, self.m)
        self.w.copy_(vec)
        self._step(row - 1, self.fill_state)
        return int(self.fill_state[-1:].cpu().numpy()[0]) < 0

    def rotate(self, Y):
        keep = Y.shape[1]
        Yd = torch.as_tensor(np.ascontiguousarray(Y.T)).to(self.dev)
        self.V[:keep].copy_(torch.matmul(Yd, self.V[:self.m]))
        self.V[keep].copy_(self.V[self.m])


class _OrthTorch:
    """The same steps with torch products on any device (the comparator of tools/bench_spectral.py and what the
    CPU test tier runs); no host synchronisation inside a step either."""

    def __init__(self, n, m, dev):
        self.n, self.m, self.dev = n, m, dev
        f = dict(dtype=torch.float64, device=dev)
        self.V = torch.zeros((m + 1, n), **f)
        self.H, self.beta, self.omega = torch.zeros((m, m), **f), torch.zeros(m, **f), torch.zeros(m, **f)
        self.broke_at = torch.full((), -1.0, **f)
        self.brk = 8.0 * _EPS * np.sqrt(n)

    def begin(self):
        self.H.zero_()
        self.beta.zero_()
        self.omega.zero_()
        self.broke_at.fill_(-1.0)

    def _cgs2(self, s, w):
        Vs = self.V[:s + 1]
        h1 = torch.mv(Vs, w)
        before = torch.dot(w, w)
        w = w - torch.mv(Vs.t(), h1)
        h2 = torch.mv(Vs, w)
        w = w - torch.mv(Vs.t(), h2)
        h3 = torch.mv(Vs, w)
        b = torch.sqrt(torch.dot(w, w))
        broke = b <= self.brk * torch.sqrt(before)
        zero = torch.zeros_like(b)
        self.V[s + 1] = torch.where(broke, torch.zeros_like(w), w / b)
        return h1 + h2, torch.where(broke, zero, b), torch.where(broke, zero, h3.abs().max() / b), broke

    def step(self, s, w):
        c, b, om, broke = self._cgs2(s, w.reshape(-1).to(torch.float64))
        self.H[:s + 1, s] = c
        self.H[s, :s + 1] = c
        self.beta[s], self.omega[s] = b, om
        first = broke & (self.broke_at < 0)
        self.broke_at.copy_(torch.where(first, torch.full_like(self.broke_at, float(s)), self.broke_at))

    def read(self):
        return self.H.cpu().numpy().copy(), self.beta.cpu().numpy().copy(), self.omega.cpu().numpy().copy(), \
            int(self.broke_at.item())

    def fill(self, row, vec):
        return not bool(self._cgs2(row - 1, vec.clone())[3].item())

    def rotate(self, Y):
        keep = Y.shape[1]
        Yd = torch.as_tensor(np.ascontiguousarray(Y.T)).to(self.dev)
        self.V[:keep] = torch.matmul(Yd, self.V[:self.m])
        self.V[keep] = self.V[self.m]


def spectral_select(theta, k, which):
    """Indices (ascending) of the `k` wanted values of the ascending array `theta`: 'LA' the largest, 'SA' the
    smallest, 'LM' the largest in magnitude, 'BE' k // 2 from the low end and the rest from the high end."""
    m = len(theta)
    if which == 'LA':
        idx = np.arange(m - k, m)
    elif which == 'SA':
        idx = np.arange(k)
    elif which == 'LM':
        idx = np.argsort(np.abs(theta), kind='stable')[m - k:]
    elif which == 'BE':
        idx = np.concatenate([np.arange(k // 2), np.arange(m - (k - k // 2), m)])
    else:
        raise ValueError(f"which must be one of {SPECTRAL_WHICH}, got {which!r}")
    return np.sort(idx)


def spectral_ncv(n, k, ncv=None):
    """The basis size: ``ncv``, or ARPACK's default min(n, max(2 k + 1, 20))."""
    return int(ncv) if ncv is not None else min(int(n), max(2 * int(k) + 1, 20))


def eigsh_restarted(apply, n, k, which='LM', ncv=None, tol=0, maxiter=None, v0=None, device=None, orth='hip'):
    """``k`` eigenvalues of the symmetric operator ``apply`` (fp64 device vector of ``n`` in, the same out) by
    thick-restart Lanczos (Wu & Simon 2000) with full CGS2 re-orthogonalisation against a stored basis of
    ``m = ncv`` (default min(n, max(2 k + 1, 20))) fp64 vectors; what ``scipy.sparse.linalg.eigsh`` computes with
    ``return_eigenvectors=False``: an ascending fp64 NumPy array.

    One cycle runs the steps j0..m-1 with no host synchronisation (``orth='hip'``: the pcs_orth_* kernels;
    ``orth='torch'``: torch products, on any device).  Then H = V^T A V and the step scalars come to the host once,
    ``eigh(H)`` gives the Ritz pairs (theta_i, y_i) and |beta_{m-1} y_i[m-1]| their residuals.  Pair i has
    converged when its residual is at most max(tol_eff max(eps^(2/3), |theta_i|), 8 eps max |theta|), tol_eff =
    ``tol`` or eps: ARPACK's criterion and a round-off floor.  Until the ``k`` wanted pairs have, the basis is
    rotated onto keep = min(k + min(nconv, (m - k) // 2), m - 1) Ritz vectors (one matmul), H = diag(theta), row
    ``keep`` becomes the last Lanczos vector and the next step's Gram-Schmidt coefficients are the coupling row.
    A breakdown (an invariant subspace, a zero operator) fills the next row with a seeded random vector,
    orthogonalised twice by the same step and normalised, and resumes there: the coupling is zero, and the rest of
    a multiple eigenvalue is found this way.  ``maxiter``: restarts, default 10 n; then
    ``scipy.sparse.linalg.ArpackNoConvergence`` with the converged values.  ``v0``: start vector (default: seeded).
    """
    n, k = int(n), int(k)
    if which not in SPECTRAL_WHICH:
        raise ValueError(f"which must be one of {SPECTRAL_WHICH}, got {which!r}")
    if not 0 < k < n:
        raise ValueError(f'k must satisfy 0 < k < n = {n}, got {k}')
    m = spectral_ncv(n, k, ncv)
    if not k < m <= n:
        raise ValueError(f'ncv must satisfy k < ncv <= n, got ncv = {m} for k = {k}, n = {n}')
    if orth not in ('hip', 'torch'):
        raise ValueError(f"orth must be 'hip' or 'torch', got {orth!r}")
    if orth == 'hip' and m > ORTH_MAX_M:
        raise ValueError(f'the device basis holds at most {ORTH_MAX_M} vectors, got ncv = {m}')
    dev = torch.device(device) if device is not None else device_of_orth(orth)
    be = (_OrthHip if orth == 'hip' else _OrthTorch)(n, m, dev)
    gen = torch.Generator(device=dev).manual_seed(0)    # on the device: no host vector of n, the same bits every run
    if v0 is None:
        q = torch.randn(n, generator=gen, dtype=torch.float64, device=dev)
    else:
        q = v0.detach() if isinstance(v0, torch.Tensor) else torch.as_tensor(np.asarray(v0, dtype=np.float64))
        q = q.to(device=dev, dtype=torch.float64).reshape(-1)
        if q.numel() != n:
            raise ValueError(f'v0 must have {n} elements, got {q.numel()}')
    nrm = float(torch.linalg.vector_norm(q))
    if not (nrm > 0 and np.isfinite(nrm)):
        raise ValueError('v0 must be a nonzero finite vector')
    be.V[0] = q / nrm
    tol_eff = float(tol) if tol else _EPS
    maxiter = 10 * n if maxiter is None else int(maxiter)
    H = np.zeros((m, m))
    betas = np.zeros(m)
    j0, restarts = 0, 0
    while True:
        j = j0
        while True:                                     # one cycle; a breakdown resumes it one row further
            be.begin()
            for s in range(j, m):
                be.step(s, apply(be.V[s]))
            Hs, beta, _, broke_at = be.read()
            end = m if broke_at < 0 else broke_at + 1
            for s in range(j, end):
                H[:s + 1, s] = Hs[:s + 1, s]
                H[s, :s + 1] = Hs[s, :s + 1]
            betas[j:end] = beta[j:end]
            if broke_at < 0 or broke_at == m - 1:
                break
            j = broke_at + 1
            if not be.fill(j, torch.randn(n, generator=gen, dtype=torch.float64, device=dev)):
                raise RuntimeError('eigsh_restarted: a random vector fell into the span of the basis')
        if not np.all(np.isfinite(H)):
            raise ValueError('eigsh_restarted: the operator returned values that are not finite')
        theta, Y = np.linalg.eigh(H)
        res = np.abs(betas[m - 1] * Y[m - 1])
        bar = np.maximum(tol_eff * np.maximum(_EPS ** (2.0 / 3.0), np.abs(theta)), 8.0 * _EPS * np.abs(theta).max())
        conv = res <= bar
        want = spectral_select(theta, k, which)
        nconv = int(conv[want].sum())
        if nconv == k:
            return theta[want].copy()
        if restarts >= maxiter:
            from scipy.sparse.linalg import ArpackNoConvergence
            raise ArpackNoConvergence(f'eigsh_restarted: {nconv} of {k} eigenvalues converged in {restarts} '
                                      f'restarts', theta[want][conv[want]].copy(), None)
        keep = min(k + min(nconv, (m - k) // 2), m - 1)
        idx = spectral_select(theta, keep, which)
        be.rotate(Y[:, idx])
        H[:] = 0.0
        H[np.arange(keep), np.arange(keep)] = theta[idx]
        j0, restarts = keep, restarts + 1


def device_of_orth(orth):
    """The default device of ``eigsh_restarted``: the current GPU ('hip' has no other; 'torch' takes the CPU
    when no GPU is visible)."""
    if orth == 'torch' and not torch.cuda.is_available():
        return torch.device('cpu')
    L.gpu()
    return device()
