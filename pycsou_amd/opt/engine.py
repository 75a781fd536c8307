"""Fused, hipGraph-replayed PDS engine for 2-D TV problems (single GPU).

Pattern-matches the problem a user script builds with the reference API
(``F = (1/2)*SquaredL2Loss(dim, data=y) [* Convolve2D]``, ``K = Gradient(shape,
kind='forward')``, ``H = lam * L21Norm(groups=tile(arange(N), 2))`` or ``lam * L1Norm``,
``G = None / NonNegativeOrthant / Segment``) and runs ``PrimalDualSplitting.iterate``
(``pycsou/opt/proxalgs.py:343-394`` inside ``pycsou/core/solver.py:55-76``) as

    per iteration:  [GRADBUF only: r = h*x - y ; g = h^T r]   (pcs_conv2d_planned x2)
                    pcs_pds2d_step        x, z  ->  x', z', per-block norm partials
                    pcs_pds_reduce_finalize      -> relative improvements, iteration
                                                    counter, device stop flag

captured once into a hipGraph of ``chunk`` iterations (x/z ping-pong between two
buffers) and replayed.  The stop flag implements the reference loop condition on the
device, so a replay after convergence is a sequence of no-op launches and the
iteration count is exactly the reference's.
"""

import collections
import ctypes
import os

import numpy as np
import torch

from .. import _lib as L
from .. import _ops as O
from ..core.functional import ProxFuncPostComp
from ..core.map import DiffMapComp, DiffMapShifted
from ..func.base import IndicatorFunctional, NullDifferentiableFunctional, NullProximableFunctional
from ..func.penalty import L1Norm, L21Norm, SquaredL2Norm
from ..linop.base import HomothetyMap
from ..linop.conv import Convolve2DOp
from ..linop.diff import GradientOp, LaplacianOp
from . import _loop
from ._loop import LaunchTimer, LoopState

# images at least this large launch chunks from C instead of replaying a captured graph
NATIVE_MIN_PIXELS = int(os.environ.get('PCS_NATIVE_MIN_PIXELS', 1 << 20))

# deferred finalization (pcs_pds2d_args.fin_partials, csrc/pds_ctrl.hpp): each step launch finalizes the
# previous launch's partials in a workgroup of its own instead of reducing its own at its end.
# PCS_DEFER_FIN=0: diagnostics, the in-launch reduction.
DEFER_FIN = os.environ.get('PCS_DEFER_FIN', '1') != '0'


def _half_loss_data(F):
    """If F is (1/2) * SquaredL2Norm.shifter(s) return s (the shift = -data), else None."""
    if (isinstance(F, DiffMapComp) and isinstance(F.map1, HomothetyMap) and F.map1.cst == 0.5
            and isinstance(F.map2, DiffMapShifted) and isinstance(F.map2.map, SquaredL2Norm)
            and not np.isscalar(F.map2.shift)):
        return F.map2.shift
    return None


def match_g(G):
    """G = None / NullProximableFunctional / NonNegativeOrthant / Segment -> {'gkind', 'seg'} or None."""
    if G is None or isinstance(G, NullProximableFunctional):
        return {'gkind': L.PCS_G_NULL, 'seg': (0.0, 1.0)}
    if isinstance(G, IndicatorFunctional) and G.kind == 'nonneg':
        return {'gkind': L.PCS_G_NONNEG, 'seg': (0.0, 1.0)}
    if isinstance(G, IndicatorFunctional) and G.kind == 'segment':
        return {'gkind': L.PCS_G_SEGMENT, 'seg': G.params}
    return None


def match_h(H, ncomp, N):
    """H = lam * (L1Norm | L21Norm over the ncomp components of each pixel) -> {'hkind', 'lam'} or None."""
    base, lam = H, 1.0
    if isinstance(H, ProxFuncPostComp):
        if H.shift != 0:
            return None
        base, lam = H.prox_func, float(H.scale)
    if ncomp > 1 and isinstance(base, L21Norm) and base.pixel_d == ncomp and base.dim == ncomp * N:
        return {'hkind': L.PCS_H_L21, 'lam': lam}
    if isinstance(base, L1Norm) and base.dim == ncomp * N:
        return {'hkind': L.PCS_H_L1, 'lam': lam}
    return None


def match_f(F, N, conv_of, conv_fkind, conv_key='conv'):
    """F = 0, (1/2) SquaredL2Loss(y) on N samples, or that composed with the problem's convolution ->
    {'fkind'[, 'shift'[, conv_key]]} or None.  `conv_of(op)`: what the engine keeps of `op` when it is a
    convolution of this problem (a Convolve2DOp on the image, a chain of Convolve1D on the volume), else
    None; such an F gets `conv_fkind`."""
    if F is None or isinstance(F, NullDifferentiableFunctional):
        return {'fkind': L.PCS_F_NULL}
    s = _half_loss_data(F)
    if s is not None and O.numel(s) == N:
        return {'fkind': L.PCS_F_DENOISE, 'shift': s}
    if isinstance(F, DiffMapComp):
        conv, s = conv_of(F.map2), _half_loss_data(F.map1)
        if conv and s is not None and O.numel(s) == N:
            return {'fkind': conv_fkind, 'shift': s, conv_key: conv}
    return None


def conv2d_on(shape):
    """match_f's `conv_of` of the 2-D problems: a Convolve2DOp on `shape`."""
    return lambda op: op if isinstance(op, Convolve2DOp) and op.dims == shape else None


def fused_spec(head, *parts):
    """The K-specific entries `head` and the matched H, G and F entries as one spec; None when any
    of them did not match."""
    if any(p is None for p in parts):
        return None
    spec = dict(head)
    for p in parts:
        spec.update(p)
    return spec


def nmarch_taps(t0, t1, half, dtype=np.float32):
    """The N = Conv^T Conv tables of the normal-operator march kernel (pds_nmarch.hpp) for a
    separable PSF with centred taps t0 (axis 0) and t1 (axis 1) of half width `half`, padded to
    the tier H (3 or 7): (Conv v)[i] = sum_d c[d] v[i - d], c[d] = t[H + d].  Away from the
    edges N is the autocorrelation a[e] = sum_m c[m] c[m + e] (window taps a[|q - 2H|],
    q = 0..4H); on the H samples nearest each edge the zero boundary removes the terms of the
    samples outside the image: N[j, k] = a[j - k] - E[j][k], E[j][k] = sum_{i < 0} c[i - j] c[i - k]
    (left / top, j, k < H) and the mirror sum over i >= n on the right / bottom.  Computed in fp64,
    returned in the layout the kernels read (64 + 32 H values) as `dtype` (the fp32 march: float32; the
    fp64 march, pds_nm64.hip: float64)."""
    H = 3 if half <= 3 else 7
    out = np.zeros(64 + 32 * H)

    def taps(t):
        w = np.zeros(2 * H + 1)
        w[H - half:H + half + 1] = np.asarray(t, dtype=np.float64)
        return lambda d: w[H + d] if -H <= d <= H else 0.0

    def window(c):
        a = [sum(c(m) * c(m + e) for m in range(-H, H + 1)) for e in range(2 * H + 1)]
        return [a[abs(q - 2 * H)] for q in range(4 * H + 1)]

    def e_lo(c):  # E[j][k], j, k < H: the rows i = -H..-1 above the image
        return [[sum(c(i - j) * c(i - k) for i in range(-H, 0)) for k in range(H)] for j in range(H)]

    def e_hi(c):  # the last H samples, j = n-H+jj, k = n-H+kk, rows i = n..n+H-1 (i - j = H + ii - jj)
        return [[sum(c(H + ii - jj) * c(H + ii - kk) for ii in range(H)) for kk in range(H)] for jj in range(H)]

    c0, c1 = taps(t0), taps(t1)
    out[0:4 * H + 1] = window(c0)
    out[32:32 + 4 * H + 1] = window(c1)
    ev_lo, ev_hi, eh_lo, eh_hi = e_lo(c0), e_hi(c0), e_lo(c1), e_hi(c1)
    base = 64
    for j in range(H):  # E_v rows: [j][k]
        out[base + 8 * j:base + 8 * j + H] = ev_lo[j]
        out[base + 8 * H + 8 * j:base + 8 * H + 8 * j + H] = ev_hi[j]
    for k in range(H):  # E_h transposed: ET[k][c] for the left band, ET[k][i] (column n1-8+i) right
        for cc in range(H):
            out[base + 16 * H + 8 * k + cc] = eh_lo[cc][k]
            out[base + 24 * H + 8 * k + (8 - H) + cc] = eh_hi[cc][k]
    return out.astype(dtype)


def match_stencil2d(F, G, H, K, has_H):
    """Engine spec for the general-stencil fused step (pcs_pds2d_stencil_step): K a 2-D Gradient of
    any kind (pycsou/linop/diff.py:777-882) or a 2-D Laplacian (diff.py:885-957), H = lam * L1 / L21,
    F = 0, (1/2) SquaredL2Loss(y), or (1/2) SquaredL2Loss(y) * Convolve2D (grad F through the
    correlation kernel into a buffer); None otherwise."""
    if not has_H:
        return None
    if isinstance(K, GradientOp) and len(K.dims) == 2:
        kk, ncomp, w = {'forward': L.PCS_K_GRAD_FORWARD, 'backward': L.PCS_K_GRAD_BACKWARD,
                        'centered': L.PCS_K_GRAD_CENTERED}[K.kind], 2, (1.0, 1.0)
    elif isinstance(K, LaplacianOp) and len(K.dims) == 2:
        kk, ncomp, w = L.PCS_K_LAPLACIAN, 1, tuple(K.weights)
    else:
        return None
    shape = tuple(K.dims)
    N = shape[0] * shape[1]
    head = {'stencil': True, 'shape': shape, 'steps': tuple(K.steps), 'kkind': kk, 'ncomp': ncomp,
            'weights': w, 'edge': bool(K.edge)}
    return fused_spec(head, match_h(H, ncomp, N), match_g(G), match_f(F, N, conv2d_on(shape), L.PCS_F_GRADBUF))


def match_pds2d(F, G, H, K, has_H):
    """Return an engine spec dict if (F, G, H, K) is a fused-engine problem, else None."""
    if not has_H or not isinstance(K, GradientOp) or len(K.dims) != 2 or K.kind != 'forward':
        return None
    shape = K.dims
    N = shape[0] * shape[1]
    return fused_spec({'shape': shape, 'steps': tuple(K.steps)}, match_h(H, 2, N), match_g(G),
                      match_f(F, N, conv2d_on(shape), L.PCS_F_SEPCONV))


def apgd_g_kind(G):
    """(kind, lam, seg) of an APGD G the fused steps take (pcs_apgd_step, pcs_apgd2d_step): null,
    lam * L1Norm, NonNegativeOrthant or Segment; None otherwise."""
    lam = 1.0
    if isinstance(G, ProxFuncPostComp) and G.shift == 0 and isinstance(G.prox_func, L1Norm):
        G, lam = G.prox_func, float(G.scale)
    if isinstance(G, L1Norm):
        return L.PCS_APGD_G_L1, lam, (0.0, 1.0)
    g = match_g(G)
    return None if g is None else (g['gkind'], 1.0, tuple(g['seg']))


def sep_rtol(dtype):
    """How close to rank one a PSF must be to run as two 1-D passes in `dtype`."""
    return 2e-7 if dtype == torch.float32 else 1e-13


def match_apgd2d(F, G, dtype=torch.float64):
    """Engine spec if (F, G) is a fused-APGD problem: F = (1/2) * SquaredL2Loss(y) * Convolve2D with a
    PSF that is separable to the tolerance of `dtype` and reaches <= 7 samples either side, G null /
    lam * L1Norm / NonNegativeOrthant / Segment; None otherwise."""
    if not (isinstance(F, DiffMapComp) and isinstance(F.map2, Convolve2DOp)):
        return None
    conv = F.map2
    shape = tuple(conv.dims)
    s = _half_loss_data(F.map1)
    if len(shape) != 2 or s is None or O.numel(s) != shape[0] * shape[1]:
        return None
    gk = apgd_g_kind(G)
    if gk is None:
        return None
    sep = conv.separable(rtol=sep_rtol(dtype))
    if sep is None or sep[2] > 7:
        return None
    return {'apgd': True, 'shape': shape, 'shift': s, 'conv': conv, 'sep': sep, 'gkind': gk[0], 'lam': gk[1],
            'seg': gk[2]}


def apgd_momentum(acceleration, d, k, t_old):
    """(t, a) of APGD iteration k (pycsou/opt/proxalgs.py:592-598): a = (t_old - 1) / t multiplies
    (x_t - past_aux).  'CD' reads the iteration index, 'BT' the previous t, anything else has no momentum."""
    if acceleration == 'BT':
        t = (1 + np.sqrt(1 + 4 * t_old ** 2)) / 2
    elif acceleration == 'CD':
        t = (k + d) / d
    else:
        t = t_old = 1
    return t, (t_old - 1) / t


def apgd_coeffs(acceleration, d, k0, n, t_old):
    """The coefficients a of iterations k0 .. k0 + n - 1 continuing from t_old, and the last t."""
    out = []
    for k in range(k0, k0 + n):
        t_old, a = apgd_momentum(acceleration, d, k, t_old)
        out.append(a)
    return out, t_old


def with_fields(a, **fields):
    """A copy of the argument struct `a` with `fields` set: a candidate or a query never touches the
    struct an engine launches with, so nothing is saved and restored."""
    b = type(a)()
    ctypes.pointer(b)[0] = a
    for k, v in fields.items():
        setattr(b, k, v)
    return b


def query(fn, a, *rest, **fields):
    """fn(a with `fields`, *rest) for a planning entry point of the library (support, path, block
    counts).  Those launch nothing and dereference nothing, but they look at which pointers are set and
    how they are aligned: a pointer the loop binds or allocates later is given an address the engine
    already holds (or, on a host without a GPU, any 16-byte-aligned number) as a placeholder for the
    query."""
    return fn(ctypes.byref(with_fields(a, **fields)), *rest)


def step_args(spec, dtype, tau, sigma, rho, lay=None, cls=L.PdsArgs, with_k=True):
    """The scalar fields of a 2-D step's arguments (pcs_pds2d_args, or `cls` = pcs_pds2d_stencil_args,
    which share them by name) from a spec and the step sizes; `lay`: the SlabLayout of a row slab.
    `with_k`: K's kind, edge rule and weights from the spec, which only the general-stencil specs carry."""
    a = cls()
    a.dtype = L.dtype_code(dtype)
    a.hkind, a.gkind = spec['hkind'], spec['gkind']
    a.n0, a.n1 = spec['shape']
    a.tau, a.sigma, a.rho, a.lam = float(tau), float(sigma), float(rho), spec['lam']
    a.step0, a.step1 = spec['steps']
    a.seg_a, a.seg_b = spec['seg']
    if lay is not None:
        # Inherited difference, kept field for field: a slab states K in full, and for a spec of
        # match_pds2d (which carries no K) with the forward Gradient's own values -- edge True, weights
        # (1, 1) -- where the whole-image forward engine (`with_k` False below) leaves kkind, edge, w0 and
        # w1 at 0.  The forward-Gradient kernels read none of them.
        a.row0, a.rows = lay.row0, lay.rows
        a.kkind, a.edge = spec.get('kkind', L.PCS_K_GRAD_FORWARD), int(spec.get('edge', True))
        a.w0, a.w1 = spec.get('weights', (1.0, 1.0))
        return a
    if with_k:
        a.kkind, a.edge = spec['kkind'], int(spec['edge'])
        a.w0, a.w1 = spec['weights']
    if cls is L.PdsArgs:  # one slab, the whole image: no halos
        a.row0, a.rows = 0, a.n0
    return a


class SepPSF:
    """The device operands of a separable PSF in the compute dtype: `taps` (axis 0, axis 1) of half width
    `half`; after normal() those of grad F = N x - Conv^T y as well: the tables `ntaps` of
    N = Conv^T Conv (nmarch_taps) and `cty` = Conv^T y."""

    @classmethod
    def of(cls, spec, dtype, dev, max_half=None):
        """The operands of the spec's PSF; None when it is not rank one to sep_rtol(dtype) or reaches
        more than `max_half` samples either side."""
        sep = spec['sep'] if 'sep' in spec else spec['conv'].separable(rtol=sep_rtol(dtype))
        if sep is None or (max_half is not None and sep[2] > max_half):
            return None
        return cls(sep, spec, dtype, dev)

    def __init__(self, sep, spec, dtype, dev):
        self.sep, self.spec, self.dtype, self.dev = sep, spec, dtype, dev
        self.half = sep[2]
        self.taps = [torch.as_tensor(t).to(device=dev, dtype=dtype) for t in sep[:2]]
        self.ntaps = self.cty = None

    def normal(self, cty64=None, tables=True):
        """Conv^T y formed once in fp64 (y = -shift exactly; `cty64`: a slab's window of it) and cast,
        and with `tables` the N tables in the compute dtype (the fp64 march reads them in fp64)."""
        t0, t1, half = self.sep
        if tables:
            np_dtype = np.float64 if self.dtype == torch.float64 else np.float32
            self.ntaps = torch.as_tensor(nmarch_taps(t0, t1, half, np_dtype)).to(self.dev)
        if cty64 is None:
            cty64 = self.spec['conv']._adj(-O.to_dev(self.spec['shift'], torch.float64))
        self.cty = cty64.to(self.dtype).contiguous()
        return self

    def attach(self, eng, a):
        """The operands as the engine's `taps`, `cty`, `ntaps` and in its step arguments."""
        eng.taps, eng.cty, eng.ntaps = self.taps, self.cty, self.ntaps
        a.half = self.half
        a.taps0, a.taps1 = self.taps[0].data_ptr(), self.taps[1].data_ptr()
        if self.cty is not None:
            a.cty = self.cty.data_ptr()
        if self.ntaps is not None:
            a.ntaps = self.ntaps.data_ptr()


class APGD2DEngine(LoopState):
    """Device state + loop of one fused 2-D APGD problem (match_apgd2d): every iteration is ONE launch
    (pcs_apgd2d_step: grad F by the two-pass normal-operator march, G.prox, the momentum step, the
    diagnostics' norms and the loop test), launched from C in chunks (pcs_apgd2d_run) with the chunk's
    momentum coefficients from the host; the control block is read once per chunk."""

    def __init__(self, spec, dtype, tau, x0, acceleration='CD', d=75., chunk=32):
        self.lib = L.gpu()
        self.spec, self.dtype = spec, dtype
        self.acceleration, self.d = acceleration, d
        n0, n1 = spec['shape']
        self.N = n0 * n1
        self.x0 = x0.to(dtype)
        dev = self.x0.device
        self.X = [torch.empty(self.N, dtype=dtype, device=dev) for _ in range(2)]
        self.AUX = [torch.empty(self.N, dtype=dtype, device=dev) for _ in range(2)]
        self.chunk = max(2, chunk + (chunk % 2))
        a = L.Apgd2dArgs()
        a.dtype = L.dtype_code(dtype)
        a.gkind, a.n0, a.n1 = spec['gkind'], n0, n1
        SepPSF.of(spec, dtype, dev).normal(tables=False).attach(self, a)
        a.tau, a.lam = float(tau), float(spec['lam'])
        a.seg_a, a.seg_b = spec['seg']
        a.x, a.xn = self.X[0].data_ptr(), self.X[1].data_ptr()
        a.aux, a.aux_n = self.AUX[0].data_ptr(), self.AUX[1].data_ptr()
        self.args = a
        if self.lib.pcs_apgd2d_supported(ctypes.byref(a)) != 1:
            raise ValueError('problem not supported by the fused APGD step')
        self._init_reduction(a, dev, self.lib.pcs_apgd2d_nblocks, self.lib.pcs_apgd2d_ws_bytes)

    def coeffs(self, k0, n, t_old):
        return apgd_coeffs(self.acceleration, self.d, k0, n, t_old)

    def start(self, max_iter, min_iter, thr):
        """Iterate x0, past_aux 0, a fresh loop control and a history with room for the first chunks."""
        self.X[0].copy_(self.x0)
        self.AUX[0].zero_()
        return self.ctl.start(max_iter, min_iter, thr, False, chunk=self.chunk)

    def launch(self, coeffs):
        """len(coeffs) (even) iterations from buffer parity 0, launched back to back."""
        self.args.hist = self.hist.data_ptr()
        L.check(self.lib.pcs_apgd2d_run(ctypes.byref(self.args), L.dbls(coeffs), len(coeffs), L.stream()),
                'pcs_apgd2d_run')

    def run(self, max_iter, min_iter, accuracy_threshold):
        """The reference loop from x0 (solver.py:55-76): (n, x, past_aux, past_t, hist[n])."""
        total = self.start(max_iter, min_iter, accuracy_threshold)
        n_chunks = -(-total // self.chunk)
        t_old = 1
        for k in range(n_chunks):
            self.ctl.reserve((k + 1) * self.chunk + 2)
            coeffs, t_old = self.coeffs(k * self.chunk, self.chunk, t_old)
            self.launch(coeffs)
            self.ctl.read_async()
            if self.ctl.poll(lag=1) is not None:  # one chunk in flight behind the one whose control is read
                break
        torch.cuda.synchronize()
        n = self.ctl.iterations()
        h = self.ctl.rows(n)[:, 0].copy()
        past_t = self.coeffs(0, n, 1)[1]
        return n, self.X[n % 2], self.AUX[n % 2], past_t, h


def forward_normal(half, dtype):
    """Whether PDS2DEngine runs a separable PSF of this half width as grad F = N x - Conv^T y (the
    normal-operator march kernel, pds_nmarch.hpp).  PCS_NMARCH=0: diagnostics, the four-pass march kernel
    (grad F = Conv^T (Conv x - y))."""
    return dtype == torch.float32 and half <= 7 and os.environ.get('PCS_NMARCH', '1') != '0'


class PDS2DEngine(LoopState):
    """Device state + captured loop for one fused 2-D PDS problem."""

    def __init__(self, spec, dtype, tau, sigma, rho, x0, z0, chunk=32, use_graph=True):
        dev = self._init_state(spec, dtype, x0, z0, chunk, use_graph)
        a = step_args(spec, dtype, tau, sigma, rho, with_k=False)
        fk = spec['fkind']
        if fk in (L.PCS_F_DENOISE, L.PCS_F_SEPCONV):
            # y = -shift (exact), so x + shift == x - y bit for bit
            self.y = -O.to_dev(spec['shift'], dtype)
            a.y = self.y.data_ptr()
        if fk == L.PCS_F_SEPCONV:
            psf = SepPSF.of(spec, dtype, dev)
            if psf is not None:
                if forward_normal(psf.half, dtype):
                    psf.normal()
                psf.attach(self, a)
            else:
                fk = L.PCS_F_GRADBUF
                self._init_grad_conv(spec['conv'], dev)
                a.gbuf = self.Gb.data_ptr()
        a.fkind = fk
        self._init_loop_state(a, fk, self.lib.pcs_pds2d_nblocks, self.lib.pcs_pds2d_ws_bytes, fk != L.PCS_F_GRADBUF)

    # ---- the pieces of a constructor (the subclasses' differ in the arguments between them)
    def _init_state(self, spec, dtype, x0, z0, chunk, use_graph, ncomp=2):
        """The iterate ping-pong buffers (z of `ncomp` components) and the loop's shape; every attribute
        only some problems fill, at its empty value; the device."""
        self.lib = L.gpu()
        self.spec = spec
        self.dtype = dtype
        n0, n1 = spec['shape']
        self.N = n0 * n1
        dev = x0.device
        self.X = [x0.to(dtype).clone(), torch.empty(self.N, dtype=dtype, device=dev)]
        self.Z = [z0.to(dtype).clone(), torch.empty(ncomp * self.N, dtype=dtype, device=dev)]
        self.chunk = max(2, chunk + (chunk % 2))
        self.use_graph = use_graph
        self.conv = self.plans = self.taps = self.cty = self.ntaps = None
        self.defer = self.nm_fused = False
        self._fixed_p = 0
        return dev

    def _init_grad_conv(self, conv, dev):
        """GRADBUF: the device PSF copies / packed correlation plans / the FFT plan exist before any
        capture; the residual and gradient buffers."""
        self.conv = conv
        conv._h.get(self.dtype), conv._hf.get(self.dtype)
        self.plans = (conv.plan(self.dtype, False), conv.plan(self.dtype, True))
        if self.plans[0] is None or self.plans[1] is None:
            conv.fft(self.dtype)
        self.R = torch.empty(self.N, dtype=self.dtype, device=dev)
        self.Gb = torch.empty(self.N, dtype=self.dtype, device=dev)

    def _init_loop_state(self, a, fk, nblocks_fn, ws_bytes_fn, may_run_native):
        """The step arguments `a` are complete but for what the loop owns (LoopState._init_reduction:
        in-kernel reduce + finalize, one launch per iteration)."""
        self.args, self.fkind = a, fk
        self._init_reduction(a, self.X[0].device, nblocks_fn, ws_bytes_fn)
        self.graph = None
        # large images: each chunk is launched back to back from C (pcs_pds2d_run) -- per-launch
        # host cost is far below the step, and back-to-back launches measured faster than
        # replaying a captured graph of the same launches; small images keep the graph
        self.native = may_run_native and self.N >= NATIVE_MIN_PIXELS

    def _alloc_partials(self, a, dev):
        """[nblocks][4] partials; with deferred finalization two such arrays, swapped with the
        iterate parity (the launch of parity p writes array p and finalizes array 1 - p)."""
        defer = DEFER_FIN and isinstance(a, L.PdsArgs)
        # pcs_pds2d_run may run an iteration as two row-band launches (the band-paired schedule, csrc/pds.hip),
        # which leave the partials of both: run_nblocks is the count its launches write and its flush reduces;
        # the arrays hold the largest count any PCS_RUN_BANDS setting can ask for
        self.run_nblocks = cap = self.nblocks
        if defer:
            self._bind(a, 0)  # the iterates only: self.defer is still False
            self.run_nblocks = int(query(self.lib.pcs_pds2d_run_nblocks, a, -1, partials=a.x))
            cap = max(cap, self.run_nblocks, int(query(self.lib.pcs_pds2d_run_nblocks, a, 1, partials=a.x)))
        nb4 = cap * 4
        self.partials = _loop.loop_buffer((2 if defer else 1) * nb4, dev)
        self.part_halves = [self.partials[:nb4], self.partials[nb4:]] if defer else [self.partials]
        a.partials = self.partials.data_ptr()
        if defer:
            a.fin_partials = self.part_halves[1].data_ptr()
        self.defer = defer

    def _bind(self, a, p):
        """Point the step's iterate buffers at parity p (reads buffers p, writes 1 - p)."""
        a.x, a.xn = self.X[p].data_ptr(), self.X[1 - p].data_ptr()
        a.z, a.zn = self.Z[p].data_ptr(), self.Z[1 - p].data_ptr()
        if self.defer:
            a.partials, a.fin_partials = self.part_halves[p].data_ptr(), self.part_halves[1 - p].data_ptr()

    def _flush(self, next_p, hist, run=False):
        """Deferred finalization: finalize the last launch's partials (parity 1 - next_p) if they
        are pending (pcs_pds_finalize_pending; a no-op when the loop has stopped).  `run`: the last
        iteration came from pcs_pds2d_run (its partials count), not from a single step."""
        if self.defer:
            L.check(self.lib.pcs_pds_finalize_pending(L.ptr(self.part_halves[1 - next_p]),
                                                      self.run_nblocks if run else self.nblocks,
                                                      L.ptr(self.ctrl), L.ptr(hist), L.stream()),
                    'pcs_pds_finalize_pending')

    # the fused step / the chunk of n steps launched back to back from C, on self.args
    def _step_call(self, st):
        L.check(self.lib.pcs_pds2d_step(ctypes.byref(self.args), st), 'pcs_pds2d_step')

    def _run_call(self, n):
        L.check(self.lib.pcs_pds2d_run(ctypes.byref(self.args), int(n), L.stream()), 'pcs_pds2d_run')

    # one iteration with parity p (reads buffers p, writes 1-p)
    def _iteration(self, p, hist):
        a, st = self.args, L.stream()
        if self.fkind == L.PCS_F_GRADBUF:
            self._grad_conv(p, st)
        self._bind(a, p)
        a.hist = hist.data_ptr()
        self._step_call(st)

    def _grad_conv(self, p, st, around=lambda name, launch: launch()):
        """GRADBUF: r = h*x - y (residual fused into the forward pass), g = h^T r -- the
        packed-plan correlation kernel (pcs_conv2d_planned) when the PSF fits its tiers.  Each of the
        two launches runs as around(name, launch) (the kernel timers put their events there)."""
        c, a, lib = self.conv, self.args, self.lib
        fwd, adj = self.plans
        n0, n1 = c.dims
        if fwd is not None and adj is not None:
            around('conv_fwd', lambda: L.check(lib.pcs_conv2d_planned(
                a.dtype, L.ptr(self.X[p]), L.ptr(self.R), n0, n1, L.ptr(fwd[1]), fwd[0], L.ptr(self.y), -1.0, st),
                'pcs_conv2d_planned'))
            around('conv_adj', lambda: L.check(lib.pcs_conv2d_planned(
                a.dtype, L.ptr(self.R), L.ptr(self.Gb), n0, n1, L.ptr(adj[1]), adj[0], None, 0.0, st),
                'pcs_conv2d_planned'))
            return
        # wider PSFs: the FFT-domain plan (rocFFT; cost independent of the PSF size)
        f = c.fft(self.dtype)
        around('conv_fwd', lambda: f.apply(self.X[p], b=self.y, beta=-1.0, out=self.R))
        around('conv_adj', lambda: f.apply(self.R, adjoint=True, out=self.Gb))

    def _chunk(self, hist):
        for i in range(self.chunk):
            self._iteration(i % 2, hist)

    def _chunk_native(self, hist):
        a = self.args
        self._bind(a, 0)
        a.hist = hist.data_ptr()
        self._run_call(self.chunk)

    def _capture(self):
        """One chunk on the current history captured into self.graph (the history is captured by
        pointer: whoever replaces it drops the graph)."""
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._chunk(self.hist)
        self.graph = g

    # ---- fixed-count loop for benchmarking (bench.py): no early stop, optional per-step events
    def prepare_fixed(self, total_iters, chunk):
        """Device state for `total_iters` iterations that never stop early, captured in
        graphs of `chunk` (even) iterations."""
        self.chunk = chunk
        self._fixed_p = 0
        self.ctl.start_fixed(total_iters, total_iters + 1)
        if not self.native:
            self._capture()
        torch.cuda.synchronize()

    def replay(self):
        if self.native:
            self._chunk_native(self.hist)
        else:
            self.graph.replay()

    def advance_fixed(self, n):
        """Enqueue exactly n iterations of a prepare_fixed() loop, continuing from the buffer
        parity the previous call left (odd counts allowed): native images as one
        pcs_pds2d_run of n launches, graph images as whole captured chunks while the parity
        allows plus eager single iterations."""
        p = self._fixed_p
        if self.native:
            a = self.args
            self._bind(a, p)
            a.hist = self.hist.data_ptr()
            self._run_call(int(n))
            self._fixed_p = p ^ (int(n) & 1)
            self._flush(self._fixed_p, self.hist, run=True)
            return
        while n >= self.chunk and p == 0:
            self.graph.replay()
            n -= self.chunk
        for _ in range(n):
            self._iteration(p, self.hist)
            p ^= 1
        self._fixed_p = p
        self._flush(p, self.hist)

    def _start_timed(self, n):
        """Fresh loop state that runs all of n eager launches on the history as it is (the in-kernel
        reduce + finalize is timed too); n, cut to what the history holds."""
        n = min(n, (self.hist.numel() - 2) // 2 - 1)
        self.ctl.start_fixed(n + 1)
        return n

    def time_iteration_kernels(self, n):
        """Median duration (ms) of each kernel of an iteration over n eager iterations, HIP
        events on the launching stream around every launch: {'step': ...} and, for a
        non-separable PSF, {'conv_fwd': ..., 'conv_adj': ...}.  (Median: a single launch
        delayed by an unrelated host or driver event does not move it.)"""
        a = self.args
        n = self._start_timed(n)
        timed = LaunchTimer()
        for i in range(n):
            p = i % 2
            if self.fkind == L.PCS_F_GRADBUF:
                self._grad_conv(p, L.stream(), timed)
            self._bind(a, p)
            a.hist = self.hist.data_ptr()
            timed('step', lambda: self._step_call(L.stream()))
        self._flush(n % 2, self.hist)
        return timed.result(np.median)

    def time_step_kernel(self, n, stream=None):
        """Average duration (ms) of the fused step kernel over `n` eager launches, measured
        with HIP events on the stream the kernel runs on."""
        a = self.args
        n = self._start_timed(n)
        timed = LaunchTimer(stream)
        a.hist = self.hist.data_ptr()
        for i in range(n):
            self._bind(a, i % 2)
            timed('step', lambda: self._step_call(L.stream()))
        self._flush(n % 2, self.hist)
        return timed.result()['step']

    def run(self, max_iter, min_iter, accuracy_threshold, has_dual=True):
        ctl = self.ctl
        total = ctl.start(max_iter, min_iter, accuracy_threshold, has_dual, chunk=self.chunk)
        if ctl.replaced:
            self.graph = None
        for k in range(-(-total // self.chunk)):
            if ctl.reserve((k + 1) * self.chunk + 2):
                self.graph = None
            if self.native:
                self._chunk_native(self.hist)
            elif self.use_graph:
                if self.graph is None:
                    self._capture()
                self.graph.replay()
            else:
                self._chunk(self.hist)
                if ctl.stopped():
                    break
                continue
            ctl.read_async()
            if ctl.poll(lag=1) is not None:  # one chunk in flight behind the one whose control is read
                break
        self._flush(0, self.hist, run=self.native)  # every chunk is an even number of launches
        torch.cuda.synchronize()
        n = ctl.iterations()
        return n, self.X[n % 2], self.Z[n % 2], ctl.rows(n)


Route = collections.namedtuple('Route', 'march fkind nm_fused drop')


def stencil_march_on():
    """PCS_STENCIL_MARCH=0: the general-stencil engine always runs the tile kernel."""
    return os.environ.get('PCS_STENCIL_MARCH', '1') != '0'


def nm_fused_route(lib, a, **fields):
    """Whether the library runs the step `a` (separable operands and N tables set) as the fused
    normal-operator march: one launch (pds_nmarch.hpp for backward / centred K in fp32, pds_nm64.hip for
    every Gradient K in fp64) that reads no gradient buffer -- asked with none."""
    return query(lib.pcs_pds2d_path, a, gbuf=None, **fields) in L.PCS_PATH_FUSED_NORMAL


def route_stencil2d(lib, a):
    """Where a general-stencil problem runs.  `a`: its pcs_pds2d_args with every candidate pointer set --
    the iterates, partials, y or the gradient buffer, and for a separable PSF fkind SEPCONV with taps, cty
    and ntaps beside the gradient buffer.  Route(march, fkind, nm_fused, drop): `march` False is the tile
    kernel (pcs_pds2d_stencil_step, on the spec's own fkind); otherwise pcs_pds2d_step takes `a` with
    `fkind` and the optional pointers named in `drop` cleared.  A separable PSF runs, in this order of
    preference, as the fused normal-operator march (`nm_fused`), as the two-launch form (N x by the
    in-plane normal-operator kernel into the gradient buffer, then the march step: no ntaps), or like any
    other PSF through the correlation passes (GRADBUF: no cty either)."""
    fk, nm_fused, drop = a.fkind, False, ()
    if not stencil_march_on():
        return Route(False, fk, False, drop)
    if fk == L.PCS_F_SEPCONV:
        nm_fused = nm_fused_route(lib, a)
        drop = () if nm_fused else ('ntaps',)
        if query(lib.pcs_pds2d_supported, a, **dict.fromkeys(drop)) != 1:
            fk, nm_fused, drop = L.PCS_F_GRADBUF, False, ('cty', 'ntaps')
    march = query(lib.pcs_pds2d_supported, a, fkind=fk, **dict.fromkeys(drop)) == 1
    return Route(march, fk, nm_fused, drop)


class PDS2DStencilEngine(PDS2DEngine):
    """Device state + loop of the general-stencil fused step (pcs_pds2d_stencil_step): the same
    loop machinery as PDS2DEngine (device stop flag, chunks launched from C for large images,
    hipGraph replay otherwise, GRADBUF convolutions before the step), another step kernel."""

    def __init__(self, spec, dtype, tau, sigma, rho, x0, z0, chunk=32, use_graph=True):
        dev = self._init_state(spec, dtype, x0, z0, chunk, use_graph, spec['ncomp'])
        fk = spec['fkind']
        if fk in (L.PCS_F_DENOISE, L.PCS_F_GRADBUF):
            self.y = -O.to_dev(spec['shift'], dtype)  # y = -shift exactly
        if fk == L.PCS_F_GRADBUF:
            self._init_grad_conv(spec['conv'], dev)
        gsrc = None if fk == L.PCS_F_NULL else (self.Gb if fk == L.PCS_F_GRADBUF else self.y)
        # images the general-stencil row-marching kernel covers (pds_smarch.hpp: 64-column strips,
        # 4-column groups; fp32 and fp64, every K kind in fp64) run through pcs_pds2d_step with K in
        # the args; the rest through the tile kernel (pcs_pds2d_stencil_step): route_stencil2d decides
        # on the march's candidate arguments
        a = step_args(spec, dtype, tau, sigma, rho)
        a.fkind = fk
        self._bind(a, 0)
        a.partials = a.x  # stands in until the loop state exists (query())
        if fk == L.PCS_F_DENOISE:
            a.y = gsrc.data_ptr()
        elif fk == L.PCS_F_GRADBUF:
            a.gbuf = gsrc.data_ptr()
            psf = SepPSF.of(spec, dtype, dev, max_half=7) if stencil_march_on() else None
            if psf is not None:
                psf.normal().attach(self, a)
                a.fkind, a.y = L.PCS_F_SEPCONV, self.y.data_ptr()
        self.march, fk, self.nm_fused, drop = route_stencil2d(self.lib, a)
        if self.march:
            a.fkind = fk
            for name in drop:
                setattr(a, name, None)
        else:
            a = step_args(spec, dtype, tau, sigma, rho, cls=L.StencilArgs)
            a.fkind = fk
            if gsrc is not None:
                a.g = gsrc.data_ptr()
        lib = self.lib
        self._init_loop_state(a, fk, lib.pcs_pds2d_nblocks if self.march else lib.pcs_pds2d_stencil_nblocks,
                              lib.pcs_pds2d_ws_bytes if self.march else lib.pcs_pds2d_stencil_ws_bytes,
                              fk != L.PCS_F_GRADBUF)

    def time_iteration_kernels(self, n):
        """As PDS2DEngine's; with a separable PSF (SEPCONV here) either the fused normal-operator
        march (one launch, `nm_fused`) or one pcs_pds2d_step call holding two launches (N x into the
        gradient buffer, the step), timed as 'step' together and 'conv_nx' alone."""
        res = PDS2DEngine.time_iteration_kernels(self, n)
        if self.fkind == L.PCS_F_SEPCONV and not self.nm_fused:
            a, lib = self.args, self.lib
            timed = LaunchTimer()
            for i in range(min(n, 50)):
                timed('conv_nx', lambda: L.check(lib.pcs_conv2d_sep_ata_planes(
                    a.dtype, L.ptr(self.X[i % 2]), L.ptr(self.Gb), 1, a.n0, a.n1, L.ptr(self.taps[0]), 2 * a.half + 1,
                    a.half, L.ptr(self.taps[1]), 2 * a.half + 1, a.half, L.stream()), 'pcs_conv2d_sep_ata_planes'))
            res.update(timed.result(np.median))
        return res

    def _step_call(self, st):
        if self.march:
            return PDS2DEngine._step_call(self, st)
        L.check(self.lib.pcs_pds2d_stencil_step(ctypes.byref(self.args), st), 'pcs_pds2d_stencil_step')

    def _run_call(self, n):
        if self.march:
            return PDS2DEngine._run_call(self, n)
        L.check(self.lib.pcs_pds2d_stencil_run(ctypes.byref(self.args), int(n), L.stream()), 'pcs_pds2d_stencil_run')


def match_masked_stencil2d(F, G, H, K, has_H):
    """Engine spec for the masked data-fidelity problem of the reference notebook (TV-LAD inpainting,
    solved by ChambollePockSplitting, pycsou/opt/proxalgs.py:628-716): F = 0,
    K = LinOpVStack(Masking(mask), K_s) (pycsou/linop/base.py:259-279, linop/sampling.py:125-196),
    H = ProxFuncHStack(L1Loss(dim=m, data=y), lam * L1Norm | lam * L21Norm) (func/base.py:21-89,
    func/loss.py:222-268) with K_s / the second block any problem match_stencil2d takes with F = 0;
    G = None / NonNegativeOrthant / Segment.  Only images the row march covers (n1 % 4 == 0, at
    least two 64-column strips); None otherwise (the generic per-operator path runs it)."""
    from ..core.functional import ProxFuncPreComp
    from ..func.base import ProxFuncHStack
    from ..linop.base import LinOpStack
    from ..linop.sampling import Masking
    if not has_H or not (F is None or isinstance(F, NullDifferentiableFunctional)):
        return None
    if not isinstance(K, LinOpStack) or K.axis != 0 or len(K.linops) != 2 or not isinstance(H, ProxFuncHStack) \
            or len(H.proxfuncs) != 2:
        return None
    M, Ks = K.linops
    h_loss, h_s = H.proxfuncs
    if not isinstance(M, Masking) or not hasattr(M, 'sampling_bool'):
        return None
    if not (isinstance(h_loss, ProxFuncPreComp) and isinstance(h_loss.prox_func, L1Norm)
            and isinstance(h_loss.scale, (int, float)) and h_loss.scale == 1 and not np.isscalar(h_loss.shift)):
        return None
    m = int(M.shape[0])
    if h_loss.dim != m or O.numel(h_loss.shift) != m:
        return None
    spec = match_stencil2d(None, G, h_s, Ks, True)
    if spec is None or spec['fkind'] != L.PCS_F_NULL:
        return None
    n0, n1 = spec['shape']
    if M.shape[1] != n0 * n1 or n1 % 4 or n1 <= 64:
        return None
    # the fused block marks unsampled pixels by a NaN in the expanded data: data that is not finite
    # itself would be read as unsampled there, so it takes the generic path (which propagates it, as
    # the reference's L1Loss prox does)
    sh = h_loss.shift
    finite = bool(torch.isfinite(sh).all().item()) if isinstance(sh, torch.Tensor) else bool(np.isfinite(sh).all())
    if not finite:
        return None
    spec['mask'] = M.sampling_bool
    spec['mask_shift'] = h_loss.shift  # = -y
    spec['m'] = m
    return spec


class PDS2DMaskEngine(PDS2DEngine):
    """The masked data-fidelity problem (match_masked_stencil2d) on the general-stencil row march with
    the masked block inside the step (pcs_pds2d_args.mkind = PCS_M_L1LOSS, pds_smarch.hpp SM_F_MASK):
    one launch per iteration.  The masked dual block z_m is held expanded to the image (ZM, 0 where the
    mask is False) and y expanded with NaN there; the solver's z = [z_m; z_s] is assembled on return."""

    def __init__(self, spec, dtype, tau, sigma, rho, x0, z0, chunk=32, use_graph=True):
        m = spec['m']
        dev = self._init_state(spec, dtype, x0, z0[m:], chunk, use_graph, spec['ncomp'])
        N = self.N
        self.idx = torch.as_tensor(np.flatnonzero(spec['mask']).astype(np.int64)).to(dev)
        self.ZM = [torch.zeros(N, dtype=dtype, device=dev), torch.zeros(N, dtype=dtype, device=dev)]
        self.ZM[0][self.idx] = z0[:m].to(dtype)
        self.ym = torch.full((N,), float('nan'), dtype=dtype, device=dev)
        self.ym[self.idx] = -O.to_dev(spec['mask_shift'], dtype)  # y = -shift, exactly
        a = step_args(spec, dtype, tau, sigma, rho)
        a.fkind = L.PCS_F_NULL
        a.mkind, a.ym = L.PCS_M_L1LOSS, self.ym.data_ptr()
        self._bind(a, 0)
        a.partials = a.x  # stands in until the loop state exists (query())
        if self.lib.pcs_pds2d_supported(ctypes.byref(a)) != 1:
            raise ValueError('masked data-fidelity problem not supported by the fused step')
        self._init_loop_state(a, L.PCS_F_NULL, self.lib.pcs_pds2d_nblocks, self.lib.pcs_pds2d_ws_bytes, True)

    def _bind(self, a, p):
        PDS2DEngine._bind(self, a, p)
        a.zm, a.zmn = self.ZM[p].data_ptr(), self.ZM[1 - p].data_ptr()

    def z_full(self, p):
        """The solver's dual variable [z_m; z_s] of buffer parity p (the reference layout)."""
        return torch.cat([self.ZM[p][self.idx], self.Z[p]])

    def run(self, max_iter, min_iter, accuracy_threshold, has_dual=True):
        n, x, _, h = PDS2DEngine.run(self, max_iter, min_iter, accuracy_threshold, has_dual)
        return n, x, self.z_full(n % 2), h


def engine_class(spec):
    """The engine class of a fused spec (proxalgs and bench.py build engines through this)."""
    from .engine3d import PDS3DEngine
    if spec.get('ndim', 2) == 3:
        return PDS3DEngine
    if 'mask' in spec:
        return PDS2DMaskEngine
    return PDS2DStencilEngine if spec.get('stencil') else PDS2DEngine
