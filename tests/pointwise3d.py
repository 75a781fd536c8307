"""Element-wise one-step parity of the fused 3-D PDS kernels (k_pds3d, k_pds3d_gen and the gradient chains of
pycsou_amd/opt/engine3d.py): inputs, fp64 oracle, rounding bound, the matrix.  The 3-D counterpart of
tests/pointwise.py, whose Bound, comparator, Segment, lam and column names it reuses.

The other 3-D tests start from x0 = z0 = 0, blur with one symmetric Gaussian on all three axes, use unit
steps and no G, and compare a relative L2 norm over the volume.  Here the state is generic (x0, z0, y all
non-zero), the taps differ per axis in length and values (U(0.5, 1.5) normalised to sum 1, not symmetric, even
lengths included), the steps may differ per axis, prox_G and the dual projection bind inside every wave, and
every voxel of x and of the three components of z is compared.

The bound (`bound`).  One iteration is (pycsou/opt/proxalgs.py:343-355)

    x~ = prox_G(x - tau grad F(x) - tau K^T z)        grad F(x) = C^T (C x - y)  |  x - y  |  0,  C = C2 C1 C0
    z~ = prox_{sigma H*}(z + sigma K (2 x~ - x))
    x' = rho x~ + (1 - rho) x,   z' = rho z~ + (1 - rho) z.

The derivation of tests/pointwise.py holds with three axes.  Each C_a has non-negative taps of sum 1, so
|C_a v| <= |v|_inf and |C_a^T v| <= |v|_inf, hence |grad F(x)| <= |x0|_inf + |y|_inf whatever the order in which
an engine groups the six passes (C0^T (C0 (C12^T C12 x) - C12^T y) included: every partial result is a
sub-convex combination of x or of y).  A first difference of step s (forward, backward, or the centred
(0.5, -0.5) pair and its one-sided edge rows) is bounded by 2 |v|_inf / |s| and so is its adjoint:

    kfac = sum_a 2 / |step_a|
    Mx   = |x0|_inf + tau (|x0|_inf + |y|_inf) + tau |z0|_inf kfac
    Mz   = |z0|_inf + 3 sigma Mx kfac                           (|2 x~ - x| <= 3 Mx)

bound every intermediate of the primal and of the dual update.  An operation on operands of magnitude <= M
errs by at most eps M, and to first order the errors of a chain of c operations add: |error| <= c eps M, with
c the roundings on the longest chain of one step: the six 1-D passes of the blur, 2 (l0 + l1 + l2)
multiply-adds, plus 16 for everything else (tap roundings, the residual, the tau / sigma / 1 / step scalings,
the stencil's adds over three axes, the prox, the relaxation); 16 alone without a blur.  The in-plane
normal-operator kernel (two passes with the 2 l - 1 taps of C_a^T C_a) has a shorter chain than the four
passes it replaces, so the same c covers it.  prox_G, the Fenchel prox of lam L1 / lam L21 and the convex
combination with rho are 1-Lipschitz and pass the error on.  For `nit` iterations the bar is nit c eps M, a
first-order budget for the one or two iterations run here (tests/test_step_pointwise3d_cpu.py checks a plain
fp32 evaluation against it).  The asserted bar is this derived quantity and never a number read off a
kernel.

Inputs are rounded to the dtype under test before the fp64 oracle sees them.
"""

import collections

import numpy as np

from oracle import pycsou_ref as OR
from tests.pointwise import D_COL, LAM, P_COL, SEG, Bound, _round, compare  # noqa: F401  (re-exported)

U1, NU = (1.0, 1.0, 1.0), (2.0, 0.5, 1.0)  # NU: one unit step and two different non-unit ones
TAPS = ('t0', 't1', 't2')


def make_state(shape, lens, seed, lam, dtype=np.float32):
    """fp64 arrays holding values of `dtype`: taps t0, t1, t2 of `lens` entries from U(0.5, 1.5) normalised to
    sum 1 (None where the length is 0), x0 and y from U(-0.5, 1.5), z0 = lam N(0, 1) with 3 N entries."""
    rng = np.random.default_rng(seed)
    N = int(np.prod(shape))
    st = {}
    for name, l in zip(TAPS, lens):
        t = rng.uniform(0.5, 1.5, max(int(l), 1))
        st[name] = _round(t / t.sum(), dtype) if l else None
    st['x0'] = _round(rng.uniform(-0.5, 1.5, N), dtype)
    st['y'] = _round(rng.uniform(-0.5, 1.5, N), dtype)
    st['z0'] = _round(lam * rng.standard_normal(3 * N), dtype)
    return st


def make_problem(shape, kind, hname, fk, gname, edge=True, steps=U1, lam=LAM, seed=0, dtype=np.float32):
    """One problem of the matrix.  kind: 'forward' | 'backward' | 'centered'; fk: 'null' | 'denoise' |
    'sepL0xL1xL2' (one Convolve1D per axis, L_a taps along axis a); gname: '' | 'nonneg' | 'segment'."""
    shape = tuple(int(n) for n in shape)
    lens = tuple(int(v) for v in fk[3:].split('x')) if fk.startswith('sep') else (0, 0, 0)
    assert len(shape) == 3 and len(lens) == 3, (shape, fk)
    p = dict(shape=shape, N=int(np.prod(shape)), kind=kind, hname=hname, fk=fk, gname=gname, edge=bool(edge),
             steps=tuple(float(s) for s in steps), lam=lam, dtype=dtype, lens=lens)
    p.update(make_state(shape, lens, seed, lam, dtype))
    return p


def kfac(p):
    return sum(2.0 / abs(s) for s in p['steps'])


def lipschitz(p):
    """The bound on |K| the tests hand to the solver: sqrt(sum_a 4 / step_a^2)."""
    return float(np.sqrt(sum(4.0 / s ** 2 for s in p['steps'])))


def step_sizes(p):
    """(tau, sigma, rho): the reference's rule for tau and sigma; rho = 0.9 given explicitly (F = 0 included),
    so the (1 - rho) terms see the non-zero x0 and z0 on every route."""
    beta = 0.0 if p['fk'] == 'null' else 1.0
    tau, sigma = OR.pds_step_sizes(beta, lipschitz(p))[:2]
    return float(tau), float(sigma), 0.9


def oracle_steps(p, nit, dtype=np.float64, l21_comps=3, first=None):
    """`nit` iterations of the oracle (OR.pds, accuracy_threshold 0) from (x0, z0) in `dtype` arithmetic, the
    construction of tests/cases.py::oracle_pds with per-axis taps, steps, edge, G and a non-zero start.
    `l21_comps`: components the L21 group norm is taken over (3; the sensitivity tests pass 2).  `first`: a
    dict that receives 'x' and 'z' after the first iteration (the nit = 1 result of the same run).
    Returns (x, z, diag, shares), shares measured at iteration 1 on the oracle's side: 'low' / 'high' the share
    of voxels prox_G clips at its lower / upper bound, 'dual' the share of dual entries (L21: voxels whose
    3-vector norm exceeds lam) the Fenchel prox projects."""
    from oracle import pylops1 as P
    shape, N = p['shape'], p['N']
    dt = np.dtype(dtype)
    y = p['y'].astype(dt)
    if p['fk'] == 'null':
        grad = lambda v: np.zeros_like(v)  # noqa: E731
    elif p['fk'] == 'denoise':
        grad = lambda v: (2 * (v + (-y))) * dt.type(0.5)  # noqa: E731
    else:
        Cs = [P.Convolve1D(N, p[n].astype(dt), offset=P.pycsou_offset(p[n].size), dims=shape, dir=a, dtype=dt)
              for a, n in enumerate(TAPS)]

        def grad(v):
            for C in Cs:
                v = C.matvec(v)
            v = (2 * (v + (-y))) * dt.type(0.5)
            for C in reversed(Cs):
                v = C.rmatvec(v)
            return v

    K = P.Gradient(shape, sampling=p['steps'], edge=p['edge'], kind=p['kind'], dtype=dt)
    lam = p['lam']

    def prox_l21(v, t):
        if l21_comps == 3:
            return OR.prox_l21_pixel(v, t, 3)
        w = v.reshape(3, -1)  # the mistake of a kernel that drops one component from the group norm
        n = np.sqrt(np.sum(w[:l21_comps] ** 2, axis=0))
        with np.errstate(divide='ignore'):
            fac = np.clip(1 - t / n, a_min=0, a_max=None)
        return (fac[None, :] * w).ravel()

    hprox = OR.postcomp(prox_l21 if p['hname'] == 'l21' else OR.prox_l1, lam)
    seg = p.get('seg', SEG)  # the sensitivity tests move a bound
    a, b = {'nonneg': (0.0, np.inf), 'segment': seg}.get(p['gname'], (-np.inf, np.inf))
    shares = {}

    def gprox(v, t):
        if 'low' not in shares:
            shares['low'], shares['high'] = float(np.mean(v < a)), float(np.mean(v > b))
        if p['gname'] == 'nonneg':
            return OR.proj_nonnegative_orthant(v)
        if p['gname'] == 'segment':
            return OR.proj_segment(v, *seg)
        return v

    def fen(w, s):
        if 'dual' not in shares:
            ws = np.abs(np.asarray(w, dtype=np.float64))
            if p['hname'] == 'l21':
                ws = np.sqrt(np.sum(ws.reshape(3, -1) ** 2, axis=0))
            shares['dual'] = float(np.mean(ws > lam))
        return OR.fenchel_prox(hprox, w, s)

    def grab(it, x, z):
        if it == 0 and first is not None:
            first['x'], first['z'] = x.copy(), z.copy()

    tau, sigma, rho = (dt.type(v) for v in step_sizes(p))
    x, z, d = OR.pds(grad, gprox, K.matvec, K.rmatvec, fen, tau, sigma, rho, p['x0'].astype(dt), p['z0'].astype(dt),
                     max_iter=nit - 1, min_iter=nit - 1, accuracy_threshold=0.0, callback=grab)
    return x, z, d, shares


def chain(p):
    """Roundings on the longest chain of one step."""
    return 2 * sum(p['lens']) + 16


def bound(p, nit=1, dtype=None):
    """{'x': Bound, 'z': Bound}: nit * c * eps(dtype) * M per variable (the module docstring derives it)."""
    eps = float(np.finfo(p['dtype'] if dtype is None else dtype).eps)
    tau, sigma, _ = step_sizes(p)
    ax0, ay, az0 = (float(np.max(np.abs(p[n]))) for n in ('x0', 'y', 'z0'))
    k = kfac(p)
    Mx = ax0 + tau * (ax0 + ay) + tau * az0 * k
    Mz = az0 + 3.0 * sigma * Mx * k
    c = chain(p)
    return {'x': Bound(nit * c * eps * Mx, eps * Mx, c), 'z': Bound(nit * c * eps * Mz, eps * Mz, c)}


# ---- the problem on the device ------------------------------------------------------------------------

def build_solver(p, nit, engine='fused'):
    """The PDS object of problem `p` for `nit` iterations from (x0, z0) in p['dtype']."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm, L21Norm, NonNegativeOrthant, Segment
    from pycsou_amd.linop.conv import Convolve1D
    from pycsou_amd.linop.diff import Gradient
    from pycsou_amd.opt.proxalgs import PDS
    shape, N, dtype = p['shape'], p['N'], p['dtype']
    tau, sigma, rho = step_sizes(p)
    F = None
    if p['fk'] != 'null':
        F = (1 / 2) * SquaredL2Loss(dim=N, data=p['y'].astype(dtype))
    if any(p['lens']):
        C = None
        for a, n in enumerate(TAPS):
            Ca = Convolve1D(N, p[n], reshape_dims=shape, axis=a)
            Ca.lipschitz_cst = Ca.diff_lipschitz_cst = 1.0
            C = Ca if C is None else Ca * C
        C.lipschitz_cst = C.diff_lipschitz_cst = 1.0
        F = F * C
    K = Gradient(shape, step=p['steps'], edge=p['edge'], kind=p['kind'])
    K.lipschitz_cst = K.diff_lipschitz_cst = lipschitz(p)
    H = p['lam'] * (L21Norm(dim=3 * N, groups=np.tile(np.arange(N), 3)) if p['hname'] == 'l21' else L1Norm(dim=3 * N))
    G = {'nonneg': NonNegativeOrthant(N), 'segment': Segment(N, *SEG)}.get(p['gname'], None)
    s = PDS(dim=N, F=F, G=G, H=H, K=K, rho=rho, engine=engine, x0=p['x0'].astype(dtype), z0=p['z0'].astype(dtype),
            max_iter=nit - 1, min_iter=nit - 1, accuracy_threshold=0.0, verbose=None)
    assert (s.tau, s.sigma, s.rho) == (tau, sigma, rho), ((s.tau, s.sigma, s.rho), (tau, sigma, rho))
    return s


def update_tile(kind, dtype):
    """(rows, columns) of the update kernel's tile (pds3d.hip: k3_rows / K3::TW for the forward kernel,
    k3g_rows / k3g_tw for k_pds3d_gen)."""
    f32 = np.dtype(dtype) == np.float32
    if kind == 'forward':
        return (8 if f32 else 12), 128
    return 12, (256 if f32 else 128)


# ---- the matrix (shared by the GPU tests and the CPU checks of its input conditions) ---------------------

VA = (20, 36, 260)    # several row tiles with a short last one, three 128-column tiles (4-column last), 3 segments
VB = (17, 9, 132)     # row tiles 8 + 1, 4-column last tile, plane segments 6 + 6 + 5
VS = (12, 33, 130)    # n2 % 4 = 2: scalar step, no ata kernel; fp32 plane bytes not a multiple of 16
VS32 = (12, 32, 130)  # fp32 plane bytes a multiple of 16: sep2 without ata, scalar step
VG32 = (20, 40, 520)  # fp32 k_pds3d_gen (12 x 256 tiles): row tile 1 x column tile 1 fully interior on planes 2..17
VG64 = (20, 40, 264)  # the same for fp64 (12 x 128 tiles)

# route -> (fkind name, ata, fold, fused0, sep2); the last two are None where the engine has no chain
ROUTES = {
    'fold': ('GRADBUF', True, True, True, True),
    'ata': ('GRADBUF', True, False, True, True),
    'sep2': ('GRADBUF', False, False, True, True),
    'conv1d': ('GRADBUF', False, False, True, False),
    'generic': ('GRADBUF', False, False, False, None),
    'denoise': ('DENOISE', False, False, None, None),
    'null': ('NULL', False, False, None, None),
}

Case = collections.namedtuple('Case', 'route shape kind fk g edge steps dtype env hs')


def _c(route, dtype, kind, fk, shape, g, steps=U1, edge=True, env=None):
    return Case(route, shape, kind, fk, g, edge, steps, dtype, env or {}, ('l1', 'l21'))


# g: the G kind of the (L1, L21) variant, alternating so that every kind meets both H on every route
CONFIGS = [
    # axis-0 pass folded into the forward update (in-plane normal operator, then k_pds3d<CONV0>)
    _c('fold', 'f32', 'forward', 'sep15x6x10', VA, ('nonneg', 'segment')),
    _c('fold', 'f32', 'forward', 'sep7x15x4', VB, ('segment', 'nonneg'), steps=NU),
    _c('fold', 'f32', 'forward', 'sep15x15x15', VB, ('', '')),
    # in-plane normal operator, separate axis-0 pass
    _c('ata', 'f32', 'forward', 'sep15x6x10', VA, ('segment', ''), steps=NU, env={'PCS_3D_FOLD': '0'}),
    _c('ata', 'f64', 'forward', 'sep6x10x15', VA, ('', 'nonneg'), steps=NU),
    _c('ata', 'f32', 'centered', 'sep15x6x10', VG32, ('nonneg', 'segment'), steps=NU),
    _c('ata', 'f32', 'backward', 'sep7x15x4', VG32, ('segment', '')),
    _c('ata', 'f32', 'centered', 'sep4x7x15', VA, ('', 'nonneg'), steps=NU, edge=False),
    _c('ata', 'f64', 'centered', 'sep15x6x10', VG64, ('nonneg', 'segment'), edge=False),
    _c('ata', 'f64', 'backward', 'sep7x15x4', VG64, ('segment', ''), steps=NU),
    # three-pass chain: both in-plane passes in one launch, no normal-operator kernel
    _c('sep2', 'f32', 'forward', 'sep15x6x10', VA, ('', 'nonneg'), env={'PCS_3D_ATA': '0'}),
    _c('sep2', 'f64', 'centered', 'sep7x15x4', VS, ('nonneg', 'segment'), steps=NU),
    _c('sep2', 'f32', 'forward', 'sep15x6x10', VS32, ('segment', ''), steps=NU),
    # separate pcs_conv1d in-plane passes around the fused axis-0 pass
    _c('conv1d', 'f32', 'backward', 'sep6x10x15', VS, ('', 'nonneg')),
    # generic chain: an axis-0 filter longer than the fused pass takes
    _c('generic', 'f32', 'forward', 'sep20x6x10', VB, ('nonneg', 'segment'), steps=NU),
    _c('generic', 'f64', 'centered', 'sep20x6x10', VB, ('segment', '')),
    # pointwise F
    _c('denoise', 'f32', 'forward', 'denoise', VA, ('', 'nonneg'), steps=NU),
    _c('null', 'f32', 'forward', 'null', VB, ('nonneg', 'segment')),
    _c('denoise', 'f64', 'forward', 'denoise', VS, ('segment', ''), steps=NU),
    _c('denoise', 'f32', 'centered', 'denoise', VG32, ('', 'nonneg'), steps=NU, edge=False),
    _c('null', 'f32', 'backward', 'null', VB, ('nonneg', 'segment'), steps=NU),
    _c('null', 'f64', 'centered', 'null', VG64, ('segment', ''), steps=NU),
    _c('denoise', 'f64', 'backward', 'denoise', VB, ('', 'nonneg')),
]

MATRIX = [(i, k) for i, c in enumerate(CONFIGS) for k in range(len(c.hs))]


def case_id(ik):
    c, k = CONFIGS[ik[0]], ik[1]
    return (f'{c.route}-{c.dtype}-{c.kind}-{c.fk}-{c.hs[k]}-{c.g[k] or "none"}-' + 'x'.join(str(n) for n in c.shape)
            + ('-nu' if c.steps == NU else '') + ('' if c.edge else '-noedge')
            + ''.join(f'-{n}={v}' for n, v in c.env.items()))


def case_problem(ik):
    """(Case, problem dict) of one entry of MATRIX."""
    c, k = CONFIGS[ik[0]], ik[1]
    p = make_problem(c.shape, c.kind, c.hs[k], c.fk, c.g[k], edge=c.edge, steps=c.steps, lam=LAM,
                     seed=10 * ik[0] + k, dtype=np.float32 if c.dtype == 'f32' else np.float64)
    return c, p
