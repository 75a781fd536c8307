"""Element-wise one-step parity of the fused 2-D PDS kernels: inputs, fp64 oracle, rounding bound, comparator.

The other GPU tests of the fused step start from x0 = z0 = 0, use Gaussian PSFs whose outer taps fall below
their tolerance, and compare a relative L2 norm over the image.  The helpers here build a step that hides
nothing: a generic state (x0, z0, y all non-zero, the prox_G bounds and the dual projection binding on a
fixed share of the elements), PSF taps of equal weight (every tap and every edge-table entry of
N = Conv^T Conv is about 1/len), and a comparison of every element against a bound that follows from the
arithmetic of one step.

The bound (`bound`).  One iteration is (pycsou/opt/proxalgs.py:343-355)

    x~ = prox_G(x - tau grad F(x) - tau K^T z)        grad F(x) = Conv^T (Conv x - y)  |  x - y  |  0
    z~ = prox_{sigma H*}(z + sigma K (2 x~ - x))
    x' = rho x~ + (1 - rho) x,   z' = rho z~ + (1 - rho) z.

With PSF taps that are non-negative and sum to 1, |Conv v| <= |v|_inf and |Conv^T v| <= |v|_inf, so
|grad F(x)| <= |x0|_inf + |y|_inf.  A first difference of step s is bounded by 2 |v|_inf / s and its adjoint
likewise, so |K^T z| <= |z0|_inf sum_a 2 / step_a for a Gradient (sum_a 4 |w_a| / step_a^2 for the
Laplacian, whose rows are w_a (1, -2, 1) / step_a^2; + 1 for the masked block's sampling rows).  Every
intermediate of the primal update is therefore at most

    Mx = |x0|_inf + tau (|x0|_inf + |y|_inf) + tau |z0|_inf kfac,      kfac = sum_a 2 / step_a (...)

in magnitude, and |2 x~ - x| <= 3 Mx makes every intermediate of the dual update at most

    Mz = |z0|_inf + sigma 3 Mx kfac      (+ sigma |y|_inf for the masked block, whose prox is shifted by y).

A floating-point operation on operands of magnitude <= M errs by at most eps M / 2 <= eps M, and to first
order the errors of a chain of c operations add: |error| <= c eps M.  c is the number of roundings on the
longest chain of one step: two 1-D passes of l0 and l1 multiply-adds for a separable PSF (2 (l0 + l1)),
q^2 multiply-adds for a q x q PSF (2 q^2), plus 16 for everything else (the stored-table and tap roundings,
tau / sigma scalings, the stencil's adds, the prox, the relaxation).  prox_G, the Fenchel prox of lam L1 /
lam L21 (projections onto convex sets) and the convex combination with rho are 1-Lipschitz, so they pass the
error on without amplifying it.  For `nit` iterations the bar is nit c eps M: every iteration adds its own
c eps M, and the error carried over enters the next step through I - tau N, tau K^T and sigma K, whose
max-norm gains are O(1) but not below 1 -- a first-order budget that is meant for the two or three iterations
run here, where the measured errors are below 2 % of it (tests/test_step_pointwise_cpu.py checks a plain
fp32 evaluation of two iterations against it).  The asserted bar is this derived c eps M and never a number
read off a kernel.

Inputs are rounded to the dtype under test before the fp64 oracle sees them, so input rounding is not
counted as kernel error.
"""

import collections
import ctypes

import numpy as np

from oracle import pycsou_ref as OR

Bound = collections.namedtuple('Bound', 'tol unit c')  # tol = nit * c * unit, unit = eps * M

SEG = (0.25, 0.75)  # the Segment under test: both bounds inside the range of x0
LAM = 0.5  # lam of every case of the matrix: z0 = lam N(0, 1) puts the dual projection at 24-60 % of the entries
P_COL = 'Relative Improvement (primal variable)'
D_COL = 'Relative Improvement (dual variable)'


def _round(a, dtype):
    return np.asarray(a, dtype=dtype).astype(np.float64)


def make_state(shape, l0, l1, seed, lam, q=0, hdim=None, dtype=np.float32):
    """fp64 arrays holding values of `dtype`: taps t0 (l0) and t1 (l1) from U(0.5, 1.5) normalised to sum 1
    (about 1 / len each, not symmetric, the axes differ), a q x q U(0.5, 1.5) PSF of sum 1 when q > 0,
    x0 and y from U(-0.5, 1.5), z0 = lam N(0, 1) with `hdim` entries (default 2 N)."""
    rng = np.random.default_rng(seed)
    N = int(shape[0]) * int(shape[1])
    st = {}
    for name, l in (('t0', l0), ('t1', l1)):
        t = rng.uniform(0.5, 1.5, max(int(l), 1))
        st[name] = _round(t / t.sum(), dtype) if l else None
    psfq = rng.uniform(0.5, 1.5, (max(q, 1), max(q, 1)))
    st['psfq'] = _round(psfq / psfq.sum(), dtype) if q else None
    st['x0'] = _round(rng.uniform(-0.5, 1.5, N), dtype)
    st['y'] = _round(rng.uniform(-0.5, 1.5, N), dtype)
    st['z0'] = _round(lam * rng.standard_normal(2 * N if hdim is None else int(hdim)), dtype)
    return st


def make_problem(shape, kind, hname, fk, gname, edge=True, steps=(1.0, 1.0), weights=(1.0, 1.0), lam=0.5, seed=0,
                 dtype=np.float32, mask_share=0.0):
    """One problem of the matrix.  kind: 'forward' | 'backward' | 'centered' | 'lap'; fk: 'null' | 'denoise' |
    'sepL' | 'sepL0xL1' (separable PSF) | 'convQ' (non-separable Q x Q); gname: '' | 'nonneg' | 'segment';
    mask_share > 0: the masked block (K = [Masking; Gradient], H = L1Loss(y_m) (+) lam H_s, F = 0)."""
    n0, n1 = shape
    N = n0 * n1
    l0 = l1 = q = 0
    if fk.startswith('sep'):
        l0, l1 = (int(v) for v in (fk[3:].split('x') * 2)[:2])
    elif fk.startswith('conv'):
        q = int(fk[4:])
    rng = np.random.default_rng(1000 + seed)
    mask = rng.random(N) < mask_share if mask_share > 0 else None
    m = int(mask.sum()) if mask is not None else 0
    ncomp = 1 if kind == 'lap' else 2
    st = make_state(shape, l0, l1, seed, lam, q=q, hdim=m + ncomp * N, dtype=dtype)
    psf = np.outer(st['t0'], st['t1']) if l0 else st['psfq']
    p = dict(shape=(n0, n1), N=N, kind=kind, hname=hname, fk=fk, gname=gname, edge=edge, steps=tuple(steps),
             weights=tuple(weights), lam=lam, psf=psf, t0=st['t0'], t1=st['t1'], x0=st['x0'], y=st['y'], z0=st['z0'],
             dtype=dtype, mask=mask, m=m, ncomp=ncomp, l0=l0, l1=l1, q=q)
    if mask is not None:
        p['ym'] = p['y'][mask].copy()
        z0 = p['z0']
        z0[:m] = _round(rng.standard_normal(m), dtype)  # the masked block projects onto |.| <= 1
    return p


def kfac(p):
    """sum_a 2 / step_a for a Gradient, sum_a 4 |w_a| / step_a^2 for the Laplacian, + 1 with sampling rows."""
    if p['kind'] == 'lap':
        k = sum(4.0 * abs(w) / s ** 2 for w, s in zip(p['weights'], p['steps']))
    else:
        k = sum(2.0 / abs(s) for s in p['steps'])
    return k + (1.0 if p.get('mask') is not None else 0.0)


def lipschitz(p):
    """The bound on |K| the tests hand to the solver (as tests/test_gpu_smarch.py)."""
    if p.get('mask') is not None:
        return float(np.sqrt(1.0 + 8.0))
    if p['kind'] == 'lap':
        return float(4.0 * sum(abs(w) / s ** 2 for w, s in zip(p['weights'], p['steps'])))
    return float(np.sqrt(sum(4.0 / s ** 2 for s in p['steps'])))


def step_sizes(p):
    """(tau, sigma, rho): the reference's rules; F = 0 (the ChambollePock masked problem included) runs with
    rho = 0.9 too, given explicitly, so the (1 - rho) terms see the non-zero x0 and z0 on every path."""
    beta = 0.0 if p['fk'] == 'null' else 1.0
    tau, sigma = OR.pds_step_sizes(beta, lipschitz(p))[:2]
    return float(tau), float(sigma), 0.9


def dense_conv1d(n, t):
    """The n x n matrix of the zero-boundary 'same' 1-D convolution with taps t at pycsou's offset:
    (C v)[i] = sum_j t[j] v[i + off - j]."""
    from oracle import pylops1 as P
    t = np.asarray(t, dtype=np.float64)
    off = P.pycsou_offset(t.size)
    C = np.zeros((n, n))
    for i in range(n):
        for j in range(t.size):
            k = i + off - j
            if 0 <= k < n:
                C[i, k] = t[j]
    return C


def oracle_steps(p, nit, dtype=np.float64, grad=None):
    """`nit` iterations of the oracle (OR.pds, accuracy_threshold 0) from (x0, z0), the construction of
    tests/test_gpu_smarch.py::_oracle with method='direct' convolutions, in `dtype` arithmetic.
    `grad`: another grad F (the sensitivity tests).  Returns (x, z, diag, shares), shares measured at
    iteration 1 on the oracle's side: 'low' / 'high' the share of pixels prox_G clips at its lower / upper
    bound, 'dual' the share of dual entries (L21: pixels) the Fenchel prox projects."""
    from oracle import pylops1 as P
    shape, N = p['shape'], p['N']
    dt = np.dtype(dtype)
    y = p['y'].astype(dt)
    if grad is None and p['fk'] == 'null':
        grad = lambda v: np.zeros_like(v)  # noqa: E731
    elif grad is None and p['fk'] == 'denoise':
        grad = lambda v: (2 * (v + (-y))) * dt.type(0.5)  # noqa: E731
    elif grad is None:
        psf = p['psf'].astype(dt)
        off = tuple(P.pycsou_offset(n) for n in psf.shape)
        C = P.Convolve2D(N, psf, shape, offset=off, method='direct', dtype=dt)
        grad = lambda v: C.rmatvec((2 * (C.matvec(v) + (-y))) * dt.type(0.5))  # noqa: E731
    if p['kind'] == 'lap':
        K = P.Laplacian(shape, weights=p['weights'], sampling=p['steps'], edge=p['edge'], dtype=dt)
    else:
        K = P.Gradient(shape, sampling=p['steps'], edge=p['edge'], kind=p['kind'], dtype=dt)
    lam = p['lam']
    if p['hname'] == 'l21':
        hs = OR.postcomp(lambda v, t: OR.prox_l21_pixel(v, t, 2), lam)
    else:
        hs = OR.postcomp(OR.prox_l1, lam)
    mask, m = p.get('mask'), p.get('m', 0)
    if mask is None:
        Kf, KT, hprox = K.matvec, K.rmatvec, hs
    else:  # tests/cases.py::oracle_cps_inpaint on in-memory inputs
        ym = p['ym'].astype(dt)

        def Kf(x):
            return np.concatenate([x[mask], K.matvec(x)])

        def KT(z):
            xa = np.zeros(N, dtype=dt)
            xa[mask] = z[:m]
            return 0 + xa + K.rmatvec(z[m:])

        def hprox(v, t):
            return np.concatenate([OR.prox_l1(v[:m] + (-ym), t) - (-ym), hs(v[m:], t)])

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
            ws = np.asarray(w[m:], dtype=np.float64)
            if p['hname'] == 'l21':
                ws = np.sqrt(np.sum(ws.reshape(2, -1) ** 2, axis=0))
            n_proj, n_all = np.sum(np.abs(ws) > lam), ws.size
            if mask is not None:  # L1Loss block: prox_{sigma (|. - y|)*} projects onto |.| <= 1
                wm = np.asarray(w[:m], dtype=np.float64) - s * p['ym']
                n_proj, n_all = n_proj + np.sum(np.abs(wm) > 1.0), n_all + m
            shares['dual'] = float(n_proj) / n_all
        return OR.fenchel_prox(hprox, w, s)

    tau, sigma, rho = (dt.type(v) for v in step_sizes(p))
    x, z, d = OR.pds(grad, gprox, Kf, KT, fen, tau, sigma, rho, p['x0'].astype(dt), p['z0'].astype(dt),
                     max_iter=nit - 1, min_iter=nit - 1, accuracy_threshold=0.0)
    return x, z, d, shares


def chain(p):
    """Roundings on the longest chain of one step."""
    if p['l0']:
        return 2 * (p['l0'] + p['l1']) + 16
    if p['q']:
        return 2 * p['q'] ** 2 + 16
    return 16


def bound(p, nit=1, dtype=None):
    """{'x': Bound, 'z': Bound}: nit * c * eps(dtype) * M per variable (the module docstring derives it)."""
    eps = float(np.finfo(p['dtype'] if dtype is None else dtype).eps)
    tau, sigma, _ = step_sizes(p)
    ax0, ay, az0 = (float(np.max(np.abs(p[n]))) for n in ('x0', 'y', 'z0'))
    k = kfac(p)
    Mx = ax0 + tau * (ax0 + ay) + tau * az0 * k
    Mz = az0 + sigma * 3.0 * Mx * k + (sigma * ay if p.get('mask') is not None else 0.0)
    c = chain(p)
    return {'x': Bound(nit * c * eps * Mx, eps * Mx, c), 'z': Bound(nit * c * eps * Mz, eps * Mz, c)}


def compare(got, ref, bound, shape, name='x', diag=None, diag_ref=None, dtype=None):
    """Assert max |got - ref| <= bound.tol element-wise; on failure name the worst element: (row, col), or (plane, row, col) when `shape` has three entries, for
    a dual variable its component, the error in units of eps * M, the column modulo 64.  With `diag`
    (the solver's diagnostics frame) and `diag_ref` (the oracle's): every row, the first included, is finite
    and within 1e-3 (fp32) / 1e-9 (fp64) relative.  Returns the worst error in units of eps * M."""
    got = np.asarray(got, dtype=np.float64).ravel()
    ref = np.asarray(ref, dtype=np.float64).ravel()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f'{name}: non-finite values'
    tol, unit = (bound.tol, bound.unit) if isinstance(bound, Bound) else (float(bound), float(bound))
    err = np.abs(got - ref)
    i = int(np.argmax(err))
    worst = float(err[i])
    if worst > tol:
        n1 = int(shape[-1])  # (rows, cols), or (planes, rows, cols) for a volume
        comp, pix = divmod(i, int(np.prod(shape)))
        row, col = divmod(pix, n1)
        where = f'row {row}, col {col}'
        if len(shape) == 3:
            plane, row = divmod(row, int(shape[1]))
            where = f'plane {plane}, row {row}, col {col}'
        raise AssertionError(
            f'{name}: |got - ref| = {worst:.3e} > {tol:.3e} at ({where}), component {comp}: '
            f'{worst / unit:.1f} eps*M (bound {tol / unit:.0f}), col % 64 = {col % 64}, got {got[i]!r}, ref {ref[i]!r}; '
            f'{int(np.sum(err > tol))} elements over the bound')
    if diag is not None:
        rtol = 1e-3 if np.dtype(dtype) == np.float32 else 1e-9
        for col, key in ((P_COL, 'primal'), (D_COL, 'dual')):
            d = diag[col].to_numpy(float) if hasattr(diag, 'columns') else np.asarray(diag[key], dtype=float)
            r = np.asarray(diag_ref[key], dtype=float)
            assert d.shape == r.shape, (col, d.shape, r.shape)
            assert np.isfinite(d).all() and np.isfinite(r).all(), (col, d, r)
            np.testing.assert_allclose(d, r, rtol=rtol, err_msg=col)
    return worst / unit


# ---- the problem on the device ------------------------------------------------------------------------

def build_solver(p, nit, engine):
    """The PDS / CPS object of problem `p` for `nit` iterations from (x0, z0) in p['dtype']."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm, L21Norm, NonNegativeOrthant, Segment
    from pycsou_amd.linop.conv import Convolve2D
    from pycsou_amd.linop.diff import Gradient, Laplacian
    from pycsou_amd.opt.proxalgs import CPS, PDS
    shape, N, dtype = p['shape'], p['N'], p['dtype']
    tau, sigma, rho = step_sizes(p)
    F = None
    if p['fk'] != 'null':
        F = (1 / 2) * SquaredL2Loss(dim=N, data=p['y'].astype(dtype))
    if p['psf'] is not None:
        C = Convolve2D(N, p['psf'], shape)
        C.lipschitz_cst = C.diff_lipschitz_cst = 1.0
        F = F * C
    if p['kind'] == 'lap':
        K = Laplacian(shape, weights=p['weights'], step=p['steps'], edge=p['edge'])
    else:
        K = Gradient(shape, step=p['steps'], edge=p['edge'], kind=p['kind'])
    nc = p['ncomp']
    H = p['lam'] * (L21Norm(dim=nc * N, groups=np.tile(np.arange(N), 2)) if p['hname'] == 'l21' else L1Norm(dim=nc * N))
    G = {'nonneg': NonNegativeOrthant(N), 'segment': Segment(N, *SEG)}.get(p['gname'], None)
    kw = dict(x0=p['x0'].astype(dtype), z0=p['z0'].astype(dtype), max_iter=nit - 1, min_iter=nit - 1,
              accuracy_threshold=0.0, verbose=None)
    if p.get('mask') is not None:
        from pycsou_amd.func import L1Loss, ProxFuncHStack
        from pycsou_amd.linop import LinOpVStack, Masking
        Kk = LinOpVStack(Masking(size=N, sampling_bool=p['mask']), K)
        Kk.lipschitz_cst = Kk.diff_lipschitz_cst = lipschitz(p)
        Hh = ProxFuncHStack(L1Loss(dim=p['m'], data=p['ym'].astype(dtype)), H)
        s = CPS(dim=N, G=G, H=Hh, K=Kk, rho=rho, **kw)
    else:
        K.lipschitz_cst = K.diff_lipschitz_cst = lipschitz(p)
        s = PDS(dim=N, F=F, G=G, H=H, K=K, rho=rho, engine=engine, **kw)
    assert (s.tau, s.sigma, s.rho) == (tau, sigma, rho), ((s.tau, s.sigma, s.rho), (tau, sigma, rho))
    return s


def engine_path(eng):
    """The kernel path of a built engine: pcs_pds2d_path on its arguments, or 'stencil_tile' for the
    general-stencil tile kernel (pcs_pds2d_stencil_step, which has no path query)."""
    from pycsou_amd import _lib as L
    if isinstance(eng.args, L.StencilArgs):
        assert not eng.march
        return 'stencil_tile'
    return int(eng.lib.pcs_pds2d_path(ctypes.byref(eng.args)))


# ---- the matrix (shared by the GPU tests and the CPU checks of its input conditions) ---------------------

A = (150, 200)  # three full 64-column strips + 8 columns, several row segments with a short last one
B = (70, 132)   # 4-column last strip
C = (250, 132)  # fp64 general-stencil march: two row segments of 8 16-row steps, the last one short and ragged
T = (67, 101)   # odd sizes: no vector path, the tile kernels
U1, NU = (1.0, 1.0), (2.0, 0.5)

Case = collections.namedtuple('Case', 'row shape kind fk g edge steps weights dtype engine env path hs')


def _c(row, shape, kind, fk, g, path, edge=True, steps=U1, weights=U1, dtype='f32', engine='stencil', env=None,
       hs=('l1', 'l21')):
    return Case(row, shape, kind, fk, g, edge, steps, weights, dtype, engine, env or {}, path, hs)


# g: the G kind of the (L1, L21) variant, so every kind meets both H on every row
CONFIGS = [
    # fused normal-operator march, forward K: G = none is the copy compiled for it (PCS_NM_GKSPLIT)
    _c('nmarch', A, 'forward', 'sep15', ('', ''), 'NMARCH', engine='fused'),
    _c('nmarch', A, 'forward', 'sep7', ('nonneg', 'segment'), 'NMARCH', engine='fused'),
    _c('nmarch', B, 'forward', 'sep6x10', ('segment', 'nonneg'), 'NMARCH', engine='fused'),
    _c('nmarch', B, 'forward', 'sep15', ('nonneg', 'segment'), 'NMARCH', engine='fused', steps=NU),
    _c('nmarch', B, 'forward', 'sep7', ('', ''), 'NMARCH', engine='fused'),
    # backward / centred K: the GEN geometry (last strip wider than the tier)
    _c('nmarch_gen', A, 'backward', 'sep15', ('segment', ''), 'NMARCH'),
    _c('nmarch_gen', A, 'centered', 'sep15', ('', 'nonneg'), 'NMARCH', edge=False),
    _c('nmarch_gen', A, 'centered', 'sep7', ('nonneg', 'segment'), 'NMARCH', steps=NU),
    _c('nmarch_gen', A, 'backward', 'sep6x10', ('', 'segment'), 'NMARCH', edge=False),
    # the same K where the last strip is narrower than the tier: N x into the buffer, then the stencil march
    _c('smarch_nx', B, 'backward', 'sep15', ('segment', ''), 'SMARCH_NX'),
    _c('smarch_nx', B, 'centered', 'sep9', ('', 'nonneg'), 'SMARCH_NX', edge=False),
    _c('smarch_nx', A, 'centered', 'sep7', ('nonneg', 'segment'), 'SMARCH_NX', env={'PCS_NMARCH_GEN': '0'}),
    # four-pass march
    _c('march', A, 'forward', 'sep15', ('', 'segment'), 'MARCH', engine='fused', env={'PCS_NMARCH': '0'}),
    _c('march', B, 'forward', 'sep7', ('nonneg', ''), 'MARCH', engine='fused', env={'PCS_NMARCH': '0'}),
    # pointwise-F march
    _c('pt', A, 'forward', 'denoise', ('segment', ''), 'PT', engine='fused', steps=NU),
    _c('pt', B, 'forward', 'denoise', ('', 'nonneg'), 'PT', engine='fused', steps=NU),
    # general-stencil march, fp32
    _c('smarch', A, 'backward', 'denoise', ('', 'segment'), 'SMARCH'),
    _c('smarch', B, 'centered', 'denoise', ('nonneg', ''), 'SMARCH', edge=False),
    _c('smarch', A, 'centered', 'null', ('segment', 'nonneg'), 'SMARCH', steps=NU),
    _c('smarch', B, 'backward', 'null', ('', 'segment'), 'SMARCH', edge=False),
    _c('smarch', A, 'lap', 'denoise', ('segment',), 'SMARCH', steps=(0.7, 1.3), weights=(2.0, 0.5), hs=('l1',)),
    _c('smarch', B, 'lap', 'null', ('nonneg',), 'SMARCH', edge=False, steps=(0.7, 1.3), weights=(2.0, 0.5), hs=('l1',)),
    _c('smarch', A, 'forward', 'denoise', ('nonneg', 'segment'), 'SMARCH', env={'PCS_SM_FWD': '1'}),
    _c('smarch', B, 'forward', 'null', ('segment', ''), 'SMARCH', env={'PCS_SM_FWD': '1'}),
    # general-stencil march, fp64
    _c('smarch', C, 'centered', 'denoise', ('segment', ''), 'SMARCH', dtype='f64'),
    _c('smarch', C, 'backward', 'null', ('', 'nonneg'), 'SMARCH', dtype='f64', edge=False),
    _c('smarch', C, 'forward', 'denoise', ('nonneg', 'segment'), 'SMARCH', dtype='f64'),
    _c('smarch', C, 'lap', 'denoise', ('segment',), 'SMARCH', dtype='f64', steps=(0.7, 1.3), weights=(2.0, 0.5),
       hs=('l1',)),
    _c('smarch', C, 'lap', 'null', ('',), 'SMARCH', dtype='f64', edge=False, hs=('l1',)),
    # fused fp64 normal-operator march and its split form
    _c('nm64', A, 'forward', 'sep15', ('', 'segment'), 'NM64', dtype='f64'),
    _c('nm64', A, 'backward', 'sep7', ('nonneg', ''), 'NM64', dtype='f64', edge=False),
    _c('nm64', A, 'centered', 'sep6x10', ('segment', 'nonneg'), 'NM64', dtype='f64'),
    _c('nm64_split', A, 'centered', 'sep15', ('', 'segment'), 'SMARCH_NX', dtype='f64', env={'PCS_NM64': '0'}),
    _c('nm64_split', A, 'forward', 'sep7', ('nonneg', ''), 'SMARCH_NX', dtype='f64', env={'PCS_NM64': '0'}),
    # non-separable 5 x 5 PSF: two correlation passes into the gradient buffer, then the step
    _c('gradbuf', A, 'forward', 'conv5', ('', 'segment'), 'PT', engine='fused'),
    _c('gradbuf', A, 'centered', 'conv5', ('nonneg', ''), 'SMARCH'),
    _c('gradbuf', A, 'forward', 'conv5', ('segment', 'nonneg'), 'SMARCH', dtype='f64'),
    _c('gradbuf', A, 'centered', 'conv5', ('', 'segment'), 'SMARCH', dtype='f64', edge=False),
    # tile kernels: odd sizes, and the stencil engine with its march switched off
    _c('tile', T, 'forward', 'sep15', ('segment', ''), 'TILE', engine='fused'),
    _c('tile', T, 'forward', 'denoise', ('', 'nonneg'), 'TILE', engine='fused', steps=NU),
    _c('tile', T, 'forward', 'sep7', ('nonneg', 'segment'), 'TILE', dtype='f64', engine='fused'),
    _c('tile', T, 'forward', 'conv5', ('', 'segment'), 'TILE', dtype='f64', engine='fused'),
    _c('tile', T, 'centered', 'denoise', ('segment', ''), 'stencil_tile'),
    _c('tile', T, 'lap', 'null', ('nonneg',), 'stencil_tile', steps=(0.7, 1.3), weights=(2.0, 0.5), hs=('l1',)),
    _c('tile', T, 'backward', 'conv5', ('', 'segment'), 'stencil_tile', dtype='f64', edge=False),
    _c('tile', A, 'centered', 'denoise', ('nonneg', 'segment'), 'stencil_tile', env={'PCS_STENCIL_MARCH': '0'}),
    _c('tile', A, 'backward', 'null', ('segment', ''), 'stencil_tile', dtype='f64', env={'PCS_STENCIL_MARCH': '0'}),
    # masked block inside the general-stencil march (CPS TV-LAD inpainting, 50 % mask)
    _c('masked', B, 'forward', 'null', ('segment', 'segment'), 'SMARCH', engine='auto'),
    _c('masked', A, 'centered', 'null', ('segment', 'nonneg'), 'SMARCH', engine='auto'),
]

MATRIX = [(i, k) for i, c in enumerate(CONFIGS) for k in range(len(c.hs))]


def case_id(ik):
    c, k = CONFIGS[ik[0]], ik[1]
    return (f'{c.row}-{c.dtype}-{c.kind}-{c.fk}-{c.hs[k]}-{c.g[k] or "none"}-{c.shape[0]}x{c.shape[1]}'
            + ('' if c.edge else '-noedge') + ''.join(f'-{n}={v}' for n, v in c.env.items()))


def case_problem(ik):
    """(Case, problem dict) of one entry of MATRIX."""
    c, k = CONFIGS[ik[0]], ik[1]
    p = make_problem(c.shape, c.kind, c.hs[k], c.fk, c.g[k], edge=c.edge, steps=c.steps, weights=c.weights,
                     lam=LAM, seed=10 * ik[0] + k, dtype=np.float32 if c.dtype == 'f32' else np.float64,
                     mask_share=0.5 if c.row == 'masked' else 0.0)
    return c, p

