"""Element-wise one-launch parity of the fused APGD kernel (pcs_apgd2d_step / pcs_apgd2d_run, the NrmApgd
output policy of csrc/sep_nrm.hpp): inputs, fp64 oracle, rounding bound, matrix.  The companion of
tests/pointwise.py, whose state generator, dense 1-D operator, `Bound` and comparator it reuses.

The older tests of this kernel (tests/test_gpu_apgd2d.py) start from x0 = 0 with past_aux = 0, run 'CD' with
d = 75 (a = 0, 0, 1/77, ...), use a sigma = 2 Gaussian PSF on a phantom in [0, 1] and compare a relative L2
norm.  Here one launch starts from a generic state: x, aux and y are independent draws from U(-0.5, 1.5), the
taps are U(0.5, 1.5) normalised (about 1 / len each, not symmetric, the axes differ), tau = 1, lam = 0.5,
Segment(0.25, 0.75), and the momentum coefficient is given explicitly (0.61, then -0.35), so N x, the edge
tables, aux, `a` and both outcomes of every prox act at full weight on every element, and every element is
compared.

The update (pycsou/opt/proxalgs.py:586-601), for explicit (x, aux, a):

    w    = prox_G(x - tau Conv^T (Conv x - y))
    x'   = w + a (w - aux)
    aux' = w
    metric = ||x - x'|| / ||x||.

The bound (`bound`).  With PSF taps that are non-negative and sum to 1, |Conv v| <= |v|_inf and
|Conv^T v| <= |v|_inf, so |grad F(x)| <= |x|_inf + |y|_inf and every intermediate of w is at most

    Mw = |x|_inf + tau (|x|_inf + |y|_inf)

in magnitude; every intermediate of x' is at most

    M = Mw + |a| (Mw + |aux|_inf).

A floating-point operation on operands of magnitude <= M errs by at most eps M / 2 <= eps M and to first
order the errors of a chain of c operations add.  c = 2 (l0 + l1) + 16 as pointwise.chain: two 1-D passes of
l0 and l1 multiply-adds for Conv and as many for Conv^T (the kernel's two passes with the 2 l - 1
autocorrelation taps of N = Conv^T Conv are no longer), plus 16 for everything else: the tap and table
roundings, Conv^T y rounded to the dtype, the subtraction, tau, the prox, and the three operations of the
momentum step.  prox_G (the identity, soft thresholding, two projections) is 1-Lipschitz.  For `nit` launches
the bar is nit c eps M for x' and nit c eps Mw for aux', with M and Mw the largest over the launches, each
evaluated on the state that launch starts from (the oracle's).  As in tests/pointwise.py it is a first-order
budget meant for the two or three launches run here: the carried error enters the next launch through
I - tau N and 1 + |a|, whose max-norm gains are O(1).  The asserted bar is this derived one, never a number
read off a kernel; tests/test_apgd_pointwise_cpu.py checks a plain fp32 evaluation against it.

Inputs are rounded to the dtype under test before the fp64 oracle sees them.
"""

import collections
import functools

import numpy as np

from oracle import pycsou_ref as OR
from oracle import pylops1 as P
from tests import pointwise as PW
from tests.pointwise import SEG, Bound

LAM = 0.5
A0, A1 = 0.61, -0.35  # the coefficients of the explicit launches: different signs and magnitudes
H_COL = 'Relative Improvement'

PSFS = {'sep15': (15, 15), 'sep7': (7, 7), 'sep6x10': (6, 10), 'sep5x9': (5, 9), 'sep1x5': (1, 5)}


def psf_half(fk):
    """The common half width the engine pads both axes to (Convolve2DOp.separable) at pycsou's offsets."""
    return max(max(P.pycsou_offset(k), k - 1 - P.pycsou_offset(k)) for k in PSFS[fk])


# shape -> ((strips, row segments) in fp32, the same in fp64): 128- / 64-column strips, max(1, n0 // 64)
# segments of ceil(n0 / nseg) rows
GEOM = {
    (16, 16): ((1, 1), (1, 1)),     # the minimum: both 7-wide edge bands overlap the whole image, both ways
    (21, 36): ((1, 1), (1, 1)),     # fewer rows than the 28-row prologue, rows no multiple of 4, a partial strip
    (70, 132): ((2, 1), (3, 1)),    # two full steps + 6 rows; a 4-column last strip (fp32), 64 + 64 + 4 (fp64)
    (150, 200): ((2, 2), (4, 2)),   # two segments of 75 rows (seam off the 4-row blocks); 128 + 72, 64 * 3 + 8
    (128, 256): ((2, 2), (4, 2)),   # nothing ragged: seam at row 64, every strip full
    (193, 68): ((1, 3), (2, 3)),    # three segments of 65 / 65 / 63 rows; a 4-column last strip in fp64
}


def make_problem(shape, fk, gname, seed=0, dtype=np.float32, tau=1.0, lam=LAM):
    """One problem: taps, x (the iterate), y from pointwise.make_state; aux an independent U(-0.5, 1.5) draw.
    gname: '' | 'l1' | 'nonneg' | 'segment'; tau = 1 / lipschitz^2 is what build_solver makes the solver use."""
    n0, n1 = shape
    l0, l1 = PSFS[fk]
    st = PW.make_state(shape, l0, l1, seed, lam, hdim=1, dtype=dtype)
    aux = PW._round(np.random.default_rng(5000 + seed).uniform(-0.5, 1.5, n0 * n1), dtype)
    return dict(shape=(n0, n1), N=n0 * n1, fk=fk, gname=gname, dtype=dtype, tau=float(tau), lam=float(lam), seg=SEG,
                t0=st['t0'], t1=st['t1'], psf=np.outer(st['t0'], st['t1']), l0=l0, l1=l1, q=0, x=st['x0'],
                aux=aux, y=st['y'], half=psf_half(fk))


def conv_grad(p, dtype=np.float64):
    """grad F = Conv^T (Conv x - y) on pylops1.Convolve2D(method='direct') in `dtype`, as pointwise.oracle_steps."""
    dt = np.dtype(dtype)
    psf, y = p['psf'].astype(dt), p['y'].astype(dt)
    off = tuple(P.pycsou_offset(n) for n in psf.shape)
    C = P.Convolve2D(p['N'], psf, p['shape'], offset=off, method='direct', dtype=dt)
    return lambda v: C.rmatvec((2 * (C.matvec(v) + (-y))) * dt.type(0.5))


def dense_grad(p, interior_row=None, interior_col=None):
    """The same grad F from the dense 1-D matrices: Conv X = C0 X C1^T, N X = (C0^T C0) X (C1^T C1).
    `interior_row` / `interior_col`: that output row / column of N takes the interior window (no edge-table
    correction), the mistake of a kernel that mis-indexes its E table."""
    n0, n1 = p['shape']
    C0, C1 = PW.dense_conv1d(n0, p['t0']), PW.dense_conv1d(n1, p['t1'])
    N0, N1 = C0.T @ C0, C1.T @ C1

    def interior(n, t, j):
        pad = 2 * len(t)
        Cb = PW.dense_conv1d(n + 2 * pad, t)
        return (Cb.T @ Cb)[j + pad, pad:pad + n]

    if interior_row is not None:
        N0 = N0.copy()
        N0[interior_row] = interior(n0, p['t0'], interior_row)
    if interior_col is not None:
        N1 = N1.copy()
        N1[:, interior_col] = interior(n1, p['t1'], interior_col)
    cty = C0.T @ p['y'].reshape(n0, n1) @ C1
    return lambda v: (N0 @ v.reshape(n0, n1) @ N1 - cty).ravel()


def prox_g(p, dtype=np.float64):
    """G.prox(v, tau) of the problem, the reference's expressions (they mutate a fresh array only)."""
    g = p['gname']
    if g == 'l1':
        return OR.postcomp(OR.prox_l1, np.dtype(dtype).type(p['lam']))
    if g == 'nonneg':
        return lambda v, t: OR.proj_nonnegative_orthant(v)
    if g == 'segment':
        return lambda v, t: OR.proj_segment(v, *p['seg'])
    return lambda v, t: v


Update = collections.namedtuple('Update', 'x aux w metric v')  # v: the prox's argument x - tau grad F(x)


def oracle_update(p, x, aux, a, dtype=np.float64, grad=None):
    """One update from the explicit state (x, aux) with coefficient a, in `dtype` arithmetic."""
    dt = np.dtype(dtype)
    grad = conv_grad(p, dt) if grad is None else grad
    x, aux = np.asarray(x, dtype=dt), np.asarray(aux, dtype=dt)
    tau = dt.type(p['tau'])
    v = x - tau * grad(x)
    w = prox_g(p, dt)(v.copy(), tau)
    xn = w + dt.type(a) * (w - aux)
    return Update(xn, w, w, OR._rel(x, xn), v)


def oracle_run(p, coeffs, dtype=np.float64, grad=None):
    """The updates of `coeffs` one after the other from (p['x'], p['aux']): a list of Update."""
    dt = np.dtype(dtype)
    grad = conv_grad(p, dt) if grad is None else grad
    x, aux, out = p['x'], p['aux'], []
    for a in coeffs:
        u = oracle_update(p, x, aux, a, dt, grad)
        out.append(u)
        x, aux = u.x, u.aux
    return out


def oracle_api(p, acc, d, nit, dtype=np.float64):
    """oracle.pycsou_ref.apgd from x0 = p['x'] (past_aux = 0, as the solver starts) for `nit` iterations:
    (x, past_aux, past_t, hist)."""
    dt = np.dtype(dtype)
    x, it, diag = OR.apgd(conv_grad(p, dt), prox_g(p, dt), dt.type(p['tau']), p['x'].astype(dt), acceleration=acc,
                          d=d, max_iter=nit - 1, min_iter=nit - 1, accuracy_threshold=0.0)
    assert diag['n_iter'] == nit
    return np.asarray(it['iterand']), np.asarray(it['past_aux']), it['past_t'], np.asarray(diag['hist'], dtype=float)


def chain(p):
    return PW.chain(p)


def magnitudes(p, x, aux, a):
    """(M, Mw) of one update from the state (x, aux) with coefficient a (the module docstring)."""
    ax, aaux, ay = (float(np.max(np.abs(v))) for v in (x, aux, p['y']))
    Mw = ax + p['tau'] * (ax + ay)
    return Mw + abs(float(a)) * (Mw + aaux), Mw


def bound(p, states, dtype=None):
    """{'x': Bound, 'aux': Bound} of the launches `states` = [(x, aux, a), ...] (each launch's own start, on the
    oracle's side): nit * c * eps * M for x', nit * c * eps * Mw for aux', M and Mw the largest of the launches."""
    eps = float(np.finfo(p['dtype'] if dtype is None else dtype).eps)
    ms = [magnitudes(p, *s) for s in states]
    M, Mw = max(m[0] for m in ms), max(m[1] for m in ms)
    c, nit = chain(p), len(states)
    return {'x': Bound(nit * c * eps * M, eps * M, c), 'aux': Bound(nit * c * eps * Mw, eps * Mw, c)}


def run_states(p, coeffs, ups):
    """The (x, aux, a) each launch of oracle_run(p, coeffs) started from."""
    xs = [p['x']] + [u.x for u in ups[:-1]]
    auxs = [p['aux']] + [u.aux for u in ups[:-1]]
    return list(zip(xs, auxs, coeffs))


def compare(got, ref, bnd, shape, name='x', hist=None, hist_ref=None, dtype=None):
    """pointwise.compare; `hist` / `hist_ref`: the history rows, every one finite and within its 1e-3 (fp32) /
    1e-9 (fp64) relative bar (APGD has the one column, handed over as both of the comparator's)."""
    if hist is None:
        return PW.compare(got, ref, bnd, shape, name)
    h, r = np.asarray(hist, dtype=float), np.asarray(hist_ref, dtype=float)
    return PW.compare(got, ref, bnd, shape, name, diag={'primal': h, 'dual': h}, diag_ref={'primal': r, 'dual': r},
                      dtype=dtype)


def ref_coeffs(acc, d, n):
    """(coefficients a of iterations 0 .. n - 1, past_t): pycsou/opt/proxalgs.py:592-598."""
    out, t_old = [], 1
    for it in range(n):
        if acc == 'BT':
            t = (1 + np.sqrt(1 + 4 * t_old ** 2)) / 2
        elif acc == 'CD':
            t = (it + d) / d
        else:
            t = t_old = 1
        out.append((t_old - 1) / t)
        t_old = t
    return out, t_old


# ---- the problem on the device ------------------------------------------------------------------------

def build_solver(p, nit, acc='CD', d=75., engine=None):
    """The APGD object of problem `p` for `nit` iterations from x0 = p['x'] in p['dtype']; tau = 1 / beta comes
    out of the Lipschitz constant handed to the blur."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm, NonNegativeOrthant, Segment
    from pycsou_amd.linop.conv import Convolve2D
    from pycsou_amd.opt.proxalgs import APGD
    shape, N, dtype = p['shape'], p['N'], p['dtype']
    C = Convolve2D(N, p['psf'], shape)
    C.lipschitz_cst = C.diff_lipschitz_cst = float(1.0 / np.sqrt(p['tau']))
    F = (1 / 2) * SquaredL2Loss(dim=N, data=p['y'].astype(dtype)) * C
    G = {'l1': lambda: p['lam'] * L1Norm(dim=N), 'nonneg': lambda: NonNegativeOrthant(N),
         'segment': lambda: Segment(N, *p['seg'])}.get(p['gname'], lambda: None)()
    s = APGD(dim=N, F=F, G=G, acceleration=acc, d=d, x0=p['x'].astype(dtype), max_iter=nit - 1, min_iter=nit - 1,
             accuracy_threshold=0.0, verbose=None, engine=engine)
    assert s.tau == p['tau'], (s.tau, p['tau'])
    return s


# ---- the matrix (shared by the GPU tests and the CPU checks of its input conditions) ---------------------

Case = collections.namedtuple('Case', 'shape fk g dtype tau')

_SHAPE_PSF = [((16, 16), 'sep15'), ((21, 36), 'sep6x10'), ((70, 132), 'sep7'), ((150, 200), 'sep15'),
              ((128, 256), 'sep5x9'), ((193, 68), 'sep1x5')]
# two G kinds per shape, each kind on three shapes; fp64 takes the next shape's pair, so a shape meets up to
# four kinds over the two types
_PAIRS = [('', 'l1'), ('nonneg', 'segment'), ('', 'nonneg'), ('l1', 'segment'), ('', 'segment'), ('l1', 'nonneg')]

CASES = []
for _i, (_shape, _fk) in enumerate(_SHAPE_PSF):
    for _dt, _shift in (('f32', 0), ('f64', 1)):
        for _g in _PAIRS[(_i + _shift) % 6]:
            CASES.append(Case(_shape, _fk, _g, _dt, 1.0))
CASES += [
    # the other PSFs at the shapes with segment and strip seams, and the even-length one on the minimum
    Case((150, 200), 'sep6x10', 'l1', 'f32', 1.0),
    Case((150, 200), 'sep7', 'segment', 'f64', 1.0),
    Case((193, 68), 'sep5x9', 'nonneg', 'f64', 1.0),
    Case((16, 16), 'sep6x10', 'segment', 'f32', 1.0),
    Case((70, 132), 'sep1x5', '', 'f64', 1.0),
    # tau != 1 (lipschitz 2, tau = 1 / 4): the L1 threshold is tau lam, not lam
    Case((150, 200), 'sep15', 'l1', 'f32', 0.25),
    Case((70, 132), 'sep7', 'l1', 'f64', 0.25),
]
MATRIX = list(range(len(CASES)))


def case_id(i):
    c = CASES[i]
    return (f'{c.dtype}-{c.fk}-{c.g or "none"}-{c.shape[0]}x{c.shape[1]}' + ('' if c.tau == 1.0 else f'-tau{c.tau}'))


def np_dtype(c):
    return np.float32 if c.dtype == 'f32' else np.float64


def case_problem(i):
    """(Case, problem dict) of one entry of MATRIX."""
    c = CASES[i]
    return c, make_problem(c.shape, c.fk, c.g, seed=100 + i, dtype=np_dtype(c), tau=c.tau)


def _frozen(ups):
    for u in ups:
        for a in (u.x, u.aux, u.v):
            a.setflags(write=False)
    return ups


@functools.lru_cache(maxsize=None)
def case_oracle(i):
    """The two explicit launches (A0, then A1) of case i on the oracle's side, computed once, read-only."""
    _, p = case_problem(i)
    return _frozen(oracle_run(p, [A0, A1]))


def geometry(c):
    """(strips, row segments) of the case's launch."""
    return GEOM[c.shape][0 if c.dtype == 'f32' else 1]
