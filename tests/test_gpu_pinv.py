"""GPU tier of the pseudo-inverse: the four CG entry points one launch at a time on exact data (array_equal), the
solver against the derived bound of tests/pinv_cases.py and against SciPy's loop, and the algebra built on it.

One launch per kernel.  Data of tests/pinv_cases.exact_vectors (every sum exact, shown on the host by
tests/test_pinv_host.py), operands once 16-byte aligned and once as offset views 8 bytes off (tests/views.py),
`partials`, the state, the control block and the history in exact-size buffers of tests/scratch.py with both
poison fills.  In the batch of three, system 1 is inactive: not a bit of its x, r, p or state may change.

Bit-for-bit batch test: a batch through ``LinOpPinv._apply_cols`` equals its single solves when the operator's
own batched form computes each line as it computes a single vector -- the CSR kernels (one workgroup scheme per
row whatever the batch) and the line loop of Convolve1D.  A dense operator goes through the BLAS, which picks
its kernel (and summation order) by the batch size, so that case is held to the bound, not to the bits.

The Kronecker bound.  K^+ = A^+ (x) B^+ is applied as two batched solves.  Line by line the first leaves an
error of at most rtol ||A^T y_l|| / sigma_A^2, which the exact B^+ amplifies by 1 / sigma_B; the second adds
rtol ||B^T z_c|| / sigma_B^2 with ||z_c|| <= ||y|| / sigma_A (to first order in rtol).  Summed over the lines
(Frobenius norm): ||x - x*|| <= rtol ||y|| (||A|| / (sigma_A^2 sigma_B) + ||B|| / (sigma_B^2 sigma_A))
<= 2 rtol ||K|| ||y|| / sigma_min(K)^2, with ||K|| = ||A|| ||B|| and sigma_min(K) = sigma_A sigma_B.
"""

import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import pinv_cases as C
from tests import scratch as S
from tests import views as V

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
OFF8 = {np.float32: 2, np.float64: 1}            # elements that put a view 8 bytes off 16-byte alignment
TOL = {np.float64: 1e-12, np.float32: 2e-6}      # tests/test_gpu_kron.py
RHO, PQ, ALPHA, BETA, TOLF, BNRM, ACTIVE, BREAK = range(8)


def _lib():
    from pycsou_amd import _lib as L
    lib = L.gpu()
    assert L.PCS_CG_MAX_BLOCKS == C.CAP
    return L, lib


def _vec(a, dtype, layout):
    """(nb, n) values as a guarded view; `layout`: 'aligned' or 'offset' (8 bytes off)."""
    off = 0 if layout == 'aligned' else OFF8[dtype]
    v = V.guarded(np.ascontiguousarray(a).astype(dtype).ravel(), off, device='cuda')
    V.assert_misaligned(v, off)
    return v


def _bits(t):
    return t.clone()


def _same(view, values, dtype):
    return V.same_bits(view, torch.as_tensor(np.ascontiguousarray(values).astype(dtype).ravel()).to(view.device))


def _loop_buffers(L, lib, n, nb, poison, it=1, max_iter=100, hist_rows=8):
    """state (zeroed, the test fills it), partials, ctrl, hist at their advertised sizes."""
    state = S.scratch(int(lib.pcs_cg_state_bytes(nb)), 'zero', 'cuda')
    partials = S.scratch(8 * int(lib.pcs_cg_nblocks(n, nb)), poison, 'cuda')
    ctrl = S.scratch(int(lib.pcs_ctrl_bytes()), poison, 'cuda')
    hist = S.scratch(8 * (2 * hist_rows + 2), poison, 'cuda')
    assert lib.pcs_ctrl_init2(L.ptr(ctrl), 0, max_iter, 0.0, 0, hist.numel(), L.stream()) == 0
    ctrl.view(torch.int32)[0] = it
    return state, partials, ctrl, hist


def _set_state(state, rows):
    state.copy_(torch.as_tensor(np.asarray(rows, dtype=np.float64).ravel()))


def _active(nb):
    return np.array([1.0] if nb == 1 else [1.0, 0.0, 1.0])


CASES = [(n, nb, dt) for n in C.ONE_LAUNCH_N for nb in C.ONE_LAUNCH_NB for dt in DTYPES]
IDS = [f'n{n}-nb{nb}-{np.dtype(dt).name}' for n, nb, dt in CASES]


# ---------------------------------------------------------------- pcs_cg_dir
@pytest.mark.parametrize('n,nb,dtype', CASES, ids=IDS)
def test_dir_one_launch(n, nb, dtype):
    L, lib = _lib()
    code = L.PCS_F32 if dtype == np.float32 else L.PCS_F64
    _, r0, p0, _ = C.exact_vectors(n, nb)
    act = _active(nb)
    for layout in ('aligned', 'offset'):
        for poison in ('poison_a', 'poison_b'):
            r, p = _vec(r0, dtype, layout), _vec(p0, dtype, layout)
            state, partials, ctrl, hist = _loop_buffers(L, lib, n, nb, poison, it=1)
            rows = np.zeros((nb, 8))
            rows[:, BETA], rows[:, ACTIVE] = C.BETA, act
            _set_state(state, rows)
            snap = [_bits(t) for t in (r, state, ctrl)]
            call = lambda: lib.pcs_cg_dir(code, L.ptr(r), L.ptr(p), n, nb, L.ptr(state), L.ptr(ctrl), L.stream())  # noqa: E731
            assert call() == 0
            torch.cuda.synchronize()
            want = np.where(act[:, None] != 0, C.dir_ref(r0, p0), p0)
            assert _same(p, want, dtype), (layout, poison)
            # iteration 0: p = r whatever p held
            p.view(V._INT[p.dtype]).fill_(V._NAN_B[p.dtype])
            keep = _bits(p)
            ctrl.view(torch.int32)[0] = 0
            snap[2] = _bits(ctrl)
            assert call() == 0
            torch.cuda.synchronize()
            got = p.view(nb, n)
            for j in range(nb):
                assert V.same_bits(got[j], (r if act[j] else keep).view(nb, n)[j]), (layout, poison, j)
            # stopped: nothing is written
            ctrl.view(torch.int32)[1] = 1
            snap[2] = _bits(ctrl)
            p.view(nb, n)[0].fill_(7.0)
            keep = _bits(p)
            assert call() == 0
            torch.cuda.synchronize()
            assert V.same_bits(p, keep)
            for t, s in zip((r, state, ctrl), snap):
                assert V.same_bits(t, s)
            V.check_guards(r, p)
            S.check(state, partials, ctrl, hist)
            assert S.high_water(partials, poison) == 0 and S.high_water(hist, poison) == 0


# ---------------------------------------------------------------- pcs_cg_dot
@pytest.mark.parametrize('n,nb,dtype', CASES, ids=IDS)
def test_dot_one_launch(n, nb, dtype):
    L, lib = _lib()
    code = L.PCS_F32 if dtype == np.float32 else L.PCS_F64
    _, _, p0, q0 = C.exact_vectors(n, nb)
    act = _active(nb)
    pq = C.dot_terms(p0, q0).sum(axis=1)
    for layout in ('aligned', 'offset'):
        for poison in ('poison_a', 'poison_b'):
            p, q = _vec(p0, dtype, layout), _vec(q0, dtype, layout)
            state, partials, ctrl, hist = _loop_buffers(L, lib, n, nb, poison)
            rows = np.zeros((nb, 8))
            rows[:, RHO], rows[:, ACTIVE], rows[:, ALPHA], rows[:, TOLF] = 0.5 * pq, act, -1.0, 3.0
            _set_state(state, rows)
            snap = [_bits(t) for t in (p, q, ctrl)]
            call = lambda: lib.pcs_cg_dot(code, L.ptr(p), L.ptr(q), n, nb, C.EPS2, L.ptr(state), L.ptr(partials),  # noqa: E731
                                          L.ptr(ctrl), L.stream())
            assert call() == 0
            torch.cuda.synchronize()
            want = rows.copy()
            want[act != 0, PQ] = pq[act != 0]
            want[act != 0, ALPHA] = C.ALPHA
            got = state.cpu().numpy().reshape(nb, 8)
            assert np.array_equal(got, want), (layout, poison, got, want)
            # stopped: nothing is written
            ctrl.view(torch.int32)[1] = 1
            snap[2] = _bits(ctrl)
            rows2 = want.copy()
            rows2[:, ALPHA] = -2.0
            _set_state(state, rows2)
            parts = _bits(partials)
            assert call() == 0
            torch.cuda.synchronize()
            assert np.array_equal(state.cpu().numpy().reshape(nb, 8), rows2) and V.same_bits(partials, parts)
            for t, s in zip((p, q, ctrl), snap):
                assert V.same_bits(t, s)
            V.check_guards(p, q)
            S.check(state, partials, ctrl, hist)
            assert S.high_water(hist, poison) == 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_dot_breakdown_freezes_the_system(dtype):
    """pq = 0 (p = 0): breakdown is set, the system goes inactive, alpha is left alone; the update that follows
    does not touch its vectors."""
    L, lib = _lib()
    code = L.PCS_F32 if dtype == np.float32 else L.PCS_F64
    n, nb = 65, 3
    x0, r0, p0, q0 = C.exact_vectors(n, nb)
    p0[2] = 0.0
    x, r, p, q = (_vec(a, dtype, 'aligned') for a in (x0, r0, p0, q0))
    state, partials, ctrl, hist = _loop_buffers(L, lib, n, nb, 'poison_a')
    pq = C.dot_terms(p0, q0).sum(axis=1)
    rows = np.zeros((nb, 8))
    rows[:, RHO], rows[:, ACTIVE], rows[:, ALPHA], rows[:, BNRM], rows[:, TOLF] = 0.5 * np.maximum(pq, 1.0), 1.0, -1.0, 2.0, 0.0
    _set_state(state, rows)
    assert lib.pcs_cg_dot(code, L.ptr(p), L.ptr(q), n, nb, C.EPS2, L.ptr(state), L.ptr(partials), L.ptr(ctrl),
                          L.stream()) == 0
    torch.cuda.synchronize()
    got = state.cpu().numpy().reshape(nb, 8)
    assert pq[2] == 0 and got[2, BREAK] == 1 and got[2, ACTIVE] == 0 and got[2, ALPHA] == -1 and got[2, PQ] == 0
    assert np.array_equal(got[:2, BREAK], [0, 0]) and np.array_equal(got[:2, ACTIVE], [1, 1])
    assert np.array_equal(got[:2, ALPHA], [C.ALPHA, C.ALPHA])
    keep = [_bits(t) for t in (x, r, p)]
    assert lib.pcs_cg_update(code, L.ptr(x), L.ptr(r), L.ptr(p), L.ptr(q), n, nb, C.EPS2, L.ptr(state), L.ptr(partials),
                             L.ptr(ctrl), L.ptr(hist), L.stream()) == 0
    torch.cuda.synchronize()
    for t, k in zip((x, r, p), keep):
        assert V.same_bits(t.view(nb, n)[2], k.view(nb, n)[2])
    assert not V.same_bits(x.view(nb, n)[0], keep[0].view(nb, n)[0])
    assert hist[3].item() == 2.0                          # row 1 (it = 1): two systems still active
    V.check_guards(x, r, p, q)
    S.check(state, partials, ctrl, hist)


# ---------------------------------------------------------------- pcs_cg_update
def _update_want(rows, act, rr, it, max_iter, hist_rows):
    """State, (it, stopped) and the history row after one update, from the exact sums rr of r' . r'."""
    want = rows.copy()
    on = act != 0
    want[on, BETA] = rr[on] / rows[on, RHO]
    want[on, RHO] = rr[on]
    want[on, ACTIVE] = np.where(np.sqrt(rr[on]) < rows[on, TOLF], 0.0, 1.0)
    ratio = np.where(want[:, BNRM] > 0, np.sqrt(want[:, RHO]) / np.where(want[:, BNRM] > 0, want[:, BNRM], 1.0), 0.0)
    cnt = float(want[:, ACTIVE].sum())
    nx = it + 1
    stopped = int(cnt == 0 or nx >= max_iter or 2 * nx + 1 >= 2 * hist_rows + 2)
    return want, (nx, stopped), (float(ratio.max()), cnt)


@pytest.mark.parametrize('n,nb,dtype', CASES, ids=IDS)
def test_update_one_launch(n, nb, dtype):
    L, lib = _lib()
    code = L.PCS_F32 if dtype == np.float32 else L.PCS_F64
    x0, r0, p0, q0 = C.exact_vectors(n, nb)
    act = _active(nb)
    xn, rn, rr = C.update_ref(x0, r0, p0, q0)
    rr = rr.sum(axis=1)
    it, max_iter, hist_rows = 2, 100, 8
    for layout in ('aligned', 'offset'):
        for poison in ('poison_a', 'poison_b'):
            x, r, p, q = (_vec(a, dtype, layout) for a in (x0, r0, p0, q0))
            state, partials, ctrl, hist = _loop_buffers(L, lib, n, nb, poison, it=it, max_iter=max_iter, hist_rows=hist_rows)
            rows = np.zeros((nb, 8))
            rows[:, RHO], rows[:, ALPHA], rows[:, ACTIVE] = 3.0 + np.arange(nb), C.ALPHA, act
            rows[:, TOLF], rows[:, BNRM] = 2.0, 4.0          # sqrt(rho') < 2 happens at the smallest sizes only
            _set_state(state, rows)
            snap = [_bits(t) for t in (p, q)]
            call = lambda: lib.pcs_cg_update(code, L.ptr(x), L.ptr(r), L.ptr(p), L.ptr(q), n, nb, C.EPS2, L.ptr(state),  # noqa: E731
                                             L.ptr(partials), L.ptr(ctrl), L.ptr(hist), L.stream())
            assert call() == 0
            torch.cuda.synchronize()
            on = act[:, None] != 0
            assert _same(x, np.where(on, xn, x0), dtype) and _same(r, np.where(on, rn, r0), dtype), (layout, poison)
            want, ctl, row = _update_want(rows, act, rr, it, max_iter, hist_rows)
            got = state.cpu().numpy().reshape(nb, 8)
            assert np.array_equal(got, want), (layout, poison, got, want)
            assert tuple(ctrl.view(torch.int32)[:2].tolist()) == ctl
            assert tuple(hist[2 * it:2 * it + 2].tolist()) == row, (hist[2 * it:2 * it + 2].tolist(), row)
            changed = S.words_changed(hist, poison).tolist()
            assert changed == [False] * (2 * it) + [True, True] + [False] * (hist.numel() - 2 * it - 2)
            # stopped: nothing is written
            ctrl.view(torch.int32)[1] = 1
            keep = [_bits(t) for t in (x, r, state, ctrl, hist, partials)]
            assert call() == 0
            torch.cuda.synchronize()
            for t, k in zip((x, r, state, ctrl, hist, partials), keep):
                assert V.same_bits(t, k)
            for t, s in zip((p, q), snap):
                assert V.same_bits(t, s)
            V.check_guards(x, r, p, q)
            S.check(state, partials, ctrl, hist)


def test_update_stops_at_max_iter_and_when_nothing_is_active():
    L, lib = _lib()
    n, nb = 257, 3
    x0, r0, p0, q0 = C.exact_vectors(n, nb)
    rr = C.update_ref(x0, r0, p0, q0)[2].sum(axis=1)
    for what in ('max_iter', 'all_converged'):
        x, r, p, q = (_vec(a, np.float64, 'aligned') for a in (x0, r0, p0, q0))
        state, partials, ctrl, hist = _loop_buffers(L, lib, n, nb, 'poison_b', it=2, max_iter=3 if what == 'max_iter' else 100)
        rows = np.zeros((nb, 8))
        rows[:, RHO], rows[:, ALPHA], rows[:, ACTIVE], rows[:, BNRM] = 1.0, C.ALPHA, 1.0, 1.0
        rows[:, TOLF] = 0.0 if what == 'max_iter' else 1e9
        _set_state(state, rows)
        assert lib.pcs_cg_update(L.PCS_F64, L.ptr(x), L.ptr(r), L.ptr(p), L.ptr(q), n, nb, C.EPS2, L.ptr(state),
                                 L.ptr(partials), L.ptr(ctrl), L.ptr(hist), L.stream()) == 0
        torch.cuda.synchronize()
        got = state.cpu().numpy().reshape(nb, 8)
        assert ctrl.view(torch.int32)[:2].tolist() == [3, 1]
        assert np.array_equal(got[:, ACTIVE], np.ones(nb) if what == 'max_iter' else np.zeros(nb))
        assert hist[4:6].tolist() == [float(np.sqrt(rr).max()), float(got[:, ACTIVE].sum())]


# ---------------------------------------------------------------- pcs_cg_init
@pytest.mark.parametrize('n,nb,dtype', CASES, ids=IDS)
def test_init_one_launch(n, nb, dtype):
    L, lib = _lib()
    code = L.PCS_F32 if dtype == np.float32 else L.PCS_F64
    b0, r0, _, _ = C.exact_vectors(n, nb)
    if nb == 3:
        b0[1] = 0.0                                       # a zero right-hand side: never active
        r0[2] = 0.0                                       # a start at the solution: converged before the first step
    rtol, max_iter = 2.0 ** -4, 7
    bb, rr = (b0 * b0).sum(axis=1), (r0 * r0).sum(axis=1)
    bn = np.sqrt(bb)
    tol = np.maximum(0.0, rtol * bn)
    act = ((bn > 0) & ~(np.sqrt(rr) < tol)).astype(np.float64)
    for layout in ('aligned', 'offset'):
        for poison in ('poison_a', 'poison_b'):
            b, r = _vec(b0, dtype, layout), _vec(r0, dtype, layout)
            state = S.scratch(int(lib.pcs_cg_state_bytes(nb)), poison, 'cuda')
            partials = S.scratch(8 * int(lib.pcs_cg_nblocks(n, nb)), poison, 'cuda')
            ctrl = S.scratch(int(lib.pcs_ctrl_bytes()), poison, 'cuda')
            hist = S.scratch(8 * 18, poison, 'cuda')
            snap = [_bits(t) for t in (b, r)]
            assert lib.pcs_cg_init(code, L.ptr(b), L.ptr(r), n, nb, rtol, 0.0, max_iter, L.ptr(state), L.ptr(partials),
                                   L.ptr(ctrl), L.ptr(hist), hist.numel(), L.stream()) == 0
            torch.cuda.synchronize()
            want = np.zeros((nb, 8))
            want[:, RHO], want[:, TOLF], want[:, BNRM], want[:, ACTIVE] = rr, tol, bn, act
            got = state.cpu().numpy().reshape(nb, 8)
            assert np.array_equal(got, want), (layout, poison, got, want)
            f = ctrl.view(torch.int32).tolist()
            assert f[:6] == [0, int(act.sum() == 0), 0, max_iter, 0, hist.numel()] and f[6] == 0, f
            assert ctrl[4].item() == 0.0
            assert S.high_water(hist, poison) == 0
            for t, s in zip((b, r), snap):
                assert V.same_bits(t, s)
            V.check_guards(b, r)
            S.check(state, partials, ctrl, hist)
    if nb == 3 and n > 1:
        assert act.tolist() == [1.0, 0.0, 0.0]


def test_init_with_no_iterations_allowed_or_nothing_to_do_is_stopped():
    L, lib = _lib()
    b0, _, _, _ = C.exact_vectors(65, 1)
    for max_iter, b_np, stopped in ((0, b0, 1), (5, np.zeros_like(b0), 1), (5, b0, 0)):
        b = _vec(b_np, np.float32, 'aligned')
        state, partials, ctrl, hist = _loop_buffers(L, lib, 65, 1, 'poison_a')
        assert lib.pcs_cg_init(L.PCS_F32, L.ptr(b), L.ptr(b), 65, 1, 1e-5, 0.0, max_iter, L.ptr(state), L.ptr(partials),
                               L.ptr(ctrl), L.ptr(hist), hist.numel(), L.stream()) == 0
        torch.cuda.synchronize()
        assert ctrl.view(torch.int32)[:2].tolist() == [0, stopped]


# ---------------------------------------------------------------- the solver
def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a).astype(dtype)).to('cuda')


_REF = {}


def _reference(name):
    """x*, bound and SciPy's three-iteration iterate per right-hand side, computed once per case."""
    if name not in _REF:
        c = C.case(name)
        k = c['Y'].shape[0]
        c0 = dict(c, eps=0.0)
        _REF[name] = {'case': c, 'xs': [C.solution(c, j) for j in range(k)], 'bound': [C.bound(c, j) for j in range(k)],
                      'xs0': C.solution(c0, 0), 'bound0': C.bound(c0, 0),
                      'x3': [C.cg_ref(*C.normal_system(c, j), maxiter=3)[0] for j in range(k)]}
    return _REF[name]


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('name', C.CASES)
def test_pinv_and_dagger_meet_the_bound(name, dtype):
    from pycsou_amd.core.linop import LinOpPinv
    ref = _reference(name)
    c = ref['case']
    op = C.make_op(c, dtype)
    n = c['A'].shape[1]
    for j, y in enumerate(c['Y'].astype(dtype)):
        x = op.pinv(y, c['eps'])
        assert isinstance(x, np.ndarray) and x.dtype == dtype and x.shape == (n,)
        err = float(np.linalg.norm(x.astype(np.float64) - ref['xs'][j]))
        print(f'PINV {name} {np.dtype(dtype).name} rhs {j}: err {err:.3e} bound {ref["bound"][j]:.3e}')
        assert err <= ref['bound'][j], (j, err, ref['bound'][j])
        # the device's own history obeys the stop rule
        D = LinOpPinv(op, c['eps'])
        X, it, info = D.solve(_dev(y, dtype).reshape(1, -1))
        assert np.array_equal(X.cpu().numpy().ravel(), x), 'two solves of one system differ'
        assert it == info.hist.shape[0] <= 10 * n and not info.breakdown.any() and not info.active.any()
        if np.any(y):
            assert it >= 1 and info.hist[-1, 0] < C.RTOL and np.all(info.hist[:-1, 0] >= C.RTOL)
            assert info.hist[-1, 1] == 0 and np.all(info.hist[:-1, 1] == 1)
        else:
            assert it == 0 and not np.any(x)
    d = op.dagger(c['Y'][0].astype(dtype))
    err = float(np.linalg.norm(d.astype(np.float64) - ref['xs0']))
    print(f'PINV {name} {np.dtype(dtype).name} dagger: err {err:.3e} bound {ref["bound0"]:.3e}')
    assert err <= ref['bound0']


@pytest.mark.parametrize('name', [n for n in C.CASES if n != 'one'])
def test_three_iterations_match_scipy_in_fp64(name):
    from pycsou_amd.core.linop import LinOpPinv
    ref = _reference(name)
    c = ref['case']
    D = LinOpPinv(C.make_op(c, np.float64), c['eps'])
    for j in range(c['Y'].shape[0]):
        if not np.any(c['Y'][j]):
            continue
        X, it, info = D.solve(_dev(c['Y'][j], np.float64).reshape(1, -1), maxiter=3)
        r = V.rel_l2(X.cpu().numpy().ravel(), ref['x3'][j])
        print(f'PINV {name} rhs {j} after 3 iterations: rel {r:.3e}')
        assert it == 3 and info.active.all() and info.hist.shape == (3, 2) and r < TOL[np.float64]


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('name', ['sparse', 'conv1d'])
def test_batch_equals_single_solves_bit_for_bit(name, dtype):
    from pycsou_amd.core.linop import LinOpPinv
    c = _reference(name)['case']
    D = LinOpPinv(C.make_op(c, dtype), c['eps'])
    Y = _dev(c['Y'], dtype)
    singles, its = [], []
    for j in range(Y.shape[0]):
        singles.append(D._apply(Y[j].contiguous()))
        its.append(D.last[0])
    singles = torch.stack(singles)
    rows = D._apply_cols(Y, 1)
    assert D.last[0] == max(its)
    cols = D._apply_cols(Y.t().contiguous(), 0)
    assert rows.shape == singles.shape and rows.is_contiguous() and cols.is_contiguous()
    assert torch.equal(rows, singles) and torch.equal(cols, singles.t())


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_dense_batch_and_zero_right_hand_side(dtype):
    """The dense batch against the bound (module docstring); the zero right-hand side gives exact zeros and never
    runs, while the others converge."""
    from pycsou_amd.core.linop import LinOpPinv
    ref = _reference('zero_rhs')
    c = ref['case']
    D = LinOpPinv(C.make_op(c, dtype), c['eps'])
    X, it, info = D.solve(_dev(c['Y'], dtype))
    Xh = X.cpu().numpy().astype(np.float64)
    assert it > 0 and not info.active.any() and not info.breakdown.any()
    assert not np.any(Xh[1]) and info.rnorm[1] == 0
    for j in (0, 2):
        assert np.linalg.norm(Xh[j] - ref['xs'][j]) <= ref['bound'][j]
    assert info.hist[-1, 0] < C.RTOL and info.hist[0, 1] == 2         # the zero system was never active
    Xz, itz, infoz = D.solve(_dev(c['Y'][1:2], dtype))
    assert itz == 0 and not bool(Xz.any()) and infoz.hist.shape == (0, 2)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_eager_and_graph_chunks_are_bit_identical_and_repeatable(dtype):
    from pycsou_amd.core.linop import LinOpPinv
    c = _reference('sparse')['case']
    D = LinOpPinv(C.make_op(c, dtype), c['eps'])
    Y = _dev(c['Y'], dtype)
    X0, it0, _ = D.solve(Y, use_graph=False)
    assert it0 > 8
    for chunk in (1, 4):
        X, it, info = D.solve(Y, chunk=chunk)
        plan = D._plans[(3, Y.dtype, chunk, True)]
        assert plan.graph is not None, 'the chunk was not captured'
        assert it == it0 and torch.equal(X, X0), chunk
        X2, it2, info2 = D.solve(Y, chunk=chunk)                          # the same plan and graph again
        assert it2 == it0 and torch.equal(X2, X0) and np.array_equal(info2.hist, info.hist)
    X1, it1, _ = D.solve(Y, use_graph=False)
    assert it1 == it0 and torch.equal(X1, X0)


def test_batch_larger_than_the_grid_is_split():
    """65 537 systems of one unknown (A = [2]: x = y / 2 after one iteration, exactly): more than the 65 535 rows
    of a grid, so two slices, the second of two systems."""
    from pycsou_amd import _ops as O
    from pycsou_amd.core.linop import LinOpPinv
    from pycsou_amd.linop import DenseLinearOperator
    D = LinOpPinv(DenseLinearOperator(np.array([[2.0]])))
    nb = O.CG_MAX_NB + 2
    Y = torch.arange(1, nb + 1, dtype=torch.float64, device='cuda').reshape(nb, 1)
    X, it, info = D.solve(Y)
    assert it == 1 and torch.equal(X, Y / 2) and info.rnorm.shape == (nb,) and not info.active.any()
    assert sorted(k[0] for k in D._plans) == [2, O.CG_MAX_NB]
    one = torch.empty((O.CG_MAX_NB + 1, 1), dtype=torch.float64, device='cuda')
    L, lib = _lib()
    assert lib.pcs_cg_dir(L.PCS_F64, L.ptr(one), L.ptr(Y), 1, O.CG_MAX_NB + 1, L.ptr(one), L.ptr(one), L.stream()) == -3


def test_x0_at_the_solution_takes_no_iteration():
    c = _reference('tall')['case']
    op = C.make_op(c, np.float64)
    y = c['Y'][0]
    x = op.pinv(y, c['eps'], rtol=1e-9)
    from pycsou_amd.core.linop import LinOpPinv
    D = LinOpPinv(op, c['eps'])
    X, it, info = D.solve(_dev(y, np.float64).reshape(1, -1), x0=_dev(x, np.float64))
    assert it == 0 and np.array_equal(X.cpu().numpy().ravel(), x) and not info.active.any()
    assert np.array_equal(op.pinv(y, c['eps'], x0=x), x)
    far = op.pinv(y, c['eps'], x0=x + 1.0)        # a start elsewhere: N is nonsingular here, the same bound holds
    assert np.linalg.norm(far - _reference('tall')['xs'][0]) <= _reference('tall')['bound'][0]


def test_keywords_tol_atol_and_ignored_ones():
    c = _reference('tall')['case']
    op = C.make_op(c, np.float64)
    y = c['Y'][0]
    loose = op.pinv(y, 0, tol=1e-2, show=True, returninfo=False)          # PyLops keywords are accepted
    assert np.array_equal(loose, op.pinv(y, 0, rtol=1e-2))
    assert not np.array_equal(loose, op.pinv(y, 0))
    assert np.array_equal(op.pinv(y, 0, atol=1e9), np.zeros(32))          # ||r|| < atol from the start


def test_null_operator_is_the_zero_rhs_path():
    from pycsou_amd.linop.base import NullOperator
    op = NullOperator((5, 4))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        x = op.pinv(np.arange(5.0) + 1.0)
        assert x.shape == (4,) and not np.any(x)
        D = op.dagger
        assert not np.any(D(np.ones(5))) and D.last[0] == 0 and not D.last[1].breakdown.any()


# ---------------------------------------------------------------- algebra
def test_projectors():
    ref = _reference('tall')
    c = ref['case']
    A = c['A']
    op = C.make_op(c, np.float64)
    x = np.random.default_rng(3).standard_normal(32)
    bnd = C.RTOL * np.linalg.norm(A.T @ (A @ x)) / C.lam_min(c)
    assert np.linalg.norm(op.RowProjector(x) - x) <= 10 * bnd
    y = c['Y'][0]
    P = op.ColProjector
    py = P(y)
    assert np.linalg.norm(P(py) - py) <= 10 * ref['bound'][0]
    assert np.linalg.norm(py - A @ ref['xs'][0]) <= 10 * ref['bound'][0]


def test_adjoint_of_the_pseudo_inverse():
    c = _reference('tall')['case']
    A = c['A']
    op = C.make_op(c, np.float64)
    v = np.random.default_rng(4).standard_normal(32)
    a, b = op.dagger.adjoint(v), op.H.dagger(v)
    assert a.shape == (48,) and np.array_equal(a, b)
    At = {'A': A.T.copy(), 'eps': 0.0, 'Y': v[None, :]}
    assert np.linalg.norm(a - C.solution(At, 0)) <= C.bound(At, 0)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_kronecker_pinv(dtype):
    from pycsou_amd.core.linop import LinOpPinv
    from pycsou_amd.linop import DenseLinearOperator, KroneckerProduct
    A, B = C._gauss(6, 4, 7), C._gauss(5, 3, 8)
    K = KroneckerProduct(DenseLinearOperator(A.astype(dtype)), DenseLinearOperator(B.astype(dtype)))
    M = np.kron(B, A)
    assert K.shape == M.shape == (30, 12)
    y = V.rounded(np.random.default_rng(5).standard_normal(30), np.float32)
    Kp = K.PinvOp
    assert isinstance(Kp, KroneckerProduct) and isinstance(Kp.linop1, LinOpPinv) and Kp.shape == (12, 30)
    x = Kp(y.astype(dtype))
    bnd = 2 * C.RTOL * np.linalg.norm(M, 2) * np.linalg.norm(y) / C.sigma_min(M) ** 2
    err = np.linalg.norm(x.astype(np.float64) - np.linalg.pinv(M) @ y)
    print(f'PINV kron {np.dtype(dtype).name}: err {err:.3e} bound {bnd:.3e}')
    assert err <= bnd
    assert Kp.linop1.last[1].rnorm.shape == (5,) and Kp.linop2.last[1].rnorm.shape == (4,)    # one batch per factor


def _gradient_matrix(shape):
    from oracle import pylops1 as P
    g = P.Gradient(shape, sampling=1.0, edge=True, kind='forward')
    n = int(np.prod(shape))
    return np.stack([g.matvec(e) for e in np.eye(n)], axis=1)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_todense_tosparse(dtype):
    from pycsou_amd.linop import DenseLinearOperator, Gradient, SparseLinearOperator
    name = np.dtype(dtype).name
    ops = {'gradient': (Gradient((5, 4), kind='forward', dtype=name), _gradient_matrix((5, 4))),
           'sparse': (C.make_op(C.case('sparse'), dtype), C.case('sparse')['A']),
           'conv1d': (C.make_op(C.case('conv1d'), dtype), C.case('conv1d')['A'])}
    for key, (op, M) in ops.items():
        D = op.todense()
        assert isinstance(D, DenseLinearOperator) and isinstance(D.mat, torch.Tensor) and D.mat.is_cuda
        assert D.shape == M.shape and D.mat.dtype == V.tdtype(dtype)
        assert V.rel_l2(D.mat.cpu().numpy(), M) < TOL[dtype], key
        v = np.random.default_rng(6).standard_normal(M.shape[1]).astype(dtype)
        assert V.rel_l2(D(v), M @ v.astype(np.float64)) < 10 * TOL[dtype]
        Sp = op.tosparse()
        assert isinstance(Sp, SparseLinearOperator) and sp.issparse(Sp.mat) and Sp.shape == M.shape
        assert V.rel_l2(Sp.mat.toarray(), M) < TOL[dtype] and Sp.mat.nnz == np.count_nonzero(M)
        assert V.rel_l2(Sp(v), M @ v.astype(np.float64)) < 10 * TOL[dtype]
    wide = DenseLinearOperator(np.arange(6.0).reshape(2, 3))
    wide.TODENSE_BLOCK = 2                                                # more than one column block
    assert np.array_equal(wide.todense().mat.cpu().numpy(), wide.mat)


def test_cond():
    from pycsou_amd.linop.base import NullOperator
    for name in ('tall', 'wide', 'conv1d'):
        c = C.case(name)
        got = C.make_op(c, np.float64).cond()
        s = np.linalg.svd(c['A'], compute_uv=False)
        want = s[0] / C.sigma_min(c['A'])
        assert abs(got - want) <= 1e-10 * want, (name, got, want)
        if name == 'tall':
            assert abs(got - np.linalg.cond(c['A'])) <= 1e-10 * got
    assert C.make_op(C.case('tall'), np.float32).cond(uselobpcg=True) > 1       # PyLops keywords are accepted
    with pytest.raises(NotImplementedError, match='2048'):
        NullOperator((2049, 2100)).cond()
