"""What the element-wise GPU tests of the fused APGD launch (tests/test_gpu_apgd_pointwise.py) rely on, proved
without a GPU: the derived bound holds for a plain fp32 evaluation of the same update, the inputs of every
case of the matrix make each prox bind on both sides and the momentum term count, and the comparator fails on
each kernel mistake the norm-based tests (tests/test_gpu_apgd2d.py) cannot be trusted to see -- while their
criterion passes two of them."""

import numpy as np
import pytest

from tests import pointwise as PW
from tests import pointwise_apgd as PA
from tests.cases import rel

A = (150, 200)  # two row segments of 75 rows, fp32 strips of 128 + 72 columns
COEFFS = [PA.A0, PA.A1, PA.A0]


@pytest.fixture(scope='module')
def base():
    """The (150, 200) 15 x 15 fp32 case with G = Segment, its one-launch fp64 reference and bound."""
    p = PA.make_problem(A, 'sep15', 'segment', seed=3, dtype=np.float32)
    u = PA.oracle_update(p, p['x'], p['aux'], PA.A0)
    return p, u, PA.bound(p, [(p['x'], p['aux'], PA.A0)])


@pytest.mark.parametrize('gname', ['', 'segment'])
@pytest.mark.parametrize('nit', [1, 2, 3])
def test_fp32_restatement_within_bound(nit, gname):
    """The oracle itself in np.float32 (NumPy's operation order, no FMA) against the fp64 oracle for launches
    with a = 0.61, -0.35, 0.61: inside nit c eps M with c = 76.  Measured worst element, in units of eps M
    (x') / eps Mw (aux'): x' 0.35 / 0.32 / 0.36 (nit 1 / 2 / 3) with G none, 0.24 / 0.21 / 0.27 with the segment
    (it clips the largest values); aux' 0.30 / 0.48 / 0.47 and 0.30 / 0.39 / 0.49.  About c / 200: roundings add
    like a random walk and the partial sums of 15 positive taps of about 1 / 15 each stay far below M."""
    p = PA.make_problem(A, 'sep15', gname, seed=3, dtype=np.float32)
    co = COEFFS[:nit]
    r = PA.oracle_run(p, co)
    s = PA.oracle_run(p, co, dtype=np.float32)
    assert s[-1].x.dtype == np.float32 and s[-1].aux.dtype == np.float32
    b = PA.bound(p, PA.run_states(p, co, r))
    assert b['x'].c == 76 and b['x'].tol == nit * 76 * b['x'].unit
    rx = PA.compare(s[-1].x, r[-1].x, b['x'], A, 'x', hist=[u.metric for u in s], hist_ref=[u.metric for u in r],
                    dtype=np.float32)
    ra = PA.compare(s[-1].aux, r[-1].aux, b['aux'], A, 'aux')
    print(f'fp32 restatement nit={nit} G={gname or "none"}: x {rx:.2f} aux {ra:.2f} eps*M (c = {b["x"].c})')
    assert 0 < rx and 0 < ra  # fp32 arithmetic did run


def test_matrix_covers_what_it_must():
    """Every shape x both dtypes with two G kinds, each G on three shapes per dtype, every PSF, every geometry."""
    kinds = ('', 'l1', 'nonneg', 'segment')
    for dt in ('f32', 'f64'):
        for shape in PA.GEOM:
            assert len({c.g for c in PA.CASES if c.shape == shape and c.dtype == dt}) >= 2, (shape, dt)
        for g in kinds:
            assert len({c.shape for c in PA.CASES if c.g == g and c.dtype == dt}) >= 3, (g, dt)
    assert {c.fk for c in PA.CASES} == set(PA.PSFS)
    assert {fk: PA.psf_half(fk) for fk in PA.PSFS} == {'sep15': 7, 'sep7': 3, 'sep6x10': 5, 'sep5x9': 4, 'sep1x5': 2}
    assert any(c.tau != 1.0 and c.g == 'l1' for c in PA.CASES)
    for shape, per_dtype in PA.GEOM.items():  # the table against the launcher's rule (csrc/sep_nrm.hpp nrm_grid)
        for tx, (nstrips, nseg) in zip((128, 64), per_dtype):
            want = max(1, shape[0] // 64)
            seg_len = -(-shape[0] // want)
            assert (nstrips, nseg) == (-(-shape[1] // tx), -(-shape[0] // seg_len)), shape


@pytest.mark.parametrize('i', PA.MATRIX, ids=PA.case_id)
def test_input_conditions(i):
    """Every case of the GPU matrix, at the first launch on the oracle's side: each bound G has clips at least
    10 % of the pixels, L1 zeroes between 10 % and 90 %, the momentum term a (w - aux) exceeds 100 x the bound on
    at least half the pixels, and both metrics are finite and positive."""
    c, p = PA.case_problem(i)
    ups = PA.case_oracle(i)
    u = ups[0]
    b = PA.bound(p, [(p['x'], p['aux'], PA.A0)])
    if p['gname'] in ('nonneg', 'segment'):
        lo = PW.SEG[0] if p['gname'] == 'segment' else 0.0
        assert np.mean(u.v < lo) >= 0.10
        assert np.all(u.w[u.v < lo] == lo)
    if p['gname'] == 'segment':
        assert np.mean(u.v > PW.SEG[1]) >= 0.10
        assert np.all(u.w[u.v > PW.SEG[1]] == PW.SEG[1])
    if p['gname'] == 'l1':
        zeroed = np.mean(np.abs(u.v) <= p['tau'] * p['lam'])
        assert 0.10 <= zeroed <= 0.90, zeroed
        assert np.mean(u.w == 0) >= 0.10
    assert np.mean(np.abs(PA.A0 * (u.w - p['aux'])) > 100 * b['x'].tol) >= 0.5
    for k in (0, 1):
        assert np.isfinite(ups[k].metric) and ups[k].metric > 0


def _fails(got, ref, bound, name='x', shape=A):
    with pytest.raises(AssertionError, match='eps\\*M'):
        PA.compare(got, ref, bound, shape, name)


def _wrong_psf(base, psf):
    p, u, b = base
    q = dict(p, psf=psf)
    uq = PA.oracle_update(q, p['x'], p['aux'], PA.A0)
    _fails(uq.x, u.x, b['x'])
    _fails(uq.aux, u.aux, b['aux'], 'aux')


def test_detects_dropped_outer_tap(base):
    p = base[0]
    for axis in (0, 1):
        t = [p['t0'].copy(), p['t1'].copy()]
        t[axis][-1] = 0.0
        _wrong_psf(base, np.outer(*t))


def test_detects_reversed_taps(base):
    p = base[0]
    _wrong_psf(base, np.outer(p['t0'][::-1], p['t1']))
    _wrong_psf(base, np.outer(p['t0'], p['t1'][::-1]))


def test_detects_swapped_axes(base):
    p = base[0]
    _wrong_psf(base, np.outer(p['t1'], p['t0']))


@pytest.mark.parametrize('axis', ['row', 'col'])
@pytest.mark.parametrize('j', [0, 3, 6])
def test_detects_interior_window_on_an_edge(base, j, axis):
    p, u, b = base
    ud = PA.oracle_update(p, p['x'], p['aux'], PA.A0, grad=PA.dense_grad(p))
    assert np.max(np.abs(ud.x - u.x)) < 1e-13  # the dense form is the oracle's operator
    uq = PA.oracle_update(p, p['x'], p['aux'], PA.A0, grad=PA.dense_grad(p, **{'interior_' + axis: j}))
    where = f'\\(row {j}, col ' if axis == 'row' else f', col {j}\\)'  # nothing else differs
    with pytest.raises(AssertionError, match=where):
        PA.compare(uq.x, u.x, b['x'], A, 'x')
    _fails(uq.aux, u.aux, b['aux'], 'aux')


def test_detects_aux_replaced_by_x(base):
    p, u, b = base
    uq = PA.oracle_update(p, p['x'], p['x'], PA.A0)  # the wrong parity buffer, or x's descriptor for aux
    _fails(uq.x, u.x, b['x'])


def test_detects_aux_stored_as_the_new_iterate(base):
    p, u, b = base
    _fails(u.x, u.aux, b['aux'], 'aux')


def test_detects_momentum_on_the_wrong_operand(base):
    p, u, b = base
    _fails(u.w + PA.A0 * (u.w - p['x']), u.x, b['x'])


def test_detects_coefficient_from_the_wrong_slot(base):
    """Two launches with the coefficients exchanged."""
    p, u, b = base
    r = PA.oracle_run(p, [PA.A0, PA.A1])
    q = PA.oracle_run(p, [PA.A1, PA.A0])
    b2 = PA.bound(p, PA.run_states(p, [PA.A0, PA.A1], r))
    _fails(q[-1].x, r[-1].x, b2['x'])


def test_detects_l1_threshold_without_tau():
    """tau = 1 / 4: a kernel thresholding at lam instead of tau lam."""
    p = PA.make_problem(A, 'sep15', 'l1', seed=4, dtype=np.float32, tau=0.25)
    u = PA.oracle_update(p, p['x'], p['aux'], PA.A0)
    uq = PA.oracle_update(dict(p, lam=p['lam'] / p['tau']), p['x'], p['aux'], PA.A0)
    b = PA.bound(p, [(p['x'], p['aux'], PA.A0)])
    _fails(uq.x, u.x, b['x'])
    _fails(uq.aux, u.aux, b['aux'], 'aux')


def test_detects_ignored_upper_bound(base):
    p, u, b = base
    uq = PA.oracle_update(dict(p, seg=(PW.SEG[0], np.inf)), p['x'], p['aux'], PA.A0)
    _fails(uq.x, u.x, b['x'])
    _fails(uq.aux, u.aux, b['aux'], 'aux')


@pytest.mark.parametrize('row,col', [(10, 128), (75, 37), (75, 128), (74, 64)])
def test_detects_single_element_at_a_seam(base, row, col):
    """One element off by 20 x the bound at the fp32 strip seam (column 128), the fp64 one (64) and the first
    row of the second row segment (75): a whole-image norm does not see it, the comparator names it."""
    p, u, b = base
    for ref, name in ((u.x, 'x'), (u.aux, 'aux')):
        q = ref.copy()
        q[row * A[1] + col] += 20 * b[name].tol
        assert rel(q, ref) < 5e-5
        msg = f'{name}: .*row {row}, col {col}.*col % 64 = {col % 64}.*; 1 elements'
        with pytest.raises(AssertionError, match=msg):
            PA.compare(q, ref, b[name], A, name)


@pytest.mark.parametrize('cid', ['f32-sep6x10-segment-21x36', 'f64-sep6x10-none-21x36'])
def test_detects_a_row_past_the_end_in_the_history(cid):
    """(21, 36): the last block of 4 rows holds rows 21-23, which are not the task's.  Their loads read 0 and
    their stores are dropped, but N x of such a row is what the ring holds -- the interior window one row past
    the end -- so without the `live` flag its x' would enter the sum of (x - x')^2.  One such row moves the
    metric by more than the history's bar."""
    i = [k for k in PA.MATRIX if PA.case_id(k) == cid][0]
    c, p = PA.case_problem(i)
    n0, n1 = p['shape']
    u = PA.case_oracle(i)[0]
    pad = 2 * len(p['t0'])
    Cb = PW.dense_conv1d(n0 + 2 * pad, p['t0'])
    C1 = PW.dense_conv1d(n1, p['t1'])
    # N x at row n0; x, aux and C^T y of that row read 0
    acc = (Cb.T @ Cb)[n0 + pad, pad:pad + n0] @ p['x'].reshape(n0, n1) @ (C1.T @ C1)
    w = PA.prox_g(p)(0.0 - p['tau'] * acc, p['tau'])
    xo = w + PA.A0 * (w - 0.0)
    d2 = np.sum((p['x'] - u.x) ** 2) + np.sum((0.0 - xo) ** 2)
    metric = np.sqrt(d2) / np.linalg.norm(p['x'])
    b = PA.bound(p, [(p['x'], p['aux'], PA.A0)])
    PA.compare(u.x, u.x, b['x'], p['shape'], 'x', hist=[u.metric], hist_ref=[u.metric], dtype=p['dtype'])
    with pytest.raises(AssertionError, match=PW.P_COL.replace('(', '\\(').replace(')', '\\)')):
        PA.compare(u.x, u.x, b['x'], p['shape'], 'x', hist=[metric], hist_ref=[u.metric], dtype=p['dtype'])


def _legacy_run(case, grad, g, acc, tau, nit=6, stale_aux=False):
    """tests/test_gpu_apgd2d.py's run on the oracle's side: x0 = 0, past_aux = 0, `nit` iterations.
    stale_aux: the momentum step reads the aux of two iterations ago (the wrong parity buffer)."""
    from oracle import pycsou_ref as OR
    prox = case.prox_G(g)
    x, aux, older = np.zeros(case.N), np.zeros(case.N), np.zeros(case.N)
    hist = []
    for a in PA.ref_coeffs(acc, 75., nit)[0]:
        w = prox(x - tau * grad(x), tau)
        xn = w + a * (w - (older if stale_aux else aux))
        hist.append(OR._rel(x, xn))
        older = aux
        x, aux = xn, w
    return x, aux, np.array(hist)


@pytest.mark.parametrize('g', ['none', 'l1', 'segment'])
def test_legacy_criterion_is_blind_to_an_edge_window(g):
    """The gap this closes: tests/apgd2d_cases.py's gauss15 problem at (70, 132) from x0 = 0, 'CD', 6 iterations,
    rel < 5e-5 on iterand and past_aux, diagnostics to 1e-3 -- row 6 of the vertical normal operator, or column
    6 of the horizontal one, computed with the interior window passes (measured rel 2e-7 ... 9e-6).  The same
    criterion does reject the window on row 0 (rel 2.5e-4 ... 3.7e-4; with L1 the row is thresholded to zero
    either way and nothing shows) and the wrong aux parity (rel 3e-3): those two it catches."""
    from tests.apgd2d_cases import case, psf_factors
    shape = (70, 132)
    c = case(shape, 'gauss15')
    t0, t1 = psf_factors('gauss15')
    q = dict(shape=shape, N=c.N, t0=t0, t1=t1, y=c.y)
    good = PA.dense_grad(q)
    assert np.max(np.abs(good(c.y) - c.grad_F(c.y))) < 1e-12  # the dense form is that oracle's grad F
    tau = 1.0  # the Gaussian taps sum to 1: beta = ||C||^2 is 1 to three digits
    x, aux, h = _legacy_run(c, good, g, 'CD', tau)
    for kw in (dict(interior_row=6), dict(interior_col=6)):
        xq, auxq, hq = _legacy_run(c, PA.dense_grad(q, **kw), g, 'CD', tau)
        assert np.max(np.abs(xq - x)) > 0
        assert rel(xq, x) < 5e-5 and rel(auxq, aux) < 5e-5, (kw, rel(xq, x), rel(auxq, aux))
        np.testing.assert_allclose(hq[1:], h[1:], rtol=1e-3)
    # ... what it does reject
    xq, auxq, hq = _legacy_run(c, good, g, 'CD', tau, stale_aux=True)
    assert rel(xq, x) > 5e-5
    if g != 'l1':
        xq, auxq, hq = _legacy_run(c, PA.dense_grad(q, interior_row=0), g, 'CD', tau)
        assert rel(xq, x) > 5e-5
    # ... and with the equal-weight taps of this module one launch shows all of them (the tests above)
