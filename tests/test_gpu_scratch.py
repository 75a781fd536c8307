"""Every C ABI entry that takes a caller-owned scratch buffer, run on scratch of exactly the advertised size,
between sentinel margins, with hostile contents (helpers, fills and data: tests/scratch.py; what they rely on,
shown without a GPU: tests/test_scratch_cpu.py).

One procedure for every case (`_procedure`): the entry point runs once per fill the header allows -- `zero`,
`poison_a` (a quiet NaN) and `poison_b` (all bytes 0xFF: NaN as a double, 0xFFFFFFFF as a counter) where the
contents may be arbitrary, `zero` alone where the header says "zeroed once before first use" -- and once more
through the ordinary wrapper as the bitwise witness.  Asserted: return code 0, every margin of every buffer
intact, inputs bit-identical, the results of all fills and the witness bit-identical, no NaN in any output, and
the result equal to the reference.  A size function that under-reports, or a kernel that writes one slot past
its partials, breaks a margin; a second stage that reads a slot the first did not fill, or a counter that is
not reset, turns a poison into a NaN or a different bit.  No case hands a launch less than the advertised size.

The reference is NumPy fp64 on integer data (values in {-3..3}, steps and scalars powers of two), every sum
exact, compared with `array_equal`; pcs_thresh_l1 keeps the exact oracle and the bound of
test_thresh_kernel_exact, the fused steps the oracle and the derived bound of tests/pointwise*.py.

Each case prints `SCRATCH <entry> ... bytes=<advertised> high=<high-water mark>` (DESIGN.md records them)."""

import ctypes

import numpy as np
import pytest
import torch

from tests import func_family_cases as FC
from tests import scratch as S
from tests import views as V

pytestmark = pytest.mark.gpu

DT = V.DTYPES
EPS64, EPS32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)


def gin(a, dtype):
    """A guarded device copy of an input and its snapshot."""
    v = V.guarded(np.asarray(a, dtype=dtype), 0, device='cuda')
    return v, v.clone()


def gout(n, dtype):
    return V.guarded_out(int(n), dtype, 0, device='cuda')


def plain(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _procedure(tag, sizes, fills, inputs, make_outs, call, witness):
    """`call(scratch views, outs) -> rc` once per fill on fresh outputs, then `witness() -> tensors`; the
    assertions of the module docstring but the reference.  `inputs`: (view, snapshot) pairs.  Returns the
    outputs (host arrays) of the first fill."""
    results, marks = [], []
    for fill in fills:
        sc = [S.scratch(nb, fill, 'cuda') for nb in sizes]
        outs = make_outs()
        rc = call(sc, outs)
        assert rc == 0, (tag, fill, rc)
        torch.cuda.synchronize()
        S.check(*sc)
        V.check_guards(*[v for v, _ in inputs], *outs)
        for i, (v, snap) in enumerate(inputs):
            assert V.same_bits(v, snap), f'{tag} {fill}: input {i} was modified'
        for i, o in enumerate(outs):
            assert not bool(torch.isnan(o).any()), f'{tag} {fill}: NaN in output {i} (unwritten, or scratch read ' \
                                                   f'before it was written)'
        marks.append([S.high_water(v, fill) for v in sc])
        results.append([o.clone() for o in outs])
    wit = witness()
    assert len(wit) == len(results[0])
    for fill, res in zip(fills, results):
        for i, (a, b) in enumerate(zip(res, wit)):
            assert V.same_bits(a.reshape(-1), b.reshape(-1)), f'{tag} {fill}: output {i} differs from the witness'
    print(f'SCRATCH {tag} bytes={list(map(int, sizes))} high={marks}')
    return [host(o) for o in results[0]]


def _ws_doubles(lib):
    """pcs_reduce_ws_bytes() in doubles; the cases below reach its last slot only while it is two per block of
    256 threads for at most n / 256 blocks."""
    nbytes = int(lib.pcs_reduce_ws_bytes())
    assert nbytes % 8 == 0
    return nbytes // 8


# ---------------------------------------------------------------- reductions

@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('n', S.RED_SIZES)
def test_reduce(n, dtype):
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    nws = _ws_doubles(lib)
    assert max(S.RED_SIZES) > S.RED_BLOCK * (nws // 2 - 1), 'the largest case fills every block the workspace serves'
    x, y = S.reduce_data(n)
    refs = S.reduce_ref(x, y)
    X, Y = gin(x, dtype), gin(y, dtype)
    for kind in range(4):
        yv = Y[0] if kind >= 2 else None
        got = _procedure(f'pcs_reduce kind={kind} n={n} {np.dtype(dtype).name}', [8 * nws], S.FILLS, [X, Y],
                         lambda: [gout(1, np.float64)],
                         lambda sc, outs: lib.pcs_reduce(L.dtcode(X[0]), kind, L.ptr(X[0]), L.ptr(yv), n,
                                                         L.ptr(outs[0]), L.ptr(sc[0]), L.stream()),
                         lambda: [O.reduce_dev(kind, X[0], yv)])
        assert got[0][0] == refs[kind], (kind, got[0][0], refs[kind])


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('n', S.REL_SIZES)
def test_rel_sums(n, dtype):
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    nws = _ws_doubles(lib)
    x, y = S.reduce_data(n)
    t = S.reduce_terms(x, y)
    X, Y = gin(x, dtype), gin(y, dtype)
    got = _procedure(f'pcs_rel_sums n={n} {np.dtype(dtype).name}', [8 * nws], S.FILLS, [X, Y],
                     lambda: [gout(2, np.float64)],
                     lambda sc, outs: lib.pcs_rel_sums(L.dtcode(X[0]), L.ptr(X[0]), L.ptr(Y[0]), n, L.ptr(outs[0]),
                                                       L.ptr(sc[0]), L.stream()),
                     lambda: [O.rel_sums(X[0], Y[0], torch.empty(2, dtype=torch.float64, device='cuda'))])
    assert got[0].tolist() == [float(np.sum(t[2])), float(np.sum(t[0]))]


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('gkind', S.GKINDS)
@pytest.mark.parametrize('n', S.RED_SIZES)
def test_apgd_step(n, gkind, dtype):
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    nws = _ws_doubles(lib)
    assert (L.PCS_G_NULL, L.PCS_G_NONNEG, L.PCS_G_SEGMENT, L.PCS_APGD_G_L1) == S.GKINDS
    x, g, aux = S.apgd_data(n)
    xn, w, t0, t1 = S.apgd_ref(x, g, aux, gkind)
    X, G, A = gin(x, dtype), gin(g, dtype), gin(aux, dtype)
    p = S.APGD
    got = _procedure(f'pcs_apgd_step gkind={gkind} n={n} {np.dtype(dtype).name}', [8 * nws], S.FILLS, [X, G, A],
                     lambda: [gout(n, dtype), gout(n, dtype), gout(2, np.float64)],
                     lambda sc, outs: lib.pcs_apgd_step(L.dtcode(X[0]), L.ptr(X[0]), L.ptr(G[0]), L.ptr(A[0]),
                                                        L.ptr(outs[0]), L.ptr(outs[1]), n, p['tau'], p['a'], gkind,
                                                        p['lam'], p['seg'][0], p['seg'][1], L.ptr(outs[2]),
                                                        L.ptr(sc[0]), L.stream()),
                     lambda: list(O.apgd_step(X[0], G[0], A[0], p['tau'], p['a'], gkind, p['lam'], p['seg'])))
    assert got[0].dtype == dtype and np.array_equal(got[0], xn) and np.array_equal(got[1], w)
    assert got[2].tolist() == [float(np.sum(t0)), float(np.sum(t1))]


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('K', (0, 2))
@pytest.mark.parametrize('n', S.RED_SIZES)
def test_mcmc_accumulate(n, K, dtype):
    """One retained sample: the moments and the two norms exactly; with K = 2 the first sample of two P-square
    states, against the host twin of the same element update (pcs_p2_update_host)."""
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    nws = _ws_doubles(lib)
    tdt = V.tdtype(dtype)
    x, s, sq = S.mcmc_data(n)
    s1, sq1, t0, t1 = S.mcmc_ref(x, s, sq)
    pvalues = (0.1, 0.9)[:K]
    des, _ = O.p2_desired(pvalues)
    des = np.ascontiguousarray(des if K else np.zeros((1, 5)))
    X = gin(x, dtype)
    hshape, pshape = (max(K, 1), 5, n), (max(K, 1), 3, n)

    def make_outs():
        return [V.guarded(s.astype(dtype), 0, device='cuda'), V.guarded(sq.astype(dtype), 0, device='cuda'),
                V.guarded(np.zeros(hshape, dtype), 0, device='cuda'), gout(2, np.float64)]

    pos = []

    def call(sc, outs):
        pos.append(torch.zeros(pshape, dtype=torch.int32, device='cuda'))
        return lib.pcs_mcmc_accumulate(L.dtcode(X[0]), L.ptr(X[0]), L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]),
                                       L.ptr(pos[-1]), n, K, 1, des.ctypes.data_as(L._pdbl), L.ptr(outs[3]),
                                       L.ptr(sc[0]), L.stream())

    def witness():
        st = O.P2State(pvalues, n, tdt)
        tot, tsq = plain(s, dtype), plain(sq, dtype)
        sums = torch.empty(2, dtype=torch.float64, device='cuda')
        O.mcmc_accumulate(X[0], tot, tsq, st, sums)
        pos.append(st.pos)
        return [tot, tsq, st.heights, sums]

    got = _procedure(f'pcs_mcmc_accumulate K={K} n={n} {np.dtype(dtype).name}', [8 * nws], S.FILLS, [X], make_outs,
                     call, witness)
    assert np.array_equal(got[0], s1) and np.array_equal(got[1], sq1)
    assert got[3].tolist() == [float(np.sum(t0)), float(np.sum(t1))]
    assert all(torch.equal(p, pos[-1]) for p in pos)
    if K:
        xh, hh = np.ascontiguousarray(x, dtype=dtype), np.zeros(hshape, dtype)
        ph = np.zeros(pshape, np.int32)
        assert lib.pcs_p2_update_host(L.dtype_code(tdt), xh.ctypes.data, hh.ctypes.data, ph.ctypes.data, n, K, 1,
                                      des.ctypes.data_as(L._pdbl)) == 0
        assert np.array_equal(got[2].view(np.uint8), hh.ravel().view(np.uint8))
        assert np.array_equal(host(pos[0]), ph)


# ---------------------------------------------------------------- proxes

THRESH_KINDS = ('quant', 'equal', 'mixed')    # ties; one value n times (the bracket closes on two adjacent
#                                              representable values around it); magnitudes over seven decades


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('kind', THRESH_KINDS)
@pytest.mark.parametrize('n', S.RED_SIZES)
def test_thresh_l1(n, kind, dtype):
    """Both modes and the b > 0 form on a workspace of pcs_thresh_ws_bytes(n) for that n, t_dev a one-double
    guarded scratch; the exact oracle and the bound of test_thresh_kernel_exact."""
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    nbytes = int(lib.pcs_thresh_ws_bytes(n))
    assert 0 < nbytes <= int(lib.pcs_thresh_ws_bytes(1 << 40)) and nbytes % 8 == 0
    assert nbytes >= int(lib.pcs_thresh_ws_bytes(max(n - 256, 0))), 'never decreases in n'
    x = FC.make_x(kind, n)
    X = gin(x, dtype)
    mx = float(np.abs(x).max())
    bound = 32 * EPS64 * mx if dtype == np.float64 else EPS32 * mx
    l1 = float(np.sum(np.abs(x)))
    forms = (('l1ball', 0.5 * l1, 0.0, 'soft'), ('linfty', 1.0, 0.0, 'clip'), ('sql1', 0.0, 0.5, 'soft'))
    for name, a, b, mode in forms:
        code = {'soft': L.PCS_THRESH_SOFT, 'clip': L.PCS_THRESH_CLIP}[mode]
        t, exact = FC.exact_prox(x, a, b, mode)

        def witness():
            t_out = torch.full((1,), -1.0, dtype=torch.float64, device='cuda')
            return [O.thresh_l1(X[0], a, b, mode, t_out), t_out]

        got = _procedure(f'pcs_thresh_l1 {name} {kind} n={n} {np.dtype(dtype).name}', [nbytes, 8], S.FILLS, [X],
                         lambda: [gout(n, dtype)],
                         lambda sc, outs: lib.pcs_thresh_l1(L.dtcode(X[0]), L.ptr(X[0]), L.ptr(outs[0]), n, a, b, code,
                                                            L.ptr(sc[1]), L.ptr(sc[0]), L.stream()),
                         lambda: witness()[:1])
        sc_t = S.scratch(8, 'poison_b', 'cuda')        # t itself, once more, into a guarded double
        out = gout(n, dtype)
        ws = S.scratch(nbytes, 'poison_a', 'cuda')
        assert lib.pcs_thresh_l1(L.dtcode(X[0]), L.ptr(X[0]), L.ptr(out), n, a, b, code, L.ptr(sc_t), L.ptr(ws),
                                 L.stream()) == 0
        torch.cuda.synchronize()
        S.check(sc_t, ws)
        wit = witness()
        assert V.same_bits(sc_t, wit[1]) and V.same_bits(out, wit[0])
        tg = float(sc_t.item())
        err, terr = float(np.max(np.abs(got[0].astype(np.float64) - exact))), abs(tg - float(t))
        print(f'  {name}: |out-exact|={err:.3e} |t-exact|={terr:.3e} bound={bound:.3e}')
        assert got[0].dtype == dtype and err <= bound and terr <= bound, (name, err, terr, bound)


CUMSUM_UNSPLIT = (((257,), 0), ((64, 5), 0))      # lines too short to split: pcs_cumsum_ws_bytes is 0, ws is NULL


def _cumsum_cases():
    from tests.test_gpu_diff_family import _exact_cases
    return _exact_cases() + list(CUMSUM_UNSPLIT)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('case', range(11))
def test_cumsum(case, dtype):
    """_exact_cases() of tests/test_gpu_diff_family.py: both layouts, split lines, forward and reverse, in place
    and out of place, on a workspace of exactly pcs_cumsum_ws_bytes -- NULL wherever that is 0, which the two
    unsplit shapes added here make sure happens."""
    from pycsou_amd import _lib as L, _ops as O
    from tests.test_gpu_diff_family import _int_data
    lib = L.gpu()
    cases = _cumsum_cases()
    assert len(cases) == 11
    shape, axis = cases[case]
    n = int(np.prod(shape))
    d = L.i64s(shape)
    nbytes = int(lib.pcs_cumsum_ws_bytes(len(shape), d, axis))
    assert 0 <= nbytes <= L.PCS_CUMSUM_WS_MAX and nbytes % 8 == 0
    assert (nbytes == 0) == (case >= 9), 'the split cases need a workspace, the unsplit ones none'
    x = _int_data(shape)
    X = gin(x, dtype)
    for reverse in (False, True):
        ref = S.cumsum_ref(x, shape, axis, 0.5, reverse).ravel()
        for in_place in (False, True):
            def call(sc, outs):
                if in_place:
                    outs[0].copy_(X[0])
                return lib.pcs_cumsum(L.dtcode(X[0]), L.ptr(outs[0] if in_place else X[0]), L.ptr(outs[0]), len(shape),
                                      d, axis, 0.5, int(reverse), L.ptr(sc[0]) if nbytes else None, L.stream())

            def witness():
                t = X[0].clone()
                return [O.cumsum(t, shape, axis, 0.5, reverse=reverse, out=t if in_place else None)]

            got = _procedure(f'pcs_cumsum {shape} axis={axis} rev={int(reverse)} inplace={int(in_place)} '
                             f'{np.dtype(dtype).name}', [nbytes], S.FILLS, [X], lambda: [gout(n, dtype)], call, witness)
            assert got[0].dtype == dtype and np.array_equal(got[0], ref), (shape, axis, reverse, in_place)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('reps', (1, 16))
@pytest.mark.parametrize('ngroups', S.L21_GROUPS)
def test_prox_l21(ngroups, reps, dtype):
    """pcs_prox_l21_labels and pcs_prox_l21_groups (one thread per group for groups of 3 elements, one wave per
    group for 48) on ws = ngroups doubles."""
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    x, gid = S.l21_case(ngroups, reps)
    n, tau = x.size, 2.0
    _, ref = S.l21_ref(x, gid, ngroups, tau, dtype)
    X = gin(x, dtype)
    gd = plain(gid, np.int32)
    order = np.argsort(gid, kind='stable').astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(gid, minlength=ngroups))]).astype(np.int64)
    maxlen = int(np.diff(off).max())
    assert maxlen == 3 * reps and (maxlen <= 32) == (reps == 1)
    od, fd = plain(order, np.int32), plain(off, np.int64)
    snaps = [t.clone() for t in (gd, od, fd)]
    got = _procedure(f'pcs_prox_l21_labels ngroups={ngroups} len={maxlen} {np.dtype(dtype).name}', [8 * ngroups],
                     S.FILLS, [X], lambda: [gout(n, dtype)],
                     lambda sc, outs: lib.pcs_prox_l21_labels(L.dtcode(X[0]), L.ptr(X[0]), L.ptr(outs[0]), n, L.ptr(gd),
                                                              ngroups, tau, L.ptr(sc[0]), L.stream()),
                     lambda: [O.prox_l21_labels(X[0], tau, gd, ngroups)])
    assert got[0].dtype == dtype and np.array_equal(got[0], ref)
    got = _procedure(f'pcs_prox_l21_groups ngroups={ngroups} len={maxlen} {np.dtype(dtype).name}', [8 * ngroups],
                     S.FILLS, [X], lambda: [gout(n, dtype)],
                     lambda sc, outs: lib.pcs_prox_l21_groups(L.dtcode(X[0]), L.ptr(X[0]), L.ptr(outs[0]), n, L.ptr(gd),
                                                              ngroups, L.ptr(od), L.ptr(fd), maxlen, tau, L.ptr(sc[0]),
                                                              L.stream()),
                     lambda: [O.prox_l21_groups(X[0], tau, gd, ngroups, od, fd, maxlen)])
    assert got[0].dtype == dtype and np.array_equal(got[0], ref)
    assert all(torch.equal(a, b) for a, b in zip((gd, od, fd), snaps))


# ---------------------------------------------------------------- sparse and Khatri-Rao

def _csr_args(D):
    from pycsou_amd import _lib as L
    return (D.shape[0], D.shape[1], D.nnz, L.ptr(D.rowptr), L.ptr(D.colind), L.ptr(D.vals))


def _chunk_args(D):
    from pycsou_amd import _lib as L
    return (D.nchunks, L.ptr(D.chunk_row), L.ptr(D.chunk_start), D.nlong, L.ptr(D.long_row), L.ptr(D.long_first))


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('name', tuple(S.SPMV_ROWS))
def test_csr_spmv(name, dtype):
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    A, x = S.spmv_case(name, O.SPMV_CHUNK, O.SPMV_LONG_ROW)
    D = O.DeviceCSR(A, V.tdtype(dtype))
    per_row = {'one_long': [2], 'three_long': [2, 3, 3], 'mixed': [2, 3, 3]}[name]
    assert D.nlong == len(per_row) and D.nchunks == sum(per_row)
    X = gin(x, dtype)
    got = _procedure(f'pcs_csr_spmv {name} {np.dtype(dtype).name}', [8 * D.nchunks], S.FILLS, [X],
                     lambda: [gout(A.shape[0], dtype)],
                     lambda sc, outs: lib.pcs_csr_spmv(L.dtcode(X[0]), *_csr_args(D), L.ptr(X[0]), L.ptr(outs[0]),
                                                       D.lanes, *_chunk_args(D), L.ptr(sc[0]), L.stream()),
                     lambda: [O.spmv(D, X[0])])
    assert got[0].dtype == dtype and np.array_equal(got[0], A @ x)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('accumulate', (0, 1))
@pytest.mark.parametrize('nb', (1, 3, 65))
@pytest.mark.parametrize('axis', (0, 1))
def test_csr_spmm(axis, nb, accumulate, dtype):
    """partials_len = nb * nchunks exactly (the header's size for the long rows of a batch; axis 0 with nb > 1
    walks the rows whole and must leave it alone)."""
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    A, _ = S.spmv_case('mixed', O.SPMV_CHUNK, O.SPMV_LONG_ROW)
    D = O.DeviceCSR(A, V.tdtype(dtype))
    nrows, ncols = A.shape
    Xb = np.stack([S.ints(ncols, 20 + b) for b in range(nb)])          # (nb, ncols)
    start = S.ints(nb * nrows, 30).reshape(nb, nrows)
    prod = (A @ Xb.T).T
    if axis == 0:
        Xh, start, prod = np.ascontiguousarray(Xb.T), np.ascontiguousarray(start.T), np.ascontiguousarray(prod.T)
    else:
        Xh = Xb
    ref = prod + start if accumulate else prod
    X = gin(Xh, dtype)
    plen = nb * D.nchunks
    assert O.spmm_plan(D, axis, nb)['partials'] in (plen, 0)

    def make_outs():
        return [V.guarded(start.astype(dtype), 0, device='cuda') if accumulate else gout(ref.size, dtype)]

    def witness():
        out = plain(start, dtype).reshape(ref.shape) if accumulate else None
        return [O.spmm(D, X[0].view(Xh.shape), axis, out=out, accumulate=bool(accumulate))]

    got = _procedure(f'pcs_csr_spmm axis={axis} nb={nb} acc={accumulate} {np.dtype(dtype).name}', [8 * plen], S.FILLS,
                     [X], make_outs,
                     lambda sc, outs: lib.pcs_csr_spmm(L.dtcode(X[0]), axis, accumulate, *_csr_args(D), L.ptr(X[0]),
                                                       L.ptr(outs[0]), nb, D.lanes, *_chunk_args(D), L.ptr(sc[0]), plen,
                                                       L.stream()),
                     witness)
    assert got[0].dtype == dtype and np.array_equal(got[0].reshape(ref.shape), ref)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('kn', S.KR_SHAPES, ids=['x'.join(map(str, s)) for s in S.KR_SHAPES])
def test_khatri_rao_fwd(kn, dtype):
    """partials_len = ngroups * n * k exactly, one slab per workgroup and all slabs in one workgroup, with
    (k, n) at the k n and at the k + n limit."""
    from pycsou_amd import _lib as L, _ops as O
    lib = L.gpu()
    assert (O.KR_SLAB, O.KR_MAX_NK, O.KR_MAX_ROWS) == (S.KR_SLAB, S.KR_MAX_NK, S.KR_MAX_ROWS)
    k, n = kn
    assert O.kr_fused_ok(k, n) and not O.kr_fused_ok(k + 1, n + 1)
    Ah, Bh, xh = S.kr_case(k, n)
    l = xh.size
    nslabs = -(-l // O.KR_SLAB)
    ref = S.kr_ref(Ah, Bh, xh)
    A, B, X = gin(Ah, dtype), gin(Bh, dtype), gin(xh, dtype)

    def witness():
        ws = torch.empty(O.kr_fwd_plan(k, n, l)[2], dtype=torch.float64, device='cuda')
        return [O.khatri_rao_fwd(A[0].view(k, l), B[0].view(n, l), X[0], ws)]

    for spg in (1, nslabs):
        ngroups = -(-nslabs // spg)
        assert ngroups <= O.KR_MAX_GROUPS
        plen = ngroups * n * k
        got = _procedure(f'pcs_khatri_rao_fwd k={k} n={n} l={l} spg={spg} {np.dtype(dtype).name}', [8 * plen], S.FILLS,
                         [A, B, X], lambda: [gout(n * k, dtype)],
                         lambda sc, outs: lib.pcs_khatri_rao_fwd(L.dtcode(X[0]), L.ptr(A[0]), L.ptr(B[0]), L.ptr(X[0]),
                                                                 L.ptr(outs[0]), k, n, l, spg, ngroups, L.ptr(sc[0]),
                                                                 plen, L.stream()),
                         witness)
        assert got[0].dtype == dtype and np.array_equal(got[0].reshape(n, k), ref)


# ---------------------------------------------------------------- fused steps

class Seam:
    """Stands in for pycsou_amd.opt._loop.loop_buffer, the one function through which the engines allocate what
    a loop lends to the kernels (control block, history, partials, reduction workspace): every buffer is a
    scratch view of exactly the size asked for, 16-byte aligned as the fused steps require, between sentinel
    margins.  What the engine asks to be filled gets that value; what it leaves uninitialised gets `poison`."""

    def __init__(self, poison):
        self.poison, self.views = poison, []

    def __call__(self, numel, device, fill=None):
        v = S.scratch(8 * int(numel), 'zero' if fill is not None else self.poison, device, align=16)
        if fill is not None and fill != 0.0:
            v.fill_(float(fill))
        self.views.append(v)
        return v

    def sizes(self):
        return sorted(v.numel() for v in self.views)

    def check(self):
        torch.cuda.synchronize()
        S.check(*self.views)


def _first_per(configs, key, prefer):
    """Index of one entry per distinct `key`, the first of the preferred shape where there is one."""
    out = {}
    for i, c in enumerate(configs):
        k = getattr(c, key)
        if k not in out or (configs[out[k]].shape != prefer and c.shape == prefer):
            out[k] = i
    return out


def _loop_sizes(eng, lib, nit, parts):
    """What a loop of max_iter = nit - 1 must have asked the seam for, in doubles: the control block, the
    placeholder history and the real one, the partials and the workspace."""
    ctrl = int(lib.pcs_ctrl_bytes())
    assert ctrl % 8 == 0
    return sorted([ctrl // 8, 2, 2 * nit + 2, parts, eng.ws.numel()])


def _run_seamed(tag, build, monkeypatch, check_first):
    """nit = 1 and 2 on seamed buffers with each poison, then without the seam: [(nit, poison, result)].
    `build(nit)` -> (engine, result tensors / arrays, sizes the seam must have seen); `check_first(nit, result)`
    runs the oracle comparison once per nit."""
    from pycsou_amd.opt import _loop
    plain_alloc = _loop.loop_buffer
    results = {}
    for poison in ('poison_a', 'poison_b', None):
        for nit in (1, 2):
            seam = Seam(poison)
            monkeypatch.setattr(_loop, 'loop_buffer', seam if poison else plain_alloc)
            eng, res, want = build(nit)
            if poison:
                seam.check()
                assert seam.sizes() == want, (nit, poison, seam.sizes(), want)
                assert eng.ws._base is not None and eng.partials._base is not None and eng.ctrl._base is not None
                marks = {n: S.high_water(getattr(eng, n), 'zero' if n in ('ws', 'ctrl') else poison)
                         for n in ('partials', 'ws', 'ctrl')}
                print(f'SCRATCH fused {tag} nit={nit} {poison} doubles={want} high={marks}')
            if poison == 'poison_a':
                check_first(nit, res)
            results[nit, poison] = res
    monkeypatch.setattr(_loop, 'loop_buffer', plain_alloc)
    for nit in (1, 2):
        ref = results[nit, None]
        for poison in ('poison_a', 'poison_b'):
            for k, (a, b) in enumerate(zip(results[nit, poison], ref)):
                a, b = np.asarray(a), np.asarray(b)
                assert not np.isnan(a).any(), (nit, poison, k)
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (nit, poison, k)


def _paths2d():
    from tests import pointwise as PW
    return _first_per(PW.CONFIGS, 'path', PW.A)


@pytest.mark.parametrize('path', ['NMARCH', 'SMARCH_NX', 'MARCH', 'PT', 'SMARCH', 'NM64', 'TILE', 'stencil_tile'])
def test_fused2d_steps(path, monkeypatch):
    """One entry per distinct kernel path of pointwise.CONFIGS: one and two iterations against the oracle with
    partials = 4 nblocks poisoned doubles (two such arrays of the run's count with deferred finalization),
    ws = *_ws_bytes() zeroed, ctrl = pcs_ctrl_bytes(), hist = 2 (max_iter + 1) + 2."""
    from pycsou_amd import _lib as L
    from tests import pointwise as PW
    from tests.test_gpu_step_pointwise import _check, _check_route
    paths = _paths2d()
    assert sorted(paths) == sorted({c.path for c in PW.CONFIGS}), 'a new path needs a case here'
    ik = (paths[path], 0)
    c, p = PW.case_problem(ik)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    lib = L.gpu()

    def build(nit):
        s = PW.build_solver(p, nit, c.engine)
        est, _, diag = s.iterate()
        eng = s._engine
        assert eng is not None, 'the fused engine must take this problem'
        _check_route(c, p, eng)
        a = eng.args
        march = isinstance(a, L.PdsArgs)
        nb = int((lib.pcs_pds2d_nblocks if march else lib.pcs_pds2d_stencil_nblocks)(ctypes.byref(a)))
        wsb = int((lib.pcs_pds2d_ws_bytes if march else lib.pcs_pds2d_stencil_ws_bytes)(ctypes.byref(a)))
        assert nb == eng.nblocks and wsb == 8 * eng.ws.numel() and s.iter == nit
        parts = 4 * nb
        if eng.defer:   # two arrays, each of the largest count a PCS_RUN_BANDS setting can ask of pcs_pds2d_run
            parts = 8 * max(nb, *(int(lib.pcs_pds2d_run_nblocks(ctypes.byref(a), m)) for m in (-1, 1)))
        res = [est['primal_variable'], est['dual_variable'], diag[PW.P_COL].to_numpy(float),
               diag[PW.D_COL].to_numpy(float)]
        return eng, res, _loop_sizes(eng, lib, nit, parts)

    def check_first(nit, res):
        s = PW.build_solver(p, nit, c.engine)      # _check wants the solver's iteration count and the frames
        est, _, diag = s.iterate()
        assert np.array_equal(est['primal_variable'], res[0])
        _check(f'scratch-{PW.case_id(ik)}', p, nit, s, est, diag)

    _run_seamed(PW.case_id(ik), build, monkeypatch, check_first)


@pytest.mark.parametrize('route', ['fold', 'ata', 'sep2', 'conv1d', 'generic', 'denoise', 'null'])
def test_fused3d_steps(route, monkeypatch):
    """One entry per route of pointwise3d.ROUTES, as test_fused2d_steps."""
    from pycsou_amd import _lib as L
    from tests import pointwise3d as PW
    from tests.test_gpu_step_pointwise3d import _check, _check_route, _oracle
    routes = _first_per(PW.CONFIGS, 'route', PW.VA)
    assert sorted(routes) == sorted(PW.ROUTES)
    ik = (routes[route], 0)
    c, p = PW.case_problem(ik)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    lib = L.gpu()
    ref = _oracle(p)

    def build(nit):
        s = PW.build_solver(p, nit)
        est, _, diag = s.iterate()
        eng = s._engine
        assert eng is not None, 'the fused engine must take this problem'
        _check_route(c, p, eng)
        a = eng.args[0]
        nb, wsb = int(lib.pcs_pds3d_nblocks(ctypes.byref(a))), int(lib.pcs_pds3d_ws_bytes(ctypes.byref(a)))
        assert nb == eng.nblocks and wsb == 8 * eng.ws.numel() and s.iter == nit
        res = [est['primal_variable'], est['dual_variable'], diag[PW.P_COL].to_numpy(float),
               diag[PW.D_COL].to_numpy(float)]
        return eng, res, _loop_sizes(eng, lib, nit, 4 * nb)

    def check_first(nit, res):
        _check(f'scratch-{PW.case_id(ik)}', p, nit, ref[nit], nit, res[0], res[1], {'primal': res[2], 'dual': res[3]})

    _run_seamed(PW.case_id(ik), build, monkeypatch, check_first)


def _apgd_cases():
    from tests import pointwise_apgd as PA
    return [i for i in PA.MATRIX if PA.CASES[i].shape == (150, 200)]


@pytest.mark.parametrize('j', range(7))
def test_fused_apgd_steps(j, monkeypatch):
    """The APGD engine's cases at 150 x 200 (both dtypes, every G kind, tau != 1): one and two iterations of
    the public API from x0 = x against the oracle, on seamed buffers."""
    from pycsou_amd import _lib as L
    from pycsou_amd.opt.engine import APGD2DEngine
    from tests import pointwise_apgd as PA
    cases = _apgd_cases()
    assert len(cases) == 7
    i = cases[j]
    c, p = PA.case_problem(i)
    lib = L.gpu()
    refs = [PA.oracle_api(p, 'CD', 2.0, nit) for nit in (1, 2)]
    coeffs, _ = PA.ref_coeffs('CD', 2.0, 2)
    states = [(p['x'], np.zeros(p['N']), coeffs[0]), (refs[0][0], refs[0][1], coeffs[1])]

    def build(nit):
        s = PA.build_solver(p, nit, acc='CD', d=2.0)
        est, conv, diag = s.iterate()
        eng = s._engine
        assert type(eng) is APGD2DEngine and eng.args.half == p['half'], 'the fused engine must take this problem'
        nb = int(lib.pcs_apgd2d_nblocks(ctypes.byref(eng.args)))
        assert nb == eng.nblocks == int(np.prod(PA.geometry(c))) and s.iter == nit
        assert int(lib.pcs_apgd2d_ws_bytes(ctypes.byref(eng.args))) == 8 * eng.ws.numel()
        res = [est['iterand'], est['past_aux'], diag[PA.H_COL].to_numpy(float)]
        return eng, res, _loop_sizes(eng, lib, nit, 4 * nb)

    def check_first(nit, res):
        xr, auxr, _, hr = refs[nit - 1]
        b = PA.bound(p, states[:nit])
        rx = PA.compare(res[0], xr, b['x'], c.shape, 'x', hist=res[2], hist_ref=hr, dtype=p['dtype'])
        ra = PA.compare(res[1], auxr, b['aux'], c.shape, 'aux')
        print(f'POINTWISE scratch-apgd-{PA.case_id(i)} nit={nit} x={rx:.2f} aux={ra:.2f}')

    _run_seamed('apgd-' + PA.case_id(i), build, monkeypatch, check_first)


# ---------------------------------------------------------------- the run loops, on the test's own buffers

STOPS = {'fixed': (2, 2, 0.0, 4, 3),         # max_iter, min_iter, threshold, launches, iterations: hist full
         'natural': (20, 3, 1e30, 8, 4)}     # the threshold is met from the start: stops once past min_iter


def _clone_args(a):
    b = type(a)()
    ctypes.memmove(ctypes.byref(b), ctypes.byref(a), ctypes.sizeof(a))
    return b


def _state(values, dtype, n):
    """[start, other parity]: guarded views, the other parity NaN_B."""
    return [V.guarded(values.astype(dtype), 0, device='cuda'), V.guarded_out(n, dtype, 0, device='cuda')]


def _run_direct(tag, lib, a, stop, poison, nparts, nws, has_dual, states, bind, launch, pending=None, ws=None):
    """One loop on scratch of the advertised sizes: `nparts` partials arrays of their doubles (poisoned), the
    control block (poisoned before pcs_ctrl_init2), hist = 2 (max_iter + 1) + 2 doubles with hist_len exactly
    that (poisoned), ws (zeroed; or the one handed in, as the last run left it).  `bind(a, states, parts)` sets
    the pointers, `launch(a, n)` runs n launches, `pending(parts, n)` finalizes what a deferring run left.
    Returns (iterations, the iterate's tensors, history rows, ws)."""
    from pycsou_amd import _lib as L
    max_iter, min_iter, thr, n, want_it = STOPS[stop]
    parts = [S.scratch(8 * d, poison, 'cuda', align=16) for d in nparts]
    ctrl = S.scratch(int(lib.pcs_ctrl_bytes()), poison, 'cuda')
    hist = S.scratch(8 * (2 * (max(max_iter, min_iter) + 1) + 2), poison, 'cuda')
    ws = S.scratch(nws, 'zero', 'cuda', align=16) if ws is None else ws
    bind(a, states, parts)
    a.ctrl, a.hist, a.ws = ctrl.data_ptr(), hist.data_ptr(), ws.data_ptr()
    assert lib.pcs_ctrl_init2(L.ptr(ctrl), min_iter, max_iter, thr, has_dual, hist.numel(), L.stream()) == 0
    assert launch(a, n) == 0
    if pending is not None:
        assert pending(parts, n, ctrl, hist) == 0
    torch.cuda.synchronize()
    S.check(*parts, ctrl, hist, ws)
    V.check_guards(*[t for pair in states for t in pair])
    it, stopped = ctrl.view(torch.int32)[:2].tolist()
    assert (it, stopped) == (want_it, 1), (stop, it, stopped)
    rows = hist[:2 * it].clone()
    assert not bool(torch.isnan(rows).any())
    assert S.words_changed(hist, poison).tolist() == [True] * (2 * it) + [False] * (hist.numel() - 2 * it), \
        'rows 0 .. it - 1 and nothing else'
    if stop == 'fixed':
        assert 2 * it + 2 == hist.numel(), 'the fixed count fills hist to its last row'
    print(f'SCRATCH run {tag} {stop} {poison} doubles parts={nparts} ws={nws // 8} high parts='
          f'{[S.high_water(v, poison) for v in parts]} ws={S.high_water(ws, "zero")}')
    return it, [pair[it % 2].clone() for pair in states], rows, ws


def _three_runs(run, witness):
    """A run on fresh buffers, a second one from the same start on the same, un-rezeroed ws with the other
    poison, and one on a freshly zeroed ws: bit for bit each other and the engine's own loop, diagnostics
    included."""
    it1, out1, rows1, ws = run('poison_a', None)
    it2, out2, rows2, _ = run('poison_b', ws)
    it3, out3, rows3, _ = run('poison_b', None)
    itw, outw, rowsw = witness()
    for it, out, rows in ((it2, out2, rows2), (it3, out3, rows3), (itw, outw, rowsw)):
        assert it == it1
        assert V.same_bits(rows.reshape(-1), rows1.reshape(-1)), 'diagnostics differ'
        for k, (a, b) in enumerate(zip(out, out1)):
            assert not bool(torch.isnan(a).any()) and V.same_bits(a.reshape(-1), b.reshape(-1)), k
    return out1, rows1


def _native(monkeypatch, bands=None):
    import pycsou_amd.opt.engine as E
    monkeypatch.setattr(E, 'NATIVE_MIN_PIXELS', 1)
    monkeypatch.setattr(E, 'DEFER_FIN', True)
    if bands is not None:
        monkeypatch.setenv('PCS_RUN_BANDS', str(bands))


@pytest.mark.parametrize('stop', list(STOPS))
@pytest.mark.parametrize('bands', [0, 1])
def test_pds2d_run(bands, stop, monkeypatch):
    """pcs_pds2d_run on the forward normal-operator march with deferred finalization: both partials arrays of
    4 pcs_pds2d_run_nblocks doubles, single launch per iteration and the band-paired schedule."""
    from pycsou_amd import _lib as L
    from tests import pointwise as PW
    from tests.test_gpu_step_pointwise import _check
    _native(monkeypatch, bands)
    lib = L.gpu()
    p = PW.make_problem(PW.A, 'forward', 'l21', 'sep15', 'segment', lam=PW.LAM, seed=77, dtype=np.float32)
    s = PW.build_solver(p, 3, 'fused')
    est, _, diag = s.iterate()
    eng = s._engine
    assert eng is not None and eng.native and eng.defer and PW.engine_path(eng) == L.PCS_PATH_NMARCH
    plan = (ctypes.c_int64 * 6)()
    assert lib.pcs_pds2d_run_plan(ctypes.byref(eng.args), -1, 0, plan) == 0 and int(plan[0]) == bands
    nb = int(lib.pcs_pds2d_run_nblocks(ctypes.byref(eng.args), -1))
    assert nb == (int(plan[2]) + int(plan[3]) if bands else eng.nblocks)
    nws = int(lib.pcs_pds2d_ws_bytes(ctypes.byref(eng.args)))
    x0, z0 = p['x0'], p['z0']

    def bind(a, st, parts):
        (X, Z) = st
        a.x, a.xn, a.z, a.zn = X[0].data_ptr(), X[1].data_ptr(), Z[0].data_ptr(), Z[1].data_ptr()
        a.partials, a.fin_partials = parts[0].data_ptr(), parts[1].data_ptr()

    def run(poison, ws):
        st = [_state(x0, np.float32, x0.size), _state(z0, np.float32, z0.size)]
        return _run_direct(f'pcs_pds2d_run bands={bands}', lib, _clone_args(eng.args), stop, poison, [4 * nb, 4 * nb],
                           nws, 1, st, bind,
                           lambda a, n: lib.pcs_pds2d_run(ctypes.byref(a), n, L.stream()),
                           lambda parts, n, ctrl, hist: lib.pcs_pds_finalize_pending(
                               L.ptr(parts[(n - 1) % 2]), nb, L.ptr(ctrl), L.ptr(hist), L.stream()), ws)

    def witness():
        eng.X[0].copy_(plain(x0, np.float32))
        eng.Z[0].copy_(plain(z0, np.float32))
        n, x, z, rows = eng.run(*STOPS[stop][:3])
        return n, [x.clone(), z.clone()], torch.as_tensor(np.ascontiguousarray(rows)).cuda()

    (x, z), rows = _three_runs(run, witness)
    if stop == 'fixed':     # the three iterations of the public API above, which the oracle checks
        assert np.array_equal(host(x), est['primal_variable']) and np.array_equal(host(z), est['dual_variable'])
        assert np.array_equal(host(rows)[0::2], diag[PW.P_COL].to_numpy(float))
        _check(f'scratch-run-bands{bands}', p, 3, s, est, diag)


@pytest.mark.parametrize('stop', list(STOPS))
def test_pds2d_stencil_run(stop, monkeypatch):
    """pcs_pds2d_stencil_run (the general-stencil tile kernel: in-launch reduction, counters in ws)."""
    from pycsou_amd import _lib as L
    from tests import pointwise as PW
    from tests.test_gpu_step_pointwise import _check
    _native(monkeypatch)
    monkeypatch.setenv('PCS_STENCIL_MARCH', '0')
    lib = L.gpu()
    p = PW.make_problem(PW.A, 'centered', 'l21', 'denoise', 'segment', lam=PW.LAM, seed=78, dtype=np.float32)
    s = PW.build_solver(p, 3, 'stencil')
    est, _, diag = s.iterate()
    eng = s._engine
    assert eng is not None and PW.engine_path(eng) == 'stencil_tile' and eng.native and not eng.defer
    nb = int(lib.pcs_pds2d_stencil_nblocks(ctypes.byref(eng.args)))
    nws = int(lib.pcs_pds2d_stencil_ws_bytes(ctypes.byref(eng.args)))
    assert nb == eng.nblocks and nb > 1
    x0, z0 = p['x0'], p['z0']

    def bind(a, st, parts):
        (X, Z) = st
        a.x, a.xn, a.z, a.zn = X[0].data_ptr(), X[1].data_ptr(), Z[0].data_ptr(), Z[1].data_ptr()
        a.partials = parts[0].data_ptr()

    def run(poison, ws):
        st = [_state(x0, np.float32, x0.size), _state(z0, np.float32, z0.size)]
        return _run_direct('pcs_pds2d_stencil_run', lib, _clone_args(eng.args), stop, poison, [4 * nb], nws, 1, st,
                           bind,
                           lambda a, n: lib.pcs_pds2d_stencil_run(ctypes.byref(a), n, L.stream()), None, ws)

    def witness():
        eng.X[0].copy_(plain(x0, np.float32))
        eng.Z[0].copy_(plain(z0, np.float32))
        n, x, z, rows = eng.run(*STOPS[stop][:3])
        return n, [x.clone(), z.clone()], torch.as_tensor(np.ascontiguousarray(rows)).cuda()

    (x, z), rows = _three_runs(run, witness)
    if stop == 'fixed':
        assert np.array_equal(host(x), est['primal_variable']) and np.array_equal(host(z), est['dual_variable'])
        _check('scratch-stencil-run', p, 3, s, est, diag)


@pytest.mark.parametrize('stop', list(STOPS))
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_apgd2d_run(dt, stop):
    """pcs_apgd2d_run at 150 x 200 (has_dual = 0: the dual column of hist reads inf)."""
    from pycsou_amd import _lib as L
    from pycsou_amd.opt.engine import APGD2DEngine
    from tests import pointwise_apgd as PA
    lib = L.gpu()
    i = [k for k in _apgd_cases() if PA.CASES[k].dtype == dt][0]
    c, p = PA.case_problem(i)
    dtype = PA.np_dtype(c)
    s = PA.build_solver(p, 3, acc='CD', d=2.0)
    est, _, diag = s.iterate()
    eng = s._engine
    assert type(eng) is APGD2DEngine, 'the fused engine must take this problem'
    nb, nws = int(lib.pcs_apgd2d_nblocks(ctypes.byref(eng.args))), int(lib.pcs_apgd2d_ws_bytes(ctypes.byref(eng.args)))
    assert nb == eng.nblocks == int(np.prod(PA.geometry(c)))
    launches = STOPS[stop][3]
    coeffs = eng.coeffs(0, launches, 1)[0]

    def bind(a, st, parts):
        (X, A) = st
        a.x, a.xn, a.aux, a.aux_n = X[0].data_ptr(), X[1].data_ptr(), A[0].data_ptr(), A[1].data_ptr()
        a.partials = parts[0].data_ptr()

    def run(poison, ws):
        st = [_state(p['x'], dtype, p['N']), _state(np.zeros(p['N']), dtype, p['N'])]
        return _run_direct(f'pcs_apgd2d_run {dt}', lib, _clone_args(eng.args), stop, poison, [4 * nb], nws, 0, st, bind,
                           lambda a, n: lib.pcs_apgd2d_run(ctypes.byref(a), L.dbls(coeffs), n, L.stream()), None, ws)

    def witness():
        n, x, aux, _, _ = eng.run(*STOPS[stop][:3])
        rows = eng.ctl.hist[:2 * n].clone()
        return n, [x.clone(), aux.clone()], rows

    (x, aux), rows = _three_runs(run, witness)
    assert bool(torch.isinf(rows[1::2]).all())
    if stop == 'fixed':     # the three iterations of the public API, against the oracle
        assert np.array_equal(host(x), est['iterand']) and np.array_equal(host(aux), est['past_aux'])
        xr, auxr, _, hr = PA.oracle_api(p, 'CD', 2.0, 3)
        r1, r2 = PA.oracle_api(p, 'CD', 2.0, 1), PA.oracle_api(p, 'CD', 2.0, 2)
        co, _ = PA.ref_coeffs('CD', 2.0, 3)
        b = PA.bound(p, [(p['x'], np.zeros(p['N']), co[0]), (r1[0], r1[1], co[1]), (r2[0], r2[1], co[2])])
        PA.compare(host(x), xr, b['x'], c.shape, 'x', hist=host(rows)[0::2], hist_ref=hr, dtype=p['dtype'])
        PA.compare(host(aux), auxr, b['aux'], c.shape, 'aux')
