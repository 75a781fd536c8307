"""Operators and proxes on views at arbitrary element offsets, inside sentinel margins (helpers, the bound and
the case matrix: tests/views.py; what they rely on, shown without a GPU: tests/test_views_cpu.py).

A  the entry points whose dispatcher picks a kernel form from the alignment of the base pointers, through the
   C ABI, each of x / out / b misaligned alone and all together: element by element against the fp64 reference
   within the derived bound, no NaN, all margins intact, inputs bit-identical, every output element written.
B  the operators and proxes whose kernels are scalar: bit-identical to the same call on an aligned clone.
C  LinOpVStack / LinOpHStack / BlockDiagonalOperator / BlockOperator / ProxFuncHStack / DiffFuncHStack whose
   first block has 5 or 37 elements, so the later blocks (a tier-15 Convolve2D, a Convolve1D, the FFT
   Convolve2D, a Gradient) receive the misaligned slices the classes cut.
D  the generic PDS loop on such a stack: hipGraph chunks == eager bit for bit, and against the oracle.
"""

import numpy as np
import pytest
import torch

from oracle import pycsou_ref as OR
from tests import views as V

pytestmark = pytest.mark.gpu

DT = V.DTYPES


def dev_in(a, off, dtype):
    return V.assert_misaligned(V.guarded(np.asarray(a, dtype=dtype), off, device='cuda'), off)


def dev_out(n, off, dtype):
    return V.assert_misaligned(V.guarded_out(n, dtype, off, device='cuda'), off)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


class _Bufs:
    """Guarded device copies of one array per offset (the inputs are shared by the calls of a case: every call
    checks that they are unchanged), and their aligned snapshots."""

    def __init__(self, a, dtype):
        self.a, self.dtype, self.v, self.s = a, dtype, {}, {}

    def at(self, off):
        if off not in self.v:
            self.v[off] = dev_in(self.a, off, self.dtype)
            self.s[off] = self.v[off].clone()
        return self.v[off], self.s[off]


def _run_combos(entry, dtype, x, b, call, refs, bnds):
    """`call(xv, outv, bv)` for every combination of offsets; `refs` / `bnds`: without and with b."""
    n = x.size
    X, B = _Bufs(x, dtype), _Bufs(b, dtype)
    for with_b in (False, True) if b is not None else (False,):
        for (ox, oo, ob), rec in V.combos(dtype, with_b):
            xv, xs = X.at(ox)
            out = dev_out(n, oo, dtype)
            ins, snaps = [xv], [xs]
            bv = None
            if with_b:
                bv, bs = B.at(ob)
                ins.append(bv)
                snaps.append(bs)
            rc = call(xv, out, bv)
            assert rc == 0, (entry, rc, (ox, oo, ob))
            torch.cuda.synchronize()
            V.check_call(out, ins, snaps, [out])
            r = V.compare(host(out), refs[with_b], bnds[with_b], f'{entry} offsets x/out/b = {(ox, oo, ob)}')
            V.record(entry, dtype, rec, r)


# ---------------------------------------------------------------- A. alignment-dependent dispatch, C ABI

@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('shape', V.SHAPES2D)
@pytest.mark.parametrize('k', V.TIERS)
def test_conv2d_planned_views(dtype, shape, k):
    from pycsou_amd import _lib as L
    from pycsou_amd import _ops as O
    lib, c = L.gpu(), k // 2
    x, b, h = V.data2d(shape, (k, k), dtype)
    for adjoint in (False, True):
        tier, w = O.conv2d_plan(h, c, c, adjoint, V.tdtype(dtype))
        assert tier == k and w.data_ptr() % 16 == 0
        ref = V.conv2d_np(x, h, c, c, adjoint=adjoint)

        def call(xv, out, bv):
            return lib.pcs_conv2d_planned(L.dtcode(xv), L.ptr(xv), L.ptr(out), shape[0], shape[1], L.ptr(w), tier,
                                          L.ptr(bv), -1.0 if bv is not None else 0.0, L.stream())
        _run_combos('pcs_conv2d_planned', dtype, x, b, call, {False: ref, True: ref - b},
                    {False: V.conv_bound(h, x, dtype), True: V.conv_bound(h, x, dtype, b, -1.0)})


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('shape', V.SHAPES2D)
@pytest.mark.parametrize('ks', V.PSF_GENERIC)
def test_conv2d_generic_views(dtype, shape, ks):
    from pycsou_amd import _lib as L
    lib = L.gpu()
    off = tuple(V.pycsou_offset(n) for n in ks)
    x, b, h = V.data2d(shape, ks, dtype)
    hd = torch.as_tensor(h.astype(dtype)).cuda()
    ref = V.conv2d_np(x, h, *off)

    def call(xv, out, bv):
        return lib.pcs_conv2d(L.dtcode(xv), L.ptr(xv), L.ptr(out), shape[0], shape[1], L.ptr(hd), ks[0], ks[1], off[0],
                              off[1], L.ptr(bv), -1.0 if bv is not None else 0.0, L.stream())
    _run_combos('pcs_conv2d', dtype, x, b, call, {False: ref, True: ref - b},
                {False: V.conv_bound(h, x, dtype), True: V.conv_bound(h, x, dtype, b, -1.0)})


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('dims,axis', V.CONV1D_CASES)
@pytest.mark.parametrize('k', V.CONV1D_K)
def test_conv1d_views(dtype, dims, axis, k):
    from pycsou_amd import _lib as L
    lib, off = L.gpu(), V.pycsou_offset(k)
    x, h = V.data1d(dims, k, dtype)
    hd = torch.as_tensor(h.astype(dtype)).cuda()
    ref = V.conv1d_np(x, h, off, axis)

    def call(xv, out, bv):
        return lib.pcs_conv1d(L.dtcode(xv), L.ptr(xv), L.ptr(out), len(dims), L.i64s(dims), axis, L.ptr(hd), k, off,
                              L.stream())
    _run_combos('pcs_conv1d', dtype, x, None, call, {False: ref}, {False: V.conv_bound(h, x, dtype)})


@pytest.mark.parametrize('dtype', DT)
def test_fftconv2d_views(dtype):
    """pcs_fftconv2d_apply (pad and crop kernels around rocFFT) through FFTConv2D.apply(out=...): forward, adjoint
    and the residual form, at the relative bars of tests/test_gpu_fftconv.py."""
    from pycsou_amd.linop.conv import Convolve2D
    shape, N = V.FFT_SHAPE, V.FFT_SHAPE[0] * V.FFT_SHAPE[1]
    h = V.rounded(V.fft_psf(), dtype)
    op = Convolve2D(N, h, shape)
    assert op.plan(V.tdtype(dtype), False) is None, 'PSF wider than the direct tiers: the FFT path'
    f = op.fft(V.tdtype(dtype))
    rng = np.random.default_rng(2)
    x, b = V.rounded(rng.standard_normal(shape), dtype), V.rounded(rng.standard_normal(shape), dtype)
    X, B = _Bufs(x, dtype), _Bufs(b, dtype)
    for adjoint, with_b in ((False, False), (True, False), (False, True)):
        ref = V.conv2d_np(x, h, 16, 16, adjoint=adjoint) - (b if with_b else 0.0)
        for (ox, oo, ob), rec in V.combos(dtype, with_b):
            (xv, xs), out = X.at(ox), dev_out(N, oo, dtype)
            ins, snaps, kw = [xv], [xs], {}
            if with_b:
                bv, bs = B.at(ob)
                ins.append(bv)
                snaps.append(bs)
                kw = {'b': bv, 'beta': -1.0}
            got = f.apply(xv, adjoint=adjoint, out=out, **kw)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr()
            V.check_call(out, ins, snaps, [out])
            r = V.rel_l2(host(out), ref)
            assert r < V.FFT_TOL[dtype], (r, adjoint, with_b, (ox, oo, ob))
            V.record('pcs_fftconv2d_apply (relative L2 / bar)', dtype, rec, r / V.FFT_TOL[dtype])


@pytest.mark.parametrize('entry', ['pcs_conv2d_sep_planes', 'pcs_conv2d_sep_ata_planes'])
@pytest.mark.parametrize('which', ['in', 'out'])
def test_sep_entry_points_refuse_misaligned(entry, which):
    """Both return PCS_EINVAL (-1) on a misaligned pointer by design, before any launch: the output is untouched."""
    from pycsou_amd import _lib as L
    lib, dims, dtype = L.gpu(), (2, 17, 36), np.float32
    x = np.random.default_rng(0).standard_normal(dims)
    xv = dev_in(x, 1 if which == 'in' else 0, dtype)
    out = dev_out(x.size, 1 if which == 'out' else 0, dtype)
    h = torch.as_tensor(np.random.default_rng(1).standard_normal(15).astype(dtype)).cuda()
    args = (L.PCS_F32, L.ptr(xv), L.ptr(out), dims[0], dims[1], dims[2], L.ptr(h), 15, 7, L.ptr(h), 15, 7)
    rc = lib.pcs_conv2d_sep_planes(*args, 1, L.stream()) if entry == 'pcs_conv2d_sep_planes' else \
        lib.pcs_conv2d_sep_ata_planes(*args, L.stream())
    torch.cuda.synchronize()
    assert rc == -1
    assert V.unwritten(out) == out.numel()
    V.check_guards(xv, out)
    # the aligned call of the same arguments succeeds
    xa, oa = dev_in(x, 0, dtype), dev_out(x.size, 0, dtype)
    args = (L.PCS_F32, L.ptr(xa), L.ptr(oa), dims[0], dims[1], dims[2], L.ptr(h), 15, 7, L.ptr(h), 15, 7)
    rc = lib.pcs_conv2d_sep_planes(*args, 1, L.stream()) if entry == 'pcs_conv2d_sep_planes' else \
        lib.pcs_conv2d_sep_ata_planes(*args, L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and V.unwritten(oa) == 0
    V.check_guards(xa, oa)


# ---------------------------------------------------------------- B. scalar kernels: bitwise against the aligned call

def _long_row_csr():
    import scipy.sparse as sp
    from pycsou_amd import _ops as O
    m = sp.random(23, O.SPMV_LONG_ROW + 300, density=0.01, random_state=3, format='lil')
    m[7, :] = np.random.default_rng(3).standard_normal(O.SPMV_LONG_ROW + 300)   # one row above the chunking limit
    return m.tocsr()


def _operators():
    import scipy.sparse as sp
    from pycsou_amd import linop as Lo
    rng = np.random.default_rng(21)
    ops = {}
    for kind in ('forward', 'backward', 'centered'):
        ops[f'Gradient-{kind}'] = Lo.Gradient((33, 20), kind=kind)
    ops['FirstDerivative'] = Lo.FirstDerivative(257, kind='centered')
    ops['SecondDerivative'] = Lo.SecondDerivative(210, shape=(5, 6, 7), axis=1)
    ops['Laplacian'] = Lo.Laplacian((33, 20), weights=(1.0, 0.5), step=(1.0, 2.0))
    ops['FirstDirectionalDerivative'] = Lo.FirstDirectionalDerivative((33, 20), [0.6, 0.8])
    ops['SecondDirectionalDerivative'] = Lo.SecondDirectionalDerivative((33, 20), [0.6, 0.8])
    ops['Integration1D-contiguous'] = Lo.Integration1D(210, shape=(5, 6, 7), axis=2, step=0.5)
    ops['Integration1D-strided'] = Lo.Integration1D(210, shape=(5, 6, 7), axis=0, step=0.5)
    ops['Pooling'] = Lo.Pooling((33, 20), (4, 3), pooling_func='mean')
    ops['SubSampling'] = Lo.SubSampling(257, rng.permutation(257)[:90])
    ops['Masking'] = Lo.Masking(257, rng.random(257) < 0.4)
    grid = np.stack(np.meshgrid(np.arange(33.0), np.arange(20.0), indexing='ij'), axis=-1).reshape(-1, 2)
    ops['NNSampling'] = Lo.NNSampling(rng.uniform(0, 19, (257, 2)), grid)
    ops['DiagonalOperator'] = Lo.DiagonalOperator(rng.standard_normal(257))
    ops['SparseLinearOperator'] = Lo.SparseLinearOperator(_long_row_csr())
    sa, sb = sp.random(6, 7, density=0.5, random_state=1, format='csr'), sp.random(5, 4, density=0.6, random_state=2,
                                                                                 format='csr')
    ops['KroneckerProduct'] = Lo.KroneckerProduct(Lo.SparseLinearOperator(sa), Lo.SparseLinearOperator(sb))
    qa, qb = sp.random(7, 7, density=0.5, random_state=4, format='csr'), sp.random(37, 37, density=0.2, random_state=5,
                                                                                 format='csr')
    ops['KroneckerSum'] = Lo.KroneckerSum(Lo.SparseLinearOperator(qa), Lo.SparseLinearOperator(qb))
    ops['KhatriRaoProduct'] = Lo.KhatriRaoProduct(Lo.DenseLinearOperator(rng.standard_normal((6, 257))),
                                                   Lo.DenseLinearOperator(rng.standard_normal((5, 257))))
    return ops


OPERATORS = ['Gradient-forward', 'Gradient-backward', 'Gradient-centered', 'FirstDerivative', 'SecondDerivative',
             'Laplacian', 'FirstDirectionalDerivative', 'SecondDirectionalDerivative', 'Integration1D-contiguous',
             'Integration1D-strided', 'Pooling', 'SubSampling', 'Masking', 'NNSampling', 'DiagonalOperator',
             'SparseLinearOperator', 'KroneckerProduct', 'KroneckerSum', 'KhatriRaoProduct']


@pytest.fixture(scope='module')
def operators():
    return _operators()


def _bitwise(fn, a, dtype):
    """`fn` on a guarded view of `a` at every non-zero offset == `fn` on an aligned clone, bit for bit."""
    ref = None
    for off in V.OFFSETS[dtype][1:]:
        v = dev_in(a, off, dtype)
        clone = v.clone()
        assert clone.data_ptr() % 16 == 0
        if ref is None:
            ref = fn(clone).reshape(-1).clone()
        got = fn(v).reshape(-1)
        torch.cuda.synchronize()
        assert got.data_ptr() != v.data_ptr()
        V.check_guards(v)
        assert V.same_bits(v, clone), 'input modified'
        assert V.same_bits(got, ref), f'offset {off}: differs from the aligned call'
        assert not bool(torch.isnan(got).any())


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('name', OPERATORS)
def test_operator_views_bitwise(operators, name, dtype):
    op = operators[name]
    assert set(operators) == set(OPERATORS)
    rng = np.random.default_rng(5)
    n_in = op.shape[1]
    n_out = op.nn_indices.size if name == 'NNSampling' else op.shape[0]   # NNSampling's shape quirk
    _bitwise(op._apply, rng.standard_normal(n_in), dtype)
    _bitwise(op._adj, rng.standard_normal(n_out), dtype)


def _proxes():
    from pycsou_amd import func as Fu
    from pycsou_amd.func import penalty as Pe
    n = 257
    lab = np.random.default_rng(3).integers(0, 40, 256)
    return {'L1Norm': (Pe.L1Norm(n), n), 'L2Norm': (Pe.L2Norm(n), n),
            'L21Norm-pixel': (Pe.L21Norm(dim=660 * 2, groups=np.tile(np.arange(660), 2)), 1320),
            'L21Norm-labels': (Pe.L21Norm(dim=256, groups=lab), 256),
            'SquaredL2Norm': (Pe.SquaredL2Norm(n), n), 'NonNegativeOrthant': (Pe.NonNegativeOrthant(n), n),
            'Segment': (Pe.Segment(n, a=-0.5, b=0.25), n), 'L2Ball': (Pe.L2Ball(n, radius=3.0), n),
            'LInftyBall': (Pe.LInftyBall(n, radius=0.7), n), 'L1Ball': (Pe.L1Ball(n, radius=20.0), n),
            'LInftyNorm': (Pe.LInftyNorm(n), n), 'SquaredL1Norm': (Pe.SquaredL1Norm(n), n),
            'ShannonEntropy': (Pe.ShannonEntropy(n), n), 'LogBarrier': (Pe.LogBarrier(n), n),
            '0.3*L1Norm': (0.3 * Pe.L1Norm(n), n),
            '0.3*L21Norm-pixel': (0.3 * Pe.L21Norm(dim=1320, groups=np.tile(np.arange(660), 2)), 1320)}


PROXES = ['L1Norm', 'L2Norm', 'L21Norm-pixel', 'L21Norm-labels', 'SquaredL2Norm', 'NonNegativeOrthant', 'Segment',
          'L2Ball', 'LInftyBall', 'L1Ball', 'LInftyNorm', 'SquaredL1Norm', 'ShannonEntropy', 'LogBarrier', '0.3*L1Norm',
          '0.3*L21Norm-pixel']


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('name', PROXES)
def test_prox_views_bitwise(name, dtype):
    f, n = _proxes()[name]
    a = 2.0 * np.random.default_rng(9).standard_normal(n)
    _bitwise(lambda t: f._prox(t, 0.37), a, dtype)
    if hasattr(f, '_fenchel'):
        _bitwise(lambda t: f._fenchel(t, 0.61), a, dtype)


@pytest.mark.parametrize('dtype', DT)
def test_kl_divergence_views_bitwise(dtype):
    """The data vector of a KLDivergence is a kernel argument too: x and y on misaligned views."""
    from pycsou_amd.func.loss import KLDivergence
    rng = np.random.default_rng(12)
    y, a = rng.uniform(0.1, 3.0, 257), 2.0 * rng.standard_normal(257)
    ref = None
    for off in V.OFFSETS[dtype][1:]:
        yv = dev_in(y, off, dtype)
        ys = yv.clone()
        fa, fv = KLDivergence(257, ys), KLDivergence(257, yv)
        assert fv._dev(yv).data_ptr() == yv.data_ptr(), 'a contiguous offset view is kept as it is'
        xv = dev_in(a, off, dtype)
        xs = xv.clone()
        ref = fa._prox(xs, 0.37) if ref is None else ref
        got = fv._prox(xv, 0.37)
        torch.cuda.synchronize()
        V.check_guards(xv, yv)
        assert V.same_bits(xv, xs) and V.same_bits(yv, ys) and V.same_bits(got, ref)
        assert V.same_bits(fv._fenchel(xv, 0.61), fa._fenchel(xs, 0.61))


@pytest.mark.parametrize('dtype', DT)
def test_torch_backed_views_tolerance(dtype):
    """DenseLinearOperator (torch.mv), ExplicitLinearFunctional (torch.dot) and a KroneckerProduct of dense
    factors (torch.matmul) go through rocBLAS, which may pick another kernel for a misaligned pointer: held to the
    families' bar against fp64 (tests/test_gpu_ops.py TOL) in place of bitwise equality."""
    from pycsou_amd import linop as Lo
    from pycsou_amd.func.base import ExplicitLinearFunctional
    rng = np.random.default_rng(6)
    tol = {np.float64: 1e-12, np.float32: 2e-6}[dtype]
    A, B, vec = rng.standard_normal((37, 257)), rng.standard_normal((5, 6)), rng.standard_normal(257)
    Ar, Br, vr = V.rounded(A, dtype), V.rounded(B, dtype), V.rounded(vec, dtype)
    D, Kp, Lf = Lo.DenseLinearOperator(A), Lo.KroneckerProduct(Lo.DenseLinearOperator(B), Lo.DenseLinearOperator(A)), \
        ExplicitLinearFunctional(vec)
    M = np.kron(Ar, Br)
    x, w, xk, wk = (V.rounded(rng.standard_normal(n), dtype) for n in (257, 37, 257 * 6, 37 * 5))
    for off in V.OFFSETS[dtype][1:]:
        for fn, a, ref in ((D._apply, x, Ar @ x), (D._adj, w, Ar.T @ w), (Kp._apply, xk, M @ xk),
                           (Kp._adj, wk, M.T @ wk), (Lf._apply, x, np.array([vr @ x]))):
            v = dev_in(a, off, dtype)
            s = v.clone()
            got = fn(v)
            torch.cuda.synchronize()
            V.check_guards(v)
            assert V.same_bits(v, s)
            r = V.rel_l2(host(got), ref)
            assert r < tol, (fn, off, r)


# ---------------------------------------------------------------- C. the library's own classes

def _check_blocks(got, names, sections, mats, vin, dtype, adjoint, split_in):
    """Block by block against the fp64 reference: `sections` cut the output (`split_in` False) or the input."""
    got = host(got)
    if split_in:     # out = sum_i block_i(v[sec_i]): compared as a whole, each term with its own bar
        ref, bar = 0.0, 0.0
        for i, n in enumerate(names):
            v = vin[sections[i]:sections[i + 1]]
            term = V.block_ref(n, mats, v, adjoint)
            kind, b = V.block_bar(n, mats, v, dtype)
            # a relative-L2 bar bounds every element by tol ||term||_2; the k - 1 additions of the stack round
            # partial sums below sum_i |term_i|_inf
            bar = bar + (b if kind == 'abs' else b * np.linalg.norm(term)) + \
                (len(names) - 1) * np.finfo(dtype).eps * np.abs(term).max()
            ref = ref + term
        V.compare(got, ref, bar, f'sum of {names}')
        return
    for i, n in enumerate(names):
        blk = got[sections[i]:sections[i + 1]]
        ref = V.block_ref(n, mats, vin, adjoint)
        kind, b = V.block_bar(n, mats, vin, dtype)
        if kind == 'abs':
            V.compare(blk, ref, b, f'block {n}')
        else:
            assert V.rel_l2(blk, ref) < b, (n, V.rel_l2(blk, ref))


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('name', ['vstack_img', 'vstack_sig', 'hstack_img', 'blockdiag'])
def test_linop_stack_views(name, dtype):
    op, names, mats, cols, rows = V.build_stack(name)
    assert V.misaligned_splits(cols, dtype) or V.misaligned_splits(rows, dtype)
    rng = np.random.default_rng(31)
    x, w = V.rounded(rng.standard_normal(op.shape[1]), dtype), V.rounded(rng.standard_normal(op.shape[0]), dtype)
    xd, wd = torch.as_tensor(x.astype(dtype)).cuda(), torch.as_tensor(w.astype(dtype)).cuda()
    xs, ws = xd.clone(), wd.clone()
    fwd, adj = op._apply(xd), op._adj(wd)
    torch.cuda.synchronize()
    assert V.same_bits(xd, xs) and V.same_bits(wd, ws)
    assert not bool(torch.isnan(fwd).any()) and not bool(torch.isnan(adj).any())
    if name.startswith('vstack'):
        _check_blocks(fwd, names, rows, mats, x, dtype, False, split_in=False)
        _check_blocks(adj, names, rows, mats, w, dtype, True, split_in=True)
    elif name == 'hstack_img':
        _check_blocks(fwd, names, cols, mats, x, dtype, False, split_in=True)
        _check_blocks(adj, names, cols, mats, w, dtype, True, split_in=False)
    else:   # block diagonal: block i maps x[cols_i] to out[rows_i]
        for got, vin, sin, sout, a in ((host(fwd), x, cols, rows, False), (host(adj), w, rows, cols, True)):
            for i, n in enumerate(names):
                v = vin[sin[i]:sin[i + 1]]
                ref = V.block_ref(n, mats, v, a)
                kind, b = V.block_bar(n, mats, v, dtype)
                blk = got[sout[i]:sout[i + 1]]
                if kind == 'abs':
                    V.compare(blk, ref, b, f'block {n}')
                else:
                    assert V.rel_l2(blk, ref) < b, (n, a, V.rel_l2(blk, ref))


@pytest.mark.parametrize('dtype', DT)
def test_block_operator_views(dtype):
    """BlockOperator [[D5, S], [S^T, C15]]: the input is cut at [0, 5, 5 + N] and the adjoint's at the same rows."""
    op, names, mats, cols, rows = V.build_stack('block2x2')
    assert V.misaligned_splits(cols, dtype) and V.misaligned_splits(rows, dtype)
    rng = np.random.default_rng(32)
    x, w = V.rounded(rng.standard_normal(op.shape[1]), dtype), V.rounded(rng.standard_normal(op.shape[0]), dtype)
    fwd = host(op._apply(torch.as_tensor(x.astype(dtype)).cuda()))
    adj = host(op._adj(torch.as_tensor(w.astype(dtype)).cuda()))
    tol = {np.float64: 1e-12, np.float32: 2e-6}[dtype]
    eps = np.finfo(dtype).eps
    for got, vin, a in ((fwd, x, False), (adj, w, True)):
        # out row-block r = sum_c block[r][c] v[sec_c]   (adjoint: block[c][r]^T)
        for r in range(2):
            terms = []
            for c in range(2):
                n = names[c][r] if a else names[r][c]
                terms.append((n, V.block_ref(n, mats, vin[cols[c]:cols[c + 1]], a), vin[cols[c]:cols[c + 1]]))
            ref = terms[0][1] + terms[1][1]
            bar = sum((V.block_bar(n, mats, v, dtype)[1] if V.block_bar(n, mats, v, dtype)[0] == 'abs'
                       else tol * np.linalg.norm(t)) + eps * np.abs(t).max() for n, t, v in terms)
            V.compare(got[rows[r]:rows[r + 1]], ref, bar, f'row block {r}, adjoint {a}')


@pytest.mark.parametrize('dtype', DT)
def test_functional_stack_views(dtype):
    """ProxFuncHStack / DiffFuncHStack behind a block of 37 elements: prox, Fenchel prox and gradient block by
    block against the oracle's NumPy proxes, at the families' bar (tests/test_gpu_ops.py TOL)."""
    tol = {np.float64: 1e-12, np.float32: 2e-6}[dtype]
    hs = V.func_stack('prox')
    off = list(hs._off)
    assert V.misaligned_splits(off, dtype)
    z = V.rounded(2.0 * np.random.default_rng(33).standard_normal(hs.dim), dtype)
    zd = torch.as_tensor(z.astype(dtype)).cuda()
    zs = zd.clone()

    def hprox(v, t):
        return np.concatenate([OR.prox_l1(v[off[0]:off[1]], t), OR.prox_l2(v[off[1]:off[2]], 0.7 * t),
                               OR.prox_l21_pixel(v[off[2]:off[3]], 0.5 * t, 2), OR.prox_l1(v[off[3]:off[4]], 0.3 * t)])
    got_p, got_f = host(hs._prox(zd, 0.37)), host(hs._fenchel(zd, 0.61))
    assert V.same_bits(zd, zs)
    ref_p, ref_f = hprox(z.copy(), 0.37), OR.fenchel_prox(hprox, z.copy(), 0.61)
    for i in range(4):
        s = slice(off[i], off[i + 1])
        assert V.rel_l2(got_p[s], ref_p[s]) < tol, (i, V.rel_l2(got_p[s], ref_p[s]))
        assert V.rel_l2(got_f[s], ref_f[s]) < tol, (i, V.rel_l2(got_f[s], ref_f[s]))
    dh, yd = V.func_stack('diff')
    o = list(dh._off)
    assert V.misaligned_splits(o, dtype)
    u = V.rounded(np.random.default_rng(34).standard_normal(dh.dim), dtype)
    g = host(dh._jacT(torch.as_tensor(u.astype(dtype)).cuda()))
    ydr = V.rounded(yd, dtype)
    ref = np.concatenate([2 * u[o[0]:o[1]], 2 * (u[o[1]:o[2]] - ydr), 2 * u[o[2]:o[3]]])
    for i in range(3):
        s = slice(o[i], o[i + 1])
        assert V.rel_l2(g[s], ref[s]) < tol, (i, V.rel_l2(g[s], ref[s]))


# ---------------------------------------------------------------- D. generic PDS on such a stack

def _pds(dtype, st):
    from pycsou_amd.func import L1Norm, ProxFuncHStack, Segment
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L21Norm
    from pycsou_amd.linop import Convolve2D, Gradient, LinOpVStack, SubSampling
    from pycsou_amd.opt import PDS
    N = V.IMG[0] * V.IMG[1]
    K = LinOpVStack(SubSampling(size=N, sampling_indices=V.SUB5), Convolve2D(N, st['h15'], V.IMG),
                    Gradient(V.IMG, kind='forward'))
    K.lipschitz_cst = K.diff_lipschitz_cst = float(np.sqrt(1.0 + 1.0 + 8.0))
    sec = [0] + [int(s) for s in np.cumsum([m.shape[0] for m in K.maps])]
    assert sec == V.pds_K_sections() and V.misaligned_splits(sec, dtype)
    H = ProxFuncHStack(L1Norm(dim=5), V.PDS_LAM * L1Norm(dim=N),
                       V.PDS_LAM * L21Norm(dim=2 * N, groups=np.tile(np.arange(N), 2)))
    assert list(H._off) == sec
    F = (1 / 2) * SquaredL2Loss(dim=N, data=torch.as_tensor(st['y']).cuda())
    m = V.PDS_NIT - 1    # max_iter = min_iter = m runs m + 1 iterations
    return PDS(dim=N, F=F, G=Segment(dim=N, a=V.PDS_SEG[0], b=V.PDS_SEG[1]), H=H, K=K, rho=V.PDS_RHO,
               x0=torch.as_tensor(st['x0']).cuda(), z0=torch.as_tensor(st['z0']).cuda(), max_iter=m, min_iter=m,
               accuracy_threshold=0.0, verbose=None, engine='generic')


@pytest.mark.parametrize('dtype', DT)
def test_generic_pds_on_misaligned_stack(monkeypatch, dtype):
    from oracle import pylops1 as P
    st = V.pds_state(dtype)
    runs = {}
    for graph in (True, False):
        monkeypatch.setenv('PCS_GENERIC_GRAPH', '1' if graph else '0')
        pds = _pds(dtype, st)
        est, _, diag = pds.iterate()
        assert pds._engine is None and bool(pds._graph_used) is graph
        runs[graph] = (pds, est, diag)
    (pg, eg, dg), (pe, ee, de) = runs[True], runs[False]
    assert pg.iter == pe.iter == V.PDS_NIT
    for k in ('primal_variable', 'dual_variable'):
        assert V.same_bits(eg[k], ee[k]), k
    assert list(dg.columns) == list(de.columns) and len(dg) == V.PDS_NIT
    for c in dg.columns:
        np.testing.assert_array_equal(dg[c].to_numpy(float), de[c].to_numpy(float))
    # the oracle, NumPy callables for the blocks
    N, idx = V.IMG[0] * V.IMG[1], np.asarray(V.SUB5)
    h, lam = V.rounded(st['h15'], dtype), V.PDS_LAM
    y = st['y'].astype(np.float64)
    D = P.Gradient(V.IMG, sampling=1.0, edge=True, kind='forward')

    def Kf(x):
        return np.concatenate([x[idx], V.conv2d_np(x.reshape(V.IMG), h, 7, 7).ravel(), D.matvec(x)])

    def KT(z):
        s = np.zeros(N)
        s[idx] = z[:5]
        return s + V.conv2d_np(z[5:5 + N].reshape(V.IMG), h, 7, 7, adjoint=True).ravel() + D.rmatvec(z[5 + N:])

    def hprox(v, t):
        return np.concatenate([OR.prox_l1(v[:5], t), OR.prox_l1(v[5:5 + N], t * lam),
                               OR.prox_l21_pixel(v[5 + N:], t * lam, 2)])
    xr, zr, dr = OR.pds(lambda x: x - y, lambda v, t: OR.proj_segment(v, *V.PDS_SEG), Kf, KT,
                        lambda w, s: OR.fenchel_prox(hprox, w, s), pg.tau, pg.sigma, pg.rho,
                        st['x0'].astype(np.float64), st['z0'].astype(np.float64), max_iter=V.PDS_NIT - 1,
                        min_iter=V.PDS_NIT - 1, accuracy_threshold=0.0)
    tol = 1e-9 if dtype == np.float64 else 5e-5
    assert pg.iter == len(dr['primal'])
    ex, ez = V.rel_l2(host(eg['primal_variable']), xr), V.rel_l2(host(eg['dual_variable']), zr)
    print(f'generic PDS on the misaligned stack, {np.dtype(dtype).name}: rel L2 x {ex:.3g}, z {ez:.3g}')
    assert ex <= tol and ez <= tol, (ex, ez)
    # the Segment and the dual projections bind, nothing multiplies zeros
    x0 = st['x0']
    assert 0.2 < np.mean((x0 < V.PDS_SEG[0]) | (x0 > V.PDS_SEG[1])) < 0.9 and np.mean(zr != 0) > 0.9

