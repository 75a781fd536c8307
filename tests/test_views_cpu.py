"""What the offset-view GPU tests (tests/test_gpu_views.py) rely on, shown without a GPU: the guarded buffers
give the misalignment they declare, the guard / bit / NaN checks fail on every planted fault of a NumPy stand-in
kernel, the bound of the direct convolutions holds for the same sums evaluated in np.float32 with a plain loop,
the element-wise comparator fails on a dropped tap, a shifted offset and an ignored b, and the stack classes
split their vectors at the misaligned offsets the GPU tests claim.

Worst fp32 restatement over the matrix, in units of the bound (printed by test_fp32_restatement_inside_bound):
0.0444 (pcs_conv2d_planned), 0.0159 (pcs_conv2d), 0.142 (pcs_conv1d).
"""

import numpy as np
import pytest
import torch

from tests import views as V


@pytest.mark.parametrize('dtype', V.DTYPES)
@pytest.mark.parametrize('kind', ['in', 'out'])
def test_guarded_declared_misalignment(dtype, kind):
    vals = np.arange(1, 38, dtype=dtype)
    for off in V.OFFSETS[dtype]:
        v = V.guarded(vals, off) if kind == 'in' else V.guarded_out(37, dtype, off)
        V.assert_misaligned(v, off)
        assert (v.data_ptr() % 16 == 0) == (off == 0)
        assert v.is_contiguous() and v.numel() == 37 and v._base.numel() == 2 * V.MARGIN + off + 37
        assert v.storage_offset() == V.MARGIN + off
        V.check_guards(v)
        if kind == 'in':
            np.testing.assert_array_equal(v.numpy(), vals)
            assert torch.isnan(v._base[:V.MARGIN + off]).all() and torch.isnan(v._base[V.MARGIN + off + 37:]).all()
        else:
            assert V.unwritten(v) == 37 and torch.isnan(v).all()
    # the two NaN patterns differ, so a margin value copied into the interior (or the reverse) is seen
    a, b = V.guarded_out(4, dtype, 0), V.guarded_out(4, dtype, 0)
    b.copy_(b._base[:4])
    assert V.unwritten(a) == 4 and V.unwritten(b) == 0


def _standin(x, out, fault=None):
    """out = 3-tap moving sum of x with zero boundary, in NumPy on the views' memory, with one planted fault."""
    xb, ob = x._base.numpy(), out._base.numpy()
    sx, so, n = x.storage_offset(), out.storage_offset(), x.numel()
    xv = xb[sx:sx + n]
    res = xv.copy()
    res[1:] += xv[:-1]
    res[:-1] += xv[1:]
    if fault == 'nan_leak':          # the element one past the view, times a zero weight
        res[n - 1] += 0.0 * xb[sx + n]
    keep = ob[so + 5]
    ob[so:so + n] = res
    if fault == 'unwritten':
        ob[so + 5] = keep
    if fault == 'past_end':
        ob[so + n] = 1.0
    if fault == 'before_start':
        ob[so - 1] = 1.0
    if fault == 'input_modified':
        xb[sx + 3] = np.nextafter(xb[sx + 3], np.inf)
    return out


@pytest.mark.parametrize('dtype', V.DTYPES)
@pytest.mark.parametrize('fault', [None, 'past_end', 'before_start', 'unwritten', 'input_modified', 'nan_leak'])
def test_checks_fail_on_planted_faults(dtype, fault):
    vals = np.random.default_rng(0).standard_normal(257).astype(dtype)
    for off in V.OFFSETS[dtype]:
        x, out = V.guarded(vals, off), V.guarded_out(257, dtype, off)
        snap = x.clone()
        got = _standin(x, out, fault)
        if fault is None:
            V.check_call(got, [x], [snap], [out])
            continue
        with pytest.raises(AssertionError) as e:
            V.check_call(got, [x], [snap], [out])
        want = {'past_end': 'outside the view', 'before_start': 'outside the view', 'unwritten': 'never written',
                'input_modified': 'was modified', 'nan_leak': 'NaN in the result'}[fault]
        assert want in str(e.value)


def _gap_fault_is_seen():
    x = V.guarded(np.ones(8, np.float32), 3)
    x._base[V.MARGIN + 1] = 0.0      # inside the offset gap, before the view
    return V.guard_faults(x)


def test_offset_gap_is_guarded():
    assert _gap_fault_is_seen() == 1


def _planned_sets():
    for shape in V.SHAPES2D:
        for k in V.TIERS:
            yield 'pcs_conv2d_planned', shape, (k, k), (k // 2, k // 2)
        for ks in V.PSF_GENERIC:
            yield 'pcs_conv2d', shape, ks, tuple(V.pycsou_offset(n) for n in ks)


def test_fp32_restatement_inside_bound():
    """The bound of tests/views.py holds for the same convolutions evaluated in np.float32 tap by tap, at every
    shape and tap set of the matrix (forward, adjoint, with beta = -1 and b)."""
    worst = {}
    f32 = np.float32
    for entry, shape, ks, off in _planned_sets():
        x, b, h = V.data2d(shape, ks, f32)
        bnd = V.conv_bound(h, x, f32, b, -1.0)
        for adj in ((False, True) if entry == 'pcs_conv2d_planned' else (False,)):
            ref = V.conv2d_np(x, h, *off, adjoint=adj)
            got = V.conv2d_np(x, h, *off, adjoint=adj, dtype=f32)
            r0 = V.compare(got, ref, V.conv_bound(h, x, f32), f'{entry} {shape} {ks}')
            r1 = V.compare(got + f32(-1.0) * b.astype(f32), ref - b, bnd, f'{entry} {shape} {ks} with b')
            worst[entry] = max(worst.get(entry, 0.0), r0, r1)
    for dims, axis in V.CONV1D_CASES:
        for k in V.CONV1D_K:
            x, h = V.data1d(dims, k, f32)
            off = V.pycsou_offset(k)
            r = V.compare(V.conv1d_np(x, h, off, axis, dtype=f32), V.conv1d_np(x, h, off, axis),
                          V.conv_bound(h, x, f32), f'pcs_conv1d {dims} axis {axis} k {k}')
            worst['pcs_conv1d'] = max(worst.get('pcs_conv1d', 0.0), r)
    print('fp32 restatement, worst element in units of the bound:', {k: f'{v:.3g}' for k, v in worst.items()})
    assert set(worst) == {'pcs_conv2d_planned', 'pcs_conv2d', 'pcs_conv1d'}
    assert all(0.0 < w <= 1.0 for w in worst.values()), worst


@pytest.mark.parametrize('dtype', V.DTYPES)
@pytest.mark.parametrize('k', V.TIERS)
def test_comparator_fails_on_wrong_kernels(dtype, k):
    """A dropped outer tap, an offset shifted by one and an ignored b each put elements outside the bound."""
    shape = (37, 132)
    x, b, h = V.data2d(shape, (k, k), dtype)
    c = k // 2
    ref = V.conv2d_np(x, h, c, c) - b
    bnd = V.conv_bound(h, x, dtype, b, -1.0)
    V.compare(V.conv2d_np(x, h, c, c, dtype=dtype) - b.astype(dtype), ref, bnd)
    for wrong in (V.conv2d_np(x, h, c, c, shift=1) - b, V.conv2d_np(x, h, c, c)):
        with pytest.raises(AssertionError):
            V.compare(wrong, ref, bnd)
    # a dropped corner tap moves some element by |h_c| |x|_inf, so it is seen whenever that exceeds the bound; at
    # tier 31 in fp32 the bound is 0.38 = 0.085 |x|_inf, and one corner of this draw (-0.084) lies just below it
    seen = 0
    for a, bb in ((0, 0), (0, k - 1), (k - 1, 0), (k - 1, k - 1)):
        wrong = V.conv2d_np(x, h, c, c, skip=(a, bb)) - b
        if abs(h[a, bb]) * np.max(np.abs(x)) > 1.01 * bnd:
            seen += 1
            with pytest.raises(AssertionError):
                V.compare(wrong, ref, bnd)
    assert seen >= 3, seen
    with pytest.raises(AssertionError):   # a NaN never passes
        bad = ref.copy()
        bad[3, 5] = np.nan
        V.compare(bad, ref, bnd)


def test_relative_l2_bar_misses_one_bad_element():
    """One element off by 20 x the bound at (37, 132), tier 3: relative L2 over the image 3.7e-6.  The convolution
    tests of tests/test_gpu_ops.py assert 10 * TOL = 2e-5 in fp32, so they pass it; against the bare TOL = 2e-6 it
    is one element off by 10 x the bound that passes (1.9e-6).  The element-wise comparison fails on both."""
    shape, k = (37, 132), 3
    x, _, h = V.data2d(shape, (k, k), np.float32)
    ref = V.conv2d_np(x, h, 1, 1)
    bnd = V.conv_bound(h, x, np.float32)
    for times, bar in ((20, 10 * V.OLD_REL_TOL), (10, V.OLD_REL_TOL)):
        bad = ref.copy()
        bad[20, 77] += times * bnd
        r = V.rel_l2(bad, ref)
        print(f'one element off by {times} x the bound ({times * bnd:.3g}): relative L2 {r:.3g}, bar {bar:.0e}')
        assert r < bar, r
        with pytest.raises(AssertionError):
            V.compare(bad, ref, bnd)


@pytest.mark.parametrize('dtype', V.DTYPES)
@pytest.mark.parametrize('name', V.STACKS)
def test_stack_splits_are_misaligned(name, dtype):
    op, names, mats, cols, rows = V.build_stack(name)
    assert cols or rows
    for sec in (cols, rows):     # every vector the class slices has a block that starts off a 16-byte boundary
        if sec:
            assert V.misaligned_splits(sec, dtype), sec
            assert 5 in np.diff(sec)    # behind a block of 5 elements


@pytest.mark.parametrize('dtype', V.DTYPES)
def test_functional_and_pds_splits_are_misaligned(dtype):
    hs = V.func_stack('prox')
    assert list(hs._off) == [0, 37, 101, 197, 257] and len(V.misaligned_splits(hs._off, dtype)) == 3
    dh, _ = V.func_stack('diff')
    assert list(dh._off) == [0, 37, 101, 197] and len(V.misaligned_splits(dh._off, dtype)) == 2
    sec = V.pds_K_sections()
    assert sec == [0, 5, 197, 581] and len(V.misaligned_splits(sec, dtype)) == 2
