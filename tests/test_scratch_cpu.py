"""What tests/test_gpu_scratch.py relies on, shown without a GPU: the exact-size scratch view and its guard
check (tests/scratch.py), the three fills, the high-water mark, and the data conditions that make every
reference of the exact cases a matter of `array_equal`."""

import numpy as np
import pytest
import torch

from tests import scratch as S
from tests import views as V

SIZES = (0, 8, 48, 49, 53, 512, 1024, 16384, 8 * 255)


@pytest.mark.parametrize('fill', S.FILLS)
@pytest.mark.parametrize('nbytes', SIZES)
def test_scratch_is_exact_and_off_the_allocator_grid(nbytes, fill):
    v = S.scratch(nbytes, fill)
    assert v.numel() * v.element_size() == nbytes
    assert v.dtype == (torch.float64 if nbytes % 8 == 0 else torch.uint8)
    at = S.address(v)
    assert at % 8 == 0 and at % 512 != 0 and (at + nbytes) % 512 != 0
    s, n = S.span(v)
    assert s >= 8 * S.MARGIN and v._base.numel() * 8 - (s + n) >= 8 * S.MARGIN
    assert np.array_equal(v.view(torch.uint8).numpy(), np.resize(S.fill_bytes(fill), nbytes))
    S.check(v)
    assert S.high_water(v, fill) == 0
    if nbytes % 8 == 0:
        V.check_guards(v)          # a float64 view is a tests/views.py view as well


@pytest.mark.parametrize('nbytes', (8, 49, 1024))
def test_one_byte_outside_is_reported_and_inside_is_not(nbytes):
    for where in ('before', 'after', 'first', 'last'):
        v = S.scratch(nbytes, 'poison_a')
        raw = v._base.view(torch.uint8)
        s, n = S.span(v)
        at = {'before': s - 1, 'after': s + n, 'first': s, 'last': s + n - 1}[where]
        raw[at] = raw[at] ^ 0x01      # one bit of one byte
        if where in ('before', 'after'):
            assert S.guard_faults(v) == 1
            with pytest.raises(AssertionError):
                S.check(v)
            if nbytes % 8 == 0:
                with pytest.raises(AssertionError):
                    V.check_guards(v)
        else:
            S.check(v)
            assert S.high_water(v, 'poison_a') == (1 if where == 'first' else nbytes)
    far = S.scratch(nbytes, 'zero')
    far._base.view(torch.float64)[0] = 0.0     # the far end of a margin counts too
    assert S.guard_faults(far) == 8


def test_fills_differ_from_the_sentinels_and_from_each_other():
    pats = {f: S._FILL_BITS[f] for f in S.FILLS}
    pats['NaN_A'], pats['NaN_B'] = V._NAN_A[torch.float64], V._NAN_B[torch.float64]
    assert len(set(pats.values())) == 5
    for f in ('poison_a', 'poison_b'):
        assert np.isnan(np.array([pats[f]], dtype=np.uint64).view(np.float64)[0])
    assert (pats['poison_a'] >> 51) & 1 == 1, 'a quiet NaN'
    assert np.array([pats['poison_b']], dtype=np.uint64).view(np.uint32).tolist() == [0xFFFFFFFF] * 2
    # no 8-byte word of a fill equals a sentinel at any byte phase either: a shifted store is still told apart
    for f in S.FILLS:
        two = np.concatenate([S.fill_bytes(f)] * 2)
        for name in ('NaN_A', 'NaN_B'):
            sent = np.array([pats[name]], dtype=np.uint64).view(np.uint8)
            assert not any(np.array_equal(two[k:k + 8], sent) for k in range(8)), (f, name)


def test_high_water_on_hand_made_cases():
    v = S.scratch(64, 'poison_b')
    assert S.high_water(v, 'poison_b') == 0
    v[2] = 1.5
    assert S.high_water(v, 'poison_b') == 24
    v[7] = 0.0
    assert S.high_water(v, 'poison_b') == 64
    z = S.scratch(64, 'zero')
    z[3] = 0.0                         # storing the fill's own value is not seen: the mark is informational
    assert S.high_water(z, 'zero') == 0
    z.view(torch.int32)[9] = 1         # a counter in the low half of word 4 (little endian: byte 36)
    assert S.high_water(z, 'zero') == 37
    u = S.scratch(13, 'poison_a')
    u[12] = 0
    assert S.high_water(u, 'poison_a') == 13
    assert S.high_water(v, 'poison_a') == 64     # against another fill everything has changed
    w = S.scratch(32, 'poison_a')
    w[1] = float('inf')                # shares its last byte (0x7f) with the NaN: one byte short, the word is seen
    assert S.high_water(w, 'poison_a') == 15 and S.words_changed(w, 'poison_a').tolist() == [False, True, False, False]


def test_assert_exact_rejects_what_is_not_exact():
    S.assert_exact(np.array([1.0, -3.0, 2.0]))
    S.assert_exact(np.array([0.25, -0.75]), scale=0.25)
    with pytest.raises(AssertionError):
        S.assert_exact(np.array([0.3]))
    with pytest.raises(AssertionError):
        S.assert_exact(np.array([0.5]))
    with pytest.raises(AssertionError):
        S.assert_exact(np.full(2 ** 22, 4.0))            # 2^24: no longer exact in fp32
    S.assert_exact(np.full(2 ** 22, 4.0), bits=53)


# ---------------------------------------------------------------- the data of the GPU cases

def test_reduction_data_is_exact():
    """pcs_reduce / pcs_rel_sums / pcs_apgd_step / pcs_mcmc_accumulate: the kernels carry and deliver the sums in
    fp64 (bits = 53); the element-wise outputs are multiples of 1/4 far below 2^24."""
    for n in S.REL_SIZES:
        x, y = S.reduce_data(n)
        assert set(np.unique(x)) <= set(range(-3, 4)) and set(np.unique(y)) <= set(range(-3, 4))
        worst = S.assert_exact(*S.reduce_terms(x, y), bits=53)
        assert worst < 2 ** 24                            # in fact exact in fp32 as well
    for n in S.RED_SIZES:
        x, g, aux = S.apgd_data(n)
        for gk in S.GKINDS:
            xn, w, t0, t1 = S.apgd_ref(x, g, aux, gk)
            assert np.array_equal(xn, xn.astype(np.float32)) and np.array_equal(w, w.astype(np.float32))
            assert np.abs(xn).max() < 16 and np.array_equal(xn * 4, np.rint(xn * 4))
            S.assert_exact(t0, scale=1 / 16, bits=53)
            S.assert_exact(t1, bits=53)
        if n > 1000:
            assert len({tuple(S.apgd_ref(x, g, aux, gk)[0][:4096]) for gk in S.GKINDS}) == 4, 'every G acts'
        x, s, sq = S.mcmc_data(n)
        s1, sq1, t0, t1 = S.mcmc_ref(x, s, sq)
        S.assert_exact(t0, t1, bits=53)
        for a in (s1, sq1):
            assert np.array_equal(a, a.astype(np.float32)) and np.array_equal(a, np.rint(a))


def test_l21_data_has_integer_norms_unsorted_scattered_labels_and_zero_groups():
    for ng in S.L21_GROUPS:
        for reps in (1, 16):
            x, gid = S.l21_case(ng, reps)
            assert x.size == 3 * reps * ng and sorted(set(gid)) == list(range(ng))
            if ng > 1:
                assert np.any(np.diff(gid[:ng]) < 0), 'unsorted labels'
                assert np.all(np.flatnonzero(gid == gid[0])[1:] - np.flatnonzero(gid == gid[0])[:-1] == ng)
            for dtype in (np.float32, np.float64):
                nrm, out = S.l21_ref(x, gid, ng, 2.0, dtype)
                assert out.dtype == dtype and np.all(np.isfinite(out))
                if ng > 1:
                    assert (nrm == 0).any() and (nrm > 2).any()
                assert not out[(nrm == 0)[gid]].any()


def test_sparse_and_khatri_rao_data_is_exact():
    chunk, long_row = 4096, 4096
    for name in S.SPMV_ROWS:
        A, x = S.spmv_case(name, chunk, long_row)
        lengths = np.diff(A.indptr)
        nlong = int((lengths > long_row).sum())
        assert nlong == {'one_long': 1, 'three_long': 3, 'mixed': 3}[name]
        if name == 'mixed':
            assert (lengths == 0).any() and ((lengths > 0) & (lengths <= long_row)).any()
        terms = A.multiply(x[None, :]).tocsr()
        for r in range(A.shape[0]):                       # every row's summands; the products are multiples of 1/2
            S.assert_exact(terms.data[terms.indptr[r]:terms.indptr[r + 1]], scale=0.5)
        X = np.stack([S.ints(A.shape[1], 20 + b) for b in range(3)])
        start = S.ints(3 * A.shape[0], 30).reshape(3, -1)
        got = (A @ X.T).T + start                         # accumulate adds an integer to a multiple of 1/2
        assert np.array_equal(got, got.astype(np.float32))
    for k, n in S.KR_SHAPES:
        assert (k * n == S.KR_MAX_NK or k + n == S.KR_MAX_ROWS) and k * n <= S.KR_MAX_NK and k + n <= S.KR_MAX_ROWS
        A, B, x = S.kr_case(k, n)
        assert -(-S.KR_L // S.KR_SLAB) == 6 and S.KR_L % S.KR_SLAB
        S.assert_exact(np.abs(A).sum(axis=0).max() * np.abs(B).max() * np.abs(x), scale=0.25)
        ref = S.kr_ref(A, B, x)
        assert np.array_equal(ref, ref.astype(np.float32)) and ref.any()


def test_cumsum_data_is_exact():
    from tests.test_gpu_diff_family import _exact_cases, _int_data
    for shape, axis in _exact_cases():
        x = _int_data(shape)
        lines = np.moveaxis(x.reshape(shape), axis, -1).reshape(-1, shape[axis])
        worst = max(np.abs(S.cumsum_ref(x, shape, axis, 1.0, rev)).max() for rev in (False, True))
        assert worst * 2 < 2 ** 24, 'every running sum of a line, in halves, is exact in fp32'
        assert np.array_equal(lines, np.rint(lines)) and np.abs(lines).max() <= 3


def test_cumsum_workspace_sizes_of_the_gpu_cases():
    """pcs_cumsum_ws_bytes is a host function: the split cases need a workspace, the two unsplit ones none (the
    GPU test passes NULL there)."""
    from pycsou_amd import _lib as L
    from tests.test_gpu_diff_family import _exact_cases
    from tests.test_gpu_scratch import CUMSUM_UNSPLIT
    lib = L.load()
    for shape, axis in _exact_cases():
        assert 0 < lib.pcs_cumsum_ws_bytes(len(shape), L.i64s(shape), axis) <= L.PCS_CUMSUM_WS_MAX
    for shape, axis in CUMSUM_UNSPLIT:
        assert lib.pcs_cumsum_ws_bytes(len(shape), L.i64s(shape), axis) == 0
