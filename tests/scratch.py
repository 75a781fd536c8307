"""Caller-owned scratch buffers at their advertised size: helpers, fills and the integer test data.

The header tells a C caller to allocate exactly what the `*_ws_bytes` / `*_nblocks` functions return.  Every
other GPU test lends the kernels tensors of the caching allocator, which rounds sizes up to 512 bytes and hands
back blocks full of earlier results, so a write one slot past the end or a read of a slot nobody wrote lands in
plausible memory.  The helpers here build on tests/views.py:

`scratch(nbytes, fill, device)`  a view of exactly `nbytes` bytes (float64 when `nbytes` is a multiple of 8,
                                 uint8 otherwise) inside a NaN_A-filled allocation with `MARGIN` doubles on
                                 both sides.  The view starts 8-byte aligned, and neither its first byte nor
                                 the byte after its last is 512-byte aligned (asserted), so what follows the view
                                 is a sentinel of this allocation and never the allocator's rounding slack.
fills                            `zero`; `poison_a`, a quiet NaN whose bits differ from both sentinels;
                                 `poison_b`, every byte 0xFF: NaN as a double, 0xFFFFFFFF as a counter.
`check(*views)`                  every byte of the allocation outside the view still holds the sentinel.
`high_water(view, fill)`         offset just past the last byte that no longer holds the fill (0: untouched).
                                 Informational: a kernel that stores the fill's own value is not seen.

All accesses a correct or a slightly wrong kernel makes (a few slots past either end) stay inside the one
allocation: no case is built to fault, and no case hands a launch less than the advertised size.

The integer test data (`ints`): values in {-3..3}, to be combined with steps and scalars that are powers of
two.  `assert_exact` states on the arrays themselves what makes every sum of the cases exact in any order.
"""

import numpy as np
import torch

from tests import views as V

MARGIN = V.MARGIN                      # doubles on either side of the view
FILLS = ('zero', 'poison_a', 'poison_b')
_FILL_BITS = {'zero': 0, 'poison_a': 0x7FF8C3C3C3C3C3C3, 'poison_b': 0xFFFFFFFFFFFFFFFF}
_SENTINEL = V._NAN_A[torch.float64]


def _i64(bits):
    return bits - (1 << 64) if bits >= (1 << 63) else bits


def fill_bytes(fill):
    """The 8 bytes of a fill, in memory order."""
    return np.array([_FILL_BITS[fill]], dtype=np.uint64).view(np.uint8)


def scratch(nbytes, fill, device='cpu', align=8):
    """A view of exactly `nbytes` bytes holding `fill`, between sentinel margins (module docstring).  `align`:
    8, or 16 for the buffers the header wants 16-byte aligned (the fused steps' partials and workspace)."""
    nbytes = int(nbytes)
    assert nbytes >= 0 and fill in FILLS and align in (8, 16)
    words = -(-nbytes // 8)
    base = V._filled(2 * MARGIN + words + 64, torch.float64, _SENTINEL, device)
    p0 = base.data_ptr()
    assert p0 % 8 == 0
    for off in range(1, 64):           # the first start that leaves both ends off the 512-byte grid
        start = p0 + 8 * (MARGIN + off)
        if start % align == 0 and start % 512 and (start + nbytes) % 512:
            break
    else:
        raise AssertionError('no start leaves both ends of the view off the 512-byte grid')
    body = base[MARGIN + off:MARGIN + off + words]
    body.view(torch.int64).fill_(_i64(_FILL_BITS[fill]))
    if nbytes % 8 == 0:
        view = body
    else:                              # the bytes past the view in its last word are sentinel again
        body[-1:].view(torch.int64).fill_(_i64(_SENTINEL))
        view = base.view(torch.uint8)[8 * (MARGIN + off):8 * (MARGIN + off) + nbytes]
        tail = torch.as_tensor(np.resize(fill_bytes(fill), nbytes)[8 * (words - 1):]).to(view.device)
        view[8 * (words - 1):].copy_(tail)
    root = view._base                   # the whole allocation (as bytes, for a uint8 view)
    assert root.data_ptr() == p0 and root.numel() * root.element_size() == base.numel() * 8
    assert view.numel() * view.element_size() == nbytes
    at = address(view)
    assert at == start and (nbytes == 0 or view.data_ptr() == at)
    assert at % align == 0 and at % 512 != 0 and (at + nbytes) % 512 != 0
    return view


def span(view):
    """(first byte, bytes) of `view` inside its allocation."""
    return view.storage_offset() * view.element_size(), view.numel() * view.element_size()


def address(view):
    """The address of the view's first byte (an empty view reports no data_ptr of its own)."""
    return view._base.data_ptr() + span(view)[0]


def guard_faults(view):
    """Bytes of the allocation outside `view` that no longer hold the sentinel."""
    base = view._base
    assert base is not None and base.dim() == 1 and base.storage_offset() == 0 and view.is_contiguous()
    s, n = span(view)
    got = base.view(torch.uint8)
    assert got.numel() % 8 == 0
    want = V._filled(got.numel() // 8, torch.float64, _SENTINEL, base.device).view(torch.uint8)
    return int((got[:s] != want[:s]).sum() + (got[s + n:] != want[s + n:]).sum())


def check(*views):
    for i, v in enumerate(views):
        bad = guard_faults(v)
        assert bad == 0, f'scratch {i}: {bad} byte(s) outside the advertised size were overwritten'


def high_water(view, fill):
    """Offset just past the last byte of `view` that no longer holds `fill` (0 when all of it does)."""
    got = view.contiguous().view(torch.uint8).cpu().numpy()
    want = np.resize(fill_bytes(fill), got.size)
    changed = np.flatnonzero(got != want)
    return int(changed[-1]) + 1 if changed.size else 0


def words_changed(view, fill):
    """Per 8-byte word of a float64 view: whether it no longer holds `fill` (a value that shares its last byte
    with the fill, as inf does with a NaN, moves `high_water` by a byte but not this)."""
    return (view.view(torch.int64) != _i64(_FILL_BITS[fill])).cpu().numpy()


# ---------------------------------------------------------------- integer data

RED_BLOCK = 256                        # threads of a reduction workgroup (csrc/prox.hip)
RED_SIZES = (1, 257, 256 * 1024 - 1, 256 * 1024 + 1)
REL_SIZES = RED_SIZES + (256 * 512 - 1, 256 * 512 + 1)
L21_GROUPS = (1, 255, 257)
TRIPLES = ((3, 4, 0), (0, 0, 0), (2, 3, 6), (1, 2, 2), (4, 4, 2), (0, 3, 4))   # integer norms 5, 0, 7, 3, 6, 5


def ints(n, seed):
    """`n` values of {-3..3} as fp64 (exact in fp32 as well)."""
    return np.random.default_rng([29, int(seed), int(n)]).integers(-3, 4, int(n)).astype(np.float64)


def assert_exact(*arrays, scale=1.0, bits=24):
    """The data condition of the exact cases, on the arrays of SUMMANDS themselves (x * x for a sum of squares,
    x * y for a dot product, the entries of a line for a running sum): each array holds integers times `scale`
    (a power of two) and the sum of its absolute values -- which bounds every partial sum taken over any subset
    in any order -- stays below 2^bits scale.  bits = 24 (the default) for a sum that is carried in or rounded
    to fp32, which is then exact in both dtypes; bits = 53 for a sum the kernels carry and deliver in fp64
    whatever the dtype of the data.  Returns the largest such sum in units of `scale`."""
    assert bits in (24, 53)
    m = np.log2(scale)
    assert m == int(m)
    worst = 0.0
    for a in arrays:
        a = np.asarray(a, dtype=np.float64) / scale
        assert np.array_equal(a, np.rint(a)), 'not integers times the scale'
        worst = max(worst, float(np.sum(np.abs(a))))
    assert worst < 2 ** bits, worst
    return worst


def l21_case(ngroups, reps=1, seed=0):
    """(x, gid): groups of 3 * reps elements holding `reps` (a square) signed copies of a triple with an integer
    norm, so the group norm is an integer too; every fifth group is all zero; the labels are a permutation of
    0..ngroups-1 (unsorted) and the elements of one group lie `ngroups` apart (non-contiguous)."""
    assert int(np.sqrt(reps)) ** 2 == reps
    rng = np.random.default_rng([31, int(ngroups), int(reps), int(seed)])
    label = rng.permutation(ngroups)
    x = np.zeros((3 * reps, ngroups))
    for j in range(ngroups):
        t = (0, 0, 0) if j % 5 == 1 else TRIPLES[int(rng.integers(len(TRIPLES)))]
        x[:, j] = np.concatenate([rng.permutation(t) * rng.choice([-1.0, 1.0], 3) for _ in range(reps)])
    gid = np.tile(label, 3 * reps).astype(np.int32)
    return x.ravel(), gid


def l21_ref(x, gid, ngroups, tau, dtype):
    """out_g = max(1 - tau / ||x_g||, 0) x_g.  The group norms are integers (asserted), so the sum of squares and
    the root are exact; the factor is formed in `dtype` as the kernel forms it (one correctly rounded division,
    one subtraction) and multiplied in `dtype`: IEEE arithmetic gives one answer."""
    ss = np.zeros(ngroups)
    np.add.at(ss, gid, x * x)
    nrm = np.sqrt(ss)
    assert np.array_equal(nrm, np.rint(nrm))
    with np.errstate(divide='ignore'):
        fac = np.maximum(dtype(1) - dtype(tau) / nrm.astype(dtype), dtype(0))
    return nrm, (fac[gid] * x.astype(dtype)).astype(dtype)


# ---------------------------------------------------------------- the exact cases: data and fp64 references

def reduce_data(n):
    return ints(n, 1), ints(n, 2)


def reduce_terms(x, y):
    """The summands of pcs_reduce kinds 0..3."""
    return x * x, np.abs(x), (x - y) ** 2, x * y


def reduce_ref(x, y):
    return [float(np.sum(t)) for t in reduce_terms(x, y)]


APGD = {'tau': 0.5, 'a': 0.5, 'lam': 1.0, 'seg': (-1.0, 2.0)}     # powers of two, a Segment that binds both ways
G_NULL, G_NONNEG, G_SEGMENT, G_L1 = 0, 1, 2, 3                     # PCS_G_* / PCS_APGD_G_L1
GKINDS = (G_NULL, G_NONNEG, G_SEGMENT, G_L1)


def apgd_data(n):
    return ints(n, 3), ints(n, 4), ints(n, 5)


def apgd_ref(x, g, aux, gkind):
    """(x', x_t, the summands of sums[0], of sums[1]) of pcs_apgd_step in fp64: every value is a multiple of
    1/4 below 16, every summand a multiple of 1/16."""
    tau, a, thr = APGD['tau'], APGD['a'], APGD['tau'] * APGD['lam']
    w = x - tau * g
    if gkind == G_L1:
        w = w - thr * np.clip(w / thr, -1.0, 1.0)
    elif gkind == G_NONNEG:
        w = np.maximum(w, 0.0)
    elif gkind == G_SEGMENT:
        w = np.clip(w, *APGD['seg'])
    xn = w + a * (w - aux)
    return xn, w, (x - xn) ** 2, x * x


def mcmc_data(n):
    """(x, running sum, running sum of squares) before the sample."""
    return ints(n, 6), ints(n, 7), ints(n, 8) ** 2


def mcmc_ref(x, s, sq):
    """(sum', sumsq', the summands of sums[0], of sums[1])."""
    return s + x, sq + x * x, x * x, s * s


SPMV_ROWS = {'one_long': (1,), 'three_long': (1, 2, 3), 'mixed': (5, 0, 1, 70, 0, 2, 65, 3, 4)}


def spmv_case(name, chunk, long_row):
    """A CSR matrix with weights in {+-1, +-0.5} and the integer vector.  SPMV_ROWS lists the row lengths; 1, 2
    and 3 stand for long rows of long_row + 1 entries (two chunks), 2 chunk + 1 (three) and 3 chunk (exactly
    three full ones), every other number is a short row of that length (0: empty)."""
    from tests import sparse_cases as SC
    long_len = {1: long_row + 1, 2: 2 * chunk + 1, 3: 3 * chunk}
    lengths = [long_len.get(c, c) for c in SPMV_ROWS[name]]
    A = SC.csr_from_lengths(lengths, 3 * chunk + 7, 40 + len(lengths), exact=True)
    return A, ints(A.shape[1], 9)


KR_SLAB, KR_MAX_NK, KR_MAX_ROWS = 64, 1024, 120     # asserted against the library's constants by the GPU tests
KR_SHAPES = ((32, 32), (112, 8), (8, 112))          # k n = 1024; k + n = 120 both ways
KR_L = 64 * 5 + 9                                   # six slabs, the last one short


def kr_case(k, n, l=KR_L):
    """A (k, l) and B (n, l) with weights in {+-1, +-0.5} and x of l integers: every product is a multiple of
    1/4 below 4, every sum exact."""
    rng = np.random.default_rng([37, k, n, l])
    w = [1.0, -1.0, 0.5, -0.5]
    return rng.choice(w, size=(k, l)), rng.choice(w, size=(n, l)), ints(l, 10)


def kr_ref(A, B, x):
    return (B * x[None, :]) @ A.T


def cumsum_ref(x, shape, axis, step, reverse):
    a = np.asarray(x).reshape(shape)
    return step * (np.flip(np.cumsum(np.flip(a, axis), axis=axis), axis) if reverse else np.cumsum(a, axis=axis))
