"""Offset views and sentinel margins for the operator and prox entry points: helpers and the case matrix.

Every other GPU test hands the kernels freshly allocated tensors (512-byte aligned, nothing of interest around
them).  The library itself calls them on slices `t[o[i]:o[i + 1]]` of a stacked vector, on rows of a matrix and
on whatever view the user passes, so a base pointer is aligned to the element and to no more.  The helpers here
place every argument inside a larger allocation whose surroundings are NaNs of a fixed bit pattern:

`guarded(values, offset)`   one tensor of `margin + offset + n + margin` elements, every element NaN_A, `values`
                            at `[margin + offset, margin + offset + n)`; that view is returned (`view._base` is
                            the allocation).  `margin` is a multiple of 4 elements, so `view.data_ptr() % 16 ==
                            offset * itemsize % 16` on a 16-byte aligned allocation.
`guarded_out(n, ...)`       the same for an output: the interior holds NaN_B, so an element no kernel wrote is seen.
`check_guards(view)`        both margins and the offset gap bit for bit (through an integer view).
`unwritten(view)`           how many interior elements still hold NaN_B.
`same_bits(a, b)`           bitwise equality of two tensors (NaNs included).

All accesses a correct or a slightly wrong kernel makes (a few elements past either end) stay inside the one
allocation: no case is built to fault.

The bound of the direct convolutions (`conv_bound`).  A K-term dot product evaluated in floating point in any
order, with or without FMA, differs from the exact one by at most gamma_K sum |h_i x_i|, gamma_K = K u / (1 - K u)
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); with eps = 2 u, K <= 961 and the final
`+ beta b` (two more roundings, each relative to a value below sum |h| |x|_inf + |beta| |b|_inf)

    |got - ref| <= (K + 2) eps sum |h| |x|_inf + 2 eps |beta| |b|_inf,       K = kh kw  (k for pcs_conv1d).

The reference is the same sum in fp64 on inputs and taps already rounded to the dtype under test (the device holds
the taps in that dtype), whose own error, (K + 2) 2^-52 sum |h| |x|_inf, is 2^-29 of the fp32 bound and of the same
form as the fp64 one; for fp64 the bound therefore covers both sides with the factor 2 that eps = 2 u leaves.
"""

import numpy as np
import torch

MARGIN = 1024
_NAN_A = {torch.float32: 0x7FC0A5A5, torch.float64: 0x7FF8A5A5A5A5A5A5}
_NAN_B = {torch.float32: 0x7FC05A5A, torch.float64: 0x7FF85A5A5A5A5A5A}
_INT = {torch.float32: torch.int32, torch.float64: torch.int64}
OFFSETS = {np.float32: (0, 1, 2, 3), np.float64: (0, 1)}
DTYPES = (np.float32, np.float64)
TDT = {np.float32: torch.float32, np.float64: torch.float64}


def tdtype(dtype):
    return dtype if isinstance(dtype, torch.dtype) else TDT[np.dtype(dtype).type]


def _filled(n, dtype, bits, device):
    base = torch.empty(n, dtype=dtype, device=device)   # the root tensor: `view._base` of every slice of it
    base.view(_INT[dtype]).fill_(bits)
    return base


def guarded(values, offset, margin=MARGIN, device='cpu', dtype=None):
    """`values` (array or tensor, flattened) as a view at element `margin + offset` of a NaN_A-filled allocation."""
    assert margin % 4 == 0 and offset >= 0
    v = torch.as_tensor(np.ascontiguousarray(values) if isinstance(values, np.ndarray) else values).reshape(-1)
    dtype = v.dtype if dtype is None else tdtype(dtype)
    n = v.numel()
    base = _filled(2 * margin + offset + n, dtype, _NAN_A[dtype], device)
    view = base[margin + offset:margin + offset + n]
    view.copy_(v.to(dtype))
    return view


def guarded_out(n, dtype, offset, margin=MARGIN, device='cpu'):
    """An output view of `n` elements built like `guarded`, its interior NaN_B."""
    assert margin % 4 == 0 and offset >= 0
    dtype = tdtype(dtype)
    base = _filled(2 * margin + offset + n, dtype, _NAN_A[dtype], device)
    view = base[margin + offset:margin + offset + n]
    view.view(_INT[dtype]).fill_(_NAN_B[dtype])
    return view


def misalignment(view):
    return view.data_ptr() % 16


def assert_misaligned(view, offset):
    """The declared misalignment, so that no case silently runs aligned."""
    want = (offset * view.element_size()) % 16
    assert misalignment(view) == want, (misalignment(view), want)
    return view


def guard_faults(view):
    """Number of margin / gap elements of `view`'s allocation that no longer hold NaN_A."""
    base = view._base
    assert base is not None and base.dim() == 1 and view.is_contiguous()
    s, n = view.storage_offset(), view.numel()
    bits = base.view(_INT[base.dtype])
    bad = (bits[:s] != _NAN_A[base.dtype]).sum() + (bits[s + n:] != _NAN_A[base.dtype]).sum()
    return int(bad)


def check_guards(*views):
    for i, v in enumerate(views):
        bad = guard_faults(v)
        assert bad == 0, f'argument {i}: {bad} element(s) outside the view were overwritten'


def unwritten(view):
    return int((view.view(_INT[view.dtype]) == _NAN_B[view.dtype]).sum())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(_INT[a.dtype]), b.view(_INT[b.dtype])))


def check_call(got, inputs, snaps, outs=()):
    """The assertions every guarded call shares: guards of all buffers intact, inputs bit-identical to their
    snapshots, every output element written, no NaN in the result."""
    check_guards(*inputs, *outs)
    for i, (t, s) in enumerate(zip(inputs, snaps)):
        assert same_bits(t, s), f'input {i} was modified'
    for o in outs:
        assert unwritten(o) == 0, f'{unwritten(o)} output element(s) never written'
    assert not bool(torch.isnan(got).any()), 'NaN in the result: something outside the input view entered it'


# ---------------------------------------------------------------- references (NumPy)

def rounded(a, dtype):
    """`a` rounded to `dtype`, as fp64."""
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def conv2d_np(x, h, off0, off1, adjoint=False, dtype=np.float64, skip=None, shift=0):
    """out[i, j] = sum_{a, b} h[a, b] x[i + off0 - a, j + off1 - b] (zero outside), or with `adjoint` the
    correlation sum h[a, b] x[i - off0 + a, j - off1 + b]; one tap after the other in `dtype` (a plain loop, no
    FMA).  Planted faults for the comparator's proof: `skip` drops tap (a, b), `shift` moves off1."""
    x = np.asarray(x, dtype=dtype)
    h = np.asarray(h, dtype=dtype)
    n0, n1 = x.shape
    out = np.zeros((n0, n1), dtype=dtype)
    for a in range(h.shape[0]):
        for b in range(h.shape[1]):
            if skip == (a, b):
                continue
            s0, s1 = (a - off0, b - off1 - shift) if adjoint else (off0 - a, off1 + shift - b)
            lo0, hi0, lo1, hi1 = max(0, -s0), min(n0, n0 - s0), max(0, -s1), min(n1, n1 - s1)
            if lo0 < hi0 and lo1 < hi1:
                out[lo0:hi0, lo1:hi1] += h[a, b] * x[lo0 + s0:hi0 + s0, lo1 + s1:hi1 + s1]
    return out


def conv1d_np(x, h, off, axis, dtype=np.float64):
    """out[i] = sum_t h[t] x[i + off - t] along `axis`, zero outside (pcs_conv1d's definition)."""
    x = np.asarray(x, dtype=dtype)
    h = np.asarray(h, dtype=dtype)
    out = np.zeros_like(x)
    n = x.shape[axis]
    for t in range(h.size):
        s = off - t
        lo, hi = max(0, -s), min(n, n - s)
        if lo >= hi:
            continue
        dst, src = [slice(None)] * x.ndim, [slice(None)] * x.ndim
        dst[axis], src[axis] = slice(lo, hi), slice(lo + s, hi + s)
        out[tuple(dst)] += h[t] * x[tuple(src)]
    return out


def conv_bound(h, x, dtype, b=None, beta=0.0):
    """The element-wise bound of the module docstring (a scalar: it uses |x|_inf)."""
    eps = float(np.finfo(dtype).eps)
    bnd = (np.size(h) + 2) * eps * float(np.sum(np.abs(h))) * float(np.max(np.abs(x)))
    if b is not None:
        bnd += 2 * eps * abs(beta) * float(np.max(np.abs(b)))
    return bnd


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bnd over the elements (inf for a non-finite result)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.all(np.isfinite(got)):
        return float('inf')
    return float(np.max(np.abs(got - ref))) / bnd


def compare(got, ref, bnd, what=''):
    """Element by element against the bound; returns the worst element in units of the bound."""
    r = worst_ratio(got, ref, bnd)
    assert r <= 1.0, f'{what}: worst element {r:.3g} x the bound {bnd:.3g}'
    return r


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


# worst element in units of the bound per (entry point, dtype name, offset): filled by the section A tests
RECORD = {}


def record(entry, dtype, offset, ratio):
    key = (entry, np.dtype(dtype).name, int(offset))
    RECORD[key] = max(RECORD.get(key, 0.0), float(ratio))


# ---------------------------------------------------------------- section A: the case matrix

SHAPES2D = ((9, 8), (37, 132), (64, 64))     # rows of whole 16-byte groups in both dtypes: the vector form when aligned
TIERS = (3, 15, 31)
PSF_GENERIC = ((4, 6), (40, 3))             # no tier takes these: k_conv2d and k_conv2d_big
CONV1D_CASES = (((5, 256), 1), ((3, 520), 1), ((12, 16, 24), 0), ((12, 16, 24), 1))
CONV1D_K = (1, 4, 15, 20)                   # 20 is above kC1K: the scalar kernel whatever the alignment
FFT_SHAPE, FFT_PSF = (40, 48), (33, 33)
FFT_TOL = {np.float64: 1e-12, np.float32: 2e-6}   # the relative bars of tests/test_gpu_fftconv.py
OLD_REL_TOL = 2e-6                          # tests/test_gpu_ops.py, fp32: relative L2 over the image


def pycsou_offset(n):
    return n // 2 - 1 if n % 2 == 0 else n // 2


def combos(dtype, has_b):
    """(offset of x, of out, of b, the offset the case is recorded under): the control, then every non-zero
    offset on each argument alone and on all together."""
    names = 3 if has_b else 2
    out = [((0,) * 3, 0)]
    for o in OFFSETS[dtype][1:]:
        for i in range(names):
            out.append((tuple(o if j == i else 0 for j in range(3)), o))
        out.append(((o, o, o if has_b else 0), o))
    return out


def data2d(shape, kshape, dtype, seed=0):
    """Random image, b and taps (`standard_normal`, as test_convolve2d draws them), rounded to `dtype`."""
    rng = np.random.default_rng(1000 * kshape[0] + 10 * kshape[1] + shape[0] + seed)
    h = rounded(rng.standard_normal(kshape), dtype)
    x = rounded(rng.standard_normal(shape), dtype)
    b = rounded(rng.standard_normal(shape), dtype)
    return x, b, h


def data1d(dims, k, dtype):
    rng = np.random.default_rng(100 * k + len(dims) + dims[-1])
    return rounded(rng.standard_normal(dims), dtype), rounded(rng.standard_normal(k), dtype)


def fft_psf(kh=FFT_PSF[0], kw=FFT_PSF[1], seed=33):
    """A non-separable PSF without symmetry, wider than the direct tiers (as tests/test_gpu_fftconv.py builds)."""
    rng = np.random.default_rng(seed)
    r0, r1 = np.arange(kh) - (kh - 1) / 2, np.arange(kw) - (kw - 1) / 2
    yy, xx = np.meshgrid(r0, r1, indexing='ij')
    h = np.exp(-0.5 * ((xx * 0.8 + yy * 0.6) ** 2 / 60.0 + (yy * 0.8 - xx * 0.6) ** 2 / 12.0))
    h += 0.05 * rng.uniform(0, 1, (kh, kw))
    return h / h.sum()


# ---------------------------------------------------------------- sections C and D: the library's own classes

IMG = (12, 16)            # the tier-15 Convolve2D, the FFT Convolve2D and the Gradient of the stacks
SIG = (4, 64)             # the Convolve1D (last axis)
SUB5 = (3, 50, 77, 120, 191)


def stack_blocks(which):
    """The operators of the section C stacks (no device work at construction)."""
    from pycsou_amd.linop import Convolve1D, Convolve2D, DenseLinearOperator, Gradient, SubSampling
    N, M = IMG[0] * IMG[1], SIG[0] * SIG[1]
    rng = np.random.default_rng(15)
    h15, h7 = rng.standard_normal((15, 15)), rng.standard_normal(7)
    ops = {'S': SubSampling(size=N, sampling_indices=SUB5), 'C15': Convolve2D(N, h15, IMG),
           'FFT': Convolve2D(N, fft_psf(), IMG), 'G': Gradient(IMG, kind='forward'),
           'S1': SubSampling(size=M, sampling_indices=SUB5), 'C1': Convolve1D(M, h7, reshape_dims=SIG, axis=1),
           'G1': Gradient(SIG, kind='centered'), 'D5': DenseLinearOperator(rng.standard_normal((5, 5)))}
    return ops, {'h15': h15, 'h7': h7, 'D5': ops['D5'].mat}


def build_stack(name):
    """(operator, blocks as a nested layout of names, input split offsets, output split offsets).  The splits
    are the element offsets at which the class slices the vector it hands to its blocks: `_off` of a horizontal
    MapStack (forward), the row sections of a vertical LinOpStack (adjoint), `_cols` / `_rows` of a
    BlockDiagonalOperator."""
    from pycsou_amd.linop import BlockDiagonalOperator, BlockOperator, LinOpHStack, LinOpVStack
    from pycsou_amd.linop.base import _sections
    ops, mats = stack_blocks(name)
    if name == 'vstack_img':
        names = ['S', 'C15', 'FFT', 'G']
        op = LinOpVStack(*[ops[n] for n in names])
        return op, names, mats, [], _sections([ops[n].shape[0] for n in names])
    if name == 'vstack_sig':
        names = ['S1', 'C1', 'G1']
        op = LinOpVStack(*[ops[n] for n in names])
        return op, names, mats, [], _sections([ops[n].shape[0] for n in names])
    if name == 'hstack_img':
        names = ['S.H', 'C15', 'FFT', 'G.H']
        blocks = [ops['S'].H, ops['C15'], ops['FFT'], ops['G'].H]
        op = LinOpHStack(*blocks)
        return op, names, mats, list(op._off), []
    if name == 'blockdiag':
        names = ['S.H', 'C15', 'S', 'C1', 'FFT', 'G']
        blocks = [ops['S'].H, ops['C15'], ops['S'], ops['C1'], ops['FFT'], ops['G']]
        op = BlockDiagonalOperator(*blocks)
        return op, names, mats, list(op._cols), list(op._rows)
    if name == 'block2x2':
        names = [['D5', 'S'], ['S.H', 'C15']]
        op = BlockOperator([[ops['D5'], ops['S']], [ops['S'].H, ops['C15']]])
        return op, names, mats, list(op.maps[0]._off), _sections([m.shape[0] for m in op.maps])
    raise KeyError(name)


STACKS = ('vstack_img', 'vstack_sig', 'hstack_img', 'blockdiag', 'block2x2')


def misaligned_splits(offsets, dtype):
    """The interior split offsets whose byte address is not a multiple of 16."""
    size = np.dtype(dtype).itemsize
    return [o for o in offsets[1:-1] if (o * size) % 16]


def block_ref(name, mats, v, adjoint):
    """fp64 NumPy reference of one named block of the stacks on the vector `v`."""
    N, M = IMG[0] * IMG[1], SIG[0] * SIG[1]
    if name.endswith('.H'):
        return block_ref(name[:-2], mats, v, not adjoint)
    idx = np.asarray(SUB5)
    if name in ('S', 'S1'):
        if not adjoint:
            return v[idx]
        out = np.zeros(N if name == 'S' else M)
        out[idx] = v
        return out
    if name == 'D5':
        return (mats['D5'].T if adjoint else mats['D5']) @ v
    if name == 'C15':
        return conv2d_np(v.reshape(IMG), mats['h15'], 7, 7, adjoint).ravel()
    if name == 'FFT':
        return conv2d_np(v.reshape(IMG), fft_psf(), 16, 16, adjoint).ravel()
    if name == 'C1':
        h = mats['h7']
        return (conv1d_np(v.reshape(SIG), h[::-1], h.size - 1 - 3, 1) if adjoint
                else conv1d_np(v.reshape(SIG), h, 3, 1)).ravel()
    from oracle import pylops1 as P
    g = P.Gradient(IMG, sampling=1.0, edge=True, kind='forward') if name == 'G' else \
        P.Gradient(SIG, sampling=1.0, edge=True, kind='centered')
    return g.rmatvec(v) if adjoint else g.matvec(v)


def block_bar(name, mats, v, dtype):
    """('abs', bound) for the convolution blocks (section A), ('rel', tol) of the family otherwise."""
    base = name[:-2] if name.endswith('.H') else name
    if base == 'C15':
        return 'abs', conv_bound(rounded(mats['h15'], dtype), v, dtype)
    if base == 'C1':
        return 'abs', conv_bound(rounded(mats['h7'], dtype), v, dtype)
    if base == 'FFT':
        return 'rel', FFT_TOL[dtype]
    return 'rel', {np.float64: 1e-12, np.float32: 2e-6}[dtype]   # tests/test_gpu_ops.py TOL


def func_stack(kind):
    """The section C functional stacks: a first block of 37 elements, then blocks of the prox families."""
    from pycsou_amd.func import DiffFuncHStack, L1Norm, L2Norm, ProxFuncHStack, SquaredL2Loss, SquaredL2Norm
    from pycsou_amd.func.penalty import L21Norm
    if kind == 'prox':
        return ProxFuncHStack(L1Norm(dim=37), 0.7 * L2Norm(dim=64),
                              0.5 * L21Norm(dim=96, groups=np.tile(np.arange(48), 2)), 0.3 * L1Norm(dim=60))
    yd = np.random.default_rng(8).standard_normal(64)
    return DiffFuncHStack(SquaredL2Norm(dim=37), SquaredL2Loss(dim=64, data=yd), SquaredL2Norm(dim=96)), yd


# ---------------------------------------------------------------- section D: the generic PDS problem

PDS_LAM, PDS_SEG, PDS_RHO, PDS_NIT = 0.5, (0.25, 0.75), 0.9, 4


def pds_state(dtype):
    """x0 and y from U(-0.5, 1.5), z0 = lam N(0, 1): the generic state of tests/pointwise.py (nothing multiplies
    zeros, the Segment and the dual projections bind)."""
    N = IMG[0] * IMG[1]
    rng = np.random.default_rng(4)
    r = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)  # noqa: E731
    return {'x0': r(rng.uniform(-0.5, 1.5, N)), 'y': r(rng.uniform(-0.5, 1.5, N)),
            'z0': r(PDS_LAM * rng.standard_normal(5 + N + 2 * N)), 'h15': rng.uniform(0.5, 1.5, (15, 15)) / 225.0}


def pds_K_sections():
    N = IMG[0] * IMG[1]
    return [0, 5, 5 + N, 5 + 3 * N]
