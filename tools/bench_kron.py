"""Times of pcs_csr_spmm, of the fused Khatri-Rao kernels pcs_khatri_rao_fwd / pcs_khatri_rao_adj and of a
KroneckerProduct of two stencil factors on one GPU, each against the composition it replaces.

Cases, each in fp32 and fp64:
  spmm_axis0 / spmm_axis1   a random CSR of `--rows` rows and columns, 16 entries per row, times a dense matrix with
                            `--nb` other-axis entries, against the loop of pcs_csr_spmv over the columns (axis 0:
                            slice, copy, product, stack -- LinearOperator._apply_cols' default) or rows (axis 1)
  kr_fwd / kr_adj           KhatriRaoProduct of two dense factors A (k x l), B (n x l) over a grid of (k, n, l) that
                            straddles the fused limit (k n <= 1024, k + n <= 120): the fused kernels against the torch
                            composition written out here, mm(B * x, A^T) and sum(mm(Y, A) * B, 0); past the limit only
                            the composition exists and is timed alone
  kron_d2                   KroneckerProduct(SecondDerivative(side), SecondDerivative(side)) against
                            SecondDerivative(N, (side, side), axis=0) * SecondDerivative(N, (side, side), axis=1)
Every leg is compared with an fp64 NumPy / SciPy result first (at a reduced size where the full one would take the
host too long), warmed up, then timed with device events around back-to-back calls, `--reps` windows of at least
`--calls` calls and `--window` seconds.  What is timed is the CALL -- wrapper, output allocation and launches -- not
the kernel alone.
One JSON line per case and dtype to stdout, appended to profiles/kron_bench.jsonl: microseconds per call (min /
median / max over the windows), the model bytes of the file headers of csrc/spmm.hip and csrc/khatri_rao.hip, and
those bytes over the median call time as a fraction of the 6.29 TB/s a float4 copy reaches (8.0 TB/s is the
datasheet peak).  A working set that fits the Infinity Cache can give a fraction above 1.  No thresholds: these are
measurements.  A run without a GPU fails.

  python tools/bench_kron.py --reps 5
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12
KR_GRID = [(8, 8, 100000), (16, 16, 100000), (32, 32, 10000), (32, 32, 100000), (64, 16, 100000), (100, 10, 100000),
           (33, 32, 100000), (64, 64, 100000)]


def events(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # microseconds per call


def stats(v):
    return {'min': round(min(v), 2), 'median': round(float(np.median(v)), 2), 'max': round(max(v), 2)}


def device_leg(fn, ref, tol, args):
    """Check against the fp64 reference, warm up, time: (stats, median, max relative difference)."""
    got = fn().double().cpu().numpy().reshape(ref.shape)
    diff = float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))
    assert diff <= tol, diff
    for _ in range(args.warmup):
        fn()
    calls = max(args.calls, int(np.ceil(args.window * 1e6 / events(fn, 20))))
    t = [events(fn, calls) for _ in range(args.reps)]
    return stats(t), float(np.median(t)), diff


def rates(out, name, nbytes, median_us):
    rate = nbytes / (median_us * 1e-6)
    out[f'{name}_model_bytes_per_call_time_over_hbm_peak'] = round(rate / HBM_PEAK, 3)
    out[f'{name}_model_bytes_per_call_time_over_hbm_copy_rate'] = round(rate / HBM_COPY, 3)


def head(case, dtype, args, **kw):
    return dict({'case': case, 'dtype': str(dtype).split('.')[-1], 'what': 'call time (wrapper + launches), device events',
                 'reps': args.reps, 'device': torch.cuda.get_device_name(0)}, **kw)


def word(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def spmm_case(A, axis, dtype, args):
    from pycsou_amd import _ops as O
    w, tol = word(dtype), (1e-4 if dtype == torch.float32 else 1e-11)
    nrows, ncols = A.shape
    nb = args.nb
    Xh = np.random.default_rng(1).standard_normal((ncols, nb) if axis == 0 else (nb, ncols))
    ref = A @ Xh if axis == 0 else (A @ Xh.T).T
    X = torch.as_tensor(Xh).to(device='cuda', dtype=dtype)
    D = O.DeviceCSR(A, dtype)
    nbytes = A.nnz * (w + 4) + 8 * nrows + w * nb * (ncols + nrows)
    out = head(f'spmm_axis{axis}', dtype, args, shape=[nrows, ncols], nnz=int(A.nnz), nb=nb, lanes=D.lanes,
               plan=O.spmm_plan(D, axis, nb), model_bytes=nbytes)
    out['spmm_us'], med, out['spmm_max_rel_diff'] = device_leg(lambda: O.spmm(D, X, axis), ref, tol, args)
    rates(out, 'spmm', nbytes, med)
    if axis == 0:
        loop = lambda: torch.stack([O.spmv(D, X[:, j].contiguous()) for j in range(nb)], dim=1)  # noqa: E731
    else:
        loop = lambda: torch.stack([O.spmv(D, X[b]) for b in range(nb)], dim=0)  # noqa: E731
    out['spmv_loop_us'], lmed, out['spmv_loop_max_rel_diff'] = device_leg(loop, ref, tol, args)
    out['spmv_loop_over_spmm'] = round(lmed / med, 3)
    return out


def kr_case(k, n, l, dtype, args):
    from pycsou_amd import _ops as O
    w, tol = word(dtype), (1e-3 if dtype == torch.float32 else 1e-10)
    rng = np.random.default_rng(2)
    Ah, Bh, xh, yh = rng.standard_normal((k, l)), rng.standard_normal((n, l)), rng.standard_normal(l), \
        rng.standard_normal((n, k))
    ref_f, ref_a = (Bh * xh[None, :]) @ Ah.T, np.sum((yh @ Ah) * Bh, axis=0)
    A, B, x, Y = (torch.as_tensor(a).to(device='cuda', dtype=dtype).contiguous() for a in (Ah, Bh, xh, yh))
    fused = O.kr_fused_ok(k, n)
    spg, ngroups, ws_len = O.kr_fwd_plan(k, n, l)
    bytes_f = w * (k + n + 1) * l + w * n * k + (16 * n * k * ngroups if fused else 0)
    bytes_a = w * (k + n + 1) * l + w * n * k
    out = head('khatri_rao', dtype, args, k=k, n=n, l=l, fused_serves_it=fused, slabs_per_group=spg, groups=ngroups,
               fwd_model_bytes=bytes_f, adj_model_bytes=bytes_a,
               torch_fwd_extra_bytes=2 * w * n * l, torch_adj_extra_bytes=3 * w * n * l)
    out['torch_fwd_us'], tf, out['torch_fwd_max_rel_diff'] = device_leg(
        lambda: torch.mm(B * x[None, :], A.T), ref_f, tol, args)
    out['torch_adj_us'], ta, out['torch_adj_max_rel_diff'] = device_leg(
        lambda: torch.sum(torch.mm(Y, A) * B, dim=0), ref_a, tol, args)
    if fused:
        ws = torch.empty(ws_len, dtype=torch.float64, device='cuda')
        out['fused_fwd_us'], ff, out['fused_fwd_max_rel_diff'] = device_leg(
            lambda: O.khatri_rao_fwd(A, B, x, ws), ref_f, tol, args)
        out['fused_adj_us'], fa, out['fused_adj_max_rel_diff'] = device_leg(
            lambda: O.khatri_rao_adj(A, B, Y.reshape(-1)), ref_a, tol, args)
        rates(out, 'fused_fwd', bytes_f, ff)
        rates(out, 'fused_adj', bytes_a, fa)
        out['torch_over_fused_fwd'], out['torch_over_fused_adj'] = round(tf / ff, 3), round(ta / fa, 3)
    rates(out, 'torch_fwd', bytes_f, tf)
    rates(out, 'torch_adj', bytes_a, ta)
    return out


def kron_case(side, dtype, args):
    from pycsou_amd.linop import KroneckerProduct, SecondDerivative
    w, tol = word(dtype), (1e-3 if dtype == torch.float32 else 1e-10)
    N = side * side
    xh = np.random.default_rng(3).standard_normal((side, side))
    d2 = sp.diags([np.ones(side - 1), -2 * np.ones(side), np.ones(side - 1)], [-1, 0, 1], format='lil')
    d2[0, :3], d2[-1, -3:] = [1, -2, 1], [1, -2, 1]
    d2 = d2.tocsr()
    ref = np.asarray((d2 @ (d2 @ xh.T).T)).ravel()              # B X A^T with A = B = D2
    x = torch.as_tensor(xh.ravel()).to(device='cuda', dtype=dtype)
    K = KroneckerProduct(SecondDerivative(size=side), SecondDerivative(size=side))
    comp = SecondDerivative(size=N, shape=(side, side), axis=0) * SecondDerivative(size=N, shape=(side, side), axis=1)
    nbytes = 4 * w * N                                           # two passes, each one read and one write
    out = head('kron_d2', dtype, args, shape=[side, side], model_bytes=nbytes)
    out['kronecker_us'], km, out['kronecker_max_rel_diff'] = device_leg(lambda: K._apply(x), ref, tol, args)
    out['composition_us'], cm, out['composition_max_rel_diff'] = device_leg(lambda: comp._apply(x), ref, tol, args)
    out['kronecker_adj_us'], _, _ = device_leg(lambda: K._adj(x), np.asarray((d2.T @ (d2.T @ xh.T).T)).ravel(), tol, args)
    rates(out, 'kronecker', nbytes, km)
    out['composition_over_kronecker'] = round(cm / km, 3)
    return out


def run(args):
    rng = np.random.default_rng(0)
    R = args.rows
    cols = rng.integers(0, R, size=(R, 16))
    A = sp.csr_matrix((rng.standard_normal(16 * R), cols.ravel(), np.arange(0, 16 * R + 1, 16)), shape=(R, R))
    A.sum_duplicates()
    A.sort_indices()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for dtype in (torch.float32, torch.float64):
        for axis in (0, 1):
            emit(spmm_case(A, axis, dtype, args))
    del A
    for k, n, l in KR_GRID:
        for dtype in (torch.float32, torch.float64):
            emit(kr_case(k, n, l, dtype, args))
    for dtype in (torch.float32, torch.float64):
        emit(kron_case(args.side, dtype, args))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=2048)
    ap.add_argument('--rows', type=int, default=1 << 18)
    ap.add_argument('--nb', type=int, default=32)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.3, help='least seconds per timed window')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'kron_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_kron: no GPU visible; nothing is measured without one')
    lines = [json.dumps(r) for r in run(args)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
