"""Times of the CSR product pcs_csr_spmv and of the pooling kernels pcs_pool_fwd / pcs_pool_adj on one GPU, against
torch and against SciPy / NumPy on the CPU.

Cases, each in fp32 and fp64:
  spmv_stencil5     a 5-diagonal (5-point stencil) CSR of side^2 rows (4096^2 by default): 5 entries per row
  spmv_random16     a random CSR of 2^20 rows and columns, 16 entries per row
  spmv_mdm          the Gaussian MappedDistanceMatrix of a 256 x 256 grid against 4 knots (sigma 1/12; every entry
                    kept, as in the reference's plot): 65536 rows of 4 entries
  spmv_mdm_T        its transpose: 4 rows of 65536 entries, the long-row path (64 chunks + partials)
  pool_2x2 / pool_3x3 / pool_10x20    mean pooling of side x side, forward and unpooling
The device legs: ours (O.spmv / O.pool / O.unpool as a solver calls them) and torch (torch.mv on a
torch.sparse_csr_tensor; torch.nn.functional.avg_pool2d where the block divides the shape).  If torch's sparse
product is unavailable on this build the line says so instead.  Every leg is compared with the fp64 SciPy / NumPy
result first, warmed up, then timed with device events around back-to-back calls, `--reps` windows of at least
`--calls` calls and `--window` seconds.  The CPU leg (csr_matrix.dot / a reshape-mean) is timed with
perf_counter over a few calls.  What is timed is the CALL -- wrapper, output allocation and launches -- not the
kernel alone.
One JSON line per case and dtype to stdout, appended to profiles/sparse_bench.jsonl: microseconds per call
(min / median / max over the windows), the model bytes -- nnz (word + 4) + 8 nrows + word (ncols + nrows) for the
product, word N (1 + 1 / B) for pooling -- and those bytes over the median call time as a fraction of the 6.29
TB/s a float4 copy reaches (8.0 TB/s is the datasheet peak).  A working set that fits the Infinity Cache can give
a fraction above 1.  No thresholds: these are measurements.  A run without a GPU fails.

  python tools/bench_sparse.py --reps 5
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12


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
    got = fn().double().cpu().numpy()
    diff = float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))
    assert diff <= tol, diff
    for _ in range(args.warmup):
        fn()
    calls = max(args.calls, int(np.ceil(args.window * 1e6 / events(fn, 20))))
    t = [events(fn, calls) for _ in range(args.reps)]
    return stats(t), float(np.median(t)), diff


def cpu_leg(fn, reps=3):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return stats(t)


def rates(out, name, nbytes, median_us):
    rate = nbytes / (median_us * 1e-6)
    out[f'{name}_model_bytes_per_call_time_over_hbm_peak'] = round(rate / HBM_PEAK, 3)
    out[f'{name}_model_bytes_per_call_time_over_hbm_copy_rate'] = round(rate / HBM_COPY, 3)


def spmv_case(case, A, dtype, args):
    from pycsou_amd import _ops as O
    w = torch.empty(0, dtype=dtype).element_size()
    tol = 1e-4 if dtype == torch.float32 else 1e-11
    nrows, ncols = A.shape
    xh = np.random.default_rng(1).standard_normal(ncols)
    ref = A @ xh
    x = torch.as_tensor(xh).to(device='cuda', dtype=dtype)
    D = O.DeviceCSR(A, dtype)
    nbytes = A.nnz * (w + 4) + 8 * nrows + w * (ncols + nrows)
    out = {'case': case, 'dtype': str(dtype).split('.')[-1], 'what': 'call time (wrapper + launches), device events',
           'shape': [nrows, ncols], 'nnz': int(A.nnz), 'lanes': D.lanes, 'long_rows': D.nlong, 'chunks': D.nchunks,
           'model_bytes': nbytes, 'reps': args.reps}
    out['ours_us'], med, out['ours_max_rel_diff'] = device_leg(lambda: O.spmv(D, x), ref, tol, args)
    rates(out, 'ours', nbytes, med)
    try:
        S = torch.sparse_csr_tensor(D.rowptr, D.colind.to(torch.int64), D.vals, size=(nrows, ncols))
        out['torch_us'], tmed, out['torch_max_rel_diff'] = device_leg(lambda: torch.mv(S, x), ref, tol, args)
        out['torch_over_ours'] = round(tmed / med, 3)
        del S
    except Exception as e:  # noqa: BLE001 -- whatever this build raises for an unsupported sparse product
        out['torch_unavailable'] = f'{type(e).__name__}: {e}'[:200]
    Ah = A.astype(np.float32 if dtype == torch.float32 else np.float64)
    xc = xh.astype(Ah.dtype)
    out['scipy_cpu_us'] = cpu_leg(lambda: Ah @ xc)
    out['device'] = torch.cuda.get_device_name(0)
    return out


def pool_case(side, block, dtype, args):
    from pycsou_amd import _ops as O
    w = torch.empty(0, dtype=dtype).element_size()
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    dims, N, B = (side, side), side * side, block[0] * block[1]
    m = O.pooled_shape(dims, block)
    xh = np.random.default_rng(2).standard_normal(dims)
    pad = np.pad(xh, [(0, m[0] * block[0] - side), (0, m[1] * block[1] - side)])

    def numpy_pool(a):
        return a.reshape(m[0], block[0], m[1], block[1]).sum(axis=(1, 3)) / B

    ref = numpy_pool(pad).ravel()
    x = torch.as_tensor(xh.ravel()).to(device='cuda', dtype=dtype)
    y = torch.as_tensor(ref).to(device='cuda', dtype=dtype)
    ref_un = np.repeat(np.repeat(y.double().cpu().numpy().reshape(m), block[0], 0), block[1], 1)[:side, :side].ravel()
    nbytes = int(w * N * (1 + 1 / B))
    out = {'case': f'pool_{block[0]}x{block[1]}', 'dtype': str(dtype).split('.')[-1],
           'what': 'call time (wrapper + launches), device events', 'shape': list(dims), 'block': list(block),
           'model_bytes': nbytes, 'reps': args.reps}
    out['pool_us'], med, out['pool_max_rel_diff'] = device_leg(lambda: O.pool(x, dims, block, 1.0 / B), ref, tol, args)
    rates(out, 'pool', nbytes, med)
    out['unpool_us'], umed, _ = device_leg(lambda: O.unpool(y, dims, block, 1.0), ref_un, 0.0, args)
    rates(out, 'unpool', nbytes, umed)
    if side % block[0] == 0 and side % block[1] == 0:
        x4 = x.view(1, 1, side, side)
        out['torch_avg_pool2d_us'], tmed, _ = device_leg(
            lambda: torch.nn.functional.avg_pool2d(x4, block).reshape(-1), ref, tol, args)
        out['torch_over_pool'] = round(tmed / med, 3)
    else:
        out['torch_avg_pool2d'] = 'the block does not divide the shape'
    padc = pad.astype(np.float32 if dtype == torch.float32 else np.float64)
    out['numpy_cpu_us'] = cpu_leg(lambda: numpy_pool(padc))
    out['device'] = torch.cuda.get_device_name(0)
    return out


def matrices(args):
    from pycsou_amd.linop import MappedDistanceMatrix
    rng = np.random.default_rng(0)
    n, N = args.side, args.side * args.side
    yield 'spmv_stencil5', sp.diags([-np.ones(N - n), -np.ones(N - 1), 4 * np.ones(N), -np.ones(N - 1), -np.ones(N - n)],
                                    [-n, -1, 0, 1, n], format='csr')
    R = args.rows
    cols = rng.integers(0, R, size=(R, 16))
    A = sp.csr_matrix((rng.standard_normal(16 * R), cols.ravel(), np.arange(0, 16 * R + 1, 16)), shape=(R, R))
    A.sum_duplicates()
    yield 'spmv_random16', A
    t = np.linspace(0, 2, 256)
    gx, gy = np.meshgrid(t, t)
    knots = np.stack((2 * np.random.default_rng(2).random(4), 2 * np.random.default_rng(3).random(4)), axis=-1)
    sigma = 1 / 12
    M = MappedDistanceMatrix(samples1=np.stack((gx.ravel(), gy.ravel()), axis=-1), samples2=knots,
                             function=lambda d: np.exp(-d ** 2 / (2 * sigma ** 2)), operator_type='dense').mat
    M = sp.csr_matrix((M.ravel(), np.tile(np.arange(4), M.shape[0]), np.arange(0, M.size + 1, 4)), shape=M.shape)
    yield 'spmv_mdm', M
    T = M.T.tocsr()
    T.sort_indices()
    yield 'spmv_mdm_T', T


def run(args):
    lines = []
    for case, A in matrices(args):
        for dtype in (torch.float32, torch.float64):
            lines.append(spmv_case(case, A, dtype, args))
            print(json.dumps(lines[-1]), flush=True)
        del A
    for block in ((2, 2), (3, 3), (10, 20)):
        for dtype in (torch.float32, torch.float64):
            lines.append(pool_case(args.side, block, dtype, args))
            print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=4096)
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.3, help='least seconds per timed window')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'sparse_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sparse: no GPU visible; nothing is measured without one')
    lines = [json.dumps(r) for r in run(args)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
