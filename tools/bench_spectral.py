"""Times of the device eigenvalue solver (pycsou_amd._ops.eigsh_restarted: thick-restart Lanczos, CGS2 against a
stored fp64 basis by the pcs_orth_* kernels) on one GPU.

Cases:
  conv2d     singularvals(k=6) of Convolve2D on `--side`^2 (2048) with a 15 x 15 Gaussian PSF, fp32
  gradient   singularvals(k=6) of the forward Gradient on `--side`^2
  sparse     eigenvals(k=6, which='LA') of a symmetric SparseLinearOperator of `--rows` (2^20) rows, 10 entries per row
Comparators, alternating in one process after a warm-up of each, timed with device events around the whole call:
  orth='hip' against orth='torch' (the same algorithm with torch.mv products), both for exactly `--restarts`
  restarts at tol = 0 (the convergence test is evaluated and, at these sizes, never met: ArpackNoConvergence ends
  the run), so both do the same operator applications and steps;
  with `--scipy`, what the parent did -- scipy's svds / eigsh through SciOp, one host round trip per application --
  on `--scipy-side`^2 / `--scipy-rows`, wall clock, against the device route on the same operator (tol = 1e-6).
The three orth launches of each step of one cycle (dots, update, update; s = 0..m-1): event pairs around each call,
once with the fused update and once with PCS_ORTH_SPLIT=1 (axpy, then dots), alternating; their model bytes -- the
basis once per launch, w read (and for update written) once: 8 n (s + 2) and 8 n (s + 3) -- over that time as a
fraction of the 8.0 TB/s datasheet peak and of the 6.29 TB/s a float4 copy reaches.  The update reads the basis
twice; whether the second read comes from a cache is not measured here.  A basis that fits the Infinity Cache can
give a fraction above 1.
One JSON line per case to stdout, appended to `--out` (profiles/spectral_bench.jsonl).  No thresholds: these are
measurements.  A run without a GPU fails.

  python tools/bench_spectral.py --reps 3
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
K = 6


def gaussian_psf(k=15, sigma=2.5):
    r = np.arange(k) - (k - 1) / 2
    g = np.exp(-0.5 * (r / sigma) ** 2)
    h = np.outer(g, g)
    return h / h.sum()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3, out          # microseconds


def stats(v):
    return {'min': round(min(v), 2), 'median': round(float(np.median(v)), 2), 'max': round(max(v), 2)}


def gram_or_self(op):
    """(apply, n, which) as LinearOperator.eigenvals / singularvals hand them to eigsh_restarted."""
    cdt = op._compute_dtype()
    if op.is_symmetric:
        return (lambda v: op._apply(v.to(cdt)).to(torch.float64)), op.shape[1], 'LA'
    if op.shape[0] >= op.shape[1]:
        return (lambda v: op._adj(op._apply(v.to(cdt))).to(torch.float64)), op.shape[1], 'LA'
    return (lambda v: op._apply(op._adj(v.to(cdt))).to(torch.float64)), op.shape[0], 'LA'


def fixed_restarts(apply, n, which, orth, restarts):
    """Exactly `restarts` restarts at tol = 0; returns (operator applications, the wanted Ritz values' count)."""
    from scipy.sparse.linalg import ArpackNoConvergence
    from pycsou_amd import _ops as O
    count = [0]

    def counted(v):
        count[0] += 1
        return apply(v)
    try:
        O.eigsh_restarted(counted, n, K, which, tol=0, maxiter=restarts, orth=orth)
        done = True
    except ArpackNoConvergence:
        done = False
    return count[0], done


def orth_launch_times(apply, n, m, split):
    """Microseconds inside the dots / update / update calls of one cycle of m steps, summed over the steps."""
    from pycsou_amd import _ops as O
    from pycsou_amd.opt._loop import LaunchTimer
    if split:
        os.environ['PCS_ORTH_SPLIT'] = '1'
    else:
        os.environ.pop('PCS_ORTH_SPLIT', None)
    try:
        be = O._OrthHip(n, m, O.device())
        q = torch.randn(n, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
        be.V[0] = (q / torch.linalg.vector_norm(q)).to(be.dev)
        be.begin()
        t = LaunchTimer()
        h1, h2, h3 = be.h
        for s in range(m):
            be.w.copy_(apply(be.V[s]))
            t('dots', lambda: O.orth_dots(be.V, s, be.w, h1, be.partials))
            t('update1', lambda: O.orth_update(be.V, s, be.w, h1, h2, be.partials))
            t('update2', lambda: O.orth_update(be.V, s, be.w, h2, h3, be.partials))
            O.orth_commit(be.V, s, m, be.w, h1, h2, h3, be.brk, be.state)
        return {k: v * 1e3 for k, v in t.result(np.sum).items()}
    finally:
        os.environ.pop('PCS_ORTH_SPLIT', None)


def run_case(name, op, args):
    from pycsou_amd import _ops as O
    apply, n, which = gram_or_self(op)
    m = O.spectral_ncv(n, K)
    runs = {o: (lambda o=o: fixed_restarts(apply, n, which, o, args.restarts)) for o in ('hip', 'torch')}
    apps = {o: runs[o]() for o in runs}                                   # warm-up of both
    assert apps['hip'] == apps['torch'], apps                            # the same work on both sides
    t = {o: [] for o in runs}
    for _ in range(args.reps):
        for o in runs:
            t[o].append(timed(runs[o])[0] / apps[o][0])
    vec = {'fused': [], 'split': []}
    orth_launch_times(apply, n, m, False), orth_launch_times(apply, n, m, True)        # warm-up
    for _ in range(args.reps):
        vec['fused'].append(orth_launch_times(apply, n, m, False))
        vec['split'].append(orth_launch_times(apply, n, m, True))
    med = {f: {k: round(float(np.median([r[k] for r in v])), 2) for k in v[0]} for f, v in vec.items()}
    model = {'dots': sum(8 * n * (s + 2) for s in range(m)), 'update1': sum(8 * n * (s + 3) for s in range(m))}
    model['update2'] = model['update1']
    total = {f: sum(med[f].values()) for f in med}
    rate = {f: sum(model.values()) / (total[f] * 1e-6) for f in med}
    return {'case': name, 'device': torch.cuda.get_device_name(0), 'n': n, 'k': K, 'ncv': m,
            'operator_dtype': str(op._compute_dtype()), 'restarts': args.restarts, 'reps': args.reps,
            'operator_applications': apps['hip'][0], 'converged_before_the_last_restart': apps['hip'][1],
            'what': 'whole eigsh_restarted call by device events / operator applications; tol = 0, fixed restarts',
            'hip_us_per_application': stats(t['hip']), 'torch_us_per_application': stats(t['torch']),
            'torch_over_hip': round(float(np.median(t['torch']) / np.median(t['hip'])), 3),
            'orth_launches_us_per_cycle': med, 'orth_launches_us_per_cycle_total': {f: round(v, 2) for f, v in total.items()},
            'split_over_fused': round(total['split'] / total['fused'], 3),
            'orth_model_bytes_per_cycle': model,
            'orth_bytes_per_time_over_hbm_peak': {f: round(r / HBM_PEAK, 3) for f, r in rate.items()},
            'orth_bytes_per_time_over_hbm_copy_rate': {f: round(r / HBM_COPY, 3) for f, r in rate.items()}}


def run_scipy(name, op, which_public):
    """The parent's path (SciPy through SciOp) against the device route, wall clock, tol = 1e-6."""
    import scipy.sparse.linalg as spls

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, np.sort(np.asarray(out, dtype=np.float64))
    if op.is_symmetric:
        ours = lambda: op.eigenvals(K, which=which_public, tol=1e-6)     # noqa: E731
        theirs = lambda: spls.eigsh(A=op.SciOp, k=K, which=which_public, return_eigenvectors=False, tol=1e-6)  # noqa: E731
    else:
        ours = lambda: op.singularvals(K, which=which_public, tol=1e-6)  # noqa: E731
        theirs = lambda: spls.svds(A=op.SciOp, k=K, which=which_public, return_singular_vectors=False, tol=1e-6)  # noqa: E731
    ours()
    t_ours, a = wall(ours)
    t_theirs, b = wall(theirs)
    return {'case': name + '_vs_scipy', 'device': torch.cuda.get_device_name(0), 'shape': list(op.shape), 'k': K,
            'which': which_public, 'tol': 1e-6, 'what': 'wall clock of one call, milliseconds',
            'device_route_ms': round(t_ours, 2), 'scipy_through_sciop_ms': round(t_theirs, 2),
            'scipy_over_device_route': round(t_theirs / t_ours, 2),
            'largest_relative_difference': float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))}


def sym_sparse(R):
    rng = np.random.default_rng(0)
    cols = rng.integers(0, R, size=(R, 5))
    A = sp.csr_matrix((rng.standard_normal(5 * R), cols.ravel(), np.arange(0, 5 * R + 1, 5)), shape=(R, R))
    A = (A + A.T).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def run(args):
    from pycsou_amd.linop import Convolve2D, Gradient, SparseLinearOperator
    out = []

    def emit(line):
        out.append(line)
        print(json.dumps(line), flush=True)

    def ops(side, rows):
        return (('conv2d', Convolve2D(side * side, gaussian_psf(), (side, side), dtype='float32'), 'LM'),
                ('gradient', Gradient((side, side), kind='forward'), 'LM'),
                ('sparse', SparseLinearOperator(sym_sparse(rows), is_symmetric=True), 'LA'))
    for name, op, _ in ops(args.side, args.rows):
        if args.only in (None, name):
            emit(run_case(name, op, args))
    if args.scipy:
        for name, op, which in ops(args.scipy_side, args.scipy_rows):
            if args.only in (None, name):
                emit(run_scipy(name, op, which))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=2048)
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--restarts', type=int, default=4)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--only', default=None, choices=('conv2d', 'gradient', 'sparse'))
    ap.add_argument('--scipy', action='store_true')
    ap.add_argument('--scipy-side', type=int, default=256)
    ap.add_argument('--scipy-rows', type=int, default=1 << 16)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'spectral_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_spectral: no GPU visible; nothing is measured without one')
    lines = [json.dumps(r) for r in run(args)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
