"""Times of the device pseudo-inverse loop (pycsou_amd._ops.CGNormal: pcs_cg_dir / pcs_cg_dot / pcs_cg_update between
two operator applications, hipGraph chunks, asynchronous stop read-back) on one GPU, against a comparator written
here: the same recurrence in plain torch ops with `.item()` for alpha, beta and the stop test -- what a user of the
library would write today, NOT an optimised baseline.  For a batch the comparator solves the right-hand sides one
after the other, as one does with a single-vector cg().

Cases (fp32):
  conv2d          Convolve2D on `--side`^2 (2048) with a 15 x 15 Gaussian PSF, eps = 0.1, nb = 1
  sparse_nb1/16   SparseLinearOperator of `--rows` x `--rows` (2^20) with 5 entries per row, eps = 0.1, nb = 1 and 16
Both loops run exactly `--iters` iterations (rtol = 0: the stop test is evaluated and never met).  They alternate in
one process after a warm-up of each; a run is timed with device events around the whole solve (A^T y, the set-up,
the loop and the final synchronise), so microseconds per iteration include that set-up spread over `--iters`.
The vector kernels alone: event pairs around each pcs_cg_* call of an eager run; their model bytes, 11 n words
per system and iteration (dir 3n, dot 2n, update 6n), over that time, as a fraction of the 8.0 TB/s datasheet
peak and of the 6.29 TB/s a float4 copy reaches (MI355X_MICROARCH.md).  A working set that fits the Infinity Cache
can give a fraction above 1.
Launches per iteration: the pcs_cg_* launches are known from the source (dir 1, dot 2, update 2 for nb = 1 and 3
for a batch); the operator's own launches are not counted, only its two applications.
One JSON line per case to stdout, appended to `--out` (profiles/pinv_bench.jsonl).  No thresholds: these are
measurements.  A run without a GPU fails.

  python tools/bench_pinv.py --reps 5
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
EPS = 0.1


def gaussian_psf(k=15, sigma=2.5):
    r = np.arange(k) - (k - 1) / 2
    g = np.exp(-0.5 * (r / sigma) ** 2)
    h = np.outer(g, g)
    return h / h.sum()


def torch_cg(op, y, eps2, iters, rtol=0.0):
    """scipy.sparse.linalg.cg's loop on (A^T A + eps2 I) x = A^T y for one right-hand side in torch ops; alpha, beta
    and the stop test come to the host with .item()."""
    b = op._adj(y)
    tol = rtol * torch.linalg.vector_norm(b).item()
    x, r, p = torch.zeros_like(b), b.clone(), None
    rho_prev = None
    for it in range(iters):
        if torch.linalg.vector_norm(r).item() < tol:
            break
        rho = torch.dot(r, r).item()
        if it > 0:
            p *= rho / rho_prev
            p += r
        else:
            p = r.clone()
        q = op._adj(op._apply(p))
        q += eps2 * p
        alpha = rho / torch.dot(p, q).item()
        x += alpha * p
        r -= alpha * q
        rho_prev = rho
    return x


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


def vector_kernel_time(plan, Y, iters):
    """Microseconds per iteration inside the pcs_cg_* calls of an eager run of `iters` iterations."""
    from pycsou_amd import _ops as O
    from pycsou_amd.opt._loop import LaunchTimer
    ctl = plan.ctl
    B = plan.adjoint(Y)
    plan.X.zero_()
    plan.R.copy_(B)
    ctl.start(iters, 0, 0.0, False, up_front=iters + 1)
    O.cg_init(B, plan.R, 0.0, 0.0, iters, plan.state, plan.partials, ctl.ctrl, ctl.hist)
    t = LaunchTimer()
    for _ in range(iters):
        t('dir', lambda: O.cg_dir(plan.R, plan.P, plan.state, ctl.ctrl))
        Q = plan.normal(plan.P)
        t('dot', lambda: O.cg_dot(plan.P, Q, plan.eps2, plan.state, plan.partials, ctl.ctrl))
        t('update', lambda: O.cg_update(plan.X, plan.R, plan.P, Q, plan.eps2, plan.state, plan.partials, ctl.ctrl,
                                        ctl.hist))
    ms = t.result(np.mean)
    assert ctl.iterations() == iters, 'the timed run stopped early: its launches were not all doing work'
    return {k: round(v * 1e3, 2) for k, v in ms.items()}


def run_case(name, op, m, nb, args):
    from pycsou_amd import _ops as O
    dtype, w, K = torch.float32, 4, args.iters
    n = op.shape[1]
    Y = torch.as_tensor(np.random.default_rng(7).standard_normal((nb, m))).to(device='cuda', dtype=dtype)
    plan = O.CGNormal(op, nb, dtype, EPS, chunk=args.chunk)
    ours = lambda: plan.solve(Y, rtol=0.0, maxiter=K)  # noqa: E731
    theirs = lambda: torch.stack([torch_cg(op, Y[j], EPS ** 2, K) for j in range(nb)])  # noqa: E731
    (X, it, info), Xt = ours(), theirs()       # warm-up of both, and the comparison of what they compute
    assert it == K and info.active.all() and not info.breakdown.any(), (it, info.active, info.breakdown)
    diff = float(torch.linalg.vector_norm(X - Xt) / torch.linalg.vector_norm(Xt))
    t_ours, t_theirs = [], []
    for _ in range(args.reps):
        t_ours.append(timed(ours)[0] / K)
        t_theirs.append(timed(theirs)[0] / K)
    vec = vector_kernel_time(plan, Y, K)
    vec_us = sum(vec.values())
    nbytes = 11 * n * nb * w
    rate = nbytes / (vec_us * 1e-6)
    return {'case': name, 'dtype': 'float32', 'device': torch.cuda.get_device_name(0), 'n': n, 'm': m, 'nb': nb,
            'eps': EPS, 'iterations': K, 'chunk': args.chunk, 'graph': plan.graph is not None, 'reps': args.reps,
            'what': 'whole solve by device events / iterations; rtol = 0, no early stop',
            'device_loop_us_per_iteration': stats(t_ours),
            'comparator': 'torch ops with .item() for alpha, beta and the stop test, one right-hand side at a time',
            'comparator_us_per_iteration': stats(t_theirs),
            'comparator_over_device_loop': round(float(np.median(t_theirs) / np.median(t_ours)), 3),
            'relative_difference_of_the_iterates': diff,
            'cg_launches_per_iteration': 5 if nb == 1 else 6, 'operator_applications_per_iteration': 2,
            'comparator_host_reads_per_iteration': 3 * nb,
            'vector_kernels_us_per_iteration': vec, 'vector_kernels_model_bytes_per_iteration': nbytes,
            'vector_kernels_bytes_per_time_over_hbm_peak': round(rate / HBM_PEAK, 3),
            'vector_kernels_bytes_per_time_over_hbm_copy_rate': round(rate / HBM_COPY, 3)}


def run(args):
    from pycsou_amd.linop import Convolve2D, SparseLinearOperator
    out = []

    def emit(line):
        out.append(line)
        print(json.dumps(line), flush=True)

    side = args.side
    emit(run_case('conv2d', Convolve2D(side * side, gaussian_psf(), (side, side), dtype='float32'), side * side, 1, args))
    R = args.rows
    rng = np.random.default_rng(0)
    cols = rng.integers(0, R, size=(R, 5))
    A = sp.csr_matrix((rng.standard_normal(5 * R).astype(np.float32), cols.ravel(), np.arange(0, 5 * R + 1, 5)),
                      shape=(R, R))
    A.sum_duplicates()
    A.sort_indices()
    S = SparseLinearOperator(A)
    for nb in (1, 16):
        emit(run_case(f'sparse_nb{nb}', S, R, nb, args))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=2048)
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--chunk', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'pinv_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pinv: no GPU visible; nothing is measured without one')
    lines = [json.dumps(r) for r in run(args)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
