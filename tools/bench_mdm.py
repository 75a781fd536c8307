"""Times of the matrix-free MappedDistanceMatrix (pcs_mdm_apply, csrc/mdm.hip) on one GPU against the route it
replaces: the dense matrix assembled on the host, uploaded and applied with torch.mv.

Cases: (L, K) = (65536, 4), (65536, 4096) and (65536, 65536) points in the unit square, forward (L outputs, K
columns) and adjoint (K outputs, L columns), in fp32 and fp64, for two functions:
  matern1_ord2       Matern(1, 0.1), Euclidean distance (the sqrt fast path, one exp per pair)
  subgauss08_ord08   SubGaussian(0.8, 1 / 12) with ord = 0.8, the reference's own example (three pow and one exp per pair)
Where the dense matrix has at most `--dense-max` entries it is built as MappedDistanceMatrix(operator_type='dense')
builds it and three more numbers are recorded: the host assembly time (once, fp64, wall clock), the upload time per
dtype (host clock around a copy that ends in a synchronise) and the torch.mv time.  The largest case has no dense
route (32 GiB in fp64).

Every device leg is first compared with an fp64 NumPy product on the first `--check-rows` outputs, warmed up, then
timed with device events around back-to-back calls, `--reps` windows of at least `--calls` calls and `--window`
seconds.  What is timed is the CALL (wrapper, output allocation, launches), not the kernel alone.  One JSON line per
case, function and dtype to stdout, appended to profiles/mdm_bench.jsonl: microseconds per call (min / median / max
over the windows), the plan, and pairs per second (L K over the median call time).  No thresholds: these are
measurements.  A run without a GPU fails.

  python tools/bench_mdm.py --reps 3
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(65536, 4), (65536, 4096), (65536, 65536)]


def functions():
    from pycsou_amd.math.green import Matern, SubGaussian
    return [('matern1_ord2', Matern(1, 0.1), 2.0), ('subgauss08_ord08', SubGaussian(0.8, 1 / 12), 0.8)]


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
    """Check the first outputs against the fp64 reference, warm up, time: (stats, median, max relative difference)."""
    got = fn().double().cpu().numpy()[:ref.size]
    diff = float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))
    assert diff <= tol, diff
    for _ in range(args.warmup):
        fn()
    calls = max(args.calls, int(np.ceil(args.window * 1e6 / events(fn, 3))))
    t = [events(fn, calls) for _ in range(args.reps)]
    return stats(t), float(np.median(t)), diff


def host_rows(func, o, A, B, v, rows):
    """fp64 NumPy reference of the first `rows` outputs of sum_j phi(||A_i - B_j||_o) v_j."""
    d = np.linalg.norm(A[:rows, None, :] - B[None, :, :], axis=-1, ord=o)
    return np.asarray(func(d)) @ v


def case(L, K, name, func, o, args):
    from pycsou_amd import _ops as O
    from pycsou_amd.linop.sampling import MappedDistanceMatrix
    rng = np.random.default_rng([71, L, K])
    s1, s2 = rng.random((L, 2)), rng.random((K, 2))
    xh, yh = rng.standard_normal(K), rng.standard_normal(L)
    rows = args.check_rows
    ref_f, ref_a = host_rows(func, o, s1, s2, xh, min(rows, L)), host_rows(func, o, s2, s1, yh, min(rows, K))
    dense = L * K <= args.dense_max
    mat, t_host = None, None
    if dense:
        t0 = time.perf_counter()
        D = MappedDistanceMatrix(samples1=s1, samples2=s2, function=func, ord=o, operator_type='dense')
        t_host = time.perf_counter() - t0
        mat = D.mat
    lines = []
    for dtype in (torch.float32, torch.float64):
        tol = 1e-4 if dtype == torch.float32 else 1e-11
        op = MappedDistanceMatrix(samples1=s1, samples2=s2, function=func, ord=o,
                                  dtype=np.float32 if dtype == torch.float32 else np.float64)
        assert op.matrix_free
        x, y = (torch.as_tensor(a).to(device='cuda', dtype=dtype) for a in (xh, yh))
        out = {'case': f'mdm_{L}x{K}', 'function': name, 'ord': o, 'dim': 2, 'dtype': str(dtype).split('.')[-1],
               'what': 'call time (wrapper + launches), device events', 'reps': args.reps,
               'device': torch.cuda.get_device_name(0), 'pairs': L * K,
               'plan_fwd': list(O.mdm_plan(L, K)), 'plan_adj': list(O.mdm_plan(K, L))}
        out['free_fwd_us'], mf, out['free_fwd_max_rel_diff'] = device_leg(lambda: op._apply(x), ref_f, tol, args)
        out['free_adj_us'], ma, out['free_adj_max_rel_diff'] = device_leg(lambda: op._adj(y), ref_a, tol, args)
        out['free_fwd_pairs_per_s'], out['free_adj_pairs_per_s'] = round(L * K / (mf * 1e-6), 1), round(L * K / (ma * 1e-6), 1)
        if dense:
            out['dense_host_assembly_s'] = round(t_host, 3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = torch.as_tensor(mat).to(device='cuda', dtype=dtype)
            torch.cuda.synchronize()
            out['dense_upload_s'] = round(time.perf_counter() - t0, 4)
            out['dense_matrix_bytes'] = M.numel() * M.element_size()
            out['dense_mv_fwd_us'], df, out['dense_mv_fwd_max_rel_diff'] = device_leg(lambda: torch.mv(M, x), ref_f, tol, args)
            out['dense_mv_adj_us'], da, out['dense_mv_adj_max_rel_diff'] = device_leg(lambda: torch.mv(M.T, y), ref_a, tol,
                                                                                      args)
            out['free_over_dense_mv_fwd'], out['free_over_dense_mv_adj'] = round(mf / df, 3), round(ma / da, 3)
            del M
        else:
            out['dense'] = 'not built: more than --dense-max entries'
        lines.append(out)
        print(json.dumps(out), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.2, help='least seconds per timed window')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--check-rows', type=int, default=64)
    ap.add_argument('--dense-max', type=int, default=65536 * 4096)
    ap.add_argument('--shapes', default=None, help='e.g. 65536x4,65536x4096 (default: the three of the docstring)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'mdm_bench.jsonl'))
    args = ap.parse_args()
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
    if not torch.cuda.is_available():
        raise SystemExit('bench_mdm: no GPU visible; nothing is measured without one')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for L, K in shapes:
        for name, func, o in functions():
            lines = case(L, K, name, func, o, args)
            with open(args.out, 'a') as f:       # case by case: a run that is cut short keeps what it measured
                f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
