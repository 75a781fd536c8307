"""APGD throughput on one GPU: the fused one-launch iteration against the operator-by-operator loop.

The problem is the C3 image through the public API: n^2 (4096^2) deconvolution with the 15x15 Gaussian PSF
(sigma = 2), y = C x* + 0.01 N(0, 1) as tools/bench2d.py:c3_l1, G = lam * L1Norm with
lam = 0.02 max |grad F(0)|, acceleration='CD'; an fp32 and an fp64 leg.

Each leg runs a fixed iteration count (max_iter = min_iter = steps - 1, threshold 0) after a warm-up
of both paths, and alternates the two paths in this process, `--reps` times each.  A timed window is a
host clock around the whole loop, which ends in a device synchronise:
  fused  APGD2DEngine.run of the solver's engine (the chunks launched from C, the control read-backs,
         the history read-back)
  eager  APGD(engine=False).iterate() (grad F by F's operators, pcs_apgd_step, the finalizer, the host
         loop with its lagged control read-backs)
One JSON line per leg: it/s and ms per step of every repetition with min / median / max, the algorithmic
bytes of a step (5 N words: x, Conv^T y, past_aux in; x', past_aux' out) and their rate over 8 TB/s --
a WHOLE-STEP figure (launch gaps, reduction and loop control included), not the kernel's share of peak;
kernel time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.

  python tools/bench_apgd.py --steps 6000 --warmup 100 --reps 3
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def problem(n, dtype, seed=0):
    """(F, G factory, x0): F and y on the device in `dtype`."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm
    from pycsou_amd.linop.conv import Convolve2D
    N = n * n
    xs = torch.as_tensor(bench.phantom((n, n), 64, seed).ravel()).to('cuda', dtype)
    C = Convolve2D(size=N, filter=bench.gaussian_psf(15, 2.0), shape=(n, n))
    C.lipschitz_cst = C.diff_lipschitz_cst = 1.0
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    y = C(xs) + 0.01 * torch.randn(N, generator=g, device='cuda', dtype=dtype)
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y) * C
    x0 = torch.zeros(N, device='cuda', dtype=dtype)
    lam = 0.02 * float(torch.as_tensor(F.gradient(x0)).abs().max())
    return F, (lambda: lam * L1Norm(dim=N)), x0


def solver(F, G, x0, steps, engine):
    from pycsou_amd.opt.proxalgs import APGD
    return APGD(dim=x0.numel(), F=F, G=G(), acceleration='CD', x0=x0, max_iter=steps - 1, min_iter=steps - 1,
                accuracy_threshold=0.0, verbose=None, engine=engine)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {'min': round(min(v), 4), 'median': round(float(np.median(v)), 4), 'max': round(max(v), 4)}


def leg(name, dtype, n, steps, warmup, reps):
    F, G, x0 = problem(n, dtype)
    # warm-up of both paths at the timed shape; the two paths on the same inputs (results must not change)
    fw = solver(F, G, x0, warmup, 'fused')
    xf = fw.iterate()[0]['iterand']
    ew = solver(F, G, x0, warmup, False)
    xe = ew.iterate()[0]['iterand']
    assert fw._engine is not None and ew._engine is None and fw.iter == ew.iter == warmup
    agree = float((xf - xe).double().norm() / xe.double().norm())
    fused = solver(F, G, x0, steps, 'fused')
    fused.iterate()  # builds the engine (Conv^T y, buffers); the timed windows rerun its loop from x0
    assert fused.iter == steps
    tf, te = [], []
    for _ in range(reps):
        out = []
        tf.append(timed(lambda: out.append(fused._engine.run(steps - 1, steps - 1, 0.0))))
        assert out[0][0] == steps
        eager = solver(F, G, x0, steps, False)
        te.append(timed(eager.iterate))
        assert eager.iter == steps
    N, sz = n * n, (4 if dtype == torch.float32 else 8)
    alg = 5 * N * sz
    ms_f, ms_e = [1e3 * t / steps for t in tf], [1e3 * t / steps for t in te]
    print(json.dumps({
        'leg': name, 'n': n, 'steps': steps, 'warmup': warmup, 'reps': reps,
        'window_s': {'fused': stats(tf), 'eager': stats(te)}, 'windows_at_least_0.5s': bool(min(tf + te) >= 0.5),
        'fused_ms_per_step': stats(ms_f), 'eager_ms_per_step': stats(ms_e),
        'fused_it_per_s': [round(steps / t, 1) for t in tf], 'eager_it_per_s': [round(steps / t, 1) for t in te],
        'speedup_median': round(float(np.median(ms_e) / np.median(ms_f)), 2),
        'slowest_fused_beats_fastest_eager': bool(max(tf) < min(te)),
        'alg_bytes_per_step': alg,
        'whole_step_alg_GBps_fused': round(alg / (np.median(ms_f) * 1e-3) / 1e9, 1),
        'whole_step_frac_of_8TBps_fused': round(alg / (np.median(ms_f) * 1e-3) / 8e12, 4),
        'whole_step_frac_of_8TBps_eager': round(alg / (np.median(ms_e) * 1e-3) / 8e12, 4),
        'rel_diff_fused_vs_eager_after_warmup': agree}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=6000)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--legs', default='fp32,fp64')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_apgd needs a GPU'
    assert a.reps >= 1 and a.steps >= 2 and a.warmup >= 2
    for name in a.legs.split(','):
        leg(name, {'fp32': torch.float32, 'fp64': torch.float64}[name], a.n, a.steps, a.warmup, a.reps)


if __name__ == '__main__':
    main()
