"""Measure the two PMYULA kernels on the GPU (bench.py measures the flagship workload and is not touched).

  python tools/bench_mcmc.py [--side 4096] [--K 2] [--reps 20] [--windows 5] [--out profiles/mcmc_bench.jsonl]

Per dtype (fp32, fp64), at side^2 pixels:
  * step_fused        pcs_myula_step, G = lam * L1 formed in the kernel, noise generated in the kernel
  * step_fused_zbuf   the same launch with the noise read from a buffer (no Philox / Box-Muller in it)
  * step_composed     the same update from the existing ops: prox_l1, three axpby, and torch.randn for the noise
  * normal_fill       pcs_mcmc_normal alone (one word written per element)
  * accumulate        pcs_mcmc_accumulate in steady state (count > 5), K p-values

Timing: device events around `reps` back-to-back calls after a warm-up of every shape, `windows` windows, the
median window; bytes are the words the algorithm must move, computed from the shapes below, and the share is
against the 6.3 TB/s a streaming kernel achieves on an MI355X (8 TB/s peak).  A step that generates its noise
moves one word less than one that reads it: if it is not slower than `step_fused_zbuf`, the Box-Muller
arithmetic is hidden under the memory traffic.  One JSON line per measurement."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12


def timed(fn, reps, windows):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=4096)
    ap.add_argument('--K', type=int, default=2)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'mcmc_bench.jsonl'))
    a = ap.parse_args()
    from pycsou_amd import _lib as L, _ops as O
    L.gpu()
    n, K = a.side * a.side, a.K
    pvalues = tuple(np.linspace(0.1, 0.9, K))
    tau, gamma, lam = 0.6, 0.2, 0.7
    rows = []
    for dtype in (torch.float32, torch.float64):
        esz = 4 if dtype == torch.float32 else 8
        gen = torch.Generator(device='cuda').manual_seed(1)
        x, g, z = (torch.randn(n, dtype=dtype, device='cuda', generator=gen) for _ in range(3))
        out = torch.empty_like(x)
        gk = (L.PCS_APGD_G_L1, lam, (0.0, 1.0))
        it = [0]

        def fused():
            it[0] += 1
            O.myula_step(x, g, tau, gamma, gk=gk, seed=1, it=it[0], out=out)

        def fused_zbuf():
            O.myula_step(x, g, tau, gamma, gk=gk, z=z, out=out)

        def composed():
            zz = torch.randn(n, dtype=dtype, device='cuda')
            p = O.prox_l1(x, tau * lam)
            t = O.axpby(x, g, 1 - gamma / tau, -gamma)
            t = O.axpby(t, p, 1.0, gamma / tau)
            O.axpby(t, zz, 1.0, float(np.sqrt(2 * gamma)), out=out)

        def fill():
            O.mcmc_normal(n, dtype, 1, 3)

        state = O.P2State(pvalues, n, dtype)
        total, total_sq = torch.zeros_like(x), torch.zeros_like(x)
        sums = torch.zeros(2, dtype=torch.float64, device='cuda')
        for i in range(6):  # past the warm-up samples of P2
            O.mcmc_accumulate(O.mcmc_normal(n, dtype, 2, i), total, total_sq, state, sums)

        def accumulate():
            O.mcmc_accumulate(x, total, total_sq, state, sums)

        acc_bytes = n * (esz * (1 + 2 * 2 + K * 5 * 2) + 4 * K * 3 * 2)
        for name, fn, nbytes in (('step_fused', fused, 3 * esz * n), ('step_fused_zbuf', fused_zbuf, 4 * esz * n),
                                 ('step_composed', composed, None), ('normal_fill', fill, esz * n),
                                 ('accumulate', accumulate, acc_bytes)):
            med, lo, hi = timed(fn, a.reps, a.windows)
            row = {'what': name, 'dtype': str(dtype).split('.')[-1], 'n': n, 'K': K, 'seconds': med, 'seconds_min': lo,
                   'seconds_max': hi, 'reps': a.reps, 'windows': a.windows, 'device': torch.cuda.get_device_name(0)}
            if nbytes is not None:
                row.update(bytes=nbytes, bytes_per_s=nbytes / med, share_of_6p3_TBps=nbytes / med / HBM_ACHIEVABLE)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del state, total, total_sq, x, g, z, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
