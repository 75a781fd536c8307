"""Time of one L1-ball projection on one GPU: pcs_thresh_l1 against a torch restatement of the same prox.

The case: n = 2^22 normal samples, radius r = 0.5 ||x||_1, fp32 and fp64.
  kernel  O.thresh_l1(x, r, 0, 'soft'): the 32-section descent of csrc/thresh.hip (19 launches fp32, 31 fp64),
          no host read-back
  torch   the reference's projection restated with torch ops on the same device: sort |x| descending, cumsum,
          the last k with |x|_(k) > (S_k - r) / k, then the soft threshold (the sort-based form of
          pycsou/math/prox.py:158-164; no host read-back either, so the comparison is launch for launch)
Both are warmed up at the timed shape, then timed with device events around `--calls` back-to-back calls,
`--reps` times each, alternating; the outputs are compared first (results must not differ beyond rounding).
Then both are captured, ten calls to a hipGraph, and the replays are timed the same way (`graph_*`: the form
in which the generic solver loop issues them).
One JSON line per dtype to stdout and to profiles/thresh_bench.jsonl: microseconds per call (min / median / max
over the repetitions), the ratio of the medians, and the algorithmic bytes of the kernel's passes over x
(a count from the shapes, not a measured rate).  A run without a GPU fails.

  python tools/bench_thresh.py --calls 200 --reps 5
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def torch_proj_l1(x, r):
    ax = x.abs()
    s, _ = torch.sort(ax, descending=True)
    cs = torch.cumsum(s.double(), 0)
    k = torch.arange(1, x.numel() + 1, device=x.device, dtype=torch.float64)
    tk = (cs - r) / k
    idx = torch.clamp((s.double() > tk).sum() - 1, min=0)  # the condition holds on a prefix: its last index
    t = tk.gather(0, idx.reshape(1))  # (tk[idx] would read idx back to the host)
    t = torch.where(cs[-1:] <= r, torch.zeros_like(t), t)
    return (torch.sign(x) * torch.clamp(ax.double() - t, min=0)).to(x.dtype)


def events(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # microseconds per call


def graphed(fn, per_graph=10):
    """`per_graph` calls of fn captured in one hipGraph (how the generic solver loop issues them): returns a
    callable that replays it.  Neither path reads anything back, so both capture."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    return g.replay


def stats(v):
    return {'min': round(min(v), 2), 'median': round(float(np.median(v)), 2), 'max': round(max(v), 2)}


def leg(dtype, n, calls, warmup, reps):
    from pycsou_amd import _ops as O
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(n, generator=g, device='cuda', dtype=dtype)
    r = 0.5 * float(x.abs().double().sum())
    kern = lambda: O.thresh_l1(x, r, 0.0, 'soft')  # noqa: E731
    ref = lambda: torch_proj_l1(x, r)              # noqa: E731
    a, b = kern(), ref()
    agree = float((a.double() - b.double()).abs().max())
    for _ in range(warmup):
        kern()
        ref()
    tk, tt, gk, gt = [], [], [], []
    for _ in range(reps):
        tk.append(events(kern, calls))
        tt.append(events(ref, calls))
    per = 10
    gkern, gref = graphed(kern, per), graphed(ref, per)
    assert torch.equal(kern(), a)
    for _ in range(3):
        gkern()
        gref()
    for _ in range(reps):
        gk.append(events(gkern, max(1, calls // per)) / per)
        gt.append(events(gref, max(1, calls // per)) / per)
    w = x.element_size()
    passes = (7 if dtype == torch.float32 else 13) + 2  # descent + statistics + active set, each one read of x
    out = {'case': 'proj_l1_ball', 'dtype': str(dtype).split('.')[-1], 'n': n, 'radius_over_l1': 0.5,
           'calls': calls, 'reps': reps, 'kernel_us': stats(tk), 'torch_sort_us': stats(tt),
           'torch_over_kernel': round(float(np.median(tt) / np.median(tk)), 2),
           'graph_kernel_us': stats(gk), 'graph_torch_sort_us': stats(gt),
           'graph_torch_over_kernel': round(float(np.median(gt) / np.median(gk)), 2), 'max_abs_diff': agree,
           'kernel_launches': 2 * passes + 1, 'kernel_bytes': (passes + 2) * n * w,
           'device': torch.cuda.get_device_name(0)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1 << 22)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'thresh_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_thresh: no GPU visible; nothing is measured without one')
    lines = [json.dumps(leg(dt, args.n, args.calls, args.warmup, args.reps)) for dt in (torch.float32, torch.float64)]
    for line in lines:
        print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
