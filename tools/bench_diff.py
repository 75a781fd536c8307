"""Times of the directional-derivative and cumulative-sum kernels on one GPU, against what the library could do
before them and against torch.

Cases, each in fp32 and fp64:
  dirderiv_fwd / dirderiv_adj   FirstDirectionalDerivative with a direction field at 4096 x 4096 (centred, edge):
          fused   one launch of pcs_dirderiv_fwd / pcs_dirderiv_adj
          composed   the same operator from the kernels the library had: pcs_grad_fwd, pcs_mul and an add
                  (forward); a tiled copy, pcs_mul and pcs_grad_adj (adjoint)
  cumsum_axis0 / cumsum_axis1   Integration1D along each axis of 4096 x 4096: pcs_cumsum against torch.cumsum
  cumsum_1d                     Integration1D of 2^24 samples: pcs_cumsum against torch.cumsum
Every pair is compared on the same seeded input first, warmed up at the timed shape, then timed with device
events around back-to-back calls, `--reps` windows each, alternating between the two.  A window holds at least
`--calls` calls and as many as fill `--window` seconds (0.5 by default; a short probe sizes it per leg).
What is timed is the CALL as a solver issues it -- the Python wrapper, its output allocation and the launches --
not the kernel alone; with the queue kept full by back-to-back calls the device time dominates, but a kernel
time needs a trace (rocprofv3 --kernel-trace --stats, in a run of its own).
One JSON line per case and dtype to stdout, appended to profiles/diff_family_bench.jsonl: microseconds per call
(min / median / max over the windows), the calls per window, the ratio of the medians, whether the two differ by
more than the spread of both, the algorithmic bytes (words per element from the shapes: fused forward 4 N,
adjoint 4 N, composition 12 N, scan 2 N unsplit and 3 N split) and `*_model_bytes_per_call_time_over_hbm_*`:
those bytes over the median call time, as a fraction of the HBM rate (8.0 TB/s datasheet peak; 6.29 TB/s is
what a float4 copy reaches).  At fp32 the 4096^2 working set (<= 256 MiB) fits the Infinity Cache, so a
fraction above 1 there is cache bandwidth, not an error.  A run without a GPU fails.

  python tools/bench_diff.py --reps 7
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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


def pair(case, dtype, ours, base, names, words, n_elem, calls, warmup, reps, tol, extra, window=0.5):
    a, b = ours(), base()
    diff = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    assert diff <= tol, (case, dtype, diff)
    del a, b
    for _ in range(warmup):
        ours()
        base()
    # calls per window: at least `calls`, and enough to fill `window` seconds (sized by a short probe)
    co = max(calls, int(np.ceil(window * 1e6 / events(ours, 20))))
    cb = max(calls, int(np.ceil(window * 1e6 / events(base, 20))))
    to, tb = [], []
    for _ in range(reps):
        to.append(events(ours, co))
        tb.append(events(base, cb))
    w = torch.empty(0, dtype=dtype).element_size()
    out = {'case': case, 'dtype': str(dtype).split('.')[-1], 'what': 'call time (wrapper + launches), device events',
           f'{names[0]}_calls_per_window': co, f'{names[1]}_calls_per_window': cb, 'reps': reps,
           f'{names[0]}_us': stats(to), f'{names[1]}_us': stats(tb),
           f'{names[1]}_over_{names[0]}': round(float(np.median(tb) / np.median(to)), 3),
           'separated': bool(max(to) < min(tb) or max(tb) < min(to)), 'max_rel_diff': diff}
    for name, t, k in ((names[0], to, words[0]), (names[1], tb, words[1])):
        if k is None:
            continue
        nbytes = k * n_elem * w
        rate = nbytes / (float(np.median(t)) * 1e-6)
        out[f'{name}_words_per_element'] = k
        out[f'{name}_bytes'] = nbytes
        out[f'{name}_model_bytes_per_call_time_over_hbm_peak'] = round(rate / HBM_PEAK, 3)
        out[f'{name}_model_bytes_per_call_time_over_hbm_copy_rate'] = round(rate / HBM_COPY, 3)
    out.update(extra)
    out['device'] = torch.cuda.get_device_name(0)
    return out


def run(args):
    from pycsou_amd import _lib as L
    from pycsou_amd import _ops as O
    lib = L.gpu()
    lines = []
    for dtype in (torch.float32, torch.float64):
        tol = 1e-5 if dtype == torch.float32 else 1e-12
        g = torch.Generator(device='cuda').manual_seed(1)
        dims = (args.side, args.side)
        N = dims[0] * dims[1]
        x = torch.randn(N, generator=g, device='cuda', dtype=dtype)
        v = torch.randn(2 * N, generator=g, device='cuda', dtype=dtype)
        steps = [1.0, 1.0]

        def fused_fwd():
            return O.dirderiv(x, v, True, dims, steps, 'centered', True)

        def comp_fwd():
            t = O.mul(O.grad_fwd(x, dims, steps, 'centered', True), v)
            return O.add(t[:N], t[N:])

        def fused_adj():
            return O.dirderiv(x, v, True, dims, steps, 'centered', True, adjoint=True)

        def comp_adj():
            return O.grad_adj(O.mul(x.repeat(2), v), dims, steps, 'centered', True)

        common = dict(shape=list(dims), working_set_bytes=4 * N * x.element_size())
        lines.append(pair('dirderiv_fwd', dtype, fused_fwd, comp_fwd, ('fused', 'composed'), (4, 12), N, args.calls,
                          args.warmup, args.reps, tol, common, args.window))
        # adjoint composition: tile 1 + 2, mul 2 + 2 + 2, grad_adj 2 + 1 words per element
        lines.append(pair('dirderiv_adj', dtype, fused_adj, comp_adj, ('fused', 'composed'), (4, 12), N, args.calls,
                          args.warmup, args.reps, tol, common, args.window))
        for axis in (0, 1):
            split = int(lib.pcs_cumsum_ws_bytes(2, L.i64s(dims), axis)) > 0
            lines.append(pair(f'cumsum_axis{axis}', dtype, lambda: O.cumsum(x, dims, axis, 1.0),
                              lambda: torch.cumsum(x.view(dims), dim=axis).view(-1), ('kernel', 'torch'),
                              (3 if split else 2, None), N, args.calls, args.warmup, args.reps, tol,
                              dict(shape=list(dims), split=split), args.window))
        del v
        n1 = args.n1d
        x1 = torch.randn(n1, generator=g, device='cuda', dtype=dtype)
        split = int(lib.pcs_cumsum_ws_bytes(1, L.i64s([n1]), 0)) > 0
        lines.append(pair('cumsum_1d', dtype, lambda: O.cumsum(x1, (n1,), 0, 1.0), lambda: torch.cumsum(x1, dim=0),
                          ('kernel', 'torch'), (3 if split else 2, None), n1, args.calls, args.warmup, args.reps,
                          1e-2 if dtype == torch.float32 else 1e-10, dict(shape=[n1], split=split), args.window))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=4096)
    ap.add_argument('--n1d', type=int, default=1 << 24)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--window', type=float, default=0.5, help='least seconds per timed window')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'diff_family_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_diff: no GPU visible; nothing is measured without one')
    lines = [json.dumps(r) for r in run(args)]
    for line in lines:
        print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
