"""PDS TV-deconvolution benchmark (BASELINE.json metric: PDS iters/sec on 4096^2
TV-deconv; achieved HBM GB/s vs roofline).

Workload: 4096 x 4096 piecewise-constant phantom, 15x15 Gaussian PSF
(sigma = 2 px, sum 1), y = h*x + 0.01 N(0,1); PDS with F = 1/2 ||Conv x - y||^2,
K = Gradient(kind='forward'), H = 0.05 * L21Norm (isotropic TV), fp32, built through the
public pycsou-style API and run by the fused engine (PDS2DEngine: chunks of iterations
launched back to back from C by pcs_pds2d_run).  One "step" = one PDS iteration = one launch
of the row-marching step kernel (update + norms + in-kernel stopping rule).

N > 1 (one process per GPU, torch.distributed over RCCL): the image is (4096 N) x 4096,
row-slab sharded, one 4096^2 slab per rank (weak scaling); every iteration exchanges
halo rows with the two neighbour ranks and all-reduces the four convergence norms.
`value` is the whole-job throughput in 4096^2-image PDS iterations per second
(= N x slab iterations/s).

Volume workloads in the same line (`volume_c4`, `volume_c5`: BASELINE configs[3], [4]): the
512^3 fp32 and the 1024^3 fp64 3-D
TV-deconvolution (three 15-tap Convolve1D, 3-D Gradient, 0.05 L21) plane-slab sharded over
the same N ranks (strong scaling: the whole volume at every N), PDS3DEngine with the banded
schedule (halo exchange and sums all-gather overlapped with the interior planes).  It runs
after the C3 measurement under a watchdog: if it fails or stalls, the C3 line is printed
without it.

Single-GPU 2-D legs in the same line (`c2`: BASELINE configs[1], 2048^2 fp32 TV denoising;
`c3_nonsep`: the C3 problem with a non-separable 15x15 PSF through the register-blocked
correlation kernel; `c2_lap` / `c2_cen`: 2048^2 denoising with a Laplacian / centered-Gradient K
on the general-stencil fused step), each with its own roofline.  The operator norms of the single-GPU 2-D
problems come from compute_lipschitz_cst() (device Lanczos, untimed setup) as in a reference
script; the multi-GPU and volume problems use the closed forms (documented in the line).

Counts: exactly --warmup untimed and --steps timed iterations (odd counts allowed).

A plain run (`bench.py --gpus N --steps K --warmup W`) does what the headline needs and no more:
it builds the problem, warms up, times the K iterations and prints the line (`value`,
`ms_per_step`, the loop-time roofline).  Everything else described above -- the CPU baseline, the
single-GPU 2-D legs, the volume legs, the isolated per-kernel timings and, at N > 1, the
communication probes and the strong-scaling entry -- runs after the headline only with `--full`
(their keys are absent or null in a plain line).

`--dump-outputs DIR` writes what the last timed iteration computed as DIR/x.npy, DIR/z.npy (the
primal and dual iterates, in the run's dtype) and DIR/diagnostics.npy (that iteration's two
relative-improvement norms, fp64); at N > 1 every rank writes its own rows as <name>_rank<r>.npy.
Outputs larger than 48 MiB in all are cut to a fixed seeded sample of their elements.  The
inputs are seeded, so two runs with the same arguments are compared file for file.

Prints ONE JSON line on rank 0.
"""

import argparse
import json
import os
import sys
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

METRIC = 'PDS iters/sec on 4096² TV-deconv; achieved HBM GB/s vs roofline at 1/2/4/8 GPU'
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md)
TRAFFIC_JSON = 'profiles/r6_profc3_traffic.json'  # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE of the step kernel (tools/prof_nm.sh r6_profc3)
DUMP_BUDGET = 48 << 20  # --dump-outputs: bytes of array data in all (larger outputs are sampled)
DUMP_WHOLE = 64 << 10  # arrays up to this many bytes are never sampled
DUMP_SEED = 20240607  # seed of the sample's indices


def phantom(shape, n_rect, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros(shape, dtype=np.float64)
    for _ in range(n_rect):
        lo = [rng.integers(0, s) for s in shape]
        hi = [min(s, l + rng.integers(max(1, s // 16), max(2, s // 3))) for s, l in zip(shape, lo)]
        x[tuple(slice(a, b) for a, b in zip(lo, hi))] = rng.uniform(0, 1)
    return x


def gaussian_psf(size=15, sigma=2.0):
    r = np.arange(size) - (size - 1) / 2
    g = np.exp(-0.5 * (r / sigma) ** 2)
    h = np.outer(g, g)
    return h / h.sum()


def aniso_psf(size=15, su=3.0, sv=1.2, angle=np.pi / 6):
    """Rotated anisotropic Gaussian (nonnegative, unit sum, rank > 1): the non-separable PSF of
    the c3_nonsep leg."""
    r = np.arange(size) - (size - 1) / 2
    yy, xx = np.meshgrid(r, r, indexing='ij')
    u = np.cos(angle) * xx + np.sin(angle) * yy
    v = -np.sin(angle) * xx + np.cos(angle) * yy
    h = np.exp(-0.5 * ((u / su) ** 2 + (v / sv) ** 2))
    return h / h.sum()


def build_problem(n0, n1, dtype, seed=0, psf=None, lipschitz='lanczos', kind='forward'):
    """The C3 problem through the public API (pycsou scripts look exactly like this).
    lipschitz='lanczos': K.compute_lipschitz_cst() / C.compute_lipschitz_cst() as a reference
    script does (device Lanczos, untimed setup); 'analytic': the closed forms (||grad_fwd|| from
    the Neumann-Laplacian spectrum, ||C|| <= 1 for a nonnegative unit-sum PSF)."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L21Norm
    from pycsou_amd.linop.conv import Convolve2D
    from pycsou_amd.linop.diff import Gradient
    from pycsou_amd.opt.proxalgs import PDS
    N = n0 * n1
    xs = torch.as_tensor(phantom((n0, n1), 64, seed).ravel()).to('cuda', dtype)
    C = Convolve2D(size=N, filter=gaussian_psf(15, 2.0) if psf is None else psf, shape=(n0, n1))
    K = Gradient(shape=(n0, n1), kind=kind)  # kind='centered': the reference's default Gradient(shape)
    if lipschitz == 'lanczos':
        C.compute_lipschitz_cst()
        K.compute_lipschitz_cst()
    else:
        C.lipschitz_cst = C.diff_lipschitz_cst = 1.0  # nonnegative PSF of unit sum: ||Conv|| <= 1
        # exact ||grad_fwd|| on an n0 x n1 grid (eigenvalues of the Neumann Laplacian)
        K.lipschitz_cst = K.diff_lipschitz_cst = float(np.sqrt(4 * np.sin(np.pi * (n0 - 1) / (2 * n0)) ** 2
                                                                + 4 * np.sin(np.pi * (n1 - 1) / (2 * n1)) ** 2))
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    y = C(xs) + 0.01 * torch.randn(N, generator=g, device='cuda', dtype=dtype)
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y) * C
    H = 0.05 * L21Norm(dim=2 * N, groups=np.tile(np.arange(N), 2))
    return PDS(dim=N, F=F, H=H, K=K, x0=torch.zeros(N, dtype=dtype, device='cuda'),
               z0=torch.zeros(2 * N, dtype=dtype, device='cuda'), verbose=None)


def build_denoise(n, dtype, seed=0, lipschitz='lanczos'):
    """C2 (BASELINE configs[1]): 2-D TV denoising n x n, F = 1/2 ||x - y||^2, K = Gradient(forward),
    H = 0.1 * L21Norm (isotropic TV), fp32."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L21Norm
    from pycsou_amd.linop.diff import Gradient
    from pycsou_amd.opt.proxalgs import PDS
    N = n * n
    xs = torch.as_tensor(phantom((n, n), 64, seed).ravel()).to('cuda', dtype)
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    y = xs + 0.1 * torch.randn(N, generator=g, device='cuda', dtype=dtype)
    K = Gradient(shape=(n, n), kind='forward')
    if lipschitz == 'lanczos':
        K.compute_lipschitz_cst()
    else:
        K.lipschitz_cst = K.diff_lipschitz_cst = float(np.sqrt(8 * np.sin(np.pi * (n - 1) / (2 * n)) ** 2))
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y)
    H = 0.1 * L21Norm(dim=2 * N, groups=np.tile(np.arange(N), 2))
    return PDS(dim=N, F=F, H=H, K=K, x0=torch.zeros(N, dtype=dtype, device='cuda'),
               z0=torch.zeros(2 * N, dtype=dtype, device='cuda'), verbose=None)


def build_denoise_k(n, dtype, kind, seed=0, lipschitz='lanczos'):
    """2-D denoising n x n fp32 with a non-forward K through the general-stencil fused step:
    kind 'lap': K = Laplacian(edge=True), H = 0.1 * L1Norm (one component per pixel);
    kind 'centered': K = Gradient(kind='centered', edge=True) (the reference's default Gradient),
    H = 0.1 * L21Norm (isotropic TV).  ||K|| from compute_lipschitz_cst() (device Lanczos) as a
    reference script does, or the closed-form bounds (8, 2) with lipschitz='analytic'."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm, L21Norm
    from pycsou_amd.linop.diff import Gradient, Laplacian
    from pycsou_amd.opt.proxalgs import PDS
    N = n * n
    xs = torch.as_tensor(phantom((n, n), 64, seed).ravel()).to('cuda', dtype)
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    y = xs + 0.1 * torch.randn(N, generator=g, device='cuda', dtype=dtype)
    if kind == 'lap':
        K = Laplacian(shape=(n, n), edge=True)
        H, hdim = 0.1 * L1Norm(dim=N), N
    else:
        K = Gradient(shape=(n, n), kind='centered', edge=True)
        H, hdim = 0.1 * L21Norm(dim=2 * N, groups=np.tile(np.arange(N), 2)), 2 * N
    if lipschitz == 'lanczos':
        K.compute_lipschitz_cst()
    else:
        K.lipschitz_cst = K.diff_lipschitz_cst = 8.0 if kind == 'lap' else 2.0
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y)
    return PDS(dim=N, F=F, H=H, K=K, x0=torch.zeros(N, dtype=dtype, device='cuda'),
               z0=torch.zeros(hdim, dtype=dtype, device='cuda'), verbose=None)


def cpu_baseline(n, iters):
    """The reference CPU op sequence (oracle restatement: NumPy temporaries, SciPy FFT
    convolution, np.linalg.norm diagnostics into a pandas DataFrame, deepcopy of the
    iterand) on the same C3 problem at full size, fp64 (the reference default)."""
    from oracle import pycsou_ref as OR
    from oracle import pylops1 as P
    N = n * n
    xs = phantom((n, n), 64, 0).ravel()
    h = gaussian_psf(15, 2.0)
    Cr = P.Convolve2D(N, h, (n, n), offset=(7, 7), method='fft')
    y = Cr.matvec(xs) + 0.01 * np.random.default_rng(1).standard_normal(N)
    Kr = P.Gradient((n, n), edge=True, kind='forward')
    Klip = float(np.sqrt(8 * np.sin(np.pi * (n - 1) / (2 * n)) ** 2))
    tau, sigma = OR.pds_step_sizes(1.0, Klip)
    hprox = OR.postcomp(lambda v, t: OR.prox_l21_pixel(v, t, 2), 0.05)
    t0 = time.perf_counter()
    OR.pds(lambda x: Cr.rmatvec((2 * (Cr.matvec(x) + (-y))) * 0.5), lambda v, t: v, Kr.matvec, Kr.rmatvec,
           lambda w, s: OR.fenchel_prox(hprox, w, s), tau, sigma, 0.9, np.zeros(N), np.zeros(2 * N),
           max_iter=iters - 1, min_iter=iters - 1, accuracy_threshold=0.0, pandas_diagnostics=True)
    dt = time.perf_counter() - t0
    return {'value': iters / dt, 'unit': 'it/s', 'cores': 1, 'kind': 'port', 'host_cpus': os.cpu_count(),
            'validation': 'this restatement ran 0.80-0.96x the real reference time per iteration (0.94x at '
                          '4096^2), identical iterates, on 512^2-4096^2 (anisotropic-L1 variant; '
                          'tests/golden/cpu_baseline_check.json); '
                          'the reference isotropic L21 is an O(G N) Python loop: 0.88 s/iter at 128^2, '
                          'extrapolated ~9e5 s/iter at 4096^2, so the L21 prox here is vectorised',
            'sample': f'{iters} PDS iterations of the same 4096x4096 TV-deconvolution (fp64, reference op '
                      f'sequence incl. SciPy FFT convolution, vectorised pixel-L21, pandas diagnostics, deepcopy) '
                      f'in {dt:.1f} s on 1 host core'}


def build_volume(n, dtype, seed=0, kind='forward'):
    """C5 through the public API: a piecewise-constant n^3 phantom blurred by a 15-tap
    Gaussian (sigma 2) along each axis (Convolve1D x 3), y = h*x + 0.01 N(0,1), PDS with the
    3-D Gradient (kind='forward', or the reference's default 'centered') and 0.05 L21Norm
    (isotropic TV)."""
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L21Norm
    from pycsou_amd.linop.conv import Convolve1D
    from pycsou_amd.linop.diff import Gradient
    from pycsou_amd.opt.proxalgs import PDS
    shape = (n, n, n)
    N = n ** 3
    xs = torch.zeros(shape, dtype=dtype, device='cuda')
    rng = np.random.default_rng(seed)
    for _ in range(32):
        lo = rng.integers(0, n, 3)
        hi = np.minimum(n, lo + rng.integers(n // 16, n // 3, 3))
        xs[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = float(rng.uniform(0, 1))
    r = np.arange(15) - 7
    taps = np.exp(-0.5 * (r / 2.0) ** 2)
    taps /= taps.sum()
    C = None
    for ax in range(3):
        Ci = Convolve1D(N, taps, reshape_dims=shape, axis=ax)
        Ci.lipschitz_cst = Ci.diff_lipschitz_cst = 1.0
        C = Ci if C is None else Ci * C
    C.lipschitz_cst = C.diff_lipschitz_cst = 1.0
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    y = C(xs.reshape(-1)) + 0.01 * torch.randn(N, generator=g, device='cuda', dtype=dtype)
    del xs
    K = Gradient(shape=shape, kind=kind)
    if kind == 'forward':
        K.lipschitz_cst = K.diff_lipschitz_cst = float(np.sqrt(3 * 4 * np.sin(np.pi * (n - 1) / (2 * n)) ** 2))
    else:  # Schur bound per axis: rows sum to <= 2, columns to <= 1.5 -> ||D|| <= sqrt(3), ||K|| <= 3
        K.lipschitz_cst = K.diff_lipschitz_cst = 3.0
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y) * C
    H = 0.05 * L21Norm(dim=3 * N, groups=np.tile(np.arange(N), 3))
    return PDS(dim=N, F=F, H=H, K=K, x0=torch.zeros(N, dtype=dtype, device='cuda'),
               z0=torch.zeros(3 * N, dtype=dtype, device='cuda'), verbose=None)


def volume_bench(n, dtype, K, W, world, rank, kind='forward'):
    """C4 / C5: the whole n^3 volume plane-slab sharded over `world` ranks; K timed iterations
    (barrier + synchronize on both sides, max over ranks)."""
    from pycsou_amd.opt.engine3d import PDS3DEngine
    from pycsou_amd.parallel import DistComm
    from pycsou_amd.parallel.slab import comm_probe
    t0 = time.perf_counter()
    pds = build_volume(n, dtype, kind=kind)
    spec = pds._fused_spec()
    assert spec is not None and spec.get('ndim') == 3, 'C5 problem must take the fused 3-D engine'
    comm = DistComm() if world > 1 else None
    eng = PDS3DEngine(spec, dtype, pds.tau, pds.sigma, pds.rho, pds.x0, pds.z0, comm=comm, rank=rank,
                      world=world, chunk=2)
    del pds, spec
    torch.cuda.empty_cache()
    # iteration budget of the device loop control: the warmup, the timed iterations and the
    # multi-GPU schedule trial (up to 8 eager iterations inside the first advance), with slack, so
    # no timed launch finds the loop already stopped
    total = W + K + 24
    eng.init_loop(total, total, -1.0)
    eng.advance(W)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    eng.advance(K)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    assert eng.iterations() == W + K, (eng.iterations(), W, K)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device='cuda' if dist.get_backend() == 'nccl' else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # after the timed region: the compute, the sums all-gather and the halo exchange timed apart
    # (idempotent re-runs on the final iterate, max over ranks), so a scaling run explains itself
    probe = comm_probe(eng) if world > 1 else None
    ms = dt * 1e3 / K
    elem = torch.empty(0, dtype=dtype).element_size()
    # the launches of one iteration timed apart (HIP events, eager, after the timed region) and the
    # roofline of each: algorithmic words per voxel -- nrm: read x, write t (2); conv0: read t and
    # C12^T y, write g (3); update: x, g, z (3) in, x', z' (3) out (9), with the axis-0 pass folded in
    # x, t, C12^T y, z (3) in (10)
    parts, roof = None, None
    if world == 1:
        parts = eng.time_parts(3)
        fold = bool(getattr(eng, 'fold', False))
        words = {'nrm': 2, 'conv0': 3, 'step': 10 if fold else 9}
        upd = 'k_pds3d' if kind == 'forward' else 'k_pds3d_gen'
        names = {'nrm': f'k_sep2d_{"nrm" if elem == 4 else "nrmm"}<{"float" if elem == 4 else "double"}>',
                 'conv0': f'k_conv0_rta<{"float" if elem == 4 else "double"},15>',
                 'step': f'{upd}<{"float" if elem == 4 else "double"}{", PCS_F_CONV0" if fold else ""}>'}
        per = {}
        for k, t in parts.items():
            if k in words:
                gbs = words[k] * n ** 3 * elem / (t * 1e-3) / 1e9
                per[k] = {'kernel': names[k], 'kernel_ms': round(t, 4), 'words_per_voxel': words[k],
                          'achieved': round(gbs, 1), 'frac': round(gbs / HBM_PEAK_GBS, 4)}
        if 'step' in per:
            s = per['step']
            roof = {'bound': 'hbm', 'kernel': s['kernel'], 'kernel_ms': s['kernel_ms'], 'achieved': s['achieved'],
                    'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': s['frac'], 'parts': per,
                    'words_per_voxel_iteration': sum(words[k] for k in per),
                    'source': 'HIP-event pairs around each launch of 3 eager iterations after the timed region'}
    alg = 9 * n ** 3 * elem  # (2d+3) N words, d = 3: read x, z (3N), y; write x', z' (3N)
    halo = 0 if world == 1 else eng.halo_planes * eng.plane * elem
    res = {'workload': f'{"C5" if elem == 8 else "C4"} 3-D TV-deconvolution {n}^3 {"f64" if elem == 8 else "f32"}, 15-tap Gaussian per axis '
                       f'(Convolve1D x3), 3-D Gradient(kind={kind}), 0.05*L21Norm, PDS3DEngine '
                       f'({"k_pds3d" if kind == "forward" else "k_pds3d_gen"} update), '
                       f'{world} plane slab(s) (strong scaling: whole volume at every N)',
           'it_per_s': round(1e3 / ms, 3), 'ms_per_iter': round(ms, 4), 'steps': K, 'warmup': W,
           'iteration_GBps': round(alg / (ms * 1e-3) / 1e9, 1),
           'iteration_frac_of_hbm_peak_per_gpu': round(alg / (ms * 1e-3) / 1e9 / (HBM_PEAK_GBS * world), 4),
           'alg_bytes_per_iter': alg, 'halo_bytes_per_side_per_iter': halo,
           'axis0_folded': bool(getattr(eng, 'fold', False)),  # axis-0 pass inside k_pds3d (13 words/voxel)
           'banded_overlap': bool(getattr(eng, 'banded', False) and eng.overlap),
           'banded_order': ((eng.order if eng.overlap else 'serial') if getattr(eng, 'banded', False) else None)
                           if world > 1 else None,
           'order_trial_ms': getattr(eng, 'tune_ms', None),
           'comm': probe,
           'roofline': roof,
           'setup_s': round(t1 - t0, 1)}
    del eng
    if comm is not None:
        comm.close()
    torch.cuda.empty_cache()
    return res


def spin_up(eng, n_launch, min_ms=60.0):
    """Untimed, before the W warmup steps: launch the step kernel until the GPU has been busy
    for >= min_ms.  Clocks ramp over the first ~10-15 ms of sustained load (rocprofv3 traces:
    the first ~80 launches of a cold run take 10-25 % longer than the steady state)."""
    busy = 0.0
    while busy < min_ms:
        busy += n_launch * eng.time_step_kernel(n_launch)


def spin_up_fixed(eng, min_ms=200.0):
    """spin_up for a prepare_fixed() engine: whole iterations (every kernel of one), back to
    back, until the GPU has been busy >= min_ms; the caller re-prepares the loop state
    afterwards."""
    busy = 0.0
    while busy < min_ms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.advance_fixed(50)
        e1.record()
        torch.cuda.synchronize()
        busy += e0.elapsed_time(e1)


def dump_outputs(dirname, arrays, budget=DUMP_BUDGET):
    """--dump-outputs: write each of `arrays` (name -> tensor or ndarray, fp32 or fp64 as computed) as
    DIR/<name>.npy.  When they hold more than `budget` bytes together, every array above DUMP_WHOLE
    bytes is cut in proportion to a fixed sample of its flattened elements: indices drawn with a fixed
    seed, sorted, the same in every run with the same shapes, so two builds are compared element for
    element."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: torch.as_tensor(v).reshape(-1) for k, v in arrays.items()}
    nbytes = {k: t.numel() * t.element_size() for k, t in arrays.items()}
    total = sum(nbytes.values())
    small = sum(b for b in nbytes.values() if b <= DUMP_WHOLE)  # short arrays (the diagnostics) stay whole
    for i, (name, t) in enumerate(arrays.items()):
        if total > budget and nbytes[name] > DUMP_WHOLE:
            m = max(1, int(t.numel() * ((budget - small) / (total - small))))
            idx = np.sort(np.random.default_rng([DUMP_SEED, i]).integers(0, t.numel(), m))
            t = t[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(dirname, f'{name}.npy'), t.cpu().numpy())


def fused_2d(pds, dtype, K, W, chunk=32, kernels=True, outputs=False):
    """Exactly W untimed then K timed iterations of a fused 2-D problem (PDS2DEngine, fixed
    count); HIP events on the launch stream bracket the K iterations.  Returns ms per
    iteration, the engine facts and, with `kernels`, the isolated per-kernel launch medians (a run
    of their own after the timed region); with `outputs`, copies of what the last timed iteration
    left (x, z and its row of the convergence diagnostics) under 'outputs'."""
    from pycsou_amd import _ops as O
    from pycsou_amd.opt.engine import engine_class
    spec = pds._fused_spec()
    assert spec is not None, 'problem must take the fused 2-D engine'
    eng = engine_class(spec)(spec, dtype, pds.tau, pds.sigma, pds.rho, O.to_dev(pds.x0, dtype), O.to_dev(pds.z0, dtype))
    total = W + K + 4
    state = [b for b in (eng.X, eng.Z, getattr(eng, 'ZM', None)) if b is not None]
    init = [b[0].clone() for b in state]
    eng.prepare_fixed(max(total, 4000), chunk)
    spin_up_fixed(eng)
    # the spin-up iterates for a time, not a count: back to the initial iterate, so the W + K
    # iterations below compute the same thing in every run
    for b, b0 in zip(state, init):
        b[0].copy_(b0)
    del init
    eng.prepare_fixed(total, chunk)  # fresh loop state: exactly W + K iterations below
    eng.advance_fixed(W)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    eng.advance_fixed(K)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / K
    it_done = int(eng.ctrl.view(torch.int32)[0].item())
    assert it_done == W + K, (it_done, W, K)  # every timed launch really iterated
    out = None
    if outputs:
        p = eng._fixed_p  # the buffers the last timed iteration wrote
        out = {'x': eng.X[p].clone(), 'z': eng.Z[p].clone(),
               'diagnostics': eng.hist[2 * (it_done - 1):2 * it_done].clone()}
    # per-kernel means: an event pair around each launch of 100 eager iterations (after the
    # timed region; the rocprofv3 kernel-trace averages in profiles/ must agree)
    kern = eng.time_iteration_kernels(min(max(K, 20), 100)) if kernels else None
    res = {'ms_per_step': ms, 'kernels_ms': kern, 'nblocks': eng.nblocks, 'native': eng.native,
           'fkind': int(eng.fkind), 'nmarch': getattr(eng, 'cty', None) is not None, 'outputs': out}
    del eng
    torch.cuda.empty_cache()
    return res


def leg_c2(args, dtype, K, W):
    """C2 (BASELINE configs[1]) 2048^2 fp32 TV denoising: it/s and the step kernel against the
    HBM roofline (7 N words per iteration)."""
    n = 2048
    t0 = time.perf_counter()
    pds = build_denoise(n, dtype, lipschitz=args.lipschitz)
    setup = time.perf_counter() - t0  # problem build incl. compute_lipschitz_cst (device Lanczos)
    r = fused_2d(pds, dtype, K, W)
    del pds
    elem = 4 if dtype == torch.float32 else 8
    alg = 7 * n * n * elem
    km = r['kernels_ms']['step']
    return {'workload': f'C2 TV denoising {n}x{n} {args.dtype}, Gradient(kind=forward), 0.1*L21Norm, '
                        f'PDS fused step (pcs_pds2d_step, row-marching pointwise-F kernel)',
            'it_per_s': round(1e3 / r['ms_per_step'], 1), 'ms_per_iter': round(r['ms_per_step'], 5),
            'steps': K, 'warmup': W, 'alg_bytes_per_iter': alg, 'setup_s': round(setup, 2),
            'iteration_frac_of_hbm_peak': round(alg / (r['ms_per_step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            'roofline': {'bound': 'hbm', 'kernel': 'pcs_pds2d_step (k_pds2d_pt<DENOISE,L21>)', 'kernel_ms': round(km, 5),
                         'achieved': round(alg / (km * 1e-3) / 1e9, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                         'frac': round(alg / (km * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}


def _leg_stencil(args, dtype, K, W, kind):
    n = 2048
    t0 = time.perf_counter()
    pds = build_denoise_k(n, dtype, kind, lipschitz=args.lipschitz)
    setup = time.perf_counter() - t0
    r = fused_2d(pds, dtype, K, W)
    del pds
    elem = 4 if dtype == torch.float32 else 8
    words = 5 if kind == 'lap' else 7  # read x, y, z (1 or 2 components); write x', z'
    alg = words * n * n * elem
    km = r['kernels_ms']['step']
    kdesc = 'Laplacian(edge=True), 0.1*L1Norm' if kind == 'lap' else 'Gradient(kind=centered, edge=True), 0.1*L21Norm'
    return {'workload': f'2-D denoising {n}x{n} {args.dtype}, K = {kdesc}, PDS fused general-stencil step '
                        f'(row-marching k_pds2d_smarch through pcs_pds2d_step), iterations launched back to back from C',
            'it_per_s': round(1e3 / r['ms_per_step'], 1), 'ms_per_iter': round(r['ms_per_step'], 5),
            'steps': K, 'warmup': W, 'alg_bytes_per_iter': alg, 'setup_s': round(setup, 2),
            'iteration_frac_of_hbm_peak': round(alg / (r['ms_per_step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            'roofline': {'bound': 'hbm', 'kernel': f'pcs_pds2d_step (k_pds2d_smarch<{kind}, DENOISE>)',
                         'kernel_ms': round(km, 5), 'achieved': round(alg / (km * 1e-3) / 1e9, 1),
                         'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': round(alg / (km * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}


def leg_c2_lap(args, dtype, K, W):
    """2048^2 fp32 denoising with K = Laplacian (north_star's second operator family) on the
    general-stencil fused step: 5 N words per iteration."""
    return _leg_stencil(args, dtype, K, W, 'lap')


def leg_c2_cen(args, dtype, K, W):
    """2048^2 fp32 TV denoising with the reference's default Gradient (kind='centered',
    edge=True) on the general-stencil fused step: 7 N words per iteration."""
    return _leg_stencil(args, dtype, K, W, 'centered')


def leg_c3_nonsep(args, dtype, K, W):
    """The C3 problem with a NON-separable 15x15 PSF (rotated anisotropic Gaussian, rank > 1):
    per iteration r = h*x - y and g = h^T r by the register-blocked correlation kernel
    (pcs_conv2d_planned, fp32-vector bound: 2 x 225 FMA per pixel), then the fused update
    with grad F read from g (pcs_pds2d_step, GRADBUF); the three launches per iteration are
    replayed from a captured hipGraph."""
    n = args.size
    t0 = time.perf_counter()
    pds = build_problem(n, n, dtype, psf=aniso_psf(), lipschitz=args.lipschitz)
    setup = time.perf_counter() - t0
    r = fused_2d(pds, dtype, K, W)
    del pds
    elem = 4 if dtype == torch.float32 else 8
    N = n * n
    alg = 7 * N * elem
    km = r['kernels_ms']
    conv_flop = 2 * 225 * N  # one pass: 225 FMA per pixel
    conv_ms = 0.5 * (km['conv_fwd'] + km['conv_adj'])
    return {'workload': f'C3 TV-deconvolution {n}x{n} {args.dtype}, NON-separable 15x15 PSF (rotated '
                        f'anisotropic Gaussian 3.0/1.2 px, 30 deg, rank > 1), Gradient(kind=forward), 0.05*L21Norm; '
                        f'conv r = h*x - y, g = h^T r (pcs_conv2d_planned x2) + fused update (GRADBUF), hipGraph-replayed',
            'it_per_s': round(1e3 / r['ms_per_step'], 1), 'ms_per_iter': round(r['ms_per_step'], 5),
            'steps': K, 'warmup': W, 'kernels_ms': {k: round(v, 5) for k, v in km.items()},
            'alg_bytes_per_iter': alg, 'setup_s': round(setup, 2),
            'iteration_frac_of_hbm_peak': round(alg / (r['ms_per_step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            'roofline': {'bound': 'fp32-vector', 'kernel': 'pcs_conv2d_planned (k_corr2d<float,15>)',
                         'kernel_ms': round(conv_ms, 5), 'achieved': round(conv_flop / (conv_ms * 1e-3) / 1e12, 2),
                         'peak': 157.3, 'unit': 'TFLOP/s',
                         'frac': round(conv_flop / (conv_ms * 1e-3) / 1e12 / 157.3, 4),
                         'flop_per_launch': conv_flop},
            'update_roofline': {'bound': 'hbm', 'kernel': 'pcs_pds2d_step (k_pds2d_pt<GRADBUF,L21>)',
                                'kernel_ms': round(km['step'], 5),
                                'achieved': round(alg / (km['step'] * 1e-3) / 1e9, 1), 'peak': HBM_PEAK_GBS,
                                'unit': 'GB/s', 'frac': round(alg / (km['step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}


def leg_c3_cen(args, dtype, K, W):
    """The C3 problem with the reference's DEFAULT K = Gradient(shape) (kind='centered', edge=True,
    pycsou/linop/diff.py:777-778): grad F = N x - Conv^T y with N = Conv^T Conv as two 29-tap passes
    inside the row-marching step (the normal-operator march generalised to centred K, one launch per
    iteration: reads x, Conv^T y, z; writes x', z' -- 7 words, as the forward-K headline kernel); with
    PCS_NMARCH_GEN=0 the two-launch form (N x by k_sep2d_nrm into a buffer, then the stencil march)."""
    n = args.size
    t0 = time.perf_counter()
    pds = build_problem(n, n, dtype, lipschitz=args.lipschitz, kind='centered')
    setup = time.perf_counter() - t0
    r = fused_2d(pds, dtype, K, W)
    del pds
    elem = 4 if dtype == torch.float32 else 8
    N = n * n
    alg = 7 * N * elem
    km = r['kernels_ms']
    two = 'conv_nx' in km
    res = {'workload': f'C3 TV-deconvolution {n}x{n} {args.dtype}, 15x15 Gaussian PSF (separable), '
                       f'K = Gradient(shape) (default kind=centered, edge=True), 0.05*L21Norm; grad F = N x - Conv^T y'
                       + (': N x by k_sep2d_nrm into a buffer + general-stencil march step (k_pds2d_smarch), two '
                          'launches per iteration' if two else
                          ', N inside the step (k_pds2d_nmarch_gen<centered>), one launch per iteration')
                       + ', back to back from C',
           'it_per_s': round(1e3 / r['ms_per_step'], 1), 'ms_per_iter': round(r['ms_per_step'], 5),
           'steps': K, 'warmup': W, 'setup_s': round(setup, 2), 'fkind': r['fkind'],
           'kernels_ms': {k: round(v, 5) for k, v in km.items()}, 'alg_bytes_per_iter': alg,
           'iteration_frac_of_hbm_peak': round(alg / (r['ms_per_step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    if two:
        upd = km['step'] - km['conv_nx']
        step_bytes = 8 * N * elem  # the update kernel's own traffic: x, N x, Conv^T y, z (2) in; x', z' (2) out
        res['roofline'] = {'bound': 'hbm', 'kernel': 'k_pds2d_smarch<centered, NB, L21> (update)',
                           'kernel_ms': round(upd, 5), 'bytes_per_launch': step_bytes,
                           'achieved': round(step_bytes / (upd * 1e-3) / 1e9, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                           'frac': round(step_bytes / (upd * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        res['nx_roofline'] = {'bound': 'lds/fp32-vector', 'kernel': 'pcs_conv2d_sep_ata_planes (k_sep2d_nrm)',
                              'kernel_ms': round(km['conv_nx'], 5), 'flop_per_launch': 116 * N,
                              'tflops': round(116 * N / (km['conv_nx'] * 1e-3) / 1e12, 2)}
    else:
        res['roofline'] = {'bound': 'hbm', 'kernel': 'pcs_pds2d_step (k_pds2d_nmarch_gen<float,7,L21,256,centered>)',
                           'kernel_ms': round(km['step'], 5), 'bytes_per_launch': alg,
                           'achieved': round(alg / (km['step'] * 1e-3) / 1e9, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                           'frac': round(alg / (km['step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           'conv_flop_per_launch': 116 * N,
                           'conv_tflops': round(116 * N / (km['step'] * 1e-3) / 1e12, 2)}
    return res


def leg_c3_f64(args, dtype, K, W, kind='forward'):
    """C3 at the reference's default precision, fp64 (x0 / z0 np.float, pycsou/opt/proxalgs.py:327,341;
    Gradient / Convolve2D dtype='float64', linop/diff.py:777, linop/conv.py:167): 4096^2, the same
    separable 15x15 blur.  fp64 takes the general-stencil engine's fp64 row march for every K kind:
    grad F = N x - Conv^T y by k_sep2d_nrm<double> into a buffer (reads x, Conv^T y; writes grad F), then
    the march step (k_pds2d_smarch<double>, GRADBUF: reads x, grad F, z; writes x', z' -- 7 words;
    PCS_NX_SUB=0: N x alone, 2 words, and the subtraction in the step, 8 words).  Algorithmic bytes of
    the iteration: 7 words x 8 B per pixel."""
    n = args.size
    dt = torch.float64
    t0 = time.perf_counter()
    pds = build_problem(n, n, dt, lipschitz=args.lipschitz, kind=kind)
    setup = time.perf_counter() - t0
    r = fused_2d(pds, dt, K, W)
    del pds
    N = n * n
    alg = 7 * N * 8
    km = r['kernels_ms']
    sub = os.environ.get('PCS_NX_SUB', '1') != '0'
    fused = 'conv_nx' not in km
    res = {'workload': f'C3 TV-deconvolution {n}x{n} f64 (the reference default dtype), 15x15 Gaussian PSF (separable), '
                       f'K = Gradient(kind={kind}), 0.05*L21Norm; grad F = N x - Conv^T y: '
                       + ('N inside the step, ONE launch per iteration (k_pds2d_nmarch64, the fused fp64 '
                          'normal-operator march)' if fused else
                          ('grad F by k_sep2d_nrmm<double> (N x minus Conv^T y as it stores) into a buffer'
                           if sub else 'N x by k_sep2d_nrmm<double> into a buffer')
                          + ' + the fp64 general-stencil march step (k_pds2d_smarch<double>)')
                       + ', back to back from C',
           'it_per_s': round(1e3 / r['ms_per_step'], 1), 'ms_per_iter': round(r['ms_per_step'], 5),
           'steps': K, 'warmup': W, 'setup_s': round(setup, 2), 'dtype': 'f64',
           'kernels_ms': {k: round(v, 5) for k, v in km.items()}, 'alg_bytes_per_iter': alg,
           'iteration_frac_of_hbm_peak': round(alg / (r['ms_per_step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    if 'conv_nx' in km:
        # the update's time = the iteration's minus N x timed alone (without the Conv^T y subtraction the
        # in-iteration launch adds: the update is if anything under-credited)
        upd = km['step'] - km['conv_nx']
        step_bytes = (7 if sub else 8) * N * 8
        res['roofline'] = {'bound': 'hbm', 'kernel': f'k_pds2d_smarch<double, {kind}, {"GRADBUF" if sub else "NB"}, L21> (update)',
                           'kernel_ms': round(upd, 5), 'bytes_per_launch': step_bytes,
                           'achieved': round(step_bytes / (upd * 1e-3) / 1e9, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                           'frac': round(step_bytes / (upd * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        res['nx_roofline'] = {'bound': 'hbm', 'kernel': 'pcs_conv2d_sep_ata_planes (k_sep2d_nrmm<double>, timed alone)',
                              'kernel_ms': round(km['conv_nx'], 5), 'bytes_per_launch': 2 * N * 8,
                              'achieved': round(2 * N * 8 / (km['conv_nx'] * 1e-3) / 1e9, 1),
                              'frac': round(2 * N * 8 / (km['conv_nx'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    else:
        res['roofline'] = {'bound': 'hbm', 'kernel': f'pcs_pds2d_step (k_pds2d_nmarch64<7, L21, {kind}>)',
                           'kernel_ms': round(km['step'], 5), 'bytes_per_launch': alg,
                           'achieved': round(alg / (km['step'] * 1e-3) / 1e9, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                           'frac': round(alg / (km['step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           'conv_flop_per_launch': 116 * N,
                           'conv_tflops_fp64': round(116 * N / (km['step'] * 1e-3) / 1e12, 2)}
    return res


def leg_c3_cen_f64(args, dtype, K, W):
    """leg_c3_f64 with the reference's default K = Gradient(shape) (centred, edge=True)."""
    return leg_c3_f64(args, dtype, K, W, kind='centered')


def leg_conv63(args, dtype, K, W):
    """Convolve2D with a 63 x 63 non-separable PSF on a 4096^2 image (the reference's default
    method='fft', pycsou/linop/conv.py:209-217, 294): one forward and one adjoint pass through the
    FFT-domain plan (pcs_fftconv2d: pad, rocFFT R2C, spectrum product, C2R, crop), HIP events
    around each of `reps` passes on the launch stream; the cost no longer grows with the PSF."""
    from pycsou_amd.linop.conv import Convolve2D
    n = args.size
    r = np.arange(63) - 31.0
    yy, xx = np.meshgrid(r, r, indexing='ij')
    h = np.exp(-0.5 * ((xx * 0.8 + yy * 0.6) ** 2 / 90.0 + (yy * 0.8 - xx * 0.6) ** 2 / 20.0))
    h /= h.sum()
    C = Convolve2D(n * n, h, (n, n))
    x = torch.randn(n * n, device='cuda', dtype=dtype)
    f = C.fft(dtype)
    out = torch.empty_like(x)
    reps = max(10, min(K, 50))
    st = torch.cuda.current_stream()
    res = {}
    for name, adj in (('forward', False), ('adjoint', True)):
        for _ in range(3):
            f.apply(x, adjoint=adj, out=out)
        evs = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            f.apply(x, adjoint=adj, out=out)
            e1.record(st)
            evs.append((e0, e1))
        torch.cuda.synchronize()
        res[name] = float(np.median([a.elapsed_time(b) for a, b in evs]))
    lib_grid = int(C.fft(dtype)._lib.pcs_fftconv2d_grid(n, 63))
    return {'workload': f'Convolve2D {n}x{n} {args.dtype}, 63x63 non-separable PSF, FFT-domain plan '
                        f'(padded grid {lib_grid}^2, rocFFT R2C/C2R + pad / spectrum-product / crop kernels)',
            'ms_per_pass': {k: round(v, 5) for k, v in res.items()}, 'reps': reps,
            'direct_flop_equiv_tflops': round(2 * 63 * 63 * n * n / (res['forward'] * 1e-3) / 1e12, 1)}


def leg_cps_inpaint(args, dtype, K, W):
    """The reference notebook's TV-LAD inpainting (CPS, K = LinOpVStack(Masking 50 %, Gradient(forward)),
    H = ProxFuncHStack(L1Loss, mu L1Norm), G = Segment) at 2048^2: ONE launch per iteration (the masked
    block inside the general-stencil row march, PCS_M_L1LOSS: PDS2DMaskEngine), timed as every fused 2-D
    leg (HIP events around the K back-to-back iterations after W warm-up ones, steady state).
    Algorithmic bytes: read x, z_s (2N), y and z_m (m each); write x', z_s', z_m' -- the engine moves
    9 N words (z_m and y expanded to the image)."""
    from pycsou_amd.func import L1Loss, L1Norm, ProxFuncHStack, Segment
    from pycsou_amd.linop import Gradient, LinOpVStack, Masking
    from pycsou_amd.opt import CPS
    n = 2048
    N = n * n
    rng = np.random.default_rng(5)
    mask = rng.random(N) < 0.5
    img = phantom((n, n), 12, 5).ravel()
    npdt = np.float32 if dtype == torch.float32 else np.float64
    t0 = time.perf_counter()
    y = torch.from_numpy(img[mask].astype(npdt)).cuda()
    m = int(mask.sum())
    Gop = Masking(size=N, sampling_bool=mask)
    Gop.lipschitz_cst = Gop.diff_lipschitz_cst = 1.0
    D = Gradient(shape=(n, n), kind='forward')
    D.compute_lipschitz_cst()
    Kop = LinOpVStack(Gop, D)
    H = ProxFuncHStack(L1Loss(dim=m, data=y), 0.1 * L1Norm(dim=2 * N))
    cps = CPS(dim=N, G=Segment(dim=N, a=0, b=1), H=H, K=Kop, x0=torch.zeros(N, dtype=dtype, device='cuda'),
              z0=torch.zeros(m + 2 * N, dtype=dtype, device='cuda'), verbose=None)
    setup = time.perf_counter() - t0
    spec = cps._fused_spec()
    assert spec is not None and 'mask' in spec, 'the inpainting problem must take the fused masked step'
    r = fused_2d(cps, dtype, K, W)
    del cps
    elem = 4 if dtype == torch.float32 else 8
    alg = int((1 + 2 + 1 + 2 * m / N + 2 + m / N) * N * elem)  # x, z_s, y(m), z_m(m) in; x', z_s', z_m' out
    eng_bytes = 9 * N * elem
    km = r['kernels_ms']['step']
    return {'workload': f'CPS TV-LAD inpainting {n}x{n} {args.dtype} (reference notebook problem): K = LinOpVStack('
                        f'Masking 50 %, Gradient(forward)), H = ProxFuncHStack(L1Loss, 0.1*L1Norm), G = Segment(0, 1); '
                        f'one launch per iteration (k_pds2d_smarch with the masked block, PDS2DMaskEngine)',
            'it_per_s': round(1e3 / r['ms_per_step'], 1), 'ms_per_iter': round(r['ms_per_step'], 5), 'steps': K,
            'warmup': W, 'launches_per_iter': 1, 'alg_bytes_per_iter': alg, 'engine_bytes_per_iter': eng_bytes,
            'setup_s': round(setup, 2),
            'iteration_frac_of_hbm_peak': round(alg / (r['ms_per_step'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            'roofline': {'bound': 'hbm', 'kernel': 'pcs_pds2d_step (k_pds2d_smarch<forward, MASK, L1>)',
                         'kernel_ms': round(km, 5), 'achieved': round(alg / (km * 1e-3) / 1e9, 1), 'peak': HBM_PEAK_GBS,
                         'unit': 'GB/s', 'frac': round(alg / (km * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}


def _timed_iters(eng, iters, native):
    """ms per iteration of `iters` iterations through the real transport, max over ranks."""
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    eng.advance(iters)
    torch.cuda.synchronize()
    dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device='cuda' if native else 'cpu')
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item()) * 1e3 / iters


def depth_trial(pds, comm, eng1, depths, W, K):
    """The communication-avoiding depth of a multi-rank slab run (native RCCL loop): the depth-1 engine
    `eng1` (its serial / overlapped schedule trial included) and one deep-halo engine per depth in `depths`
    each run 16 untimed then 32 timed iterations through the real transport; the fastest (max over ranks)
    is returned with the trial times.  A depth whose halo does not fit the slabs is skipped."""
    from pycsou_amd.parallel import SlabPDS2D
    trials, best, best_ms = {}, None, None
    for d in (1,) + tuple(depths):
        if d == 1:
            eng = eng1
        else:
            try:
                eng = SlabPDS2D.from_pds(pds, comm, native=True, depth=d)
            except ValueError as e:  # a slab thinner than the deep halo: that depth does not apply
                trials[d] = f'skipped: {e}'[:120]
                continue
        total = 64 + W + K
        eng.init_loop(total, total, -1.0)
        eng.advance(16)  # untimed (plan creation; depth 1: its schedule trial)
        ms = _timed_iters(eng, 32, True)
        trials[d] = round(ms, 4)
        if best_ms is None or ms < best_ms:
            if best is not None and best is not eng1:
                best._destroy_plan()
            best, best_ms = eng, ms
        elif eng is not eng1:
            eng._destroy_plan()
    return best, trials


def slab_bench(n, dtype, K, W, world, full=True, outputs=False):
    """Weak scaling: a (n world) x n image, one n x n row slab per rank; K timed iterations
    (barrier + synchronize on both sides; the caller takes the max over ranks).  `full`: after the
    timed region also the communication probe and the isolated step timing; `outputs`: this rank's
    rows of x and z and the diagnostics row of the last timed iteration under 'outputs'."""
    from pycsou_amd.parallel import DistComm, SlabPDS2D
    from pycsou_amd.parallel.slab import comm_probe
    pds = build_problem(n * world, n, dtype, lipschitz='analytic')
    comm = DistComm() if world > 1 else None
    kw = dict(rank=0 if comm is None else None, world=1 if comm is None else None)
    fallback = False
    if world > 1 and dist.get_backend() != 'nccl':
        # gloo rehearsal (several ranks on one GPU): the library's RCCL binding needs one GPU per
        # rank, so the torch.distributed-issued loop is the designed path here, not a fallback
        eng = SlabPDS2D.from_pds(pds, comm, native=False, **kw)
    else:
        try:  # the native loop (RCCL bound by the library) unless it cannot be set up on this box
            eng = SlabPDS2D.from_pds(pds, comm, native=True, **kw)
            eng.overlapped()
        except Exception as e:  # noqa: BLE001 -- the torch.distributed-issued loop runs the same kernels
            # reported in the line (top-level 'loop' / 'loop_fallback'), never silent
            print(f'bench: WARNING native slab loop unavailable ({type(e).__name__}: {e}); falling back to the '
                  f'torch.distributed per-iteration loop (reported as loop_fallback=true)', file=sys.stderr)
            eng = SlabPDS2D.from_pds(pds, comm, native=False, **kw)
            fallback = True
    trials = None
    if world > 1 and eng.native:
        # communication-avoiding depths (halos k iterations deep, one exchange per k iterations): kept only when
        # faster through the real transport than the per-iteration exchange
        eng, trials = depth_trial(pds, comm, eng, (2, 4), W, K)
    del pds
    torch.cuda.empty_cache()
    total = W + K + 4
    eng.init_loop(total, total, -1.0)
    spin_up(eng, min(K, 50))
    if world > 1 and eng.depth == 1:  # the one-off serial / overlapped schedule trial, never in the timed region
        eng.init_loop(total, total, -1.0)
        eng.advance(8)
        torch.cuda.synchronize()
    # the spin-up and the trials iterated for a time, not a count: back to the initial iterate
    # (x0 = z0 = 0, halos and padding included), so the W + K iterations below compute the same
    # thing in every run
    torch.cuda.synchronize()
    for b in eng.X + eng.Z:
        b.zero_()
    eng.init_loop(total, total, -1.0)  # fixed count: the loop never stops early
    eng.advance(W)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.advance(K)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    it_done = eng.iterations()
    assert it_done == W + K, (it_done, W, K)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device='cuda' if dist.get_backend() == 'nccl' else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    out = None
    if outputs:
        _, x, z, h = eng.result()
        out = {'x': x, 'z': z, 'diagnostics': h[-1]}
    probe = comm_probe(eng) if world > 1 and full else None  # compute / all-gather / exchange timed apart
    kern_ms = eng.time_step_kernel(min(K, 100)) if full else None  # a step here also holds the sums all-gather + halos
    if eng.depth > 1:
        loop = f'native deep-halo, depth {eng.depth} (pcs_slab2d_deep_run)'
    else:
        loop = ('native, overlapped halo exchange' if eng.overlapped() else 'native, serial') if eng.native else (
            'python (gloo rehearsal)' if world > 1 and dist.get_backend() != 'nccl' else 'python')
    return {'ms_per_step': dt * 1e3 / K, 'kernel_ms': kern_ms, 'kernel_ms_isolated': kern_ms, 'nblocks': eng.nblocks,
            'loop': loop, 'loop_fallback': fallback, 'schedule_trial_ms': getattr(eng, 'tune_ms', None),
            'depth': eng.depth, 'depth_trial_ms_per_iter': trials, 'comm': probe, 'outputs': out}


def strong_bench(n, dtype, K, W, world, depths=(1, 2, 4, 8)):
    """The metric as written (BASELINE: 'PDS iters/sec on 4096^2 TV-deconv ... at 1/2/4/8 GPU'): ONE n x n
    image split into `world` row slabs (strong scaling), the native RCCL loop.  Depth 1 is the
    per-iteration exchange (serial / overlapped schedule trial); depth k > 1 the communication-avoiding
    loop (pcs_slab2d_deep_run: halos k iterations deep, one all-gather + exchange per k iterations, the
    shrinking halo rows recomputed locally).  Each depth is timed over 2 chunks of 16 iterations through
    the real transport (max over ranks) and the fastest runs the W + K measurement; the trial times are
    reported.  gloo rehearsals (no RCCL) run depth 1 on the torch.distributed loop only."""
    from pycsou_amd.parallel import DistComm, SlabPDS2D
    from pycsou_amd.parallel.slab import comm_probe, row_split
    pds = build_problem(n, n, dtype, lipschitz='analytic')
    comm = DistComm()
    native = dist.get_backend() == 'nccl'
    rank = comm.rank
    rows = row_split(n, world, rank)[1]
    eng = SlabPDS2D.from_pds(pds, comm, native=native, depth=1)
    if native:
        eng.overlapped()
        eng, trials = depth_trial(pds, comm, eng, tuple(d for d in depths if d > 1), W, K)
    else:
        trials = {1: None}
    total = W + K + 4
    eng.init_loop(total, total, -1.0)
    eng.advance(W)
    ms = _timed_iters(eng, K, native)
    assert eng.iterations() == W + K, (eng.iterations(), W, K)
    probe = comm_probe(eng)
    elem = 4 if dtype == torch.float32 else 8
    alg = 7 * n * n * elem  # the whole image's (2d+3) N words per iteration, all ranks together
    res = {'workload': f'C3 TV-deconvolution {n}x{n} (ONE image, {world} row slabs of ~{rows} rows: strong scaling), '
                       f'15x15 Gaussian PSF, Gradient(forward), 0.05*L21Norm, fused normal-operator march per slab',
           'it_per_s': round(1e3 / ms, 2), 'ms_per_iter': round(ms, 5), 'steps': K, 'warmup': W,
           'depth': eng.depth, 'depth_trial_ms_per_iter': trials,
           'loop': ('native deep-halo (pcs_slab2d_deep_run)' if eng.depth > 1 else
                    ('native, overlapped' if eng.native and eng.overlapped() else
                     'native, serial' if eng.native else 'python (gloo rehearsal)')),
           'iteration_GBps': round(alg / (ms * 1e-3) / 1e9, 1),
           'iteration_frac_of_hbm_peak_per_gpu': round(alg / (ms * 1e-3) / 1e9 / (HBM_PEAK_GBS * world), 4),
           'alg_bytes_per_iter': alg, 'comm': probe, 'scaling': 'strong'}
    if probe is not None and eng.depth > 1:
        probe['per'] = f'one chunk of {eng.depth} iterations (all-gather of {4 * eng.depth} sums, deep-halo exchange)'
    eng._destroy_plan()
    del eng, pds
    comm.close()
    torch.cuda.empty_cache()
    return res


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def self_launch(args, backend):
    """`python bench.py --gpus N` without an external launcher: start N ranks as
    `python -m torch.distributed.run --nproc-per-node N ... bench.py <same args>` in a child
    process (never exec: nothing has touched the GPU yet, and the parent only waits) and return
    its exit status.  With backend nccl the node must show N GPUs (device_count() does not
    initialise the runtime)."""
    n = args.gpus
    if backend == 'nccl' and not args.launch_check:
        have = torch.cuda.device_count()
        if have < n:
            print(f'bench: --gpus {n} needs {n} visible GPUs with backend nccl (one rank per GPU); '
                  f'this node shows {have}.  Use PCS_BENCH_BACKEND=gloo for a one-GPU rehearsal.', file=sys.stderr)
            return 2
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}',
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', '1')
    import subprocess
    return subprocess.run(cmd, env=env).returncode


def check_world(args, world, backend):
    """The rank count must be what --gpus asks for; nccl needs one GPU per local rank."""
    if world != args.gpus:
        print(f'bench: --gpus {args.gpus} but WORLD_SIZE={world}: the launcher and the flag disagree', file=sys.stderr)
        sys.exit(2)
    if backend == 'nccl' and world > 1 and not args.launch_check:
        lw = int(os.environ.get('LOCAL_WORLD_SIZE', str(world)))
        have = torch.cuda.device_count()
        if have < lw:
            print(f'bench: {lw} local ranks but {have} visible GPUs (backend nccl: one rank per GPU)', file=sys.stderr)
            sys.exit(2)


def launch_check(args, world, rank, backend):
    """--launch-check: the launch path without GPU work -- join the process group, all-reduce the
    rank ids, rank 0 prints the launch facts as one JSON line."""
    if world > 1:
        dev = 'cpu'
        if backend == 'nccl':
            dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
            torch.cuda.set_device(dev)
        dist.init_process_group(backend)
        t = torch.tensor([float(rank)], device=dev)
        dist.all_reduce(t)
        ok = int(t.item()) == world * (world - 1) // 2
        dist.destroy_process_group()
    else:
        ok = True
    if rank == 0:
        print(json.dumps({'launch_check': bool(ok), 'n_gpus': world, 'backend': backend,
                          'parallelism': f'slab{world}' if world > 1 else 'single',
                          'self_launched': os.environ.get('TORCHELASTIC_RUN_ID') is not None}), flush=True)
    return 0 if ok else 1


def headline_watchdog(args, rank, world, dtype):
    """Watchdog on the N > 1 slab headline (the first multi-rank RCCL run): after
    --headline-timeout seconds rank 0 prints the line with an `error` field and every rank exits
    1, so a hang still yields a line and a non-zero status."""
    def fire():
        if rank == 0:
            print(json.dumps({'metric': METRIC, 'value': None, 'unit': 'it/s', 'n_gpus': world,
                              'steps': args.steps, 'warmup': args.warmup, 'higher_is_better': True,
                              'scaling': 'weak', 'vs_baseline': None, 'dtype': args.dtype, 'data': 'synthetic',
                              'config': {'workload': f'C3 TV-deconvolution {args.size}x{args.size} per GPU, slab engine',
                                         'parallelism': f'slab{world}'},
                              'error': f'slab headline: no result within {args.headline_timeout:.0f} s'}), flush=True)
        sys.stderr.write(f'bench: rank {rank}: slab headline timed out\n')
        sys.stderr.flush()
        os._exit(1)
    timer = threading.Timer(args.headline_timeout, fire)
    timer.daemon = True
    timer.start()
    return timer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=500)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'f64'])
    ap.add_argument('--full', action='store_true',
                    help='after the headline: the CPU baseline, the 2-D legs, the volume legs, the isolated per-kernel '
                         'timings and (N > 1) the communication probes and the strong-scaling entry; without it the '
                         'run sets up, warms up, times --steps iterations and prints the line')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps write what the last of them computed (x, z, its diagnostics row) as '
                         'DIR/<name>.npy; outputs above 48 MiB in all are cut to a fixed seeded sample')
    ap.add_argument('--cpu-iters', type=int, default=3)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--volumes', default='c4:512:f32:20,c5:1024:f64:20,c4_cen:512:f32:20:centered,c5_cen:1024:f64:20:centered',
                    help='--full: volume legs name:edge:dtype:steps[:kind], comma separated ("" skips them)')
    ap.add_argument('--volume-timeout', type=float, default=240.0)
    ap.add_argument('--legs', default='c2,c3_nonsep,c2_lap,c2_cen,c3_cen,c3_f64,c3_cen_f64,conv63,cps_inpaint',
                    help='--full: single-GPU 2-D legs after the headline: c2 (2048^2 denoising), c3_nonsep (non-separable '
                         'PSF), c2_lap / c2_cen (Laplacian / centered-Gradient K), c3_cen (C3 with the default '
                         'centered Gradient), conv63 (63x63 FFT Convolve2D), cps_inpaint (generic path); "" skips them')
    ap.add_argument('--lipschitz', default='lanczos', choices=['lanczos', 'analytic'],
                    help='operator norms of the single-GPU 2-D problems: compute_lipschitz_cst() or closed forms')
    ap.add_argument('--engine', default='auto', choices=['auto', 'slab'],
                    help='slab: run the row-slab (multi-GPU) engine even at N=1 (diagnostics)')
    ap.add_argument('--headline-timeout', type=float, default=420.0,
                    help='watchdog (s) on the N > 1 slab headline: a stall prints the line with an error and exits 1')
    ap.add_argument('--no-strong', dest='strong', action='store_false',
                    help='N > 1: skip the strong-scaling entry (one --size^2 image split over the N ranks)')
    ap.add_argument('--launch-check', action='store_true',
                    help='start the ranks, join the process group, all-reduce once and print the launch facts '
                         '(no GPU work; with PCS_BENCH_BACKEND=gloo it runs on a host without GPUs)')
    args = ap.parse_args()

    # PCS_BENCH_BACKEND=gloo + several ranks on one GPU: a rehearsal of the N > 1 code path on a
    # one-GPU box (host-staged transport; the timing is not a scaling number)
    backend = os.environ.get('PCS_BENCH_BACKEND', 'nccl')
    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N`: start the N ranks ourselves (before anything touches the GPU)
        sys.exit(self_launch(args, backend))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    check_world(args, world, backend)
    if args.launch_check:
        sys.exit(launch_check(args, world, rank, backend))
    if backend != 'nccl':
        local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    if world > 1:
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        else:
            dist.init_process_group(backend)
    dtype = torch.float32 if args.dtype == 'f32' else torch.float64
    n = args.size
    K = max(1, args.steps)  # exactly the requested counts (odd counts run a single trailing launch)
    W = max(0, args.warmup)

    out = None
    if world > 1 or args.engine == 'slab':
        # the first multi-rank RCCL run must not lose the line: a stall prints it with an error
        timer = headline_watchdog(args, rank, world, dtype)
        try:
            res = slab_bench(n, dtype, K, W, world, full=args.full, outputs=args.dump_outputs is not None)
        finally:
            timer.cancel()
        res['kernel_ms_isolated'] = res['kernel_ms']
        # --full: the isolated slab steps' mean; a plain run has only the timed loop itself
        res['step_ms_loop'] = res['kernel_ms'] if args.full else res['ms_per_step']
        if res['outputs'] is not None:  # every rank writes the rows of its own slab
            sfx = f'_rank{rank}' if world > 1 else ''
            dump_outputs(args.dump_outputs, {k + sfx: v for k, v in res.pop('outputs').items()}, DUMP_BUDGET // world)
    else:
        t0 = time.perf_counter()
        pds = build_problem(n, n, dtype, lipschitz=args.lipschitz)
        setup = time.perf_counter() - t0  # phantom, blur, compute_lipschitz_cst of K and Conv (device Lanczos)
        lips = {'K': pds.K.lipschitz_cst, 'Conv': pds.F.map2.lipschitz_cst}
        spec = pds._fused_spec()
        assert spec is not None and spec['fkind'] == 2, 'C3 problem must take the fused separable engine'
        res = fused_2d(pds, dtype, K, W, kernels=args.full, outputs=args.dump_outputs is not None)
        del pds
        if res['outputs'] is not None:
            dump_outputs(args.dump_outputs, res.pop('outputs'))
        # one kernel per iteration, launched back to back from C: the step kernel's duration is
        # the timed region's HIP-event time / K (inter-launch gaps included, so it never exceeds
        # ms_per_step); with --full the median of isolated event pairs is reported beside it
        res['step_ms_loop'] = res['ms_per_step']
        res['kernel_ms_isolated'] = res['kernels_ms']['step'] if args.full else None
        res['lipschitz'] = lips
        res['setup_s'] = round(setup, 2)

    if rank == 0:
        elem = 4 if dtype == torch.float32 else 8
        N = n * n
        alg_bytes = 7 * N * elem  # (2d+3) N words: read x, z (2N), y; write x', z' (2N)
        ms = res['ms_per_step']
        value = world / (ms * 1e-3)  # 4096^2-image iterations per second, whole job
        # the roofline's time base: the timed loop's HIP-event time / K (inter-launch gaps included, so
        # `achieved` never overstates the kernel); `kernel_ms` keeps the earlier rounds' meaning, the
        # median of isolated launches
        achieved = alg_bytes / (res['step_ms_loop'] * 1e-3) / 1e9
        traffic, tsrc = None, None
        tpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), TRAFFIC_JSON)
        nm = res.get('nmarch', False)
        if os.path.exists(tpath) and dtype == torch.float32 and n == 4096 and nm:
            traffic = round(json.load(open(tpath))['traffic_bytes'])  # PMC FETCH/WRITE per launch (corrected)
            tsrc = TRAFFIC_JSON
        out = {
            'metric': METRIC, 'value': round(value, 3), 'unit': 'it/s', 'n_gpus': world, 'steps': K, 'warmup': W,
            'ms_per_step': round(ms, 5), 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': args.dtype, 'data': 'synthetic',
            'config': {'workload': f'C3 TV-deconvolution {n}x{n} per GPU ({n * world}x{n} global, row slabs), '
                                   f'15x15 Gaussian PSF sigma=2 (rank-1: grad F = N x - Conv^T y, N = Conv^T Conv as two 29-tap passes), isotropic TV '
                                   f'0.05*L21Norm, Gradient(kind=forward), PDS fused step, '
                                   + ('iterations launched back to back from C (pcs_pds2d_run)'
                                      if 'nblocks' in res and world == 1
                                      and args.engine != 'slab' else
                                      f'slab engine ({res.get("loop", "python")} loop): per-iteration RCCL '
                                      f'all-gather of 4 sums + neighbour halo exchange'),
                       'global_shape': [n * world, n], 'parallelism': f'slab{world}' if world > 1 else 'single',
                       'schedule_trial_ms_serial_overlap': res.get('schedule_trial_ms'),
                       'lipschitz': args.lipschitz if world == 1 else 'analytic',
                       'lipschitz_csts': res.get('lipschitz'), 'setup_s': res.get('setup_s')},
            'steps_requested': args.steps, 'warmup_requested': args.warmup,
            'roofline': {'bound': 'hbm', 'achieved': round(achieved, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                         'frac': round(achieved / HBM_PEAK_GBS, 4), 'traffic': traffic, 'traffic_unit': 'bytes/launch', 'traffic_source': tsrc,
                         'kernel': ('pcs_pds2d_step (k_pds2d_nmarch<float,7,L21,256>: grad F = N x - Conv^T y, '
                                    'N = Conv^T Conv as two 29-tap passes)' if nm else
                                    'pcs_pds2d_step (k_pds2d_march<float,7,L21,256>)'),
                         'step_ms_loop': round(res['step_ms_loop'], 5),
                         'step_ms_loop_source': ('HIP events on the launch stream around the K back-to-back launches '
                                                 'of the timed region, / K (one kernel per iteration; the basis of '
                                                 '`achieved`)'
                                                 if world == 1 and args.engine != 'slab' else
                                                 'mean of HIP-event pairs around isolated slab steps'),
                         'kernel_ms': round(res['kernel_ms_isolated'], 5) if args.full else None,
                         'kernel_ms_source': 'median of HIP-event pairs around isolated launches (rounds 1-3 meaning; '
                                             'a run of its own: --full only)',
                         'alg_bytes_per_launch': alg_bytes,
                         # the 15x15 PSF work beside the bandwidth figure -- per pixel the
                         # normal operator's two 29-tap passes (nmarch) or the four 15-tap separable
                         # passes (2 flop per tap)
                         'conv_flop_per_launch': (116 if nm else 120) * N,
                         'conv_tflops': round((116 if nm else 120) * N / (res['step_ms_loop'] * 1e-3) / 1e12, 2),
                         'fp32_vector_peak_tflops': 157.3},
            'iteration_GBps': round(alg_bytes / (ms * 1e-3) / 1e9, 1),
        }
        if 'loop' in res:  # multi-GPU: which slab loop ran (native RCCL loop, or the torch.distributed fallback)
            out['loop'] = res['loop']
            out['loop_fallback'] = res['loop_fallback']
            out['comm'] = res.get('comm')  # compute / all-gather / exchange ms, halo GB/s per side
        out['full'] = args.full
        if args.full and world == 1 and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(n, args.cpu_iters)
        else:
            out['cpu_baseline'] = None
        if args.full and world == 1 and args.engine != 'slab':
            for leg in filter(None, args.legs.split(',')):
                fn = {'c2': leg_c2, 'c3_nonsep': leg_c3_nonsep, 'c2_lap': leg_c2_lap, 'c2_cen': leg_c2_cen,
                      'c3_cen': leg_c3_cen, 'c3_f64': leg_c3_f64, 'c3_cen_f64': leg_c3_cen_f64, 'conv63': leg_conv63,
                      'cps_inpaint': leg_cps_inpaint}[leg]
                try:
                    out[leg] = fn(args, dtype, K, W)
                except Exception as e:  # noqa: BLE001 -- the C3 line stands on its own
                    out[leg] = {'error': f'{type(e).__name__}: {e}'[:300]}
                    print(f'bench: leg {leg} failed: {out[leg]["error"]}', file=sys.stderr)
    for leg in filter(None, args.volumes.split(',') if args.full else ()):
        name, edge, vdt, vsteps, *vk = leg.split(':')
        out = volume_leg(args, out if rank == 0 else None, f'volume_{name}', int(edge),
                         torch.float64 if vdt == 'f64' else torch.float32, int(vsteps), world, rank,
                         vk[0] if vk else 'forward')
    if world > 1 and args.strong and args.full:
        # the metric as written: one 4096^2 image over the N ranks (strong scaling), beside the weak headline
        try:
            sres = strong_bench(args.size, dtype, K, W, world)
        except Exception as e:  # noqa: BLE001 -- the headline line stands on its own
            sres = {'error': f'{type(e).__name__}: {e}'[:300]}
            print(f'bench: strong-scaling entry failed: {sres["error"]}', file=sys.stderr)
        if rank == 0:
            out['strong_4096'] = sres
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def volume_leg(args, out, key, edge, dtype_v, steps, world, rank, kind='forward'):
    """Run volume_bench under a watchdog; `out` (rank 0) gains `key`.  A failure leaves the C3
    line as it was; a stall past --volume-timeout prints it (with the leg's `error`) and ends the
    process with status 1, so a hung leg is never mistaken for a clean run."""
    def fire():
        if out is not None:
            out[key] = {'error': f'no result within {args.volume_timeout:.0f} s'}
            print(json.dumps(out), flush=True)
        sys.stderr.write('bench: volume leg timed out\n')
        sys.stderr.flush()
        os._exit(1)
    timer = threading.Timer(args.volume_timeout, fire)
    timer.daemon = True
    timer.start()
    try:
        K = max(2, steps + steps % 2)
        if os.environ.get('PCS_BENCH_TEST_STALL') == key:  # tests only: a leg that never returns
            time.sleep(1e6)
        vres = volume_bench(edge, dtype_v, K, 8, world, rank, kind)  # warmup also picks the schedule
    except Exception as e:  # noqa: BLE001 -- the C3 line stands on its own
        vres = {'error': f'{type(e).__name__}: {e}'[:300]}
        print(f'bench: volume leg failed: {vres["error"]}', file=sys.stderr)
    timer.cancel()
    if out is not None:
        out[key] = vres
    return out


if __name__ == '__main__':
    main()
