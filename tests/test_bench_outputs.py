"""bench.py's plain / --full split and --dump-outputs: a plain run carries the headline alone, --full
adds the other measurements, and the dumped arrays are what the last timed iteration computed."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, 'bench.py')


def _bench(args):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, BENCH] + args, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_dump_outputs_sample(tmp_path):
    """Arrays within the budget are written whole; above it the long ones are cut to the same sorted
    seeded sample in every call, the short ones stay whole, and the files stay within the budget."""
    import torch

    import bench
    rng = np.random.default_rng(0)
    x = rng.standard_normal(30000).astype(np.float32)
    z = rng.standard_normal(60000)
    d = np.array([1e-3, 2e-3])
    arrays = {'x': torch.from_numpy(x), 'z': torch.from_numpy(z), 'diagnostics': d}
    bench.dump_outputs(str(tmp_path / 'whole'), arrays)
    for k, v in (('x', x), ('z', z), ('diagnostics', d)):
        got = np.load(tmp_path / 'whole' / f'{k}.npy')
        assert got.dtype == v.dtype and np.array_equal(got, v)
    budget = 200000  # x: 120 kB, z: 480 kB
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), arrays, budget=budget)
    total = 0
    for k, v in (('x', x), ('z', z)):
        a, b = np.load(tmp_path / 'a' / f'{k}.npy'), np.load(tmp_path / 'b' / f'{k}.npy')
        assert a.dtype == v.dtype and np.array_equal(a, b)
        assert 0.3 * v.size < a.size * (x.nbytes + z.nbytes) / budget <= v.size  # cut in proportion
        assert np.isin(a, v).all()
        total += a.nbytes
    dd = np.load(tmp_path / 'a' / 'diagnostics.npy')
    assert np.array_equal(dd, d)
    assert total + dd.nbytes <= budget


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_last_step(tmp_path):
    """A plain run: exactly --steps timed iterations, ms_per_step consistent with value, none of the
    --full measurements; the dumped x, z and diagnostics are those of a (warmup + steps)-iteration
    run of the same problem through the solver."""
    import torch

    import bench
    n, K, W = 256, 7, 3
    out = tmp_path / 'dump'
    d = _bench(['--gpus', '1', '--steps', str(K), '--warmup', str(W), '--size', str(n), '--dump-outputs', str(out)])
    assert d['steps'] == K and d['warmup'] == W and d['full'] is False
    assert d['unit'] == 'it/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert d['ms_per_step'] > 0 and d['value'] == pytest.approx(1e3 / d['ms_per_step'], rel=1e-3)
    assert d['cpu_baseline'] is None and d['roofline']['kernel_ms'] is None
    assert not [k for k in d if k.startswith('volume_') or k in ('c2', 'c3_nonsep', 'conv63', 'cps_inpaint')], sorted(d)
    x, z, diag = (np.load(out / f'{k}.npy') for k in ('x', 'z', 'diagnostics'))
    assert x.dtype == np.float32 and x.shape == (n * n,) and z.shape == (2 * n * n,)
    assert diag.dtype == np.float64 and diag.shape == (2,) and np.isfinite(diag).all()
    from pycsou_amd import _ops as O
    from pycsou_amd.opt.engine import engine_class
    f32 = torch.float32
    pds = bench.build_problem(n, n, f32)
    spec = pds._fused_spec()
    eng = engine_class(spec)(spec, f32, pds.tau, pds.sigma, pds.rho, O.to_dev(pds.x0, f32), O.to_dev(pds.z0, f32))
    it, xr, zr, h = eng.run(W + K - 1, W + K - 1, 0.0)
    assert it == W + K
    # the same deterministic kernel on the same seeded inputs: bit for bit
    assert np.array_equal(x, xr.cpu().numpy())
    assert np.array_equal(z, zr.cpu().numpy())
    np.testing.assert_allclose(diag, np.asarray(h)[-1], rtol=1e-12)


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements():
    """--full: the isolated kernel timing and the requested leg and volume beside the same headline."""
    d = _bench(['--gpus', '1', '--full', '--steps', '6', '--warmup', '2', '--size', '256', '--legs', 'c2',
                '--volumes', 'c4:64:f32:2', '--no-cpu-baseline'])
    assert d['full'] is True and d['steps'] == 6 and d['ms_per_step'] > 0
    assert d['roofline']['kernel_ms'] > 0
    assert d['c2']['it_per_s'] > 0 and d['volume_c4']['it_per_s'] > 0, d
