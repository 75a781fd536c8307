"""Record the fused-engine spec every solver problem of the element-wise matrices is matched to, and the problems
the matchers refuse: ``python tests/golden/make_golden_specs.py`` writes ``tests/golden/fused_specs.json``.
Only ``PDS._fused_spec()``, ``APGD._engine_takes`` and the ``match_*`` functions are called, by name, on
solvers built on the host: no GPU is needed, and the same script runs on the commit that recorded the table
(its hash is in the file) and on every later one (tests/test_match_host.py regenerates the table and compares).

Problems: every entry of tests/pointwise.py MATRIX, tests/pointwise3d.py MATRIX and tests/pointwise_apgd.py
CASES, built with their own build_solver in fp32 and in fp64, the PDS ones under the engine modes 'auto',
'fused' and 'stencil' (the masked problems are CPS objects, which take no mode: 'auto').  APGD._fused_spec also
asks whether a GPU is visible, so the APGD problems record its two machine-independent parts instead:
match_apgd2d and APGD._engine_takes.

A spec is recorded as its keys with scalars, tuples and lists as they are, arrays as [dtype, numel], operators as
[class name, dims], no match as null; the table is stored in the form of tests/golden/packed.py.
"""

import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'fused_specs.json')
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _packed():
    """tests/golden/packed.py: the stored form of the table."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('golden_packed', os.path.join(HERE, 'packed.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


packed = _packed()

DTYPES = {'f32': np.float32, 'f64': np.float64}
MODES = ('auto', 'fused', 'stencil')


def serial(v):
    import torch
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (np.bool_, np.integer, np.floating)):
        return v.item()
    if isinstance(v, (tuple, list)):
        return [serial(e) for e in v]
    if isinstance(v, np.ndarray):
        return [str(v.dtype), int(v.size)]
    if isinstance(v, torch.Tensor):
        return [str(v.dtype).replace('torch.', ''), int(v.numel())]
    return [type(v).__name__, serial(getattr(v, 'dims', None))]


def spec_record(spec):
    return None if spec is None else {k: serial(v) for k, v in spec.items()}


def _with_dtype(p, dtype):
    q = dict(p)
    q['dtype'] = dtype
    return q


def matrix_records():
    """[[id, record], ...] of the three matrices."""
    from tests import pointwise as PW
    from tests import pointwise3d as PW3
    from tests import pointwise_apgd as PA
    from pycsou_amd.opt.engine import match_apgd2d
    from pycsou_amd.opt.proxalgs import APGD
    import torch
    out = []
    for tag, mod in (('2d', PW), ('3d', PW3)):
        for ik in mod.MATRIX:
            c, p = mod.case_problem(ik)
            modes = ('auto',) if getattr(c, 'row', '') == 'masked' else MODES
            for dn, dt in DTYPES.items():
                for mode in modes:
                    s = mod.build_solver(_with_dtype(p, dt), 1, mode)
                    out.append([f'{tag}:{mod.case_id(ik)}:{dn}:{mode}', spec_record(s._fused_spec())])
    for i in PA.MATRIX:
        c, p = PA.case_problem(i)
        for dn, dt in DTYPES.items():
            s = PA.build_solver(_with_dtype(p, dt), 1)
            tdt = torch.float32 if dt == np.float32 else torch.float64
            spec = match_apgd2d(s.F, s.G, tdt)
            takes = None if spec is None else bool(APGD._engine_takes(spec, tdt))
            out.append([f'apgd:{PA.case_id(i)}:{dn}', {'spec': spec_record(spec), 'engine_takes': takes}])
    return out


def refusal_records():
    """Problems one test away from a match; every one is recorded (null = refused)."""
    from tests import pointwise as PW
    from pycsou_amd.core.functional import ProxFuncPostComp
    from pycsou_amd.func import L1Loss, ProxFuncHStack
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm, L21Norm
    from pycsou_amd.linop import LinOpVStack, Masking
    from pycsou_amd.linop.conv import Convolve2D
    from pycsou_amd.linop.diff import Gradient
    from pycsou_amd.opt import engine as E
    from pycsou_amd.opt import engine3d as E3
    out = []
    n0, n1 = 12, 20
    N = n0 * n1
    y = np.linspace(0.0, 1.0, N).astype(np.float32)
    K2 = Gradient((n0, n1), kind='forward')
    K2c = Gradient((n0, n1), kind='centered')
    K3 = Gradient((4, 6, 10), kind='forward')
    N3 = 240
    F = (1 / 2) * SquaredL2Loss(dim=N, data=y)
    H2 = 0.5 * L1Norm(dim=2 * N)

    def l21(dim, d, n):
        return 0.5 * L21Norm(dim=dim, groups=np.tile(np.arange(n), d))

    def every(name, F_, G_, H_, K_, has_H=True):
        for fn in ('match_pds2d', 'match_stencil2d', 'match_masked_stencil2d'):
            out.append([f'{name}:{fn}', spec_record(getattr(E, fn)(F_, G_, H_, K_, has_H))])
        out.append([f'{name}:match_pds3d', spec_record(E3.match_pds3d(F_, G_, H_, K_, has_H))])

    every('accepted-2d', F, None, H2, K2)  # the base problem the refusals below depart from
    every('no-H', F, None, H2, K2, has_H=False)
    every('H-shifted', F, None, ProxFuncPostComp(L1Norm(dim=2 * N), 0.5, 1.0), K2)
    every('H-shifted-3d', None, None, ProxFuncPostComp(L1Norm(dim=3 * N3), 0.5, 1.0), K3)
    every('L21-pixel_d-3-on-2d', F, None, l21(3 * N, 3, N), K2)
    every('L21-dim-wrong', F, None, l21(2 * (N + 2), 2, N + 2), K2c)
    every('L21-pixel_d-2-on-3d', None, None, l21(2 * N3, 2, N3), K3)
    every('L21-dim-wrong-3d', None, None, l21(3 * (N3 + 2), 3, N3 + 2), K3)
    every('L1-dim-wrong', F, None, 0.5 * L1Norm(dim=2 * N + 1), K2)
    every('K-1d', F, None, H2, Gradient((N,), kind='forward'))
    every('G-L1Norm', F, 0.5 * L1Norm(dim=N), H2, K2)
    every('F-data-length', (1 / 2) * SquaredL2Loss(dim=N + 1, data=np.zeros(N + 1, dtype=np.float32)), None, H2, K2)
    t = np.array([0.25, 0.5, 0.25])
    every('F-conv-accepted', F * Convolve2D(N, np.outer(t, t), (n0, n1)), None, H2, K2)
    every('F-conv-other-shape', F * Convolve2D(N, np.outer(t, t), (n1, n0)), None, H2, K2)

    def masked(shape, dtype=np.float32, bad=None):
        """match_masked_stencil2d on the CPS problem of tests/pointwise.py at `shape`; `bad`: a value put
        into the masked data."""
        p = PW.make_problem(shape, 'forward', 'l1', 'null', 'segment', lam=PW.LAM, seed=5, dtype=dtype,
                            mask_share=0.5)
        m, Nn = p['m'], p['N']
        ym = p['ym'].astype(dtype)
        if bad is not None:
            ym[m // 2] = bad
        K = LinOpVStack(Masking(size=Nn, sampling_bool=p['mask']), Gradient(shape, kind='forward'))
        H = ProxFuncHStack(L1Loss(dim=m, data=ym), 0.5 * L1Norm(dim=2 * Nn))
        return spec_record(E.match_masked_stencil2d(None, None, H, K, True))

    out.append(['masked-accepted-70x132', masked((70, 132))])
    out.append(['masked-nan', masked((70, 132), bad=np.nan)])
    out.append(['masked-inf', masked((70, 132), bad=np.inf)])
    out.append(['masked-n1%4-70x130', masked((70, 130))])
    out.append(['masked-n1<=64-70x64', masked((70, 64))])
    out.append(['masked-n1=68-70x68', masked((70, 68))])
    # the fp64 branch of PDS._fused_spec (images the row march covers) does not try the masked matcher, but it
    # asks K for its dims and the stacked K of this problem has none, so the problem takes the other branch in
    # fp64 too: recorded as it is
    p = PW.make_problem((70, 132), 'forward', 'l1', 'null', 'segment', lam=PW.LAM, seed=5, dtype=np.float64,
                        mask_share=0.5)
    for dn, dt in DTYPES.items():
        s = PW.build_solver(_with_dtype(p, dt), 1, 'auto')
        out.append([f'masked-solver-70x132:{dn}', spec_record(s._fused_spec())])
    return out


def records():
    return matrix_records() + refusal_records()


def main():
    commit = subprocess.run(['git', '-C', REPO, 'rev-parse', 'HEAD'], stdout=subprocess.PIPE).stdout.decode().strip()
    doc = {'commit': commit, **packed.pack(records())}
    with open(OUT, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print(f'{OUT}: {len(doc["rows"])} rows, {len(doc["records"])} distinct records')


if __name__ == '__main__':
    main()
