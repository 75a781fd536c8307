"""Record what every engine constructor decides for the problems of the element-wise matrices:
``python tests/golden/make_golden_engines.py`` (on a GPU) writes ``tests/golden/engine_routes.json`` with the
commit it was recorded at.  Engines are built and nothing is iterated.

Per engine: the class name, every non-pointer field of its argument struct, null / non-null for every pointer
field, and the attributes that name its route (below).  Built are
  - for every entry of tests/pointwise.py MATRIX the engine ``engine_class(spec)`` gives, under the case's
    environment switches, and -- except for the masked problems, which a slab does not take --
    ``SlabPDS2D(spec, ..., rank, 2, comm=None, native=False)`` for both ranks (a constructor that raises
    ValueError is recorded as 'ValueError');
  - the PDS3DEngine of every entry of tests/pointwise3d.py MATRIX;
  - the APGD2DEngine of every entry of tests/pointwise_apgd.py CASES.
The table is stored in the form of tests/golden/packed.py (equal records once, and of each record only what
departs from the most common values of its class).
tests/test_gpu_engine_routes.py rebuilds the records and compares everything.
"""

import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'engine_routes.json')
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

ATTRS_2D = ('fkind', 'march', 'nm_fused', 'native', 'defer', 'nblocks', 'run_nblocks')
ATTRS_SLAB = ('mode', 'fkind', 'nm_fused', 'hx', 'hy', 'hz', 'reach', 'pad', 'overlap', 'nblocks')
ATTRS_3D = ('fkind', 'fused0', 'sep2', 'ata', 'fold', 'banded', 'hx', 'hz', 'hg', 'g_lo', 'zdepth', 'halo_planes',
            'nblocks')
# an attribute an engine does not carry reads as the default its own code read it with
DEFAULTS = {'nm_fused': False, 'defer': False}


def args_record(a):
    out = {}
    for name, ctype in a._fields_:
        v = getattr(a, name)
        out[name] = (v is not None and v != 0) if ctype is ctypes.c_void_p else v
    return out


def _plain(v):
    return list(v) if isinstance(v, tuple) else v


def engine_record(eng, attrs):
    a = eng.args[0] if isinstance(eng.args, list) else eng.args
    rec = {'class': type(eng).__name__, 'args_type': type(a).__name__, 'args': args_record(a)}
    for n in attrs:
        rec[n] = _plain(getattr(eng, n, DEFAULTS.get(n)))
    for n in ('partials', 'ws'):
        t = getattr(eng, n, None)
        rec[n + '_numel'] = None if t is None else int(t.numel())
    return rec


class _Env:
    """The case's environment switches for the time an engine is built."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _solver_inputs(s):
    from pycsou_amd import _ops as O
    dtype = s._compute_dtype()
    return dtype, O.to_dev(s.x0, dtype), (O.to_dev(s.z0, dtype) if getattr(s, 'z0', None) is not None else None)


def records():
    """[[id, record], ...]; a record is a dict, or 'ValueError'."""
    import torch
    from tests import pointwise as PW
    from tests import pointwise3d as PW3
    from tests import pointwise_apgd as PA
    from pycsou_amd.opt.engine import APGD2DEngine, engine_class
    from pycsou_amd.opt.engine3d import PDS3DEngine
    from pycsou_amd.parallel.slab import SlabPDS2D
    assert 'PCS_NO_MARCH' not in os.environ
    out = []
    for ik in PW.MATRIX:
        c, p = PW.case_problem(ik)
        with _Env(c.env):
            s = PW.build_solver(p, 1, c.engine)
            spec = s._fused_spec()
            dtype, x0, z0 = _solver_inputs(s)
            eng = engine_class(spec)(spec, dtype, s.tau, s.sigma, s.rho, x0, z0)
            out.append([f'2d:{PW.case_id(ik)}', engine_record(eng, ATTRS_2D)])
            del eng
            if 'mask' in spec:
                continue
            for rank in (0, 1):
                try:
                    slab = SlabPDS2D(spec, dtype, s.tau, s.sigma, s.rho, x0, z0, rank, 2, comm=None, native=False)
                    rec = engine_record(slab, ATTRS_SLAB)
                    del slab
                except ValueError:
                    rec = 'ValueError'
                out.append([f'slab{rank}:{PW.case_id(ik)}', rec])
    for ik in PW3.MATRIX:
        c, p = PW3.case_problem(ik)
        with _Env(c.env):
            s = PW3.build_solver(p, 1)
            spec = s._fused_spec()
            dtype, x0, z0 = _solver_inputs(s)
            eng = PDS3DEngine(spec, dtype, s.tau, s.sigma, s.rho, x0, z0)
            rec = engine_record(eng, ATTRS_3D)
            T = getattr(eng, 'T', [])
            rec['gbuf_is_T'] = next((i for i, t in enumerate(T) if t is eng.gbuf), None)
            rec['T_len'] = len(T)
            out.append([f'3d:{PW3.case_id(ik)}', rec])
            del eng
    for i in PA.MATRIX:
        c, p = PA.case_problem(i)
        s = PA.build_solver(p, 1, engine='fused')
        dtype, x0, _ = _solver_inputs(s)
        eng = APGD2DEngine(s._fused_spec(dtype), dtype, s.tau, x0)
        out.append([f'apgd:{PA.case_id(i)}', engine_record(eng, ('nblocks',))])
        del eng
    torch.cuda.synchronize()
    return out


def group(rec):
    return rec['class'] + '/' + rec['args_type']


def main():
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    if len(sys.argv) > 1:  # recorded from a copy of the tree that carries no history: the hash by hand
        commit = sys.argv[1]
    else:
        commit = subprocess.run(['git', '-C', REPO, 'rev-parse', 'HEAD'], stdout=subprocess.PIPE).stdout.decode().strip()
    doc = {'commit': commit, **packed.pack(records(), group)}
    with open(out, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print(f'{out}: {len(doc["rows"])} engines, {len(doc["records"])} distinct records')


if __name__ == '__main__':
    main()
