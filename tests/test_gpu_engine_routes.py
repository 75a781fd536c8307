"""What every engine constructor decides for the problems of the element-wise matrices -- the engine class, every
scalar of its argument struct, which of its pointers are set, its route attributes, halo depths and block counts
-- rebuilt by tests/golden/make_golden_engines.py and compared with tests/golden/engine_routes.json, recorded on
an MI355X (the commit is in the file).  First recorded before the constructors shared their builders; recorded
again when the reduction workspace lost its two doubles of slack: `ws_numel` went from 8 to 6 on the 170 engines
that own one and no other entry of the 348 records moved.  Engines are built, nothing is iterated."""

import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden_engines',
                                               os.path.join(_HERE, 'golden', 'make_golden_engines.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def test_engine_routes():
    with open(gen.OUT) as f:
        doc = json.load(f)
    assert len(doc['commit']) == 40
    got = json.loads(json.dumps(gen.records()))
    assert gen.packed.ids_digest([k for k, _ in got]) == doc['ids']
    got = dict(got)
    want = dict(zip(got, gen.packed.unpack(doc)))
    assert len(want) == len(got) == doc['ids'][0]
    bad = []
    for name in want:
        g, w = got[name], want[name]
        if g != w:
            diff = {k: (g.get(k), w.get(k)) for k in set(g) | set(w) if g.get(k) != w.get(k)} \
                if isinstance(g, dict) and isinstance(w, dict) else (g, w)
            bad.append((name, diff))
    assert not bad, f'{len(bad)} of {len(want)} engines differ, first (got, recorded): {bad[:3]}'
    # the workspace is the advertised size and no more: one group of at most 1024 workgroups in every case here,
    # 4 group sums + 2 counters padded to 16 bytes = 48 bytes (red_ws_bytes, csrc/pds_ctrl.hpp)
    owners = [w for w in want.values() if isinstance(w, dict) and w['ws_numel'] is not None]
    assert len(owners) == 170 and all(w['ws_numel'] == 6 and w['nblocks'] <= 1024 for w in owners)
    classes = {w['class'] for w in want.values() if isinstance(w, dict)}
    assert classes == {'PDS2DEngine', 'PDS2DStencilEngine', 'PDS2DMaskEngine', 'SlabPDS2D', 'PDS3DEngine', 'APGD2DEngine'}
    assert any(w == 'ValueError' for w in want.values())
