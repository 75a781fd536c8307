"""What every engine constructor decides for the problems of the element-wise matrices -- the engine class, every
scalar of its argument struct, which of its pointers are set, its route attributes, halo depths and block counts
-- rebuilt by tests/golden/make_golden_engines.py and compared with tests/golden/engine_routes.json, recorded on
an MI355X before the constructors shared their builders (the commit is in the file).  Engines are built, nothing
is iterated."""

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
    classes = {w['class'] for w in want.values() if isinstance(w, dict)}
    assert classes == {'PDS2DEngine', 'PDS2DStencilEngine', 'PDS2DMaskEngine', 'SlabPDS2D', 'PDS3DEngine', 'APGD2DEngine'}
    assert any(w == 'ValueError' for w in want.values())
