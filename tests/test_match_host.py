"""What every problem of the element-wise matrices is matched to, and what the matchers refuse: the table of
tests/golden/make_golden_specs.py regenerated on the host and compared with tests/golden/fused_specs.json, which
was recorded before the matchers shared their H / G / F pieces (the commit is in the file).  No GPU is needed."""

import importlib.util
import json
import os

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden_specs',
                                               os.path.join(_HERE, 'golden', 'make_golden_specs.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope='module')
def golden():
    with open(gen.OUT) as f:
        doc = json.load(f)
    assert len(doc['commit']) == 40
    return doc['ids'], gen.packed.unpack(doc)


@pytest.fixture(scope='module')
def regenerated():
    return {'matrix': json.loads(json.dumps(gen.matrix_records())),
            'refusals': json.loads(json.dumps(gen.refusal_records()))}


def _compare(got, want):
    assert len(got) == len(want)
    bad = [(k, g, w) for (k, g), w in zip(got, want) if g != w]
    assert not bad, f'{len(bad)} of {len(got)} specs differ, first (id, got, recorded): {bad[0]}'


def test_same_problems(golden, regenerated):
    ids = [k for k, _ in regenerated['matrix'] + regenerated['refusals']]
    assert gen.packed.ids_digest(ids) == golden[0]


def test_matrix_specs(golden, regenerated):
    n = len(regenerated['matrix'])
    assert n > 800  # 93 + 46 problems x 2 dtypes x up to 3 modes, 31 APGD problems x 2 dtypes
    _compare(regenerated['matrix'], golden[1][:n])


def test_refusals(golden, regenerated):
    got = regenerated['refusals']
    _compare(got, golden[1][len(golden[1]) - len(got):])
    by = dict(got)
    # each departure from an accepted problem is refused by every matcher
    for name in ('no-H', 'H-shifted', 'H-shifted-3d', 'L21-pixel_d-3-on-2d', 'L21-dim-wrong', 'L21-pixel_d-2-on-3d',
                 'L21-dim-wrong-3d', 'L1-dim-wrong', 'K-1d', 'G-L1Norm', 'F-data-length', 'F-conv-other-shape'):
        for fn in ('match_pds2d', 'match_stencil2d', 'match_masked_stencil2d', 'match_pds3d'):
            assert by[f'{name}:{fn}'] is None, (name, fn)
    assert by['accepted-2d:match_pds2d'] is not None and by['F-conv-accepted:match_stencil2d'] is not None
    for name in ('masked-nan', 'masked-inf', 'masked-n1%4-70x130', 'masked-n1<=64-70x64'):
        assert by[name] is None, name
    assert by['masked-accepted-70x132'] is not None and by['masked-n1=68-70x68'] is not None
