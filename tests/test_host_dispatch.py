"""The dispatch table of the fused 2-D step (csrc/pds_host.hpp select_path): which kernel family takes a call and
with which grid, regenerated from the built library by the planning queries (nothing is launched, the fake
device addresses are never dereferenced) and compared with tests/golden/pds2d_dispatch.json, recorded before the
selector existed (the commit is in the file).  Paths, support flags, `paired`, the split row and the band order
do not depend on the device and are compared everywhere; the block counts follow the device's occupancy and are
compared only where no GPU is visible -- there every occupancy query takes its fallback, so they pin those too.

The switches read per call (PCS_NM64, PCS_NMARCH_GEN, PCS_SM_FWD) are flipped inside this process, which is
how the GPU tests use them; PCS_NO_MARCH is read once per process and gets a fresh child."""

import importlib.util
import json
import os

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden_dispatch',
                                               os.path.join(_HERE, 'golden', 'make_golden_dispatch.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope='module')
def golden():
    with open(gen.OUT) as f:
        doc = json.load(f)
    assert doc['cases'] == gen.cases() and doc['fsets'] == [list(f) for f in gen.FSETS]
    assert set(doc['sections']) == set(gen.SECTIONS)
    return gen.unpack(doc)


def _compare(name, got, want):
    cases = gen.cases()
    assert len(got) == len(want) == len(cases)
    counts = set(gen.count_positions()) if torch.cuda.device_count() > 0 else set()
    bad = []
    for case, g, w in zip(cases, got, want):
        assert len(g) == len(w)
        if any(x != y for k, (x, y) in enumerate(zip(g, w)) if k not in counts):
            bad.append((case, g, w))
    assert not bad, f'{name}: {len(bad)} of {len(cases)} cases differ, first: {bad[0]}'


@pytest.mark.parametrize('name', [n for n in gen.SECTIONS if n != 'PCS_NO_MARCH=1'])
def test_dispatch_table(name, golden, monkeypatch):
    assert 'PCS_NO_MARCH' not in os.environ  # read once: this process must never have seen it
    for k in gen.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in gen.SECTIONS[name].items():
        monkeypatch.setenv(k, v)
    _compare(name, gen.section_records(), golden[name])


def test_dispatch_table_no_march(golden):
    _compare('PCS_NO_MARCH=1', gen.child_records('PCS_NO_MARCH=1'), golden['PCS_NO_MARCH=1'])
