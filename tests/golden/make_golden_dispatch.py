"""Record which kernel family takes a fused 2-D PDS step, and with which grid, for a grid of argument sets:
``python tests/golden/make_golden_dispatch.py`` writes ``tests/golden/pds2d_dispatch.json`` from the built
library.  Only the planning queries of the C ABI are called: nothing is launched and the fake device addresses
are never dereferenced, so it runs without a GPU (tests/test_host_dispatch.py regenerates the table and
compares; the block counts are device-dependent and recorded on a machine with no GPU visible, where every
occupancy query takes its fallback).

Per argument set and process-wide setting (each setting gathered in a fresh child process, because
PCS_NO_MARCH is read once):
  [pcs_pds2d_supported, pcs_pds2d_path, pcs_pds2d_nblocks,
   pcs_pds2d_nblocks_bands of (0, m, m, m), (m, rows, rows, rows), (0, 16, rows - 16, rows),
   then for modes 0, 1, 2: pcs_pds2d_run_nblocks, the six outputs of pcs_pds2d_run_plan at iteration 0, at 1]
with m the split row of the paired run loop.  Equal records are stored once (`records`); `sections` maps a
setting to one record index per case, in the order of `cases`.
"""

import ctypes
import itertools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'pds2d_dispatch.json')

# process-wide settings, one section each
SECTIONS = {'default': {}, 'PCS_NM64=0': {'PCS_NM64': '0'}, 'PCS_NMARCH_GEN=0': {'PCS_NMARCH_GEN': '0'},
            'PCS_SM_FWD=1': {'PCS_SM_FWD': '1'}, 'PCS_NO_MARCH=1': {'PCS_NO_MARCH': '1'}}
# every environment switch of the dispatch: cleared before a section's own setting is applied
SWITCHES = ('PCS_NM64', 'PCS_NMARCH_GEN', 'PCS_SM_FWD', 'PCS_NO_MARCH', 'PCS_RUN_BANDS', 'PCS_SM_SPLIT',
            'PCS_NX_SUB', 'PCS_PT_SLOTS', 'PCS_SM_SLOTS', 'PCS_NMARCH_SLOTS', 'PCS_NM64_SLOTS', 'PCS_ATA_KERNEL')

SHAPES = [(64, 64), (63, 65), (160, 128), (208, 192), (96, 60), (128, 100), (2048, 2048), (4096, 4096)]
# (fkind name, half, cty / ntaps / gbuf present, masked block)
F_NULL, F_DENOISE, F_SEPCONV, F_GRADBUF, F_CONV2D = 0, 1, 2, 3, 4
FSETS = ([('null', 0, 0, 0), ('null', 0, 0, 1), ('denoise', 0, 0, 0), ('denoise', 0, 0, 1), ('gradbuf', 0, 1, 0)] +
         [('sepconv', h, c, 0) for h in (2, 7, 11, 16) for c in (1, 0)] +
         [('conv2d', 0, 1, 0), ('conv2d-noplans', 0, 1, 0)])
FKIND = {'null': F_NULL, 'denoise': F_DENOISE, 'gradbuf': F_GRADBUF, 'sepconv': F_SEPCONV, 'conv2d': F_CONV2D,
         'conv2d-noplans': F_CONV2D}
# slabs: rows [32, n0 - 32) with halos (x, y, z)
HALOS = {'whole': None, 'slab-15-8-4': (15, 8, 4), 'slab-16-16-4': (16, 16, 4), 'slab-1-1-1': (1, 1, 1)}


def cases():
    """[dtype, fset, kkind, hkind, n0, n1, slab, extra] per case; `extra`: '' or a one-off variation."""
    out = []
    for dt, f, kk, hk, (n0, n1) in itertools.product((0, 1), range(len(FSETS)), range(4), (0, 1), SHAPES):
        out.append([dt, f, kk, hk, n0, n1, 'whole', ''])
    for slab in ('slab-15-8-4', 'slab-16-16-4', 'slab-1-1-1'):
        for dt, f, kk, (n0, n1) in itertools.product((0, 1), range(len(FSETS)), range(4), [(160, 128), (2048, 2048)]):
            out.append([dt, f, kk, 1, n0, n1, slab, ''])
    sep7 = next(i for i, f in enumerate(FSETS) if f == ('sepconv', 7, 1, 0))
    for dt, f, kk in itertools.product((0, 1), (0, 2, sep7), (0, 2)):
        out.append([dt, f, kk, 1, 160, 128, 'whole', 'x-unaligned'])
    for dt, kk in itertools.product((0, 1), (0, 2)):
        out.append([dt, sep7, kk, 1, 160, 128, 'whole', 'no-gbuf'])
        out.append([dt, sep7, kk, 1, 160, 128, 'whole', 'cty-unaligned'])
    return out


def make_args(_lib, case):
    dt, f, kk, hk, n0, n1, slab, extra = case
    name, half, cty, masked = FSETS[f]
    a = _lib.PdsArgs()
    a.dtype, a.fkind, a.hkind, a.gkind, a.kkind = dt, FKIND[name], hk, 0, kk
    a.mkind = 1 if masked else 0
    a.half = half
    a.n0 = a.rows = n0
    a.n1 = n1
    if HALOS[slab] is not None:
        a.row0, a.rows = 32, n0 - 64
        a.halo_x, a.halo_y, a.halo_z = HALOS[slab]
    a.tau = a.sigma = a.step0 = a.step1 = a.lam = 1.0
    a.rho = 0.9
    fields = ['x', 'xn', 'z', 'zn', 'y', 'partials']
    if name == 'sepconv':
        fields += ['taps0', 'taps1']
    if cty:
        fields += ['cty', 'ntaps', 'gbuf']
    if masked:
        fields += ['ym', 'zm', 'zmn']
    if name == 'conv2d':
        fields += ['conv_fwd', 'conv_adj', 'rbuf']
    if name.startswith('conv2d'):
        a.conv_tier = 3
    for k, fld in enumerate(fields):  # distinct fake device addresses on the 16-byte grid
        setattr(a, fld, 0x100000 * (k + 1))
    if extra == 'x-unaligned':
        a.x = a.x + 4
    elif extra == 'cty-unaligned':
        a.cty = a.cty + 8
    elif extra == 'no-gbuf':
        a.gbuf = None
    return a


def record(lib, a):
    p = ctypes.byref(a)
    rows = a.rows
    m = (rows // 2 + 8) // 16 * 16
    r = [lib.pcs_pds2d_supported(p), lib.pcs_pds2d_path(p), lib.pcs_pds2d_nblocks(p)]
    for b in ((0, m, m, m), (m, rows, rows, rows), (0, 16, rows - 16, rows)):
        r.append(lib.pcs_pds2d_nblocks_bands(p, *b))
    out = (ctypes.c_int64 * 6)()
    for mode in (0, 1, 2):
        r.append(lib.pcs_pds2d_run_nblocks(p, mode))
        for i in (0, 1):
            assert lib.pcs_pds2d_run_plan(p, mode, i, out) == 0
            r += list(out)
    return [int(v) for v in r]


# positions in a record of the device-dependent block counts (everything else is compared on every machine):
# nblocks, the three band counts, and per mode run_nblocks and the T / B task counts of both iterations
def count_positions():
    pos = [2, 3, 4, 5]
    for k in range(3):
        base = 6 + 13 * k
        pos += [base, base + 3, base + 4, base + 9, base + 10]
    return pos


def section_records():
    """Records of every case under the current process's environment."""
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from pycsou_amd import _lib
    lib = _lib.load()
    return [record(lib, make_args(_lib, c)) for c in cases()]


def section_env(name):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(SECTIONS[name])
    return env


def child_records(name):
    """The section's records from a fresh child process (it never launches anything)."""
    res = subprocess.run([sys.executable, os.path.abspath(__file__), '--section'], env=section_env(name), check=True,
                         stdout=subprocess.PIPE)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def pack(by_section):
    """{section: records} -> the stored form (equal records once)."""
    index, records, sections = {}, [], {}
    for name, recs in by_section.items():
        ids = []
        for r in recs:
            key = tuple(r)
            if key not in index:
                index[key] = len(records)
                records.append(r)
            ids.append(index[key])
        sections[name] = ids
    return {'cases': cases(), 'fsets': [list(f) for f in FSETS], 'records': records, 'sections': sections}


def unpack(doc):
    return {name: [doc['records'][i] for i in ids] for name, ids in doc['sections'].items()}


def main():
    if '--section' in sys.argv:
        print(json.dumps(section_records(), separators=(',', ':')))
        return
    commit = subprocess.run(['git', '-C', REPO, 'rev-parse', 'HEAD'], stdout=subprocess.PIPE).stdout.decode().strip()
    doc = pack({name: child_records(name) for name in SECTIONS})
    doc = {'commit': commit, **doc}
    with open(OUT, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print(f'{OUT}: {len(doc["cases"])} cases x {len(SECTIONS)} sections, {len(doc["records"])} distinct records')


if __name__ == '__main__':
    main()
