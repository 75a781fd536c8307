"""Compare the device assembly of the kernel units of two source trees, kernel by kernel.

    python tools/asm_ab.py TREE_A TREE_B [--units pds,pds_nm,...] [--jobs N] [--keep DIR]

Each unit is compiled in each tree with that tree's Makefile flags plus `--cuda-device-only -S`, at most
16 compiles at a time.  Per kernel symbol one line:
    identical   the kernel's text (body, .amdhsa block, metadata entry) is the same in both trees
    reordered   the same multiset of body lines, identical .amdhsa block and metadata entry
    different   anything else; also a kernel that only one tree has
followed, for reordered and different kernels, by the resource fields that differ (vgpr, sgpr, LDS,
scratch, spills, occupancy).  Exit status 1 if any kernel is `different`.  The tool compares the two trees
and reads nothing else out of the assembly."""
import argparse
import collections
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

UNITS = ['pds', 'pds_nm', 'pds_sm32', 'pds_sm64', 'pds_nm64', 'pds_gen', 'pds3d', 'corr2d', 'sep_ata', 'apgd2d', 'conv']
FIELDS = ['.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
          '.vgpr_spill_count', '.sgpr_spill_count', 'Occupancy']


def make_flags(tree):
    """FLAGS and FLAGS_<unit> of the tree's Makefile, $(ARCH) and $(HIPCC) resolved."""
    var = {}
    for line in open(os.path.join(tree, 'Makefile')):
        m = re.match(r'(\w+)\s*[:?]?=\s*(.*)', line)
        if m:
            var[m.group(1)] = re.sub(r'\$\((\w+)\)', lambda r: var.get(r.group(1), ''), m.group(2).strip())
    return var


def compile_unit(tree, unit, out):
    var = make_flags(tree)
    cmd = [var['HIPCC']] + var['FLAGS'].split() + var.get('FLAGS_' + unit, '').split() + [
        '--cuda-device-only', '-S', os.path.join('pycsou_amd', 'csrc', unit + '.hip'), '-o', out]
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f'{tree}: {unit}: {r.stderr[-2000:]}')
    return out


def parse(path):
    """{kernel symbol: (body lines, .amdhsa lines, metadata entry lines, {field: value})}"""
    lines = open(path).read().split('\n')
    names = [l.split()[1] for l in lines if l.lstrip().startswith('.amdhsa_kernel ')]
    label = re.compile(r'(\w+):\s*(;.*)?$')  # "name:   ; @name"
    start = {m.group(1): i for i, m in enumerate(map(label.match, lines)) if m and m.group(1) in set(names)}
    out = {}
    for n in names:
        i = start[n]
        body = []
        while not lines[i].lstrip().startswith('.amdhsa_kernel '):
            body.append(lines[i].strip())
            i += 1
        hsa = []
        while not lines[i].lstrip().startswith('.end_amdhsa_kernel'):
            hsa.append(lines[i].strip())
            i += 1
        fields = {}
        while not lines[i].startswith('; Occupancy:'):
            i += 1
        fields['Occupancy'] = lines[i].split(':')[1].strip()
        out[n] = [body, hsa, [], fields]
    # metadata: one entry per kernel under amdhsa.kernels, each starting with "  - ."
    i = lines.index('amdhsa.kernels:') + 1
    entry = []
    while True:
        top = not lines[i].startswith('   ')  # a new entry ("  - .") or the end of the list
        if top and entry:
            name = next(l.split()[-1] for l in entry if re.match(r'[ -]{4}\.name:', l))
            if name in out:
                out[name][2] = entry
                for l in entry:
                    m = re.match(r'[ -]{4}(\.\w+):\s+(\S+)$', l)
                    if m and m.group(1) in FIELDS:
                        out[name][3][m.group(1)] = m.group(2)
            entry = []
        if not lines[i].startswith('  '):
            break
        entry.append(lines[i])
        i += 1
    return out


def demangle(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True)
    short = [re.sub(r'^void pcs::', '', re.sub(r'\(.*', '', l)) for l in r.stdout.split('\n')]
    return dict(zip(names, short))


def compare(a, b):
    if a is None or b is None:
        return 'different', ['only in ' + ('B' if a is None else 'A')]
    diff = [f'{f} {a[3].get(f)} -> {b[3].get(f)}' for f in FIELDS if a[3].get(f) != b[3].get(f)]
    same_meta = a[1] == b[1] and a[2] == b[2]
    if same_meta and a[0] == b[0]:
        return 'identical', []
    if same_meta and collections.Counter(a[0]) == collections.Counter(b[0]):
        moved = sum(x != y for x, y in zip(a[0], b[0]))
        return 'reordered', diff + [f'{moved} of {len(a[0])} lines at another place']
    ca, cb = collections.Counter(a[0]), collections.Counter(b[0])
    return 'different', diff + [f'{sum((ca - cb).values())} lines only in A, {sum((cb - ca).values())} only in B']


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('tree_a')
    ap.add_argument('tree_b')
    ap.add_argument('--units', default=','.join(UNITS))
    ap.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument('--keep', help='directory for the .s files (default: a temporary one)')
    args = ap.parse_args()
    units = args.units.split(',')
    tmp = None if args.keep else tempfile.TemporaryDirectory()
    work = args.keep or tmp.name
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max(1, min(16, args.jobs))) as ex:
        for side, tree in (('a', args.tree_a), ('b', args.tree_b)):
            os.makedirs(os.path.join(work, side), exist_ok=True)
            for u in units:
                jobs[side, u] = ex.submit(compile_unit, os.path.abspath(tree), u,
                                          os.path.abspath(os.path.join(work, side, u + '.s')))
    count = collections.Counter()
    for u in units:
        ka, kb = parse(jobs['a', u].result()), parse(jobs['b', u].result())
        names = sorted(set(ka) | set(kb))
        short = demangle(names)
        for n in names:
            verdict, notes = compare(ka.get(n), kb.get(n))
            count[verdict] += 1
            print(f'{u:9s} {verdict:10s} {short[n]}' + (': ' + '; '.join(notes) if notes else ''))
    print('total: ' + ', '.join(f'{count[v]} {v}' for v in ('identical', 'reordered', 'different')))
    return 1 if count['different'] else 0


if __name__ == '__main__':
    sys.exit(main())
