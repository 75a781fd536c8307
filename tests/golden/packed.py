"""The stored form of a golden table of [id, record] rows whose records are dicts that mostly agree (or a string,
or null): a few kilobytes of JSON where the rows written out would be hundreds.

  bases    per group (rows of one kind, `group(record)`): the entries every record of the group has, at their
           most common value
  pairs    every distinct (key, value) by which some record departs from its base, once; a nested dict's
           entries are keyed 'outer.inner'
  records  the distinct records, each [group, [pair, ...]] (a string or null as it is)
  rows     per row the index of its record, in the generator's order
  ids      the number of rows and the SHA-256 of their ids joined by newlines: the generator gives the ids, the
           table only pins them

unpack() gives the records back exactly (dict order aside); make_golden_specs.py / make_golden_engines.py check
that before they write."""

import collections
import hashlib
import json


def _flat(d, pre=''):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flat(v, pre + k + '.'))
        else:
            out[pre + k] = v
    return out


def _nested(flat):
    out = {}
    for k, v in flat.items():
        d = out
        *outer, last = k.split('.')
        for o in outer:
            d = d.setdefault(o, {})
        d[last] = v
    return out


def ids_digest(ids):
    return [len(ids), hashlib.sha256('\n'.join(ids).encode()).hexdigest()]


def pack(rows, group=lambda rec: ''):
    rows = json.loads(json.dumps(rows))  # tuples as the lists they are stored as
    flats = {}
    for _, r in rows:
        if isinstance(r, dict):
            flats.setdefault(group(r), []).append(_flat(r))
    bases = {}
    for g, fs in flats.items():
        common = [k for k in fs[0] if all(k in f for f in fs)]
        bases[g] = {k: json.loads(collections.Counter(json.dumps(f[k]) for f in fs).most_common(1)[0][0])
                    for k in common}
    pairs, records, index, rws = {}, [], {}, []
    for _, r in rows:
        if isinstance(r, dict):
            g = group(r)
            dev = [json.dumps([k, v]) for k, v in _flat(r).items() if k not in bases[g] or bases[g][k] != v]
            r = [g, [pairs.setdefault(p, len(pairs)) for p in dev]]
        key = json.dumps(r)
        if key not in index:
            index[key] = len(records)
            records.append(r)
        rws.append(index[key])
    doc = {'ids': ids_digest([k for k, _ in rows]), 'bases': bases, 'pairs': [json.loads(p) for p in pairs],
           'records': records, 'rows': rws}
    assert unpack(doc) == [r for _, r in rows]
    return doc


def unpack(doc):
    """The records of the rows, in order."""
    recs = []
    for r in doc['records']:
        if isinstance(r, list):
            flat = dict(doc['bases'][r[0]])
            flat.update((doc['pairs'][i][0], doc['pairs'][i][1]) for i in r[1])
            r = _nested(flat)
        recs.append(r)
    return [recs[i] for i in doc['rows']]
