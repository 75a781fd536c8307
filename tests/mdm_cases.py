"""Cases, references and the error bound of the Green-function and matrix-free MappedDistanceMatrix tests
(tests/test_green_host.py, tests/test_gpu_mdm.py, tests/golden/make_golden_green.py).

Inputs.  ``points(dim)``: P = rng.random((130, dim)), Q = rng.random((600, dim)), x and y standard normal, all
rounded to fp32 so that both dtypes and the reference see the same numbers (a difference of two fp32 coordinates
then has a RELATIVE error in fp32, which is what the bound below assumes).  ``sphere()``: the dim = 3 points
recentred, normalised and rounded, columns drawn until every |<P_i, Q_j>| > 1e-3 (asserted): an inner product at
the jump of a k = 1 causal function could legitimately fall on either side.

The fixture (tests/golden/green_mdm.npz, from the reference's own classes, fp64) holds stacked arrays indexed by
the orders of the tuples below:
  eval[f]            the function FUNCS[f] on EVAL_R (0, the support edges, negative values)
  sweep_fwd[f, o]    the dense reference operator of FUNCS[f], ord ORDS[o], on P[:65], Q[:257] (dim 2) applied to x
  sweep_adj[f, o]    its adjoint applied to y
  zonal_fwd / _adj   the same for ZONAL_FUNCS on the sphere
  shape[d, c]        Matern(1, 0.5), ord 2, all 130 rows against Q[:NCOLS[c]] in dim DIMS[d] (row i of a product
                     depends on P_i alone, so the first nrows entries serve every nrows of the sweep)
  sym_fwd            samples2 = None on P[:65] (dim 2), Matern(1, 0.5)

The bound.  With u = 2^-24 or 2^-53,
    |out_l - ref_l| <= C u sum_k |x_k| (|phi(d_lk)| + s_lk |phi'(d_lk)|),
s = d in radial mode (the distance carries a relative error), s = 1 in zonal mode (the inner product an absolute
one); phi' is a central difference in fp64 (relative step 1e-6 in radial mode, so it never crosses 0; absolute
1e-6 in zonal mode, where |d| > 1e-3).  A plain |Phi| |x| bound cannot hold: near the edge of a Wendland support the
entry is a cancellation.  C = 32: ``model`` below evaluates the same formulas in fp32 NumPy (sums in fp64) and the
host test holds it to C / 2 on every case; nothing in C is measured on the device code.
"""

import numpy as np

C = 32
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
NP, NQ = 130, 600
SWEEP = (65, 257)                       # rows past one tile, columns past one slab
DIMS = (1, 2, 3, 4)
ORDS = (2.0, 1.0, np.inf, 0.8, 3.0)
NROWS = (1, 4, 16, 17, 63, 64, 65, 130)
NCOLS = (1, 255, 256, 257, 600)
EVAL_N = (1, 63, 64, 65, 1000)

# name -> (class name, constructor arguments)
FUNCS = (
    ('matern0', 'Matern', (0, 0.5)), ('matern1', 'Matern', (1, 0.5)), ('matern2', 'Matern', (2, 0.5)),
    ('matern3', 'Matern', (3, 0.5)),
    ('wendland0', 'Wendland', (0, 0.75)), ('wendland1', 'Wendland', (1, 0.75)), ('wendland2', 'Wendland', (2, 0.75)),
    ('wendland3', 'Wendland', (3, 0.75)),
    ('subgauss08', 'SubGaussian', (0.8, 0.5)), ('subgauss15', 'SubGaussian', (1.5, 0.5)),
    ('iter1', 'CausalGreenIteratedDerivative', (1,)), ('iter2', 'CausalGreenIteratedDerivative', (2,)),
    ('iter4', 'CausalGreenIteratedDerivative', (4,)),
    ('cexp1', 'CausalGreenExponential', (1, 1.5)), ('cexp2', 'CausalGreenExponential', (2, 1.5)),
    ('cexp4', 'CausalGreenExponential', (4, 1.5)),
)
FUNC_NAMES = tuple(f[0] for f in FUNCS)
ZONAL_FUNCS = ('matern1', 'matern3', 'wendland1', 'wendland2', 'iter1', 'iter2', 'iter4', 'cexp1', 'cexp2', 'cexp4')
SHAPE_FUNC = 'matern1'


def make(G, name):
    """FUNCS[name] built from the classes of module ``G`` (this package's or the reference's)."""
    _, cls, args = FUNCS[FUNC_NAMES.index(name)]
    return getattr(G, cls)(*args)


def rounded(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def ord_tag(o):
    return 'inf' if np.isinf(o) else str(o).replace('.', 'p')


_cache = {}


def points(dim):
    """(P (130, dim), Q (600, dim), x (600), y (130)), fp32-exact fp64 arrays (read-only, shared)."""
    if ('pts', dim) not in _cache:
        rng = np.random.default_rng([61, dim])
        out = tuple(rounded(a) for a in (rng.random((NP, dim)), rng.random((NQ, dim)), rng.standard_normal(NQ),
                                         rng.standard_normal(NP)))
        for a in out:
            a.setflags(write=False)
        _cache['pts', dim] = out
    return _cache['pts', dim]


def sphere():
    """(P (130, 3), Q (600, 3), x, y) on the unit sphere with every |<P_i, Q_j>| > 1e-3."""
    if 'sphere' not in _cache:
        P0, _, x, y = points(3)
        unit = lambda a: rounded(a / np.linalg.norm(a, axis=-1, keepdims=True))  # noqa: E731
        P = unit(P0 - 0.5)
        rng = np.random.default_rng([67, 3])
        cols = []
        while len(cols) < NQ:
            q = unit(rng.random(3) - 0.5)
            if np.min(np.abs(P @ q)) > 2e-3:
                cols.append(q)
        Q = np.stack(cols)
        ip = P @ Q.T
        assert np.min(np.abs(ip)) > 1e-3 and np.min(ip) < -0.5 and np.max(ip) > 0.5
        for a in (P, Q):
            a.setflags(write=False)
        _cache['sphere'] = (P, Q, x, y)
    return _cache['sphere']


EVAL_R = rounded(np.concatenate([[0.0, 0.5, 0.75, 1.5, 1e-3, 0.7499, 0.7501], np.linspace(-1.0, 3.0, 41),
                                 np.geomspace(1e-2, 2.0, 12)]))
EVAL_R.setflags(write=False)


# ---------------------------------------------------------------- fp64 reference and bound

def distances(P, Q, mode, ord):
    """d(P_i, Q_j) as MappedDistanceMatrix forms it (fp64 for fp64 inputs)."""
    if mode == 'radial':
        return np.linalg.norm(P[:, None, :] - Q[None, :, :], axis=-1, ord=ord)
    return np.clip(np.sum(P[:, None, :] * Q[None, :, :], axis=-1), a_min=-1, a_max=1)


def slope_term(func, d, mode):
    """s |phi'(d)| by central differences in fp64: s = d with a relative step (radial; also the element-wise
    evaluation tests), s = 1 with an absolute step (zonal)."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(all='ignore'):
        if mode == 'radial':
            t = np.abs(np.asarray(func(d * (1 + 1e-6))) - np.asarray(func(d * (1 - 1e-6)))) / 2e-6
            return np.where(d == 0, 0.0, t)
        return np.abs(np.asarray(func(d + 1e-6)) - np.asarray(func(d - 1e-6))) / 2e-6


def entry_bound(func, d, mode):
    """|phi(d)| + s |phi'(d)|, the bound of one entry in units of C u."""
    with np.errstate(all='ignore'):
        return np.abs(np.asarray(func(np.asarray(d, dtype=np.float64)), dtype=np.float64)) + slope_term(func, d, mode)


def product_bound(func, P, Q, x, mode, ord):
    """sum_k |x_k| (|phi| + s |phi'|) per row, in units of C u."""
    return entry_bound(func, distances(P, Q, mode, ord), mode) @ np.abs(x)


def units(got, ref, bnd, u):
    """max |got - ref| / (u bnd) over the elements: to be held to C (inf for a NaN that the reference does not
    have, or the reverse)."""
    got, ref, bnd = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, bnd))
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan) or not np.all(np.isfinite(got[~nan])):
        return float('inf')
    err, b = np.abs(got - ref)[~nan], u * bnd[~nan]
    if err.size == 0:
        return 0.0
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / b)
    return float(np.max(r))


# ---------------------------------------------------------------- the fp32 model

def model(func, P, Q, x, mode, ord):
    """The product with distances and phi in fp32 NumPy and fp64 sums: what an fp32 kernel of these formulas
    computes, up to the order of its operations."""
    f32 = np.float32
    P, Q = P.astype(f32), Q.astype(f32)
    if mode == 'radial':
        diff = P[:, None, :] - Q[None, :, :]
        if ord == 2:
            d = np.sqrt(np.sum(diff * diff, axis=-1, dtype=f32))
        elif ord == 1:
            d = np.sum(np.abs(diff), axis=-1, dtype=f32)
        elif np.isinf(ord):
            d = np.max(np.abs(diff), axis=-1)
        else:
            d = np.power(np.sum(np.power(np.abs(diff), f32(ord)), axis=-1, dtype=f32), f32(1.0 / ord))
    else:
        d = np.clip(np.sum(P[:, None, :] * Q[None, :, :], axis=-1, dtype=f32), f32(-1), f32(1))
    phi = np.asarray(func(d))
    assert d.dtype == f32 and phi.dtype == f32, (d.dtype, phi.dtype)
    return (phi.astype(np.float64) * x[None, :]).sum(axis=1)


def sweep_inputs(mode):
    """(P, Q, x, y) of the class / ord sweep and of the zonal cases: the SWEEP prefix of the dim-2 points or of
    the sphere."""
    P, Q, x, y = points(2) if mode == 'radial' else sphere()
    return P[:SWEEP[0]], Q[:SWEEP[1]], x[:SWEEP[1]], y[:SWEEP[0]]


def sweep_cases():
    """(mode, function name, ord, index into the fixture's stacked arrays)."""
    out = [('radial', f, o, (i, j)) for i, f in enumerate(FUNC_NAMES) for j, o in enumerate(ORDS)]
    return out + [('zonal', f, 2.0, (i,)) for i, f in enumerate(ZONAL_FUNCS)]
