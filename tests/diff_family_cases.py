"""Inputs, parameters and the NumPy definitions shared by the directional-derivative / Integration1D tests and
by ``tests/golden/make_golden_diff_family.py`` (which runs the reference on the same inputs; only outputs
are stored in ``tests/golden/diff_family.npz``).

Definitions (PyLops 1.x, as wrapped by ``pycsou/linop/diff.py:380-774, 1071-1137``):

* first directional derivative: ``Sum(axis 0) * Diagonal(v) * Gradient``, i.e. ``y = (v_0 . D_0 x + v_1 . D_1 x)
  + v_2 . D_2 x`` and adjoint ``sum_k D_k^T (v_k . y)``, with ``oracle.pylops1.Gradient`` for the ``D_k``;
* second directional derivative: ``mask . (-Dv^T Dv x)`` with ``Dv`` centred, the mask zeroing two samples at
  both ends of every axis; adjoint ``-Dv^T Dv (mask . y)``;
* Integration1D: ``step * cumsum`` along the axis; adjoint the same sum from the far end.
"""

import numpy as np

FIXTURE_SHAPES = ((7, 9), (5, 6, 7))
KINDS = ('forward', 'centered', 'backward')
EDGES = (True, False)
STEPS = (0.5, 2.0, 1.25)                  # per axis, non-unit
INT_STEP = 0.5
TV_SHAPE, TV_LAM, TV_ITERS = (40, 33), 0.1, 30
LASSO_ITERS = 60


def f32(a):
    """fp64 values that are exactly representable in fp32, so both dtypes run the same numbers."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def make_x(shape, seed=0):
    rng = np.random.default_rng([11, seed] + [int(s) for s in shape])
    return f32(rng.standard_normal(int(np.prod(shape))))


def make_dirs(shape, field, seed=0):
    """A unit direction per entry, ``(ndim, N)`` in [k][p] order, or one common direction of ``ndim`` values."""
    nd, N = len(shape), int(np.prod(shape))
    rng = np.random.default_rng([13, seed, int(field)] + [int(s) for s in shape])
    v = rng.standard_normal((nd, N if field else 1))
    v /= np.linalg.norm(v, axis=0, keepdims=True)
    return f32(v if field else v[:, 0])


def steps(shape):
    return list(STEPS[:len(shape)]) if len(shape) <= 3 else [STEPS[k % 3] for k in range(len(shape))]


def kill_mask(shape):
    """1 at the entries whose every coordinate i satisfies 2 <= i < n - 2, else 0 (flat)."""
    coords = np.indices(shape).reshape(len(shape), -1)
    keep = [all(2 <= int(c) < n - 2 for c, n in zip(coords[:, p], shape)) for p in range(coords.shape[1])]
    return np.array(keep, dtype=np.float64)


def _vfield(v, shape):
    nd, N = len(shape), int(np.prod(shape))
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.repeat(v, N).reshape(nd, N) if v.size == nd else v.reshape(nd, N)


def first_dir(x, v, shape, step, kind, edge, adjoint=False):
    """fp64 NumPy evaluation of FirstDirectionalDerivative (or its adjoint) at x."""
    from oracle import pylops1 as P
    nd, N = len(shape), int(np.prod(shape))
    G = P.Gradient(tuple(shape), sampling=step, edge=edge, kind=kind)
    vv = _vfield(v, shape)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if adjoint:
        return G.rmatvec((vv * x[None, :]).reshape(-1))
    t = vv * G.matvec(x).reshape(nd, N)
    y = t[0]
    for k in range(1, nd):
        y = y + t[k]
    return y


def second_dir(x, v, shape, step, edge, adjoint=False):
    """fp64 NumPy evaluation of SecondDirectionalDerivative (edge mask included) or its adjoint."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    m = kill_mask(shape)
    if adjoint:
        x = m * x
    w = -first_dir(first_dir(x, v, shape, step, 'centered', edge), v, shape, step, 'centered', edge, adjoint=True)
    return w if adjoint else m * w


def integ(x, shape, axis, step, adjoint=False):
    a = np.asarray(x).reshape(shape)
    if adjoint:
        return (step * np.flip(np.cumsum(np.flip(a, axis), axis=axis), axis)).reshape(-1)
    return (step * np.cumsum(a, axis=axis)).reshape(-1)


def vector_cases():
    """[(tag, shape, field, kind, edge)] of fixture part (a), first directional derivative."""
    out = []
    for shape in FIXTURE_SHAPES:
        for field in (True, False):
            for kind in KINDS:
                for edge in EDGES:
                    tag = 'x'.join(map(str, shape)) + f"_{'field' if field else 'const'}_{kind}_{'edge' if edge else 'noedge'}"
                    out.append((tag, shape, field, kind, edge))
    return out


def second_cases():
    out = []
    for shape in FIXTURE_SHAPES:
        for field in (True, False):
            for edge in EDGES:
                tag = 'x'.join(map(str, shape)) + f"_{'field' if field else 'const'}_{'edge' if edge else 'noedge'}"
                out.append((tag, shape, field, edge))
    return out


def integ_cases():
    return [('129_ax0', (129,), 0)] + [(f'5x6x7_ax{a}', (5, 6, 7), a) for a in range(3)]


LAPLACIAN_SHAPE, LAPLACIAN_WEIGHTS = (7, 9), [3, 0.5]


def tv_problem():
    """Directional-TV denoising inputs at TV_SHAPE: noisy image y, a smooth unit field v and its rotation by
    90 degrees, both ``(2, N)``."""
    n0, n1 = TV_SHAPE
    i, j = np.meshgrid(np.arange(n0), np.arange(n1), indexing='ij')
    img = ((i - 18.0) ** 2 / 150.0 + (j - 15.0) ** 2 / 90.0 < 1.0).astype(np.float64)
    img[5:12, 20:30] = 0.5
    y = f32(img.ravel() + 0.1 * np.random.default_rng(21).standard_normal(n0 * n1))
    theta = 0.6 * np.sin(i / 9.0) + 0.8 * np.cos(j / 7.0)
    v = np.stack([np.cos(theta).ravel(), np.sin(theta).ravel()])
    vp = np.stack([-v[1], v[0]])
    return y, f32(v), f32(vp)


def lasso_signal():
    return np.repeat([0, 2, 1, 3, 0, 2, 0], 32).astype(np.float64)


def lasso_noise(m):
    return 0.05 * np.random.default_rng(0).standard_normal(m)
