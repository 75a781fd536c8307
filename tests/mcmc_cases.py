"""Seeded inputs and fresh NumPy definitions for the PMYULA sampler and the P-square estimator
(pycsou/opt/mcmc.py, pycsou/util/stats.py).  Shared by tests/golden/make_golden_mcmc.py (the real reference runs
on these inputs) and by the tests, which regenerate the inputs instead of storing them.

``P2Restated`` is a restatement of the P-square update written here: every pixel goes through the reference's
scalar operations in the reference's order, in float64 or float32, all pixels at once through masks.  It counts
how often the parabolic and the linear branch and the two end replacements fire.  oracle/ is frozen, so it lives
here."""

import numpy as np

# ---------------------------------------------------------------- P2 streams
STREAMS = ('gauss', 'ties', 'ascending', 'descending', 'cauchy')
P2_WIDTH, P2_SAMPLES = 67, 40
P2_CHECKPOINTS = (4, 5, 6, 7, 40)
P2_PVALUES = (0.1, 0.5, 0.9)      # K = 1, 2, 3 take the first K
DOCTEST_Q = 1.51436338            # stats.py:36


def stream(kind, width=P2_WIDTH, samples=P2_SAMPLES):
    """(samples, width) float64; column 0 is held constant.  Zeros are +0.0."""
    rng = np.random.default_rng([31, STREAMS.index(kind), int(width)])
    g = rng.standard_normal((samples, width))
    if kind == 'gauss':
        s = g
    elif kind == 'ties':
        s = np.round(2.0 * g) / 2.0
    elif kind == 'ascending':
        s = np.cumsum(rng.uniform(0.05, 1.0, (samples, width)), axis=0) * rng.uniform(0.5, 2.0, width)
    elif kind == 'descending':
        s = -np.cumsum(rng.uniform(0.05, 1.0, (samples, width)), axis=0) * rng.uniform(0.5, 2.0, width)
    else:
        s = rng.standard_cauchy((samples, width))
    s[:, 0] = 0.75
    return np.ascontiguousarray(s + 0.0)


class P2Restated:
    """One P-square estimator over ``n`` pixels in ``dtype`` arithmetic (d = desired - position in float64)."""

    def __init__(self, pvalue, dtype=np.float64):
        p = float(pvalue)
        self.pvalue, self.dtype, self.count = p, np.dtype(dtype).type, 0
        self.desired = np.array([1, 1 + 2 * p, 1 + 4 * p, 3 + 2 * p, 5], dtype=np.float64)
        self.increments = np.array([0, p / 2, p, (p + 1) / 2, 1], dtype=np.float64)
        self.heights = self.positions = self.q = None
        self.fired = {'parabolic': 0, 'linear': 0, 'low': 0, 'high': 0}

    def add_sample(self, sample):
        T = self.dtype
        s = np.ascontiguousarray(sample, dtype=T).reshape(-1)
        self.count += 1
        c = self.count
        if c == 1:
            self.heights = s[:, None].copy()
            return
        if c <= 5:
            self.heights = np.sort(np.concatenate((self.heights, s[:, None]), axis=1), axis=1)
            if c == 5:
                self.positions = np.tile(np.arange(1, 6, dtype=np.int64), (s.size, 1))
            return
        self.desired = self.desired + self.increments
        q, n = self.heights, self.positions
        low = s < q[:, 0]
        cells = [(q[:, j] <= s) & (s < q[:, j + 1]) for j in range(4)]
        k = np.select([low] + cells, [0, 0, 1, 2, 3], default=-1)
        high = k < 0
        q[low, 0] = s[low]
        q[high, 4] = s[high]
        k[high] = 3
        self.fired['low'] += int(low.sum())
        self.fired['high'] += int(high.sum())
        n += np.arange(5)[None, :] > k[:, None]
        with np.errstate(all='ignore'):
            for i in (1, 2, 3):
                d = self.desired[i] - n[:, i].astype(np.float64)
                move = ((d >= 1) & (n[:, i + 1] - n[:, i] > 1)) | ((d <= -1) & (n[:, i - 1] - n[:, i] < -1))
                sd = np.where(d > 0, 1, -1).astype(np.int64)
                dt = sd.astype(T)
                t1 = ((n[:, i] - n[:, i - 1] + sd).astype(T) * (q[:, i + 1] - q[:, i])) / (n[:, i + 1] - n[:, i]).astype(T)
                t2 = ((n[:, i + 1] - n[:, i] - sd).astype(T) * (q[:, i] - q[:, i - 1])) / (n[:, i] - n[:, i - 1]).astype(T)
                qt = q[:, i] + (dt / (n[:, i + 1] - n[:, i - 1]).astype(T)) * (t1 + t2)
                par = move & (q[:, i - 1] < qt) & (qt < q[:, i + 1])
                lin = move & ~par
                qo = np.where(sd > 0, q[:, i + 1], q[:, i - 1])
                no = np.where(sd > 0, n[:, i + 1], n[:, i - 1])
                ql = q[:, i] + (dt * (qo - q[:, i])) / (no - n[:, i]).astype(T)
                q[:, i] = np.where(par, qt, np.where(lin, ql, q[:, i]))
                n[:, i] += np.where(move, sd, 0)
                self.fired['parabolic'] += int(par.sum())
                self.fired['linear'] += int(lin.sum())
        assert q.dtype == T
        self.q = q[:, 2]


def restated_states(samples, pvalues, dtype, checkpoints=P2_CHECKPOINTS):
    """{checkpoint: (heights (K, 5, n) with unset markers 0, positions (K, 3, n) int32)} in the device layout,
    plus the estimators."""
    est = [P2Restated(p, dtype) for p in pvalues]
    out = {}
    for t, row in enumerate(samples, start=1):
        for e in est:
            e.add_sample(row)
        if t in checkpoints:
            out[t] = device_layout([e.heights for e in est], [e.positions for e in est], dtype)
    return out, est


def device_layout(heights, positions, dtype):
    """Reference-shaped (n, m <= 5) heights and (n, 5) positions (or None) of K estimators -> the layout of
    pcs_p2_update: (K, 5, n) heights with unset markers 0 and (K, 3, n) int32 positions of markers 1..3."""
    K, n = len(heights), heights[0].shape[0]
    h = np.zeros((K, 5, n), dtype=dtype)
    p = np.zeros((K, 3, n), dtype=np.int32)
    for k in range(K):
        m = heights[k].shape[1]
        h[k, :m] = np.asarray(heights[k]).T
        if positions[k] is not None:
            p[k] = np.asarray(positions[k])[:, 1:4].T
    return h, p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- chains
DENSE_SHAPE = (24, 37)
DENSE = dict(max_iter=120, min_iter=1, nb_burnin_iterations=20, thinning_factor=3, pvalues=(0.1, 0.9), seed=5)
DENSE_LAM, DENSE_COUNT = 0.3, 33
DEMO_N = 8
DEMO = dict(max_iter=300, min_iter=1, nb_burnin_iterations=50, thinning_factor=5, pvalues=(0.05, 0.95), seed=7,
            tau=1e-4)
DEMO_RADIUS = 2
PROBLEMS = ('dense_l1', 'dense_null', 'demo')


def dense_problem():
    """A (24 x 37), data y, a non-zero start for the G = None variant."""
    rng = np.random.default_rng(41)
    A = rng.standard_normal(DENSE_SHAPE) / np.sqrt(DENSE_SHAPE[0])
    xs = np.zeros(DENSE_SHAPE[1])
    xs[rng.choice(DENSE_SHAPE[1], 6, replace=False)] = rng.choice([-2.0, 1.5, 3.0], 6)
    y = A @ xs + 0.05 * rng.standard_normal(DENSE_SHAPE[0])
    x0 = 0.3 * rng.standard_normal(DENSE_SHAPE[1])
    return A, y, x0


def demo_signal():
    return np.repeat([0, 2, 1, 3, 0, 2, 0], DEMO_N).astype(np.float64)   # mcmc.py:221


def demo_noise(m):
    return 0.05 * np.random.default_rng(43).standard_normal(m)

