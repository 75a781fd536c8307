"""Proximal Langevin sampler (mirrors ``pycsou/opt/mcmc.py``).

``PMYULA`` has the reference's signature, validation, hyperparameter rules, iterand keys and diagnostics
columns.  One iteration is ``F._grad`` on the device plus one launch (``pcs_myula_step``: prox of the G kinds the
fused APGD step knows, the four-term update and the noise); one retained sample is one more launch
(``pcs_mcmc_accumulate``: both running moments, every P-square state and the diagnostic's two sums).  Because the
reference's ``stopping_metric`` is always ``inf`` the loop length is known in advance, so ``iterate`` never waits
for the device: the diagnostic sums go to a device history that is read once when the run ends.

The reference draws its noise from an undefined module global ``rng`` (``mcmc.py:112``); the constructor builds
``self.rng`` and using it is the evident intent.  ``noise='numpy'`` does exactly that (host draw, one upload per
iteration: the parity mode); ``noise='philox'`` (default) generates the normals inside the step kernel.
"""

from numbers import Number

import numpy as np
import torch

from .. import _ops as O
from ..core.functional import ProximableFunctional
from ..core.map import DifferentiableMap
from ..core.solver import GenericIterativeAlgorithm
from ..func.base import NullDifferentiableFunctional, NullProximableFunctional
from ..util.stats import P2Algorithm
from .proxalgs import _find_arrays, _wants_torch

COLUMNS = ['Iter', 'Relative Improvement (MMSE)', 'Nb of samples']


def mcmc_retained(it, nb_burnin_iterations, thinning_factor):
    """Whether iteration ``it`` (0-based) contributes a sample (``mcmc.py:123-124``): a pure function of the
    iteration index."""
    return bool(it > max(nb_burnin_iterations, 4) and (it - nb_burnin_iterations) % thinning_factor == 0)


def mcmc_iterations(max_iter, min_iter, accuracy_threshold=0.0):
    """Number of iterations ``iterate`` runs (``solver.py:65-66`` with a stopping metric that is always inf)."""
    it = 0
    while ((it <= max_iter) and (np.inf > accuracy_threshold)) or (it <= min_iter):
        it += 1
    return it


def mcmc_count(max_iter, min_iter, nb_burnin_iterations, thinning_factor, accuracy_threshold=0.0):
    """Number of retained samples of a full run."""
    n = mcmc_iterations(max_iter, min_iter, accuracy_threshold)
    return sum(mcmc_retained(it, nb_burnin_iterations, thinning_factor) for it in range(n))


class _Moments:
    """Running sum, running sum of squares and P2 states of one retained stream (the chain, or a linop of it)."""

    def __init__(self, n, dtype, dev, pvalues):
        self.total = torch.zeros(n, dtype=dtype, device=dev)
        self.total_sq = torch.zeros(n, dtype=dtype, device=dev)
        self.state = O.P2State(() if pvalues is None else pvalues, n, dtype, dev)


class PMYULA(GenericIterativeAlgorithm):
    """``mcmc.py:14-208``; one extra keyword, ``noise='philox' | 'numpy'``."""

    def __init__(self, dim, F=None, G=None, tau=None, gamma=None, x0=None, max_iter=1e5, min_iter=200, beta=None,
                 accuracy_threshold=1e-5, nb_burnin_iterations=1000, thinning_factor=100, verbose=1, seed=0,
                 linops=None, store_mcmc_samples=False, pvalues=(0.10, 0.9), noise='philox'):
        if noise not in ('philox', 'numpy'):
            raise ValueError(f"noise must be 'philox' or 'numpy', got {noise!r}")
        self.dim = dim
        self.seed = seed
        self.noise = noise
        self.rng = np.random.default_rng(seed=seed)
        self.linops = linops
        self.nb_burnin_iterations = nb_burnin_iterations
        self.thinning_factor = thinning_factor
        self.store_mcmc_samples = store_mcmc_samples
        self.mcmc_samples = []
        self.pvalues = pvalues
        self.count = 0
        if isinstance(F, DifferentiableMap):
            if F.shape[1] != dim:
                raise ValueError(f'F does not have the proper dimension: {F.shape[1]}!={dim}.')
            self.F = F
            if F.diff_lipschitz_cst < np.inf:
                self.beta = self.F.diff_lipschitz_cst if beta is None else beta
            elif (beta is not None) and isinstance(beta, Number):
                self.beta = beta
            else:
                raise ValueError('F must be a differentiable functional with Lipschitz-continuous gradient.')
        elif F is None:
            self.F = NullDifferentiableFunctional(dim=dim)
            self.beta = 0
        else:
            raise TypeError(f'F must be of type {DifferentiableMap}.')
        if isinstance(G, ProximableFunctional):
            if G.dim != dim:
                raise ValueError(f'G does not have the proper dimension: {G.dim}!={dim}.')
            self.G = G
        elif G is None:
            self.G = NullProximableFunctional(dim=dim)
        else:
            raise TypeError(f'G must be of type {ProximableFunctional}.')
        if (tau is not None) and (gamma is not None):
            self.tau, self.gamma = tau, gamma
        elif tau is not None:
            self.tau = tau
            self.gamma = tau / (self.F.diff_lipschitz_cst * tau + 1)
        else:
            self.tau, self.gamma = self.set_hyperparameters()
        self._torch_out = _wants_torch(x0, F)
        self.x0 = x0 if isinstance(x0, torch.Tensor) else (np.asarray(x0) if x0 is not None
                                                           else self.initialize_mcmc())
        init_iterand = {'init_mcmc_sample': self.x0, 'mmse_raw': self.x0}
        super().__init__(objective_functional=self.F + self.G, init_iterand=init_iterand, max_iter=max_iter,
                         min_iter=min_iter, accuracy_threshold=accuracy_threshold, verbose=verbose)
        self._dev = None
        self._rows = []

    def set_hyperparameters(self):
        if isinstance(self.G, NullProximableFunctional):
            tau = None
            gamma = 1 / self.beta
        else:
            tau = 2 / self.beta
            gamma = tau / (self.beta * tau + 1)
        return tau, gamma

    def initialize_mcmc(self):
        return np.zeros(shape=(self.dim,), dtype=np.float64)

    # ------------------------------------------------------------ device state

    def _compute_dtype(self):
        for a in [self.x0] + _find_arrays(self.F):
            if isinstance(a, torch.Tensor) and a.dtype in (torch.float32, torch.float64):
                return a.dtype
            if isinstance(a, np.ndarray) and a.dtype in (np.float32, np.float64):
                return torch.float32 if a.dtype == np.float32 else torch.float64
        return torch.float64

    def _out(self, t):
        return t if self._torch_out else t.detach().cpu().numpy()

    def _start(self):
        """Fresh device state: the chain at x0, empty moments."""
        from .engine import apgd_g_kind
        dtype = self._compute_dtype()
        x = O.to_dev(self.x0, dtype).clone()
        if x.numel() != self.dim:
            raise ValueError(f'x0 does not have the proper dimension: {x.numel()}!={self.dim}.')
        self.rng = np.random.default_rng(seed=self.seed)
        self.count = 0
        self.mcmc_samples = []
        if isinstance(self.G, NullProximableFunctional):
            prox = 'none'
            gk = None
        else:
            gk = apgd_g_kind(self.G)
            prox = 'buffer' if gk is None else 'kind'
        lin = [] if self.linops is None else [_Moments(int(op.shape[0]), dtype, x.device, self.pvalues)
                                              for op in self.linops]
        self._dev = {'x': x, 'raw': _Moments(self.dim, dtype, x.device, self.pvalues), 'lin': lin, 'prox': prox,
                     'gk': gk, 'scratch': torch.zeros(2, dtype=torch.float64, device=x.device),
                     'lin_scratch': torch.zeros(2, dtype=torch.float64, device=x.device)}

    def _step(self, it, sums):
        """Iteration ``it`` on the device (``mcmc.py:112-137``); the diagnostic's two sums go to ``sums`` when the
        sample is retained.  Returns whether it was."""
        d = self._dev
        x = d['x']
        g = self.F._grad(x)
        z = None
        if self.noise == 'numpy':
            z = O.to_dev(self.rng.standard_normal(size=self.dim), x.dtype)
        if d['prox'] == 'none':
            xn = O.myula_step(x, g, None, self.gamma, z=z, seed=self.seed, it=it)
        elif d['prox'] == 'kind':
            xn = O.myula_step(x, g, self.tau, self.gamma, gk=d['gk'], z=z, seed=self.seed, it=it)
        else:
            xn = O.myula_step(x, g, self.tau, self.gamma, p=self.G._prox(x, self.tau), z=z, seed=self.seed, it=it)
        d['x'] = xn
        if self.store_mcmc_samples:
            self.mcmc_samples.append(self._out(xn))
        if not mcmc_retained(it, self.nb_burnin_iterations, self.thinning_factor):
            return False
        self.count += 1
        O.mcmc_accumulate(xn, d['raw'].total, d['raw'].total_sq, d['raw'].state, sums)
        for op, m in zip(self.linops or (), d['lin']):
            O.mcmc_accumulate(op._apply(xn), m.total, m.total_sq, m.state, d['lin_scratch'])
        return True

    def _p2_views(self, m):
        if self.pvalues is None:
            return None
        return [P2Algorithm._view(m.state, k, self._torch_out) for k in range(m.state.K)]

    def _iterand(self):
        """The reference's iterand dict (``mcmc.py:139-143``) from the device state."""
        d = self._dev
        have = self.count > 0
        raw = d['raw']
        it = {'mcmc_sample': self._out(d['x']), 'mmse_raw': self._out(raw.total.clone()) if have else 0,
              'second_moment_raw': self._out(raw.total_sq.clone()) if have else 0, 'p2_raw': self._p2_views(raw)}
        if self.linops is not None:
            it['mmse_linops'] = [self._out(m.total.clone()) if have else 0 for m in d['lin']]
            it['second_moment_linops'] = [self._out(m.total_sq.clone()) if have else 0 for m in d['lin']]
            it['p2_linops'] = [self._p2_views(m) for m in d['lin']]
        return it

    # ------------------------------------------------------------ solver interface

    def update_iterand(self):
        if self._dev is None or self.iter == 0:
            self._start()
        self._last = (self._step(self.iter, self._dev['scratch']), self.count)
        return self._iterand()

    def iterate(self):
        """The reference loop (``solver.py:55-76``) without a host synchronisation: the schedule is a function of
        the iteration index, and the diagnostic sums of every retained sample land in a device history."""
        self._start()
        d = self._dev
        n_iter = mcmc_iterations(self.max_iter, self.min_iter, self.accuracy_threshold)
        n_ret = sum(mcmc_retained(it, self.nb_burnin_iterations, self.thinning_factor) for it in range(n_iter))
        hist = torch.zeros((n_ret + 1, 2), dtype=torch.float64, device=d['x'].device)
        O.reduce_dev(0, d['x'], out=hist[n_ret, 0:1])  # ||x0||^2: the first row's 'old' MMSE is x0 (mcmc.py:73)
        kept = []
        for it in range(n_iter):
            self.iter = it
            kept.append(self._step(it, hist[min(self.count, n_ret - 1)] if n_ret else d['scratch']))
        self.iter = n_iter
        h = hist.cpu().numpy()
        rows, count = [], 0
        for it in range(n_iter):
            if it == 0:
                rel = np.inf if h[n_ret, 0] == 0 else 1.0  # ||x0 - 0|| / ||x0||
            elif kept[it]:
                x2, s2 = h[count]
                rel = np.inf if s2 == 0 else float(np.sqrt(x2) / np.sqrt(s2))
            else:
                rel = np.inf if count == 0 else 0.0  # the sum did not move
            count += int(kept[it])
            rows.append([it, rel, count])
        self._rows = rows
        from pandas import DataFrame
        self.diagnostics = DataFrame(rows, columns=COLUMNS)
        if self.verbose is not None:
            for row in rows[::self.verbose]:
                print(dict(zip(COLUMNS, row)))
        self.converged = True
        self.iterand = self._iterand()
        self.iterand = self.postprocess_iterand()
        return self.iterand, self.converged, self.diagnostics

    def postprocess_iterand(self):
        """``mcmc.py:146-184``, once per run, in the reference's own NumPy arithmetic on the downloaded sums."""
        def host(a):
            return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a

        def back(a):
            return O.to_dev(a, self._dev['x'].dtype) if self._torch_out else a

        def moments(total, total_sq):
            mean = host(total) / self.count
            second = host(total_sq) / self.count
            return back(mean), back(np.sqrt(second - mean ** 2))

        def quantiles(p2):
            return None if self.pvalues is None else [pp.q for pp in p2]

        it = self.iterand
        mmse_raw, std_raw = moments(it['mmse_raw'], it['second_moment_raw'])
        if self.linops is None:
            return {'mcmc_sample': it['mcmc_sample'], 'mmse': mmse_raw, 'std': std_raw,
                    'quantiles': quantiles(it['p2_raw']), 'pvalues': self.pvalues}
        lin = [moments(a, b) for a, b in zip(it['mmse_linops'], it['second_moment_linops'])]
        return {'mcmc_sample': it['mcmc_sample'], 'mmse_raw': mmse_raw, 'std_raw': std_raw,
                'quantiles_raw': quantiles(it['p2_raw']), 'mmse_linops': [m for m, _ in lin],
                'std_linops': [s for _, s in lin], 'quantiles_linops': [quantiles(p) for p in it['p2_linops']],
                'pvalues': self.pvalues}

    def stopping_metric(self):
        return np.inf

    def print_diagnostics(self):
        print(dict(zip(COLUMNS, self._rows[-1])))

    def update_diagnostics(self):
        """API-level twin of the history read in ``iterate`` (one read-back per call)."""
        if self.iter == 0:
            self._rows = []
        kept, count = self._last
        old = self.old_iterand['mmse_raw']
        if kept and count > 1:
            x2, s2 = self._dev['scratch'].tolist()
            rel = np.inf if s2 == 0 else float(np.sqrt(x2) / np.sqrt(s2))
        elif isinstance(old, Number) or O.norm(O.to_dev(old)) == 0:
            rel = np.inf
        else:
            rel = 1.0 if self.iter == 0 else 0.0
        self._rows.append([self.iter, rel, count])
        from pandas import DataFrame
        self.diagnostics = DataFrame(self._rows, columns=COLUMNS)
