"""CPU tier of the device eigenvalue solver (pycsou/core/linop.py:208-219): the NumPy oracle ``spectral_ref``, the
solver itself with ``orth='torch'`` on the CPU and SciPy's ``eigsh``, each against the exact spectrum within the
bound of tests/spectral_cases.py; the measured constants behind that bound; the new C-ABI entry points, their size
functions and argument checks (they run before any device call); the ``k`` ranges; the data conditions of the exact
one-launch cases.  No compute calls on a GPU."""

import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

from tests import scratch as S
from tests import spectral_cases as SC
from tests.cases import GOLDEN

NEW_SYMBOLS = ('pcs_orth_state_bytes', 'pcs_orth_nblocks', 'pcs_orth_state_init', 'pcs_orth_dots',
               'pcs_orth_update', 'pcs_orth_commit')
SWEEP = [(name, which, tol) for name, which in SC.COMBOS for tol in SC.TOLS]
IDS = [f'{n}-{w}-{t:g}' for n, w, t in SWEEP]


def _torch_cpu(name, which, tol, **kw):
    from pycsou_amd import _ops as O
    M = torch.as_tensor(SC.sym(name))
    return O.eigsh_restarted(lambda v: torch.mv(M, v), M.shape[0], SC.CASES[name][1], SC.gram_which(name, which),
                             tol=tol, orth='torch', device='cpu', **kw)


def _scipy(name, which, tol):
    """None where ARPACK itself gives up: the zero matrix ('Starting vector is zero')."""
    if name == 'zeros_sym':
        return None
    return spla.eigsh(SC.sym(name), k=SC.CASES[name][1], which=SC.gram_which(name, which), tol=tol,
                      return_eigenvectors=False)


# ---------------------------------------------------------------- the references and the CPU solver within the bound
@pytest.mark.parametrize('name,which,tol', SWEEP, ids=IDS)
def test_oracle_solver_and_scipy_within_the_bound(name, which, tol):
    tol = SC.case_tol(name, tol)
    want, bnd = SC.wanted(name, which), SC.bound(name, which, tol)
    got = {'spectral_ref': SC.spectral_ref(SC.sym(name), SC.CASES[name][1], SC.gram_which(name, which), tol=tol)[0],
           'torch_cpu': _torch_cpu(name, which, tol), 'scipy': _scipy(name, which, tol)}
    for key, val in got.items():
        if val is None:
            continue
        val = np.sort(np.asarray(val, dtype=np.float64))
        err = np.abs(val - want)
        print(f'SPECTRAL host {name} {which} tol {tol:g} {key}: worst err / bound {np.max(err / bnd):.3g}')
        assert val.shape == want.shape and np.all(err <= bnd), (key, err, bnd)
    assert np.all(np.diff(got['torch_cpu']) >= 0) and got['torch_cpu'].dtype == np.float64      # ascending, as eigsh


def test_measured_ratios():
    """The figures behind C and ORTH_BOUND (module docstring of spectral_cases): printed, and still covered."""
    worst = {'spectral_ref': 0.0, 'scipy': 0.0}
    for name, which in SC.COMBOS:
        if SC.case_tol(name, 0.0) != 0.0:
            continue
        got = {'spectral_ref': SC.spectral_ref(SC.sym(name), SC.CASES[name][1], SC.gram_which(name, which))[0],
               'scipy': _scipy(name, which, 0.0)}
        for key, val in got.items():
            if val is not None:
                r = SC.ratio(name, which, 0.0, val)
                print(f'SPECTRAL ratio {name} {which} {key}: {r:.2f}')
                worst[key] = max(worst[key], r)
    V = SC.ref_basis(SC.sym('sym_dense'), 20)
    orth = float(np.abs(V @ V.T - np.eye(21)).max())
    print(f'SPECTRAL worst ratios {worst}, C = {SC.C}; orthogonality of the oracle basis {orth:.3e}, bar '
          f'{SC.ORTH_BOUND:.3e}')
    assert SC.C == 2.0 ** np.ceil(np.log2(8 * max(SC.RATIO_REF, SC.RATIO_SCIPY)))
    assert 8 * max(worst.values()) <= SC.C and orth <= SC.ORTH_BOUND == 8 * SC.ORTH_REF


@pytest.mark.parametrize('name,which', [c for c in SC.COMBOS if c[0] not in SC.BREAKDOWN_CASES],
                         ids=lambda v: str(v))
def test_wanted_values_are_simple(name, which):
    """Neighbouring values are more than two bounds apart: the exact spectrum is an oracle for every one."""
    for tol in SC.TOLS:
        assert SC.separation(name, which, SC.case_tol(name, tol)) > 2.0


def test_breakdown_cases_known_answers():
    """The doctest operator (0.5 x a shift: the Krylov space has dimension 2) gives three singular values of 0.5
    to 1e-12, the homothety [2, 2, 2], the zero matrix zeros."""
    s = np.sqrt(np.maximum(_torch_cpu('conv1d_doc', 'LM', 1e-3), 0.0))
    assert s.shape == (3,) and np.all(np.abs(s - 0.5) <= 1e-12), s
    assert np.sum(np.abs(SC.spectrum('conv1d_doc') - 0.25) < 1e-14) == 29
    for which in SC.WHICH_EIG:
        assert np.all(np.abs(_torch_cpu('homothety', which, 0.0) - 2.0) <= 1e-14)
        assert np.array_equal(_torch_cpu('zeros_sym', which, 0.0), np.zeros(3))
    from pycsou_amd import _ops as O
    assert O.spectral_ncv(5, 2) == 5 == SC.sym('tiny').shape[0] and O.spectral_ncv(1480, 6) == 20     # tiny: m = n


def test_select_follows_arpack():
    lam = np.array([-5.0, -2.0, 0.5, 1.0, 3.0, 4.0])
    from pycsou_amd import _ops as O
    for which, want in (('LA', [1.0, 3.0, 4.0]), ('SA', [-5.0, -2.0, 0.5]), ('LM', [-5.0, 3.0, 4.0]),
                        ('BE', [-5.0, 3.0, 4.0])):
        assert np.array_equal(lam[SC.select(lam, 3, which)], want)
        assert np.array_equal(O.spectral_select(lam, 3, which), SC.select(lam, 3, which))
    S6 = np.diag(lam) + 0.0
    assert np.allclose(np.sort(spla.eigsh(S6, k=3, which='BE', return_eigenvectors=False)), [-5.0, 3.0, 4.0])


def test_start_vector_and_reproducibility():
    a = _torch_cpu('gauss_tall', 'LM', 0.0)
    assert np.array_equal(a, _torch_cpu('gauss_tall', 'LM', 0.0))                       # seeded: the same bits
    v0 = np.random.default_rng(5).standard_normal(80)
    b = _torch_cpu('gauss_tall', 'LM', 0.0, v0=v0)
    assert np.all(np.abs(b - SC.wanted('gauss_tall', 'LM')) <= SC.bound('gauss_tall', 'LM', 0.0))
    c = _torch_cpu('gauss_tall', 'LM', 0.0, ncv=12)
    assert np.all(np.abs(c - SC.wanted('gauss_tall', 'LM')) <= SC.bound('gauss_tall', 'LM', 0.0))


# ---------------------------------------------------------------- non-convergence and the argument ranges
def test_no_convergence_carries_the_converged_values():
    with pytest.raises(spla.ArpackNoConvergence) as e:
        _torch_cpu('grad2d', 'LM', 0.0, maxiter=1)
    assert hasattr(e.value, 'eigenvalues') and len(e.value.eigenvalues) < 6
    with pytest.raises(spla.ArpackNoConvergence) as e:
        SC.spectral_ref(SC.sym('grad2d'), 6, 'LA', maxiter=1)
    assert hasattr(e.value, 'eigenvalues')


def test_k_and_keyword_ranges():
    from pycsou_amd import _ops as O
    from pycsou_amd.linop import DenseLinearOperator
    ident = lambda v: v     # noqa: E731
    for k in (0, -1, 10, 11):
        with pytest.raises(ValueError):
            O.eigsh_restarted(ident, 10, k, 'LA', orth='torch', device='cpu')
    for bad in (dict(which='SM'), dict(which='XX'), dict(ncv=3), dict(ncv=11), dict(orth='numpy'),
                dict(v0=np.zeros(10)), dict(v0=np.ones(9))):
        kw = dict(which='LA', orth='torch', device='cpu')
        kw.update(bad)
        with pytest.raises(ValueError):
            O.eigsh_restarted(ident, 10, 3, **kw)
    with pytest.raises(ValueError):
        O.eigsh_restarted(ident, 1000, 3, 'LA', ncv=257, orth='hip', device='cpu')
    A = DenseLinearOperator(SC.matrix('tiny'), is_symmetric=True)
    for k in (0, 5, 6):
        with pytest.raises(ValueError):
            A.eigenvals(k)
    G = DenseLinearOperator(SC.matrix('gauss_tall'))
    for k in (0, 80, 81):
        with pytest.raises(ValueError):
            G.singularvals(k)
    assert A._device_spectral(5, 2, dict(tol=1e-3, ncv=4, maxiter=5, v0=None, return_eigenvectors=False),
                              'return_eigenvectors') == dict(tol=1e-3, ncv=4, maxiter=5, v0=None)
    for kw in (dict(sigma=0.0), dict(return_eigenvectors=True), dict(ncv=257), dict(mode='normal')):
        assert A._device_spectral(1000, 2, kw, 'return_eigenvectors') is None
    assert A._device_spectral(1000, 128, {}, 'return_eigenvectors') is None             # default ncv = 257


# ---------------------------------------------------------------- the exact one-launch data
@pytest.mark.parametrize('rows', SC.ROWS)
@pytest.mark.parametrize('n', SC.ONE_N + (SC.BIG_N,))
def test_exact_data_conditions(n, rows):
    V, w, h_in = SC.one_launch(n, rows, 3)
    assert V.shape == (rows + 1, n + 3) and np.abs(V[:, :n]).max() <= 3 and np.all(V[:, n:] == 7)
    assert np.all(np.abs(h_in) <= 2) and np.array_equal(2 * h_in, np.rint(2 * h_in))
    S.assert_exact(V[:rows, :n] * w, w * w, bits=53)                                   # the summands of dots
    terms = np.concatenate([w[None], -h_in[:rows, None] * V[:rows, :n]])               # the running sum of update
    S.assert_exact(terms.T, scale=0.5, bits=53)
    wn, h = SC.update_ref(V, w, h_in, n, rows)
    S.assert_exact(V[:rows, :n] * wn, wn * wn, scale=0.25, bits=53)
    assert np.abs(wn).max() <= 3 + 2 * 3 * rows and h.shape == (rows + 1,)


def test_constants_of_the_one_launch_cases():
    from pycsou_amd import _lib, _ops
    assert (SC.GROUP, SC.TILE, SC.CAP) == (_lib.PCS_ORTH_GROUP, _lib.PCS_ORTH_TILE, _lib.PCS_ORTH_MAX_BLOCKS)
    assert (_ops.ORTH_MAX_M, _ops.ORTH_GROUP) == (256, SC.GROUP)
    assert set(SC.ROWS) >= {1, 2, SC.GROUP - 1, SC.GROUP, SC.GROUP + 1, 20, 41}
    reg = _lib.PCS_ORTH_REG_ROWS                       # pcs_orth_update changes kernel after 8, 16 and 24 rows
    assert reg == 24 and set(SC.ROWS) >= {8, 9, 16, 17, reg, reg + 1}
    assert SC.BIG_N == SC.CAP * SC.TILE + 3


# ---------------------------------------------------------------- the C ABI
def test_new_symbols_exported_abi_unchanged():
    from pycsou_amd import _lib, _ops
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pcs_abi_version() == 10 and _lib.ABI_VERSION == 10
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'pycsou_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert f'{name}(' in header
    for macro, val in (('PCS_ORTH_MAX_M', 256), ('PCS_ORTH_GROUP', SC.GROUP), ('PCS_ORTH_MAX_BLOCKS', SC.CAP),
                       ('PCS_ORTH_REG_ROWS', 24)):
        assert f'#define {macro} {val}' in header and getattr(_lib, macro) == val
    for name in ('orth_dots', 'orth_update', 'orth_commit', 'orth_state', 'orth_partials', 'orth_state_init',
                 'eigsh_restarted'):
        assert callable(getattr(_ops, name))


def test_scratch_sizes():
    from pycsou_amd import _lib
    lib = _lib.load()
    assert [lib.pcs_orth_state_bytes(m) for m in (1, 2, 20, 256)] == [8 * (m * m + 2 * m + 1) for m in (1, 2, 20, 256)]
    assert lib.pcs_orth_state_bytes(0) == -1 == lib.pcs_orth_state_bytes(-3) and lib.pcs_orth_state_bytes(257) == -3
    bps = {n: lib.pcs_orth_nblocks(n, 1) // 2 for n in (0, 1, 512, 513, SC.CAP * 512, SC.CAP * 512 + 1, 1 << 33)}
    assert bps == {0: 1, 1: 1, 512: 1, 513: 2, SC.CAP * 512: SC.CAP, SC.CAP * 512 + 1: SC.CAP, 1 << 33: SC.CAP}
    assert lib.pcs_orth_nblocks(513, 20) == 21 * 2 and lib.pcs_orth_nblocks(SC.BIG_N, 256) == 257 * SC.CAP
    assert lib.pcs_orth_nblocks(-1, 1) == -1 == lib.pcs_orth_nblocks(5, 0) and lib.pcs_orth_nblocks(5, 257) == -3


N_, LDV = 100, 104
VB, W, H1, H2, H3, PA, ST = (0x10000000 * k for k in range(1, 8))   # stand-in addresses: never dereferenced


def _call(lib, which, **over):
    kw = dict(V=VB, ldv=LDV, s=4, m=20, w=W, n=N_, h=H1, h_in=H1, h_out=H2, h1=H1, h2=H2, h3=H3, brk=1e-14,
              partials=PA, state=ST)
    kw.update(over)
    order = {'dots': ('V', 'ldv', 's', 'w', 'n', 'h', 'partials'),
             'update': ('V', 'ldv', 's', 'w', 'n', 'h_in', 'h_out', 'partials'),
             'commit': ('V', 'ldv', 's', 'm', 'w', 'n', 'h1', 'h2', 'h3', 'brk', 'state')}[which]
    return getattr(lib, f'pcs_orth_{which}')(*[kw[k] for k in order], None)


ROWS_END = VB + 8 * (5 * LDV + N_)      # one past row s + 1 = 5 of the basis
COMMON_BAD = {'V': dict(V=None), 'w': dict(w=None), 'n_neg': dict(n=-1), 's_neg': dict(s=-1), 'ldv': dict(ldv=N_ - 1),
              'w_in_row0': dict(w=VB), 'w_in_next_row': dict(w=ROWS_END - 8), 'w_below': dict(w=VB - 8 * (N_ - 1))}
INF, NAN = float('inf'), float('nan')
BAD = {
    'dots': dict(COMMON_BAD, h=dict(h=None), partials=dict(partials=None)),
    'update': dict(COMMON_BAD, h_in=dict(h_in=None), h_out=dict(h_out=None), partials=dict(partials=None),
                   h_alias=dict(h_out=H1)),
    'commit': dict(COMMON_BAD, h1=dict(h1=None), h2=dict(h2=None), h3=dict(h3=None), state=dict(state=None),
                   s_is_m=dict(s=20), s_above_m=dict(s=21), m0=dict(m=0, s=0), brk_neg=dict(brk=-1e-14),
                   brk_inf=dict(brk=INF), brk_nan=dict(brk=NAN)),
}


@pytest.mark.parametrize('which,bad', [(w, b) for w in sorted(BAD) for b in sorted(BAD[w])])
def test_argument_checks(which, bad):
    """Every bad-argument case returns PCS_EINVAL before any device call (no GPU here)."""
    from pycsou_amd import _lib
    assert _call(_lib.load(), which, **BAD[which][bad]) == -1


def test_basis_limit_is_unsupported():
    from pycsou_amd import _lib
    lib = _lib.load()
    assert _call(lib, 'dots', s=256) == -3 == _call(lib, 'update', s=256)
    assert _call(lib, 'commit', m=257, s=0) == -3 == _call(lib, 'commit', m=257, s=256)
    assert _call(lib, 'commit', m=257, s=0, n=-1) == -1                    # a bad argument is still reported first
    assert lib.pcs_orth_state_init(ST, 257, None) == -3
    assert lib.pcs_orth_state_init(None, 20, None) == -1 == lib.pcs_orth_state_init(ST, 0, None)
