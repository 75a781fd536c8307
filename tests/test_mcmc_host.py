"""Host side of the PMYULA sampler and the P-square estimator: the exported symbols, the Philox4x32-10 known
answers, the host twin of the P2 update against the reference fixture (bit for bit), the host normals, and the
host logic of PMYULA (hyperparameters, schedule, validation, alias).  No GPU."""

import os

import numpy as np
import pytest

from tests import mcmc_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mcmc.npz')
NEW_SYMBOLS = ('pcs_p2_update', 'pcs_p2_update_host', 'pcs_mcmc_accumulate', 'pcs_myula_step', 'pcs_mcmc_normal',
               'pcs_mcmc_philox', 'pcs_mcmc_philox_host', 'pcs_mcmc_normal_host')


@pytest.fixture(scope='module')
def lib():
    from pycsou_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_exports_and_abi(lib):
    from pycsou_amd import _lib
    assert lib.pcs_abi_version() == 10 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


# ---------------------------------------------------------------- Philox
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers(lib, ctr, key, want):
    c, k, o = np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    assert lib.pcs_mcmc_philox_host(c.ctypes.data, k.ctypes.data, o.ctypes.data) == 0
    assert tuple(int(v) for v in o) == want
    assert lib.pcs_mcmc_philox_host(None, k.ctypes.data, o.ctypes.data) < 0


# ---------------------------------------------------------------- P2 host twin
def host_states(lib, samples, pvalues, dtype, checkpoints=C.P2_CHECKPOINTS):
    """Drive pcs_p2_update_host over a stream; the desired positions are accumulated as add_sample does."""
    from pycsou_amd import _lib as L
    from pycsou_amd._ops import p2_desired
    K, n = len(pvalues), samples.shape[1]
    h, p = np.zeros((K, 5, n), dtype=dtype), np.zeros((K, 3, n), dtype=np.int32)
    des, inc = p2_desired(pvalues)
    out = {}
    for t, row in enumerate(samples, start=1):
        if t > 5:
            des += inc
        x = np.ascontiguousarray(row, dtype=dtype)
        rc = lib.pcs_p2_update_host(L.PCS_F64 if dtype == np.float64 else L.PCS_F32, x.ctypes.data, h.ctypes.data,
                                    p.ctypes.data, n, K, t, des.ctypes.data_as(L._pdbl))
        assert rc == 0
        if t in checkpoints:
            out[t] = (h.copy(), p.copy())
    return out


@pytest.mark.parametrize('kind', C.STREAMS)
@pytest.mark.parametrize('K', [1, 2, 3])
def test_p2_host_fp64_equals_reference_bitwise(lib, golden, kind, K):
    s = C.stream(kind)
    got = host_states(lib, s, C.P2_PVALUES[:K], np.float64)
    rest, _ = C.restated_states(s, C.P2_PVALUES[:K], np.float64)
    for t in C.P2_CHECKPOINTS:
        ref_h, ref_p = golden[f'p2_{kind}_{t}_heights'][:K], golden[f'p2_{kind}_{t}_pos'][:K]
        assert C.same_bits(rest[t][0], ref_h) and C.same_bits(rest[t][1], ref_p), ('restatement', t)
        assert C.same_bits(got[t][0], ref_h), ('heights', t, np.argwhere(got[t][0] != ref_h)[:4])
        assert C.same_bits(got[t][1], ref_p), ('positions', t)


@pytest.mark.parametrize('kind', C.STREAMS)
@pytest.mark.parametrize('K', [1, 2, 3])
def test_p2_host_fp32_equals_float32_restatement_bitwise(lib, kind, K):
    s = C.stream(kind).astype(np.float32)
    got = host_states(lib, s, C.P2_PVALUES[:K], np.float32)
    rest, est = C.restated_states(s, C.P2_PVALUES[:K], np.float32)
    assert all(e.fired['parabolic'] > 0 and e.fired['linear'] > 0 for e in est)
    for t in C.P2_CHECKPOINTS:
        assert C.same_bits(got[t][0], rest[t][0]) and C.same_bits(got[t][1], rest[t][1]), t


def test_p2_host_rejects_bad_arguments(lib):
    from pycsou_amd import _lib as L
    x, h, p = np.zeros(4), np.zeros((9, 5, 4)), np.zeros((9, 3, 4), dtype=np.int32)
    des = np.zeros((9, 5))
    args = lambda **kw: [kw.get('dt', L.PCS_F64), kw.get('x', x.ctypes.data), h.ctypes.data, p.ctypes.data,
                         kw.get('n', 4), kw.get('K', 1), 1, des.ctypes.data_as(L._pdbl)]
    assert lib.pcs_p2_update_host(*args()) == 0
    for bad in (dict(dt=7), dict(x=None), dict(n=-1), dict(K=9), dict(K=0)):
        assert lib.pcs_p2_update_host(*args(**bad)) < 0, bad


# ---------------------------------------------------------------- host normals
def normals(lib, seed, it, n, stream=0):
    out = np.empty(n, dtype=np.float32)
    assert lib.pcs_mcmc_normal_host(seed, it, stream, n, out.ctypes.data) == 0
    return out


def check_normal_statistics(draw):
    """The bounds of the issue at n = 65536: draw(seed, iteration, n) -> float array."""
    n = 65536
    a, b, c = draw(3, 0, n).astype(np.float64), draw(3, 1, n).astype(np.float64), draw(4, 0, n).astype(np.float64)
    assert abs(a.mean()) <= 5 / np.sqrt(n)
    assert abs(a.var() - 1) <= 5 * np.sqrt(2 / n)
    for other in (b, c):
        assert abs(np.corrcoef(a, other)[0, 1]) <= 5 / np.sqrt(n)
    assert np.array_equal(draw(3, 0, n), draw(3, 0, n))
    assert np.array_equal(draw(3, 0, 1001), draw(3, 0, n)[:1001])


def test_normal_host_statistics_and_determinism(lib):
    check_normal_statistics(lambda seed, it, n: normals(lib, seed, it, n))
    assert not np.array_equal(normals(lib, 3, 0, 64, stream=0), normals(lib, 3, 0, 64, stream=1))
    assert lib.pcs_mcmc_normal_host(0, 0, 0, -1, normals(lib, 0, 0, 4).ctypes.data) < 0


# ---------------------------------------------------------------- PMYULA host logic
def _problem():
    from pycsou_amd.func import L1Norm
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.linop.base import DenseLinearOperator
    A, y, x0 = C.dense_problem()
    op = DenseLinearOperator(A)
    op.lipschitz_cst = op.diff_lipschitz_cst = float(np.linalg.norm(A, 2))
    F = (1 / 2) * SquaredL2Loss(dim=A.shape[0], data=y) * op
    return F, C.DENSE_LAM * L1Norm(dim=A.shape[1]), A.shape[1]


def test_hyperparameter_branches(golden):
    from pycsou_amd.opt.mcmc import PMYULA
    F, G, dim = _problem()
    beta = F.diff_lipschitz_cst
    assert beta == pytest.approx(float(golden['dense_l1_beta']), rel=1e-12)
    s = PMYULA(dim=dim, F=F, G=G, verbose=None)
    assert s.tau == 2 / beta and s.gamma == s.tau / (beta * s.tau + 1)
    assert (s.tau, s.gamma) == pytest.approx((float(golden['dense_l1_tau']), float(golden['dense_l1_gamma'])), rel=1e-12)
    s = PMYULA(dim=dim, F=F, G=None, verbose=None)
    assert s.tau is None and s.gamma == 1 / beta
    s = PMYULA(dim=dim, F=F, G=G, tau=0.01, verbose=None)
    assert s.tau == 0.01 and s.gamma == 0.01 / (beta * 0.01 + 1)
    s = PMYULA(dim=dim, F=F, G=G, tau=0.01, gamma=0.002, verbose=None)
    assert (s.tau, s.gamma) == (0.01, 0.002)
    assert s.init_iterand['init_mcmc_sample'].dtype == np.float64 and s.rng is not None


def test_schedule_is_a_host_function():
    from pycsou_amd.opt.mcmc import mcmc_count, mcmc_iterations, mcmc_retained
    assert mcmc_iterations(120, 1) == 121 and mcmc_iterations(10, 200) == 201
    assert mcmc_count(120, 1, 20, 3) == C.DENSE_COUNT
    assert mcmc_count(300, 1, 50, 5) == 50
    for burnin, thin in ((20, 3), (0, 1), (2, 2), (7, 4)):
        kept = [it for it in range(60) if mcmc_retained(it, burnin, thin)]
        assert kept and min(kept) > max(burnin, 4)
        assert all((it - burnin) % thin == 0 for it in kept)
    assert [it for it in range(12) if mcmc_retained(it, 0, 1)] == list(range(5, 12))


def test_validation_errors():
    from pycsou_amd.func import L1Norm
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.opt.mcmc import PMYULA
    F, G, dim = _problem()
    with pytest.raises(ValueError, match='F does not have the proper dimension'):
        PMYULA(dim=dim + 1, F=F, G=None)
    with pytest.raises(ValueError, match='G does not have the proper dimension'):
        PMYULA(dim=dim, F=F, G=L1Norm(dim=dim + 1))
    with pytest.raises(TypeError, match='F must be of type'):
        PMYULA(dim=dim, F='F')
    with pytest.raises(TypeError, match='G must be of type'):
        PMYULA(dim=dim, F=F, G='G')
    from pycsou_amd.linop.base import DenseLinearOperator
    unbounded = SquaredL2Loss(dim=24, data=np.zeros(24)) * DenseLinearOperator(C.dense_problem()[0])
    assert unbounded.diff_lipschitz_cst == np.inf
    with pytest.raises(ValueError, match='Lipschitz-continuous gradient'):
        PMYULA(dim=dim, F=unbounded)
    assert PMYULA(dim=dim, F=unbounded, beta=3.0, verbose=None).beta == 3.0
    with pytest.raises(ValueError, match='noise'):
        PMYULA(dim=dim, F=F, noise='mt19937')


def test_alias_modules():
    import pycsou_amd
    pycsou_amd.install_alias()
    from pycsou.opt.mcmc import PMYULA
    from pycsou.util import P2Algorithm, is_range_broadcastable, peaks, range_broadcast_shape  # noqa: F401
    from pycsou.util.stats import P2Algorithm as P2
    assert PMYULA is pycsou_amd.opt.mcmc.PMYULA and P2 is P2Algorithm
    p = P2Algorithm(pvalue=0.95)
    assert p.pvalue == 0.95 and p.count == 0 and p.q is None and p.marker_heights is None
    np.testing.assert_array_equal(p.desired_marker_positions, [1, 1 + 2 * 0.95, 1 + 4 * 0.95, 3 + 2 * 0.95, 5])
    np.testing.assert_array_equal(p.increments, [0, 0.95 / 2, 0.95, 1.95 / 2, 1])
