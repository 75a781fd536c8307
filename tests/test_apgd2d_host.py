"""Host side of the fused APGD engine (no GPU): problem matching, the chunked momentum coefficients and
the C ABI's support query."""

import ctypes

import numpy as np
import pytest

from pycsou_amd import _lib
from pycsou_amd.opt.engine import apgd_coeffs, match_apgd2d
from tests.apgd2d_cases import psf_of


def _problem(shape=(32, 32), psf='gauss15', g='l1'):
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm, L21Norm
    from pycsou_amd.linop.conv import Convolve2D
    N = shape[0] * shape[1]
    C = Convolve2D(N, psf_of(psf), shape)
    C.lipschitz_cst = C.diff_lipschitz_cst = 1.0
    F = (1 / 2) * SquaredL2Loss(dim=N, data=np.linspace(0.0, 1.0, N)) * C
    G = 0.1 * (L1Norm(dim=N) if g == 'l1' else L21Norm(dim=N, groups=np.tile(np.arange(N // 2), 2)))
    return F, G


def test_match_apgd2d_takes_the_separable_blur_problem():
    from pycsou_amd.func.penalty import NonNegativeOrthant, Segment
    F, G = _problem()
    spec = match_apgd2d(F, G)
    assert spec is not None and spec['shape'] == (32, 32) and spec['sep'][2] == 7
    assert spec['gkind'] == _lib.PCS_APGD_G_L1 and spec['lam'] == 0.1
    assert match_apgd2d(F, None)['gkind'] == _lib.PCS_G_NULL
    assert match_apgd2d(F, NonNegativeOrthant(1024))['gkind'] == _lib.PCS_G_NONNEG
    s = match_apgd2d(F, Segment(1024, 0.0, 1.0))
    assert s['gkind'] == _lib.PCS_G_SEGMENT and tuple(s['seg']) == (0.0, 1.0)
    # different factors on the two axes: padded to the common half width
    assert match_apgd2d(*_problem(psf='rank1_5x9'))['sep'][2] == 4
    # n1 % 4 != 0 matches as a problem; the library's support query is what refuses the image
    assert match_apgd2d(*_problem(shape=(32, 30))) is not None


def test_match_apgd2d_refuses_the_rest():
    from pycsou_amd.func.loss import SquaredL2Loss
    from pycsou_amd.func.penalty import L1Norm
    from pycsou_amd.linop.base import DenseLinearOperator
    from pycsou_amd.linop.conv import Convolve2D
    assert match_apgd2d(*_problem(psf='nonsep7')) is None
    assert match_apgd2d(*_problem(g='l21')) is None
    A = DenseLinearOperator(np.arange(32.0).reshape(4, 8))
    A.lipschitz_cst = A.diff_lipschitz_cst = 1.0
    assert match_apgd2d((1 / 2) * SquaredL2Loss(dim=4, data=np.ones(4)) * A, 0.1 * L1Norm(dim=8)) is None
    assert match_apgd2d(None, None) is None
    # half width 8
    N = 40 * 40
    t = np.ones(17) / 17
    C = Convolve2D(N, np.outer(t, t), (40, 40))
    C.lipschitz_cst = C.diff_lipschitz_cst = 1.0
    assert match_apgd2d((1 / 2) * SquaredL2Loss(dim=N, data=np.ones(N)) * C, None) is None


def _ref_coeffs(acceleration, d, n):
    """pycsou/opt/proxalgs.py:592-598, iteration by iteration."""
    out, t_old = [], 1
    for it in range(n):
        if acceleration == 'BT':
            t = (1 + np.sqrt(1 + 4 * t_old ** 2)) / 2
        elif acceleration == 'CD':
            t = (it + d) / d
        else:
            t = t_old = 1
        out.append((t_old - 1) / t)
        t_old = t
    return out, t_old


@pytest.mark.parametrize('acc', ['CD', 'BT', None])
@pytest.mark.parametrize('chunk', [4, 32])
def test_chunked_momentum_is_the_reference_bitwise(acc, chunk):
    ref, t_ref = _ref_coeffs(acc, 75., 71)
    got, t_old, k = [], 1, 0
    while k < 71:  # chunk after chunk, t carried across the boundary
        n = min(chunk, 71 - k)
        a, t_old = apgd_coeffs(acc, 75., k, n, t_old)
        got += a
        k += n
    assert len(got) == 71
    assert [float(v).hex() for v in got] == [float(v).hex() for v in ref]
    assert t_old == t_ref and type(t_old) is type(t_ref)
    # past_t of n iterations, recomputed from scratch
    assert apgd_coeffs(acc, 75., 0, 8, 1)[1] == _ref_coeffs(acc, 75., 8)[1]


def _args(**kw):
    a = _lib.Apgd2dArgs()
    a.dtype, a.gkind, a.n0, a.n1, a.half = _lib.PCS_F32, _lib.PCS_APGD_G_L1, 64, 64, 7
    a.tau, a.lam = 0.5, 0.1
    for i, f in enumerate(('taps0', 'taps1', 'x', 'xn', 'aux', 'aux_n', 'cty')):
        setattr(a, f, 4096 * (i + 1))  # aligned, distinct; the query dereferences nothing
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_library_exports_and_support_query():
    lib = _lib.load()
    for name in ('pcs_apgd2d_supported', 'pcs_apgd2d_nblocks', 'pcs_apgd2d_ws_bytes', 'pcs_apgd2d_step',
                 'pcs_apgd2d_run'):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    sup = lambda a: lib.pcs_apgd2d_supported(ctypes.byref(a))  # noqa: E731
    assert sup(_args()) == 1
    assert sup(_args(dtype=_lib.PCS_F64)) == 1
    assert sup(_args(half=8)) == 0
    assert sup(_args(n1=18)) == 0
    assert sup(_args(cty=None)) == 0
    assert sup(_args(n0=15)) == 0
    assert sup(_args(xn=4096 * 3)) == 0          # x aliases xn
    assert sup(_args(x=4096 * 3 + 8)) == 0       # off the 16-B grid
    assert sup(_args(n0=1 << 14, n1=1 << 14)) == 0  # 2^30 bytes
    # an unsupported image is refused without a launch
    assert lib.pcs_apgd2d_step(ctypes.byref(_args(n1=18)), 0.0, None) == -3
    assert lib.pcs_apgd2d_run(ctypes.byref(_args(half=8)), _lib.dbls([0.0, 0.0]), 2, None) == -3
    assert lib.pcs_abi_version() == 10 and lib.pcs_ctrl_bytes() == 64
