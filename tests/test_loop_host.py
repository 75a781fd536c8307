"""The host arithmetic of the shared device loop control (pycsou_amd/opt/_loop.py): how many history rows a
loop allocates at its start and how the history grows, against tables written out here; and the named
fields of the control block (pcs::Ctrl, csrc/pds_ctrl.hpp: six int32 fields, 48 bytes = 12 int32)."""

import itertools

import pytest

from pycsou_amd.opt import _loop

BIG = 10 ** 9

# (total, chunk) -> rows: min(total, max(4096, 2 * chunk))
INITIAL = {
    (1, 2): 1, (5, 2): 5, (4096, 2): 4096, (4097, 2): 4096, (BIG, 2): 4096,
    (1, 32): 1, (5, 32): 5, (4096, 32): 4096, (4097, 32): 4096, (BIG, 32): 4096,
    (1, 4096): 1, (5, 4096): 5, (4096, 4096): 4096, (4097, 4096): 4097, (BIG, 4096): 8192,
}

# (have, need, total) -> rows
GROWN = {
    # need == have: nothing to do, whatever the total
    (8, 8, 7): 8, (8, 8, 8): 8, (8, 8, 9): 8, (8, 8, BIG): 8,
    (64, 64, 63): 64, (64, 64, 64): 64, (64, 64, 65): 64, (64, 64, BIG): 64,
    (4096, 4096, 4095): 4096, (4096, 4096, 4096): 4096, (4096, 4096, 4097): 4096, (4096, 4096, BIG): 4096,
    # need == have + 1: doubled, at most the total; a history that already holds the total stays
    (8, 9, 7): 8, (8, 9, 8): 8, (8, 9, 9): 9, (8, 9, 16): 16, (8, 9, 17): 16, (8, 9, BIG): 16,
    (64, 65, 63): 64, (64, 65, 64): 64, (64, 65, 65): 65, (64, 65, 128): 128, (64, 65, 129): 128, (64, 65, BIG): 128,
    (4096, 4097, 4095): 4096, (4096, 4097, 4096): 4096, (4096, 4097, 4097): 4097, (4096, 4097, 8192): 8192,
    (4096, 4097, 8193): 8192, (4096, 4097, BIG): 8192,
    # need == 2 * have + 1: past the doubling
    (8, 17, 7): 8, (8, 17, 8): 8, (8, 17, 9): 9, (8, 17, 16): 16, (8, 17, 17): 17, (8, 17, 18): 17, (8, 17, BIG): 17,
    (64, 129, 63): 64, (64, 129, 64): 64, (64, 129, 65): 65, (64, 129, 128): 128, (64, 129, 129): 129,
    (64, 129, 130): 129, (64, 129, BIG): 129,
    (4096, 8193, 4095): 4096, (4096, 8193, 4096): 4096, (4096, 8193, 4097): 4097, (4096, 8193, 8192): 8192,
    (4096, 8193, 8193): 8193, (4096, 8193, 8194): 8193, (4096, 8193, BIG): 8193,
}


def test_hist_chunk():
    assert _loop.HIST_CHUNK == 4096


@pytest.mark.parametrize('total,chunk', sorted(INITIAL))
def test_initial_rows_table(total, chunk):
    assert _loop.initial_rows(total, chunk) == INITIAL[total, chunk]


@pytest.mark.parametrize('total,chunk,up_front', [(5, 2, 7), (BIG, 32, 42), (1, 4096, 1), (4097, 2, 4097)])
def test_initial_rows_up_front_is_exact(total, chunk, up_front):
    assert _loop.initial_rows(total, chunk, up_front) == up_front


@pytest.mark.parametrize('have,need,total', sorted(GROWN))
def test_grown_rows_table(have, need, total):
    assert _loop.grown_rows(have, need, total) == GROWN[have, need, total]


def test_grown_rows_properties():
    for have, need, total in itertools.product((1, 8, 41, 64, 4096), (1, 8, 9, 17, 42, 4097, 8193, BIG),
                                               (1, 7, 8, 9, 41, 4096, 8193, BIG)):
        g = _loop.grown_rows(have, need, total)
        assert _loop.grown_rows(g, need, total) == g, (have, need, total)  # a fixed point
        if g != have:  # it grew: never above the total, and room for what was asked up to the total
            assert have < g <= total and g >= min(need, total), (have, need, total, g)


def test_loop_control_field_indices():
    C = _loop.LoopControl
    idx = [C.IT, C.STOPPED, C.MIN_ITER, C.MAX_ITER, C.HAS_DUAL, C.HIST_LEN]
    assert len(set(idx)) == 6 and all(0 <= i < 12 for i in idx)
    assert 8 * C.THR >= 4 * (max(idx) + 1) and 8 * (C.THR + 1) <= 48  # the double lies behind the int32 fields
