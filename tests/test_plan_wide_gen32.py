"""Planner and layout of the geneing wide kernel's 32-row ring instances
(kernels_persist_wide_gen.hip k_persist_wide_gen32): host only, through
wrnn_debug_plan / wrnn_debug_stream_bytes with flag 256 (the 32-row instances are available and
selected, as after wrnn_set_gen_wide_rows(32); it needs flag 128, the in-kernel conditioning, and
the head's wide image flag), the rate keys wide_gen32 / wide_gen32_mol / wide_gen32_beta, and the
library's checks of the doubled exchange layout.

A 32-row launch (17 .. 32 rows per XCD group) exists only as a ring instance, so it enters only
plans whose launches are all wide; without flag 256 every answer is what it was.
"""
import pytest

from test_plan_wide_gen import plan
from test_plan_wide_gen_ring import streams

FAT, RR, GEN = 0, 1, 2
RAW, MOL, BETA = 0, 1, 2
RING, WIDE, RR_MOL, GEN_MOL, GEN_BETA, GEN_FRAMES, GEN32 = 2, 4, 16, 32, 64, 128, 256
S = 6000
# (mode, the head's wide image flag, its 32-row rate key, a cheap table: below twice the head's
# 16-row rate, so one 32-row launch beats two 16-row ones)
HEADS = [pytest.param(RAW, WIDE, 'wide_gen32', 'wide_gen32 4.2 0.01', id='bits'),
         pytest.param(MOL, GEN_MOL, 'wide_gen32_mol', 'wide_gen32_mol 3.6 0.01', id='mol'),
         pytest.param(BETA, GEN_BETA, 'wide_gen32_beta', 'wide_gen32_beta 5.8 0.03', id='beta')]
KEYS = ('wide_gen32', 'wide_gen32_mol', 'wide_gen32_beta')
ROWS = (33, 131, 152, 360, 2115)

# the built-in plans of the fork default 8-utterance call (360 rows = 45 per group) with 32 rows
# selected, by the shipped wide_gen32* rates (profiles/wide_gen32/summary.md)
DEFAULT_360_GEN32 = {RAW: [(13, True), (32, True)], MOL: [(16, True), (29, True)], BETA: [(16, True), (29, True)]}


def test_layout_of_both_tiles_has_no_violation():
    from wavernn_amd import _abi
    lib = _abi.load_library()
    assert [lib.wrnn_debug_wide_gen32_layout(r) for r in range(1, 33)] == [0] * 32
    assert lib.wrnn_debug_wide_gen32_layout(0) == _abi.WRNN_ERR_INVALID
    assert lib.wrnn_debug_wide_gen32_layout(33) == _abi.WRNN_ERR_INVALID
    for n in (30, 2):
        assert [lib.wrnn_debug_wide_gen32_mol_layout(r, n) for r in range(1, 33)] == [0] * 32
        assert lib.wrnn_debug_wide_gen32_mol_layout(0, n) == _abi.WRNN_ERR_INVALID
        assert lib.wrnn_debug_wide_gen32_mol_layout(33, n) == _abi.WRNN_ERR_INVALID
    for n in (0, 1, 7, 29, 31, 32, 512):
        assert lib.wrnn_debug_wide_gen32_mol_layout(8, n) == _abi.WRNN_ERR_INVALID
    # (the 16-row entry points keep their range)
    assert lib.wrnn_debug_wide_gen_layout(17) == _abi.WRNN_ERR_INVALID
    assert lib.wrnn_debug_wide_gen_mol_layout(17, 30) == _abi.WRNN_ERR_INVALID


@pytest.mark.parametrize('mode, flag, key, cheap', HEADS)
@pytest.mark.parametrize('rows', ROWS)
def test_a_dear_key_leaves_the_plan_as_without_the_flag(rows, mode, flag, key, cheap):
    for seq in (1200, S):
        base = plan(rows, S=seq, mode=mode, flags=flag)
        assert plan(rows, S=seq, mode=mode, flags=flag | GEN_FRAMES | GEN32, table=f'{key} 100 1') == base


@pytest.mark.parametrize('mode, flag, key, cheap', HEADS)
@pytest.mark.parametrize('rows', ROWS)
def test_the_keys_price_only_their_head_and_only_with_the_flag(rows, mode, flag, key, cheap):
    tables = [f'{k} {v}' for k in KEYS for v in ('0.1 0.001', '100 1')]
    # a call without flag 256: no key of the three matters (with or without the in-kernel form)
    for fl in (flag, flag | GEN_FRAMES):
        base = plan(rows, mode=mode, flags=fl)
        for t in tables:
            assert plan(rows, mode=mode, flags=fl, table=t) == base, t
    # with the flag: the other heads' keys do not matter
    base = plan(rows, mode=mode, flags=flag | GEN_FRAMES | GEN32)
    for t in tables:
        if t.split()[0] != key:
            assert plan(rows, mode=mode, flags=flag | GEN_FRAMES | GEN32, table=t) == base, t


@pytest.mark.parametrize('model, mode, rows, seq, flags', [
    (FAT, RAW, 144, 12100, RING | WIDE), (FAT, MOL, 144, 12100, RING | WIDE),
    (RR, RAW, 232, 8000, RING | WIDE), (RR, MOL, 232, 8000, RING | WIDE | RR_MOL)])
def test_other_topologies_read_neither_flag_nor_keys(model, mode, rows, seq, flags):
    base = plan(rows, S=seq, model=model, bits=9, mode=mode, flags=flags)
    sb = streams(rows, seq=seq, model=model, bits=9, mode=mode, flags=flags)
    every = flags | GEN_MOL | GEN_BETA | GEN_FRAMES | GEN32
    assert plan(rows, S=seq, model=model, bits=9, mode=mode, flags=every) == base
    assert streams(rows, seq=seq, model=model, bits=9, mode=mode, flags=every) == sb
    for k in KEYS:
        for v in ('0.1 0.001', '100 1'):
            assert plan(rows, S=seq, model=model, bits=9, mode=mode, flags=every, table=f'{k} {v}') == base


@pytest.mark.parametrize('mode, flag, key, cheap', HEADS)
def test_a_cheap_key_plans_32_row_launches(mode, flag, key, cheap):
    fl = flag | GEN_FRAMES | GEN32
    # 4 and 5 utterances of 45 rows: 23 and 29 rows per group in one launch instead of two
    assert plan(180, mode=mode, flags=fl, table=cheap) == ([(23, True)], 0)
    assert plan(225, mode=mode, flags=fl, table=cheap) == ([(29, True)], 0)
    assert len(plan(180, mode=mode, flags=flag)[0]) == 2
    # 8 utterances: two launches instead of three, all wide, rows 0 .. 359 once (launch k runs the
    # rows from 8 x the rows per group of the launches before it: 45 per group in all, no padding)
    p, rot = plan(360, mode=mode, flags=fl, table=cheap)
    assert rot == 0 and len(p) == 2 and all(w for _, w in p), p
    assert all(1 <= nr <= 32 for nr, _ in p) and sum(nr for nr, _ in p) == 45, p
    assert max(nr for nr, _ in p) > 16, p


@pytest.mark.parametrize('mode, flag, key, cheap', HEADS)
@pytest.mark.parametrize('rows', [1, 8, 18, 24, 32])
def test_calls_of_at_most_32_rows_keep_their_plans(rows, mode, flag, key, cheap):
    for seq in (1200, S, 14000):
        base = plan(rows, S=seq, mode=mode, flags=flag)
        for t in (cheap, f'{key} 0.1 0.001', None):
            assert plan(rows, S=seq, mode=mode, flags=flag | GEN_FRAMES | GEN32, table=t) == base


@pytest.mark.parametrize('mode, flag, key, cheap', HEADS)
def test_no_32_row_launch_without_the_ring_or_the_image(mode, flag, key, cheap):
    for rows in (180, 225, 360, 2115):
        base = plan(rows, mode=mode, flags=flag)
        # flag 256 without flag 128: the call would write streams
        assert plan(rows, mode=mode, flags=flag | GEN32, table=cheap) == base
        assert streams(rows, mode=mode, flags=flag | GEN32) == streams(rows, mode=mode, flags=flag)
        # ... and without the head's wide image there is no wide launch at all
        p, _ = plan(rows, mode=mode, flags=GEN_FRAMES | GEN32, table=cheap)
        assert p and not any(w for _, w in p), p


@pytest.mark.parametrize('mode, flag, key, cheap', HEADS)
def test_a_mixed_plan_holds_no_32_row_launch(mode, flag, key, cheap):
    """Rates that make the register-resident launches the cheapest for a remainder: whatever the
    32-row key, a plan with a register-resident launch has no launch above 16 rows per group."""
    for t in (cheap, f'{key} 3.6 0.0001', f'{key} 2.0 0.05'):
        for rows in (33, 131, 137, 152, 265, 360):
            for tt in (t, t + '\ngen 0.5 0.6 0.7 0.8'):
                p, _ = plan(rows, S=1200, mode=mode, flags=flag | GEN_FRAMES | GEN32, table=tt)
                assert p
                if not all(w for _, w in p):
                    assert all(nr <= 16 for nr, w in p if w), (rows, tt, p)


@pytest.mark.parametrize('mode, flag, key, cheap', HEADS)
def test_a_32_row_plan_takes_the_ring(mode, flag, key, cheap):
    """Built-in rates: 180 rows are one launch of 23 rows per group; it writes no P1 stream and,
    for BITS, no noise (MOL keeps its [S][Bp][12] draws, Bp padded to the launch: 8 x 23)."""
    fl = flag | GEN_FRAMES | GEN32
    assert plan(180, mode=mode, flags=fl) == ([(23, True)], 0)
    assert streams(180, mode=mode, flags=fl) == (0, S * 184 * 12 * 4 if mode == MOL else 0, 1)
    p, _ = plan(2115, mode=mode, flags=fl)
    assert all(w for _, w in p) and max(nr for nr, _ in p) > 16, p
    Bp = 8 * sum(nr for nr, _ in p)
    assert streams(2115, mode=mode, flags=fl) == (0, S * Bp * 12 * 4 if mode == MOL else 0, 1)


def test_large_batch_stays_on_the_persistent_engine():
    assert streams(2115, flags=WIDE | GEN_FRAMES | GEN32)[2] == 1
    assert streams(2880, flags=WIDE | GEN_FRAMES | GEN32) == (0, 0, 1)


@pytest.mark.parametrize('mode, flag, key, cheap', HEADS)
def test_built_in_plan_of_the_fork_default_batch(mode, flag, key, cheap):
    """(the plans profiles/wide_gen32/summary.md reports for the shipped rates)"""
    assert plan(360, mode=mode, flags=flag | GEN_FRAMES | GEN32) == (DEFAULT_360_GEN32[mode], 0)
    assert plan(360, mode=mode, flags=flag | GEN_FRAMES) == ([(13, True), (16, True), (16, True)], 0)


@pytest.mark.parametrize('table', ['wide_gen32 5', 'wide_gen32_mol 5 0.1 3', 'wide_gen32_beta 5 x', 'wide_gen32 5 -1'])
def test_malformed_lines_are_refused(table):
    with pytest.raises(ValueError):
        plan(360, table=table)
