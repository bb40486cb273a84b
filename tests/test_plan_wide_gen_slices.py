"""Planner of the geneing wide kernel's time-sliced instances (kernels_persist_wide_gen.hip
k_persist_wide_gen_rot): host only, through wrnn_debug_plan /
wrnn_debug_stream_bytes with flag 1024 (the time-sliced instances are available and selected, as
after wrnn_set_gen_wide_slices(1); it needs flag 128, the in-kernel conditioning, and the head's
wide image flag) and wrnn_debug_slice_plan.

The slices are opt-in: without flag 1024 every answer is what it was. With it, a call of 8 R_g rows
(rows padded to a multiple of 8) with R_g > 16, not a multiple of 16, runs as launches of 16 rows
per group over rotating row sets when `slice[0]` per extra launch plus steps x the head's
wide_gen_slice* key (the measured step of the sliced instances) is below `slice[1]` x the cost of
the plan made otherwise (the 32-row plan included, when 32 rows are selected as well).
"""
import ctypes

import numpy as np
import pytest

from test_plan_wide_gen import DEFAULT_360, plan
from test_plan_wide_gen32 import DEFAULT_360_GEN32
from test_plan_wide_gen_ring import P1_ROW_STEP, streams
from test_rotation import slice_plan

FAT, RR, GEN = 0, 1, 2
RAW, MOL, BETA = 0, 1, 2
RING, WIDE, RR_MOL, GEN_MOL, GEN_BETA, GEN_FRAMES, GEN32, SLICES = 2, 4, 16, 32, 64, 128, 256, 1024
# (mode, the head's wide image flag, noise bytes per row and step of its stream)
HEADS = [pytest.param(RAW, WIDE, 1024 * 4, id='bits'), pytest.param(MOL, GEN_MOL, 12 * 4, id='mol'),
         pytest.param(BETA, GEN_BETA, 0, id='beta')]
ROWS = (33, 45, 131, 136, 144, 152, 360, 2115)
# a table under which any admissible sliced plan is taken, and one under which none is
CHEAP, DEAR = 'slice 0.001 0.999', 'slice 1000000 0.98'


def wide16(k):
    return [(16, True)] * k


@pytest.mark.parametrize('mode, flag, noise', HEADS)
@pytest.mark.parametrize('rows', ROWS)
def test_without_the_flag_nothing_changes(rows, mode, flag, noise):
    """No flag 1024: the slice key does not reach a geneing plan, whatever it says, and the flag
    without its prerequisites (flag 128, the head's image) is no flag."""
    for seq in (1200, 6000):
        for fl in (flag, flag | GEN_FRAMES, flag | GEN_FRAMES | GEN32):
            base = plan(rows, S=seq, mode=mode, flags=fl)
            assert base[0]
            for t in (CHEAP, DEAR):
                assert plan(rows, S=seq, mode=mode, flags=fl, table=t) == base, (fl, t)
        base = plan(rows, S=seq, mode=mode, flags=flag)
        assert plan(rows, S=seq, mode=mode, flags=flag | SLICES, table=CHEAP) == base
        assert streams(rows, seq=seq, mode=mode, flags=flag | SLICES) == streams(rows, seq=seq, mode=mode, flags=flag)
        p, _ = plan(rows, S=seq, mode=mode, flags=GEN_FRAMES | SLICES, table=CHEAP)
        assert p and not any(w for _, w in p), p


def test_default_plans_stay_pinned():
    assert plan(360, flags=WIDE | GEN_FRAMES) == (DEFAULT_360, 0)
    assert plan(136, S=1200, flags=WIDE | GEN_FRAMES) == ([(1, False), (16, True)], 0)


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_136_rows_run_as_17_wide_launches(mode, flag, noise):
    fl = flag | GEN_FRAMES | SLICES
    assert plan(136, S=1200, mode=mode, flags=fl) == (wide16(17), 0)
    K, rs, _ = slice_plan(136, 1200)
    assert K == 17 and rs.tolist() == [[16, 75]] * 17
    # 1,400 steps: 87 per launch, the remaining 8 of every row in tail launches of 16 and 1 rows
    assert plan(136, S=1400, mode=mode, flags=fl) == (wide16(18) + [(1, True)], 0)
    K, rs, _ = slice_plan(136, 1400)
    assert rs.tolist() == [[16, 87]] * 17 + [[16, 8], [1, 8]]


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_152_and_360_rows_at_6000_steps(mode, flag, noise):
    """K = 19 and 45 launches of 375 steps, taken by the shipped rates for every head. (At 360 rows
    it is 45 launches against 3: priced with the unsliced wide_gen* keys, BITS and MOL would miss
    the 2 % rule by 0.001 % and 0.7 %; their own measured keys admit them.)"""
    fl = flag | GEN_FRAMES | SLICES
    for rows, K in ((152, 19), (360, 45)):
        k, rs, _ = slice_plan(rows, 6000)
        assert k == K and rs.tolist() == [[16, 375]] * K
        assert plan(rows, mode=mode, flags=fl) == (wide16(K), 0)
        assert plan(rows, mode=mode, flags=fl, table='slice 1 0.98') == (wide16(K), 0)
    unsliced = {RAW: 'wide_gen_slice 3.508 0.0082', MOL: 'wide_gen_slice_mol 3.025 0.0094'}
    if mode in unsliced:
        assert plan(360, mode=mode, flags=fl, table=unsliced[mode]) == (DEFAULT_360, 0)


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_the_sliced_keys_price_their_head_and_sliced_plans_only(mode, flag, noise):
    keys = {RAW: 'wide_gen_slice', MOL: 'wide_gen_slice_mol', BETA: 'wide_gen_slice_beta'}
    fl = flag | GEN_FRAMES | SLICES
    for rows, seq in ((136, 1200), (152, 6000), (360, 6000)):
        base = plan(rows, S=seq, mode=mode, flags=flag | GEN_FRAMES)
        sliced = plan(rows, S=seq, mode=mode, flags=fl)
        assert sliced != base and all(nr == 16 for nr, _ in sliced[0][:16])
        for m, key in keys.items():
            for v in ('0.01 0.001', '100 1'):
                # without the flag no such key matters; with it only the head's own
                assert plan(rows, S=seq, mode=mode, flags=flag | GEN_FRAMES, table=f'{key} {v}') == base
                want = sliced if m != mode or v == '0.01 0.001' else base
                assert plan(rows, S=seq, mode=mode, flags=fl, table=f'{key} {v}') == want, (key, v)
    for t in ('wide_gen_slice 5', 'wide_gen_slice_mol 5 0.1 3', 'wide_gen_slice_beta 5 x', 'wide_gen_slice 5 -1'):
        with pytest.raises(ValueError):
            plan(360, table=t)


@pytest.mark.parametrize('rows, seq', [(136, 1200), (136, 1400), (144, 1200), (152, 6000), (360, 6000), (264, 6000)])
def test_virtual_row_map_invariants(rows, seq):
    """Every physical row at most once per launch and in its own group; its offset is the steps it
    has run; every row ends at S. The launches are those wrnn_debug_plan reports."""
    K, rs, vm = slice_plan(rows, seq)
    assert K > 0
    done = np.zeros(rows, dtype=np.int64)
    for k in range(K):
        nr, steps = rs[k]
        assert 1 <= nr <= 16 and steps >= 1
        seen = set()
        for r in range(16):
            for g in range(8):
                row, off = vm[k, r, g]
                if r >= nr:
                    assert row == -1
                    continue
                assert 0 <= row < rows and row % 8 == g and row not in seen
                assert off == done[row]
                seen.add(int(row))
        for row in seen:
            done[row] += steps
    assert (done == seq).all()
    p, rot = plan(rows, S=seq, flags=WIDE | GEN_FRAMES | SLICES, table='slice 1 0.98')
    assert rot == 0 and p == [(int(nr), True) for nr, _ in rs]


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_rows_are_padded_to_the_groups(mode, flag, noise):
    """131 rows plan as 136 (five padding rows, as the plain launches run them): Bplan 136 in the
    MOL draw stream."""
    fl = flag | GEN_FRAMES | SLICES
    for rows in (129, 131, 135):
        assert plan(rows, S=1200, mode=mode, flags=fl) == (wide16(17), 0)
        assert streams(rows, seq=1200, mode=mode, flags=fl) == (0, 1200 * 136 * 12 * 4 if mode == MOL else 0, 1)
    assert plan(137, S=1200, mode=mode, flags=fl) == plan(144, S=1200, mode=mode, flags=fl) == (wide16(9), 0)


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_a_sliced_call_writes_step_0_of_p1_and_no_bits_noise(mode, flag, noise):
    fl = flag | GEN_FRAMES
    assert streams(136, seq=1200, mode=mode, flags=fl | SLICES) == (0, 1200 * 136 * 12 * 4 if mode == MOL else 0, 1)
    # the same call without the flag: the mixed plan's streams, as ever
    assert plan(136, S=1200, mode=mode, flags=fl)[0] == [(1, False), (16, True)]
    assert streams(136, seq=1200, mode=mode, flags=fl) == (1200 * 136 * P1_ROW_STEP, 1200 * 136 * noise, 1)
    # any size passes the workspace check sliced (2,120 rows: R_g = 265, gcd(265, 249) = 1 -> too many
    # launches, so 2,116 -> 2,120 stays unsliced; 2,104 rows = 263 per group likewise); a size that
    # slices: 200 rows x 100,000 steps
    assert streams(200, seq=100000, mode=mode, flags=fl | SLICES)[2] == 1
    assert plan(200, S=100000, mode=mode, flags=fl | SLICES) == (wide16(25), 0)


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_no_slices_without_their_conditions(mode, flag, noise):
    fl = flag | GEN_FRAMES | SLICES
    for rows, seq in ((136, 1200), (152, 6000), (360, 6000)):
        base = plan(rows, S=seq, mode=mode, flags=flag)
        assert len(base[0]) <= 3
        # flag 128 missing: the call would write streams
        assert plan(rows, S=seq, mode=mode, flags=flag | SLICES, table=CHEAP) == base
        # the head's image missing: no wide launch at all
        p, _ = plan(rows, S=seq, mode=mode, flags=GEN_FRAMES | SLICES, table=CHEAP)
        assert p and not any(w for _, w in p)
        # a prohibitive price
        assert plan(rows, S=seq, mode=mode, flags=fl, table=DEAR) == base
        assert plan(rows, S=seq, mode=mode, flags=fl, table='slice 60 0.01') == base
    # at most 32 rows: register-resident plans, whatever the rates
    for rows in (8, 17, 24, 32):
        assert plan(rows, S=1200, mode=mode, flags=fl, table=CHEAP) == plan(rows, S=1200, mode=mode, flags=flag)
    # R_g a multiple of 16 (or at most 16): full launches already
    for rows in (40, 128, 256, 384):
        assert plan(rows, mode=mode, flags=fl, table=CHEAP) == plan(rows, mode=mode, flags=flag)
    # fewer than 64 steps per launch: not sliced
    assert plan(136, S=1000, mode=mode, flags=fl, table=CHEAP) == plan(136, S=1000, mode=mode, flags=flag)


def test_other_topologies_do_not_read_the_flag():
    for model, mode, rows, seq, flags in ((FAT, RAW, 144, 12100, RING | WIDE), (FAT, MOL, 144, 12100, RING | WIDE),
                                          (RR, RAW, 232, 8000, RING | WIDE), (RR, MOL, 232, 8000, RING | WIDE | RR_MOL),
                                          (FAT, RAW, 131, 12100, RING | WIDE)):
        base = plan(rows, S=seq, model=model, bits=9, mode=mode, flags=flags)
        sb = streams(rows, seq=seq, model=model, bits=9, mode=mode, flags=flags)
        every = flags | GEN_MOL | GEN_BETA | GEN_FRAMES | SLICES
        assert plan(rows, S=seq, model=model, bits=9, mode=mode, flags=every) == base
        assert streams(rows, seq=seq, model=model, bits=9, mode=mode, flags=every) == sb


def test_cheapest_of_three_plans_with_32_rows_selected():
    """Flags 256 and 1024 together: the plan made otherwise is the cheaper of the default and the
    32-row plan, and the slices must beat slice[1] x that. Shipped rates (us per step at 6,000
    steps; wide_gen 3.508 + 0.0082 r, gen 2.61 at 1 row, wide_gen32 6.347 + 0.0066 r, wide_gen_slice
    3.46 + 0.0082 r, slice 60 us per extra launch):
      136 rows BITS: mixed 3.639 + 2.61 = 6.249 | one 17-row launch 6.459 | 17 slices 3.976 -> slices;
               a 32-row key of 3.0 + 0.01 r (3.17 per step) flips it to the 17-row launch
      360 rows BITS: default 10.893 | 13 + 32 rows 10.173 | 45 slices 10.540 -> the 32-row plan;
               a dear 32-row key leaves default against slices: 10.540 < 0.98 x 10.893 -> slices
      360 rows Beta: default 16.005 | 16 + 29 rows 13.791 | slices 15.222 -> the 32-row plan;
               a dear 32-row key: 15.222 < 0.98 x 16.005 -> slices"""
    fl = WIDE | GEN_FRAMES | GEN32 | SLICES
    assert plan(136, flags=fl) == (wide16(17), 0)
    assert plan(136, flags=fl, table='wide_gen32 3.0 0.01') == ([(17, True)], 0)
    assert plan(136, flags=fl, table='wide_gen32 3.0 0.01\nslice 1 0.98') == ([(17, True)], 0)
    assert plan(360, flags=fl) == (DEFAULT_360_GEN32[RAW], 0)
    assert plan(360, flags=fl, table='wide_gen32 100 1') == (wide16(45), 0)
    assert plan(360, flags=fl, table='wide_gen32 100 1\nwide_gen_slice 100 1') == (DEFAULT_360, 0)
    bf = GEN_BETA | GEN_FRAMES | GEN32 | SLICES
    assert plan(360, mode=BETA, flags=bf) == (DEFAULT_360_GEN32[BETA], 0)
    assert plan(360, mode=BETA, flags=bf, table='wide_gen32_beta 100 1') == (wide16(45), 0)
    assert plan(136, mode=BETA, flags=bf) == (wide16(17), 0)
    assert plan(136, mode=BETA, flags=bf, table='wide_gen32_beta 2.0 0.01') == ([(17, True)], 0)
    # a sliced plan holds 16-row launches only, and reports the ring's streams
    assert streams(136, seq=1200, flags=fl) == (0, 0, 1)


def test_setter_refuses_a_null_handle():
    from wavernn_amd import _abi
    lib = _abi.load_library()
    for v in (0, 1, 2, -1):
        assert lib.wrnn_set_gen_wide_slices(None, v) == _abi.WRNN_ERR_INVALID
        assert 'null handle' in _abi.last_error()
    assert 'wrnn_set_gen_wide_slices' in _abi.EXPORTED
