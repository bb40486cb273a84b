"""Planner of the block-sparse wide launches (csrc/plan.cpp): host only,
through wrnn_debug_plan with flag 512 (the sparse-wide image of a pruned fatchord RAW model
exists; it needs the wide image's flag 4) and the rate key `wide_sp` (base, per row, 1024-class
term, like `wide`).

With the image, each wide launch -- full or time-sliced, by the same slice rule -- is priced with
the cheaper of `wide` and `wide_sp` and reported as wide == 2 when that is `wide_sp`. Without flag
512 the key moves nothing, and under the shipped table (where `wide_sp` is not below `wide`) every
plan is what it was.
"""
import ctypes

import pytest

FAT, RR, GEN = 0, 1, 2
RAW, MOL, BETA = 0, 1, 2
SP, RING, WIDE, FORCE_SP, WIDE_SP = 1, 2, 4, 8, 512
CHEAP = 'wide_sp 3.0 0.2 1.0'    # 6.2 us at 16 rows per group: below the dense 9.72
DEAR = 'wide_sp 30 1 5'


def plan(rows, S=12100, table=None, model=FAT, bits=9, mode=RAW, flags=RING | WIDE):
    """([(rows per group, wide: 0 register-resident, 1 MFMA, 2 block-sparse)], rotation launches)"""
    from wavernn_amd import _abi
    lib = _abi.load_library()
    n, rot = ctypes.c_int(), ctypes.c_int()
    cap = 128
    nr, wd = (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    rc = lib.wrnn_debug_plan(table.encode() if table else None, model, bits, mode, rows, S, flags,
                             ctypes.byref(n), nr, wd, cap, ctypes.byref(rot))
    if rc:
        raise ValueError(_abi.last_error())
    return [(nr[i], wd[i]) for i in range(n.value)], rot.value


def test_c4_batch_plans_11_sliced_sparse_launches_under_a_cheap_key():
    """144 rows x 12,100 steps at 9 bits (BASELINE configs[3] per GPU): 9 launches of 16 rows per
    group and 2 for the remaining steps (§3.0f), every one block-sparse"""
    p, rot = plan(144, table=CHEAP, flags=RING | WIDE | WIDE_SP)
    assert rot == 0 and [nr for nr, _ in p] == [16] * 10 + [2], p
    assert all(w == 2 for _, w in p), p
    # the same launches run dense without the image
    assert plan(144) == ([(nr, 1) for nr, _ in p], 0)


def test_10_bit_default_batch_plans_17_sliced_sparse_launches_under_a_cheap_key():
    """136 rows (17 per group) of the 10-bit default's 14,000 steps"""
    p, rot = plan(136, S=14000, bits=10, table=CHEAP, flags=RING | WIDE | WIDE_SP)
    assert rot == 0 and len(p) == 17 and all(w == 2 for _, w in p), p
    assert len(plan(136, S=14000, bits=10)[0]) == 17


ROWS = (1, 8, 18, 24, 32, 33, 45, 72, 131, 136, 144, 152, 232, 360, 2115)


@pytest.mark.parametrize('bits', [9, 10])
@pytest.mark.parametrize('rows', ROWS)
def test_a_dear_key_gives_the_plan_without_the_image(rows, bits):
    for S in (63, 1200, 12100, 14000):
        for fl in (WIDE, RING | WIDE, SP | RING | WIDE, SP | RING | WIDE | FORCE_SP):
            base = plan(rows, S=S, bits=bits, flags=fl)
            assert all(w < 2 for _, w in base[0])
            for t in (DEAR, None):  # (shipped: wide_sp is not below wide)
                assert plan(rows, S=S, bits=bits, flags=fl | WIDE_SP, table=t) == base, (S, fl, t)


@pytest.mark.parametrize('rows', ROWS)
def test_without_the_flag_the_key_has_no_effect(rows):
    for bits in (9, 10):
        for fl in (0, RING, WIDE, RING | WIDE, SP | RING | WIDE):
            base = plan(rows, bits=bits, flags=fl)
            for t in (CHEAP, DEAR, 'wide_sp 0.01 0.001 0.01'):
                assert plan(rows, bits=bits, flags=fl, table=t) == base, (bits, fl, t)
    # flag 512 without the wide image (flag 4): no wide launch at all, so nothing to price
    base = plan(rows, flags=RING)
    assert plan(rows, flags=RING | WIDE_SP, table=CHEAP) == base
    assert not any(w for _, w in base[0])


@pytest.mark.parametrize('model, mode, bits, flags', [
    (FAT, MOL, 9, RING | WIDE), (RR, RAW, 9, RING | WIDE), (RR, RAW, 10, RING | WIDE),
    (RR, MOL, 9, RING | WIDE | 16), (GEN, RAW, 10, WIDE), (GEN, MOL, 9, WIDE | 32), (GEN, BETA, 9, WIDE | 64)])
def test_other_heads_read_neither_the_flag_nor_the_key(model, mode, bits, flags):
    for rows in (18, 45, 144, 232, 360):
        for S in (6000, 12100):
            base = plan(rows, S=S, model=model, bits=bits, mode=mode, flags=flags)
            for t in (CHEAP, DEAR, None):
                assert plan(rows, S=S, model=model, bits=bits, mode=mode, flags=flags | WIDE_SP, table=t) == base


@pytest.mark.parametrize('rows', range(1, 33))
def test_calls_of_at_most_32_rows_are_unchanged_under_the_shipped_table(rows):
    """(their register-resident rates of 4-9 us per step are below any wide rate)"""
    for bits in (9, 10):
        for S in (1200, 12100, 14000):
            for fl in (RING | WIDE, SP | RING | WIDE):
                assert plan(rows, S=S, bits=bits, flags=fl | WIDE_SP) == plan(rows, S=S, bits=bits, flags=fl)


def test_a_launch_takes_the_cheaper_of_the_two_keys_by_its_own_rows():
    """wide_sp dearer per row than wide: small fills run sparse, full ones dense (the key crosses
    wide's 9.32 + 0.025 r between 5 and 6 rows per group)"""
    t = 'wide_sp 5.0 0.8 1.0\nfat9 50 60 70 80'  # (register-resident launches priced out)
    fl = RING | WIDE | WIDE_SP
    assert plan(40, S=63, table=t, flags=fl) == ([(5, 2)], 0)
    assert plan(48, S=63, table=t, flags=fl) == ([(6, 1)], 0)
    assert plan(128, S=63, table=t, flags=fl) == ([(16, 1)], 0)


@pytest.mark.parametrize('table', ['wide_sp 5', 'wide_sp 5 0.1', 'wide_sp 5 0.1 1 2', 'wide_sp 5 x 1', 'wide_sp 5 -1 1',
                                   'wide_sp 0 0.1 1'])
def test_malformed_lines_are_refused(table):
    with pytest.raises(ValueError):
        plan(144, table=table)


def test_the_shipped_key_is_the_fit_of_the_committed_measurement(tmp_path):
    """tools/make_rates.py over profiles/wide_sp/rates.log gives the wide_sp line of the shipped
    rates_mi355x.txt, which is also the built-in default (read here through a plan on the key's
    edge: a dense key just above / below it at 16 rows per group flips the launch)."""
    import os
    import subprocess
    import sys
    from conftest import PKG, REPO
    out = tmp_path / 'rates.txt'
    subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'make_rates.py'), str(out),
                    os.path.join(REPO, 'profiles', 'wide_sp')], check=True, capture_output=True)
    fitted = [ln for ln in out.read_text().splitlines() if ln.startswith('wide_sp ')]
    shipped = [ln.strip() for ln in open(os.path.join(PKG, 'wavernn_amd', 'rates_mi355x.txt')) if ln.startswith('wide_sp ')]
    assert fitted == shipped == ['wide_sp 22.434 0.1173 1.518']
    fl = RING | WIDE | WIDE_SP
    at16 = 22.434 + 0.1173 * 16
    t = 'fat9 90 91 92 93\nwide {} 0.0001 1'
    assert plan(128, S=63, table=t.format(at16 + 0.01), flags=fl) == ([(16, 2)], 0)
    assert plan(128, S=63, table=t.format(at16 - 0.01), flags=fl) == ([(16, 1)], 0)
