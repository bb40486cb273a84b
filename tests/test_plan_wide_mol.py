"""Planner and layout of the MOL head on the wide MFMA kernel (kernels_persist_wide.hip
k_persist_wide<.., MOL, ..>): host only, through wrnn_debug_plan, a rate
table with the `wide_mol` key, and the library's check of the logit-pair layout.

MOL batches past 32 rows take wide launches as RAW batches do (C4's 144 rows: time-sliced wide
launches); calls of at most 32 rows keep their register-resident plans under the shipped rates.
"""
import ctypes

import pytest

FAT, RR, GEN = 0, 1, 2
RAW, MOL = 0, 1
RING, WIDE = 2, 4


def plan(rows, S=12100, table=None, model=FAT, bits=9, mode=MOL, flags=RING | WIDE):
    from wavernn_amd import _abi
    lib = _abi.load_library()
    n, rot = ctypes.c_int(), ctypes.c_int()
    cap = 128
    nr, wd = (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    rc = lib.wrnn_debug_plan(table.encode() if table else None, model, bits, mode, rows, S, flags,
                             ctypes.byref(n), nr, wd, cap, ctypes.byref(rot))
    if rc:
        raise ValueError(_abi.last_error())
    return [(nr[i], bool(wd[i])) for i in range(n.value)], rot.value


def test_mol_c4_rows_are_all_wide_launches():
    """144 rows (C4 per GPU) x 12,100 steps: only wide launches -- the time-sliced plan RAW gets
    (10 launches of 16 rows per group and the remainder's)."""
    p, rot = plan(144)
    assert p and all(w for _, w in p) and rot == 0, p
    assert p == plan(144, mode=RAW)[0]


def test_mol_c2_rows_stay_rotated_register_resident():
    p, rot = plan(18)
    assert p == [(3, False)] * 3 and rot == 3


@pytest.mark.parametrize('rows', [1, 8, 18, 24, 32])
def test_mol_small_calls_stay_register_resident(rows):
    """(what keeps fold-range pieces and shards of small MOL calls bit-equal to the whole call)"""
    p, _ = plan(rows)
    assert p and not any(w for _, w in p), p


def test_mol_without_wide_images_has_no_wide_launch():
    p, _ = plan(144, flags=RING)
    assert p and not any(w for _, w in p), p


def test_mol_runtimeracer_has_no_wide_launch():
    """(k_persist_wide_rr is RAW only)"""
    p, _ = plan(232, S=8000, model=RR)
    assert p and not any(w for _, w in p), p


def test_wide_mol_rate_key_moves_the_plan():
    assert plan(144, table='wide_mol 9.32 0.025')[0] == plan(144)[0]
    p, _ = plan(144, table='wide_mol 100 1')
    assert p and not any(w for _, w in p), p
    # and a cheap one takes even a small call
    assert plan(18, table='wide_mol 1.0 0.01')[0] == [(3, True)]
    # the RAW key does not price MOL launches, nor the MOL key RAW ones
    assert plan(144, table='wide 100 1 1')[0] == plan(144)[0]
    assert plan(144, mode=RAW, table='wide_mol 100 1')[0] == plan(144, mode=RAW)[0]


@pytest.mark.parametrize('table', ['wide_mol 9.32', 'wide_mol 9.32 0.025 1.24', 'wide_mol 9.32 x',
                                   'wide_mol 9.32 -1'])
def test_malformed_wide_mol_lines_are_refused(table):
    with pytest.raises(ValueError):
        plan(144, table=table)


@pytest.mark.parametrize('kw', [dict(bits=40), dict(bits=0), dict(bits=-1), dict(mode=7), dict(mode=-1),
                                dict(rows=10 ** 9)])
def test_absurd_plan_arguments_are_refused(kw):
    args = dict(rows=18)
    args.update(kw)
    with pytest.raises(ValueError):
        plan(**args)


def test_mol_logit_pair_layout_has_no_violation():
    """wide_layout.h logit_off: every (row, logit) pair aligned, inside the candidate area, written
    by exactly one fc3 epilogue lane and read by exactly one hop-D lane, for every group fill."""
    from wavernn_amd import _abi
    lib = _abi.load_library()
    assert [lib.wrnn_debug_wide_mol_layout(r) for r in range(1, 17)] == [0] * 16
    assert lib.wrnn_debug_wide_mol_layout(0) == _abi.WRNN_ERR_INVALID
    assert lib.wrnn_debug_wide_mol_layout(17) == _abi.WRNN_ERR_INVALID
    # today's layouts: unchanged
    assert [lib.wrnn_debug_wide_layout(r) for r in range(1, 17)] == [0] * 16
