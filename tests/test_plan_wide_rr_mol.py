"""Planner and layout of the mixture-of-logistics head of the runtimeracer wide MFMA launch
(kernels_persist_wide_rr.hip k_persist_wide_rr<ROT, MOL = true, DBG>):
host only, through wrnn_debug_plan's flag 16, a rate table with the `wide_rr_mol` key, and the
library's check of the logit-pair layout.

Runtimeracer MOL calls of more than 32 rows (no single register-resident launch holds them) may
take wide launches, priced at a + b r us per step; calls of at most 32 rows keep their plans
whatever the rates. The fork's generation defaults (target 6000 / overlap 1000, hop 200) make 29
fold rows of 8,000 steps from a 1000-frame mel, 232 rows from 8 of them.
"""
import ctypes

import pytest

FAT, RR, GEN = 0, 1, 2
RAW, MOL, BETA = 0, 1, 2
RING, WIDE, RR_MOL = 2, 4, 16


def plan(rows=232, S=8000, table=None, model=RR, bits=9, mode=MOL, flags=RING | WIDE | RR_MOL):
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


def test_batch_of_232_rows_follows_the_wide_rr_mol_rate():
    p, rot = plan(table='wide_rr_mol 1.0 0.01')
    assert p and all(w for _, w in p) and rot == 0, p
    p, _ = plan(table='wide_rr_mol 100 1')
    assert p and not any(w for _, w in p), p


def test_default_plan_of_the_fork_default_batch():
    """(the plans profiles/wide_rr_mol/summary.md reports for the shipped rates: 29 time-sliced
    launches of 16 rows per group for 8 utterances, one utterance register-resident as before)"""
    assert plan() == ([(16, True)] * 29, 0)
    assert plan(29) == plan(29, flags=RING)
    assert not any(w for _, w in plan(29)[0])


@pytest.mark.parametrize('table', [None, 'wide_rr_mol 1.0 0.01', 'wide_rr_mol 100 1', 'wide_rr 0.1 0.001'])
def test_flag_4_alone_does_not_cover_runtimeracer_mol(table):
    p, _ = plan(flags=RING | WIDE, table=table)
    assert p and not any(w for _, w in p), p


@pytest.mark.parametrize('rows', [1, 8, 18, 24, 29, 32])
@pytest.mark.parametrize('S', [8000, 12100])
def test_calls_of_at_most_32_rows_keep_their_plans(rows, S):
    """The 32-row rule: a call one register-resident launch holds never plans a wide launch,
    however cheap the rate -- the same launches and the same rotation as without the image."""
    assert plan(rows, S=S, table='wide_rr_mol 0.1 0.001') == plan(rows, S=S, flags=RING)


def test_wide_rr_mol_key_prices_runtimeracer_mol_only():
    cheap, dear = 'wide_rr_mol 0.1 0.001', 'wide_rr_mol 100 1'
    others = ((RR, RAW, 232, 8000), (FAT, MOL, 144, 12100), (GEN, RAW, 360, 6000))
    for model, mode, rows, S in others:
        base = plan(rows, S=S, model=model, mode=mode, bits=10 if model == GEN else 9)
        assert any(w for _, w in base[0]), (model, base)  # (a plan the wide rates do decide)
        for table in (cheap, dear):
            assert plan(rows, S=S, model=model, mode=mode, bits=10 if model == GEN else 9, table=table) == base
    base = plan()
    for key in ('wide_rr', 'wide_mol', 'wide_gen'):
        assert plan(table=f'{key} 0.1 0.001') == base, key
        assert plan(table=f'{key} 100 1') == base, key


@pytest.mark.parametrize('table', ['wide_rr_mol 5', 'wide_rr_mol 5 0.1 3', 'wide_rr_mol 5 x', 'wide_rr_mol 5 -1'])
def test_malformed_wide_rr_mol_lines_are_refused(table):
    with pytest.raises(ValueError):
        plan(table=table)


def test_wide_rr_mol_layout_has_no_violation():
    """Every (row, logit) pair 8-byte aligned inside the logit area, written by exactly one fc5
    epilogue lane and read in every B slot by exactly one hop-B7 lane that expects it, disjoint
    from the vector slots, for every group fill; the vector layout's check is unchanged."""
    from wavernn_amd import _abi
    lib = _abi.load_library()
    assert [lib.wrnn_debug_wide_rr_mol_layout(r) for r in range(1, 17)] == [0] * 16
    assert lib.wrnn_debug_wide_rr_mol_layout(0) == _abi.WRNN_ERR_INVALID
    assert lib.wrnn_debug_wide_rr_mol_layout(17) == _abi.WRNN_ERR_INVALID
    assert [lib.wrnn_debug_wide_layout(r) for r in range(1, 17)] == [0] * 16
