"""Planner and layout of the geneing wide MFMA launch (kernels_persist_wide_gen.hip
k_persist_wide_gen): host only, through wrnn_debug_plan, a rate table
with the `wide_gen` key, and the library's check of the exchange layout.

geneing BITS calls of more than 32 rows (no single register-resident launch holds them) may take
wide launches, priced at a + b r us per step; calls of at most 32 rows keep their plans whatever
the rates. The fork's geneing defaults (target 3000 / overlap 1500, hop 200) make 45 fold rows of
6,000 steps from a 1000-frame mel, 360 rows from 8 of them.
"""
import ctypes

import pytest

FAT, RR, GEN = 0, 1, 2
RAW, MOL, BETA = 0, 1, 2
RING, WIDE = 2, 4

# the shipped default plan of 8 x 45 rows x 6,000 steps (profiles/wide_gen/summary.md)
DEFAULT_360 = [(13, True), (16, True), (16, True)]
# ... and of one utterance's 45 rows
DEFAULT_45 = [(6, True)]


def plan(rows, S=6000, table=None, model=GEN, bits=10, mode=RAW, flags=WIDE):
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


def test_batch_of_360_rows_follows_the_wide_gen_rate():
    p, rot = plan(360, table='wide_gen 1.0 0.01')
    assert len(p) == 3 and all(w for _, w in p) and rot == 0, p
    assert sum(r for r, _ in p) >= 45, p
    p, _ = plan(360, table='wide_gen 100 1')
    assert p and not any(w for _, w in p), p


def test_default_plan_of_the_fork_default_batch():
    """(the plan profiles/wide_gen/summary.md reports for the shipped rates)"""
    assert plan(360) == (DEFAULT_360, 0)
    assert plan(45) == (DEFAULT_45, 0)


def test_single_utterance_of_45_rows_follows_the_wide_gen_rate():
    assert plan(45, table='wide_gen 1.0 0.01')[0] == [(6, True)]
    p, _ = plan(45, table='wide_gen 100 1')
    assert p and not any(w for _, w in p), p


@pytest.mark.parametrize('rows', [1, 8, 18, 24, 32])
@pytest.mark.parametrize('bits', [9, 10])
def test_calls_of_at_most_32_rows_keep_their_plans(rows, bits):
    """The 32-row rule: a call one register-resident launch holds never plans a wide launch,
    however cheap the rate (rotation included)."""
    assert plan(rows, bits=bits, table='wide_gen 0.1 0.001') == plan(rows, bits=bits, flags=0)
    assert plan(rows, S=14000, bits=bits, table='wide_gen 0.1 0.001') == plan(rows, S=14000, bits=bits, flags=0)


def test_without_wide_images_no_wide_launch():
    p, _ = plan(360, flags=0, table='wide_gen 0.1 0.001')
    assert p and not any(w for _, w in p), p


@pytest.mark.parametrize('mode', [MOL, BETA])
def test_mol_and_beta_have_no_wide_launch(mode):
    p, _ = plan(360, mode=mode, table='wide_gen 0.1 0.001')
    assert p and not any(w for _, w in p), p


def test_wide_gen_key_prices_geneing_only():
    for model, rows, S in ((FAT, 144, 12100), (RR, 232, 8000)):
        base = plan(rows, S=S, model=model, bits=9, flags=RING | WIDE)
        assert plan(rows, S=S, model=model, bits=9, flags=RING | WIDE, table='wide_gen 0.1 0.001') == base
        assert plan(rows, S=S, model=model, bits=9, flags=RING | WIDE, table='wide_gen 100 1') == base
    for rows in (45, 360):
        base = plan(rows)
        assert plan(rows, table='wide 100 1 1') == base
        assert plan(rows, table='wide 0.1 0.001 0.1') == base
        assert plan(rows, table='wide_rr 100 1') == base
        assert plan(rows, table='wide_rr 0.1 0.001') == base
        assert plan(rows, table='wide_mol 0.1 0.001') == base


@pytest.mark.parametrize('table', ['wide_gen 5', 'wide_gen 5 0.1 3', 'wide_gen 5 x', 'wide_gen 5 -1'])
def test_malformed_wide_gen_lines_are_refused(table):
    with pytest.raises(ValueError):
        plan(360, table=table)


def test_wide_gen_layout_has_no_violation():
    """Every x1 / h1 / y1 producer packet lands on exactly the consumer packet that expects its
    (row, unit quad), inside its parity slot; candidate pairs aligned inside their area; for
    every group fill."""
    from wavernn_amd import _abi
    lib = _abi.load_library()
    assert [lib.wrnn_debug_wide_gen_layout(r) for r in range(1, 17)] == [0] * 16
    assert lib.wrnn_debug_wide_gen_layout(0) == _abi.WRNN_ERR_INVALID
    assert lib.wrnn_debug_wide_gen_layout(17) == _abi.WRNN_ERR_INVALID
