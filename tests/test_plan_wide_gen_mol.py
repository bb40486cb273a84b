"""Planner and layout of the continuous heads of the geneing wide MFMA launch
(kernels_persist_wide_gen.hip k_persist_wide_gen<MODE = 1 MOL | 2 BETA, DBG>, DESIGN.md §3.0d2 /
§3.0h): host only, through wrnn_debug_plan's flags 32 (MOL image) and 64 (Beta image), rate tables
with the `wide_gen_mol` / `wide_gen_beta` keys, and the library's check of the logit-pair layout.

geneing MOL / Beta ('RAW') calls of more than 32 rows (no single register-resident launch holds
them) may take wide launches, priced at a + b r us per step by the head's own key; calls of at
most 32 rows keep their plans whatever the rates. Flag 4 and the key `wide_gen` keep meaning BITS
only. The fork's geneing defaults (target 3000 / overlap 1500, hop 200) make 45 fold rows of 6,000
steps from a 1000-frame mel, 360 rows from 8 of them.
"""
import ctypes

import pytest

FAT, RR, GEN = 0, 1, 2
RAW, MOL, BETA = 0, 1, 2
RING, WIDE, RR_MOL, GEN_MOL, GEN_BETA = 2, 4, 16, 32, 64

# (mode, the head's image flag, its rate key, its logits, the other head's flag and key)
HEADS = [pytest.param(MOL, GEN_MOL, 'wide_gen_mol', 30, GEN_BETA, 'wide_gen_beta', id='mol'),
         pytest.param(BETA, GEN_BETA, 'wide_gen_beta', 2, GEN_MOL, 'wide_gen_mol', id='beta')]

# the shipped default plans of 8 x 45 and of 45 rows x 6,000 steps (profiles/wide_gen_mol/summary.md)
DEFAULT_360 = {MOL: [(13, True), (16, True), (16, True)], BETA: [(13, True), (16, True), (16, True)]}
DEFAULT_45 = {MOL: [(6, True)], BETA: [(6, True)]}


def plan(rows, S=6000, table=None, model=GEN, bits=10, mode=MOL, flags=GEN_MOL):
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


@pytest.mark.parametrize('mode, flag, key, n, oflag, okey', HEADS)
def test_batch_of_360_rows_follows_the_heads_rate(mode, flag, key, n, oflag, okey):
    p, rot = plan(360, mode=mode, flags=flag, table=f'{key} 1.0 0.01')
    assert len(p) == 3 and all(w for _, w in p) and rot == 0, p
    assert sum(r for r, _ in p) >= 45, p
    p, _ = plan(360, mode=mode, flags=flag, table=f'{key} 100 1')
    assert p and not any(w for _, w in p), p


@pytest.mark.parametrize('mode, flag, key, n, oflag, okey', HEADS)
def test_flag_4_and_the_other_heads_flag_give_no_wide_launch(mode, flag, key, n, oflag, okey):
    for flags in (WIDE, WIDE | oflag):
        for table in (None, f'{key} 1.0 0.01', f'{key} 100 1', 'wide_gen 0.1 0.001'):
            p, _ = plan(360, mode=mode, flags=flags, table=table)
            assert p and not any(w for _, w in p), (flags, table, p)


@pytest.mark.parametrize('mode, flag, key, n, oflag, okey', HEADS)
@pytest.mark.parametrize('rows', [1, 8, 18, 24, 32])
def test_calls_of_at_most_32_rows_keep_their_plans(rows, mode, flag, key, n, oflag, okey):
    """The 32-row rule: a call one register-resident launch holds never plans a wide launch,
    however cheap the rate -- the same launches and the same rotation as without the image."""
    for S in (6000, 14000):
        got = plan(rows, S=S, mode=mode, flags=flag, table=f'{key} 0.1 0.001')
        assert got == plan(rows, S=S, mode=mode, flags=0), (rows, S)
        assert not any(w for _, w in got[0])


@pytest.mark.parametrize('mode, flag, key, n, oflag, okey', HEADS)
def test_the_key_prices_its_own_head_only(mode, flag, key, n, oflag, okey):
    cheap, dear = ' 0.1 0.001', ' 100 1'
    others = ((GEN, RAW, 360, 6000, 10, WIDE), (FAT, MOL, 144, 12100, 9, RING | WIDE),
              (RR, MOL, 232, 8000, 9, RING | WIDE | RR_MOL))
    for model, omode, rows, S, bits, flags in others:
        flags |= GEN_MOL | GEN_BETA
        base = plan(rows, S=S, model=model, mode=omode, bits=bits, flags=flags)
        assert any(w for _, w in base[0]), (model, base)  # (a plan the wide rates do decide)
        for k in ('wide_gen_mol', 'wide_gen_beta'):
            for v in (cheap, dear):
                assert plan(rows, S=S, model=model, mode=omode, bits=bits, flags=flags, table=k + v) == base, (model, k, v)
    for rows in (45, 360):
        base = plan(rows, mode=mode, flags=flag | oflag | WIDE | RR_MOL)
        for k in ('wide_gen', 'wide_mol', 'wide_rr', 'wide_rr_mol', okey):
            for v in (cheap, dear):
                assert plan(rows, mode=mode, flags=flag | oflag | WIDE | RR_MOL, table=k + v) == base, (rows, k, v)
    # (and its own key does move it)
    assert plan(360, mode=mode, flags=flag, table=key + cheap) != plan(360, mode=mode, flags=flag, table=key + dear)


@pytest.mark.parametrize('mode, flag, key, n, oflag, okey', HEADS)
@pytest.mark.parametrize('tail', ['5', '5 0.1 3', '5 x', '5 -1'])
def test_malformed_lines_are_refused(tail, mode, flag, key, n, oflag, okey):
    with pytest.raises(ValueError):
        plan(360, mode=mode, flags=flag, table=f'{key} {tail}')


@pytest.mark.parametrize('mode, flag, key, n, oflag, okey', HEADS)
def test_logit_pair_layout_has_no_violation(mode, flag, key, n, oflag, okey):
    """Every (row, logit) pair 8-byte aligned inside the candidate area, written by exactly one fc3
    epilogue lane of one slot and read in every slot by exactly one hop-3 lane that expects it,
    disjoint from the vector slots, for every group fill; the vector layout's check is unchanged."""
    from wavernn_amd import _abi
    lib = _abi.load_library()
    assert [lib.wrnn_debug_wide_gen_mol_layout(r, n) for r in range(1, 17)] == [0] * 16
    assert lib.wrnn_debug_wide_gen_mol_layout(0, n) == _abi.WRNN_ERR_INVALID
    assert lib.wrnn_debug_wide_gen_mol_layout(17, n) == _abi.WRNN_ERR_INVALID
    assert lib.wrnn_debug_wide_gen_mol_layout(8, 7) == _abi.WRNN_ERR_INVALID
    assert [lib.wrnn_debug_wide_gen_layout(r) for r in range(1, 17)] == [0] * 16


@pytest.mark.parametrize('mode, flag, key, n, oflag, okey', HEADS)
def test_default_plan_of_the_fork_default_batch(mode, flag, key, n, oflag, okey):
    """(the plans profiles/wide_gen_mol/summary.md reports for the shipped rates; the built-in
    defaults equal the shipped rates_mi355x.txt lines)"""
    assert plan(360, mode=mode, flags=flag) == (DEFAULT_360[mode], 0)
    assert plan(45, mode=mode, flags=flag) == (DEFAULT_45[mode], 0)
    import os
    from wavernn_amd import _abi
    shipped = open(os.path.join(os.path.dirname(_abi.__file__), 'rates_mi355x.txt')).read()
    assert plan(360, mode=mode, flags=flag, table=shipped) == (DEFAULT_360[mode], 0)
    assert plan(45, mode=mode, flags=flag, table=shipped) == (DEFAULT_45[mode], 0)
