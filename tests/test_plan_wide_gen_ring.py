"""Which per-step streams a planned call writes, and whether the workspace check admits the
persistent engine (wrnn_debug_stream_bytes): host only.

A geneing call whose launches are all wide forms P1 and (BITS) the Gumbel noise in-kernel
(k_persist_wide_gen<MODE, RING = true, DBG>) when the per-frame P1 form is available -- flag 128 of
wrnn_debug_stream_bytes. Such a call writes no P1 stream and, for BITS, no noise stream (MOL keeps
its [S][Bp][12] draws, Beta never had one), so it stays on the persistent engine at any size. A
plan with a register-resident launch keeps its streams; fatchord and runtimeracer answers do not
depend on the flag; no launch plan changes.

The fork's geneing defaults (target 3000 / overlap 1500, hop 200) make 45 fold rows of 6,000 steps
from a 1000-frame mel: 360 rows from 8 of them, 2,880 from 64.
"""
import ctypes

import pytest

from test_plan_wide_gen import plan

FAT, RR, GEN = 0, 1, 2
RAW, MOL, BETA = 0, 1, 2
RING, WIDE, RR_MOL, GEN_MOL, GEN_BETA, GEN_FRAMES = 2, 4, 16, 32, 64, 128
S = 6000
P1_ROW_STEP = 4 * 256 * 4  # bytes of P1 (r, z, n, cI of 256 units) per row and step
# (mode, the head's wide image flag, noise bytes per row and step of its stream form)
HEADS = [pytest.param(RAW, WIDE, 1024 * 4, id='bits'), pytest.param(MOL, GEN_MOL, 12 * 4, id='mol'),
         pytest.param(BETA, GEN_BETA, 0, id='beta')]


def streams(rows, seq=S, model=GEN, bits=10, mode=RAW, flags=WIDE):
    from wavernn_amd import _abi
    lib = _abi.load_library()
    p1, nz, ok = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(-1)
    rc = lib.wrnn_debug_stream_bytes(model, bits, mode, rows, seq, flags, ctypes.byref(p1), ctypes.byref(nz),
                                     ctypes.byref(ok))
    if rc:
        raise ValueError(_abi.last_error())
    return p1.value, nz.value, ok.value


def padded_rows(rows, seq=S, **kw):
    """Rows the planned launches run (8 x rows per group, summed), and whether all are wide."""
    p, rot = plan(rows, S=seq, **kw)
    assert p and rot == 0, (p, rot)
    return 8 * sum(nr for nr, _ in p), all(w for _, w in p)


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_fork_default_batch_writes_no_p1_stream(mode, flag, noise):
    Bp, all_wide = padded_rows(360, mode=mode, flags=flag)
    assert Bp == 360 and all_wide
    p1, nz, ok = streams(360, mode=mode, flags=flag | GEN_FRAMES)
    assert p1 == 0 and ok == 1
    # BITS draws in-kernel, MOL keeps its [S][Bp][12] draws, Beta has no stream
    assert nz == (S * Bp * 12 * 4 if mode == MOL else 0)


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_without_the_per_frame_form_the_streams_stay(mode, flag, noise):
    Bp, _ = padded_rows(360, mode=mode, flags=flag)
    assert streams(360, mode=mode, flags=flag) == (S * Bp * P1_ROW_STEP, S * Bp * noise, 1)


def test_large_batch_stays_on_the_persistent_engine():
    """2,880 rows x 6,000 steps of 10-bit BITS: 2 x 70.8 GB of streams exceed the workspace cap, so
    the stream form is refused (engine='auto' runs CHAIN); the ring form writes none."""
    Bp, all_wide = padded_rows(2880)
    assert Bp == 2880 and all_wide
    p1, nz, ok = streams(2880, flags=WIDE)
    assert ok == 0 and p1 + nz == S * Bp * (P1_ROW_STEP + 1024 * 4) > 96 * 2 ** 30
    assert streams(2880, flags=WIDE | GEN_FRAMES) == (0, 0, 1)


def test_the_cap_counts_what_the_call_writes():
    """The first 1000-frame utterance count whose streams pass the cap without the per-frame form;
    with it every count up to 64 whose launches are all wide is admitted and writes nothing, and a
    count whose plan holds a register-resident launch is judged by the streams it keeps."""
    first = next(u for u in range(1, 65) if not streams(45 * u, flags=WIDE)[2])
    # (the cliff exactly: the padded rows of the plan, 8,192 stream bytes per row and step)
    over, under = padded_rows(45 * first)[0], padded_rows(45 * (first - 1))[0]
    assert over * S * (P1_ROW_STEP + 4096) > 96 * 2 ** 30 >= under * S * (P1_ROW_STEP + 4096)
    n_wide = 0
    for u in range(1, 65):
        _, all_wide = padded_rows(45 * u)
        got = streams(45 * u, flags=WIDE | GEN_FRAMES)
        assert got == ((0, 0, 1) if all_wide else streams(45 * u, flags=WIDE)), u
        n_wide += all_wide
    assert n_wide >= 50


@pytest.mark.parametrize('mode, flag, noise', HEADS)
def test_mixed_plan_keeps_its_streams(mode, flag, noise):
    """131 rows x 1,200 steps: a register-resident launch of 1 row per group and a wide one of 16
    (as test_gpu_wide_gen pins it for BITS): the register-resident kernel reads the streams."""
    p, _ = plan(131, S=1200, mode=mode, flags=flag)
    assert sorted(p) == [(1, False), (16, True)], p
    want = (1200 * 136 * P1_ROW_STEP, 1200 * 136 * noise, 1)
    assert streams(131, seq=1200, mode=mode, flags=flag | GEN_FRAMES) == want
    assert streams(131, seq=1200, mode=mode, flags=flag) == want


def test_register_resident_calls_keep_their_streams():
    for rows in (1, 8, 32):
        assert streams(rows, flags=WIDE | GEN_FRAMES) == streams(rows, flags=WIDE)
        assert streams(rows, flags=WIDE)[0] > 0
    assert streams(360, flags=GEN_FRAMES) == streams(360, flags=0)  # (no wide image: no wide launch)


@pytest.mark.parametrize('model, mode, rows, seq, flags', [
    (FAT, RAW, 144, 12100, RING | WIDE), (FAT, RAW, 144, 12100, WIDE), (FAT, MOL, 144, 12100, RING | WIDE),
    (RR, RAW, 232, 8000, RING | WIDE), (RR, RAW, 232, 8000, WIDE), (RR, MOL, 232, 8000, RING | WIDE | RR_MOL)])
def test_other_topologies_do_not_read_the_flag(model, mode, rows, seq, flags):
    base = streams(rows, seq=seq, model=model, bits=9, mode=mode, flags=flags)
    assert streams(rows, seq=seq, model=model, bits=9, mode=mode, flags=flags | GEN_FRAMES) == base
    assert base[2] == 1


def test_other_topologies_report_their_streams():
    """fatchord C4 (144 x 12,100, P1 ring, a register-resident launch beside the wide one): no P1
    stream, the noise stream's extent; without the ring the P1 stream of 4 x 512 floats.
    runtimeracer (232 x 8,000, wide launches only): neither with the per-frame form."""
    # (144 = 8 x 18 and 232 = 8 x 29 rows: no padding rows, whatever the launches)
    p, _ = plan(144, S=12100, model=FAT, bits=9, flags=RING | WIDE)
    all_wide = all(w for _, w in p)
    p1, nz, _ = streams(144, seq=12100, model=FAT, bits=9, flags=RING | WIDE)
    assert p1 == 0 and nz == (0 if all_wide else 12100 * 144 * 512 * 4)
    p1, _, _ = streams(144, seq=12100, model=FAT, bits=9, flags=WIDE)
    assert p1 == 12100 * 144 * 4 * 512 * 4
    p, _ = plan(232, S=8000, model=RR, bits=9, flags=RING | WIDE)
    assert all(w for _, w in p)
    assert streams(232, seq=8000, model=RR, bits=9, flags=RING | WIDE)[:2] == (0, 0)
    assert streams(232, seq=8000, model=RR, bits=9, flags=WIDE)[:2] == (8000 * 232 * 4 * 256 * 4, 0)


@pytest.mark.parametrize('mode, flag, noise', HEADS)
@pytest.mark.parametrize('rows', [45, 131, 360, 2880])
def test_launch_plans_do_not_change(rows, mode, flag, noise):
    for seq in (1200, S):
        assert plan(rows, S=seq, mode=mode, flags=flag | GEN_FRAMES) == plan(rows, S=seq, mode=mode, flags=flag)


def test_bad_arguments_are_refused():
    from wavernn_amd import _abi
    for kw in (dict(rows=0), dict(seq=0), dict(bits=11), dict(mode=3), dict(model=7)):
        args = dict(rows=360)
        args.update(kw)
        with pytest.raises(ValueError):
            streams(**args)
    lib = _abi.load_library()
    assert lib.wrnn_debug_stream_bytes(GEN, 10, RAW, 360, S, WIDE, None, None, None) == _abi.WRNN_ERR_INVALID
