"""The 32-row ring instances of the geneing wide launch (kernels_persist_wide_gen.hip
k_persist_wide_gen32<MODE, DBG>: up to 32 rows per XCD group as two MFMA column tiles, DESIGN.md
§3.0d2), selected by ``WaveRNN.set_wide_rows(32)`` / ``WRNN_GEN_WIDE_ROWS=32``.

A row of tile 1 is an MFMA column like any other and every row keeps the 16-row ring instance's
arithmetic, so the bar is bit equality with the 16-row launches of the same call (labels; float
samples and logits compared as uint32). The 16-row instances are pinned to the reference by
test_gpu_wide_gen / test_gpu_wide_gen_mol / test_gpu_wide_gen_ring (bit-exact labels, per-fold RMS
<= 1e-4 for MOL / Beta, logits within 1e-5 x max(1, |l|)); one fixture is checked against the
oracle here as well.
"""
import numpy as np
import pytest

from conftest import golden_case
from test_gpu_wide_gen import _dev_mels, _first, _names, _oracle_labels

pytestmark = pytest.mark.gpu

BITS = ['geneing_bits10_tiny', 'geneing_bits9_defaults']  # 1024 and 512 classes
CONT = ['geneing_mol_tiny', 'geneing_raw_beta_tiny']
FILLS = (17, 23, 32)  # tile 1: one row or none per group | partly filled | full, some groups 31 rows
_MELS = {}  # utterance count -> the device mels, built once per session


def _model(name):
    from test_gpu_parity import make_model
    meta, gold = golden_case(name)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    return meta, m, hp, sd


def _mels(n):
    if n not in _MELS:
        _MELS[n] = _dev_mels(6, [700 + u for u in range(n)])
    return _MELS[n]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _both(m, meta, dev, batched=False, target=0, overlap=0):
    """The same call with 32 rows selected and with 16: {rows: (outputs, plan, stream_info)}."""
    out = {}
    for rows in (32, 16):
        m.set_wide_rows(rows)
        m.set_seed(meta['noise_seed'])
        res, roff, S = m.generate_batch_device(dev, batched, target, overlap)
        assert _names(m) == ['persist_wide'], (rows, _names(m))
        out[rows] = (res.cpu().numpy(), m.plan_info(), m.stream_info())
    m.set_wide_rows(16)
    return out


@pytest.mark.parametrize('R', FILLS)
@pytest.mark.parametrize('name', BITS + CONT)
def test_32_row_launch_equals_16_row_launches_bit_for_bit(name, R, monkeypatch):
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    monkeypatch.delenv('WRNN_GEN_WIDE_ROWS', raising=False)
    monkeypatch.delenv('WRNN_GEN_RING', raising=False)
    meta, m, hp, sd = _model(name)
    n = 8 * R - R % 3
    out = _both(m, meta, _mels(n))
    assert out[32][1] == [(0, R, True)], out[32][1]
    assert out[32][2][0] == 0
    if name in BITS:
        assert out[32][2] == (0, 0)
    else:  # MOL keeps its [S][Bp][12] draws (Bp: the 32-row launch's padding), Beta has no stream
        assert out[32][2][1] == (1200 * 8 * R * 12 * 4 if name == 'geneing_mol_tiny' else 0)
    assert out[16][1] and all(w and nr <= 16 for _, nr, w in out[16][1]), out[16][1]
    a, b = out[32][0], out[16][0]
    assert a.shape == b.shape == (n, 1200) and a.dtype == b.dtype
    assert a.dtype == (np.float32 if name in CONT else a.dtype) and np.isfinite(a.astype(np.float64)).all()
    d = np.argwhere(_bits(a) != _bits(b))
    assert len(d) == 0, f'{name} R={R}: {len(d)} values differ, first (row, step) {_first(d)}'
    if name == 'geneing_bits10_tiny' and R in (17, 32):
        # utterance 128 is row 16 of group 0: the first row of tile 1
        for u in (0, 128, n - 1):
            ref = _oracle_labels(name, sd, hp, meta, 6, 700 + u, u)
            d = np.argwhere(a[u:u + 1] != ref)
            assert len(d) == 0, f'R={R} utt {u}: first divergence from the oracle {_first(d)}'


def test_dbg_instance_logits_of_both_tiles(monkeypatch):
    """R = 17: the DBG instance's logits of every row, the tile-1 rows included, at both sides of
    the first frame boundary and at the last steps: bit-equal to the 16-row launches', finite."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    monkeypatch.delenv('WRNN_GEN_WIDE_ROWS', raising=False)
    meta, m, hp, sd = _model('geneing_bits10_tiny')
    steps = [0, 1, 199, 200, 201, 1197, 1198, 1199]
    m.set_debug_steps(steps)
    n = 8 * 17 - 17 % 3
    got = {}
    for rows in (32, 16):
        m.set_wide_rows(rows)
        m.set_seed(meta['noise_seed'])
        m.generate_batch_device(_mels(n), False, 0, 0)
        plan = m.plan_info()
        assert (plan == [(0, 17, True)]) if rows == 32 else all(nr <= 16 for _, nr, _ in plan), plan
        got[rows] = np.stack([m.debug_logits(s, range(n)) for s in steps])
        assert got[rows].shape == (8, n, 1024) and np.isfinite(got[rows]).all()
    d = np.argwhere(got[32].view(np.uint32) != got[16].view(np.uint32))
    assert len(d) == 0, f'{len(d)} logits differ, first (step index, row, class) {d[0].tolist()}'


def test_two_32_row_launches_on_one_exchange_area(monkeypatch):
    """320 one-row utterances (40 rows per group), wide forced: more than one launch, at least one
    above 16 rows per group; every launch primes both tile copies anew."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    monkeypatch.delenv('WRNN_GEN_WIDE_ROWS', raising=False)
    meta, m, hp, sd = _model('geneing_bits10_tiny')
    out = _both(m, meta, _mels(320))
    plan = out[32][1]
    assert len(plan) >= 2 and all(w for _, _, w in plan) and max(nr for _, nr, _ in plan) > 16, plan
    assert sum(nr for _, nr, _ in plan) == 40 and out[32][2] == (0, 0), (plan, out[32][2])
    assert all(nr <= 16 for _, nr, _ in out[16][1]), out[16][1]
    d = np.argwhere(out[32][0] != out[16][0])
    assert len(d) == 0, f'first divergence {_first(d)}'


def test_fork_default_shape(monkeypatch):
    """8 x 1000-frame mels at 3000 / 1500: 360 rows x 6,000 steps under the default plan with 32
    rows selected: all wide, some launch above 16 rows per group, no stream written, labels equal
    to the shipped default plan's."""
    from test_plan_wide_gen import DEFAULT_360
    for k in ('WRNN_PERSIST_WIDE', 'WRNN_GEN_WIDE_ROWS', 'WRNN_GEN_RING'):
        monkeypatch.delenv(k, raising=False)
    meta, m, hp, sd = _model('geneing_bits10_tiny')
    out = _both(m, meta, _dev_mels(1000, range(8)), True, 3000, 1500)
    plan = out[32][1]
    assert all(w for _, _, w in plan) and max(nr for _, nr, _ in plan) > 16, plan
    assert out[32][2] == (0, 0)
    assert [(nr, w) for _, nr, w in out[16][1]] == DEFAULT_360, out[16][1]
    lab = out[32][0]
    assert lab.shape == (360, 6000) and lab.min() >= 0 and lab.max() < 1024
    d = np.argwhere(lab != out[16][0])
    assert len(d) == 0, f'{len(d)} labels differ, first divergence {_first(d)}'


def test_setter_and_switches(monkeypatch):
    from test_gpu_parity import make_model
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    monkeypatch.delenv('WRNN_GEN_WIDE_ROWS', raising=False)
    fmeta, _ = golden_case('fatchord_raw9_tiny')
    fm, _, _ = make_model(fmeta)
    with pytest.raises(ValueError):
        fm.set_wide_rows(32)
    fm.set_wide_rows(16)
    meta, m, hp, sd = _model('geneing_bits10_tiny')
    for bad in (24, 0, 33, 64):
        with pytest.raises(ValueError):
            m.set_wide_rows(bad)
    n = 8 * 17 - 17 % 3
    # the env switch overrides the handle's setting, either way
    m.set_seed(meta['noise_seed'])
    monkeypatch.setenv('WRNN_GEN_WIDE_ROWS', '32')
    m.generate_batch_device(_mels(n), False, 0, 0)
    assert m.plan_info() == [(0, 17, True)], m.plan_info()
    m.set_wide_rows(32)
    monkeypatch.setenv('WRNN_GEN_WIDE_ROWS', '16')
    m.generate_batch_device(_mels(n), False, 0, 0)
    assert all(nr <= 16 for _, nr, _ in m.plan_info()), m.plan_info()
    # a 32-row launch exists only as a ring instance
    monkeypatch.setenv('WRNN_GEN_WIDE_ROWS', '32')
    monkeypatch.setenv('WRNN_GEN_RING', '0')
    m.generate_batch_device(_mels(n), False, 0, 0)
    assert all(nr <= 16 for _, nr, _ in m.plan_info()) and m.stream_info()[0] > 0, (m.plan_info(), m.stream_info())


def test_abort_from_the_progress_callback(monkeypatch):
    """A callback that raises during a 32-row launch stops it (WRNN_ERR_ABORTED inside, the
    exception outside); the next call on the handle succeeds with the same labels as a 16-row call."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    monkeypatch.delenv('WRNN_GEN_WIDE_ROWS', raising=False)
    meta, m, hp, sd = _model('geneing_bits10_tiny')
    n = 8 * 17 - 17 % 3
    m.set_wide_rows(32)
    calls = []

    class Stop(Exception):
        pass

    def cb(i, *a):
        calls.append(i)
        if i >= 200:
            raise Stop()
    with pytest.raises(Stop):
        m.generate_batch_device(_mels(n), False, 0, 0, progress_callback=cb)
    assert calls == [0, 100, 200]
    out = _both(m, meta, _mels(n))
    assert out[32][1] == [(0, 17, True)]
    assert np.array_equal(out[32][0], out[16][0])
