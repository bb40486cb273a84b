"""The ring instances of the geneing wide MFMA launch (kernels_persist_wide_gen.hip
k_persist_wide_gen<MODE, RING = true, DBG>): waves 4-7 of every slot form the
slot's P1 (from the per-frame tables, k_p1_expand's fp32 operations) and, for BITS, its Gumbel
words (k_gumbel's Philox keys and fixed-point form) into LDS, so a call whose launches are all wide
writes no [S][Bp][256][4] P1 stream and no [S][Bp][n] noise stream. ``WRNN_GEN_RING=1|0`` forces the
ring where it is possible / the streams; ``WRNN_PERSIST_WIDE=1`` makes every launch wide.

Both forms feed the same kernel family the same fp32 values, so the bar between them is bit
equality: labels (BITS), float samples (MOL, Beta) and recorded logits. Against the reference the
bars are the existing ones: bit-exact labels and waveform (test_gpu_wide_gen), per-fold RMS <= 1e-4
(test_gpu_wide_gen_mol), logits within 1e-5 x max(1, |l|) (test_gpu_logits).
"""
import numpy as np
import pytest

from conftest import golden_case, wave_equal
from test_gpu_wide_gen import _dev_mels, _first, _names

pytestmark = pytest.mark.gpu

BITS = ['geneing_bits10_tiny', 'geneing_bits9_defaults']  # 1024 and 512 classes
CONT = ['geneing_mol_tiny', 'geneing_raw_beta_tiny']


def _model(name):
    from test_gpu_parity import make_model
    meta, gold = golden_case(name)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    return meta, gold, m, hp


def _golden_call(m, hp, meta):
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    mel = synth_mel(meta['n_frames'], meta['mel_seed']) / sp.max_abs_value
    return m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law, sp.preemphasize,
                      progress_callback=lambda *a: None)


def _forms(m, meta, dev, monkeypatch, settings=('1', '0')):
    """The same unbatched call under each WRNN_GEN_RING setting (None: unset):
    {setting: (outputs, plan, stream_info)}."""
    out = {}
    for ring in settings:
        if ring is None:
            monkeypatch.delenv('WRNN_GEN_RING', raising=False)
        else:
            monkeypatch.setenv('WRNN_GEN_RING', ring)
        m.set_seed(meta['noise_seed'])
        res, roff, S = m.generate_batch_device(dev, False, 0, 0)
        assert S == 1200 and roff[-1] == len(dev)
        out[ring] = (res.cpu().numpy(), m.plan_info(), m.stream_info())
    return out


@pytest.mark.parametrize('name', BITS)
def test_ring_goldens_bit_exact(name, monkeypatch):
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    monkeypatch.setenv('WRNN_GEN_RING', '1')
    meta, gold, m, hp = _model(name)
    wav = _golden_call(m, hp, meta)
    assert _names(m) == ['persist_wide']
    assert m.stream_info() == (0, 0)
    lab = m.last_labels
    assert lab.shape == gold['labels'].shape == (meta['num_folds'], meta['seq_len'])
    d = np.argwhere(lab != gold['labels'])
    assert len(d) == 0, f'first divergence {_first(d)}'
    assert wave_equal(wav, gold)


@pytest.mark.parametrize('name', CONT)
def test_ring_continuous_goldens_within_tolerance(name, monkeypatch):
    from test_gpu_wide_gen_mol import _check_golden
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    monkeypatch.setenv('WRNN_GEN_RING', '1')
    meta, gold, m, hp = _model(name)
    wav = _golden_call(m, hp, meta)
    _check_golden(name, m, meta, gold, wav)
    p1, noise = m.stream_info()
    assert p1 == 0
    # MOL keeps its [S][Bp][12] draws (5 rows padded to 8), Beta draws in-kernel
    assert noise == (1200 * 8 * 12 * 4 if meta['mode'] == 'MOL' else 0)


@pytest.mark.parametrize('R', [1, 5, 16])
@pytest.mark.parametrize('name', BITS + CONT)
def test_ring_equals_stream_bit_for_bit(name, R, monkeypatch):
    """8 R - R % 3 one-row utterances of 1,200 steps: padding rows in some groups (R = 1, 5, 16), a
    partial tile (5) and a full one (16). Labels / float samples of the two forms are identical."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, _, m, hp = _model(name)
    n = 8 * R - R % 3
    out = _forms(m, meta, _dev_mels(6, [700 + u for u in range(n)]), monkeypatch)
    for ring in ('1', '0'):
        assert out[ring][1] == [(0, R, True)], out[ring][1]
    assert out['1'][2][0] == 0 and out['0'][2][0] == 1200 * 8 * R * 4 * 256 * 4, (out['1'][2], out['0'][2])
    if name in BITS:
        assert out['1'][2] == (0, 0) and out['0'][2][1] == 1200 * 8 * R * (1 << meta['bits']) * 4
        assert out['1'][0].dtype.kind == 'i'
    else:
        assert out['1'][2][1] == out['0'][2][1]  # (MOL: the same draws; Beta: none)
        assert out['1'][0].dtype == np.float32
    a, b = out['1'][0], out['0'][0]
    d = np.argwhere(a.view(np.uint32 if a.dtype == np.float32 else a.dtype) !=
                    b.view(np.uint32 if b.dtype == np.float32 else b.dtype))
    assert len(d) == 0, f'{name} R={R}: {len(d)} values differ, first {_first(d)}'


def _edge_steps(S):
    return [0, 1, 199, 200, 201, S - 3, S - 2, S - 1]


def _logits(m, steps, rows):
    return np.stack([m.debug_logits(s, range(rows)) for s in steps])


def test_logits_at_the_frame_edges_batched(monkeypatch):
    """geneing_bits9_defaults (3 folds of 6,000 steps, the last one runs 4,400 steps into the tail
    pad): the DBG instances' logits at both sides of the first frame boundary (hop 200), at the
    clamp of the last step and in the pad region -- ring and stream agree bit for bit, and both
    lie within the logit bar of the golden's logits at the step it stores."""
    from test_gpu_logits import LOGIT_ABS_TOL
    name = 'geneing_bits9_defaults'
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, gold, m, hp = _model(name)
    steps = _edge_steps(meta['seq_len'])
    m.set_debug_steps(steps)
    got = {}
    for ring in ('1', '0'):
        monkeypatch.setenv('WRNN_GEN_RING', ring)
        m.set_seed(meta['noise_seed'])
        _golden_call(m, hp, meta)
        assert _names(m) == ['persist_wide'] and (m.stream_info()[0] == 0) == (ring == '1')
        assert np.array_equal(m.last_labels, gold['labels'])
        got[ring] = _logits(m, steps, meta['num_folds'])
        assert np.isfinite(got[ring]).all()
    d = np.argwhere(got['1'].view(np.uint32) != got['0'].view(np.uint32))
    assert len(d) == 0, f'{len(d)} logits differ, first (step index, row, class) {d[0].tolist()}'
    stored = [int(s) for s in gold['logits_steps'] if int(s) in steps]
    assert stored == [0]
    tol = LOGIT_ABS_TOL * max(1.0, float(np.abs(gold['logits']).max()))
    for s in stored:
        ref = gold['logits'][list(gold['logits_steps']).index(s)].astype(np.float64)
        for ring in ('1', '0'):
            err = float(np.abs(got[ring][steps.index(s)].astype(np.float64) - ref).max())
            print(f'{name} WRNN_GEN_RING={ring} step {s}: max |dlogit| {err:.3g} (tol {tol:.3g})')
            assert err <= tol


def test_logits_at_the_frame_edges_unbatched(monkeypatch):
    """Unbatched 6-frame utterances (1,200 steps, no pad region; 9 rows, so one group holds two):
    the same steps, ring against stream, bit for bit."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, _, m, hp = _model('geneing_bits10_tiny')
    steps = _edge_steps(1200)
    m.set_debug_steps(steps)
    dev = _dev_mels(6, [700 + u for u in range(9)])
    got = {}
    for ring in ('1', '0'):
        monkeypatch.setenv('WRNN_GEN_RING', ring)
        m.set_seed(meta['noise_seed'])
        m.generate_batch_device(dev, False, 0, 0)
        assert (m.stream_info()[0] == 0) == (ring == '1')
        got[ring] = _logits(m, steps, 9)
        assert np.isfinite(got[ring]).all()
    d = np.argwhere(got['1'].view(np.uint32) != got['0'].view(np.uint32))
    assert len(d) == 0, f'{len(d)} logits differ, first (step index, row, class) {d[0].tolist()}'


def test_debug_p1_answers_for_ring_calls(monkeypatch):
    """wrnn_debug_p1 re-forms a ring call's P1 on the host from the device tables: equal to the
    stream call's copy at a frame boundary, at the last step and in the pad region (-0.0 == 0.0)."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, gold, m, hp = _model('geneing_bits10_tiny')
    got = {}
    for ring in ('1', '0'):
        monkeypatch.setenv('WRNN_GEN_RING', ring)
        m.set_seed(meta['noise_seed'])
        _golden_call(m, hp, meta)
        assert (m.stream_info()[0] == 0) == (ring == '1')
        got[ring] = np.stack([m.debug_p1(s, r) for s in (0, 1, 199, 200, 201, 1199) for r in (0, 4)])
    assert got['1'].shape == (12, 256, 4) and np.array_equal(got['1'], got['0'])


def test_two_wide_launches_on_one_exchange_area(monkeypatch):
    """152 one-row utterances, wide forced: a launch of 3 rows per group and one of 16. The second
    launch primes its LDS arrays anew; labels equal the stream form's row for row."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, _, m, hp = _model('geneing_bits10_tiny')
    out = _forms(m, meta, _dev_mels(6, [700 + u for u in range(152)]), monkeypatch)
    for ring in ('1', '0'):
        assert sorted((nr, w) for _, nr, w in out[ring][1]) == [(3, True), (16, True)], out[ring][1]
    assert out['1'][2] == (0, 0) and min(out['0'][2]) > 0
    d = np.argwhere(out['1'][0] != out['0'][0])
    assert len(d) == 0, f'first divergence {_first(d)}'


def test_mixed_plan_keeps_its_streams(monkeypatch):
    """131 one-row utterances under the default plan: a register-resident launch of 1 row per group
    and a wide one of 16. The register-resident kernel reads the streams, so the call writes them
    whatever the switch says, and the labels are the stream form's."""
    monkeypatch.delenv('WRNN_PERSIST_WIDE', raising=False)
    meta, _, m, hp = _model('geneing_bits10_tiny')
    out = _forms(m, meta, _dev_mels(6, [700 + u for u in range(131)]), monkeypatch, settings=(None, '1', '0'))
    want = (1200 * 136 * 4 * 256 * 4, 1200 * 136 * 1024 * 4)
    for ring in (None, '1', '0'):
        assert sorted((nr, w) for _, nr, w in out[ring][1]) == [(1, False), (16, True)], out[ring][1]
        assert out[ring][2] == want, (ring, out[ring][2])
    for ring in (None, '1'):
        d = np.argwhere(out[ring][0] != out['0'][0])
        assert len(d) == 0, f'WRNN_GEN_RING={ring}: first divergence {_first(d)}'
