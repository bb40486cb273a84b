"""The geneing wide-row launch (kernels_persist_wide_gen.hip: up to 16 rows per XCD group, every
product on the fp32 matrix cores, three exchanges per step) against the reference's golden
outputs, the oracle and the register-resident geneing kernel. ``WRNN_PERSIST_WIDE=1`` makes every
launch of a call wide; the default plan takes wide launches only past 32 rows.

Reference step: vocoder/models/geneing_version.py:193-205; bar: bit-exact labels (9 / 10 bit),
recorded logits within 1e-5 x max(1, |l|) of the golden logits (test_gpu_logits).
"""
import numpy as np
import pytest

from conftest import golden_case, wave_equal
from test_plan_wide_gen import DEFAULT_360

pytestmark = pytest.mark.gpu

FIXTURES = ['geneing_bits10_tiny', 'geneing_bits9_defaults']
_ORACLE = {}  # (case, mel seed, stream) -> the oracle's labels, computed once per session


def _names(m):
    return [s[0] for s in m.stage_info()]


def _dev_mels(n_frames, seeds):
    import torch
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    return [torch.from_numpy((synth_mel(n_frames, s) / sp.max_abs_value).astype(np.float32)).cuda() for s in seeds]


def _oracle_labels(case, sd, hp, meta, n_frames, mel_seed, stream):
    key = (case, n_frames, mel_seed, stream)
    if key not in _ORACLE:
        import torch
        from oracle.wavernn_oracle import oracle_infer_waveform
        from wavernn_amd.synth import synth_mel
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        ref = oracle_infer_waveform(sd, hp, meta['model_type'], synth_mel(n_frames, mel_seed), batched=False,
                                    target=None, overlap=None, seed=meta['noise_seed'], stream=stream,
                                    post=False)
        _ORACLE[key] = ref['labels'].copy()
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def _first(d):
    return d[np.argmin(d[:, 1])].tolist()


@pytest.mark.parametrize('name', FIXTURES)
def test_wide_gen_golden_bit_exact(name, monkeypatch):
    from test_gpu_parity import make_model
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, gold = golden_case(name)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    mel = synth_mel(meta['n_frames'], meta['mel_seed']) / sp.max_abs_value
    wav = m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law,
                     sp.preemphasize, progress_callback=lambda *a: None)
    assert _names(m) == ['persist_wide']
    lab = m.last_labels
    assert lab.shape == gold['labels'].shape == (meta['num_folds'], meta['seq_len'])
    d = np.argwhere(lab != gold['labels'])
    assert len(d) == 0, f'first divergence {_first(d)}'
    assert wave_equal(wav, gold)


@pytest.mark.parametrize('name', FIXTURES)
def test_wide_gen_logits_match_reference(name, monkeypatch):
    """The DBG instance records the logits (p_dbg_logit) at the golden's steps: within the logit
    bar of the reference's own."""
    from test_gpu_logits import _check, _run
    meta, gold, m, got = _run(name, 'persist', wide=True, monkeypatch=monkeypatch)
    _check(name, meta, gold, got, m.last_labels)


def _both(m, meta, dev, monkeypatch):
    out = {}
    for wide in ('1', '0'):
        monkeypatch.setenv('WRNN_PERSIST_WIDE', wide)
        m.set_seed(meta['noise_seed'])
        lab, roff, S = m.generate_batch_device(dev, False, 0, 0)
        assert S == 1200 and roff[-1] == len(dev)
        assert _names(m) == (['persist_wide'] if wide == '1' else ['persist']), (wide, _names(m))
        out[wide] = (lab.cpu().numpy(), m.plan_info())
    return out


@pytest.mark.parametrize('R', range(1, 17))
def test_wide_gen_every_rows_per_group(R, monkeypatch):
    """Every group fill, 1..16 rows per group, with padding rows in some groups (8 R - R % 3
    unbatched 6-frame utterances, 1200 steps): wide labels equal the register-resident kernel's
    row for row; for R = 1 and 16 utterances 0, the middle one and the last also equal the
    oracle's (k_persist_gen is oracle-pinned, the other fills lean on it)."""
    from test_gpu_parity import make_model
    name = 'geneing_bits10_tiny'
    meta, _ = golden_case(name)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    n = 8 * R - R % 3
    out = _both(m, meta, _dev_mels(6, [700 + u for u in range(n)]), monkeypatch)
    assert out['1'][1] == [(0, R, True)], out['1'][1]
    d = np.argwhere(out['1'][0] != out['0'][0])
    assert len(d) == 0, f'R={R} ({n} rows): first divergence {_first(d)}'
    if R in (1, 16):
        for u in sorted({0, n // 2, n - 1}):
            ref = _oracle_labels(name, sd, hp, meta, 6, 700 + u, u)
            d = np.argwhere(out['1'][0][u:u + 1] != ref)
            assert len(d) == 0, f'R={R} utt {u}: first divergence from the oracle {_first(d)}'


def test_wide_gen_two_launches_one_nearly_empty(monkeypatch):
    """131 one-row utterances: a launch of 16 rows per group and one of 1 row per group with padding
    rows (the planner runs the small one first); equal to the register-resident launches' labels
    row for row. The default plan of this call mixes the two kernels (a register-resident launch
    of 1 row per group, then a wide one of 16) on one exchange area: equal too."""
    from test_gpu_parity import make_model
    meta, _ = golden_case('geneing_bits10_tiny')
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    dev = _dev_mels(6, [700 + u for u in range(131)])
    out = _both(m, meta, dev, monkeypatch)
    plan = out['1'][1]
    assert sorted((nr, w) for _, nr, w in plan) == [(1, True), (16, True)], plan
    assert plan[0][0] == 0 and plan[1][0] == 8 * plan[0][1], plan
    d = np.argwhere(out['1'][0] != out['0'][0])
    assert len(d) == 0, f'first divergence {_first(d)}'
    monkeypatch.delenv('WRNN_PERSIST_WIDE')
    m.set_seed(meta['noise_seed'])
    lab, roff, S = m.generate_batch_device(dev, False, 0, 0)
    assert sorted((nr, w) for _, nr, w in m.plan_info()) == [(1, False), (16, True)], m.plan_info()
    d = np.argwhere(lab.cpu().numpy() != out['0'][0])
    assert len(d) == 0, f'default plan: first divergence {_first(d)}'


def test_default_plan_at_the_fork_default_shape(monkeypatch):
    """8 x 1000-frame mels at 3000 / 1500: 360 rows x 6,000 steps, the one size at which the P1 and
    noise stream offsets pass 4 GiB. The default plan is the one the host test pins; labels in
    range and equal to the register-resident launches' row for row (no oracle at this size)."""
    from test_gpu_parity import make_model
    meta, _ = golden_case('geneing_bits10_tiny')
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    dev = _dev_mels(1000, range(8))
    out = {}
    for wide in (None, '0'):
        if wide is None:
            monkeypatch.delenv('WRNN_PERSIST_WIDE', raising=False)
        else:
            monkeypatch.setenv('WRNN_PERSIST_WIDE', wide)
        m.set_seed(meta['noise_seed'])
        lab, roff, S = m.generate_batch_device(dev, True, 3000, 1500)
        assert roff[-1] == 360 and S == 6000, (roff, S)
        out[wide] = lab.cpu().numpy()
        if wide is None:
            assert [(nr, w) for _, nr, w in m.plan_info()] == DEFAULT_360, m.plan_info()
        else:
            assert not any(w for _, _, w in m.plan_info()), m.plan_info()
    lab = out[None]
    assert lab.shape == (360, 6000) and lab.min() >= 0 and lab.max() < 1024
    d = np.argwhere(lab != out['0'])
    assert len(d) == 0, f'{len(d)} labels differ, first divergence {_first(d)}'


def test_wide_gen_abort_from_the_progress_callback(monkeypatch):
    """A callback that raises on a wide geneing call stops the launch (WRNN_ERR_ABORTED inside,
    the exception outside), and the next call on the handle succeeds with the golden labels."""
    from test_gpu_parity import make_model
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, gold = golden_case('geneing_bits10_tiny')
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    mel = synth_mel(meta['n_frames'], meta['mel_seed']) / sp.max_abs_value
    calls = []

    class Stop(Exception):
        pass

    def cb(i, *a):
        calls.append(i)
        if i >= 200:
            raise Stop()
    with pytest.raises(Stop):
        m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law, sp.preemphasize,
                   progress_callback=cb)
    assert calls == [0, 100, 200]
    m.set_seed(meta['noise_seed'])
    wav = m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law, sp.preemphasize,
                     progress_callback=lambda *a: None)
    assert _names(m) == ['persist_wide']
    assert np.array_equal(m.last_labels, gold['labels'])
    assert wave_equal(wav, gold)
