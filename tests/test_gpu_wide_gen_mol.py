"""The continuous heads of the geneing topology on the wide MFMA launch (kernels_persist_wide_gen.hip
k_persist_wide_gen<MODE = 1 MOL | 2 BETA, DBG>: the fc3 epilogue of slots 0 and 1 publishes the 30
/ 2 logits as tagged pairs in the candidate area, hop 3 forms the sample from the k_mol_noise draws
or the Philox gamma draws) against the reference's golden outputs, the oracle and
the register-resident k_persist_gen. ``WRNN_PERSIST_WIDE=1`` makes every launch of a call wide; the
planner offers geneing MOL / Beta calls wide launches only past 32 rows.

Reference: vocoder/distribution.py:104-140 (sample_from_discretized_mix_logistic) and :7-20
(sample_from_beta_dist) after vocoder/models/geneing_version.py:193-210. Bars (the project's own):
per-fold sample / waveform RMS <= 1e-4 (test_gpu_parity.MOL_RMS_TOL) against the reference golden,
the oracle or the register-resident launch; recorded logits within 1e-5 x max(1, |l|) of the golden
logits (test_gpu_logits).
"""
import numpy as np
import pytest

from conftest import golden_case

pytestmark = pytest.mark.gpu

# (fixture, the head's rate key)
HEADS = [pytest.param('geneing_mol_tiny', 'wide_gen_mol', id='mol'),
         pytest.param('geneing_raw_beta_tiny', 'wide_gen_beta', id='beta')]
FILLS = [('geneing_mol_tiny', R) for R in (1, 2, 3, 5, 8, 11, 13, 16)] + \
        [('geneing_raw_beta_tiny', R) for R in (1, 4, 7, 16)]
_ORACLE = {}  # (fixture, mel seed, stream) -> the oracle's samples, computed once per session


def _names(m):
    return [s[0] for s in m.stage_info()]


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _oracle_samples(name, sd, hp, meta, n_frames, mel_seed, stream):
    key = (name, n_frames, mel_seed, stream)
    if key not in _ORACLE:
        import torch
        from oracle.wavernn_oracle import oracle_infer_waveform
        from wavernn_amd.synth import synth_mel
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        ref = oracle_infer_waveform(sd, hp, meta['model_type'], synth_mel(n_frames, mel_seed), batched=False,
                                    target=None, overlap=None, seed=meta['noise_seed'], stream=stream,
                                    post=False)  # (the samples only: a 6-frame wave is too short to fade)
        _ORACLE[key] = ref['samples'].copy()
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def _dev_mels(n_frames, seeds):
    import torch
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    return [torch.from_numpy((synth_mel(n_frames, s) / sp.max_abs_value).astype(np.float32)).cuda() for s in seeds]


def _model(name):
    from test_gpu_parity import make_model
    meta, gold = golden_case(name)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    return meta, gold, m, hp, sd


def _golden_call(m, hp, meta, cb=lambda *a: None):
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    mel = synth_mel(meta['n_frames'], meta['mel_seed']) / sp.max_abs_value
    return m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law, sp.preemphasize,
                      progress_callback=cb)


def _check_golden(name, m, meta, gold, wav):
    from test_gpu_parity import MOL_RMS_TOL
    assert _names(m) == ['persist_wide']
    s = m.last_samples
    assert s.shape == gold['samples'].shape == (meta['num_folds'], meta['seq_len'])
    rms, rms_w = _rms(s, gold['samples']), _rms(wav, gold['wav'])
    print(f'{name}: per-fold sample RMS {rms:.3g}, waveform RMS {rms_w:.3g}')
    assert rms <= MOL_RMS_TOL, f'{name}: per-fold sample RMS {rms}'
    assert rms_w <= MOL_RMS_TOL, f'{name}: waveform RMS {rms_w}'


@pytest.mark.parametrize('name, key', HEADS)
def test_wide_gen_mol_golden_within_tolerance(name, key, monkeypatch):
    """24 frames at 1000 / 100: 5 rows of 1,200 steps, so five groups hold one row and three hold
    only padding."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, gold, m, hp, sd = _model(name)
    assert (meta['num_folds'], meta['seq_len']) == (5, 1200)
    wav = _golden_call(m, hp, meta)
    assert m.plan_info() == [(0, 1, True)], m.plan_info()
    _check_golden(name, m, meta, gold, wav)


@pytest.mark.parametrize('name, key', HEADS)
def test_wide_gen_mol_logits_match_reference(name, key, monkeypatch):
    """The DBG instance of the wide MOL / Beta launch records the 30 / 2 logits (p_dbg_logit) at
    the golden's steps: within the logit bar of the reference's own."""
    from test_gpu_logits import _check, _run
    meta, gold, m, got = _run(name, 'persist', wide=True, monkeypatch=monkeypatch)
    _check(name, meta, gold, got)


@pytest.mark.parametrize('name, R', FILLS, ids=[f'{"beta" if "beta" in n else "mol"}-{R}' for n, R in FILLS])
def test_wide_gen_mol_rows_per_group(name, R, monkeypatch):
    """Group fills of the wide launch, with padding rows in some groups (8 R - R % 3 unbatched
    6-frame utterances, 1200 steps): utterances 0, the middle one and the last against the oracle,
    and against the register-resident launches of the same call (WRNN_PERSIST_WIDE=0), both
    within the RMS bar."""
    from test_gpu_parity import MOL_RMS_TOL
    meta, _, m, hp, sd = _model(name)
    n = 8 * R - R % 3
    dev = _dev_mels(6, [700 + u for u in range(n)])
    out = {}
    for wide in ('1', '0'):
        monkeypatch.setenv('WRNN_PERSIST_WIDE', wide)
        m.set_seed(meta['noise_seed'])
        res, roff, S = m.generate_batch_device(dev, False, 0, 0)
        assert S == 1200 and roff[-1] == n
        plan = m.plan_info()
        assert plan and all(w == (wide == '1') for _, _, w in plan), (R, wide, plan)
        assert _names(m) == (['persist_wide'] if wide == '1' else ['persist']), (R, wide, _names(m))
        if wide == '1':
            assert plan == [(0, R, True)], plan
        out[wide] = res.cpu().numpy()
    for u in sorted({0, n // 2, n - 1}):
        ref = _oracle_samples(name, sd, hp, meta, 6, 700 + u, u)
        r_w, r_0 = _rms(out['1'][u], ref[0]), _rms(out['0'][u], ref[0])
        r_x = _rms(out['1'][u], out['0'][u])
        print(f'{name} R={R} utt {u}: RMS wide / oracle {r_w:.3g}, register-resident / oracle {r_0:.3g}, '
              f'wide / register-resident {r_x:.3g}')
        assert r_w <= MOL_RMS_TOL, f'R={R} utt {u}: wide launch RMS {r_w} (register-resident {r_0})'
        assert r_x <= MOL_RMS_TOL, f'R={R} utt {u}: wide against register-resident RMS {r_x}'


@pytest.mark.parametrize('name, key', HEADS)
def test_wide_gen_mol_two_launches_on_one_exchange_area(name, key, monkeypatch):
    """131 one-row utterances: forced wide, a launch of 16 rows per group and one of 1 row per group
    with padding rows on the same exchange area; with a cheap rate for the head and no environment
    override, a plan with at least one wide launch. Both within the bar of the register-resident
    launches' samples, row for row."""
    from test_gpu_parity import MOL_RMS_TOL
    meta, _, m, hp, sd = _model(name)
    dev = _dev_mels(6, [700 + u for u in range(131)])

    def call():
        m.set_seed(meta['noise_seed'])
        res, roff, S = m.generate_batch_device(dev, False, 0, 0)
        assert S == 1200 and roff[-1] == 131
        return res.cpu().numpy(), m.plan_info()
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '0')
    reg, plan = call()
    assert plan and not any(w for _, _, w in plan), plan
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    forced, plan = call()
    assert sorted((nr, w) for _, nr, w in plan) == [(1, True), (16, True)], plan
    assert _names(m) == ['persist_wide']
    monkeypatch.delenv('WRNN_PERSIST_WIDE')
    m.set_rates(f'{key} 1.0 0.01')
    rated, plan = call()
    assert any(w for _, _, w in plan), plan
    for what, got in (('forced wide', forced), ('cheap rate', rated)):
        rms = [_rms(got[r], reg[r]) for r in range(131)]
        worst = int(np.argmax(rms))
        print(f'{name} {what}: worst row {worst} RMS {rms[worst]:.3g}')
        assert rms[worst] <= MOL_RMS_TOL, f'{what}: row {worst} RMS {rms[worst]}'


@pytest.mark.parametrize('name, key', HEADS)
def test_wide_gen_mol_calls_of_at_most_32_rows_stay_register_resident(name, key, monkeypatch):
    """18 one-row utterances under a very cheap rate for the head: no wide launch, and the samples
    of the call equal the WRNN_PERSIST_WIDE=0 call's bit for bit."""
    meta, _, m, hp, sd = _model(name)
    dev = _dev_mels(6, [700 + u for u in range(18)])
    monkeypatch.delenv('WRNN_PERSIST_WIDE', raising=False)
    m.set_rates(f'{key} 0.1 0.001')
    m.set_seed(meta['noise_seed'])
    res, roff, S = m.generate_batch_device(dev, False, 0, 0)
    plan = m.plan_info()
    assert roff[-1] == 18 and plan and not any(w for _, _, w in plan), plan
    got = res.cpu().numpy()
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '0')
    m.set_seed(meta['noise_seed'])
    res0, _, _ = m.generate_batch_device(dev, False, 0, 0)
    d = np.argwhere(got != res0.cpu().numpy())
    assert len(d) == 0, f'first divergence {d[np.argmin(d[:, 1])].tolist()}'


@pytest.mark.parametrize('name, key', HEADS)
def test_wide_gen_mol_abort_from_the_progress_callback(name, key, monkeypatch):
    """A callback that raises on a wide call stops the launch (WRNN_ERR_ABORTED inside, the
    exception outside), and the next call on the handle gives the golden within the bar."""
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, gold, m, hp, sd = _model(name)
    calls = []

    class Stop(Exception):
        pass

    def cb(i, *a):
        calls.append(i)
        if i >= 200:
            raise Stop()
    with pytest.raises(Stop):
        _golden_call(m, hp, meta, cb)
    assert calls == [0, 100, 200]
    m.set_seed(meta['noise_seed'])
    wav = _golden_call(m, hp, meta)
    _check_golden(name, m, meta, gold, wav)
