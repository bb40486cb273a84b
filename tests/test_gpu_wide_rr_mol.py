"""Runtimeracer mixture-of-logistics batches on the wide MFMA launch (kernels_persist_wide_rr.hip
k_persist_wide_rr<ROT, MOL = true, DBG>: the fc5 epilogue of B slots 0 and 1 publishes the 30
logits as tagged pairs, hop B7 forms the sample from the k_mol_noise draws)
against the reference's golden outputs, the oracle and the register-resident k_persist_rr.
``WRNN_PERSIST_WIDE=1`` makes every launch of a call wide; the default plan offers runtimeracer MOL
calls wide launches past 32 rows (time-sliced when the groups hold more than 16, §3.0f).

Reference: vocoder/distribution.py:104-140 (sample_from_discretized_mix_logistic) after
vocoder/models/runtimeracer_version.py:244-270. Bars (the project's own): per-fold sample / waveform
RMS <= 1e-4 (test_gpu_parity.MOL_RMS_TOL) against the reference golden or the oracle; recorded
logits within 1e-5 x max(1, |l|) of the golden logits (test_gpu_logits).
"""
import numpy as np
import pytest

from conftest import golden_case

pytestmark = pytest.mark.gpu

NAME = 'runtimeracer_mol_tiny'
_ORACLE = {}  # (mel key, stream, fold) -> the oracle's samples, computed once per session


def _stage_names(m):
    return [s[0] for s in m.stage_info()]


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _oracle_samples(sd, hp, meta, n_frames, mel_seed, stream, batched, target, overlap):
    key = (n_frames, mel_seed, stream, batched, target, overlap)
    if key not in _ORACLE:
        import torch
        from oracle.wavernn_oracle import oracle_infer_waveform
        from wavernn_amd.synth import synth_mel
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        ref = oracle_infer_waveform(sd, hp, meta['model_type'], synth_mel(n_frames, mel_seed), batched=batched,
                                    target=target, overlap=overlap, seed=meta['noise_seed'], stream=stream,
                                    post=False)  # (the samples only: a 6-frame wave is too short to fade)
        _ORACLE[key] = ref['samples'].copy()
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def _dev_mels(n_frames, seeds):
    import torch
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    return [torch.from_numpy((synth_mel(n_frames, s) / sp.max_abs_value).astype(np.float32)).cuda() for s in seeds]


def test_wide_rr_mol_golden_within_tolerance(monkeypatch):
    from test_gpu_parity import MOL_RMS_TOL, make_model
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, gold = golden_case(NAME)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    mel = synth_mel(meta['n_frames'], meta['mel_seed']) / sp.max_abs_value
    wav = m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law,
                     sp.preemphasize, progress_callback=lambda *a: None)
    assert _stage_names(m) == ['persist_wide']
    s = m.last_samples
    assert s.shape == gold['samples'].shape == (meta['num_folds'], meta['seq_len'])
    rms, rms_w = _rms(s, gold['samples']), _rms(wav, gold['wav'])
    print(f'{NAME}: per-fold sample RMS {rms:.3g}, waveform RMS {rms_w:.3g}')
    assert rms <= MOL_RMS_TOL, f'{NAME}: per-fold sample RMS {rms}'
    assert rms_w <= MOL_RMS_TOL, f'{NAME}: waveform RMS {rms_w}'


def test_wide_rr_mol_logits_match_reference(monkeypatch):
    """The DBG instance of the wide MOL launch records the 30 logits (p_dbg_logit) at the golden's
    steps: within the logit bar of the reference's own."""
    from test_gpu_logits import _check, _run
    meta, gold, m, got = _run(NAME, 'persist', wide=True, monkeypatch=monkeypatch)
    _check(NAME, meta, gold, got)


@pytest.mark.parametrize('R', [1, 2, 3, 5, 8, 11, 13, 16])
def test_wide_rr_mol_rows_per_group(R, monkeypatch):
    """Group fills of the wide MOL launch, with padding rows in some groups (8 R - R % 3 unbatched
    6-frame utterances, 1200 steps): utterances 0, the middle one and the last against the oracle,
    and against the register-resident launches of the same call (WRNN_PERSIST_WIDE=0), both
    within the RMS bar."""
    from test_gpu_parity import MOL_RMS_TOL, make_model
    meta, _ = golden_case(NAME)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
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
        assert _stage_names(m) == (['persist_wide'] if wide == '1' else ['persist']), (R, wide, _stage_names(m))
        if wide == '1':
            assert plan == [(0, R, True)], plan
        out[wide] = res.cpu().numpy()
    for u in sorted({0, n // 2, n - 1}):
        ref = _oracle_samples(sd, hp, meta, 6, 700 + u, u, False, None, None)
        r_w, r_0 = _rms(out['1'][u], ref[0]), _rms(out['0'][u], ref[0])
        r_x = _rms(out['1'][u], out['0'][u])
        print(f'R={R} utt {u}: RMS wide / oracle {r_w:.3g}, register-resident / oracle {r_0:.3g}, '
              f'wide / register-resident {r_x:.3g}')
        assert r_w <= MOL_RMS_TOL, f'R={R} utt {u}: wide launch RMS {r_w} (register-resident {r_0})'
        assert r_x <= MOL_RMS_TOL, f'R={R} utt {u}: wide against register-resident RMS {r_x}'


def test_wide_rr_mol_time_sliced_batch_matches_oracle():
    """8 utterances of 17 fold rows (136 rows, 17 per group) at target 1000 / overlap 100
    (S = 1200): 17 time-sliced wide launches of 16 rows per group x 75 steps, each row in 16 of them
    with its state and its draws' step offset carried across (§3.0f; plan_wide_slices wants at
    least 64 steps per launch, so S >= 1024); utterances 0 and 7 against the oracle. The rate
    table is the test's own (the RAW wide rate for both runtimeracer wide keys), so the plan does
    not follow whatever rates_mi355x.txt holds."""
    from test_gpu_parity import MOL_RMS_TOL, make_model
    meta, _ = golden_case(NAME)
    m, hp, sd = make_model(meta)
    T = next(t for t in range(2, 2000) if m.fold_shape(t, True, 1000, 100)[0] == 17)
    dev = _dev_mels(T, [700 + u for u in range(8)])
    m.set_engine('persist')
    m.set_seed(meta['noise_seed'])
    m.set_rates('wide_rr_mol 12.0 0.025\nrr 6.7 7.75 8.81 9.87\nslice 60 0.98\n')
    m.enable_stage_timing(True)
    res, roff, S = m.generate_batch_device(dev, True, 1000, 100)
    plan = m.plan_info()
    assert roff[-1] == 136 and S == 1200 and S % 16 == 0, (roff, S)
    assert len(plan) > 1 and all(w for _, _, w in plan), plan
    assert plan == [(0, 16, True)] * 17, plan
    assert _stage_names(m) == ['persist_wide']
    res = res.cpu().numpy()
    for u in (0, 7):
        ref = _oracle_samples(sd, hp, meta, T, 700 + u, u, True, 1000, 100)
        rms = _rms(res[roff[u]:roff[u + 1]], ref)
        print(f'utt {u}: per-fold sample RMS {rms:.3g}')
        assert rms <= MOL_RMS_TOL, f'utt {u}: per-fold sample RMS {rms}'


def test_default_plan_uses_wide_launches_for_the_fork_default_mol_batch():
    """232 MOL rows (8 x 1000 frames at the fork's generation defaults, 6000 / 1000: 29 rows per
    group) -> only wide launches under the shipped rates (profiles/wide_rr_mol/summary.md); the
    samples are finite and inside [-1, 1] (no oracle at this size)."""
    from test_gpu_parity import make_model
    meta, _ = golden_case(NAME)
    m, hp, sd = make_model(meta)
    dev = _dev_mels(1000, range(8))
    m.enable_stage_timing(True)
    out, roff, S = m.generate_batch_device(dev, True, 6000, 1000)
    assert roff[-1] == 232 and S == 8000
    plan = m.plan_info()
    assert plan and all(w for _, _, w in plan), plan
    assert _stage_names(m) == ['persist_wide']
    out = out.cpu().numpy()
    assert out.shape == (232, S) and np.isfinite(out).all()
    assert out.min() >= -1.0 and out.max() <= 1.0


def test_wide_rr_mol_p1_ring_equals_stream(monkeypatch):
    """The wide MOL launch with P1 formed by half A from the per-frame tables or copied from
    k_p1_expand's stream (WRNN_P1_RING=0): identical samples -- one kernel family runs both."""
    from test_gpu_parity import make_model
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, _ = golden_case(NAME)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    dev = _dev_mels(meta['n_frames'], [300 + u for u in range(4)])
    out = []
    for ring in ('1', '0'):
        monkeypatch.setenv('WRNN_P1_RING', ring)
        m.set_seed(meta['noise_seed'])
        res, roff, S = m.generate_batch_device(dev, meta['batched'], meta['target'], meta['overlap'])
        assert _stage_names(m) == ['persist_wide']
        out.append(res.cpu().numpy())
    d = np.argwhere(out[0] != out[1])
    assert len(d) == 0, f'first divergence {d[np.argmin(d[:, 1])].tolist()}'
