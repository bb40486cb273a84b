"""Mixture-of-logistics batches on the wide MFMA launch (kernels_persist_wide.hip
k_persist_wide<ROT, false, MOL = true, DBG>: the fc3 epilogue publishes the 30 logits as tagged
pairs, hop D forms the sample from the k_mol_noise draws) against the reference's
golden outputs and the oracle. ``WRNN_PERSIST_WIDE=1`` makes every launch of a call wide; the
default plan takes wide launches for MOL past 32 rows (C4: time-sliced, §3.0f).

Reference: vocoder/distribution.py:104-140 (sample_from_discretized_mix_logistic) after
vocoder/models/fatchord_version.py:192-236. Bars (the project's own): per-fold sample / waveform
RMS <= 1e-4 (test_gpu_parity.MOL_RMS_TOL) against the reference golden or the oracle; recorded
logits within 1e-5 x max(1, |l|) of the golden logits (test_gpu_logits).
"""
import numpy as np
import pytest

from conftest import golden_case

pytestmark = pytest.mark.gpu

_ORACLE = {}  # (case, mel key, stream) -> the oracle's samples, computed once per session


def _stage_names(m):
    return [s[0] for s in m.stage_info()]


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _oracle_samples(case, sd, hp, meta, n_frames, mel_seed, stream, batched, target, overlap):
    key = (case, n_frames, mel_seed, stream, batched, target, overlap)
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


@pytest.mark.parametrize('name', ['fatchord_mol_tiny', 'fatchord_mol_pruned_tiny'])
def test_wide_mol_golden_within_tolerance(name, monkeypatch):
    from test_gpu_parity import MOL_RMS_TOL, make_model
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
    assert _stage_names(m) == ['persist_wide']
    s = m.last_samples
    assert s.shape == gold['samples'].shape == (meta['num_folds'], meta['seq_len'])
    rms, rms_w = _rms(s, gold['samples']), _rms(wav, gold['wav'])
    print(f'{name}: per-fold sample RMS {rms:.3g}, waveform RMS {rms_w:.3g}')
    assert rms <= MOL_RMS_TOL, f'{name}: per-fold sample RMS {rms}'
    assert rms_w <= MOL_RMS_TOL, f'{name}: waveform RMS {rms_w}'


def test_wide_mol_logits_match_reference(monkeypatch):
    """The DBG instance of the wide MOL launch records the 30 logits (p_dbg_logit) at the golden's
    steps: within the logit bar of the reference's own."""
    from test_gpu_logits import _check, _run
    meta, gold, m, got = _run('fatchord_mol_tiny', 'persist', wide=True, monkeypatch=monkeypatch)
    _check('fatchord_mol_tiny', meta, gold, got)


@pytest.mark.parametrize('R', range(1, 17))
def test_wide_mol_every_rows_per_group(R, monkeypatch):
    """Every group fill of the wide MOL launch, 1..16 rows per group, with padding rows in some
    groups (8 R - R % 3 unbatched 6-frame utterances, 1200 steps): utterances 0, the middle one
    and the last against the oracle, and against the register-resident launch of the same call
    (WRNN_PERSIST_WIDE=0), both within the RMS bar."""
    from test_gpu_parity import MOL_RMS_TOL, make_model
    name = 'fatchord_mol_tiny'
    meta, _ = golden_case(name)
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
        names = _stage_names(m)
        assert names == (['persist_wide'] if wide == '1' else ['persist']), (R, wide, names)
        out[wide] = res.cpu().numpy()
    for u in sorted({0, n // 2, n - 1}):
        ref = _oracle_samples(name, sd, hp, meta, 6, 700 + u, u, False, None, None)
        r_w, r_0 = _rms(out['1'][u], ref[0]), _rms(out['0'][u], ref[0])
        r_x = _rms(out['1'][u], out['0'][u])
        print(f'R={R} utt {u}: RMS wide / oracle {r_w:.3g}, register-resident / oracle {r_0:.3g}, '
              f'wide / register-resident {r_x:.3g}')
        assert r_w <= MOL_RMS_TOL, f'R={R} utt {u}: wide launch RMS {r_w} (register-resident {r_0})'
        assert r_x <= MOL_RMS_TOL, f'R={R} utt {u}: wide against register-resident RMS {r_x}'


def test_wide_mol_time_sliced_batch_matches_oracle():
    """8 utterances of 17 fold rows (136 rows, 17 per group) at target 1000 / overlap 100
    (S = 1200): 17 time-sliced wide launches of 16 rows per group x 75 steps, each row in 16 of them
    with its state and its draws' step offset carried across (§3.0f; plan_wide_slices wants at
    least 64 steps per launch, so S >= 1024); utterances 0 and 7 against the oracle."""
    from test_gpu_parity import MOL_RMS_TOL, make_model
    name = 'fatchord_mol_tiny'
    meta, _ = golden_case(name)
    m, hp, sd = make_model(meta)
    T = next(t for t in range(2, 2000) if m.fold_shape(t, True, 1000, 100)[0] == 17)
    dev = _dev_mels(T, [700 + u for u in range(8)])
    m.set_engine('persist')
    m.set_seed(meta['noise_seed'])
    m.enable_stage_timing(True)
    res, roff, S = m.generate_batch_device(dev, True, 1000, 100)
    plan = m.plan_info()
    assert roff[-1] == 136 and S == 1200 and S % 16 == 0, (roff, S)
    assert len(plan) > 1 and all(w for _, _, w in plan), plan
    assert plan == [(0, 16, True)] * 17, plan
    res = res.cpu().numpy()
    for u in (0, 7):
        ref = _oracle_samples(name, sd, hp, meta, T, 700 + u, u, True, 1000, 100)
        rms = _rms(res[roff[u]:roff[u + 1]], ref)
        print(f'utt {u}: per-fold sample RMS {rms:.3g}')
        assert rms <= MOL_RMS_TOL, f'utt {u}: per-fold sample RMS {rms}'


def test_default_plan_uses_wide_launches_for_c4_mol_rows():
    """144 MOL rows (C4 per GPU, 8 x 1000 frames at 11000 / 550) -> only wide launches under the
    shipped rates; the samples are finite and inside [-1, 1] (no oracle at this size)."""
    from test_gpu_parity import make_model
    meta, _ = golden_case('fatchord_mol_tiny')
    m, hp, sd = make_model(meta)
    dev = _dev_mels(1000, range(8))
    m.enable_stage_timing(True)
    out, roff, S = m.generate_batch_device(dev, True, 11000, 550)
    assert roff[-1] == 144
    plan = m.plan_info()
    assert plan and all(w for _, _, w in plan), plan
    assert _stage_names(m) == ['persist_wide']
    out = out.cpu().numpy()
    assert out.shape == (144, S) and np.isfinite(out).all()
    assert out.min() >= -1.0 and out.max() <= 1.0


def test_wide_mol_p1_ring_equals_stream(monkeypatch):
    """The wide MOL launch with P1 formed in its LDS ring (p1_make) or copied from k_p1_expand's
    stream (WRNN_P1_RING=0): identical samples -- one kernel family runs both."""
    from test_gpu_parity import make_model
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    meta, _ = golden_case('fatchord_mol_tiny')
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
