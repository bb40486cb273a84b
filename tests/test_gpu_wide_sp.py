"""GPU: the block-sparse wide launch of pruned fatchord models (kernels_persist_wide_sp.hip
k_persist_wide_sp, DESIGN.md §3.0g "the wide form").

The reference's Pruner (vocoder/pruner.py:60-88) leaves 90 % of the step matrices' 1 x 4 blocks
zero; its native backend skips them (vocoder/libwavernn/runtimeracer_version/src/wavernn.cpp:
162-184). Here wide row batches of such a model run VALU products over per-slot lists of the live
blocks. Every case sets WRNN_SPARSE_WIDE=1 (and WRNN_PERSIST_WIDE=1 where few rows must run wide)
and asserts sparse_wide_info()['last_call'] and the stage name `persist_wide_sp`.

The sums run in their own fixed order, so labels are compared with the reference / the oracle /
the dense wide kernel exactly, and a differing row is accepted only as a measured near-tie
(tests/near_tie_util.analyse), at most one row per case, its record printed -- zero expected.
Within the kernel a row's labels and logits are bit-identical across group fills, time slicing
and fold ranges.
"""
import numpy as np
import pytest

from conftest import golden_case, wave_equal

pytestmark = pytest.mark.gpu

FIXTURES = ['fatchord_raw9_c2_pruned', 'fatchord_raw10_pruned_defaults', 'fatchord_raw9_c2_pruned_peaked']


@pytest.fixture(autouse=True)
def sparse_wide(monkeypatch):
    monkeypatch.setenv('WRNN_SPARSE_WIDE', '1')
    monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    monkeypatch.delenv('WRNN_PERSIST_SLICE', raising=False)


def ran_sparse_wide(m, only=True):
    names = [s[0] for s in m.stage_info()]
    info = m.sparse_wide_info()
    assert info['available'] and info['last_call'], info
    assert 'persist_wide_sp' in names and (not only or names == ['persist_wide_sp']), names
    return info


def pruned_tiny():
    """fatchord_raw9_tiny's hyper-parameters, its seeded weights pruned at 0.9"""
    from test_gpu_parity import make_model
    meta, _ = golden_case('fatchord_raw9_tiny')
    meta = dict(meta, prune=0.9)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    return meta, m, hp, sd


def dev_mels(frames, n, seed0):
    import torch
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    mels = [synth_mel(frames, seed0 + u) / sp.max_abs_value for u in range(n)]
    return mels, [torch.from_numpy(x.astype(np.float32)).cuda() for x in mels]


def accept_near_ties(what, lab, ref, seed, row_stream, row_fold, logits_of, ref_logits_of):
    """lab == ref, or at most one row differs and its first difference is a near-tie:
    logits_of(steps) / ref_logits_of(steps) -> {step: (rows, classes)} recorded teacher-forced
    by the two sides at those steps."""
    from near_tie_util import analyse, first_divergence_per_row
    from wavernn_amd import _abi
    assert lab.shape == ref.shape, (what, lab.shape, ref.shape)
    fd = first_divergence_per_row(lab, ref)
    bad = np.flatnonzero(fd >= 0)
    if len(bad) == 0:
        return 0
    assert len(bad) <= 1, f'{what}: rows {bad.tolist()} differ, first at steps {fd[bad].tolist()}'
    r, s = int(bad[0]), int(fd[bad[0]])
    g, o = logits_of([s]), ref_logits_of([s])
    _, recs = analyse(_abi.load_library(), seed, int(row_stream[r]), lab[r:r + 1], ref[r:r + 1], {s: g[s][r:r + 1]},
                      {s: o[s][r:r + 1]}, fold0=int(row_fold[r]))
    for rec in recs:
        print(f'{what}: near-tie check of row {r}: {rec}')
    assert recs and all(rec['near_tie'] for rec in recs), (what, recs)
    return 1


@pytest.mark.parametrize('name', FIXTURES)
def test_reference_fixture_on_the_sparse_wide_kernel(name):
    """Labels equal the reference's, the waveform is the reference's, and the teacher-forced
    logits at the fixture's recorded steps are within 1e-5 x max(1, |l|) of the reference's (the
    project's bar for every engine, test_gpu_logits.py)."""
    import torch
    from oracle.wavernn_oracle import OracleWaveRNN
    from test_gpu_parity import make_model
    from conftest import hparams_of, state_dict_of
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    meta, gold = golden_case(name)
    mel = synth_mel(meta['n_frames'], meta['mel_seed']) / sp.max_abs_value
    gsteps = [int(s) for s in gold['logits_steps']]
    rows = range(meta['num_folds'])

    def run(steps):
        m, hp, sd = make_model(meta)
        m.set_engine('persist')
        m.enable_stage_timing(True)
        m.set_debug_steps(steps)
        wav = m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law,
                         sp.preemphasize, progress_callback=lambda *a: None)
        info = ran_sparse_wide(m)
        assert info['density'] < 0.2 and 0 < info['fill_f4'] <= 4096, info
        return m, wav

    m, wav = run(gsteps)
    lab = m.last_labels
    got = np.stack([m.debug_logits(s, rows) for s in gsteps])
    assert np.isfinite(got).all()
    # (a row that left the reference before a recorded step is not teacher-forced there)
    live = np.array([[(lab[r, :s] == gold['labels'][r, :s]).all() for r in rows] for s in gsteps])
    dl = np.abs(got.astype(np.float64) - gold['logits'].astype(np.float64)).max(axis=-1)
    err, top = float(dl[live].max()), float(np.abs(gold['logits']).max())
    print(f'{name}: max |dlogit| {err:.3g}, |logit| <= {top:.3g}, tol {1e-5 * max(1.0, top):.3g}')
    assert err <= 1e-5 * max(1.0, top)

    def sparse_logits(steps):
        m2, _ = run(steps)
        assert np.array_equal(m2.last_labels, lab)
        return {s: m2.debug_logits(s, rows) for s in steps}

    def oracle_logits(steps):
        hp = hparams_of(meta)
        sdt = {k: torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v
               for k, v in state_dict_of(meta).items()}
        o = OracleWaveRNN(sdt, hp, meta['model_type']).generate(
            torch.from_numpy(mel[None].astype(np.float32)), meta['batched'], meta['target'], meta['overlap'],
            hp.mu_law, True, seed=meta['noise_seed'], stream=0, max_steps=max(steps) + 1, record_logits=steps,
            post=False)
        return o['logits']

    n = accept_near_ties(name, lab, gold['labels'], meta['noise_seed'], np.zeros(len(lab), int),
                         np.arange(len(lab)), sparse_logits, oracle_logits)
    if n == 0:
        assert wave_equal(wav, gold)


def test_every_group_fill_matches_the_dense_wide_kernel(monkeypatch):
    """Every group fill 1..16 with padding rows in some groups (8 R - R % 3 unbatched 6-frame
    utterances, the shape of test_wide_every_rows_per_group_matches_register_resident): the labels
    equal those of the same call with WRNN_SPARSE_WIDE=0."""
    meta, m, hp, sd = pruned_tiny()
    accepted = 0
    for R in range(1, 17):
        n = 8 * R - R % 3
        _, dev = dev_mels(6, n, 700)

        def call(sparse, steps=None):
            monkeypatch.setenv('WRNN_SPARSE_WIDE', sparse)
            m.set_debug_steps(steps or [])
            m.set_seed(meta['noise_seed'])
            lab, roff, S = m.generate_batch_device(dev, False, 0, 0)
            if sparse == '1':
                ran_sparse_wide(m)
            else:
                assert [s[0] for s in m.stage_info()] == ['persist_wide'] and not m.sparse_wide_info()['last_call']
            assert m.plan_info() == [(0, R, True)]
            out = lab.cpu().numpy()
            return out, ({s: m.debug_logits(s, range(n)) for s in steps} if steps else None)

        sp_lab, _ = call('1')
        de_lab, _ = call('0')
        accepted += accept_near_ties(f'R={R}', sp_lab, de_lab, meta['noise_seed'], np.arange(n), np.zeros(n, int),
                                     lambda st: call('1', st)[1], lambda st: call('0', st)[1])
    assert accepted <= 1


def test_a_rows_results_do_not_depend_on_the_group_fill():
    """The same 5 utterances alone (1 row in 5 groups) and as the first 5 of 65 (9 rows per group
    in one): their rows' labels and recorded logits are bit-identical."""
    meta, m, hp, sd = pruned_tiny()
    _, dev = dev_mels(6, 65, 900)
    out = []
    for n in (5, 65):
        m.set_seed(meta['noise_seed'])
        lab, roff, S = m.generate_batch_device(dev[:n], False, 0, 0)
        steps = [0, 1, S // 2, S - 1]
        m.set_debug_steps(steps)
        m.set_seed(meta['noise_seed'])
        lab2, _, _ = m.generate_batch_device(dev[:n], False, 0, 0)
        ran_sparse_wide(m)
        assert np.array_equal(lab.cpu().numpy(), lab2.cpu().numpy())
        out.append((lab.cpu().numpy()[:5], np.stack([m.debug_logits(s, range(5)) for s in steps])))
        m.set_debug_steps([])
    assert np.array_equal(out[0][0], out[1][0])
    assert np.isfinite(out[0][1]).all() and np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def sliced_shape(m, folds):
    """The smallest target / overlap whose folds are 512 steps long (plan_wide_slices needs S / 8
    >= 64 at 18 rows per group), and a mel length that makes `folds` of them."""
    for overlap in range(8, 64, 8):
        target = 512 - 2 * overlap
        for t in range(2, 400):
            nf, S = m.fold_shape(t, True, target, overlap)[:2]
            if nf == folds and S == 512:
                return t, target, overlap
    raise AssertionError('no such shape')


def test_time_sliced_9_bit_batch_matches_the_oracle_and_the_unsliced_call(monkeypatch):
    """8 utterances of 18 folds (144 rows, 18 per group): time-sliced sparse-wide launches.
    Utterances 0 and 7 against the oracle on the pruned weights; every row against the unsliced
    sparse-wide call (WRNN_PERSIST_SLICE=0), bit for bit."""
    from oracle.wavernn_oracle import oracle_infer_waveform
    from wavernn_amd.hparams import sp
    meta, m, hp, sd = pruned_tiny()
    T, target, overlap = sliced_shape(m, 18)
    mels, dev = dev_mels(T, 8, 500)
    m.set_seed(meta['noise_seed'])
    lab, roff, S = m.generate_batch_device(dev, True, target, overlap)
    plan = m.plan_info()
    ran_sparse_wide(m)
    # (9 launches of 16 rows per group x 64 steps: every row in 8 of them, no steps left over)
    assert roff[-1] == 144 and S == 512 and plan == [(0, 16, True)] * 9, (roff, S, plan)
    lab = lab.cpu().numpy()
    monkeypatch.setenv('WRNN_PERSIST_SLICE', '0')
    m.set_seed(meta['noise_seed'])
    whole, _, _ = m.generate_batch_device(dev, True, target, overlap)
    ran_sparse_wide(m)
    assert sorted(p[1:] for p in m.plan_info()) == [(2, True), (16, True)], m.plan_info()
    assert np.array_equal(lab, whole.cpu().numpy())
    for u in (0, 7):
        ref = oracle_infer_waveform(sd, hp, meta['model_type'], mels[u] * sp.max_abs_value, target=target,
                                    overlap=overlap, seed=meta['noise_seed'], stream=u)
        got = lab[roff[u]:roff[u + 1]]
        d = np.argwhere(got != ref['labels'])
        # (no near-tie allowance taken: a difference fails with its place)
        assert len(d) == 0, f'utt {u}: first divergence {d[np.argmin(d[:, 1])].tolist()}'


def test_time_sliced_10_bit_batch_matches_the_oracle(monkeypatch):
    """The 136-row shape of test_wide_10bit_time_sliced_batch_matches_oracle on pruned weights: 17
    time-sliced launches on the 1024-class instances, utterances 0 and 7 against the oracle."""
    import torch
    from oracle.wavernn_oracle import oracle_infer_waveform
    from test_gpu_parity import make_model
    from wavernn_amd.hparams import sp
    monkeypatch.delenv('WRNN_PERSIST_WIDE')
    meta, _ = golden_case('fatchord_raw10_pruned_defaults')
    m, hp, sd = make_model(meta)
    T = next(t for t in range(2, 2000) if m.fold_shape(t, True, 3000, 1500)[0] == 17)
    mels, dev = dev_mels(T, 8, 700)
    m.set_engine('persist')
    m.set_seed(meta['noise_seed'])
    m.enable_stage_timing(True)
    lab, roff, S = m.generate_batch_device(dev, True, 3000, 1500)
    plan = m.plan_info()
    ran_sparse_wide(m)
    assert roff[-1] == 136 and S == 6000 and plan == [(0, 16, True)] * 17, (roff, S, plan)
    lab = lab.cpu().numpy()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    for u in (0, 7):
        ref = oracle_infer_waveform(sd, hp, meta['model_type'], mels[u] * sp.max_abs_value,
                                    target=3000, overlap=1500, seed=meta['noise_seed'], stream=u)
        got = lab[roff[u]:roff[u + 1]]
        d = np.argwhere(got != ref['labels'])
        assert len(d) == 0, f'utt {u}: first divergence {d[np.argmin(d[:, 1])].tolist()}'


def test_fold_ranges_equal_the_whole_call():
    """A ranged call on the 144-row shape: the two halves of every utterance's folds equal the
    whole sparse-wide call's rows bit for bit."""
    meta, m, hp, sd = pruned_tiny()
    T, target, overlap = sliced_shape(m, 18)
    _, dev = dev_mels(T, 8, 500)
    streams = list(range(8))
    m.set_seed(meta['noise_seed'])
    whole, roff, S = m.generate_batch_device(dev, True, target, overlap, streams=streams)
    ran_sparse_wide(m)
    whole = whole.cpu().numpy().reshape(8, 18, S)
    for lo, hi in ((0, 9), (9, 18)):
        m.set_seed(meta['noise_seed'])
        part, proff, _ = m.generate_batch_device(dev, True, target, overlap, streams=streams,
                                                 fold_ranges=[(lo, hi)] * 8)
        ran_sparse_wide(m)
        assert proff[-1] == 8 * (hi - lo)
        assert np.array_equal(part.cpu().numpy().reshape(8, hi - lo, S), whole[:, lo:hi])


def test_abort_then_the_next_call_is_correct():
    """A callback abort ends the sparse-wide launch (WRNN_ERR_ABORTED behind the exception) and
    the handle runs the next call correctly. The aborted call is the call that ran whole just
    before it (same handle, weights, input and switches: the same plan), and the handle's record
    of it says a launch of it was planned block-sparse."""
    from test_gpu_parity import make_model
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    meta, gold = golden_case('fatchord_raw9_c2_pruned')
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    mel = synth_mel(meta['n_frames'], meta['mel_seed']) / sp.max_abs_value
    m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law, sp.preemphasize,
               progress_callback=lambda *a: None)
    ran_sparse_wide(m)
    plan = m.plan_info()
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
    # (the aborted call's own plan: wrnn_sparse_wide_info reads what that call planned)
    assert m.sparse_wide_info()['last_call']
    m.set_seed(meta['noise_seed'])
    wav = m.generate(mel[None], meta['batched'], meta['target'], meta['overlap'], hp.mu_law, sp.preemphasize,
                     progress_callback=lambda *a: None)
    ran_sparse_wide(m)
    assert m.plan_info() == plan
    assert np.array_equal(m.last_labels, gold['labels']) and wave_equal(wav, gold)


def test_dense_weights_have_no_image_and_run_the_mfma_kernel():
    from test_gpu_parity import make_model
    meta, gold = golden_case('fatchord_raw9_tiny')
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    _, dev = dev_mels(meta['n_frames'], 1, meta['mel_seed'])
    info = m.sparse_wide_info()
    assert not info['available'] and info['density'] > 0.99, info
    m.set_seed(meta['noise_seed'])
    lab, _, _ = m.generate_batch_device(dev, meta['batched'], meta['target'], meta['overlap'])
    assert [s[0] for s in m.stage_info()] == ['persist_wide'] and not m.sparse_wide_info()['last_call']
    assert np.array_equal(lab.cpu().numpy(), gold['labels'])
