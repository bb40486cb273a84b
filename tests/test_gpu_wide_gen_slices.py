"""Time-sliced instances of the geneing wide launch (kernels_persist_wide_gen.hip
k_persist_wide_gen_rot<MODE, DBG>), selected by
``WaveRNN.set_wide_slices(True)`` / ``WRNN_GEN_SLICE=1``.

A call of 8 R_g rows with R_g just above 16 runs as launches of 16 rows per group over rotating row
sets; a row crosses launches through its chunk state (x1, h1) and runs every launch at its own step
offset. Its arithmetic is the 16-row ring instance's, so the bar is bit equality with the unsliced
wide launches of the same call (labels; float samples and logits compared as uint32), and the
project's bars against the oracle: bit-exact labels, per-row sample RMS <= 1e-4 (MOL / Beta),
logits within 1e-5 x max(1, |l|).

Shapes: 136 one-row unbatched utterances of 6 frames (1,200 steps, R_g = 17: 17 launches of 75
steps, row i of every group sits out launch i), of 7 frames (1,400 steps: 17 launches of 87 steps
and tail launches of 16 and 1 rows per group x 8 steps), 144 utterances (R_g = 18: 9 launches of 150 steps,
two rows of a group idle in each) and 131 utterances (padded to 136 rows).
"""
import numpy as np
import pytest

from conftest import golden_case
from test_gpu_wide_gen import _dev_mels, _first, _names
from test_gpu_wide_gen_mol import _rms

pytestmark = pytest.mark.gpu

BITS, MOL, BETA = 'geneing_bits10_tiny', 'geneing_mol_tiny', 'geneing_raw_beta_tiny'
HEADS = [pytest.param(BITS, id='bits'), pytest.param(MOL, id='mol'), pytest.param(BETA, id='beta')]
ENV = ('WRNN_PERSIST_WIDE', 'WRNN_GEN_SLICE', 'WRNN_GEN_RING', 'WRNN_GEN_WIDE_ROWS', 'WRNN_PERSIST_SLICE')
ORACLE_ROWS = (0, 8, 135)  # sits out the first launch | runs from it, next to row 0 in its wave | the last row
# step 0, both sides of the slice boundaries 74 | 75, 374 | 375 and 1124 | 1125, the last step
LOGIT_STEPS = (0, 74, 75, 374, 375, 1124, 1125, 1199)
MIXED = [(1, False), (16, True)]  # the default plan of 136 rows: one register-resident row per group
_MELS = {}    # (frames, utterances) -> the device mels, built once per session
_ORACLE = {}  # (fixture, frames, utterance) -> the oracle's outputs and logits, computed once per session


def _model(name):
    from test_gpu_parity import make_model
    meta, gold = golden_case(name)
    m, hp, sd = make_model(meta)
    m.set_engine('persist')
    m.enable_stage_timing(True)
    return meta, m, hp, sd


def _mels(frames, n):
    if (frames, n) not in _MELS:
        _MELS[frames, n] = _dev_mels(frames, [700 + u for u in range(n)])
    return _MELS[frames, n]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _clean(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _call(m, meta, dev, slices, monkeypatch, wide=False, cb=None):
    """One call: (outputs, plan, stream_info, S). wide: every launch forced wide (unsliced when the
    switch is off)."""
    _clean(monkeypatch)
    if wide:
        monkeypatch.setenv('WRNN_PERSIST_WIDE', '1')
    m.set_wide_slices(slices)
    m.set_seed(meta['noise_seed'])
    res, roff, S = m.generate_batch_device(dev, False, 0, 0, progress_callback=cb, streams=list(range(len(dev))))
    assert roff[-1] == len(dev)
    return res.cpu().numpy(), m.plan_info(), m.stream_info(), S


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype
    d = np.argwhere(_bits(a) != _bits(b))
    assert len(d) == 0, f'{what}: {len(d)} values differ, first (row, step) {_first(d)}'


def _oracle(name, sd, hp, meta, frames, u):
    """(labels for BITS, else samples; {step: logits at LOGIT_STEPS}) of utterance u from the oracle,
    free-running from the same seed and stream. One run serves the output and the logit checks."""
    key = (name, frames, u)
    if key not in _ORACLE:
        import torch
        from oracle.wavernn_oracle import oracle_infer_waveform
        from wavernn_amd.synth import synth_mel
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        ref = oracle_infer_waveform(sd, hp, meta['model_type'], synth_mel(frames, 700 + u), batched=False,
                                    target=None, overlap=None, seed=meta['noise_seed'], stream=u, post=False,
                                    record_logits=list(LOGIT_STEPS))
        out = ref['labels' if name == BITS else 'samples'].copy()
        _ORACLE[key] = (out, {int(s): np.asarray(l).copy() for s, l in ref['logits'].items()})
    return _ORACLE[key]


def _check_sliced_plan(plan, m, S, n_rows, expect):
    """expect: [(rows per group, steps)] of the launches, all wide from row 0."""
    assert plan == [(0, nr, True) for nr, _ in expect], plan
    assert _names(m) == ['persist_wide'] and m.rot_info() == (0, 0, 0)
    steps = sum(s for _, s in expect)
    assert m.persist_steps(0) == pytest.approx(steps / len(expect))


@pytest.mark.parametrize('name', HEADS)
def test_sliced_call_equals_the_unsliced_plans(name, monkeypatch):
    """136 rows x 1,200 steps: 17 wide launches of 75 steps, no stream but the MOL draws; equal to
    the forced-wide unsliced plan bit for bit (BITS: and to the default mixed plan)."""
    meta, m, hp, sd = _model(name)
    dev = _mels(6, 136)
    got, plan, streams, S = _call(m, meta, dev, True, monkeypatch)
    assert S == 1200 and got.shape == (136, 1200)
    _check_sliced_plan(plan, m, S, 136, [(16, 75)] * 17)
    assert streams == (0, 1200 * 136 * 12 * 4 if name == MOL else 0), streams
    assert np.isfinite(got.astype(np.float64)).all()
    wide, wplan, _, _ = _call(m, meta, dev, False, monkeypatch, wide=True)
    assert sorted((nr, w) for _, nr, w in wplan) == [(1, True), (16, True)], wplan
    _same(got, wide, f'{name} sliced against forced wide')
    if name == BITS:
        dflt, dplan, dstreams, _ = _call(m, meta, dev, False, monkeypatch)
        assert sorted((nr, w) for _, nr, w in dplan) == MIXED and dstreams[0] > 0, (dplan, dstreams)
        _same(got, dflt, 'sliced against the default plan')


@pytest.mark.parametrize('u', ORACLE_ROWS)
@pytest.mark.parametrize('name', HEADS)
def test_sliced_rows_against_the_oracle(name, u, monkeypatch):
    """The same call against the oracle, one row a case (an oracle row takes 1-3 s): row 0 sits out
    the first launch, row 8 runs from it and shares row 0's wave span, row 135 is the last."""
    from test_gpu_parity import MOL_RMS_TOL
    meta, m, hp, sd = _model(name)
    got, plan, _, _ = _call(m, meta, _mels(6, 136), True, monkeypatch)
    assert len(plan) == 17
    ref, _ = _oracle(name, sd, hp, meta, 6, u)
    if name == BITS:
        d = np.argwhere(got[u:u + 1] != ref)
        assert len(d) == 0, f'utt {u}: first divergence from the oracle {_first(d)}'
    else:
        rms = _rms(got[u], ref[0])
        print(f'{name} utt {u}: sample RMS against the oracle {rms:.3g}')
        assert rms <= MOL_RMS_TOL, f'{name} utt {u}: sample RMS {rms}'


@pytest.mark.parametrize('name', HEADS)
def test_tail_launches_and_the_last_step(name, monkeypatch):
    """1,400 steps: 17 launches of 87 steps and two tail launches of 8 (16 and 1 rows per group);
    every row's last steps (its own clamp of P1) equal the unsliced plan's."""
    meta, m, hp, sd = _model(name)
    dev = _mels(7, 136)
    got, plan, streams, S = _call(m, meta, dev, True, monkeypatch)
    assert S == 1400
    _check_sliced_plan(plan, m, S, 136, [(16, 87)] * 17 + [(16, 8), (1, 8)])
    assert streams == (0, 1400 * 136 * 12 * 4 if name == MOL else 0), streams
    wide, wplan, _, _ = _call(m, meta, dev, False, monkeypatch, wide=True)
    assert all(w for _, _, w in wplan) and len(wplan) == 2, wplan
    assert np.array_equal(_bits(got[:, -1]), _bits(wide[:, -1])), 'last sample of some row differs'
    _same(got, wide, f'{name} 1,400 steps')


@pytest.mark.parametrize('name', HEADS)
def test_two_idle_rows_per_group(name, monkeypatch):
    """144 rows (R_g = 18): 9 launches of 150 steps, the idle pair of a group moves on by 2 rows."""
    meta, m, hp, sd = _model(name)
    dev = _mels(6, 144)
    got, plan, streams, S = _call(m, meta, dev, True, monkeypatch)
    _check_sliced_plan(plan, m, S, 144, [(16, 150)] * 9)
    wide, wplan, _, _ = _call(m, meta, dev, False, monkeypatch, wide=True)
    assert sorted((nr, w) for _, nr, w in wplan) == [(2, True), (16, True)], wplan
    _same(got, wide, f'{name} 144 rows')


@pytest.mark.parametrize('name', HEADS)
def test_rows_that_are_no_multiple_of_8_are_padded(name, monkeypatch):
    """131 utterances: planned as 136 rows (five padding rows, drawn and never returned)."""
    meta, m, hp, sd = _model(name)
    dev = _mels(6, 131)
    got, plan, streams, S = _call(m, meta, dev, True, monkeypatch)
    assert got.shape == (131, 1200)
    _check_sliced_plan(plan, m, S, 131, [(16, 75)] * 17)
    assert streams == (0, 1200 * 136 * 12 * 4 if name == MOL else 0), streams
    if name == BITS:
        ref, rplan, _, _ = _call(m, meta, dev, False, monkeypatch)
        assert not all(w for _, _, w in rplan), rplan
    else:
        ref, rplan, _, _ = _call(m, meta, dev, False, monkeypatch, wide=True)
    _same(got, ref, f'{name} 131 rows')


@pytest.mark.parametrize('name', HEADS)
def test_dbg_instance_logits_across_slice_boundaries(name, monkeypatch):
    """The DBG instances: logits of every row at step 0, at both sides of the boundary 74 | 75 (rows
    0-7, which start in the second launch) and 374 | 375 (rows 40-47, idle in launch 5; most other
    rows cross 75 x k boundaries there too), at 1124 | 1125 and at the last step. From launch 2 on,
    the slots of a wave's 4-row span hold rows at two different offsets. Bit-equal to the unsliced
    wide DBG launch (the oracle: the next test)."""
    meta, m, hp, sd = _model(name)
    steps = list(LOGIT_STEPS)
    m.set_debug_steps(steps)
    dev = _mels(6, 136)
    got = {}
    for sl in (True, False):
        out, plan, _, _ = _call(m, meta, dev, sl, monkeypatch, wide=not sl)
        assert len(plan) == (17 if sl else 2) and all(w for _, _, w in plan), plan
        got[sl] = np.stack([m.debug_logits(s, range(136)) for s in steps])
        assert got[sl].shape[:2] == (8, 136) and np.isfinite(got[sl]).all()
    d = np.argwhere(got[True].view(np.uint32) != got[False].view(np.uint32))
    assert len(d) == 0, f'{len(d)} logits differ, first (step index, row, class) {d[0].tolist()}'


@pytest.mark.parametrize('u', ORACLE_ROWS)
@pytest.mark.parametrize('name', HEADS)
def test_dbg_instance_logits_against_the_oracle(name, u, monkeypatch):
    """The sliced DBG launch's logits of an oracle row at LOGIT_STEPS (1024 for BITS, 30 for MOL, 2
    for Beta) within 1e-5 x max(1, |l|) of the oracle's at the same steps, one row a case. The
    oracle runs free from the same seed: its trajectory is the kernel's for BITS (bit-exact labels)
    and within 5e-8 RMS of it for MOL and Beta, so the logits of late steps carry that difference
    too. Measured: at most 7.5e-8 (BITS), 6.0e-8 (MOL), 4.3e-8 (Beta)."""
    from test_gpu_logits import LOGIT_ABS_TOL
    meta, m, hp, sd = _model(name)
    steps = list(LOGIT_STEPS)
    m.set_debug_steps(steps)
    out, plan, _, _ = _call(m, meta, _mels(6, 136), True, monkeypatch)
    assert len(plan) == 17 and all(w for _, _, w in plan), plan
    _, ref = _oracle(name, sd, hp, meta, 6, u)
    for s in steps:
        got = m.debug_logits(s, [u])[0].astype(np.float64)
        r = ref[s].reshape(-1).astype(np.float64)
        assert got.shape == r.shape == ({BITS: 1024, MOL: 30, BETA: 2}[name],)
        tol = LOGIT_ABS_TOL * max(1.0, float(np.abs(r).max()))
        err = float(np.abs(got - r).max())
        print(f'{name} utt {u} step {s}: max |dlogit| {err:.3g} (tol {tol:.3g})')
        assert err <= tol, f'{name} utt {u} step {s}: max logit error {err}'


def test_progress_and_abort(monkeypatch):
    """The callback sequence of a sliced call is i = 0, 100, .. < S, once each; a callback that
    raises aborts the call, and the handle's next call is whole."""
    meta, m, hp, sd = _model(BITS)
    dev = _mels(6, 136)
    calls = []
    got, plan, _, S = _call(m, meta, dev, True, monkeypatch, cb=lambda i, *a: calls.append(i))
    assert len(plan) == 17 and calls == list(range(0, 1200, 100)), calls

    class Stop(Exception):
        pass

    seen = []

    def cb(i, *a):
        seen.append(i)
        if i >= 200:
            raise Stop()
    with pytest.raises(Stop):
        _call(m, meta, dev, True, monkeypatch, cb=cb)
    assert seen == [0, 100, 200]
    again, plan, _, _ = _call(m, meta, dev, True, monkeypatch)
    assert len(plan) == 17
    _same(again, got, 'the call after an aborted one')


def test_setter_and_switches(monkeypatch):
    from test_gpu_parity import make_model
    _clean(monkeypatch)
    fmeta, _ = golden_case('fatchord_raw9_tiny')
    fm, _, _ = make_model(fmeta)
    with pytest.raises(ValueError):
        fm.set_wide_slices(True)
    fm.set_wide_slices(False)
    meta, m, hp, sd = _model(BITS)
    from wavernn_amd import _abi
    for bad in (2, -1, 16):
        assert m._lib.wrnn_set_gen_wide_slices(m._h, bad) == _abi.WRNN_ERR_INVALID
    dev = _mels(6, 136)
    mixed = MIXED

    def run():
        m.set_seed(meta['noise_seed'])
        m.generate_batch_device(dev, False, 0, 0)
        return sorted((nr, w) for _, nr, w in m.plan_info())
    assert run() == mixed  # off by default
    m.set_wide_slices(True)
    assert run() == [(16, True)] * 17
    # the env switch overrides the handle's setting, either way
    monkeypatch.setenv('WRNN_GEN_SLICE', '0')
    assert run() == mixed
    m.set_wide_slices(False)
    monkeypatch.setenv('WRNN_GEN_SLICE', '1')
    assert run() == [(16, True)] * 17
    # a time-sliced launch exists only as a ring instance; WRNN_PERSIST_SLICE=0 forbids it as well
    monkeypatch.setenv('WRNN_GEN_RING', '0')
    assert run() == mixed and m.stream_info()[0] > 0
    monkeypatch.delenv('WRNN_GEN_RING')
    monkeypatch.setenv('WRNN_PERSIST_SLICE', '0')
    assert run() == mixed
