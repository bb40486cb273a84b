"""Streaming sessions on the GPU (wrnn_stream_*): however the mel is cut into
pushes, a session's labels equal the unbatched one-shot call's bit for bit -- against the
reference's own labels (fixture fatchord_raw10_unbatched_tiny) and the oracle restatement pinned
to it (tests/test_oracle_golden.py). Default-init fixtures: the GPU path is bit-exact on them, so
no near-tie allowance applies. Every case is a few thousand steps."""
import ctypes

import numpy as np
import pytest

from conftest import golden_case
from test_gpu_parity import first_divergence, make_model

pytestmark = pytest.mark.gpu

HOP = 200
UNB = 'fatchord_raw10_unbatched_tiny'
# (frames per push, ...); the last push ends the utterance, except the final case: all 22 frames,
# then an empty last push. [2, 1, 19] and [1] * 22 put chunk ends on the first ready step and on
# every hop boundary.
SPLITS = [[22], [1] * 22, [3, 19], [2, 1, 19], [5, 1, 7, 9], [21, 1], [22, 0]]

_ORACLE = {}


def _mel(frames, seed):
    from wavernn_amd.hparams import sp
    from wavernn_amd.synth import synth_mel
    raw = synth_mel(frames, seed)
    return raw, (raw / sp.max_abs_value).astype(np.float32)


def _oracle(case, frames, mel_seed, stream):
    """The oracle's unbatched labels (S,) for the case's weights and seed; computed once."""
    key = (case, frames, mel_seed, stream)
    if key not in _ORACLE:
        from conftest import hparams_of, state_dict_of
        from oracle.wavernn_oracle import oracle_infer_waveform
        meta, _ = golden_case(case)
        raw, _ = _mel(frames, mel_seed)
        _ORACLE[key] = oracle_infer_waveform(state_dict_of(meta), hparams_of(meta), meta['model_type'], raw,
                                             target=meta['target'], overlap=meta['overlap'],
                                             seed=meta['noise_seed'], stream=stream, batched=False,
                                             post=False)['labels'][0].copy()
    return _ORACLE[key]


def _ready(frames, last, la=2):
    return frames * HOP if last else max(0, frames - la) * HOP


def _stream_split(m, mel, split, stream):
    """Push `mel` in the split's chunks; after every push the count equals the readiness rule."""
    s = m.open_stream(mel.shape[1], stream=stream)
    assert s.info()['lookahead'] == 2
    out, pos, done = [], 0, 0
    for i, n in enumerate(split):
        last = i == len(split) - 1
        lab = s.push(mel[:, pos:pos + n] if n else None, last=last)
        pos += n
        assert lab.dtype == np.int16 and len(lab) == _ready(pos, last) - done, (split, i, len(lab))
        done += len(lab)
        info = s.info()
        assert (info['frames'], info['ended'], info['steps_done'], info['steps_ready']) == (pos, last, done, done)
        out.append(lab)
    s.close()
    return np.concatenate(out)


@pytest.fixture(scope='module')
def unb():
    meta, gold = golden_case(UNB)
    m, hp, sd = make_model(meta)
    return meta, gold, m, hp, sd


@pytest.mark.parametrize('split', SPLITS, ids=['-'.join(map(str, s)) for s in SPLITS])
def test_one_session_equals_the_reference(unb, split):
    meta, gold, m, hp, sd = unb
    _, mel = _mel(meta['n_frames'], meta['mel_seed'])
    m.set_seed(meta['noise_seed'])
    lab = _stream_split(m, mel, split, meta['stream'])
    assert lab.shape == (4400,)
    assert np.array_equal(lab, gold['labels'][0]), first_divergence(lab[None], gold['labels'])


def test_infer_waveform_stream_equals_the_reference_waveform():
    from conftest import state_dict_of
    from wavernn_amd import inference
    from wavernn_amd.synth import synth_mel
    meta, gold = golden_case(UNB)
    inference.load_model(None, verbose=False, state_dict=state_dict_of(meta), model_type=meta['model_type'])
    inference.set_seed(meta['noise_seed'])
    mel = synth_mel(meta['n_frames'], meta['mel_seed'])
    for split in ([5, 1, 7, 9], [22]):
        inference.set_seed(meta['noise_seed'])  # (stream 0 again)
        cuts = np.cumsum([0] + split)
        chunks = list(inference.infer_waveform_stream(mel[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])))
        wav = np.concatenate(chunks)
        assert wav.dtype == np.float64 and wav.shape == gold['wav'].shape
        assert np.array_equal(wav, gold['wav'])
    inference.set_seed(meta['noise_seed'])
    one = inference.infer_waveform(mel, batched=False, progress_callback=lambda *a: None)
    assert np.array_equal(one, gold['wav'])


@pytest.fixture(scope='module')
def nine():
    meta, _ = golden_case('fatchord_raw9_tiny')
    m, hp, sd = make_model(meta)
    return meta, m


def test_nine_bits_against_the_oracle(nine):
    """512 classes: the 16-classes-per-slot streaming instance."""
    meta, m = nine
    _, mel = _mel(6, 41)
    m.set_seed(meta['noise_seed'])
    lab = _stream_split(m, mel, [3, 1, 2], 3)
    ref = _oracle('fatchord_raw9_tiny', 6, 41, 3)
    assert np.array_equal(lab, ref), first_divergence(lab[None], ref[None])


def test_table_rows_equal_the_one_shot_call(unb):
    """p1q / p1a / fcond rows of a session pushed as [5, 1, 7, 9] against the rows the one-shot
    call computed for the whole mel, bit for bit (NaN marks a row that was never written)."""
    meta, gold, m, hp, sd = unb
    _, mel = _mel(meta['n_frames'], meta['mel_seed'])
    frames = [-1, 0, 2, 3, 4, 5, 12, 20, 21]
    m.set_seed(meta['noise_seed'])
    m.set_engine('persist')
    m.generate_rows(mel, False, 0, 0)
    m.set_engine('auto')
    ref = {(f, t): m.debug_frame_row(f, t) for f in frames for t in range(3)}
    s = m.open_stream(22, stream=0)
    pos = 0
    for i, n in enumerate([5, 1, 7, 9]):
        s.push(mel[:, pos:pos + n], last=i == 3)
        pos += n
    for (f, t), want in ref.items():
        got = s.debug_row(f, t)
        assert got.shape == want.shape and not np.isnan(want).any()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (f, t)
    s.close()
    # before the end, a row behind the pushed frames is still NaN (p1a needs frame + pad)
    s = m.open_stream(22, stream=0)
    s.push(mel[:, :6])
    assert not np.isnan(s.debug_row(5, 0)).any() and np.isnan(s.debug_row(5, 1)).all()
    assert np.isnan(s.debug_row(6, 0)).all()
    s.close()


def test_three_sessions_interleaved(nine):
    """Mels of 22, 9 and 6 frames on streams 5, 6, 7, advanced together: one advance has a
    session with nothing ready and groups of different step counts, a later one a session that
    has already ended."""
    meta, m = nine
    spec = [(22, 51, 5), (9, 52, 6), (6, 53, 7)]
    mels = [_mel(T, sd)[1] for T, sd, _ in spec]
    m.set_seed(meta['noise_seed'])
    ss = [m.open_stream(T, stream=st) for T, _, st in spec]
    got = [[], [], []]
    rounds = [[(0, 5, False), (0, 2, False), (0, 6, True)],      # 600, 0, 1200 steps
              [(5, 15, False), (2, 9, True), None],              # 2000, 1800, ended
              [(15, 22, True), None, None]]                      # 1800, -, -
    want = [[600, 0, 1200], [2000, 1800, 0], [1800, 0, 0]]
    for r, pushes in enumerate(rounds):
        for i, p in enumerate(pushes):
            if p is not None:
                ss[i].push_frames(mels[i][:, p[0]:p[1]], last=p[2])
        labs = m.advance_streams(ss)
        assert [len(x) for x in labs] == want[r], r
        for i in range(3):
            got[i].append(labs[i])
    for i, (T, sd, st) in enumerate(spec):
        lab = np.concatenate(got[i])
        ref = _oracle('fatchord_raw9_tiny', T, sd, st)
        assert lab.shape == ref.shape and np.array_equal(lab, ref), (i, first_divergence(lab[None], ref[None]))
        info = ss[i].info()
        assert info['ended'] and info['steps_done'] == T * HOP
        ss[i].close()


def test_eight_sessions_equal_the_unbatched_batch_call(nine):
    import torch
    meta, m = nine
    _, mel = _mel(6, 41)
    m.set_seed(meta['noise_seed'])
    dev = [torch.from_numpy(mel).cuda() for _ in range(8)]
    ref, roff, S = m.generate_batch_device(dev, False, 0, 0, streams=list(range(8)))
    ref = ref.cpu().numpy()
    assert ref.shape == (8, 1200)
    ss = [m.open_stream(6, stream=u) for u in range(8)]
    out = [[] for _ in range(8)]
    for a, b, last in [(0, 4, False), (4, 6, True)]:
        for s in ss:
            s.push_frames(mel[:, a:b], last=last)
        for u, lab in enumerate(m.advance_streams(ss)):
            assert len(lab) == (1200 if last else 400) - sum(len(x) for x in out[u])
            out[u].append(lab)
    for u in range(8):
        lab = np.concatenate(out[u])
        assert np.array_equal(lab, ref[u]), (u, first_divergence(lab[None], ref[u][None]))
        ss[u].close()
    assert len({ref[u].tobytes() for u in range(8)}) == 8  # the streams do differ


def test_handle_reuse_between_pushes():
    """Half-way through a session a batched generate_rows of fatchord_raw10_defaults on the same
    handle equals its golden labels; the session then runs to its end unharmed. (One handle holds
    one set of weights, so the session runs the defaults fixture's weights and is held against the
    oracle's unbatched labels for them.)"""
    name = 'fatchord_raw10_defaults'
    meta, gold = golden_case(name)
    m, hp, sd = make_model(meta)
    _, mel6 = _mel(6, 41)
    _, mel = _mel(meta['n_frames'], meta['mel_seed'])
    m.set_seed(meta['noise_seed'])
    s = m.open_stream(6, stream=9)
    first = s.push(mel6[:, :3])
    assert len(first) == 200
    m.set_stream(meta['stream'])
    labels, _, B, S = m.generate_rows(mel, True, meta['target'], meta['overlap'])
    assert np.array_equal(labels, gold['labels'])
    rest = s.push(mel6[:, 3:], last=True)
    lab = np.concatenate([first, rest])
    ref = _oracle(name, 6, 41, 9)
    assert np.array_equal(lab, ref), first_divergence(lab[None], ref[None])
    s.close()


def test_refusals_on_the_device(nine):
    from wavernn_amd import _abi
    meta, m = nine
    lib = m._lib
    _, mel = _mel(6, 41)
    ref = _oracle('fatchord_raw9_tiny', 6, 41, 3)
    m.set_seed(meta['noise_seed'])
    s = m.open_stream(6, stream=3)
    a = s.push(mel[:, :4])
    with pytest.raises(BufferError):  # 4 + 3 > max_frames: WRNN_ERR_CAPACITY, nothing changes
        s.push_frames(mel[:, 3:6])
    assert s.info()['frames'] == 4
    # too small a capacity: WRNN_ERR_CAPACITY and nothing ran
    s.push_frames(mel[:, 4:], last=True)
    before = s.info()
    need = before['steps_ready'] - before['steps_done']
    assert need == 800
    small = np.full(need, -1, np.int16)
    ss = (ctypes.c_void_p * 1)(s._s)
    ptr = (ctypes.c_void_p * 1)(small.ctypes.data)
    cap = (ctypes.c_size_t * 1)(need - 1)
    got = (ctypes.c_size_t * 1)(7)
    assert lib.wrnn_stream_advance(ss, 1, ptr, cap, got) == _abi.WRNN_ERR_CAPACITY
    assert s.info() == before and (small == -1).all()
    b = m.advance_streams([s])[0]
    assert np.array_equal(np.concatenate([a, b]), ref)  # the session completes correctly
    with pytest.raises(ValueError):  # push after the last frames
        s.push_frames(mel[:, :1])
    # a 9th session, a duplicate, sessions of two handles
    more = [m.open_stream(2) for _ in range(8)]
    with pytest.raises(ValueError):
        m.advance_streams(more + [s])
    with pytest.raises(ValueError):
        m.advance_streams([more[0], more[1], more[0]])
    m2, _, _ = make_model(meta)
    other = m2.open_stream(2)
    with pytest.raises(ValueError):
        m.advance_streams([more[0], other])
    assert [len(x) for x in m.advance_streams(more)] == [0] * 8  # nothing ready: no launch, no error
    for x in more + [other, s]:
        x.close()


@pytest.mark.parametrize('case', ['runtimeracer_raw9_tiny', 'geneing_bits9_defaults', 'fatchord_mol_tiny',
                                  'chain'])
def test_open_is_refused_outside_the_scope(case):
    meta, _ = golden_case('fatchord_raw9_tiny' if case == 'chain' else case)
    m, hp, sd = make_model(meta)
    if case == 'chain':
        m.set_engine('chain')
    with pytest.raises(ValueError):
        m.open_stream(8)
    assert m.get_stream() == 0  # a refused open takes no stream id
