"""Streaming sessions, the parts that need no GPU: the C ABI's refusals of null
arguments, the readiness rule (wrnn_debug_stream_ready: the function the runtime itself calls) and
the chunked f64 post-processing (audio.StreamPost) against the reference waveform of the unbatched
fixture. The device side is tests/test_gpu_stream.py."""
import ctypes

import numpy as np
import pytest

from conftest import golden_case, hparams_of

SPLITS = [[22], [1] * 22, [3, 19], [2, 1, 19], [5, 1, 7, 9], [21, 1], [22, 0]]


def _lib():
    from wavernn_amd import _abi
    return _abi, _abi.load_library()


def _ready(lib, frames, last, hop=200, la=2):
    out = ctypes.c_int64(-1)
    rc = lib.wrnn_debug_stream_ready(frames, last, hop, la, ctypes.byref(out))
    return rc, out.value


def test_every_entry_point_refuses_null_arguments():
    _abi, lib = _lib()
    inv = _abi.WRNN_ERR_INVALID
    s = ctypes.c_void_p()
    fr = ctypes.c_int()
    steps = ctypes.c_int64()
    mel = np.zeros((80, 2), np.float32)
    buf = np.zeros(8, np.float32)
    w = ctypes.c_int()
    fp = ctypes.POINTER(ctypes.c_float)
    ss = (ctypes.c_void_p * 1)(None)
    lab = (ctypes.c_void_p * 1)(None)
    cap = (ctypes.c_size_t * 1)(0)
    got = (ctypes.c_size_t * 1)(0)
    calls = {
        'open: null handle': lambda: lib.wrnn_stream_open(None, 10, ctypes.byref(s)),
        'open: null out': lambda: lib.wrnn_stream_open(None, 10, None),
        'push: null session': lambda: lib.wrnn_stream_push(None, mel.ctypes.data_as(fp), 2, 0),
        'advance: null list': lambda: lib.wrnn_stream_advance(None, 1, lab, cap, got),
        'advance: null session': lambda: lib.wrnn_stream_advance(ss, 1, lab, cap, got),
        'advance: null outputs': lambda: lib.wrnn_stream_advance(ss, 1, None, None, None),
        'advance: negative n': lambda: lib.wrnn_stream_advance(ss, -1, lab, cap, got),
        'status: null session': lambda: lib.wrnn_stream_status(None, ctypes.byref(fr), None, None, None, None),
        'ready: null out': lambda: lib.wrnn_debug_stream_ready(3, 0, 200, 2, None),
        'row: null session': lambda: lib.wrnn_debug_stream_row(None, 0, 0, buf.ctypes.data_as(fp), 8, ctypes.byref(w)),
        'frame row: null handle': lambda: lib.wrnn_debug_frame_row(None, 0, 0, buf.ctypes.data_as(fp), 8,
                                                                   ctypes.byref(w)),
    }
    for what, call in calls.items():
        assert call() == inv, what
        assert lib.wrnn_last_error(), what  # a message, not an empty string
    assert s.value is None
    lib.wrnn_stream_close(None)  # a no-op
    del steps


def test_ready_rule_values():
    _abi, lib = _lib()
    for frames, last, want in [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 200), (22, 0, 4000), (22, 1, 4400),
                               (0, 1, 0)]:
        assert _ready(lib, frames, last) == (0, want), (frames, last)
    for la in (0, 2, 5):
        vals = [_ready(lib, f, 0, la=la)[1] for f in range(60)]
        assert vals == sorted(vals) and vals[-1] == (59 - la) * 200
        assert all(_ready(lib, f, 1, la=la)[1] == f * 200 for f in range(60))  # the end frees everything
        assert all(_ready(lib, f, 1, la=la)[1] >= vals[f] for f in range(60))
    for bad in [(-1, 0, 200, 2), (3, 0, 0, 2), (3, 0, -200, 2), (3, 0, 200, -1)]:
        out = ctypes.c_int64()
        assert lib.wrnn_debug_stream_ready(*bad, ctypes.byref(out)) == _abi.WRNN_ERR_INVALID, bad


def _random_splits(total, seed, count):
    """Seeded splits of `total` frames into 1 .. total chunks (every chunk >= 1), plus all-ones."""
    rng = np.random.default_rng(seed)
    out = [[1] * total]
    for k in range(1, total + 1):
        for _ in range(count):
            cuts = np.sort(rng.choice(np.arange(1, total), size=k - 1, replace=False)) if k > 1 else np.array([], int)
            out.append(np.diff(np.concatenate([[0], cuts, [total]])).astype(int).tolist())
    return out


@pytest.mark.parametrize('la', [0, 2, 5])
def test_ready_increments_sum_to_the_utterance(la):
    _abi, lib = _lib()
    for split in _random_splits(22, 7 + la, 4):
        assert sum(split) == 22 and min(split) >= 1
        frames, done, incs = 0, 0, []
        for i, n in enumerate(split):
            frames += n
            r = _ready(lib, frames, int(i == len(split) - 1), la=la)[1]
            assert r >= done
            incs.append(r - done)
            done = r
        assert sum(incs) == 4400, split


def _label_counts(lib, split, la=2, hop=200):
    """Labels each push of `split` (frames; the last push ends the utterance) releases."""
    frames, done, out = 0, 0, []
    for i, n in enumerate(split):
        frames += n
        r = _ready(lib, frames, int(i == len(split) - 1), hop, la)[1]
        out.append(r - done)
        done = r
    return out


@pytest.mark.parametrize('split', SPLITS, ids=['-'.join(map(str, s)) for s in SPLITS])
@pytest.mark.parametrize('native', [False, True])
def test_stream_post_equals_the_reference_waveform(split, native):
    """The golden labels of the unbatched fixture, fed in the label chunks the frame splits
    release, give its waveform bit for bit; nothing from the fade / truncation region (the last
    21 hops of labels) leaves before the end."""
    from wavernn_amd.audio import StreamPost
    _abi, lib = _lib()
    meta, gold = golden_case('fatchord_raw10_unbatched_tiny')
    hp = hparams_of(meta)
    labels = gold['labels']
    assert labels.shape == (1, 4400) and gold['wav'].shape == (4200,)
    post = StreamPost(2 ** meta['bits'], 200, hp.mu_law, True, lib if native else None)
    counts = _label_counts(lib, split)
    assert sum(counts) == 4400
    chunks, pos = [], 0
    for c in counts:
        out = post.feed(labels[0, pos:pos + c])
        pos += c
        chunks.append(out)
        assert out.dtype == np.float64
        assert post.n_out <= max(0, pos - 21 * 200)  # final samples only
        assert post.n_out <= 4200 - 20 * 200          # none from inside the fade
    chunks.append(post.finish())
    wav = np.concatenate(chunks)
    assert wav.shape == gold['wav'].shape and np.array_equal(wav, gold['wav'])
    with pytest.raises(ValueError):
        post.feed(labels[0, :1])


def test_stream_post_short_utterance_fails_like_the_one_shot_path():
    """An utterance shorter than the 20-hop fade: numpy's broadcast error, as postprocess()."""
    from wavernn_amd.audio import StreamPost
    post = StreamPost(512, 200, True, True, None)
    assert post.feed(np.zeros(600, np.int16)).size == 0
    with pytest.raises(ValueError):
        post.finish()
