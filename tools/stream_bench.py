"""Latency of the streaming sessions (wrnn_stream_*) on one MI355X.

A 1000-frame seeded mel through default-init fatchord 9-bit weights, pushed in chunks of 4, 16, 64
and 1000 frames into 1 and into 8 sessions (advanced together), after one warm-up session. Per
configuration, as one JSON line:

* first_audio_ms : first push -> end of the first advance that returned labels;
* per advance    : its time (push of every session's chunk + the advance) against the duration of
                   the audio it produced per session (steps / sample_rate): median and worst ratio,
                   and how many advances took longer than their audio lasts;
* total_ms       : the whole utterance(s).

Then `generate_rows(batched=False)` of the same mel -- the parent's path, unchanged -- against one
session fed the whole mel in one push and in 64-frame chunks, alternated three times in this run.
No rate is assumed in advance; the tool reports what it measures.

usage: python tools/stream_bench.py [--out DIR] [--frames 1000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'real-time-voice-cloning_amd'))
sys.path.insert(0, REPO)


def make_model(bits):
    from wavernn_amd.hparams import sp, wavernn_fatchord
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synth import synth_state_dict
    hp = wavernn_fatchord.copy(bits=bits, mode='RAW')
    mt = 'fatchord-wavernn'
    m = WaveRNN(hp.rnn_dims, hp.fc_dims, hp.bits, hp.pad, hp.upsample_factors, sp.num_mels, hp.compute_dims,
                hp.res_out_dims, hp.res_blocks, sp.hop_size, sp.sample_rate, mode=hp.mode, model_type=mt, device=0)
    m.load_state_dict(synth_state_dict(hp, mt, seed=1))
    m.set_seed(101)
    return m, sp


def run_streams(m, mel, chunk, n_sessions, rate):
    """One streamed run; returns (labels of session 0, record)."""
    T = mel.shape[1]
    ss = [m.open_stream(T, stream=u) for u in range(n_sessions)]
    out, adv = [], []
    first = None
    t_begin = time.perf_counter()
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        t0 = time.perf_counter()
        for s in ss:
            s.push_frames(mel[:, a:b], last=b == T)
        t1 = time.perf_counter()
        labs = m.advance_streams(ss)
        t2 = time.perf_counter()
        n = len(labs[0])
        out.append(labs[0])
        if n:
            if first is None:
                first = t2 - t_begin
            adv.append(dict(push_ms=(t1 - t0) * 1e3, advance_ms=(t2 - t1) * 1e3, steps=n, audio_ms=n / rate * 1e3))
    total = time.perf_counter() - t_begin
    for s in ss:
        s.close()
    ratios = [(x['push_ms'] + x['advance_ms']) / x['audio_ms'] for x in adv]
    steady = adv[1:-1] or adv  # (without the first advance and the tail flush)
    rec = dict(kind='stream', sessions=n_sessions, chunk_frames=chunk, frames=T, advances=len(adv),
               first_audio_ms=round(first * 1e3, 3), total_ms=round(total * 1e3, 3),
               audio_ms=round(T * m.hop_length / rate * 1e3, 1),
               ratio_median=round(statistics.median(ratios), 4), ratio_max=round(max(ratios), 4),
               slower_than_audio=sum(r > 1.0 for r in ratios),
               push_ms_median=round(statistics.median(x['push_ms'] for x in steady), 4),
               advance_ms_median=round(statistics.median(x['advance_ms'] for x in steady), 4),
               us_per_step_median=round(statistics.median(x['advance_ms'] * 1e3 / x['steps'] for x in steady), 4))
    return np.concatenate(out), rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='directory for stream.jsonl')
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--bits', type=int, default=9)
    args = ap.parse_args()
    from wavernn_amd.synth import synth_mel
    m, sp = make_model(args.bits)
    rate = float(sp.sample_rate)
    mel = (synth_mel(args.frames, 11) / sp.max_abs_value).astype(np.float32)
    recs = []

    def emit(r):
        recs.append(r)
        print(json.dumps(r), flush=True)

    run_streams(m, mel[:, :64], 16, 1, rate)  # warm-up session (kernel load, allocations)
    m.set_stream(0)
    ref, _, _, S = m.generate_rows(mel, False, 0, 0)  # (also the one-shot path's warm-up)
    for n_sessions in (1, 8):
        for chunk in (4, 16, 64, args.frames):
            lab, rec = run_streams(m, mel, chunk, n_sessions, rate)
            rec['equal_one_shot'] = bool(np.array_equal(lab, ref[0]))
            emit(rec)
    for rep in range(3):
        m.set_stream(0)
        t0 = time.perf_counter()
        m.generate_rows(mel, False, 0, 0)
        t1 = time.perf_counter()
        emit(dict(kind='one_shot', rep=rep, total_ms=round((t1 - t0) * 1e3, 3), steps=S))
        for chunk in (args.frames, 64):
            _, rec = run_streams(m, mel, chunk, 1, rate)
            emit(dict(kind='stream_total', rep=rep, chunk_frames=chunk, total_ms=rec['total_ms'],
                      first_audio_ms=rec['first_audio_ms']))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'stream.jsonl'), 'w') as f:
            for r in recs:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
