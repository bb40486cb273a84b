"""Launch plan of the persistent engine (plan.cpp plan_call, on the inputs runtime.hip plan_inputs reads from
the handle and the device: cost-minimising sequence of register-resident and wide launches) on the BASELINE shapes, read back through wrnn_plan_info.

A regression here costs throughput, not correctness, so the parity tests would not notice it:
in round 2 the runtimeracer / geneing plan took 4 rows per group for 18 rows (one launch,
padded to 32 slots, 12-17 % slower) until the plan costed every variant."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(model_type, mode, bits, n_utts, frames=1000, target=11000, overlap=550):
    import torch
    from wavernn_amd.base import hparams_for
    from wavernn_amd.hparams import sp
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synth import synth_mel, synth_state_dict
    hp = hparams_for(model_type).copy(bits=bits, mode=mode)
    m = WaveRNN(hp.rnn_dims, hp.fc_dims, hp.bits, hp.pad, hp.upsample_factors, sp.num_mels,
                hp.compute_dims, hp.res_out_dims, hp.res_blocks, sp.hop_size, sp.sample_rate,
                mode=hp.mode, model_type=model_type, device=0)
    m.load_state_dict(synth_state_dict(hp, model_type, seed=0))
    mels = [torch.from_numpy((synth_mel(frames, u) / sp.max_abs_value).astype(np.float32)).cuda()
            for u in range(n_utts)]
    m.generate_batch_device(mels, True, target, overlap)
    assert m.last_engine() == 'persist'
    return m.plan_info()


def test_c2_shape_geneing_is_rotated_over_three_launches(monkeypatch):
    """geneing 10-bit at C2 (18 rows): the rotated k_persist_gen, three launches
    of 3 / 2 rows per group; WRNN_PERSIST_ROT=0 restores the single 3-row launch."""
    assert _run('geneing-wavernn', 'BITS', 10, 1) == [(0, 3, False)] * 3
    monkeypatch.setenv('WRNN_PERSIST_ROT', '0')
    assert _run('geneing-wavernn', 'BITS', 10, 1) == [(0, 3, False)]


def test_c2_shape_runtimeracer_is_rotated_over_three_launches(monkeypatch):
    """runtimeracer 9-bit at C2 (18 rows): the rotated k_persist_rr, three
    launches of 3 / 2 rows per group; WRNN_PERSIST_ROT=0 restores the single 3-row launch."""
    assert _run('runtimeracer-wavernn', 'RAW', 9, 1) == [(0, 3, False)] * 3
    monkeypatch.setenv('WRNN_PERSIST_ROT', '0')
    assert _run('runtimeracer-wavernn', 'RAW', 9, 1) == [(0, 3, False)]


@pytest.mark.parametrize('mode', ['RAW', 'MOL'])
def test_c2_fatchord_is_rotated_over_three_launches(mode, monkeypatch):
    """fatchord 9-bit at C2 (18 rows: 2 groups of 3 rows, 6 of 2): the row rotation (DESIGN.md
    §3.0e) -- three launches, every row 3,706 steps in a 3-row group and 2 x 4,197 in 2-row
    groups; WRNN_PERSIST_ROT=0 restores the single launch."""
    assert _run('fatchord-wavernn', mode, 9, 1) == [(0, 3, False)] * 3
    monkeypatch.setenv('WRNN_PERSIST_ROT', '0')
    assert _run('fatchord-wavernn', mode, 9, 1) == [(0, 3, False)]


def test_c4_shape_is_time_sliced_over_wide_launches(monkeypatch):
    """C4 per GPU (144 rows, 18 per group): time-sliced wide launches -- 9 of
    16 rows per group x 1,512 steps, then the last 4 steps in launches of 16 and 2 rows per
    group; WRNN_PERSIST_SLICE=0 restores one wide launch of 128 rows + one register-resident
    launch of 2 rows per group."""
    plan = _run('fatchord-wavernn', 'RAW', 9, 8)
    assert plan == [(0, 16, True)] * 10 + [(0, 2, True)], plan
    monkeypatch.setenv('WRNN_PERSIST_SLICE', '0')
    plan = _run('fatchord-wavernn', 'RAW', 9, 8)
    assert sorted((nr, wide) for _, nr, wide in plan) == [(2, False), (16, True)]
    assert sum(8 * nr for _, nr, _ in plan) == 144


def test_fatchord_10bit_default_batch_is_time_sliced_over_wide_launches():
    """The fork's fatchord default (10 bits, target 3,000 / overlap 1,500: 45 rows per 1000-frame
    utterance) at 8 utterances: 360 rows, 45 per group -- 45 time-sliced wide launches of 16 rows
    per group x 375 steps on the 1024-class instances (VERDICT r4 missing #3), no
    register-resident launch."""
    plan = _run('fatchord-wavernn', 'RAW', 10, 8, target=3000, overlap=1500)
    assert plan == [(0, 16, True)] * 45, plan


def test_runtimeracer_default_batch_is_time_sliced_over_wide_launches():
    """runtimeracer 10-bit defaults (target 6,000 / overlap 1,000) at 8 x 1000 frames: 232 rows,
    29 per group -- 29 time-sliced wide launches (kernels_persist_wide_rr.hip) of 16 rows per
    group x 500 steps instead of a 16-row and a 13-row launch of 8,000 steps each."""
    plan = _run('runtimeracer-wavernn', 'RAW', 10, 8, target=6000, overlap=1000)
    assert plan == [(0, 16, True)] * 29, plan


def test_fatchord_10bit_single_utterance_default_is_one_wide_launch():
    """The fork's fatchord default on one 1000-frame mel (10 bits, 3000 / 1500: 45 rows x 6,000
    steps, VERDICT r5 missing #2): one wide launch of 6 rows per group -- measured 10.6 us per
    step, 3.04 M samples/s, against two register-resident launches of 3 rows per group (13.0 us
    per step of S, 2.43 M) and the other row counts (profiles/r06/b u10*.log)."""
    plan = _run('fatchord-wavernn', 'RAW', 10, 1, target=3000, overlap=1500)
    assert plan == [(0, 6, True)], plan


def test_pruned_c2_plans_by_measured_rates(monkeypatch):
    """90 %-pruned weights at C2: the sparse image exists, but the dense rotated launches are
    faster on MI355X (5.4 against 7.4 us per step), so the planner keeps them;
    WRNN_SPARSE=1 runs the sparse instances on the same rotated plan."""
    import torch
    from wavernn_amd.base import hparams_for
    from wavernn_amd.hparams import sp
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.prune import prune_state_dict
    from wavernn_amd.synth import synth_mel, synth_state_dict
    mt = 'fatchord-wavernn'
    hp = hparams_for(mt).copy(bits=9)
    m = WaveRNN(hp.rnn_dims, hp.fc_dims, hp.bits, hp.pad, hp.upsample_factors, sp.num_mels,
                hp.compute_dims, hp.res_out_dims, hp.res_blocks, sp.hop_size, sp.sample_rate,
                mode=hp.mode, model_type=mt, device=0)
    m.load_state_dict(prune_state_dict(synth_state_dict(hp, mt, seed=0), mt, z=0.9))
    mel = [torch.from_numpy((synth_mel(1000, 0) / sp.max_abs_value).astype(np.float32)).cuda()]
    m.generate_batch_device(mel, True, 11000, 550)
    assert m.sparse_info()['available'] and not m.sparse_info()['last_call']
    assert m.plan_info() == [(0, 3, False)] * 3
    monkeypatch.setenv('WRNN_SPARSE', '1')
    m.generate_batch_device(mel, True, 11000, 550)
    assert m.sparse_info()['last_call'] and m.plan_info() == [(0, 3, False)] * 3


def test_rate_table_beside_the_library_is_loaded_and_overridable(tmp_path, monkeypatch):
    """The handle plans with rates_mi355x.txt beside the library (the per-build table the
    measurement pass emits); WRNN_RATES names another file, set_rates overrides
    keys per handle -- and the plan follows: C2 with 3 rows per group made expensive runs one
    launch of 4 rows per group."""
    import os
    from wavernn_amd import _abi
    beside = os.path.join(os.path.dirname(_abi.LIB_PATH), 'rates_mi355x.txt')
    assert os.path.exists(beside)
    import torch
    from wavernn_amd.base import hparams_for
    from wavernn_amd.hparams import sp
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synth import synth_mel, synth_state_dict
    mt = 'fatchord-wavernn'
    hp = hparams_for(mt).copy(bits=9)

    def model():
        m = WaveRNN(hp.rnn_dims, hp.fc_dims, hp.bits, hp.pad, hp.upsample_factors, sp.num_mels,
                    hp.compute_dims, hp.res_out_dims, hp.res_blocks, sp.hop_size, sp.sample_rate,
                    mode=hp.mode, model_type=mt, device=0)
        m.load_state_dict(synth_state_dict(hp, mt, seed=0))
        return m
    mel = [torch.from_numpy((synth_mel(1000, 0) / sp.max_abs_value).astype(np.float32)).cuda()]
    m = model()
    assert m.rates().splitlines()[0] == '# source: ' + beside
    m.generate_batch_device(mel, True, 11000, 550)
    assert m.plan_info() == [(0, 3, False)] * 3
    m.set_rates('fat9 4.8 5.15 50 6.92')
    m.generate_batch_device(mel, True, 11000, 550)
    assert m.plan_info() == [(0, 4, False)]
    f = tmp_path / 'rates.txt'
    f.write_text('fat9 4.8 5.15 50 6.92\n')
    monkeypatch.setenv('WRNN_RATES', str(f))
    m2 = model()
    assert m2.rates().splitlines()[0] == '# source: ' + str(f)
    m2.generate_batch_device(mel, True, 11000, 550)
    assert m2.plan_info() == [(0, 4, False)]
