"""Host side of the block-sparse wide image (csrc/sparse_wide_pack.{h,cpp}, DESIGN.md §3.0g "the
wide form"): the packer that turns a pruned fatchord model's step matrices into per-slot lists of
live 1 x 4 blocks, through its handle-free entry points -- no device.

* wrnn_debug_wide_sp_pack on seeded matrices pruned by wavernn_amd.prune (the reference Pruner's
  mask, vocoder/pruner.py:60-88) at 0.9, the shapes of the step matrices (1536 x 512 gate
  matrices, 512 x 512 layers, the 1024 x 512 fc3 of 10 bits), every slot: each row's list size is
  its live-block count, and the densified lists give the matrix back -- live blocks bit for bit,
  dead blocks as +0.0 (the Pruner's mask product leaves -0.0 words where the weight was negative:
  a block of those is dead, so the reconstruction equals the matrix as values there);
* the fit rule (wrnn_debug_wide_sp_image): a model pruned at 0.9 fits the kernel's LDS carve, one
  pruned at 0.5 gets no image;
* the eight kernel instances of the built library use no scratch and spill no VGPR;
* `make wide_sp_check`: the packer and the planner's use of the image as a stand-alone program
  under AddressSanitizer + UndefinedBehaviorSanitizer.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG

CSRC = os.path.join(PKG, 'csrc')
F32P = ctypes.POINTER(ctypes.c_float)


def _ptr(a):
    return a.ctypes.data_as(F32P)


def pack(W, slot):
    """(reconstruction [16 rows / 512][cols], list sizes, total blocks) of one slot"""
    from wavernn_amd import _abi
    lib = _abi.load_library()
    W = np.ascontiguousarray(W, dtype=np.float32)
    nr = 16 * (W.shape[0] // 512)
    rec = np.full((nr, W.shape[1]), np.nan, np.float32)
    sizes = np.full(nr, -1, np.int32)
    tot = ctypes.c_int(-1)
    _abi.check(lib.wrnn_debug_wide_sp_pack(_ptr(W), W.shape[0], W.shape[1], slot, _ptr(rec),
                                           sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(tot)))
    return rec, sizes, tot.value


def slot_rows(W, slot):
    return np.concatenate([np.arange(k * 512 + 16 * slot, k * 512 + 16 * slot + 16) for k in range(W.shape[0] // 512)])


def live_mask(W):
    """[rows][cols / 4]: a block is live unless its four words are +0.0 or -0.0"""
    bits = np.ascontiguousarray(W, dtype=np.float32).view(np.uint32).reshape(W.shape[0], -1, 4)
    return ((bits & 0x7fffffff) != 0).any(axis=2)


def check_slot(W, slot):
    rec, sizes, tot = pack(W, slot)
    src = W[slot_rows(W, slot)]
    live = live_mask(src)
    assert np.array_equal(sizes, live.sum(axis=1)), slot
    assert tot == int(live.sum()), slot
    full = np.repeat(live, 4, axis=1)
    rb, sb = rec.view(np.uint32), np.ascontiguousarray(src).view(np.uint32)
    assert np.array_equal(rb[full], sb[full]), slot  # live blocks: bit for bit
    assert not rb[~full].any(), slot  # dead blocks: +0.0
    assert np.array_equal(rec, src), slot  # the matrix as values (-0.0 == +0.0)


@pytest.fixture(scope='module')
def pruned():
    """seeded matrices of the step matrices' shapes, pruned at 0.9 as the reference would"""
    from wavernn_amd.prune import mask_from_matrix
    rng = np.random.default_rng(20240611)
    out = {}
    for rows, splits in ((1536, 3), (512, 1), (1024, 1)):
        W = rng.standard_normal((rows, 512)).astype(np.float32)
        out[rows] = np.ascontiguousarray(W * mask_from_matrix(W, 0.9, 4, splits).numpy())
    return out


@pytest.mark.parametrize('rows', [1536, 512, 1024])
def test_lists_of_a_pruned_matrix_rebuild_it(pruned, rows):
    W = pruned[rows]
    live = live_mask(W)
    assert 0.099 < live.mean() < 0.101, live.mean()
    assert np.signbit(W[~np.repeat(live, 4, axis=1)]).any()  # (the mask product's -0.0 words are there)
    for slot in range(32):
        check_slot(W, slot)


def test_a_block_of_negative_zeros_is_dead_and_special_words_are_kept():
    W = np.zeros((512, 512), np.float32)
    W[16, 0:4] = -0.0                      # dead
    W[16, 4:8] = [-0.0, 0.0, 0.0, 1.5]     # live: one value
    W[16, 8] = np.float32(1e-45)           # live: a denormal
    W[16, 12] = np.nan                     # live: a NaN (the dense kernels multiply it too)
    W[17, 508:512] = [1, 2, 3, 4]          # the last block of a row
    rec, sizes, tot = pack(W, 1)
    assert list(sizes[:2]) == [3, 1] and tot == 4 and not sizes[2:].any()
    assert np.array_equal(rec.view(np.uint32)[0, 4:16], W.view(np.uint32)[16, 4:16])
    assert not rec.view(np.uint32)[0, 0:4].any()
    assert np.array_equal(rec[1], W[17])
    for slot in (0, 2, 31):
        assert pack(W, slot)[2] == 0


def test_a_fully_live_row_is_kept_exactly(pruned):
    rng = np.random.default_rng(7)
    W = pruned[1536].copy()
    W[512 + 16 * 5 + 3] = rng.standard_normal(512).astype(np.float32) + 4.0  # slot 5, gate z, row 3
    W[16 * 5 + 4] = 0.0                                                      # and an empty row beside it
    rec, sizes, _ = pack(W, 5)
    assert sizes[16 + 3] == 128 and sizes[4] == 0
    check_slot(W, 5)
    dense = rng.standard_normal((512, 512)).astype(np.float32) + 4.0         # a full slot
    assert pack(dense, 9)[2] == 16 * 128
    check_slot(dense, 9)
    check_slot(np.zeros((1024, 512), np.float32), 0)                         # an empty one


def test_bad_arguments_are_refused():
    W = np.zeros((512, 512), np.float32)
    for shape, slot in (((511, 512), 0), ((2048, 512), 0), ((512, 510), 0), ((512, 516), 0), ((512, 512), 32),
                        ((512, 512), -1)):
        with pytest.raises(ValueError):
            pack(np.zeros(shape, np.float32), slot)
    from wavernn_amd import _abi
    assert _abi.load_library().wrnn_debug_wide_sp_pack(None, 512, 512, 0, None, None, None) == _abi.WRNN_ERR_INVALID
    assert pack(W, 0)[2] == 0


def image_of(sd):
    from wavernn_amd import _abi
    lib = _abi.load_library()
    m = {k: np.ascontiguousarray(np.asarray(sd[k], dtype=np.float32)) for k in
         ('rnn2.weight_ih_l0', 'rnn1.weight_hh_l0', 'rnn2.weight_hh_l0', 'fc1.weight', 'fc2.weight', 'fc3.weight')}
    assert m['rnn1.weight_hh_l0'].shape == m['rnn2.weight_hh_l0'].shape == (1536, 512)
    fits, fill, dens = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_double(-1)
    _abi.check(lib.wrnn_debug_wide_sp_image(
        _ptr(m['rnn2.weight_ih_l0']), m['rnn2.weight_ih_l0'].shape[1], _ptr(m['rnn1.weight_hh_l0']),
        _ptr(m['rnn2.weight_hh_l0']), _ptr(m['fc1.weight']), m['fc1.weight'].shape[1], _ptr(m['fc2.weight']),
        m['fc2.weight'].shape[1], _ptr(m['fc3.weight']), m['fc3.weight'].shape[0], ctypes.byref(fits),
        ctypes.byref(dens), ctypes.byref(fill)))
    # the live fraction of the x / h parts the image packs
    live = total = 0
    for k, W in m.items():
        lm = live_mask(W[:, :512])
        live, total = live + int(lm.sum()), total + lm.size
    assert dens.value == pytest.approx(live / total, abs=1e-12)
    return bool(fits.value), dens.value, fill.value


@pytest.mark.parametrize('bits', [9, 10])
def test_fit_rule(bits):
    from wavernn_amd.hparams import wavernn_fatchord
    from wavernn_amd.prune import prune_state_dict
    from wavernn_amd.synth import synth_state_dict
    hp = wavernn_fatchord.copy(bits=bits, mode='RAW')
    sd = synth_state_dict(hp, 'fatchord-wavernn', seed=5)
    fits, dens, fill = image_of(prune_state_dict(sd, 'fatchord-wavernn', z=0.9))
    # (the Pruner masks whole matrices, aux columns included: the x parts are near 10 %, not at it)
    assert fits and 0.05 < dens < 0.15 and 0 < fill <= 4096, (fits, dens, fill)
    fits, dens, fill = image_of(prune_state_dict(sd, 'fatchord-wavernn', z=0.5))
    assert not fits and 0.4 < dens < 0.6, (fits, dens, fill)
    fits, dens, fill = image_of(sd)
    assert not fits and dens > 0.99, (fits, dens, fill)


def test_kernel_instances_use_no_scratch_and_spill_no_vgpr():
    """The eight k_persist_wide_sp instances (ROT, C10, DBG) of the built library, by their gfx950
    code objects' metadata (tools/isa_check.py resources_of)."""
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import isa_check
    assert isa_check.tools_available(), 'the LLVM binary tools that read the code objects are missing'
    res = {k: v for k, v in isa_check.resources_of(isa_check.LIB).items() if 'k_persist_wide_sp' in k}
    assert len(res) == 8, sorted(res)
    for k, v in res.items():
        assert v['private_segment_fixed_size'] == 0 and v['vgpr_spill_count'] == 0, (k, v)


def test_packer_clean_under_asan_ubsan():
    r = subprocess.run(['make', '-C', CSRC, 'wide_sp_check'], capture_output=True, text=True)
    assert r.returncode == 0, 'make wide_sp_check failed:\n' + r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1')
    r = subprocess.run([os.path.join(CSRC, 'build', 'asan', 'wide_sp_check')], env=env, capture_output=True,
                       text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert 'AddressSanitizer' not in out and 'runtime error:' not in out, out[-4000:]
    assert 'checks held' in r.stdout
