"""Host side of the training loop (kinetic-gan_amd/train.py, csrc/kg_input.hip) without a GPU: the numpy definition of
the random streams against Random123's known answers, the counter layout, the batch order against DeviceBatches, the
n_critic schedule, and the C ABI of the new entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd import train as ktrain
from kinetic_gan_amd.feeder import DeviceBatches, Feeder

import abi_layout
import train_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u32(*words):
    return np.array([int(w, 16) for w in words], dtype=np.uint32)


@pytest.mark.parametrize("ctr,key,out", [
    (("0", "0", "0", "0"), ("0", "0"), ("6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8")),
    (("ffffffff",) * 4, ("ffffffff",) * 2, ("408f276d", "41c83b0e", "a20bc7c6", "6d5451fd")),
    (("243f6a88", "85a308d3", "13198a2e", "03707344"), ("a4093822", "299f31d0"), ("d16cfe09", "94fdcceb", "5001e420", "24126ea1")),
])
def test_philox_known_answers(ctr, key, out):
    """Random123's kat_vectors for philox4x32-10"""
    got = train_def.philox4x32_10(_u32(*ctr)[None, :], _u32(*key)[None, :])[0]
    assert [hex(int(v)) for v in got] == [hex(int(v)) for v in _u32(*out)]


def test_stream_layout_has_no_collisions():
    """no (stream, step, index) - nor rank - maps to the counter of another, at the NTU sizes of a 64-sample iteration"""
    import kinetic_gan_amd.generator as KG
    G = KG.Generator(512, 3, 60, 64, 4, dataset="ntu")
    n_noise = sum(int(np.prod(s)) for s in train_def.plane_shapes(G, 64))
    sizes = {train_def.STREAM_Z: 64 * 512, train_def.STREAM_ALPHA: 64, train_def.STREAM_NOISE_D: n_noise,
             train_def.STREAM_NOISE_G: n_noise}
    assert 250_000 < 2 * n_noise + 64 * 512 < 400_000          # "about 0.3 M values"
    all_c = []
    for rank in (0, 1):
        for step in range(4):
            for stream, n in sizes.items():
                all_c.append(train_def.counters(n, stream, step, rank))
    c = np.concatenate(all_c)
    packed = c.view(np.dtype((np.void, 16))).reshape(-1)
    assert np.unique(packed).size == c.shape[0]
    # a step beyond 2^32 moves into the fourth counter word
    hi = train_def.counters(4, 0, (1 << 32) + 5)
    assert hi[0, 2] == 5 and hi[0, 3] == 1


def test_uniform_and_normal_definition_ranges():
    u = train_def.uniforms(1 << 16, 7, train_def.STREAM_ALPHA, 0)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    n32 = train_def.normals(1 << 16, 7, train_def.STREAM_Z, 0)
    n64 = train_def.normals(1 << 16, 7, train_def.STREAM_Z, 0, dtype=np.float64)
    assert np.isfinite(n32).all() and np.abs(n32 - n64).max() < 1e-5
    assert abs(n64.mean()) < 5 / 256 and abs(n64.var() - 1) < 5 * (2 / 65536) ** 0.5


@pytest.mark.parametrize("layout", ["ntu", "h36m"])
@pytest.mark.parametrize("norm", [True, False])
def test_batch_order_matches_device_batches(tmp_path, layout, norm):
    """the definition's batch of iteration s is the s-th batch DeviceBatches yields on the CPU, bit for bit, over two
    epochs (epoch turn-over, dropped tail: 23 samples in batches of 5), for one rank and for two"""
    c = 3 if layout == "ntu" else 2
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 23, c, 12, 7, 4, layout, seed=3)
    f = Feeder(dp, lp, norm=norm, dataset=layout)
    for world in (1, 2):
        for rank in range(world):
            db = DeviceBatches(f, 5, 8, "cpu", seed=11, rank=rank, world=world)
            bpe = len(db)
            assert bpe == (23 // 5) // world
            s = 0
            for _ in range(2):
                for x, y in db:
                    real, labels = train_def.batch(f, 5, 8, 11, s, rank, world)
                    assert x.dtype == torch.float32 and tuple(x.shape) == real.shape
                    assert np.array_equal(x.numpy().view(np.uint32), real.view(np.uint32)), (world, rank, s)
                    assert np.array_equal(y.numpy(), labels)
                    s += 1
            assert s == 2 * bpe
    scale, shift = ktrain.norm_constants(f)
    db = DeviceBatches(f, 5, 8, "cpu")
    assert (scale, shift) == (db.scale, db.shift)
    assert np.array_equal(ktrain.epoch_permutation(23, 11, 1), train_def.permutation(23, 11, 1))


@pytest.mark.parametrize("bpe,n_critic", [(3, 2), (7, 5), (10, 5), (4, 1), (2, 5)])
def test_update_pattern_restarts_every_epoch(bpe, n_critic):
    want = []
    for epoch in range(3):
        for i in range(bpe):
            want.append(i % n_critic == 0)          # kinetic-gan.py:160, i = batch index inside the epoch
    assert ktrain.update_pattern(bpe, n_critic, 3 * bpe) == want
    assert ktrain.update_pattern(bpe, n_critic, bpe, start=bpe + 1) == want[bpe + 1:2 * bpe + 1]
    loop = ktrain.TrainLoop.__new__(ktrain.TrainLoop)      # the schedule only: no device
    loop.bpe, loop.n_critic = bpe, n_critic
    for s in range(3 * bpe):
        loop.step_count = s
        assert loop.with_g() == want[s] and loop.epoch == s // bpe


def test_step_inputs_abi():
    """struct size and field offsets of the ctypes mirror against the compiled header; the symbols are exported"""
    build.build()
    lib = _native.load_library()
    assert hasattr(lib, "kg_step_inputs") and hasattr(lib, "kg_loss_append")
    assert lib.kg_abi_version() == 9
    abi_layout.assert_mirror("KgStepInputsArgs")
    consts = abi_layout.header_constants()
    assert [consts[k] for k in ("KG_STEP_MAX_PLANES", "KG_STREAM_Z", "KG_STREAM_ALPHA", "KG_STREAM_NOISE_D", "KG_STREAM_NOISE_G")] == \
        [_native.STEP_MAX_PLANES, _native.STREAM_Z, _native.STREAM_ALPHA, _native.STREAM_NOISE_D, _native.STREAM_NOISE_G]
    assert (train_def.STREAM_Z, train_def.STREAM_ALPHA, train_def.STREAM_NOISE_D, train_def.STREAM_NOISE_G) == (0, 1, 2, 3)


def test_step_inputs_validates_without_gpu():
    build.build()
    lib = _native.load_library()
    a = _native._StepInputsArgs()
    assert lib.kg_step_inputs(ctypes.byref(a), None) < 0 and b"kg_step_inputs" in lib.kg_last_error()
    a.step, a.ticket, a.B, a.world = 0x1000, 0x2000, 4, 1
    assert lib.kg_step_inputs(ctypes.byref(a), None) < 0 and b"nothing to write" in lib.kg_last_error()
    a.rank = 1
    assert lib.kg_step_inputs(ctypes.byref(a), None) < 0 and b"rank" in lib.kg_last_error()
    a.rank, a.noise, a.n_planes = 0, 0x3000, 9
    assert lib.kg_step_inputs(ctypes.byref(a), None) < 0 and b"n_planes" in lib.kg_last_error()
    a.noise, a.data, a.C, a.T, a.V, a.n_rows = None, 0x4000, 3, 8, 5, 10
    assert lib.kg_step_inputs(ctypes.byref(a), None) < 0 and b"gather needs" in lib.kg_last_error()
    assert lib.kg_loss_append(None, 4, None, None, None, None) < 0 and b"kg_loss_append" in lib.kg_last_error()
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.step_inputs(torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0, 4, z=torch.zeros(4, 8))
