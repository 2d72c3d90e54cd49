"""Host side of the replay loops (kinetic-gan_amd/replay.py) without a GPU: the slot arithmetic of the loss record on a CPU
ring - wrap, flush when full, resume - and the optimiser state of a ``FlatParams``."""
import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd.replay import LossRecord
from kinetic_gan_amd.wgan_gp import FlatParams

RING_LEN, STEPS = 4, 11
ROWS = (np.arange(2 * STEPS, dtype=np.float32).reshape(STEPS, 2) + 0.5) / 3.0


def _record():
    """a record on a CPU ring, and the list that counts its device-to-host reads (one entry per read)"""
    rec, reads = LossRecord(RING_LEN, "cpu"), []
    read = rec._read

    def counted():
        reads.append(rec.flushed)
        return read()
    rec._read = counted
    return rec, reads


def _steps(rec, reads, start, stop):
    """iterations start .. stop - 1: the hook in front of each, then the row of iteration s into slot s % ring_len, as
    kg_loss_append writes it for step - 1; returns the iterations in front of which the ring was read"""
    at = []
    for s in range(start, stop):
        n, unread = len(reads), s - rec.flushed
        rec.before_step(s)
        assert len(reads) - n == (1 if unread == RING_LEN else 0), (s, unread)      # one read, of a full ring only
        assert unread <= RING_LEN and rec.flushed == (s if unread == RING_LEN else s - unread)
        if len(reads) != n:
            at.append(s)
        rec.ring[s % RING_LEN] = torch.as_tensor(ROWS[s])
    return at


def test_loss_record_wraps_and_flushes_when_full():
    rec, reads = _record()
    assert tuple(rec.ring.shape) == (RING_LEN, 2) and rec.ring.dtype == torch.float32 and torch.isnan(rec.ring).all()
    assert _steps(rec, reads, 0, STEPS) == [4, 8]            # only in front of an iteration that would overwrite an unread row
    a, b = rec.history(STEPS)
    assert len(reads) == 3                                   # (the three rows left: one more read)
    assert a.dtype == b.dtype == np.float32
    assert np.array_equal(a, ROWS[:, 0]) and np.array_equal(b, ROWS[:, 1])
    a2, b2 = rec.history(STEPS)                              # nothing new: no read, the same history
    assert len(reads) == 3 and np.array_equal(a2, a) and np.array_equal(b2, b)


def test_loss_record_resumes_in_the_middle():
    first, reads = _record()
    _steps(first, reads, 0, 6)
    a0, b0 = first.history(6)
    assert np.array_equal(a0, ROWS[:6, 0]) and np.array_equal(b0, ROWS[:6, 1])
    last = first.last_row(6)
    assert np.array_equal(last.numpy(), ROWS[5])
    assert LossRecord(RING_LEN, "cpu").last_row(0) is None
    rec, reads = _record()
    rec.load(6, last)
    assert rec.flushed == 6
    ring = rec.ring.numpy()
    assert np.array_equal(ring[(6 - 1) % RING_LEN], ROWS[5])                 # the restored row, before any new write
    assert np.isnan(np.delete(ring, (6 - 1) % RING_LEN, axis=0)).all()
    assert _steps(rec, reads, 6, STEPS) == [10]
    a1, b1 = rec.history(STEPS)
    assert np.array_equal(a1, ROWS[6:, 0]) and np.array_equal(b1, ROWS[6:, 1])
    # a state of before the first iteration holds no row: the record starts empty
    rec.load(0, None)
    assert rec.flushed == 0 and rec.history(0)[0].shape == (0,)


def _module(seed, out=2):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, out))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_flat_params_state_round_trip():
    g = torch.Generator().manual_seed(5)
    ma, mb = _module(1), _module(2)
    a, b = FlatParams(ma), FlatParams(mb)
    a.exp_avg.copy_(torch.randn(a.flat.shape, generator=g))
    a.exp_avg_sq.copy_(torch.rand(a.flat.shape, generator=g))
    a.step.fill_(7)
    sd = a.state_dict()
    assert set(sd) == {"flat", "exp_avg", "exp_avg_sq", "adam_step"}
    assert all(t.device.type == "cpu" for t in sd.values())
    assert not torch.equal(a.flat, b.flat)
    b.grad.fill_(1.0)
    b.load_state_dict(sd)
    for mine, theirs in ((b.flat, a.flat), (b.exp_avg, a.exp_avg), (b.exp_avg_sq, a.exp_avg_sq), (b.step, a.step)):
        assert mine.dtype == theirs.dtype and torch.equal(_bits(mine), _bits(theirs))
    assert torch.count_nonzero(b.grad) == 0
    for p, q in zip(mb.parameters(), ma.parameters()):       # the module's parameters are views into the loaded buffer
        assert torch.equal(_bits(p), _bits(q))


def test_flat_params_rejects_another_numel():
    sd = FlatParams(_module(1)).state_dict()
    c = FlatParams(_module(3, out=5))
    keep = c.flat.clone()
    with pytest.raises(ValueError):
        c.load_state_dict(sd)
    assert torch.equal(c.flat, keep)
