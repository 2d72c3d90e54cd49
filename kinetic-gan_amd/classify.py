"""Training loop of the action classifier (classifier.Classifier) on replayed hipGraphs - ``train.TrainLoop``'s structure
with one network and a supervised loss.

One iteration is one fixed launch sequence: ``kg_step_inputs`` with the gather only (the batch of the iteration from the
device-resident dataset through the epoch's permutation, normalised, with its labels; the launch advances the iteration
counter on the device), the trunk forward, the head (kg_cls_head_fwd: forward + finish), the head's backward, the trunk
backward without an input gradient for block 0, the deferred parameter-gradient launches and the head's, flat-buffer Adam
(kg_adam_step_fused) and ``kg_loss_append`` of (loss, batch accuracy) into a device ring.  With ``use_graph`` that sequence
is captured once and replayed; the host only uploads the next epoch's permutation, one epoch ahead, on a side stream.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from . import _native as nv
from .replay import LossRecord, Pacer, PermutationFeed, capture_keeping
from .train import ResidentDataset
from .wgan_gp import FlatParams, _const_like


class ClassifierLoop:
    """``data``: a ``Feeder`` or a ``train.ResidentDataset`` (resident datasets only: one that does not fit raises).
    ``step()`` runs one iteration without host synchronisation; ``losses()`` reads (loss, batch accuracy) of every iteration
    from the device ring; ``state_dict()`` / ``load_state_dict()`` resume a run bit for bit; ``evaluate()`` scores a held-out
    set off the timed path."""

    def __init__(self, C, data, batch_size: int, t_size: int, seed: int = 0, lr: float = 1e-3, b1: float = 0.9,
                 b2: float = 0.999, use_graph: bool = True, ring_len: int = 4096, run_ahead: int = 16):
        self.C = C
        self.device = next(C.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("ClassifierLoop runs on the GPU only (there is no CPU fallback)")
        self.B, self.seed, self.use_graph = int(batch_size), int(seed), bool(use_graph)
        self.lr, self.b1, self.b2 = float(lr), float(b1), float(b2)
        if isinstance(data, ResidentDataset):
            self.resident, feeder = data, data.feeder
        else:
            feeder = data
            self.resident = ResidentDataset(feeder, t_size, self.device)
        if not self.resident.fits:
            raise ValueError("ClassifierLoop: the dataset (%d bytes) does not fit on the device; only resident datasets are "
                             "supported" % self.resident.nbytes)
        self.feeder = feeder
        self.t = self.resident.t
        self.n = len(feeder)
        self.bpe = self.n // self.B                      # batches of one epoch, tail dropped
        if self.bpe < 1:
            raise ValueError("ClassifierLoop: the dataset holds fewer than batch_size samples")
        self.flat = FlatParams(C)
        self.flat.fused_step = True                      # the Adam launch clears the bucket it has consumed
        dev, B = self.device, self.B
        self.real = torch.zeros((B, feeder.C, self.t, feeder.V), dtype=torch.float32, device=dev)
        self.labels = torch.zeros(B, dtype=torch.int64, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self._record = LossRecord(ring_len, dev)         # (loss, batch accuracy) of every iteration
        self.ring, self.ring_len = self._record.ring, self._record.ring_len
        self.step_count = 0                              # host mirror of step_dev
        self._pacer = Pacer(run_ahead)
        self.run_ahead = self._pacer.run_ahead
        self._graph_obj = None
        r = self.resident
        self._perm = PermutationFeed(self.n, self.bpe * B, self.seed, dev)
        self._gather = nv.StepData(r.data, r.labels, self._perm.perm, self.bpe, r.scale, r.shift, self.real, self.labels)

    @property
    def epoch(self) -> int:
        return self.step_count // self.bpe

    # ---- the iteration ---------------------------------------------------------------------------------------------
    def _iteration(self):
        """what a graph holds"""
        nv.step_inputs(self.step_dev, self._ticket, self.seed, self.B, gather=self._gather)
        f = self.flat
        f.zero_grad()
        out = self.C.classify(self.real, self.labels)
        loss = out["loss"]
        loss.backward(_const_like(loss, 1.0))
        f.allreduce_and_step(self.lr, self.b1, self.b2)
        acc = torch.mul(out["correct"], 1.0 / self.B)             # int32 count -> fp32 fraction, one launch
        nv.loss_append(self.ring, self.step_dev, loss.detach(), acc)

    def _state_tensors(self) -> List[torch.Tensor]:
        f = self.flat
        return [self.step_dev, self.ring, self.real, self.labels, f.flat, f.grad, f.exp_avg, f.exp_avg_sq, f.step]

    def _graph(self):
        """The captured iteration.  The warm-up calls in front of the capture are real iterations: everything they move
        (parameters, optimiser state, the counter, the ring; on the host, whether the gradient bucket is known to be zero)
        is put back afterwards."""
        if self._graph_obj is None:
            clean = self.flat._clean
            self._graph_obj = capture_keeping(self._iteration, self._state_tensors(), self.device,
                                              restore_host=lambda: setattr(self.flat, "_clean", clean))
        return self._graph_obj

    def step(self) -> None:
        """One iteration; no host synchronisation (loss and accuracy stay in the device ring until ``losses()``); the host
        runs at most ~run_ahead iterations ahead of the device, as ``TrainLoop.step``."""
        self._record.before_step(self.step_count)
        self._pacer.tick(self.step_count)
        self._perm.feed(self.step_count, self.bpe)
        if self.use_graph:
            self._graph().replay()
        else:
            self._iteration()
        self.step_count += 1

    # ---- record ----------------------------------------------------------------------------------------------------
    def losses(self) -> Tuple[np.ndarray, np.ndarray]:
        """(loss, batch accuracy) of every iteration since the run (or its resumption) began.  Synchronises."""
        return self._record.history(self.step_count)

    # ---- resume ----------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        self._record.flush(self.step_count)
        return {"step": self.step_count, "seed": self.seed, "batch_size": self.B, "batches_per_epoch": self.bpe,
                **self.flat.state_dict(), "last_losses": self._record.last_row(self.step_count)}

    def load_state_dict(self, sd: dict) -> None:
        for k, mine in (("seed", self.seed), ("batch_size", self.B), ("batches_per_epoch", self.bpe)):
            if sd[k] != mine:
                raise ValueError("ClassifierLoop.load_state_dict: %s is %r in the checkpoint, %r here" % (k, sd[k], mine))
        self.flat.load_state_dict(sd)
        self.step_count = int(sd["step"])
        self.step_dev.fill_(self.step_count)
        self._record.load(self.step_count, sd.get("last_losses"))
        torch.cuda.synchronize(self.device)

    # ---- held-out accuracy -------------------------------------------------------------------------------------------
    def evaluate(self, x, labels, batch: int = 256) -> dict:
        """Accuracy of the classifier on (x (N, C, T, V) - normalised as the training batches are -, labels (N,)): dict(accuracy,
        correct (L,), total (L,)) with the per-class counts as numpy int64.  Off the timed path (synchronises)."""
        return evaluate(self.C, x, labels, batch)


def evaluate(clf, x, labels, batch: int = 256) -> dict:
    dev = next(clf.parameters()).device
    x = torch.as_tensor(x)
    y = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(torch.int64)
    L = clf.n_classes
    correct = torch.zeros(L, dtype=torch.int64, device=dev)
    total = torch.zeros(L, dtype=torch.int64, device=dev)
    with torch.no_grad():
        for lo in range(0, x.shape[0], batch):
            xb = x[lo:lo + batch].to(dev, dtype=torch.float32)
            yb = y[lo:lo + batch].to(dev)
            pred = clf.classify(xb, yb)["pred"].to(torch.int64)
            ok = (yb >= 0) & (yb < L)
            total += torch.bincount(yb[ok], minlength=L)
            correct += torch.bincount(yb[ok & (pred == yb)], minlength=L)
    correct, total = correct.cpu().numpy(), total.cpu().numpy()
    return {"accuracy": float(correct.sum()) / max(1, int(x.shape[0])), "correct": correct, "total": total}

