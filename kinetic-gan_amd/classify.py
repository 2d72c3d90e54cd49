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

import collections
from typing import List, Tuple

import numpy as np
import torch

from . import _native as nv
from .train import ResidentDataset, _capture, epoch_permutation
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
        self.ring_len = int(ring_len)
        self.ring = torch.full((self.ring_len, 2), float("nan"), dtype=torch.float32, device=dev)
        self.step_count = 0                              # host mirror of step_dev
        self.run_ahead = max(2, int(run_ahead))
        self._marks = collections.deque()
        self._flushed = 0
        self._hist: List[np.ndarray] = []
        self._graph_obj = None
        r = self.resident
        plen = self.bpe * B
        self._perm = torch.zeros((2, plen), dtype=torch.int64, device=dev)
        self._perm_host = [torch.empty(plen, dtype=torch.int64, pin_memory=True) for _ in range(2)]
        self._perm_done = [None, None]
        self._perm_wait = [False, False]
        self._perm_epochs = [None, None]                 # epoch held by each slot of the device permutation
        self._copy_stream = torch.cuda.Stream(device=dev)
        self._gather = nv.StepData(r.data, r.labels, self._perm, self.bpe, r.scale, r.shift, self.real, self.labels)

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
        (parameters, optimiser state, the counter, the ring) is put back afterwards, as ``TrainLoop._graph`` does."""
        if self._graph_obj is None:
            torch.cuda.synchronize(self.device)
            ts = self._state_tensors()
            keep = [t.clone() for t in ts]
            clean = self.flat._clean
            g = _capture(self._iteration)
            for t, k in zip(ts, keep):
                t.copy_(k)
            self.flat._clean = clean
            torch.cuda.synchronize(self.device)
            self._graph_obj = g
        return self._graph_obj

    def _upload_perm(self, epoch: int):
        """permutation of `epoch` into slot epoch & 1 on the copy stream, behind the work enqueued so far; the training
        stream waits for it when it first needs the slot (``TrainLoop._upload_perm``)"""
        slot = epoch & 1
        if self._perm_done[slot] is not None:
            self._perm_done[slot].synchronize()
        idx = epoch_permutation(self.n, self.seed, epoch)
        self._perm_host[slot].numpy()[:] = idx[:self._perm.shape[1]]
        self._copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._copy_stream):
            self._perm[slot].copy_(self._perm_host[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        self._perm_done[slot] = ev
        self._perm_epochs[slot] = epoch
        self._perm_wait[slot] = True

    def _feed(self):
        epoch = self.step_count // self.bpe
        if self._perm_epochs[epoch & 1] != epoch:
            self._upload_perm(epoch)
        if self._perm_epochs[(epoch + 1) & 1] != epoch + 1:
            self._upload_perm(epoch + 1)
        if self._perm_wait[epoch & 1]:
            torch.cuda.current_stream(self.device).wait_event(self._perm_done[epoch & 1])
            self._perm_wait[epoch & 1] = False

    def step(self) -> None:
        """One iteration; no host synchronisation (loss and accuracy stay in the device ring until ``losses()``); the host
        runs at most ~run_ahead iterations ahead of the device, as ``TrainLoop.step``."""
        if self.step_count - self._flushed >= self.ring_len:
            self._flush()
        if self.step_count % (self.run_ahead // 2) == 0:
            if len(self._marks) >= 2:
                self._marks.popleft().synchronize()
            ev = torch.cuda.Event()
            ev.record()
            self._marks.append(ev)
        self._feed()
        if self.use_graph:
            self._graph().replay()
        else:
            self._iteration()
        self.step_count += 1

    # ---- record ----------------------------------------------------------------------------------------------------
    def _flush(self):
        n = self.step_count - self._flushed
        if n <= 0:
            return
        ring = self.ring.cpu().numpy()
        slots = np.arange(self._flushed, self.step_count) % self.ring_len
        self._hist.append(ring[slots].copy())
        self._flushed = self.step_count

    def losses(self) -> Tuple[np.ndarray, np.ndarray]:
        """(loss, batch accuracy) of every iteration since the run (or its resumption) began.  Synchronises."""
        self._flush()
        h = np.concatenate(self._hist) if self._hist else np.zeros((0, 2), dtype=np.float32)
        return h[:, 0], h[:, 1]

    # ---- resume ----------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        self._flush()
        f = self.flat
        return {"step": self.step_count, "seed": self.seed, "batch_size": self.B, "batches_per_epoch": self.bpe,
                "flat": f.flat.cpu(), "exp_avg": f.exp_avg.cpu(), "exp_avg_sq": f.exp_avg_sq.cpu(), "adam_step": f.step.cpu(),
                "last_losses": self.ring[(self.step_count - 1) % self.ring_len].cpu() if self.step_count else None}

    def load_state_dict(self, sd: dict) -> None:
        for k, mine in (("seed", self.seed), ("batch_size", self.B), ("batches_per_epoch", self.bpe)):
            if sd[k] != mine:
                raise ValueError("ClassifierLoop.load_state_dict: %s is %r in the checkpoint, %r here" % (k, sd[k], mine))
        f = self.flat
        if sd["flat"].numel() != f.flat.numel():
            raise ValueError("ClassifierLoop.load_state_dict: the checkpoint's parameters do not fit this classifier")
        f.flat.copy_(sd["flat"])
        f.exp_avg.copy_(sd["exp_avg"])
        f.exp_avg_sq.copy_(sd["exp_avg_sq"])
        f.step.copy_(sd["adam_step"])
        f.grad.zero_()
        self.step_count = self._flushed = int(sd["step"])
        self._hist = []
        self.step_dev.fill_(self.step_count)
        if sd.get("last_losses") is not None:
            self.ring[(self.step_count - 1) % self.ring_len].copy_(sd["last_losses"])
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

