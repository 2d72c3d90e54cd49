"""What every loop that replays a captured launch sequence does on the host, once: the capture and the
capture that puts the state back, the epoch permutation's double buffer, the run-ahead pacing and the two-column loss
record.  ``train.TrainLoop``, ``classify.ClassifierLoop``, ``sample.Sampler`` and ``evaluate.Evaluator`` are built from these;
this module imports none of them."""
from __future__ import annotations

import collections
from typing import List, Tuple

import numpy as np
import torch


def capture(fn, before_capture=None, warmup: int = 3):
    """fn() as a hipGraph: allocator warm-up on a side stream, then a thread-local capture (other threads of the process
    - a checkpoint writer, a collective's watchdog - cannot invalidate it).  ``before_capture`` runs between the two."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    if before_capture is not None:
        before_capture()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        fn()
    torch.cuda.synchronize()
    return graph


def capture_keeping(fn, tensors, device, before_capture=None, restore_host=None):
    """``capture(fn)`` around which the state stands still.  The warm-up calls in front of a capture are real calls:
    everything they move on the device - ``tensors`` - is cloned before and copied back afterwards, and ``restore_host()``
    puts back what they moved on the host.  Synchronises ``device`` first (work in flight on other streams included) and
    last."""
    torch.cuda.synchronize(device)
    keep = [t.clone() for t in tensors]
    graph = capture(fn, before_capture=before_capture)
    for t, k in zip(tensors, keep):
        t.copy_(k)
    if restore_host is not None:
        restore_host()
    torch.cuda.synchronize(device)
    return graph


def epoch_permutation(n: int, seed: int, epoch: int, shuffle: bool = True) -> np.ndarray:
    """The sample order of one epoch, exactly ``DeviceBatches._order``'s."""
    idx = np.arange(n)
    if shuffle:
        np.random.RandomState(seed + epoch).shuffle(idx)
    return idx


class PermutationFeed:
    """The epoch permutations of a resident dataset of ``n`` samples on the device: ``perm`` (2, plen) int64, which
    kg_step_inputs gathers through - slot ``epoch & 1`` holds the first ``plen`` entries of ``epoch_permutation(n, seed,
    epoch)``.  ``feed()`` in front of every iteration keeps it one epoch ahead without stalling the replays."""

    def __init__(self, n: int, plen: int, seed: int, device):
        self.n, self.seed, self.device = int(n), int(seed), device
        self.perm = torch.zeros((2, plen), dtype=torch.int64, device=device)
        self._host = [torch.empty(plen, dtype=torch.int64, pin_memory=True) for _ in range(2)]
        self._done = [None, None]
        self._wait = [False, False]
        self._epochs = [None, None]          # epoch held by each slot
        self._copy_stream = torch.cuda.Stream(device=device)

    def _upload(self, epoch: int):
        """permutation of `epoch` into slot epoch & 1 on the copy stream, behind the work enqueued so far (replays that
        still read the slot's previous epoch); the training stream waits for it when it first needs the slot"""
        slot = epoch & 1
        if self._done[slot] is not None:
            self._done[slot].synchronize()                   # the pinned buffer's last copy (an epoch ago)
        idx = epoch_permutation(self.n, self.seed, epoch)
        self._host[slot].numpy()[:] = idx[:self.perm.shape[1]]
        self._copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._copy_stream):
            self.perm[slot].copy_(self._host[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        self._done[slot] = ev
        self._epochs[slot] = epoch
        self._wait[slot] = True

    def feed(self, step_count: int, bpe: int) -> None:
        """host work in front of iteration ``step_count`` of epochs of ``bpe`` iterations: none inside an epoch"""
        epoch = step_count // bpe
        if self._epochs[epoch & 1] != epoch:                 # first iteration of a (resumed) run
            self._upload(epoch)
        if self._epochs[(epoch + 1) & 1] != epoch + 1:
            # one epoch ahead (normally at i == 0): every replay of the epoch this slot held has been enqueued
            self._upload(epoch + 1)
        if self._wait[epoch & 1]:
            torch.cuda.current_stream(self.device).wait_event(self._done[epoch & 1])
            self._wait[epoch & 1] = False


class Pacer:
    """The host enqueues at most ~run_ahead iterations ahead of the device (an event every run_ahead / 2 iterations, the
    host waits for the one before last): a queue filled to its limit replays measurably slower."""

    def __init__(self, run_ahead: int):
        self.run_ahead = max(2, int(run_ahead))
        self._marks = collections.deque()

    def tick(self, step_count: int) -> None:
        if step_count % (self.run_ahead // 2) == 0:
            if len(self._marks) >= 2:
                self._marks.popleft().synchronize()      # long complete unless the host is run_ahead iterations ahead
            ev = torch.cuda.Event()
            ev.record()
            self._marks.append(ev)


class LossRecord:
    """Two numbers per iteration.  ``ring`` (ring_len, 2) fp32 on ``device``, NaN until written: kg_loss_append writes the
    row of iteration ``s`` into slot ``s % ring_len``.  The host keeps what it has read: ``before_step()`` reads the ring in
    one piece when it holds ``ring_len`` unread rows, so nothing is overwritten unread and nothing synchronises in between."""

    def __init__(self, ring_len: int, device):
        self.ring_len = int(ring_len)
        self.ring = torch.full((self.ring_len, 2), float("nan"), dtype=torch.float32, device=device)
        self.flushed = 0                     # iterations whose rows have been read from the ring
        self._hist: List[np.ndarray] = []

    def _read(self) -> np.ndarray:
        return self.ring.cpu().numpy()       # ONE device -> host read

    def flush(self, step_count: int) -> None:
        if step_count <= self.flushed:
            return
        slots = np.arange(self.flushed, step_count) % self.ring_len
        self._hist.append(self._read()[slots])
        self.flushed = step_count

    def before_step(self, step_count: int) -> None:
        if step_count - self.flushed >= self.ring_len:
            self.flush(step_count)           # the ring is full: one bulk read per ring_len iterations at the most

    def history(self, step_count: int) -> Tuple[np.ndarray, np.ndarray]:
        """both columns of every iteration since the record (or its resumption) began.  Synchronises."""
        self.flush(step_count)
        h = np.concatenate(self._hist) if self._hist else np.zeros((0, 2), dtype=np.float32)
        return np.ascontiguousarray(h[:, 0]), np.ascontiguousarray(h[:, 1])

    def last_row(self, step_count: int):
        """the row of the last finished iteration on the host (None before the first): what a resumed run needs of the
        ring - kg_loss_append repeats the previous row's second column on an iteration that has none of its own"""
        return self.ring[(step_count - 1) % self.ring_len].cpu().clone() if step_count else None

    def load(self, step_count: int, last_row) -> None:
        """the record of a run resumed at ``step_count``: empty, with ``last_row`` back in its slot"""
        self.flushed = int(step_count)
        self._hist = []
        if last_row is not None:
            self.ring[(step_count - 1) % self.ring_len].copy_(last_row)
