"""The training loop of the reference's main program (kinetic-gan.py:117-197) on replayed hipGraphs.

One iteration is ONE graph replay.  The graph starts with ``kg_step_inputs`` (csrc/kg_input.hip): a single launch that
gathers the batch of the iteration from the device-resident dataset through the epoch's permutation, normalises it,
gathers its labels and draws every random input - latents, the penalty's interpolation weights, the injected noise of
both generator syntheses - from a counter-based generator (Philox4x32-10) keyed by the seed and an iteration counter
that lives in device memory and that the launch advances.  Then ``Trainer.iteration`` on those static buffers, then one
launch that appends the two losses to a device ring.  A replay therefore needs no host work and no host-to-device
traffic: the host only chooses between the two captured graphs - critic only, critic + generator (``i % n_critic == 0``
with ``i`` the batch index inside the epoch, kinetic-gan.py:160) - and uploads the next epoch's permutation, one epoch
ahead, on a side stream.

``ResidentDataset``: the cropped raw samples (first person, first ``t_size`` frames, unnormalised) and the labels on
the device.  A dataset that does not fit is streamed instead: ``DeviceBatches`` copies every batch into the same static
buffers in front of the replay; the random inputs still come from the kernel.

Definitions the tests pin this against: tests/train_def.py (numpy).  DESIGN.md 11.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _native as nv
from .checkpoint import AsyncCheckpointWriter
from .evaluate import write_metrics_csv
from .feeder import DeviceBatches, Feeder
from .replay import LossRecord, Pacer, PermutationFeed, capture_keeping
from .replay import epoch_permutation  # noqa: F401  (re-exported)
from .sample import sample_actions
from .wgan_gp import Trainer


def update_pattern(batches_per_epoch: int, n_critic: int, n_steps: int, start: int = 0) -> List[bool]:
    """with_g of iterations start .. start + n_steps - 1: the generator is updated when the batch index INSIDE the epoch
    is a multiple of n_critic (kinetic-gan.py:160), so the pattern restarts with every epoch."""
    return [((s % batches_per_epoch) % n_critic) == 0 for s in range(start, start + n_steps)]


def norm_constants(feeder: Feeder) -> Tuple[float, float]:
    """(scale, shift) with 2 (x - min) / (max - min) - 1 == x * scale + shift, as ``DeviceBatches`` computes them."""
    if not feeder.norm:
        return 1.0, 0.0
    span = float(feeder.max) - float(feeder.min)
    return 2.0 / span, -2.0 * float(feeder.min) / span - 1.0


class ResidentDataset:
    """The dataset on the device: ``data`` (N, C, t, V) fp32 - cropped to ``t_size`` frames, first person of an NTU
    array, NOT normalised (the gather normalises) - and ``labels`` (N,) int64.  ``fits`` is False (and nothing is
    uploaded) when the cropped array is larger than ``max_bytes`` (default: half of the free device memory)."""

    def __init__(self, feeder: Feeder, t_size: int, device, max_bytes: Optional[int] = None, chunk: int = 2048):
        self.feeder = feeder
        self.device = torch.device(device)
        self.t = min(int(t_size), feeder.T)
        self.n = len(feeder)
        self.shape = (self.n, feeder.C, self.t, feeder.V)
        self.nbytes = 4 * self.n * feeder.C * self.t * feeder.V
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        self.fits = self.nbytes <= int(max_bytes)
        self.scale, self.shift = norm_constants(feeder)
        self.data = self.labels = None
        if not self.fits:
            return
        self.data = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        stage = [torch.empty((chunk,) + self.shape[1:], dtype=torch.float32, pin_memory=True) for _ in range(2)]
        done = [None, None]
        for k, lo in enumerate(range(0, self.n, chunk)):
            hi, slot = min(self.n, lo + chunk), k & 1
            if done[slot] is not None:
                done[slot].synchronize()
            src = feeder.data[lo:hi, :, :self.t, :, 0] if feeder.dataset == 'ntu' else feeder.data[lo:hi, :, :self.t]
            stage[slot].numpy()[:hi - lo] = src
            self.data[lo:hi].copy_(stage[slot][:hi - lo], non_blocking=True)
            done[slot] = torch.cuda.Event()
            done[slot].record()
        self.labels = torch.as_tensor(np.asarray(feeder.label, dtype=np.int64)).to(self.device)
        torch.cuda.synchronize(self.device)


class TrainLoop:
    """``data``: a ``Feeder`` (made resident if it fits ``max_resident_bytes``, else streamed) or a ``ResidentDataset``.
    ``step()`` runs one iteration (a graph replay; with ``use_graph=False`` the same launches eagerly); ``run()`` is the
    reference's loop with its side effects; ``state_dict()`` / ``load_state_dict()`` resume a run bit for bit."""

    def __init__(self, G, D, data, batch_size: int, t_size: int, n_critic: int = 5, seed: int = 0, lr: float = 2e-4,
                 b1: float = 0.5, b2: float = 0.999, lambda_gp: float = 10.0, use_graph: bool = True,
                 ring_len: int = 4096, max_resident_bytes: Optional[int] = None, rank: int = 0, world: int = 1,
                 run_ahead: int = 16, ema_decay: Optional[float] = None, ema_warmup: float = 10.0,
                 eval_interval: Optional[int] = None, eval_pairs: int = 10, eval_select: Optional[str] = None,
                 eval_modes=("avg", "joint"), eval_trunc: Optional[float] = None, eval_trunc_mode: str = "-",
                 eval_data: Optional[Feeder] = None, eval_prdc: int = 0, eval_prdc_k: int = 5,
                 eval_frechet: int = 0, eval_frechet_modes=("pose", "motion"), eval_classifier=None,
                 eval_classifier_samples: int = 0, eval_classifier_batch: int = 512, eval_diversity_pairs: int = 200,
                 eval_multimodality_pairs: int = 20, eval_memorisation: Optional[str] = None,
                 eval_memorisation_samples: int = 0, eval_memorisation_method: str = "exact", *, eval_kinematics: int = 0,
                 eval_kinematics_still_eps: float = 1e-3):
        self.G, self.D = G, D
        self.device = next(G.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("TrainLoop runs on the GPU only (there is no CPU fallback)")
        if world > 1 and use_graph:
            raise NotImplementedError("TrainLoop: the data-parallel loop is not captured (use_graph=False runs it eagerly)")
        self.B, self.n_critic, self.seed = int(batch_size), int(n_critic), int(seed)
        self.rank, self.world, self.use_graph = int(rank), int(world), bool(use_graph)
        if isinstance(data, ResidentDataset):
            self.resident, feeder = data, data.feeder
        else:
            feeder = data
            self.resident = ResidentDataset(feeder, t_size, self.device, max_resident_bytes)
        self.feeder = feeder
        self.streaming = not self.resident.fits
        if eval_interval and eval_memorisation and self.streaming:
            raise ValueError("TrainLoop: eval_memorisation=%r searches the training set on the device, but this dataset is "
                             "streamed (%.1f MB cropped do not fit max_resident_bytes): pass a ResidentDataset that fits, or "
                             "score memorisation offline with tools/nearest_actions.py" % (eval_memorisation, self.resident.nbytes / 1e6))
        self.t = self.resident.t
        self.n = len(feeder)
        self.bpe = (self.n // self.B) // self.world          # batches of one epoch per rank, tail dropped
        if self.bpe < 1:
            raise ValueError("TrainLoop: the dataset holds fewer than batch_size * world samples")
        # ema_decay (None or 0: off): an exponential moving average of the generator's weights, moved by the generator's
        # Adam launch - inside the captured iteration; ema_generator() is the module over it
        self.ema_decay = float(ema_decay) if ema_decay else None
        self.ema_warmup = float(ema_warmup)
        self.trainer = Trainer(G, D, lr=lr, b1=b1, b2=b2, lambda_gp=lambda_gp, n_critic=n_critic, world_size=self.world,
                               ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
        dev, B = self.device, self.B
        self.latent = G.mlp.mlp[0].in_features - G.label_emb.num_embeddings
        self.n_classes = G.label_emb.num_embeddings
        # static inputs of the captured iteration
        self.real = torch.zeros((B, feeder.C, self.t, feeder.V), dtype=torch.float32, device=dev)
        self.labels = torch.zeros(B, dtype=torch.int64, device=dev)
        self.z = torch.zeros((B, self.latent), dtype=torch.float32, device=dev)
        self.alpha = torch.zeros(B, dtype=torch.float32, device=dev)
        self.plane_shapes = [(B, 1, gcn.up_t, G.graph.num_node[gcn.lvl]) for gcn in G.st_gcn_networks]
        self.plane_len = [int(np.prod(s)) for s in self.plane_shapes]
        self.noise = torch.zeros(2 * sum(self.plane_len), dtype=torch.float32, device=dev)
        self.noise_d, self.noise_g = nv.noise_views(self.noise, self.plane_shapes)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self._record = LossRecord(ring_len, dev)             # (d_loss, g_loss) of every iteration
        self.ring, self.ring_len = self._record.ring, self._record.ring_len
        self.step_count = 0                  # host mirror of step_dev
        self._pacer = Pacer(run_ahead)
        self.run_ahead = self._pacer.run_ahead
        self._graphs: Dict[bool, object] = {}
        self._gather = self._perm = None
        self._batches = self._batch_iter = None
        if self.streaming:
            self._batches = DeviceBatches(feeder, B, self.t, dev, seed=self.seed, rank=self.rank, world=self.world)
        else:
            r = self.resident
            self._perm = PermutationFeed(self.n, self.bpe * self.world * B, self.seed, dev)
            self._gather = nv.StepData(r.data, r.labels, self._perm.perm, self.bpe, r.scale, r.shift, self.real, self.labels)
        # eval_interval (None or 0: off): every eval_interval finished iterations one Evaluator replay is enqueued behind the
        # iteration - it scores the live (and the averaged) generator, appends to a record on the device and snapshots the
        # best-scoring weights there.  Off: no launch, no file, no state key is added.  eval_prdc (0: off):
        # the evaluation also scores precision / recall / density / coverage on that many samples per class.
        # eval_frechet (0: off): and the Frechet distance of eval_frechet_modes on that many samples per class.
        # eval_classifier (a trained classifier.Classifier) with eval_classifier_samples > 0: and accuracy, feature Frechet
        # distance, diversity and multimodality on that many samples per class.  eval_memorisation ("features":
        # the classifier round's features; "raw": eval_memorisation_samples samples per class): and authenticity / label
        # agreement against the loop's own ResidentDataset, searched where it lies; a streamed dataset is refused.
        # eval_kinematics (0: off): and the six kinematic W1 distances on that many samples per class, on the skeleton of the
        # feeder's dataset.
        self.eval_interval = int(eval_interval) if eval_interval else None
        self.evaluator = None
        if self.eval_interval:
            from .evaluate import Evaluator
            gens = {"live": G}
            if self.ema_decay:
                gens["ema"] = self.ema_generator()
            self.evaluator = Evaluator(gens, eval_data if eval_data is not None else feeder, pairs=eval_pairs, modes=eval_modes,
                                       select=eval_select, seed=self.seed, trunc=eval_trunc, trunc_mode=eval_trunc_mode,
                                       iteration=self.step_dev, use_graph=self.use_graph, t_size=self.t,
                                       prdc_per_class=eval_prdc, prdc_k=eval_prdc_k, frechet_per_class=eval_frechet,
                                       frechet_modes=eval_frechet_modes, classifier=eval_classifier,
                                       classifier_per_class=eval_classifier_samples, classifier_batch=eval_classifier_batch,
                                       diversity_pairs=eval_diversity_pairs, multimodality_pairs=eval_multimodality_pairs,
                                       memorisation=eval_memorisation or None,
                                       memorisation_train=self.resident if eval_memorisation else None,
                                       memorisation_per_class=eval_memorisation_samples,
                                       memorisation_method=eval_memorisation_method,
                                       kinematics_per_class=eval_kinematics,
                                       kinematics_dataset=getattr(feeder, "dataset", None) if eval_kinematics else None,
                                       kinematics_still_eps=eval_kinematics_still_eps)

    # ---- schedule ------------------------------------------------------------------------------------------------
    @property
    def epoch(self) -> int:
        return self.step_count // self.bpe

    def with_g(self, step: Optional[int] = None) -> bool:
        s = self.step_count if step is None else step
        return ((s % self.bpe) % self.n_critic) == 0

    def ema_generator(self):
        """The averaged generator (``Trainer.ema_generator``): weights from the moving average, BatchNorm statistics shared
        with the live generator.  A ``Sampler`` captured over it follows the training replays without a rebuild."""
        return self.trainer.ema_generator()

    # ---- the iteration ---------------------------------------------------------------------------------------------
    def _iteration(self, with_g: bool):
        """kg_step_inputs, the WGAN-GP iteration on the static buffers, the loss record: what a graph holds"""
        nv.step_inputs(self.step_dev, self._ticket, self.seed, self.B, z=self.z, alpha=self.alpha, noise=self.noise,
                       plane_len=self.plane_len, gather=self._gather, rank=self.rank, world=self.world)
        d_loss, g_loss = self.trainer.iteration(self.real, self.labels, self.z, self.alpha.view(-1, 1, 1, 1),
                                                self.noise_d, self.noise_g if with_g else None, with_g=with_g)
        nv.loss_append(self.ring, self.step_dev, d_loss, g_loss)

    def _state_tensors(self) -> List[torch.Tensor]:
        tr = self.trainer
        ts = [self.step_dev, self.ring, self.real, self.labels, self.z, self.alpha, self.noise]
        for f in (tr.fG, tr.fD):
            ts += [f.flat, f.grad, f.exp_avg, f.exp_avg_sq, f.step]
        if tr.fG.ema is not None:
            ts.append(tr.fG.ema)
        for m in (self.G, self.D):
            ts += list(m.buffers())
        return ts

    def _graph(self, with_g: bool):
        """The captured iteration.  The warm-up calls in front of a capture are real iterations: everything they move
        (parameters, optimiser state, BatchNorm statistics, the counter, the ring) is put back afterwards."""
        g = self._graphs.get(with_g)
        if g is not None:
            return g
        tr = self.trainer

        def drop_warmup_graph():
            # a sample the last warm-up call left behind would keep its autograd graph (created on the warm-up stream)
            tr._w = tr._fake_g = None
        g = capture_keeping(lambda: self._iteration(with_g), self._state_tensors(), self.device, before_capture=drop_warmup_graph)
        self._graphs[with_g] = g
        return g

    def _feed(self):
        """host work in front of an iteration: none inside an epoch on the resident path"""
        epoch, i = divmod(self.step_count, self.bpe)
        if self.streaming:
            if self._batch_iter is None:
                self._batches.epoch = epoch
                self._batch_iter = iter(self._batches)
                for _ in range(i):
                    next(self._batch_iter)
            x, y = next(self._batch_iter)
            self.real.copy_(x)
            self.labels.copy_(y)
            if i == self.bpe - 1:
                self._batch_iter = None
            return
        self._perm.feed(self.step_count, self.bpe)

    def step(self) -> None:
        """One iteration; no host synchronisation (the losses stay in the device ring until ``losses()``)."""
        self._record.before_step(self.step_count)
        self._pacer.tick(self.step_count)
        self._feed()
        wg = self.with_g()
        if self.use_graph:
            self._graph(wg).replay()
        else:
            self._iteration(wg)
        self.step_count += 1
        if self.evaluator is not None and self.step_count % self.eval_interval == 0:
            self.evaluator.evaluate()        # enqueued behind the iteration; reads step_dev = the finished count

    # ---- losses ----------------------------------------------------------------------------------------------------
    def losses(self) -> Tuple[np.ndarray, np.ndarray]:
        """(d_loss, g_loss) of every iteration since the run (or its resumption) began; an iteration without generator
        step repeats the last g_loss, as the reference's record does.  Synchronises."""
        return self._record.history(self.step_count)

    # ---- resume ----------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Everything a bit-exact continuation needs, on the host."""
        self._record.flush(self.step_count)
        tr = self.trainer
        out = {"step": self.step_count, "epoch": self.epoch, "seed": self.seed, "n_critic": self.n_critic,
               "batch_size": self.B, "batches_per_epoch": self.bpe, "last_losses": self._record.last_row(self.step_count)}
        for name, f, m in (("G", tr.fG, self.G), ("D", tr.fD, self.D)):
            out[name] = dict(f.state_dict(), buffers={k: b.cpu() for k, b in m.named_buffers()})
        if tr.fG.ema is not None:
            out["G"]["ema"] = tr.fG.ema.cpu()
            out["ema"] = {"decay": self.ema_decay, "warmup": self.ema_warmup}
        if self.evaluator is not None:
            out["eval"] = self.evaluator.state_dict()
        return out

    def load_state_dict(self, sd: dict) -> None:
        for k, mine in (("seed", self.seed), ("n_critic", self.n_critic), ("batch_size", self.B), ("batches_per_epoch", self.bpe)):
            if sd[k] != mine:
                raise ValueError("TrainLoop.load_state_dict: %s is %r in the checkpoint, %r here" % (k, sd[k], mine))
        tr = self.trainer
        if self.evaluator is not None and sd.get("eval") is not None:
            self.evaluator.check_compatible(sd["eval"])      # (raises before anything is loaded)
        have = sd.get("ema") is not None and sd["G"].get("ema") is not None
        if tr.fG.ema is not None and have:
            for k, mine in (("decay", self.ema_decay), ("warmup", self.ema_warmup)):
                if float(sd["ema"][k]) != mine:
                    raise ValueError("TrainLoop.load_state_dict: ema %s is %r in the checkpoint, %r here" % (k, sd["ema"][k], mine))
        for name, f, m in (("G", tr.fG, self.G), ("D", tr.fD, self.D)):
            s = sd[name]
            f.load_state_dict(s)
            bufs = dict(m.named_buffers())
            if set(bufs) != set(s["buffers"]):
                raise ValueError("TrainLoop.load_state_dict: buffers of %s do not match" % name)
            for k, b in bufs.items():
                b.copy_(s["buffers"][k])
        if tr.fG.ema is not None:                # (an average in the state is ignored by a loop without one)
            if have:
                tr.fG.ema.copy_(sd["G"]["ema"])
            else:
                warnings.warn("TrainLoop.load_state_dict: the checkpoint holds no weight average; it starts from the loaded "
                              "generator weights")
                tr.fG.ema.copy_(tr.fG.flat)
        self.step_count = int(sd["step"])
        self.step_dev.fill_(self.step_count)
        self._record.load(self.step_count, sd.get("last_losses"))
        self._batch_iter = None
        if self.evaluator is not None:           # (a record in the state is ignored by a loop without evaluation)
            if sd.get("eval") is not None:
                self.evaluator.load_state_dict(sd["eval"])
            else:
                self.evaluator.reset()
        torch.cuda.synchronize(self.device)

    # ---- the reference's loop ------------------------------------------------------------------------------------------
    def sample_action(self, path: str, G=None) -> None:
        """kinetic-gan.py:84-91: 10 samples per class, labels 0 .. n_classes-1 repeated, saved as one .npy (``G``: another
        generator than the live one - the averaged module)"""
        imgs, _, _ = sample_actions(self.G if G is None else G, self.n_classes, self.latent, gen_qtd=10, qtd=10)
        with open(path, "wb") as f:
            np.save(f, imgs.cpu().numpy())

    def save_losses(self, path: str) -> None:
        from scipy.io import savemat
        d, g = self.losses()
        savemat(path, {"d_loss": d, "g_loss": g})

    def run(self, n_epochs: int, sample_interval: int = 5000, checkpoint_interval: int = 10000, out_dir: str = "runs",
            log_interval: int = 100, log=print, state_path: Optional[str] = None) -> None:
        """Epochs ``self.epoch .. n_epochs - 1`` with the reference's side effects (kinetic-gan.py:176-197), none of them
        on the timed path: the progress line - printed every ``log_interval`` iterations from ONE bulk read of the loss
        ring -, ``actions/<batches_done>.npy`` and ``plot_loss.mat`` every ``sample_interval`` iterations, both networks'
        checkpoints (``models/generator_<batches_done>.pth``, written in the background) every ``checkpoint_interval``.
        ``state_path``: ``state_dict()`` is saved there with every checkpoint and at the end (``load_state_dict`` of that
        file continues the run bit for bit).  With the weight average on (``ema_decay``) the averaged generator is written
        next to the live one at the same intervals: ``models/generator_ema_<batches_done>.pth`` and
        ``actions_ema/<batches_done>.npy``.  With evaluation on (``eval_interval``): ``metrics.csv`` (one row per evaluation:
        iteration, every score, improved) at every ``sample_interval`` and at the end, ``models/generator_best.pth`` (the
        snapshot of the best-scoring weights) at every ``checkpoint_interval`` and at the end whenever the best iteration
        has changed since the last write, and the best value and its iteration on the progress line."""
        models_out, actions_out = os.path.join(out_dir, "models"), os.path.join(out_dir, "actions")
        os.makedirs(models_out, exist_ok=True)
        os.makedirs(actions_out, exist_ok=True)
        ema_G = self.ema_generator() if self.ema_decay else None
        if ema_G is not None:
            ema_actions_out = os.path.join(out_dir, "actions_ema")
            os.makedirs(ema_actions_out, exist_ok=True)
        log_interval = max(1, min(int(log_interval), self.ring_len))
        writer = AsyncCheckpointWriter()
        ev, best_written = self.evaluator, -1

        def write_best():
            nonlocal best_written
            b = ev.best()
            if b["iteration"] != best_written and b["iteration"] >= 0:
                writer.save(ev.best_generator(), os.path.join(models_out, "generator_best.pth"))
                best_written = b["iteration"]
        try:
            while self.step_count < n_epochs * self.bpe:
                batches_done = self.step_count
                epoch, i = divmod(batches_done, self.bpe)
                self.step()
                if (batches_done + 1) % log_interval == 0 or batches_done + 1 == n_epochs * self.bpe:
                    d, g = self.losses()
                    line = "[Epoch %d/%d] [Batch %d/%d] [D loss: %f] [G loss: %f]" % (epoch, n_epochs, i, self.bpe, d[-1], g[-1])
                    if ev is not None:
                        b = ev.best()
                        line += " [best %s: %f @ %d]" % (ev.select, b["value"], b["iteration"])
                    log(line)
                if batches_done % sample_interval == 0:
                    self.sample_action(os.path.join(actions_out, "%d.npy" % batches_done))
                    if ema_G is not None:
                        self.sample_action(os.path.join(ema_actions_out, "%d.npy" % batches_done), ema_G)
                    self.save_losses(os.path.join(out_dir, "plot_loss.mat"))
                    if ev is not None:
                        write_metrics_csv(os.path.join(out_dir, "metrics.csv"), ev.records())
                if checkpoint_interval != -1 and batches_done % checkpoint_interval == 0:
                    writer.save(self.G, os.path.join(models_out, "generator_%d.pth" % batches_done))
                    writer.save(self.D, os.path.join(models_out, "discriminator_%d.pth" % batches_done))
                    if ema_G is not None:
                        writer.save(ema_G, os.path.join(models_out, "generator_ema_%d.pth" % batches_done))
                    if ev is not None:
                        write_best()
                    if state_path is not None:
                        torch.save(self.state_dict(), state_path)
            self.save_losses(os.path.join(out_dir, "plot_loss.mat"))
            if ev is not None:
                write_metrics_csv(os.path.join(out_dir, "metrics.csv"), ev.records())
                write_best()
            if state_path is not None:
                torch.save(self.state_dict(), state_path)
        finally:
            writer.close()
