"""Projection of real motions into the generator's W space: for each target sequence the latent ``w`` whose
synthesis reproduces it best, found by ``steps`` iterations of a per-sample Adam on the objective of kg_proj_loss.

One iteration is
    x = G.synthesis(w, noise)             the module path in eval mode (running statistics), differentiable in w
    kg_proj_loss(x, target) -> loss, gx   ONE launch: position / velocity / bone terms and dL/dx
    gw = autograd.grad(x, w, gx)          the generator's backward pass without parameter gradients
    kg_proj_step                          ONE launch: prior, schedule, Adam on w, best-so-far record, history row
    step += 1
captured once (``replay.capture_keeping``) and replayed ``steps`` times; nothing is read back until the caller does.

The Projector reads ``G`` through the live parameters and statistics and writes none of them: parameters, ``.grad``,
``requires_grad``, running statistics, ``num_batches_tracked`` and every module's ``training`` flag are what they were when a
call returns (the flags are switched on the host while it runs).  A generator that training updates in between is followed
without a rebuild; ``refresh_mean()`` re-estimates the starting point."""
from __future__ import annotations

import contextlib

import torch

from . import _native as nv
from . import ops
from .graph import Graph_h36m, graph_ntu
from .replay import capture_keeping

_BONES = {"ntu": graph_ntu.bones, "h36m": Graph_h36m.bones}


class Projector:
    """``Projector(G, n).project(targets, labels)`` inverts ``n`` sequences at a time.

    ``lambdas`` = (position, velocity, bone) weights of the objective, ``lambda_w`` the weight of the prior
    mean_d (w - wmean[label])^2; ``ramp_up`` / ``ramp_down``: fractions of ``steps`` over which the learning rate rises
    linearly from 0 and falls along a half cosine to 0 (0: off); ``noise``: "zero" planes or seven "fixed" planes drawn once
    from ``seed``; ``wmean[k]``: the mean of ``G.mapping(z, k)`` over ``mean_size`` draws from ``seed``, the starting point of
    class k; ``bones``: joint pairs (default: the dataset's skeleton); ``use_graph=False`` runs the same launches eagerly."""

    def __init__(self, G, n: int, dataset: str = "ntu", steps: int = 200, lr: float = 0.05, betas=(0.9, 0.999),
                 lambdas=(1.0, 1.0, 0.1), lambda_w: float = 0.0, ramp_up: float = 0.05, ramp_down: float = 0.25,
                 noise: str = "zero", seed: int = 0, mean_size: int = 1000, bones=None, use_graph: bool = True, eps: float = 1e-8):
        if dataset not in _BONES:
            raise ValueError("Projector: undefined dataset %r" % (dataset,))
        if noise not in ("zero", "fixed"):
            raise ValueError("Projector: noise must be 'zero' or 'fixed'")
        if int(n) < 1 or int(steps) < 1:
            raise ValueError("Projector: n and steps must be at least 1")
        if len(lambdas) != 3 or any(not (float(v) >= 0.0) for v in lambdas) or not (float(lambda_w) >= 0.0):
            raise ValueError("Projector: lambdas are three numbers >= 0 and lambda_w a number >= 0")
        if not (0.0 <= float(ramp_up) <= 1.0 and 0.0 <= float(ramp_down) <= 1.0):
            raise ValueError("Projector: ramp_up and ramp_down are fractions of steps in [0, 1]")
        self.G = G
        self.device = dev = next(G.parameters()).device
        self.n, self.steps, self.seed, self.mean_size = int(n), int(steps), int(seed), int(mean_size)
        self.n_classes = G.label_emb.num_embeddings
        self.D = G.mlp.mlp[0].in_features
        self.latent = self.D - self.n_classes
        last = G.st_gcn_networks[-1]
        self.C, self.T, self.V = int(last.out_channels), int(last.up_t), int(G.graph.num_node[last.lvl])
        self.bones = [tuple(int(j) for j in b) for b in (_BONES[dataset] if bones is None else bones)]
        if any(not (0 <= j < self.V) for b in self.bones for j in b):
            raise ValueError("Projector: bones name a joint outside [0, V=%d)" % self.V)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.lambdas, self.lambda_w = tuple(float(v) for v in lambdas), float(lambda_w)
        self.ramp_up, self.ramp_down = int(round(ramp_up * self.steps)), int(round(ramp_down * self.steps))
        self.use_graph = bool(use_graph) and dev.type == "cuda"
        n, D, f32 = self.n, self.D, torch.float32
        shapes = [(n, 1, int(g.up_t), int(G.graph.num_node[g.lvl])) for g in G.st_gcn_networks]
        if noise == "zero":
            self.noise = [torch.zeros(s, dtype=f32, device=dev) for s in shapes]
        else:
            gen = torch.Generator().manual_seed(self.seed)
            self.noise = [torch.randn(s, generator=gen, dtype=f32).to(dev) for s in shapes]
        # static buffers of a run
        self.target = torch.zeros((n, self.C, self.T, self.V), dtype=f32, device=dev)
        self.mask = torch.ones((n, self.T, self.V), dtype=f32, device=dev)
        self.labels = torch.zeros(n, dtype=torch.int64, device=dev)
        self.w = torch.zeros((n, D), dtype=f32, device=dev, requires_grad=True)
        self.am, self.av = torch.zeros((n, D), dtype=f32, device=dev), torch.zeros((n, D), dtype=f32, device=dev)
        self.loss = torch.zeros((n, 4), dtype=f32, device=dev)
        self.gx = torch.zeros((n, self.C, self.T, self.V), dtype=f32, device=dev)
        self.best_obj = torch.zeros(n, dtype=f32, device=dev)
        self.best_loss = torch.zeros((n, 4), dtype=f32, device=dev)
        self.best_w = torch.zeros((n, D), dtype=f32, device=dev)
        self.history = torch.zeros((self.steps, n), dtype=f32, device=dev)
        self.nonfinite = torch.zeros(n, dtype=torch.int32, device=dev)
        self.step = torch.ones(1, dtype=torch.int32, device=dev)
        self.wmean = torch.zeros((self.n_classes, D), dtype=f32, device=dev)
        self._affine = (1.0, 0.0)
        self._graph = None
        self.refresh_mean()

    # ---- the generator stands still -------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _reading(self):
        """eval mode and no parameter gradients while the block runs; every flag is put back on the host"""
        flags = [(m, m.training) for m in self.G.modules()]
        grads = [(p, p.requires_grad) for p in self.G.parameters()]
        try:
            self.G.eval()
            for p, _ in grads:
                p.requires_grad_(False)
            with ops.no_param_grads():
                yield
        finally:
            for m, f in flags:
                m.training = f
            for p, f in grads:
                p.requires_grad_(f)

    @torch.no_grad()
    def refresh_mean(self) -> None:
        """``wmean[k]`` = mean of ``G.mapping(z, k)`` over ``mean_size`` draws from ``seed`` (the same draws for every class)"""
        gen = torch.Generator().manual_seed(self.seed)
        z = torch.randn((self.mean_size, self.latent), generator=gen, dtype=torch.float32).to(self.device)
        with self._reading():
            for k in range(self.n_classes):
                lab = torch.full((self.mean_size,), k, dtype=torch.int64, device=self.device)
                self.wmean[k].copy_(self.G.mapping(z, lab).mean(0))

    # ---- the launch sequence --------------------------------------------------------------------------------------------
    def _iteration(self) -> None:
        scale, shift = self._affine
        with torch.enable_grad():
            x = self.G.synthesis(self.w, self.noise)
            nv.proj_loss(x.detach(), self.target, self.bones, self.lambdas, mask=self.mask, scale=scale, shift=shift,
                         loss=self.loss, gx=self.gx)
            gw, = torch.autograd.grad(x, self.w, self.gx)
        nv.proj_step(self.w.detach(), self.am, self.av, gw.contiguous(), self.wmean, self.labels, self.loss, self.step,
                     self.best_obj, self.best_loss, self.best_w, self.nonfinite, self.history, self.steps, self.lr,
                     self.betas[0], self.betas[1], self.eps, self.lambda_w, self.ramp_up, self.ramp_down)
        self.step.add_(1)

    def _state(self):
        return [self.w.detach(), self.am, self.av, self.loss, self.best_obj, self.best_loss, self.best_w, self.history,
                self.nonfinite, self.step]

    def _input(self, t, shape, what: str) -> torch.Tensor:
        t = torch.as_tensor(t)
        if tuple(t.shape) != tuple(shape):
            raise ValueError("Projector.project: %s has shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
        return t.to(self.device, torch.float32)

    @torch.no_grad()
    def _reset(self, targets, labels, mask, w_init) -> None:
        n = self.n
        self.target.copy_(self._input(targets, self.target.shape, "targets"))
        lab = torch.as_tensor(labels)
        if lab.dim() == 2:
            lab = lab.argmax(-1)
        if lab.shape != (n,):
            raise ValueError("Projector.project: %d labels for n=%d samples" % (lab.shape[0] if lab.dim() else 0, n))
        if not lab.is_cuda and lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= self.n_classes):
            raise ValueError("Projector.project: a label outside [0, %d)" % self.n_classes)
        self.labels.copy_(lab.to(self.device, torch.int64))
        if mask is None:
            self.mask.fill_(1.0)
        else:
            m = torch.as_tensor(mask)
            if tuple(m.shape) not in ((self.T, self.V), (n, self.T, self.V)):
                raise ValueError("Projector.project: mask has shape %s, expected (T, V) or (n, T, V)" % (tuple(m.shape),))
            self.mask.copy_(m.to(self.device, torch.float32).expand(n, self.T, self.V))
        w0 = self.wmean[self.labels] if w_init is None else self._input(w_init, (n, self.D), "w_init")
        self.w.detach().copy_(w0)
        self.best_w.copy_(w0)
        self.am.zero_()
        self.av.zero_()
        self.loss.fill_(float("nan"))
        self.best_obj.fill_(float("inf"))
        self.best_loss.fill_(float("nan"))
        self.history.fill_(float("nan"))
        self.nonfinite.zero_()
        self.step.fill_(1)

    def project(self, targets, labels, mask=None, w_init=None, scale: float = 1.0, shift: float = 0.0, on_step=None) -> dict:
        """Invert ``targets`` (n, C, T, V), read as ``targets * scale + shift``, with class ``labels`` (n,) (ids or one-hot
        rows).  ``mask``: weights >= 0, (T, V) or (n, T, V); an entry of weight 0 is not looked at (it may hold NaN).
        ``w_init`` (n, D) replaces the class means as the starting point.  Returns device tensors: ``w`` (n, D) after the last
        step, ``best_w`` the latents of each sample's smallest objective, ``recon`` (n, C, T, V) their synthesis, ``loss``
        (n, 4) of the last step and ``best_loss`` (n, 4) = [L, L_pos, L_vel, L_bone], ``best_obj`` (n,), ``history``
        (steps, n) the objective per step, ``nonfinite`` (n,) int32 the steps a sample was frozen because its objective or
        gradient was not finite.  ``on_step(s)``: called after iteration s, which then runs eagerly (a caller that reads the
        state back step by step)."""
        affine = (float(scale), float(shift))
        if affine != self._affine:              # (launch arguments of kg_proj_loss: a captured iteration holds them)
            self._affine, self._graph = affine, None
        self._reset(targets, labels, mask, w_init)
        with self._reading():
            replay = self.use_graph and on_step is None
            if replay and self._graph is None:
                self._graph = capture_keeping(self._iteration, self._state(), self.device)
            for s in range(1, self.steps + 1):
                if replay:
                    self._graph.replay()
                else:
                    self._iteration()
                    if on_step is not None:
                        on_step(s)
            with torch.no_grad():
                recon = self.G.synthesis(self.best_w, self.noise)
        return dict(w=self.w.detach().clone(), best_w=self.best_w.clone(), recon=recon, loss=self.loss.clone(),
                    best_loss=self.best_loss.clone(), best_obj=self.best_obj.clone(), history=self.history.clone(),
                    nonfinite=self.nonfinite.clone())
