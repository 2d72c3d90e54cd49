"""Inference path of the reference's sampling script on the HIP generator (row N2 of SURVEY.md 8f).

``sample_actions`` is the loop of generate.py:85-105 without its file I/O: per round it draws ``qtd`` latents for
every class still short of ``gen_qtd`` samples, applies Z-space truncation (generate.py:14-21) or passes the W-space
truncation factor to ``Generator.forward`` (generator.py:86,97-108), and collects skeleton sequences, labels and
latents.  The generator runs in eval mode under ``torch.no_grad()``: BatchNorm uses its running statistics, folded
into the tcn / residual conv weights (generator.st_gcn) so that no statistics launch remains.

``Sampler`` is the same loop as a fixed launch sequence on static buffers: the random inputs of a round
come from ONE kg_sample_inputs launch driven by a device counter, the truncation trick is ONE kg_trunc_lerp launch, the
eval-mode BatchNorm coefficients of all layers come from ONE kg_bn_eval_coef launch that reads the live running
statistics, and the seven blocks run on the inference schedule ``infer_pass`` - the blocks that fit LDS as one
kg_genblock_infer launch each.  A round is therefore one hipGraph replay with no host work, and it follows every
in-place update of the generator (training replays in between) without a rebuild.
"""
from __future__ import annotations

from collections import Counter
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as nv
from . import gen_trunk as gt
from .generator import truncate_z
from .replay import capture_keeping


@torch.no_grad()
def sample_actions(G, n_classes: int, latent_dim: int, gen_qtd: int, qtd: int = 25, label: int = -1,
                   trunc: Optional[float] = None, trunc_mode: str = "-", mean_size: int = 1000,
                   stochastic_z: Optional[torch.Tensor] = None, keep_on_device: bool = False):
    """Returns (imgs (M, C, T, V), labels (M,), z (M, latent)) with at least ``gen_qtd`` samples of every requested
    class (all classes for ``label == -1``), in the order generate.py produces them.  ``trunc_mode``: 'z', 'w' or
    '-' (generate.py:38-41); ``stochastic_z``: one fixed latent point for every sample (generate.py:80-83)."""
    was_training = G.training
    G.eval()
    dev = next(G.parameters()).device
    classes = list(range(n_classes)) if label == -1 else [label]
    imgs, labs, zs = [], [], []
    count = Counter()
    try:
        while classes:
            n = qtd * len(classes)
            if stochastic_z is not None:
                z = stochastic_z.to(dev).reshape(1, latent_dim).repeat(n, 1)
            else:
                z = torch.as_tensor(np.random.normal(0, 1, (n, latent_dim)), dtype=torch.float32, device=dev)
            if trunc_mode == "z":
                z = truncate_z(z, mean_size, trunc)
            labels_np = np.array([num for _ in range(qtd) for num in classes])
            labels = torch.as_tensor(labels_np, dtype=torch.long, device=dev)
            out = G(z, labels, trunc) if trunc_mode == "w" else G(z, labels)
            imgs.append(out if keep_on_device else out.cpu())
            zs.append(z if keep_on_device else z.cpu())
            labs.append(labels_np)
            count.update(labels_np.tolist())
            classes = [c for c in classes if count[c] < gen_qtd]
    finally:
        G.train(was_training)
    return torch.cat(imgs, 0), np.concatenate(labs, 0), torch.cat(zs, 0)


def _infer_fusable(g, n: int, p) -> bool:
    return (g.T > 1 and g.Tc * g.Vc >= gt.FUSED_MIN_COLS and
            nv.genblock_infer_supported(g.dims, n, p["wg"], p["wr"] if g.res == "conv" else None, p["wt"]))


def infer_pass(meta, w, noise, adjs, params, coefs):
    """The inference schedule of the seven blocks (gen_trunk.fwd_pass without tape and statistics): x = w.view(N, lat,
    1, 1) -> out.  ``coefs[i]`` = (ct, cr): the (4, C) eval-mode BatchNorm coefficients of block i's tcn / residual
    branch (kg_bn_eval_coef) or None.  A block that fits LDS is ONE kg_genblock_infer launch; the weight-bound front
    blocks take the staged launches head conv -> kg_gen_expand -> tcn conv -> kg_affine_act.  The weights are used as
    they are: no BatchNorm fold, no per-channel stock ops."""
    x = w.view(w.shape[0], w.shape[1], 1, 1)
    n = w.shape[0]
    for i, g in enumerate(meta.geoms):
        p = meta.block_params(params, i)
        ct, cr = coefs[i]
        C = g.cout
        if _infer_fusable(g, n, p):
            x = nv.genblock_infer(g.dims, x=x, wg=p["wg"], wr=p["wr"], br=p["br"], wt=p["wt"], bt=p["bt"], B=adjs[i], U=g.U,
                                  ct=ct, cr=cr, noise=noise[i], nw=p["nw"], slope=gt.SLOPE)
            continue
        yc = gt._head_conv(g, x, p["wg"], p["wr"])
        rs = yc[:, g.Mg:] if g.res == "conv" else (x if g.res == "identity" else None)
        z, r = nv.gen_expand(yc[:, :g.Mg], None, g.U, g.rep, C, rs=rs, rbias=p["br"] if g.res == "conv" else None, B=adjs[i])
        st = g.spec_t
        u = nv.conv([nv.Group(z, gt._tcn_weight(g, p["wt"]), st.wv, C, st.taps, nv.TAP_TIME, 1, False, None)], n, C, g.T, g.V,
                    bias0=p["bt"])
        x = nv.affine_act(u, ct[0] if ct is not None else None, ct[1] if ct is not None else None, r,
                          cr[0] if cr is not None else None, cr[1] if cr is not None else None,
                          noise[i], p["nw"].reshape(-1), g.act, gt.SLOPE)
    return x


class Sampler:
    """generate.py's sampling loop on the inference-only HIP path.  One ``next()`` is one round of the reference's loop:
    ``qtd`` samples of every requested class (all for ``label == -1``), labels in generate.py:91's order.

    ``trunc_mode``: '-' none, 'z' Z-space (generate.py:14-21), 'w' W-space (generator.py:97-108); the truncation mean is
    re-estimated from ``mean_size`` fresh draws on every call, as the reference does.  ``fixed_z``: one latent point for
    every sample (generate.py:80-83; only the injected noise then differs between samples).  ``use_graph``: ``next()``
    replays a captured hipGraph (single stream, no parallel branches); False runs the same launches eagerly.

    The Sampler reads ``G`` through pointers and never writes to it: the ``training`` flag, parameters, running
    statistics and ``num_batches_tracked`` stay as they are, and updates made between calls (an optimiser step on the
    flat parameter buffer, BatchNorm statistics of training replays) are seen by the next call.  Build it after the
    parameters have moved to their final storage (``Trainer`` / ``FlatParams``)."""

    def __init__(self, G, qtd: int = 10, label: int = -1, seed: int = 0, trunc: Optional[float] = None, trunc_mode: str = "-",
                 mean_size: int = 1000, fixed_z: Optional[torch.Tensor] = None, use_graph: bool = True):
        if trunc_mode not in ("-", "z", "w"):
            raise ValueError("Sampler: trunc_mode must be '-', 'z' or 'w'")
        if trunc_mode != "-" and trunc is None:
            raise ValueError("Sampler: trunc_mode %r needs a truncation factor" % trunc_mode)
        self.G = G
        self.device = dev = next(G.parameters()).device
        self.n_classes = G.label_emb.num_embeddings
        self.latent = G.mlp.mlp[0].in_features - self.n_classes
        self.classes = list(range(self.n_classes)) if label == -1 else [int(label)]
        self.qtd, self.seed = int(qtd), int(seed)
        self.n = n = self.qtd * len(self.classes)
        self.trunc, self.trunc_mode, self.mean_size = trunc, trunc_mode, int(mean_size)
        self.use_graph = bool(use_graph) and dev.type == "cuda"
        layers = list(G.mlp.mlp)
        if not all(isinstance(m, torch.nn.Linear if i % 2 == 0 else torch.nn.LeakyReLU) for i, m in enumerate(layers)) or \
                len({m.negative_slope for m in layers[1::2]}) != 1:
            raise NotImplementedError("Sampler: the mapping network must be Linear / LeakyReLU pairs with one slope")
        self._linears, self._map_slope = layers[0::2], float(layers[1].negative_slope)
        self.meta = gt.GenTrunkMeta(G, dev)
        self.params, self.bns = gt.collect_params(G)
        if not self.meta.ok:
            raise NotImplementedError("Sampler: a block of this generator has no contract-first form (gen_trunk.GenBlockGeom)")
        for b in (b for pair in self.bns for b in pair if b is not None):
            if b.running_mean is None:
                raise NotImplementedError("Sampler: BatchNorm layers without running statistics have no eval mode")
        # static buffers of a round
        self.labels_np = np.array([c for _ in range(self.qtd) for c in self.classes])
        self.labels = torch.as_tensor(self.labels_np, dtype=torch.long, device=dev)
        self.z = torch.zeros((n, self.latent), dtype=torch.float32, device=dev)
        self.fixed_z = None
        if fixed_z is not None:
            self.fixed_z = fixed_z.detach().to(dev, torch.float32).reshape(1, self.latent).repeat(n, 1).contiguous()
            self.z.copy_(self.fixed_z)
        self.plane_shapes = [(n, 1, g.T, g.V) for g in self.meta.geoms]
        self.noise_flat = torch.zeros(sum(int(np.prod(s)) for s in self.plane_shapes), dtype=torch.float32, device=dev)
        self.noise = self._planes(self.noise_flat)
        dt = {"-": 0, "z": self.latent, "w": self.latent + self.n_classes}[trunc_mode]
        self.t = torch.zeros((self.mean_size, dt), dtype=torch.float32, device=dev) if dt else None
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_count = 0                  # host mirror of step_dev
        self._adj = torch.zeros(self.meta.adj_numel, dtype=torch.float32, device=dev)
        # one coefficient buffer for all BatchNorm layers: (4, C) per layer, in block order
        self._bn_layers = [(i, k, b) for i, pair in enumerate(self.bns) for k, b in enumerate(pair) if b is not None]
        self._coef = torch.zeros(max(1, sum(4 * b.num_features for _, _, b in self._bn_layers)), dtype=torch.float32, device=dev)
        self.coefs, off = [[None, None] for _ in self.bns], 0
        for i, k, b in self._bn_layers:
            self.coefs[i][k] = self._coef[off:off + 4 * b.num_features].view(4, b.num_features)
            off += 4 * b.num_features
        self._graph = None
        self._out = None

    def _planes(self, flat):
        out, off = [], 0
        for shp in self.plane_shapes:
            k = int(np.prod(shp))
            out.append(flat[off:off + k].view(*shp))
            off += k
        return out

    # ---- the launch sequence ---------------------------------------------------------------------------------------
    def _map(self, x, labels):
        """Mapping_Net on x (generator.py:22-37): with ``labels`` the embedding + cat is the first layer's operand load"""
        emb = self.G.label_emb.weight if labels is not None else None
        for i, lin in enumerate(self._linears):
            x = nv.linear_fwd(x, lin.weight, lin.bias, nv.ACT_LRELU, self._map_slope, emb=emb if i == 0 else None,
                              labels=labels if i == 0 else None)
        return x

    def _synthesis(self, z, labels, noise, t):
        """[kg_trunc_lerp on z] -> mapping -> [mapping of t, kg_trunc_lerp on w] -> adjacency -> kg_bn_eval_coef ->
        infer_pass; z is truncated in place in 'z' mode"""
        if self.trunc_mode == "z":
            nv.trunc_lerp(z, t, self.trunc)
        w = self._map(z, labels)
        if self.trunc_mode == "w":
            nv.trunc_lerp(w, self._map(t, None), self.trunc)       # (the reference's truncate: mlp(t) without embedding)
        G, meta = self.G, self.meta
        adjs, jobs = [], []
        learnable = isinstance(G.edge_importance, torch.nn.ParameterList)
        for i, (g, (oa, ob)) in enumerate(zip(meta.geoms, meta.adj_off)):
            k, v, vc = g.K, g.V, g.Vc
            ae = self._adj[oa:oa + k * v * v].view(k, v, v)
            b = self._adj[ob:ob + k * vc * v].view(k, vc, v)
            jobs.append(dict(a=g.A_fixed, imp=G.edge_importance[i].detach() if learnable else None, u=g.U, aeff=ae, b=b))
            adjs.append(b[:g.Kp])
        nv.gen_adj_prepare(jobs)
        bn_jobs = [dict(gamma=b.weight, beta=b.bias, running_mean=b.running_mean, running_var=b.running_var, eps=b.eps,
                        coef=self.coefs[i][k]) for i, k, b in self._bn_layers]
        for q in range(0, len(bn_jobs), nv.BN_EVAL_MAX_JOBS):
            nv.bn_eval_coef(bn_jobs[q:q + nv.BN_EVAL_MAX_JOBS])
        return infer_pass(meta, w, noise, adjs, self.params, self.coefs)

    def _round(self):
        """what a graph holds: the draws of replay ``step_dev`` (advanced by the launch), then the synthesis"""
        nv.sample_inputs(self.step_dev, self._ticket, self.seed, z=None if self.fixed_z is not None else self.z,
                         noise=self.noise_flat, t=self.t)
        if self.fixed_z is not None and self.trunc_mode == "z":
            self.z.copy_(self.fixed_z)          # (the in-place truncation must start from the pinned point every round)
        self._out = self._synthesis(self.z, self.labels, self.noise, self.t)

    def _capture(self):
        """Single-stream capture.  The warm-up rounds in front of it are real draws: the counter is put back."""
        return capture_keeping(self._round, [self.step_dev], self.device)

    @torch.no_grad()
    def next(self):
        """One round.  Returns (imgs (n, C, T, V), labels (n,) int64, z (n, latent)): views of the Sampler's buffers, valid
        until the next call."""
        if self.use_graph:
            if self._graph is None:
                self._graph = self._capture()
            self._graph.replay()
        else:
            self._round()
        self.step_count += 1
        return self._out, self.labels, self.z

    @torch.no_grad()
    def forward(self, z, labels, noise, trunc_t=None):
        """The same schedule, eagerly, on the caller's inputs: z (N, latent), labels (N,) int64, ``noise`` the seven
        (N, 1, T, V) planes, ``trunc_t`` (mean_size, Dt) the truncation draws (required when truncation is on).  The
        inputs are not modified."""
        if self.trunc_mode != "-" and trunc_t is None:
            raise ValueError("Sampler.forward: trunc_mode %r needs trunc_t" % self.trunc_mode)
        z = z.to(self.device, torch.float32)
        z = z.clone() if self.trunc_mode == "z" else z.contiguous()
        t = None if trunc_t is None else trunc_t.to(self.device, torch.float32).contiguous()
        return self._synthesis(z, labels.to(self.device).contiguous(), [q.to(self.device) for q in noise], t)

    def generate(self, gen_qtd: int, keep_on_device: bool = False):
        """``ceil(gen_qtd / qtd)`` rounds; returns (imgs, labels, z) in the shape and order of ``sample_actions`` (every
        class reaches ``gen_qtd`` in the same round, so one captured round serves the whole run)."""
        imgs, labs, zs = [], [], []
        for _ in range(max(1, -(-int(gen_qtd) // self.qtd))):
            out, _, z = self.next()
            # (the buffers are overwritten by the next round: a copy either way)
            imgs.append(out.cpu() if out.is_cuda and not keep_on_device else out.clone())
            zs.append(z.cpu() if z.is_cuda and not keep_on_device else z.clone())
            labs.append(self.labels_np)
        return torch.cat(imgs, 0), np.concatenate(labs, 0), torch.cat(zs, 0)

    def state_dict(self) -> dict:
        return {"seed": self.seed, "step": self.step_count}

    def load_state_dict(self, sd: dict) -> None:
        """Same seed and counter: the same samples bit for bit (the seed is a launch argument: a captured graph is dropped
        when it changes)."""
        if int(sd["seed"]) != self.seed:
            self.seed, self._graph = int(sd["seed"]), None
        self.step_count = int(sd["step"])
        self.step_dev.fill_(self.step_count)
