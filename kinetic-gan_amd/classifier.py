"""Action classifier on the critic's kernels: the six ``st_gcn`` blocks of the discriminator as an ST-GCN feature
extractor, a two-layer classification head with softmax cross-entropy on top.

Trained on the user's own dataset (classify.ClassifierLoop) it gives what a raw-coordinate metric cannot: the recognition
accuracy of generated samples against their conditioning label and features for a Frechet distance
(metrics.classifier_scores), the protocol of Action2Motion / ACTOR - without any external weights.

  trunk   disc_trunk.DiscTrunkFn (head=False, label_bias=False, const_channels=0 everywhere): block 0 takes the bare
          ``in_channels`` - no label channels, no ``label_emb``
  head    h (N, latent, T', V') -> pooled = mean_{t,v} h -> feat = lrelu_0.2(fc1 pooled) -> logits = fcn feat
          loss = mean_n (logsumexp(logits_n) - logits_n[y_n]);  pred_n = lowest class index holding the largest logit
          one autograd node (ClsHeadFn) over kg_cls_head_fwd / _bwd / _wgrad
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _native as nv
from . import ops
from .discriminator import _GraphModule, _adjacency_list, st_gcn
from .graph import build_graph

SLOPE = 0.2


class ClsHeadFn(Function):
    """(logits, feat, pred, loss, loss_per_sample, correct) = head(h, labels); ``labels`` None: the last three are None.
    Only ``loss`` is differentiable (first order): its scalar gradient stays on the device (kg_cls_head_bwd reads it there),
    the parameter gradients go to the flat-bucket sink where one is registered, else back to autograd."""

    @staticmethod
    def forward(ctx, h, labels, w1, b1, w2, b2, masked=False):
        out = nv.cls_head_fwd(h.detach(), w1.detach(), b1.detach(), w2.detach(), b2.detach(), labels, SLOPE)
        ctx.set_materialize_grads(False)
        ctx.masked = bool(masked)
        ctx.labels = labels
        ctx.pooled = out["pooled"]
        ctx.save_for_backward(h, w1, b1, w2, b2)
        nd = [out["logits"], out["feat"], out["pred"]]
        if labels is not None:
            nd += [out["loss_per_sample"], out["correct"]]
        ctx.mark_non_differentiable(*nd)
        # (the tensors kept on ctx are not the returned objects' only owners: no output -> grad_fn -> ctx -> output cycle
        # through saved attributes, see disc_trunk.fwd_pass)
        ctx.feat, ctx.logits = out["feat"].detach(), out["logits"].detach()
        return out["logits"], out["feat"], out["pred"], out["loss"], out["loss_per_sample"], out["correct"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logits, g_feat, g_pred, g_loss, g_lps, g_correct):
        if g_loss is None:
            return (None,) * 7
        h, w1, b1, w2, b2 = ctx.saved_tensors
        gtop = g_loss.reshape(1).to(torch.float32).contiguous()
        g, ws = nv.cls_head_bwd(gtop, h, w1, w2, ctx.labels, ctx.feat, ctx.logits, masked=ctx.masked, slope=SLOPE)
        grads = [None] * 4
        if not ops._SKIP_PARAM_GRADS and any(ctx.needs_input_grad[2:6]):
            params = (w1, b1, w2, b2)
            sinks = [ops._sink_of(p) for p in params]
            if all(s is not None for s in sinks):
                nv.cls_head_wgrad(ws, ctx.pooled, ctx.feat, w2.shape[0], *sinks, accumulate=True)
            else:
                outs = [torch.empty(p.numel(), dtype=torch.float32, device=p.device) for p in params]
                nv.cls_head_wgrad(ws, ctx.pooled, ctx.feat, w2.shape[0], *outs, accumulate=False)
                grads = [o.view(p.shape) for o, p in zip(outs, params)]
        return (g if ctx.needs_input_grad[0] else None, None, *grads, None)


class Classifier(_GraphModule):
    def __init__(self, in_channels, n_classes, t_size, latent=512, feat_dim=64, edge_importance_weighting=True,
                 dataset='ntu', **kwargs):
        super().__init__()
        if not 1 <= feat_dim <= nv.FRECHET_MAX_DIM:
            raise ValueError("Classifier: feat_dim=%d outside [1, %d] (the features must fit metrics.frechet_features)"
                             % (feat_dim, nv.FRECHET_MAX_DIM))
        if not (1 <= latent <= nv.CLS_MAX_C and 1 <= n_classes <= nv.CLS_MAX_CLASSES):
            raise ValueError("Classifier: latent / n_classes beyond the head kernel's limits (%d / %d)"
                             % (nv.CLS_MAX_C, nv.CLS_MAX_CLASSES))
        self.graph = build_graph(dataset)
        self.A = _adjacency_list(self.graph)
        spatial_kernel_size = [A.size(0) for A in self.A]
        temporal_kernel_size = [3 for _ in self.A]
        kernel_size = (temporal_kernel_size, spatial_kernel_size)
        self.t_size, self.n_classes, self.feat_dim = t_size, n_classes, feat_dim
        g = self.graph
        # the critic's blocks and arguments (discriminator.Discriminator); block 0 takes the bare input channels
        self.st_gcn_networks = nn.ModuleList((
            st_gcn(in_channels, 32, kernel_size, 1, graph=g, lvl=0, dw_s=True, dw_t=t_size, residual=False, **kwargs),
            st_gcn(32, 64, kernel_size, 1, graph=g, lvl=1, dw_s=False, dw_t=t_size, **kwargs),
            st_gcn(64, 128, kernel_size, 1, graph=g, lvl=1, dw_s=True, dw_t=int(t_size / 2), **kwargs),
            st_gcn(128, 256, kernel_size, 1, graph=g, lvl=2, dw_s=False, dw_t=int(t_size / 4), **kwargs),
            st_gcn(256, 512, kernel_size, 1, graph=g, lvl=2, dw_s=True, dw_t=int(t_size / 8), **kwargs),
            st_gcn(512, latent, kernel_size, 1, graph=g, lvl=3, dw_s=False, dw_t=int(t_size / 16), **kwargs),
        ))
        if edge_importance_weighting:
            self.edge_importance = nn.ParameterList([
                nn.Parameter(torch.ones(self.A[i.lvl].size())) for i in self.st_gcn_networks])
        else:
            self.edge_importance = [1] * len(self.st_gcn_networks)
        self.fc1 = nn.Linear(latent, feat_dim)
        self.fcn = nn.Linear(feat_dim, n_classes)
        self._trunk_cache = {}

    def _trunk_meta(self, T, V, device):
        key = (T, V, str(device))
        meta = self._trunk_cache.get(key)
        if meta is None:
            from .disc_trunk import BlockGeom, TrunkMeta
            geoms, t, v = [], T, V
            for blk in self.st_gcn_networks:
                if not (blk.dw_t <= t and t % blk.dw_t == 0):
                    raise ValueError("Classifier: %d input frames are no whole multiple of the block's %d" % (t, blk.dw_t))
                g = BlockGeom(blk, t, v, device, const_channels=0)
                geoms.append(g)
                t, v = g.t_out, g.W
            meta = TrunkMeta(geoms, [self.A[blk.lvl] for blk in self.st_gcn_networks], head=False, label_bias=False)
            self._trunk_cache[key] = meta
        return meta

    def trunk_params(self):
        """the blocks' parameters in DiscTrunkFn's order"""
        params = []
        for blk in self.st_gcn_networks:
            params += [blk.gcn.conv.weight, blk.tcn.weight, blk.tcn.bias]
            if blk.res_kind == "conv":
                params += [blk.residual.weight, blk.residual.bias]
        return params

    def _trunk(self, x):
        """h (N, latent, T', V') of the last block; without autograd no tape is kept"""
        from .disc_trunk import DiscTrunkFn, MaskedAdjacencyFn, _pack, fwd_pass
        N, C, T, V = x.shape
        meta = self._trunk_meta(T, V, x.device)
        weighted = isinstance(self.edge_importance, nn.ParameterList)
        params = self.trunk_params()
        if not torch.is_grad_enabled():
            ak_all = nv.masked_adj_fwd(meta.A_all, _pack(list(self.edge_importance)), meta.sel) if weighted else meta.A_sel
            h, _ = fwd_pass(meta, x, None, meta.ak_views(ak_all), [p.detach() for p in params], want_xa=False)
            return h
        ak_all = MaskedAdjacencyFn.apply(meta, *self.edge_importance) if weighted else meta.A_sel
        return DiscTrunkFn.apply(meta, x, None, None, ak_all, *params)[0]

    def classify(self, x, labels=None):
        """dict(logits (N, L), features (N, feat_dim), pred (N,) int32) and, with ``labels`` (N,) int64: loss (0-d, the only
        differentiable entry), loss_per_sample (N,), correct (0-d int32).  Everything on the device, no host sync."""
        h = self._trunk(x)
        if labels is not None:
            labels = labels.contiguous()
        logits, feat, pred, loss, lps, correct = ClsHeadFn.apply(h, labels, self.fc1.weight, self.fc1.bias,
                                                                 self.fcn.weight, self.fcn.bias)
        out = dict(logits=logits, features=feat, pred=pred)
        if labels is not None:
            out.update(loss=loss, loss_per_sample=lps, correct=correct)
        return out

    def forward(self, x):
        return self.classify(x)["logits"]

    def features(self, x):
        return self.classify(x)["features"]


def load_classifier(path, device):
    """(Classifier on ``device``, meta) from a ``classifier_<n>.pth`` of tools/train_classifier.py: the state dict plus
    ``meta`` - in_channels, n_classes, t_size, latent, feat_dim, dataset and the training set's normalisation (scale, shift)"""
    sd = torch.load(path, weights_only=False)
    meta = sd.pop("meta")
    clf = Classifier(meta["in_channels"], meta["n_classes"], meta["t_size"], latent=meta["latent"], feat_dim=meta["feat_dim"],
                     dataset=meta["dataset"])
    clf.load_state_dict(sd)
    return clf.to(device), meta


META_MUST_AGREE = ("dataset", "n_classes", "in_channels", "t_size", "scale", "shift")


def check_classifier_meta(meta: dict, run: dict) -> None:
    """ValueError unless the checkpoint's ``meta`` agrees with the run's ``dataset``, ``n_classes``, ``in_channels``, ``t_size``
    and the Feeder's ``scale`` / ``shift``: a classifier trained on another normalisation scores garbage silently"""
    bad = {k: (meta.get(k), run[k]) for k in META_MUST_AGREE if k not in meta or meta[k] != run[k]}
    if bad:
        raise ValueError("the classifier checkpoint disagrees with the run (checkpoint, run): %s" % bad)
