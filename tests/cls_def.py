"""Definitions behind the action-classifier tests (helpers, no tests):

(a) ``head_def``: the classification head's forward / backward / weight gradients in numpy, exactly the formulas of
    include/kgan_hip.h ("action classifier head"), every sum taken in index order.  Evaluated in float64 it is the yardstick
    of the kernels; evaluated in float32 (same order) its distance E to the float64 value sets their tolerance (4 E).
(b) torch emulations of the new native calls, installed on top of oracle/prim_ref.py for the CPU tests (``emulated_native``).
(c) ``OracleClassifier``: the same network assembled from oracle/modules_ref.py and stock ``nn.Linear``.
(d) ``synthetic_set``: the four-class toy set of the learning test.
"""
import contextlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from kinetic_gan_amd import _native
from oracle import modules_ref as M
from oracle import prim_ref
from oracle.graph_tables import load_graph


# ---- (a) the definition ------------------------------------------------------------------------------------------------

def _seq_dot(a, b):
    """(n, k) x (k, m) with the contraction index taken in order, in the operands' dtype"""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=a.dtype)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * b[None, k, :]
    return acc


def _seq_sum(a, axis):
    a = np.moveaxis(a, axis, 0)
    acc = np.zeros(a.shape[1:], dtype=a.dtype)
    for k in range(a.shape[0]):
        acc = acc + a[k]
    return acc


def pred_rule(logits):
    """lowest class index holding the largest logit: start at class 0, replace on a strict '>' (NaN never wins)"""
    out = np.zeros(logits.shape[0], dtype=np.int32)
    for n, row in enumerate(logits):
        best = 0
        for l in range(1, len(row)):
            if row[l] > row[best]:
                best = l
        out[n] = best
    return out


def head_def(h, w1, b1, w2, b2, labels=None, slope=0.2, gtop=None, masked=False, dtype=np.float64):
    """h (N, C, T, V); returns a dict with every output of the three entry points (the backward ones with ``gtop``).  The
    slope is the fp32 value the struct carries."""
    dt = np.dtype(dtype).type
    h, w1, b1, w2, b2 = (np.asarray(t, dtype=dtype) for t in (h, w1, b1, w2, b2))
    N, C, T, V = h.shape
    P, L = T * V, w2.shape[0]
    sl = dt(np.float32(slope))
    pooled = _seq_sum(h.reshape(N, C, P), 2) / dt(P)
    pre = _seq_dot(pooled, w1.T.copy()) + b1[None]
    feat = np.where(pre > 0, pre, pre * sl).astype(dtype)
    logits = (_seq_dot(feat, w2.T.copy()) + b2[None]).astype(dtype)
    out = dict(pooled=pooled, feat=feat, logits=logits, pred=pred_rule(logits))
    if labels is None:
        return out
    y = np.asarray(labels, dtype=np.int64)
    ok = (y >= 0) & (y < L)
    ys = np.where(ok, y, 0)
    with np.errstate(invalid="ignore"):
        m = np.max(np.where(np.isnan(logits), -np.inf, logits), axis=1).astype(dtype)
        e = np.exp(logits - m[:, None]).astype(dtype)
        se = _seq_sum(e, 1)
        lps = (m + np.log(se).astype(dtype)) - logits[np.arange(N), ys]
    lps = np.where(ok, lps, np.nan).astype(dtype)
    out.update(loss_per_sample=lps, loss=mean_in_order(lps), correct=int(np.sum(ok & (out["pred"] == y))))
    if gtop is None:
        return out
    g = dt(gtop)
    onehot = np.zeros((N, L), dtype=dtype)
    onehot[np.arange(N), ys] = 1
    dlogits = ((e / se[:, None] - onehot) * g) / dt(N)
    dlogits = np.where(ok[:, None], dlogits, np.nan).astype(dtype)
    dfeat = (_seq_dot(dlogits, w2) * np.where(feat > 0, dt(1), sl)).astype(dtype)
    dpooled = _seq_dot(dfeat, w1)
    gh = np.repeat((dpooled / dt(P))[:, :, None], P, axis=2).reshape(N, C, T, V)
    if masked:
        gh = gh * np.where(h > 0, dt(1), sl)
    out.update(dlogits=dlogits, dfeat=dfeat, g=gh.astype(dtype),
               dw2=_seq_dot(dlogits.T.copy(), feat), db2=_seq_sum(dlogits, 0),
               dw1=_seq_dot(dfeat.T.copy(), pooled), db1=_seq_sum(dfeat, 0))
    return out


def mean_in_order(lps):
    """the finishing launch: the per-sample losses added in sample-index order in fp64, one division"""
    s = np.float64(0.0)
    for v in np.asarray(lps):
        s = s + np.float64(v)
    return s / np.float64(len(lps))


def workspace_bytes(N, F_, L):
    """the documented formula of kg_cls_head_workspace_bytes: dlogits (N, L) and dfeat (N, F) in fp32"""
    return 4 * N * (L + F_)


# ---- (b) emulations of the native calls ----------------------------------------------------------------------------------

def cls_head_fwd(h, w1, b1, w2, b2, labels=None, slope=0.2):
    n, L = h.shape[0], w2.shape[0]
    pooled = h.mean(dim=(2, 3))
    feat = F.leaky_relu(F.linear(pooled, w1, b1), slope)
    logits = F.linear(feat, w2, b2)
    pred = torch.as_tensor(pred_rule(logits.detach().cpu().numpy()), device=h.device)
    out = dict(pooled=pooled.contiguous(), feat=feat.contiguous(), logits=logits.contiguous(), pred=pred,
               loss_per_sample=None, loss=None, correct=None)
    if labels is not None:
        ok = (labels >= 0) & (labels < L)
        ys = torch.where(ok, labels, torch.zeros_like(labels))
        lps = torch.logsumexp(logits, 1) - logits.gather(1, ys.view(-1, 1)).view(-1)
        lps = torch.where(ok, lps, torch.full_like(lps, float("nan")))
        out.update(loss_per_sample=lps, loss=lps.double().sum().div(n).float(),
                   correct=(ok & (pred.long() == labels)).sum().to(torch.int32))
    return out


def cls_head_bwd(gtop, h, w1, w2, labels, feat, logits, masked=True, slope=0.2):
    n, L = logits.shape
    ok = (labels >= 0) & (labels < L)
    ys = torch.where(ok, labels, torch.zeros_like(labels))
    dl = (torch.softmax(logits, 1) - F.one_hot(ys, L).to(logits.dtype)) * gtop.view(1, 1) / n
    dl = torch.where(ok.view(-1, 1), dl, torch.full_like(dl, float("nan")))
    df = (dl @ w2) * torch.where(feat > 0, torch.ones_like(feat), torch.full_like(feat, slope))
    dp = df @ w1
    g = (dp / float(h.shape[2] * h.shape[3])).view(n, -1, 1, 1).expand_as(h)
    if masked:
        g = g * torch.where(h > 0, torch.ones_like(h), torch.full_like(h, slope))
    return g.contiguous(), torch.cat((dl.reshape(-1), df.reshape(-1)))


def cls_head_wgrad(ws, pooled, feat, n_classes, dw1, db1, dw2, db2, accumulate=True):
    n, L = pooled.shape[0], int(n_classes)
    dl, df = ws[:n * L].view(n, L), ws[n * L:n * L + feat.numel()].view(n, -1)
    for dst, val in ((dw1, df.t() @ pooled), (db1, df.sum(0)), (dw2, dl.t() @ feat), (db2, dl.sum(0))):
        val = val.reshape(dst.shape)
        dst.copy_(dst + val if accumulate else val)


NAMES = ["cls_head_fwd", "cls_head_bwd", "cls_head_wgrad"]


@contextlib.contextmanager
def emulated_native():
    """tests/util.emulated_native plus the classifier head's calls"""
    restore = prim_ref.install(_native)
    saved = {k: getattr(_native, k) for k in NAMES}
    for k in NAMES:
        setattr(_native, k, globals()[k])
    try:
        yield
    finally:
        for k, f in saved.items():
            setattr(_native, k, f)
        restore()


# ---- (c) the host oracle ------------------------------------------------------------------------------------------------

class OracleClassifier(nn.Module):
    """classifier.Classifier in the reference's dense formulation: the critic's six blocks (block 0 on the bare input
    channels), global average pool, Linear + LeakyReLU(0.2), Linear.  Same state_dict keys."""

    def __init__(self, in_channels, n_classes, t_size, latent=512, feat_dim=64, dataset="ntu"):
        super().__init__()
        self.graph = load_graph(dataset)
        self.A = M._adjacency(self.graph)
        ks = ([3 for _ in self.A], [a.size(0) for a in self.A])
        g = self.graph
        self.st_gcn_networks = nn.ModuleList((
            M.DiscBlock(in_channels, 32, ks, 1, graph=g, lvl=0, dw_s=True, dw_t=t_size, residual=False),
            M.DiscBlock(32, 64, ks, 1, graph=g, lvl=1, dw_s=False, dw_t=t_size),
            M.DiscBlock(64, 128, ks, 1, graph=g, lvl=1, dw_s=True, dw_t=int(t_size / 2)),
            M.DiscBlock(128, 256, ks, 1, graph=g, lvl=2, dw_s=False, dw_t=int(t_size / 4)),
            M.DiscBlock(256, 512, ks, 1, graph=g, lvl=2, dw_s=True, dw_t=int(t_size / 8)),
            M.DiscBlock(512, latent, ks, 1, graph=g, lvl=3, dw_s=False, dw_t=int(t_size / 16))))
        self.edge_importance = nn.ParameterList(
            [nn.Parameter(torch.ones(self.A[b.lvl].size())) for b in self.st_gcn_networks])
        self.fc1 = nn.Linear(latent, feat_dim)
        self.fcn = nn.Linear(feat_dim, n_classes)

    def features(self, x):
        for blk, imp in zip(self.st_gcn_networks, self.edge_importance):
            x, _ = blk(x, self.A[blk.lvl].to(x.device) * imp)
        return F.leaky_relu(self.fc1(x.mean(dim=(2, 3))), 0.2)

    def forward(self, x):
        return self.fcn(self.features(x))

    def loss(self, x, labels):
        return F.cross_entropy(self(x), labels)


# ---- (d) the synthetic set of the learning test -----------------------------------------------------------------------------

def synthetic_set(rs_seed, n_classes=4, per_class=8, C=2, T=32, V=16):
    """x = 0.1 N(0, 1), plus 0.6 (1 - 2 (c // 2)) on channel c % 2 at every (t, v) for a sample of class c; drawn from
    RandomState(rs_seed).  Returns (x (n, C, T, V) float32, labels (n,) int64), classes in blocks of ``per_class``."""
    rs = np.random.RandomState(rs_seed)
    labels = np.repeat(np.arange(n_classes), per_class)
    x = 0.1 * rs.randn(len(labels), C, T, V)
    for i, c in enumerate(labels):
        x[i, c % 2] += 0.6 * (1 - 2 * (c // 2))
    return torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(labels, dtype=torch.int64)
