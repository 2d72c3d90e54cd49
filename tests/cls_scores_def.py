"""The float64 definition of kg_cls_scores (include/kgan_hip.h "classifier scores") in numpy, and the in-order
means of a given distance table - what the tests pin the kernel against."""
import numpy as np


def in_order_means(dist, Sd):
    """(diversity, multimodality) of ONE set's distances (Sd + K*Sl,): fp64 sums in index order, one division each"""
    dist = np.asarray(dist, dtype=np.float64)
    sd = np.float64(0.0)
    for v in dist[:Sd]:
        sd = sd + v
    sm = np.float64(0.0)
    for v in dist[Sd:]:
        sm = sm + v
    return sd / np.float64(Sd), sm / np.float64(dist.size - Sd)


def cls_scores_def(feats, preds, labels, div_pairs, mm_pairs, n_classes):
    """feats: S arrays (N, F); preds: S arrays (N,); labels (N,); div_pairs (Sd, 2); mm_pairs (K*Sl, 2).  Returns dict(dist
    (S, Sd + K*Sl) fp64, scores64 (S, 3) fp64, scores (S, 3) fp32, correct (S,), correct_per_class (S, K), count_per_class
    (K,) int32)."""
    K = int(n_classes)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    N = lab.size
    pairs = np.concatenate([np.asarray(div_pairs).reshape(-1, 2), np.asarray(mm_pairs).reshape(-1, 2)]).astype(np.int64)
    Sd = np.asarray(div_pairs).reshape(-1, 2).shape[0]
    S = len(feats)
    dist = np.empty((S, pairs.shape[0]), dtype=np.float64)
    cpc = np.zeros((S, K), dtype=np.int32)
    cnt = np.zeros(K, dtype=np.int32)
    for c in range(K):
        cnt[c] = int((lab == c).sum())
    scores64 = np.empty((S, 3), dtype=np.float64)
    for s in range(S):
        x = np.asarray(feats[s]).astype(np.float64)
        pr = np.asarray(preds[s]).astype(np.int64).reshape(-1)
        for p, (i, j) in enumerate(pairs):
            if 0 <= i < N and 0 <= j < N:
                d = x[i] - x[j]
                dist[s, p] = np.sqrt(np.sum(d * d))
            else:
                dist[s, p] = np.nan
        for c in range(K):
            cpc[s, c] = int(((lab == c) & (pr == c)).sum())
        div, mm = in_order_means(dist[s], Sd)
        scores64[s] = (np.float64(int(cpc[s].sum())) / np.float64(N), div, mm)
    return dict(dist=dist, scores64=scores64, scores=scores64.astype(np.float32), correct=cpc.sum(1).astype(np.int32),
                correct_per_class=cpc, count_per_class=cnt)
