"""Definition of kg_nn_sets and kg_nn_scores.  Test code only.

kg_nn_sets is kg_nn set by set: ``nn_sets_def`` is nn_def.reference per set, nothing else.

kg_nn_scores, per set g and query j with i = idx[g][j], in integers:
    authentic_j = d2[g][j] >= base_loo[i]         (equality is authentic)
    agree_j     = base_labels[i] == query_labels[j]
    counts[g] = (#authentic, #agreeing); counts_per_class[g, c] = the same over the queries whose label is c;
    scores64[g] = counts[g] / Q in float64; scores[g] = its one rounding to float32.
Written in numpy with plain loops over the sets and boolean sums - no shared code with the kernel.
"""
import numpy as np
import torch

import nn_def


def nn_sets_def(queries, b, k, t=0.0):
    """queries: a list of (K, Q, D) tensors, b (K, N, D) -> nn_def.reference of every set, stacked on a leading set axis"""
    per = [nn_def.reference(q, b, k, False, t) for q in queries]
    return {key: torch.stack([p[key] for p in per]) for key in per[0]}


def nn_scores_def(idx, d2, query_labels, base_labels, base_loo, n_classes):
    """idx (nsets, Q) integers, d2 (nsets, Q) float32, query_labels (Q,), base_labels (N,), base_loo (N,) float32 ->
    dict(counts (nsets, 2) int64, counts_per_class (nsets, n_classes, 2) int32, scores64 (nsets, 2), scores (nsets, 2))"""
    idx, d2 = np.asarray(idx).astype(np.int64), np.asarray(d2, dtype=np.float32)
    ql, bl = np.asarray(query_labels).astype(np.int64), np.asarray(base_labels).astype(np.int64)
    loo = np.asarray(base_loo, dtype=np.float32)
    nsets, Q = idx.shape
    counts = np.zeros((nsets, 2), dtype=np.int64)
    per_class = np.zeros((nsets, n_classes, 2), dtype=np.int32)
    scores64 = np.zeros((nsets, 2), dtype=np.float64)
    scores = np.zeros((nsets, 2), dtype=np.float32)
    for g in range(nsets):
        authentic = d2[g] >= loo[idx[g]]
        agree = bl[idx[g]] == ql
        for w, flags in enumerate((authentic, agree)):
            counts[g, w] = int(flags.sum())
            for c in range(n_classes):
                per_class[g, c, w] = int((flags & (ql == c)).sum())
            scores64[g, w] = np.float64(counts[g, w]) / Q
            scores[g, w] = np.float32(np.float64(counts[g, w]) / Q)
    return dict(counts=counts, counts_per_class=per_class, scores64=scores64, scores=scores)
