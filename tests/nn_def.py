"""Float64 definition of the k-nearest-neighbour search of kg_nn and of the scores built on it, the error model
a correct fp32 kernel must stay inside, and stand-ins for the binding.  Test code only: torch, any device.

For one class, queries (Q, D) and base points (N, D), d2(a, b) = sum_d (a_d - b_d)^2 (prdc_def.sqdist: direct differences):
the k neighbours of query i are the k smallest of {(d2(q_i, b_j), j)} in the order (d2, j) - a STABLE sort of the distances
along j, so ties go to the lower index and a duplicate is a neighbour at 0; exclude_self leaves j == i out by index.

Error model (that of prdc_def): every fp32 distance has relative error at most tau_D = (D + 3) 2^-24.  A query is DECIDED
when every gap among its first k + 1 reference distances exceeds the bound, d_(r+1) (1 - tau) > d_(r) (1 + tau): every
admissible rounding then returns the reference list in the reference order.
"""
import numpy as np
import torch

import prdc_def

tau = prdc_def.tau


def distances(q, b, exclude_self=False):
    """(Q, N) float64 squared distances; the pairs i == j are +inf with exclude_self"""
    d = prdc_def.sqdist(q, b)
    if exclude_self:
        i = torch.arange(min(d.shape), device=d.device)
        d[i, i] = float("inf")
    return d


def knn(q, b, k, exclude_self=False, t=0.0):
    """dict for one class: idx (Q, k) int64, d2 (Q, k) float64, dist (Q, N) float64 (inf where left out); with t > 0 also
    decided (Q,) bool"""
    d = distances(q, b, exclude_self)
    val, order = torch.sort(d, dim=1, stable=True)
    out = dict(idx=order[:, :k].contiguous(), d2=val[:, :k].contiguous(), dist=d)
    if t > 0:
        first = val[:, :k + 1]
        if first.shape[1] == k:                 # k == N: nothing behind the k-th
            first = torch.cat([first, torch.full_like(first[:, :1], float("inf"))], 1)
        out["decided"] = (first[:, 1:] * (1 - t) > first[:, :-1] * (1 + t)).all(1)
    return out


def reference(q, b, k, exclude_self=False, t=0.0):
    """q (K, Q, D), b (K, N, D) -> the dict of knn with a leading class axis on everything"""
    per = [knn(q[c], b[c], k, exclude_self, t) for c in range(q.shape[0])]
    return {key: torch.stack([p[key] for p in per]) for key in per[0]}


def undecided_share(q, b, k, exclude_self=False):
    """the share of queries the error model cannot pin down at this shape: the tests bound it BEFORE looking at the kernel"""
    D = q.shape[-1]
    return 1.0 - reference(q, b, k, exclude_self, tau(D))["decided"].double().mean().item()


def _gather(v, pts, d_outer, d_inner, classes, affine):
    """(classes, pts, D) fp32: what kg_nn reads through a view, its affine applied as two fp32 roundings"""
    x = torch.as_strided(v.t, (classes, pts, d_outer, d_inner), (v.sc, v.sp, v.so, 1), v.t.storage_offset())
    x = x.reshape(classes, pts, d_outer * d_inner).float()
    if affine is not None:
        x = x * torch.tensor(affine[0], dtype=torch.float32, device=x.device)
        x = x + torch.tensor(affine[1], dtype=torch.float32, device=x.device)
    return x


def native_nn(query, base, Q, N, d_outer, d_inner, classes, k, exclude_self=False, q_affine=None, b_affine=None, tile=0,
              split=0, ws=None):
    """the definition behind the signature of _native.nn (any device): (idx (classes, Q, k) int32, d2 fp32)"""
    ref = reference(_gather(query, Q, d_outer, d_inner, classes, q_affine),
                    _gather(base, N, d_outer, d_inner, classes, b_affine), k, exclude_self)
    return ref["idx"].to(torch.int32), ref["d2"].float()


def two_sample(F, R):
    """the leave-one-out 1-NN two-sample test of one class by its definition: F, R (n, D) -> (correct reals, correct fakes);
    the nearest OTHER sample of the union, a tie between a real and a fake neighbour going to the real one"""
    rr, ff = distances(R, R, True).min(1).values, distances(F, F, True).min(1).values
    rf, fr = distances(R, F).min(1).values, distances(F, R).min(1).values
    return int((rr <= rf).sum()), int((ff < fr).sum())


def planted(seed, n_train, n_gen, C, T, V, classes, noise=1e-4):
    """the memorisation case: a training set (prdc_def.make_class of one seed, labels cycling through the classes) and a
    generated set whose FIRST quarter is training samples plus `noise` * N(0, 1) (copies, with the copied sample's label),
    the rest draws of the same model moved by 3 in every coordinate - further from every training sample than any two
    training samples are from each other, so authentic by construction.  float32 numpy: train, lab_train, gen, lab_gen,
    copied (the copied training indices)"""
    D = C * T * V
    pool, _ = prdc_def.make_class(seed, 0, n_train + n_gen, 1, D)
    g = np.random.RandomState(seed + 1000)
    train, fresh = pool[:n_train], pool[n_train:] + 3.0
    lab_train = np.arange(n_train) % classes
    nc = n_gen // 4
    copied = g.permutation(n_train)[:nc]
    gen = fresh.copy()
    gen[:nc] = train[copied] + noise * g.randn(nc, D)
    lab_gen = np.arange(n_gen) % classes
    lab_gen[:nc] = lab_train[copied]
    return (train.astype(np.float32).reshape(n_train, C, T, V), lab_train, gen.astype(np.float32).reshape(n_gen, C, T, V),
            lab_gen, copied)
