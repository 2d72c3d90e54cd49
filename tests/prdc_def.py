"""Float64 definition of precision / recall / density / coverage (the formulas of DESIGN.md 16), the bracket a correct fp32
kernel must land in, and the test data generator.  Test code only: torch, any device.

For one class, R (n, D) real and F (m, D) fake points, d2(a, b) = sum_d (a_d - b_d)^2:
  rho_R(i) = k-th smallest of {d2(r_i, r_l) : l != i}  (left out by index),  rho_F(j) likewise,
  P_ij = [d2(r_i, f_j) <= rho_R(i)],  Q_ij = [d2(r_i, f_j) <= rho_F(j)],
  cP = #{j : exists i P_ij}, cR = #{i : exists j Q_ij}, cD = sum_ij P_ij, cC = #{i : exists j P_ij},
  precision, recall, density, coverage = cP / m, cR / n, cD / (k m), cC / n.

Error model: with direct differences in fp32 every term of a distance is non-negative, so a computed d2 over D
dimensions has relative error at most tau_D = (D + 3) 2^-24 in any summation order; order statistics are monotone, so a
computed radius has the same bound.  Under the tight predicate d2 (1 + tau) <= rho (1 - tau) a pair is inside for every
admissible rounding, under the loose one d2 (1 - tau) <= rho (1 + tau) it may be: the counts under each are `lo`, `hi`.
"""
import numpy as np
import torch

NAMES = ("precision", "recall", "density", "coverage")


def tau(D):
    return (D + 3) * 2.0 ** -24


def sqdist(a, b, budget=1 << 24):
    """(n, m) float64 squared distances by direct differences (rows in chunks: never more than `budget` elements)"""
    a, b = a.double(), b.double()
    n, D = a.shape
    step = max(1, budget // max(1, b.shape[0] * D))
    return torch.cat([((a[i:i + step, None, :] - b[None, :, :]) ** 2).sum(-1) for i in range(0, n, step)])


def radii(x, k):
    """(n,) k-th smallest squared distance to the OTHER points of the set (the point itself is left out by index)"""
    d = sqdist(x, x)
    d.fill_diagonal_(float("inf"))
    return d.kthvalue(k, dim=1).values


def _counts(P, Q):
    hits = P.sum(0)
    flags = Q.any(1).to(torch.uint8) | (P.any(1).to(torch.uint8) << 1)
    counts = torch.stack([(hits > 0).sum(), Q.any(1).sum(), P.sum(), P.any(1).sum()]).to(torch.int64)
    return counts, hits.to(torch.int64), flags


def one_class(R, F, k, t=0.0):
    """dict for one class.  counts / fake_hits / real_flags / radii under the exact predicate; with t > 0 also the
    tight (`*_lo`) and loose (`*_hi`) versions"""
    R, F = R.double(), F.double()
    rr, rf = radii(R, k), radii(F, k)
    d = sqdist(R, F)
    counts, hits, flags = _counts(d <= rr[:, None], d <= rf[None, :])
    out = dict(counts=counts, fake_hits=hits, real_flags=flags, radii_real=rr, radii_fake=rf)
    if t > 0:
        lo = _counts(d * (1 + t) <= rr[:, None] * (1 - t), d * (1 + t) <= rf[None, :] * (1 - t))
        hi = _counts(d * (1 - t) <= rr[:, None] * (1 + t), d * (1 - t) <= rf[None, :] * (1 + t))
        out.update(counts_lo=lo[0], fake_hits_lo=lo[1], real_flags_lo=lo[2],
                   counts_hi=hi[0], fake_hits_hi=hi[1], real_flags_hi=hi[2])
    return out


def reference(R, F, k, t=0.0):
    """R (K, n, D), F (K, m, D) -> the dict of one_class with a leading class axis on everything"""
    per = [one_class(R[c], F[c], k, t) for c in range(R.shape[0])]
    return {key: torch.stack([p[key] for p in per]) for key in per[0]}


def values_of(counts, n, m, k):
    """(K, 4) float64 values from (K, 4) integer counts"""
    den = torch.tensor([m, n, k * m, n], dtype=torch.float64, device=counts.device)
    return counts.double() / den


def bracket_is_narrow(ref):
    """the condition that keeps the bracket from hiding a failure: hi - lo <= max(1, 0.01 exact) for every count"""
    width = ref["counts_hi"] - ref["counts_lo"]
    cap = torch.clamp((0.01 * ref["counts"].double()).floor().to(torch.int64), min=1)
    return bool((width <= cap).all()), width


def make_class(seed, c, n, m, D):
    """the test data of class c: a 4-dimensional latent mixed into D dimensions, a quarter of the fakes collapsed onto real
    sample 0 (so precision != recall).  float64 numpy (R (n, D), F (m, D))"""
    g = np.random.RandomState(seed + c)
    B = 3 * g.randn(4, D) / np.sqrt(D)
    u_r = g.randn(n, 4)
    u_f = 0.8 * g.randn(m, 4) + 0.3
    u_f[:m // 4] = u_r[0] + 0.05 * g.randn(m // 4, 4)
    R = u_r @ B + 0.01 * g.randn(n, D)
    F = u_f @ B + 0.01 * g.randn(m, D)
    return R, F


def make_data(seed, classes, n, m, D, integer=False):
    """(R (K, n, D), F (K, m, D)) float32 torch (CPU); integer: round(3 x) clipped to [-8, 8] - with D * 256 < 2^24 every fp32
    distance and comparison is exact"""
    Rs, Fs = zip(*(make_class(seed, c, n, m, D) for c in range(classes)))
    R, F = np.stack(Rs), np.stack(Fs)
    if integer:
        R, F = np.clip(np.round(3 * R), -8, 8), np.clip(np.round(3 * F), -8, 8)
    return torch.from_numpy(R.astype(np.float32)), torch.from_numpy(F.astype(np.float32))
