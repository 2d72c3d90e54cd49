"""Float64 definition of the reference's MMD evaluation (evaluation/mmd-actions.py:14-115) and of its sample
selection (:131-163), the yardsticks of tests/test_mmd_cpu.py and tests/test_mmd_gpu.py.

    k(a, b) = exp(-|a - b|^2 / bw),  h = kxx + kyy - 2 kxy,  MMD^2 = sum_{i != j} h_ij / (m (m - 1)),  MMD = sqrt(MMD^2)

computed in float64 torch (on whatever device the inputs live); squared distances as |a|^2 + |b|^2 - 2 a.b, clamped at
0 (float64 leaves ~1e-16 |a|^2 of cancellation, far below the tolerances the tests apply).
"""
import math

import numpy as np
import torch

BANDWIDTHS = tuple(10.0 ** j for j in range(-4, 10))


def _sqdist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)).clamp_min(0.0)


def pair_sums_batched(x, y, bandwidths, with_tail=False):
    """x, y (G, m, dim) -> (S, A) float64 (G, nbw): S = sum_{i != j} h_ij, A = sum_{i != j} (kxx + kyy + 2 kxy)
    (the magnitude the roundoff of S is measured against); with_tail: also B = sum_{i != j} (kxx dxx + kyy dyy +
    2 kxy dxy) / bw, the sensitivity of S to a relative error of the squared distances (an fp32 distance of relative
    error e moves k(d) by k d / bw * e: far in the tail, d / bw >> 1, that dominates any fp32 evaluation)"""
    x, y = torch.as_tensor(x).double(), torch.as_tensor(y).double()
    m = x.shape[1]
    off = ~torch.eye(m, dtype=torch.bool, device=x.device)

    def sq(a, b):
        return ((a * a).sum(-1)[:, :, None] + (b * b).sum(-1)[:, None, :] - 2.0 * (a @ b.transpose(1, 2))).clamp_min(0.0)

    dxx, dyy, dxy = sq(x, x), sq(y, y), sq(x, y)
    S, A, B = [], [], []
    for bw in bandwidths:
        kxx, kyy, kxy = (-dxx / bw).exp(), (-dyy / bw).exp(), (-dxy / bw).exp()
        S.append(((kxx + kyy - 2.0 * kxy) * off).sum((1, 2)))
        A.append(((kxx + kyy + 2.0 * kxy) * off).sum((1, 2)))
        B.append(((kxx * dxx + kyy * dyy + 2.0 * kxy * dxy) / bw * off).sum((1, 2)))
    if with_tail:
        return torch.stack(S, 1), torch.stack(A, 1), torch.stack(B, 1)
    return torch.stack(S, 1), torch.stack(A, 1)


def pair_sums(x, y, bandwidths):
    """x, y (m, dim) -> (S, A) float64 (nbw,), see pair_sums_batched"""
    S, A = pair_sums_batched(torch.as_tensor(x)[None], torch.as_tensor(y)[None], bandwidths)
    return S[0], A[0]


def mmd2(x, y, bandwidths):
    """MMD^2 (nbw,) float64; NaN for m = 1 (0 / 0, as the reference)"""
    m = x.shape[0]
    S, _ = pair_sums(x, y, bandwidths)
    return S / (m * (m - 1)) if m > 1 else S * float("nan")


def _sqrt(v: float) -> float:
    return math.sqrt(v) if v >= 0 else float("nan")      # torch's pow(0.5) of a negative number


def sequence_mmd(seq1, seq2, bandwidths, mode):
    """compute_sequence_mmd of (N, L, D) sequences for each bandwidth -> list of floats"""
    seq1, seq2 = torch.as_tensor(seq1).double(), torch.as_tensor(seq2).double()
    n, L, D = seq1.shape
    if mode == "avg":
        per = [mmd2(seq1[:, f], seq2[:, f], bandwidths).tolist() for f in range(L)]
        return [sum(_sqrt(per[f][b]) / L for f in range(L)) for b in range(len(bandwidths))]
    if mode == "joint":
        return [_sqrt(v) for v in mmd2(seq1.reshape(n, L * D), seq2.reshape(n, L * D), bandwidths).tolist()]
    raise Exception("undefined mode")


EPS32 = float(np.finfo(np.float32).eps)


def roundoff(x, y, bws):
    """per bandwidth: MMD^2 (float64) and the fp32 roundoff bound of the reference's sum (a few ulps of the magnitude
    sum_{i != j}(kxx + kyy + 2 kxy) / (m (m-1)), and no less than the bottom of the normal fp32 range)"""
    m = x.shape[0]
    S, A = pair_sums(x, y, bws)
    return (S / (m * (m - 1))).cpu().numpy(), 8 * EPS32 * (A / (m * (m - 1))).cpu().numpy() + 1e-30


def sqrt_err(v, bound):
    """bound on |sqrt(v + e) - sqrt(v)| for |e| <= bound"""
    return np.minimum(np.sqrt(bound), bound / (2 * np.sqrt(np.abs(v)) + 1e-300))


def sequence_roundoff(seq1, seq2, bws, mode):
    """the reference's fp32 roundoff of compute_sequence_mmd (propagated through sqrt and the frame mean) per bandwidth"""
    seq1, seq2 = torch.as_tensor(seq1).double(), torch.as_tensor(seq2).double()
    if mode == "avg":
        return np.mean([sqrt_err(*roundoff(seq1[:, f], seq2[:, f], bws)) for f in range(seq1.shape[1])], 0)
    n = seq1.shape[0]
    return sqrt_err(*roundoff(seq1.reshape(n, -1), seq2.reshape(n, -1), bws))


def class_value(values):
    """the reference's per-class maximum: r = 0, replaced when a value is strictly larger (NaN never wins)"""
    r = 0.0
    for v in values:
        if v > r:
            r = v
    return r


def calculate_mmd(gen, real, labels, mode, bandwidths=BANDWIDTHS):
    """calcualte_mmd on (N, C, T, V) gen / real and class ids -> (mean over classes, per-class values, per-(class, bw))"""
    gen, real = torch.as_tensor(gen), torch.as_tensor(real)
    labels = np.asarray(labels)
    k = int(labels.max()) + 1
    per_bw, per_class = [], []
    for c in range(k):
        i = int(np.flatnonzero(labels == c)[0])
        g0, r0 = gen[i].permute(2, 1, 0), real[i].permute(2, 1, 0)           # (V, T, C), mmd-actions.py:180-181
        vals = sequence_mmd(g0, r0, bandwidths, mode)
        per_bw.append(vals)
        per_class.append(class_value(vals))
    return float(np.mean(per_class)), per_class, per_bw


def select_scan(labels, classes, per_class=100):
    """the selection loop of mmd-actions.py:131-142 written out as the scan it is (one label at a time) -> dataset
    indices in selection order; IndexError where the script would run past the end"""
    out, i, c = [], 0, 0
    while c < len(classes):
        if labels[i] == classes[c]:
            out.append(i)
            if len(out) == per_class * c + per_class:
                c += 1
                i = 0
        i += 1
    return out
