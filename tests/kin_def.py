"""The float64 definition of the kinematic plausibility scores (include/kgan_hip.h, "kinematic plausibility") in
numpy, the error bracket of a descriptor, and the test data.  Nothing here touches the GPU.

Descriptors of one sample x (C, T, V) fp32, everything in float64 (differences of fp32 values are exact there):
    L[b, f] = |x[:, f, u_b] - x[:, f, v_b]|,  mu_b, sd_b (population, two passes),  s = mean L
    0 bone_cv, 1 asymmetry, 2 speed, 3 accel, 4 jerk, 5 still           (KIN_NAMES)
each rounded once to float32.  Scores of the stored float32 matrices: pairwise-tree means and the exact W1 of the issue.
"""
import numpy as np

KIN_NAMES = ("bone_cv", "asymmetry", "speed", "accel", "jerk", "still")
U = 2.0 ** -53          # unit roundoff of float64
U32 = 2.0 ** -24        # and of float32

NTU_BONES = [(i - 1, j - 1) for i, j in [
    (1, 2), (2, 21), (3, 21), (4, 3), (5, 21), (6, 5), (7, 6), (8, 7), (9, 21), (10, 9),
    (11, 10), (12, 11), (1, 13), (14, 13), (15, 14), (16, 15), (1, 17), (18, 17), (19, 18),
    (20, 19), (22, 8), (23, 8), (24, 12), (25, 12)]]
H36M_BONES = [(1, 2), (2, 3), (0, 1), (4, 5), (5, 6), (0, 4), (0, 7), (7, 8), (8, 9),
              (8, 10), (10, 11), (11, 12), (8, 13), (13, 14), (14, 15)]
# joint-level left / right pairs (zero-based): the source the mirror tables are derived from
NTU_JOINT_PAIRS = [(4, 8), (5, 9), (6, 10), (7, 11), (21, 23), (22, 24), (12, 16), (13, 17), (14, 18), (15, 19)]
H36M_JOINT_PAIRS = [(1, 4), (2, 5), (3, 6), (10, 13), (11, 14), (12, 15)]


def mirror_from_joints(bones, joint_pairs):
    """pairs (a, b) of bone indices, a < b, such that swapping left and right joints maps bone a onto bone b"""
    swap = {}
    for l, r in joint_pairs:
        swap[l], swap[r] = r, l
    key = {frozenset(b): i for i, b in enumerate(bones)}
    out = set()
    for i, (u, v) in enumerate(bones):
        j = key.get(frozenset((swap.get(u, u), swap.get(v, v))))
        if j is not None and j != i:
            out.add((min(i, j), max(i, j)))
    return sorted(out)


def skeleton(name):
    """(C, V, bones, mirror) of the two test skeletons: NTU (3, 25, 24 bones, 10 pairs), H36M (2, 16, 15 bones, 6 pairs)"""
    if name == "ntu":
        return 3, 25, NTU_BONES, mirror_from_joints(NTU_BONES, NTU_JOINT_PAIRS)
    return 2, 16, H36M_BONES, mirror_from_joints(H36M_BONES, H36M_JOINT_PAIRS)


# ---- descriptors -----------------------------------------------------------------------------------------------------------

def _norm(d):
    """Euclidean norm over the channel axis 0"""
    return np.sqrt((d * d).sum(0))


def lengths(x, bones):
    """L (B, T) float64 of one sample x (C, T, V)"""
    x = np.asarray(x, dtype=np.float64)
    b = np.asarray(bones, dtype=np.int64).reshape(-1, 2)
    return _norm(x[:, :, b[:, 0]] - x[:, :, b[:, 1]]).T


def steps(x):
    """(|D1| (T-1, V), |D2| (T-2, V), |D3| (T-3, V)) float64 of one sample"""
    x = np.asarray(x, dtype=np.float64)
    d1 = x[:, 1:] - x[:, :-1]
    d2 = (x[:, 2:] - 2.0 * x[:, 1:-1]) + x[:, :-2]
    d3 = ((x[:, 3:] - 3.0 * x[:, 2:-1]) + 3.0 * x[:, 1:-2]) - x[:, :-3]
    return _norm(d1), _norm(d2), _norm(d3)


def descriptors64(x, bones, mirror, still_eps=1e-3):
    """(six float64 values, degenerate, still count) of one sample"""
    with np.errstate(invalid="ignore", divide="ignore"):
        L = lengths(x, bones)
        mu = L.mean(1)
        sd = np.sqrt(((L - mu[:, None]) ** 2).mean(1))
        s = L.mean()
        if s == 0.0:
            return np.zeros(6), True, 0
        cv = np.where(mu != 0.0, sd / np.where(mu != 0.0, mu, 1.0), 0.0)
        cv = np.where(np.isnan(mu), np.nan, cv)
        out = np.zeros(6)
        out[0] = cv.mean()
        mir = np.asarray(mirror, dtype=np.int64).reshape(-1, 2)
        if len(mir):
            ma, mb = mu[mir[:, 0]], mu[mir[:, 1]]
            den = 0.5 * (ma + mb)
            t = np.where(den != 0.0, np.abs(ma - mb) / np.where(den != 0.0, den, 1.0), 0.0)
            t = np.where(np.isnan(den), np.nan, t)
            out[1] = t.mean()
        v1, v2, v3 = steps(x)
        out[2], out[3], out[4] = v1.mean() / s, v2.mean() / s, v3.mean() / s
        count = int((v1 < still_eps * s).sum())
        out[5] = count / v1.size
        return out, False, count


def descriptors(x, bones, mirror, still_eps=1e-3):
    """x (K, n, C, T, V) -> dict(d64 (K, n, 6), desc (K, n, 6) float32, degenerate (K,), nonfinite (K,), still (K, n))"""
    K, n = x.shape[:2]
    d64, deg, cnt = np.zeros((K, n, 6)), np.zeros((K, n), dtype=bool), np.zeros((K, n), dtype=np.int64)
    for k in range(K):
        for i in range(n):
            d64[k, i], deg[k, i], cnt[k, i] = descriptors64(x[k, i], bones, mirror, still_eps)
    desc = d64.astype(np.float32)
    return dict(d64=d64, desc=desc, degenerate=deg.sum(1).astype(np.int32), still=cnt,
                nonfinite=(~np.isfinite(desc)).any(2).sum(1).astype(np.int32))


def eval_error(x, bones, mirror, d64):
    """Relative bound, per descriptor, on |kernel's fp64 value - this file's fp64 value| of one sample - BOTH evaluations'
    rounding errors, whatever the order of their sums.  With u = 2^-53, C channels, T frames, V joints, B bones, M pairs:
      e_len = (C + 3) u         one length or step norm: C squares, C - 1 adds, a root, the exact differences (D2 / D3: up to 3
                                more roundings when the four terms do not fit one exponent window - counted)
      e_mu  = e_len + T u       a mean of T lengths in any order (first-order bound n u for n terms)
      e_s   = e_len + B T u     the unit s
      bone_cv: sd_b is a root of a mean of (L - mu_b)^2.  An ABSOLUTE error of (e_len + e_mu) mu_b in L - mu_b is a relative
               one of (e_len + e_mu) mu_b / sd_b in sd_b, so sd_b / mu_b carries the absolute error (e_len + e_mu) plus
               (sd_b / mu_b) ((T + 4) u + e_mu); the mean over B bones adds (B + 1) u.  Relative to bone_cv:
               (e_len + e_mu) / bone_cv + (T + 4) u + e_mu + (B + 1) u      - the division by bone_cv of the issue.
      asymmetry: |mu_a - mu_b| has the absolute error e_mu (mu_a + mu_b), so a term has 2 e_mu plus term (e_mu + 3 u);
               relative to the descriptor: 2 e_mu / asymmetry + e_mu + (M + 4) u.
      speed, accel, jerk: (e_len + 3 u) + T V u for the mean, e_s and 2 u for the divisions.
      still: an exact count - no bracket (the caller checks that no step sits at the threshold).
    Each doubled: two evaluations."""
    C, T, V = x.shape
    B, M = len(bones), len(mirror)
    e_len = (C + 3) * U
    e_mu = e_len + T * U
    e_s = e_len + B * T * U
    out = np.zeros(6)
    out[0] = (e_len + e_mu) / d64[0] + (T + 4) * U + e_mu + (B + 1) * U if d64[0] > 0 else np.inf
    out[1] = (2 * e_mu / d64[1] + e_mu + (M + 4) * U if d64[1] > 0 else np.inf) if M else 0.0
    out[2:5] = (e_len + 3 * U) + T * V * U + e_s + 2 * U
    return 2.0 * out


def threshold_margin(x, bones, still_eps=1e-3):
    """the smallest relative distance of a step's |D1| / s from still_eps over one sample (inf when still_eps == 0)"""
    s = lengths(x, bones).mean()
    v1 = steps(x)[0]
    if still_eps == 0 or s == 0:
        return np.inf
    return float(np.abs(v1 / s - still_eps).min() / still_eps)


# ---- scores of stored float32 descriptor matrices -----------------------------------------------------------------------------

def tree_sum(t):
    """pad with +0.0 to the next power of two P, then t[i] += t[i + h] for h = P/2 .. 1"""
    t = np.asarray(t, dtype=np.float64)
    P = 1
    while P < t.size:
        P *= 2
    buf = np.zeros(P)
    buf[:t.size] = t
    h = P // 2
    with np.errstate(invalid="ignore"):
        while h >= 1:
            buf[:h] = buf[:h] + buf[h:2 * h]
            h //= 2
    return buf[0]


def tree_mean(col):
    return tree_sum(np.asarray(col, dtype=np.float32).astype(np.float64)) / np.float64(len(col))


def w1(real, fake):
    """the Wasserstein-1 distance of two float32 samples by the issue's four steps (NaN for a non-finite value)"""
    real, fake = np.asarray(real, dtype=np.float32), np.asarray(fake, dtype=np.float32)
    n, m = real.size, fake.size
    z = np.concatenate([real, fake])
    if not np.isfinite(z).all():
        return np.nan
    side = np.concatenate([np.zeros(n, dtype=np.int64), np.ones(m, dtype=np.int64)])
    order = np.argsort(z, kind="stable")
    z, side = z[order].astype(np.float64), side[order]
    cr = np.cumsum(side == 0)[:-1].astype(np.int64)
    cf = np.cumsum(side == 1)[:-1].astype(np.int64)
    term = np.abs(cr * m - cf * n).astype(np.float64) * (z[1:] - z[:-1])
    return tree_sum(term) / np.float64(n * m)


def scores(real_desc, fake_descs):
    """real_desc (K, n, 6), fake_descs list of (K, m, 6), float32 -> the outputs of kg_kin_scores"""
    real_desc = np.asarray(real_desc, dtype=np.float32)
    K, n, _ = real_desc.shape
    G = len(fake_descs)
    out = dict(mean_real=np.zeros((K, 6)), mean_fake=np.zeros((G, K, 6)), w1=np.zeros((G, K, 6)),
               nonfinite=np.zeros((G + 1, K), dtype=np.int32))
    out["nonfinite"][0] = (~np.isfinite(real_desc)).any(2).sum(1)
    for k in range(K):
        for j in range(6):
            out["mean_real"][k, j] = tree_mean(real_desc[k, :, j])
    for g, fd in enumerate(fake_descs):
        fd = np.asarray(fd, dtype=np.float32)
        out["nonfinite"][g + 1] = (~np.isfinite(fd)).any(2).sum(1)
        for k in range(K):
            for j in range(6):
                out["mean_fake"][g, k, j] = tree_mean(fd[k, :, j])
                out["w1"][g, k, j] = w1(real_desc[k, :, j], fd[k, :, j])
    mean = np.zeros((G, 6))
    with np.errstate(invalid="ignore"):
        for k in range(K):                          # class order
            mean = mean + out["w1"][:, k]
    out["w1_mean"] = mean / np.float64(K)
    out["scores"] = out["w1_mean"].astype(np.float32)
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------

def make_data(seed, K, n, C, T, V, scale=1.0, shift=0.0):
    """(K, n, C, T, V) float32: p0 ~ N(0, 1) per joint, plus a per-joint random walk of step 0.02 and a walk of step 0.05
    shared by the joints of a sample (the body drifts, the bones wobble)"""
    rng = np.random.RandomState(seed)
    p0 = rng.normal(size=(K, n, C, 1, V))
    own = np.cumsum(0.02 * rng.normal(size=(K, n, C, T, V)), axis=3)
    shared = np.cumsum(0.05 * rng.normal(size=(K, n, C, T, 1)), axis=3)
    return ((p0 + own + shared) * scale + shift).astype(np.float32)


def int_skeleton(name, T, seed=0):
    """an integer-valued sample (C, T, V) float32 whose left and right limbs are mirror images (x -> -x) and whose joints
    are all distinct; every length below is exact in float64"""
    C, V, bones, mirror = skeleton(name)
    rng = np.random.RandomState(seed)
    pose = rng.randint(-40, 41, size=(C, V)).astype(np.float64)
    pairs = NTU_JOINT_PAIRS if name == "ntu" else H36M_JOINT_PAIRS
    paired = {j for p in pairs for j in p}
    for v in range(V):
        if v not in paired:
            pose[0, v] = 0.0                      # the trunk lies in the mirror plane
    pose[1] += np.arange(V) * 100                 # no two joints coincide
    for l, r in pairs:
        pose[:, r] = pose[:, l]
        pose[0, l] = abs(pose[0, l]) + 1 + l
        pose[0, r] = -pose[0, l]
    return np.repeat(pose[:, None, :], T, axis=1).astype(np.float32), bones, mirror
