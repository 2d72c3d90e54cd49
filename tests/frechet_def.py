"""Float64 definition of the Frechet pose / motion distance (the formulas of DESIGN.md 18), its error model and the test data
generator.  Test code only: numpy, no GPU, nothing of the product.

One class, a real point set R (P_r, d) and a fake point set F (P_f, d):
  mu_X = mean of the points,  S_X = unbiased covariance (np.cov(rowvar=False): divided by P - 1)
  S_r = V diag(l) V^T, l clamped at 0,  G = V diag(sqrt l)  (G G^T = S_r; it is always the REAL covariance that is decomposed)
  H = sym(G^T S_f G),  e = eigenvalues of H,  T = sum_i sqrt(max(e_i, 0))  (= tr sqrt(S_r S_f))
  FD = |mu_r - mu_f|^2 + tr S_r + tr S_f - 2 T
Points of n samples (C, t, V): pose = the frames x[i, :, f, :] flattened c-major (P = n t); motion = x[i, :, f + 1, :] -
x[i, :, f, :] formed in float64 (P = n (t - 1)); an (N, d) feature matrix is C = 1, t = 1.

Error model (derived, not measured), eps = 2^-52:
  moments      any fp64 summation of P terms |x| <= xmax: every entry of S within tol_S = 4 P eps xmax^2, of mu within
               tol_mu = 4 P eps xmax (products of two fp32 values are exact in fp64)
  eigenvalues  a backward-stable symmetric solver: eigenvalues of H within delta_eig = 64 d eps lambda_max(H)
  moments -> H the moment error moves the eigenvalues of H by at most delta_mom = 2 d tol_S max(lambda_max S_r, lambda_max S_f)
  square roots |sqrt(e + delta) - sqrt(e)| <= min(delta / (2 sqrt e), sqrt delta), so
               tol_tr(e, delta) = sum_i min(delta / (2 sqrt(max(e_i, 0))), sqrt delta)
The sqrt(delta) branch is what a null eigenvalue of a rank-deficient set (P - 1 < d) costs: round-off in every
implementation, numpy included.
"""
import numpy as np

EPS = 2.0 ** -52
TERMS = ("dmu2", "tr_real", "tr_fake", "tr_sqrt")


def points(x, mode="pose"):
    """x (n, C, t, V) -> (P, C*V) float64 points"""
    x = np.asarray(x, dtype=np.float64)
    n, C, t, V = x.shape
    if mode == "motion":
        x = x[:, :, 1:, :] - x[:, :, :-1, :]
    elif mode != "pose":
        raise ValueError(mode)
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(-1, C * V)


def moments(pts):
    """(mu (d,), S (d, d)) of (P, d) points"""
    pts = np.asarray(pts, dtype=np.float64)
    return pts.mean(0), np.atleast_2d(np.cov(pts, rowvar=False))


def trace_sqrt(S_r, S_f):
    """(T, e, lambda_max S_r, lambda_max S_f): T = tr sqrt(S_r S_f) through the eigen-decomposition of S_r"""
    l, V = np.linalg.eigh(S_r)
    l = np.maximum(l, 0.0)
    G = V * np.sqrt(l)[None, :]
    H = G.T @ S_f @ G
    H = 0.5 * (H + H.T)
    e = np.linalg.eigvalsh(H)
    lf = np.linalg.eigvalsh(S_f)
    return float(np.sqrt(np.maximum(e, 0.0)).sum()), e, float(l.max()), float(max(lf.max(), 0.0))


def from_moments(mu_r, S_r, mu_f, S_f):
    """dict(fd, terms (4,), e, lam_r, lam_f, scale) of one class from its moments"""
    T, e, lam_r, lam_f = trace_sqrt(S_r, S_f)
    dmu = mu_r - mu_f
    terms = np.array([dmu @ dmu, np.trace(S_r), np.trace(S_f), T])
    scale = terms[0] + terms[1] + terms[2]
    return dict(fd=scale - 2.0 * T, terms=terms, e=e, lam_r=lam_r, lam_f=lam_f, scale=scale)


def one_class(R, F):
    """R (P_r, d), F (P_f, d) points -> the dict of from_moments plus the moments"""
    mu_r, S_r = moments(R)
    mu_f, S_f = moments(F)
    out = from_moments(mu_r, S_r, mu_f, S_f)
    out.update(mu_real=mu_r, cov_real=S_r, mu_fake=mu_f, cov_fake=S_f)
    return out


def reference(real, fake, mode="pose"):
    """real (K, n, C, t, V), fake (K, m, C, t, V) -> [one_class per class], mean of fd (summed in class order)"""
    per = [one_class(points(real[c], mode), points(fake[c], mode)) for c in range(len(real))]
    s = 0.0
    for p in per:
        s += p["fd"]
    return per, s / len(per)


# ---- error model ---------------------------------------------------------------------------------------------------

def tol_S(P, xmax):
    return 4.0 * P * EPS * xmax * xmax


def tol_mu(P, xmax):
    return 4.0 * P * EPS * xmax


def delta_eig(d, lam_max_H):
    return 64.0 * d * EPS * lam_max_H


def delta_mom(d, tolS, lam_r, lam_f):
    return 2.0 * d * tolS * max(lam_r, lam_f)


def tol_tr(e, delta):
    e = np.maximum(np.asarray(e, dtype=np.float64), 0.0)
    if delta <= 0.0:
        return 0.0
    root = np.sqrt(e)
    with np.errstate(divide="ignore"):
        return float(np.minimum(np.where(root > 0, delta / (2.0 * root), np.inf), np.sqrt(delta)).sum())


def tolerances(ref, P_r, P_f, d, xmax):
    """dict(b, e2e) for one class (the dict of one_class): stage (b) - the trace term on given covariances - and end to
    end from raw data whose points are bounded by xmax"""
    lam_H = float(max(ref["e"].max(), 0.0))
    de = delta_eig(d, lam_H)
    tS, tm = tol_S(max(P_r, P_f), xmax), tol_mu(max(P_r, P_f), xmax)
    dm = delta_mom(d, tS, ref["lam_r"], ref["lam_f"])
    b = tol_tr(ref["e"], de)
    e2e = 2.0 * tol_tr(ref["e"], de + dm) + 2.0 * d * tS + 2.0 * np.sqrt(d) * np.sqrt(ref["terms"][0]) * tm
    return dict(b=b, e2e=e2e, tol_S=tS, tol_mu=tm)


def full_rank(P_r, P_f, d):
    return min(P_r, P_f) >= 4 * d


def caps(P_r, P_f, d, scale):
    """what the tolerances may not exceed (so that they hide nothing): (stage (b), end to end)"""
    return (1e-8 * scale, 1e-5 * scale) if full_rank(P_r, P_f, d) else (1e-4 * scale, 1e-4 * scale)


# ---- data ----------------------------------------------------------------------------------------------------------

def make_class(seed, c, n, m, C, t, V):
    """int8 (q_real (n, C, t, V), q_fake (m, C, t, V)): correlated Gaussian frames, column scales 0.05 .. 1; the fake set is
    mixed a little differently, scaled and shifted"""
    g = np.random.RandomState(1000 * seed + c)
    d = C * V
    mix = g.randn(d, d) / np.sqrt(d)
    col = g.uniform(0.05, 1.0, size=d)
    mix_f = mix + 0.3 * g.randn(d, d) / np.sqrt(d)
    shift = 0.1 * g.randn(d)

    def draw(cnt, M, gain, off):
        z = g.randn(cnt, t, d) @ M * col * gain + off               # (cnt, t, d), |x| mostly below 1
        q = np.clip(np.round(127 * 0.3 * z), -127, 127).astype(np.int8)
        return np.ascontiguousarray(q.reshape(cnt, t, C, V).transpose(0, 2, 1, 3))

    return draw(n, mix, 1.0, 0.0), draw(m, mix_f, 0.9, shift)


def make_data(seed, classes, n, m, C, t, V):
    """(real (K, n, C, t, V), fake (K, m, C, t, V)) float32 numpy, every value q / 127 with q int8: exact in fp32"""
    qs = [make_class(seed, c, n, m, C, t, V) for c in range(classes)]
    real = np.stack([q[0] for q in qs]).astype(np.float32) / np.float32(127)
    fake = np.stack([q[1] for q in qs]).astype(np.float32) / np.float32(127)
    return real, fake


def make_dyadic(seed, n, t, C, V):
    """(n, C, t, V) float32 of multiples of 1 / 128 in [-100, 100] / 128: sums, shifts and small multiples are exact in fp32"""
    g = np.random.RandomState(seed)
    d = C * V
    z = g.randn(n, t, d) @ (g.randn(d, d) / np.sqrt(d)) * g.uniform(0.05, 1.0, size=d)
    q = np.clip(np.round(40 * z), -100, 100)
    return np.ascontiguousarray((q / 128).astype(np.float32).reshape(n, t, C, V).transpose(0, 2, 1, 3))


def closed_form_pairs(n, t, C, V, seed=5):
    """R and {name: F}: identical sets, F = R + b and F = 1.5 R on dyadic data (every value exact in fp32); b (1, C, 1, V)"""
    R = make_dyadic(seed, n, t, C, V)
    b = (np.arange(C * V) % 7 - 3).astype(np.float32).reshape(1, C, 1, V) / np.float32(128)
    return R, b, {"identical": R.copy(), "shift": R + b, "scale": np.float32(1.5) * R}
