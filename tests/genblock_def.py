"""Float64 definition of the fused generator block (kg_genblock_fwd / _bwd / _infer, include/kgan_hip.h; the reference's
generator.py:168-182), the brackets a correct kernel must land in, and the data and the two case tables of
tests/test_genblock_def_cpu.py and tests/test_genblock_forms_gpu.py.  Test code only: torch ops that run on any device,
nothing of oracle/prim_ref.py is called.

The operation, stage by stage (W_h = [W_gcn[:Kp C]; W_res], j = (tc, vc) on the input grid, t' = tc rep + q on the output grid):
  x   = the finished input, or  pact(pu s_t[g] + b_t[g] + pr s_r[g] + b_r[g] + pnw pnoise),  g = n / (N / groups)      (tail)
  yc  = W_h x                                                                                                         (head)
  z[c, t', w] = sum_k sum_vc yc[k C + c, tc, vc] B[k, vc, w]                                                          (expand)
  r[c, t', w] = sum_vc rs[c, tc, vc] U[vc, w] + b_res[c],  rs = yc's residual rows (conv) | x (identity; no bias)
  u[c, t, w]  = b_tcn[c] + sum_c' sum_d W_tcn[c, c', d] z[c', t + d - 1, w]        (frames outside [0, T) are zero)   (tcn)
  BatchNorm of u / r per batch of N / groups samples: coef (groups, 4, C) = [gamma rstd, beta - mean gamma rstd, mean, rstd],
      rstd = 1 / sqrt(biased var + eps); running statistics take the batches in order, the UNBIASED variance averaged
  out = act(u + r + nw noise)            when the block has no BatchNorm at all (it finishes itself)
  inference: out = act(u s_t + b_t + r s_r + b_r + nw noise) with the coefficients as inputs
  backward:  gp = g act'(out);  du = a_t gp + b_t u + c_t (coef rows 0-2; gp without bn_t), dr likewise (rows 3-5; gp for an
      identity residual);  gz = W_tcn^T (*) du;  zf = gz summed over the repeated frames;  gyc = [fold(gz B_k^T); fold(dr U^T)];
      gx = W_h^T gyc (+ fold(dr U^T) for an identity residual);  with a previous block: gpp = gx pact'(px), the sums
      s0 = sum gpp, s1 = sum gpp (pu - mean_t), s2 = sum gpp (pr - mean_r), s3 = sum gpp pnoise  ->  pcoef (6, Cin) rows
      a = gamma rstd, b = -a rstd (s rstd) / n, c = -a s0 / n - b mean per branch ((1, 0, 0) without BatchNorm), and
      dgamma += s rstd, dbeta += s0, dnw += s3.

Brackets (derived, not measured).  u = 2^-24.  A linear stage is compared with its definition applied to the KERNEL's own
taped input of that stage, so every bracket is a single-stage one of the conv_def.py kind, valid in any summation order:
    |result - ref| <= (n + b) u S + c u |ref|
n = the element's products, S = the same sum over absolute values (plus |bias|), counted per element; b = 2 (second-order part
of the classical bound for n u <= 2^-10, one spare) + 1 where a bias is added outside the chain (`acc + bz`, `v += Brs[c]`) + 1
for the identity residual's `GX[e] += GID[e]`; c = 1 (the stored value).  Counts from csrc/kg_genblock.hip: head n = Cin;
expand n = Kp Vc (z), Vc (r); tcn n = C times the taps whose frame exists; backward gz as tcn; fold n = rep V; gx n = Mh;
zf = `s += gp[q V]` from 0: rep roundings of partial sums <= S.
Where nothing is taped in between - gz inside backward (zf, gyc), the identity residual's fold inside gx, the whole chain of
inference - the input's bracket E is carried through the linear stage by |operator| E in float64 and the stage's own bracket
is added (S then takes |input| + E).
Element-wise stages, counted from the code: the pending tail / inference tail `fmaf(u, s0, b0)`, `v += fmaf(r, s1, b1)`,
`fmaf(w, nz, v)`: 4 roundings of partial sums <= S = |u s0| + |b0| + |r s1| + |b1| + |w nz|; the self-finished tail `v += R`,
`fmaf`: 2.  The activations are 1-Lipschitz; c = 1 + [LeakyReLU's multiply] + 2 TANH_ULP [tanh: conv_def.TANH_ULP, OpenCL's
5 ulp, 1 ulp <= 2 u |ref|].  Backward stage 0: gp = g act'(out) carries 3 u |g| (tanh: `o * o`, `1 - .`, the product; less
for LeakyReLU), du = fmaf(k0, gp, fmaf(k1, u, k2)): |k0| 3 u |g| + 2 u (|k0 gp| + |k1 u| + |k2|).
BatchNorm statistics, from the tree the kernel uses (per-sample two-pass over Nf = T V elements, samples pooled 32 at a time,
chunks merged after Chan et al.), h = N / groups samples, nch = ceil(h / 32) chunks, A = the largest per-sample mean of |x|:
  every computed mean (sample, chunk, running) is a convex combination of sample means, so it is at most A and its error is at
  most E_m = 1.01 (Nf + 33 + 7 nch) u A: Nf roundings for a sample's sum and division, 33 for a chunk's sum of 32 and division,
  7 per merge (delta, nb / n_new, their product - on magnitudes <= 2 A - and the add);
  M2 is a sum of non-negative terms w (difference of two means)^2 and the per-sample centred sums, which with exact means add
  up to the exact M2 (Chan's identity).  A mean off by <= E_m changes a term by <= w (4 |D| E_m + 4 E_m^2); by Cauchy-Schwarz
  sum w |D| <= sqrt(W M2) with W = (2 h + 32) Nf >= the sum of the weights: P = 4 E_m sqrt(W M2) + 4 E_m^2 W.  Every term
  then passes at most K = Nf + 39 + 8 nch roundings on its way to the root (Nf + 2 inside a sample, 4 + 32 in a chunk, 8 per
  merge, the final division), all relative since every term is non-negative:  E_var = (1.01 K u (M2 + P) + P) / (h Nf);
  rstd = 1 / sqrt(var + eps): with E = E_var + u val the error of val = var + eps, rsqrt changes by at most the relative
  1 / sqrt(1 - E / val) - 1 (= E / (2 val), the derivative of rsqrt at val, to first order; E < val / 2 is asserted and the
  float data has var of order 1, where the factor is 1/2) + 11 u for sqrtf and the division (OpenCL's 3 and 2.5 ulp);
  scale = gamma rstd: + u; shift = beta - mean scale: |scale| E_m + |mean| E_scale + 2 u (|beta| + |mean scale|); running statistics, batch by batch: E' = (1 - mom) E + mom E_batch + 3 u (|(1 - mom) r| + |mom v|), the
  unbiased variance var n / (n - 1) with two more roundings.
Tail statistics of the previous block, from the kernel's own gx: s0 .. s3 are sums of n = N Tc Vc products in any order, each
product carrying 3-4 roundings of its own (act', the subtraction of the mean): (n + 4) u S; a, b, c and the sink adds carry
these through the expressions of kg_tail_bwd_branch (1 / n is rounded once) with 1 u per operation.
Every count above is first-order in u; the products of two roundings (a rounding of an already rounded partial sum) are
paid by one factor 1 + 2^-10 on every bracket (SECOND_ORDER: far above (1 + u)^k - 1 - k u for every k used here).
No term of any bracket had to be measured.

Exact cases.  Integer data: x, weights, B, U, biases, coefficients, g, noise small integers (weights sparse: about six
non-zeros per contraction), slope 2^-2, LeakyReLU in place of a forward tanh, tanh's `out` operand in backward from
{0, +-0.5} (act' = 1, 3/4), mean / rstd / gamma of the previous block integers and powers of two.  Every value is a multiple
of 2^-4 and the module asserts per case that 16 S < 2^24 for every S above, so every fp32 operation of every order is exact: every
tape tensor of forward and every backward output equals the definition bit for bit, except the rows that pass a division or
rsqrt (BatchNorm coefficients and running statistics, pcoef's rows), which keep their bracket.

Tables.  TABLE_A: the six compile-time geometries (GB_GEOMETRIES) at N = 4 / groups = 2 and N = 5 / groups = 1; every launch
kind of a case runs in the GbGeo form and under KG_GB_RT=1 - INSTANTIATIONS is the literal list, (6 + 1) per direction.
TABLE_B: the logical edges in the run-time form at the smallest shapes that reach them; a case names the KgGenBlockForm
fields it expects per direction.  On the depth edges of the head contraction: a depth of 48 or 64 is a multiple of 16 and
takes the matrix cores from 17 rows on, so the ragged VALU-32 bucket is entered at depth 44 and its edge K * 32 <= 2048 at
depth 60 (68 is refused; for the tcn 3 C = 63 is taken, 66 refused); the depths 48 and 64 are cases with the path they take.
"""
import math
from typing import NamedTuple, Optional, Tuple

import torch

from tests.conv_def import TANH_ULP, worst_ratio  # noqa: F401  (one tanh bound, one ratio for every *_def module)

ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
U = 2.0 ** -24
SLOPE_EXACT = 0.25
SLOPE_FLOAT = float(torch.tensor(0.2, dtype=torch.float32))          # the value the kernel receives
MOMENTUM = float(torch.tensor(0.1, dtype=torch.float32))
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
DATA_SEED = 7
EXACT_LIMIT = 2.0 ** 24 / 16.0       # 16 S < 2^24 (module docstring)
SB = 32                              # samples the last arriver pools at a time
SECOND_ORDER = 1.0 + 2.0 ** -10      # every bracket is a first-order count of roundings: the products of two of them are below this

# Cin, C, Kp, Tc, Vc, V, rep, residual kind, BatchNorm behind the tcn: GB_GEOMETRIES of csrc/kg_genblock.hip, in its order
GEOMETRIES = [(128, 64, 3, 4, 5, 5, 2, 2, 1), (64, 32, 3, 8, 5, 11, 2, 2, 0), (32, 3, 3, 16, 11, 11, 2, 2, 1),
              (3, 3, 3, 32, 11, 25, 2, 1, 0), (32, 2, 3, 8, 7, 7, 2, 2, 1), (2, 2, 3, 16, 7, 16, 2, 1, 0)]
# every compiled instantiation a launch can reach: (kernel, geometry index | -1 = GbRt)
INSTANTIATIONS = [
    ("fwd", 0), ("fwd", 1), ("fwd", 2), ("fwd", 3), ("fwd", 4), ("fwd", 5), ("fwd", -1),
    ("bwd", 0), ("bwd", 1), ("bwd", 2), ("bwd", 3), ("bwd", 4), ("bwd", 5), ("bwd", -1),
    ("infer", 0), ("infer", 1), ("infer", 2), ("infer", 3), ("infer", 4), ("infer", 5), ("infer", -1),
]
KINDS = ("fwd", "pend", "bwd", "bwdprev", "infer")          # launch kinds: forward from x / from a pending tail, backward
DIR_OF = {"fwd": "fwd", "pend": "fwd", "bwd": "bwd", "bwdprev": "bwd", "infer": "infer"}     # without / with a previous block


class Case(NamedTuple):
    name: str
    N: int
    groups: int
    Cin: int
    C: int
    Kp: int
    Tc: int
    Vc: int
    V: int
    rep: int
    res: int                        # 0 none, 1 identity, 2 conv + BatchNorm
    bn_t: int
    act: int = ACT_LRELU
    up: Optional[bool] = None       # an up-sampling matrix U is given (None: exactly when Vc != V)
    kinds: Tuple[str, ...] = KINDS
    prev: str = "trn"               # the previous block of "bwdprev": t / r = BatchNorm on its tcn / residual branch, n = noise,
                                    # "i" = an identity residual (pr without statistics)
    pend: str = "trn"               # the pending tail of "pend": t / r = coefficient rows given, n = noise
    K: int = 3
    expect: Optional[dict] = None   # {direction: {KgGenBlockForm field: value}}
    rt: bool = True                 # the case runs under KG_GB_RT=1 (TABLE_A runs both forms)
    reject: Tuple[str, ...] = ()    # directions whose form query must answer lds_bytes -1 (or, "dims", the error code)

    @property
    def T(self):
        return self.Tc * self.rep

    @property
    def has_U(self):
        return self.Vc != self.V if self.up is None else self.up

    @property
    def Mg(self):
        return self.Kp * self.C

    @property
    def Mh(self):
        return self.Mg + (self.C if self.res == 2 else 0)

    def geometry(self):
        key = (self.Cin, self.C, self.Kp, self.Tc, self.Vc, self.V, self.rep, self.res, self.bn_t)
        return GEOMETRIES.index(key) if key in GEOMETRIES else -1

    def act_for(self, integer, kind):
        """forward tanh is not exact: integer launches of forward / inference take LeakyReLU instead"""
        return ACT_LRELU if (integer and self.act == ACT_TANH and DIR_OF[kind] != "bwd") else self.act


def slope_of(integer):
    return SLOPE_EXACT if integer else SLOPE_FLOAT


# ---- the path rule, written from the header's description (a second statement of gb_use_mfma / path_ok, for the tables) ----
def use_mfma(M, K, N, at):
    return (at or K % 16 == 0) and (M >= 17 or N >= 64)


def bucket(M):
    return 4 if M <= 4 else 16 if M <= 16 else 32


def paths(c, direction):
    """-> dict(mfma0, mfma1, mv0, mv1) the case must take in `direction`, or None where a contraction has no path"""
    Nc, Nf = c.Tc * c.Vc, c.T * c.V
    bwd = direction == "bwd"
    M0, K0 = (c.Cin, c.Mh) if bwd else (c.Mh, c.Cin)
    out = {}
    for i, (M, K, N) in enumerate(((M0, K0, Nc), (c.C, 3 * c.C, Nf))):
        m = use_mfma(M, K, N, bwd)
        if not m and not (M <= 32 and K * bucket(M) <= 2048):
            return None
        out["mfma%d" % i], out["mv%d" % i] = int(m), 0 if m else bucket(M)
    return out


# ---- float64 pieces ---------------------------------------------------------------------------------------------------------
def act64(v, act, slope):
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * slope)
    if act == ACT_TANH:
        return torch.tanh(v)
    return v


def dact64(o, act, slope):
    if act == ACT_LRELU:
        return torch.where(o > 0, torch.ones_like(o), torch.full_like(o, slope))
    if act == ACT_TANH:
        return 1.0 - o * o
    return torch.ones_like(o)


def act_c(act):
    return 1 + (act == ACT_LRELU) + (2 * TANH_ULP if act == ACT_TANH else 0)


def head_weight(c, wg, wr):
    w = wg.double().reshape(-1, c.Cin)[:c.Mg]
    return torch.cat([w, wr.double().reshape(c.C, c.Cin)]) if c.res == 2 else w


def op_head(W, x):
    return torch.einsum("mc,nctv->nmtv", W, x)


def op_headT(W, gyc):
    return torch.einsum("mc,nmtv->nctv", W, gyc)


def frames(c, t, mutate=None):
    """output frame -> input-grid frame (t / rep; the mutation repeats one frame late)"""
    idx = torch.arange(c.T, device=t.device)
    if mutate == "repeat":
        idx = (idx + 1).clamp_max(c.T - 1)
    return t[:, :, torch.div(idx, c.rep, rounding_mode="floor")]


def op_expand_z(c, yg, B, mutate=None):
    n = yg.shape[0]
    if mutate == "kswap":
        B = B.flip(0)
    return frames(c, torch.einsum("nkctv,kvw->nctw", yg.reshape(n, c.Kp, c.C, c.Tc, c.Vc), B), mutate)


def op_expand_r(c, src, Um, mutate=None):
    return frames(c, torch.einsum("nctv,vw->nctw", src, Um), mutate)


def tap_count(c, dev):
    """(T,) taps of the 3-tap temporal conv whose frame exists"""
    t = torch.arange(c.T, device=dev)
    return ((t - 1 >= 0).double() + 1.0 + (t + 1 < c.T).double())


def op_tcn(c, wt, z, mutate=None):
    """u[c, t] = sum_c' sum_d wt[c, c', d] z[c', t + d - 1]"""
    zp = torch.nn.functional.pad(z, (0, 0, 1, 1))
    return sum(torch.einsum("oc,nctv->notv", wt[:, :, 2 - d if mutate == "tapflip" else d], zp[:, :, d:d + c.T]) for d in range(3))


def op_tcnT(c, wt, du):
    """gz[c', t] = sum_c sum_d wt[c, c', d] du[c, t + 1 - d]"""
    dp = torch.nn.functional.pad(du, (0, 0, 1, 1))
    return sum(torch.einsum("oc,notv->nctv", wt[:, :, d], dp[:, :, 2 - d:2 - d + c.T]) for d in range(3))


def op_sumrep(c, t):
    n, ch, _, v = t.shape
    return t.reshape(n, ch, c.Tc, c.rep, v).sum(3)


def op_fold_z(c, gz, B):
    n = gz.shape[0]
    return torch.einsum("nctw,kvw->nkctv", op_sumrep(c, gz), B).reshape(n, c.Mg, c.Tc, c.Vc)


def op_fold_r(c, dr, Um):
    return torch.einsum("nctw,vw->nctv", op_sumrep(c, dr), Um)


def lin(n, S, ref, b=2, cc=1):
    return (n + b) * U * S + cc * U * ref.abs()


def um_of(c, o):
    return o["U"].double() if o.get("U") is not None else torch.eye(c.V, dtype=torch.float64, device=o["B"].device)


def vec(t):
    return t.double().view(1, -1, 1, 1)


class Exact:
    """collects the largest S of a case: integer data is exact in every order while 16 S < 2^24"""

    def __init__(self):
        self.smax = 0.0

    def __call__(self, S):
        self.smax = max(self.smax, float(S.abs().max())) if S.numel() else self.smax
        return S


# ---- forward ------------------------------------------------------------------------------------------------------------------
def tail_apply(u, r, ct, cr, noise, nw, act, slope, groups, mutate=None):
    """act(u s_t + b_t + r s_r + b_r + nw noise) with per-batch coefficient rows (groups, 4, C) (None: 1 / 0) -> (ref, bracket, S)"""
    N = u.shape[0]
    grp = torch.div(torch.arange(N, device=u.device), N // groups, rounding_mode="floor")
    if mutate == "grouprow":
        grp = (grp + 1) % groups
    pre = u.double()
    S = torch.zeros_like(pre)
    if ct is not None:
        s, b = ct.double()[grp, 0][:, :, None, None], ct.double()[grp, 1][:, :, None, None]
        pre, S = pre * s + b, (pre * s).abs() + b.abs()
    else:
        S = pre.abs()
    if r is not None:
        rr = r.double()
        if cr is not None:
            s, b = cr.double()[grp, 0][:, :, None, None], cr.double()[grp, 1][:, :, None, None]
            pre, S = pre + rr * s + b, S + (rr * s).abs() + b.abs()
        else:
            pre, S = pre + rr, S + rr.abs()
    if noise is not None and nw is not None:
        t = vec(nw) * noise.double()
        pre, S = pre + t, S + t.abs()
    ref = act64(pre, act, slope)
    return ref, 4 * U * S + act_c(act) * U * ref.abs(), S


def bn_stats(xk, groups, layer, mutate=None):
    """training-mode BatchNorm statistics of xk (N, C, T, V) float64 in `groups` batches -> dict of (ref, bracket) pairs:
    coef (groups, 4, C), running_mean, running_var (C) after the batches in order (module docstring for the brackets)"""
    N, C, T, V = xk.shape
    h, Nf = N // groups, T * V
    nch = (h + SB - 1) // SB
    n_tot = float(h * Nf)
    xg = xk.reshape(groups, h, C, Nf)
    mean = xg.mean((1, 3))                                                   # (groups, C)
    M2 = ((xg - mean[:, None, :, None]) ** 2).sum((1, 3))
    var = M2 / n_tot
    A = xg.abs().mean(3).amax(1)
    E_m = 1.01 * (Nf + 33 + 7 * nch) * U * A
    W = (2 * h + SB) * Nf
    P = 4 * E_m * (W * M2).sqrt() + 4 * E_m ** 2 * W
    E_var = (1.01 * (Nf + 39 + 8 * nch) * U * (M2 + P) + P) / n_tot
    gamma = layer["gamma"].double() if layer.get("gamma") is not None else torch.ones(C, dtype=torch.float64, device=xk.device)
    beta = layer["beta"].double() if layer.get("beta") is not None else torch.zeros(C, dtype=torch.float64, device=xk.device)
    eps, mom = layer["eps"], layer["momentum"]
    val = var + eps
    E_val = E_var + U * val
    assert float((E_val / val).max()) < 0.5, "the statistics are too uncertain for a bracket on rstd: use operands with var of order 1"
    rstd = 1.0 / val.sqrt()
    rel = (1.0 / (1.0 - E_val / val).sqrt() - 1.0) + 11 * U
    scale = gamma * rstd
    E_scale = scale.abs() * (rel + U)
    shift = beta - mean * scale
    E_shift = 1.01 * (scale.abs() * E_m + mean.abs() * E_scale + 2 * U * (beta.abs() + (mean * scale).abs()))
    coef = torch.stack([scale, shift, mean, rstd], 1)
    E_coef = torch.stack([E_scale, E_shift, E_m, rstd * rel], 1)
    rm, rv = layer["running_mean"].double().clone(), layer["running_var"].double().clone()
    E_rm, E_rv = torch.zeros_like(rm), torch.zeros_like(rv)
    ratio = 1.0 if mutate == "biased" else n_tot / max(n_tot - 1.0, 1.0)
    for g in range(groups):
        unb = var[g] * ratio
        E_unb = (E_var[g] + 2 * U * var[g]) * ratio
        E_rm = (1 - mom) * E_rm + mom * E_m[g] + 3 * U * (((1 - mom) * rm).abs() + (mom * mean[g]).abs())
        E_rv = (1 - mom) * E_rv + mom * E_unb + 3 * U * (((1 - mom) * rv).abs() + (mom * unb).abs())
        rm = (1 - mom) * rm + mom * mean[g]
        rv = (1 - mom) * rv + mom * unb
    return dict(coef=(coef, E_coef), running_mean=(rm, E_rm), running_var=(rv, E_rv))


def forward(c, o, kind, slope, act, taped=None, mutate=None):
    """kind "fwd" | "pend" -> ({name: ref}, {name: bracket}, largest S): x (pend), yc, z, r, u, out, ct, cr, and per
    BatchNorm layer t / r: rm_*, rv_*.  taped: the kernel's own x, yc, z, r, u (each stage from the kernel's input of that
    stage); None: the chain of the definition itself."""
    ex = Exact()
    ref, br = {}, {}
    tp = {k: v.double() for k, v in (taped or {}).items() if v is not None}
    if kind == "pend":
        p = o["pend"]
        ref["x"], br["x"], S = tail_apply(p["u"], p.get("r"), p.get("ct"), p.get("cr"), p.get("noise"), p.get("nw"), p["act"], slope,
                                          c.groups, mutate)
        ex(S)
        x = tp.get("x", ref["x"])
    else:
        x = o["x"].double()
    Wh = head_weight(c, o["wg"], o.get("wr"))
    ref["yc"] = op_head(Wh, x)
    S = ex(op_head(Wh.abs(), x.abs()))
    br["yc"] = lin(c.Cin, S, ref["yc"])
    yc = tp.get("yc", ref["yc"])
    B, Um = o["B"].double(), um_of(c, o)
    ref["z"] = op_expand_z(c, yc[:, :c.Mg], B, mutate)
    S = ex(op_expand_z(c, yc[:, :c.Mg].abs(), B.abs()))
    br["z"] = lin(c.Kp * c.Vc, S, ref["z"])
    if c.res != 0:
        src = yc[:, c.Mg:] if c.res == 2 else x
        ref["r"] = op_expand_r(c, src, Um, mutate)
        S = op_expand_r(c, src.abs(), Um.abs())
        if c.res == 2 and o.get("br") is not None and mutate != "nobias":
            ref["r"] = ref["r"] + vec(o["br"])
            S = S + vec(o["br"]).abs()
        ex(S)
        br["r"] = lin(c.Vc, S, ref["r"], b=3)
    z = tp.get("z", ref["z"])
    wt = o["wt"].double().reshape(c.C, c.C, 3)
    ref["u"] = op_tcn(c, wt, z, mutate) + vec(o["bt"])
    S = ex(op_tcn(c, wt.abs(), z.abs()) + vec(o["bt"]).abs())
    br["u"] = lin(c.C * tap_count(c, z.device).view(1, 1, -1, 1), S, ref["u"], b=3)
    uk = tp.get("u", ref["u"])
    rk = tp.get("r", ref.get("r"))
    for key, on, src in (("t", c.bn_t, uk), ("r", c.res == 2, rk)):
        if on:
            st = bn_stats(src, c.groups, o["bn_" + key], mutate)
            ref["c" + key], br["c" + key] = st["coef"]
            ref["rm_" + key], br["rm_" + key] = st["running_mean"]
            ref["rv_" + key], br["rv_" + key] = st["running_var"]
    if not c.bn_t and c.res != 2:
        pre, S = uk, uk.abs()
        if c.res != 0:
            pre, S = pre + rk, S + rk.abs()
        if o.get("noise") is not None and o.get("nw") is not None:
            t = vec(o["nw"]) * o["noise"].double()
            pre, S = pre + t, S + t.abs()
        ex(S)
        ref["out"] = act64(pre, act, slope)
        br["out"] = 2 * U * S + act_c(act) * U * ref["out"].abs()
    return ref, br, ex.smax


def infer(c, o, slope, act, mutate=None):
    """eval mode: out (N, C, T, V) with the brackets carried through the chain -> (ref, bracket, largest S)"""
    ex = Exact()
    x = o["x"].double()
    Wh = head_weight(c, o["wg"], o.get("wr"))
    yc = op_head(Wh, x)
    E_yc = lin(c.Cin, ex(op_head(Wh.abs(), x.abs())), yc)
    B, Um = o["B"].double(), um_of(c, o)
    z = op_expand_z(c, yc[:, :c.Mg], B, mutate)
    ayc = yc.abs() + E_yc
    E_z = op_expand_z(c, E_yc[:, :c.Mg], B.abs()) + lin(c.Kp * c.Vc, ex(op_expand_z(c, ayc[:, :c.Mg], B.abs())), z)
    r = E_r = None
    if c.res != 0:
        src, asrc, E_src = (yc[:, c.Mg:], ayc[:, c.Mg:], E_yc[:, c.Mg:]) if c.res == 2 else (x, x.abs(), torch.zeros_like(x))
        r = op_expand_r(c, src, Um, mutate)
        S = op_expand_r(c, asrc, Um.abs())
        if c.res == 2 and o.get("br") is not None and mutate != "nobias":
            r, S = r + vec(o["br"]), S + vec(o["br"]).abs()
        E_r = op_expand_r(c, E_src, Um.abs()) + lin(c.Vc, ex(S), r, b=3)
    wt = o["wt"].double().reshape(c.C, c.C, 3)
    u = op_tcn(c, wt, z, mutate) + vec(o["bt"])
    S = ex(op_tcn(c, wt.abs(), z.abs() + E_z) + vec(o["bt"]).abs())
    E_u = op_tcn(c, wt.abs(), E_z) + lin(c.C * tap_count(c, z.device).view(1, 1, -1, 1), S, u, b=3)
    ct = None if o.get("ict") is None else o["ict"].unsqueeze(0)
    cr = None if o.get("icr") is None else o["icr"].unsqueeze(0)
    ref, E_tail, S = tail_apply(u, r, ct, cr, o.get("noise"), o.get("nw"), act, slope, 1)
    ex(S)
    E = E_tail + E_u * (ct.double()[0, 0].abs().view(1, -1, 1, 1) if ct is not None else 1.0)
    if r is not None:
        E = E + E_r * (cr.double()[0, 0].abs().view(1, -1, 1, 1) if cr is not None else 1.0)
    return ref, E * (1.0 + 8 * U), ex.smax


# ---- backward -----------------------------------------------------------------------------------------------------------------
def branch_rows(s0, s, st, n, sink_g, sink_b):
    """kg_tail_bwd_branch in float64 with brackets: s0 = (sum gp, bracket), s = (sum gp (x - mean), bracket), st = (gamma, mean, rstd)
    -> rows (a, b, c) and their brackets, the two sinks after the add and theirs"""
    (v0, E0), (v1, E1) = s0, s
    gamma, mean, rstd = (t.double() for t in st)
    inv_n = 1.0 / n
    q, E_q = v1 * rstd, rstd.abs() * E1 + U * (v1 * rstd).abs()
    a = gamma * rstd
    E_a = 2 * U * a.abs()
    b = -a * rstd * q * inv_n
    E_b = 1.01 * ((a * rstd * inv_n).abs() * E_q + 7 * U * b.abs())
    t1 = -a * v0 * inv_n
    cc = t1 - b * mean
    E_c = 1.01 * ((a * inv_n).abs() * E0 + 6 * U * t1.abs() + E_b * mean.abs() + 2 * U * (b * mean).abs() + U * cc.abs())
    dg, db = sink_g.double() + q, sink_b.double() + v0
    return (a, b, cc), (E_a, E_b, E_c), (dg, E_q + U * dg.abs()), (db, E0 + U * db.abs())


def prev_stats(c, o, gx, slope, ex, mutate=None):
    """the previous block's tail statistics from gx (N, Cin, Tc, Vc) float64 -> {name: (ref, bracket)}: pcoef, sink_*"""
    p = o["prev"]
    N, Nc = gx.shape[0], c.Tc * c.Vc
    n = float(N * Nc)
    dx = dact64(p["x"].double(), p["act"], slope)
    gp, agx = gx * dx, gx.abs()
    Cin = c.Cin
    one, zero = torch.ones(Cin, dtype=torch.float64, device=gx.device), torch.zeros(Cin, dtype=torch.float64, device=gx.device)

    def sums(w, aw):
        S = (agx * aw).sum((0, 2, 3))
        ex(S)
        return (gp * w).sum((0, 2, 3)), (n + 4) * U * S

    s0 = sums(torch.ones_like(gx), torch.ones_like(gx))
    out, rows, E_rows = {}, [], []
    for key, src in (("t", p.get("u")), ("r", p.get("r"))):
        st = p.get("bn_" + key)
        if st is None:
            rows += [one, zero, zero]
            E_rows += [zero, zero, zero]
            continue
        m = st[1].double().view(1, -1, 1, 1)
        s = sums(src.double() - m, src.double().abs() + m.abs())
        r3, E3, dg, db = branch_rows(s0, s, st, n, p["sinks"]["gamma_" + key], p["sinks"]["beta_" + key])
        rows += list(r3)
        E_rows += list(E3)
        out["sink_gamma_" + key], out["sink_beta_" + key] = dg, db
    if p.get("noise") is not None:
        v, E = sums(p["noise"].double().expand_as(gx), p["noise"].double().abs().expand_as(gx))
        nwv = p["sinks"]["nw"].double() + v
        out["sink_nw"] = (nwv, E + U * nwv.abs())
    out["pcoef"] = (torch.stack(rows), torch.stack(E_rows))
    return out


def backward(c, o, kind, slope, got=None, mutate=None):
    """kind "bwd" | "bwdprev" -> ({name: ref}, {name: bracket}, largest S): du, dr, zf, gyc, gx, and with a previous block
    pcoef, sink_*.  got: the kernel's own du, dr, gyc, gx (each stage from the kernel's input of that stage)."""
    ex = Exact()
    ref, br = {}, {}
    gt = {k: v.double() for k, v in (got or {}).items() if v is not None}
    g, outp = o["g"].double(), o["out"].double()
    gp = g * dact64(outp, c.act, slope)
    E_gp = 3 * U * g.abs()
    coef = o["coef"].double()

    def ap(x, k0):
        k = [coef[k0 + i].view(1, -1, 1, 1) for i in range(3)]
        S = ex((k[0] * gp).abs() + (k[1] * x).abs() + k[2].abs())
        return k[0] * gp + k[1] * x + k[2], k[0].abs() * E_gp + 2 * U * S

    ex(gp)
    ref["du"], br["du"] = ap(o["u"].double(), 0) if c.bn_t else (gp, E_gp)
    if c.res != 0:
        ref["dr"], br["dr"] = ap(o["r"].double(), 3) if c.res == 2 else (gp, E_gp)
    du = gt.get("du", ref["du"])
    dr = (gt.get("dr", ref["dr"]) if (c.res == 2 or c.bn_t) else du) if c.res != 0 else None     # no BatchNorm at all: dr is du
    wt = o["wt"].double().reshape(c.C, c.C, 3)
    gz = op_tcnT(c, wt, du)
    S_gz = ex(op_tcnT(c, wt.abs(), du.abs()))
    E_gz = lin(c.C * tap_count(c, du.device).view(1, 1, -1, 1), S_gz, gz)
    agz = gz.abs() + E_gz
    ref["zf"] = op_sumrep(c, gz)
    br["zf"] = op_sumrep(c, E_gz) + c.rep * U * op_sumrep(c, agz) + U * ref["zf"].abs()
    B, Um = o["B"].double(), um_of(c, o)
    gy = op_fold_z(c, gz, B)
    E_gy = op_fold_z(c, E_gz, B.abs()) + lin(c.rep * c.V, ex(op_fold_z(c, agz, B.abs())), gy)
    gid = E_gid = None
    if c.res != 0:
        gid = op_fold_r(c, dr, Um)
        E_gid = lin(c.rep * c.V, ex(op_fold_r(c, dr.abs(), Um.abs())), gid)
    ref["gyc"], br["gyc"] = (torch.cat([gy, gid], 1), torch.cat([E_gy, E_gid], 1)) if c.res == 2 else (gy, E_gy)
    gyc = gt.get("gyc", ref["gyc"])
    Wh = head_weight(c, o["wg"], o.get("wr"))
    ref["gx"] = op_headT(Wh, gyc)
    S = op_headT(Wh.abs(), gyc.abs())
    if mutate == "ragged":                  # the zero-filled k = Mh of the ragged last chunk kept: A(m, 0) * B(Mh - 1)
        ref["gx"] = ref["gx"] + torch.einsum("c,ntv->nctv", Wh[0], gyc[:, c.Mh - 1])
    if c.res == 1:
        ref["gx"] = ref["gx"] + gid
        br["gx"] = lin(c.Mh, ex(S + gid.abs() + E_gid), ref["gx"], b=3) + E_gid
    else:
        br["gx"] = lin(c.Mh, ex(S), ref["gx"])
    if kind == "bwdprev":
        for k, (v, E) in prev_stats(c, o, gt.get("gx", ref["gx"]), slope, ex, mutate).items():
            ref[k], br[k] = v, E
    return ref, br, ex.smax


# ---- data -------------------------------------------------------------------------------------------------------------------
def operands(c, kind, seed, integer):
    """dict of CPU fp32 tensors for one launch of `kind` (module docstring: integer data is exact)"""
    gen = torch.Generator().manual_seed(seed)

    def ints(*shape, lo=-2, hi=2):
        return torch.randint(lo, hi + 1, shape, generator=gen).float()

    def draw(*shape, scale=1.0, lo=-2, hi=2):
        return ints(*shape, lo=lo, hi=hi) if integer else torch.randn(*shape, generator=gen) * scale

    def weight(*shape, fan):
        if not integer:
            return torch.randn(*shape, generator=gen) / math.sqrt(fan)
        keep = (torch.rand(*shape, generator=gen) < min(1.0, 6.0 / fan)).float()
        return ints(*shape, lo=-1, hi=1) * keep

    def positive(*shape):
        """gamma, running_var: ints 1 .. 2 / uniform 0.5 .. 1.5"""
        return ints(*shape, lo=1, hi=2) if integer else torch.rand(*shape, generator=gen) + 0.5

    N, Cin, C, T, V, Tc, Vc = c.N, c.Cin, c.C, c.T, c.V, c.Tc, c.Vc
    o = dict(wg=weight(c.K * C, Cin, fan=Cin), wt=weight(C, C, 3, fan=3 * C), bt=draw(C, lo=-1, hi=1))
    if c.res == 2:
        o["wr"], o["br"] = weight(C, Cin, fan=Cin), draw(C, lo=-1, hi=1)
    o["B"] = ints(c.Kp, Vc, V, lo=0, hi=1) if integer else torch.rand(c.Kp, Vc, V, generator=gen) / math.sqrt(Vc)
    if c.has_U:
        o["U"] = ints(Vc, V, lo=0, hi=1) if integer else torch.rand(Vc, V, generator=gen) * (2.0 / math.sqrt(Vc))
    if kind in ("fwd", "pend", "infer"):
        o["noise"], o["nw"] = draw(N, 1, T, V, lo=-1, hi=1), draw(C, scale=0.3, lo=-1, hi=1)
        for key, on in (("t", c.bn_t), ("r", c.res == 2)):
            if on and kind != "infer":
                o["bn_" + key] = dict(gamma=positive(C), beta=draw(C, lo=-1, hi=1), running_mean=draw(C), running_var=positive(C),
                                      num_batches_tracked=torch.tensor(3, dtype=torch.int64), momentum=MOMENTUM, eps=EPS)
    if kind in ("fwd", "infer"):
        o["x"] = draw(N, Cin, Tc, Vc)
    if kind == "infer":
        if c.bn_t:
            o["ict"] = torch.stack([positive(C), draw(C, lo=-1, hi=1), draw(C), positive(C)])
        if c.res == 2:
            o["icr"] = torch.stack([positive(C), draw(C, lo=-1, hi=1), draw(C), positive(C)])
    if kind == "pend":
        p = dict(u=draw(N, Cin, Tc, Vc, lo=-1, hi=1), act=ACT_LRELU if integer else (ACT_TANH if c.act == ACT_TANH else ACT_LRELU))
        if "r" in c.pend or "i" in c.pend:
            p["r"] = draw(N, Cin, Tc, Vc, lo=-1, hi=1)
        if "t" in c.pend:
            p["ct"] = draw(c.groups, 4, Cin, scale=0.5, lo=-1, hi=1)
        if "r" in c.pend:
            p["cr"] = draw(c.groups, 4, Cin, scale=0.5, lo=-1, hi=1)
        if "n" in c.pend:
            p["noise"], p["nw"] = draw(N, 1, Tc, Vc, lo=-1, hi=1), draw(Cin, scale=0.2, lo=-1, hi=1)
        o["pend"] = p
    if kind in ("bwd", "bwdprev"):
        o["g"] = draw(N, C, T, V)
        if integer:
            o["out"] = ints(N, C, T, V, lo=-1, hi=1) * 0.5
        else:
            o["out"] = torch.tanh(torch.randn(N, C, T, V, generator=gen))
        o["u"], o["r"] = draw(N, C, T, V, scale=1.5), draw(N, C, T, V)
        o["coef"] = draw(6, C, lo=-1, hi=1)
    if kind == "bwdprev":
        def stats():
            if integer:
                return ints(Cin, lo=1, hi=2), ints(Cin, lo=-1, hi=1), 2.0 ** ints(Cin, lo=-1, hi=1)
            return torch.rand(Cin, generator=gen) + 0.5, torch.randn(Cin, generator=gen) * 0.3, torch.rand(Cin, generator=gen) + 0.5
        px = ints(N, Cin, Tc, Vc, lo=-1, hi=1) * 0.5 if integer else torch.tanh(torch.randn(N, Cin, Tc, Vc, generator=gen))
        p = dict(x=px, act=ACT_LRELU if c.act != ACT_TANH else ACT_TANH, sinks={})
        if "t" in c.prev:
            p["u"], p["bn_t"] = draw(N, Cin, Tc, Vc, lo=-1, hi=1), stats()
        if "r" in c.prev:
            p["r"], p["bn_r"] = draw(N, Cin, Tc, Vc, lo=-1, hi=1), stats()
        elif "i" in c.prev:
            p["r"] = draw(N, Cin, Tc, Vc, lo=-1, hi=1)
        if "n" in c.prev:
            p["noise"] = draw(N, 1, Tc, Vc, lo=-1, hi=1)
        p["sinks"] = {k: torch.full((Cin,), 0.25) for k in ("gamma_t", "beta_t", "gamma_r", "beta_r", "nw")}
        o["prev"] = p
    return o


def reference(c, o, kind, integer, got=None, mutate=None):
    """-> ({name: ref}, {name: bracket}) of one launch; on integer data the definition's own chain (got ignored except for the
    rows that keep a bracket) and the assertion that the case is exact in fp32"""
    slope, act = slope_of(integer), c.act_for(integer, kind)
    if kind == "infer":
        r, b, smax = infer(c, o, slope, act, mutate)
        ref, br = {"out": r}, {"out": b}
    elif kind in ("fwd", "pend"):
        ref, br, smax = forward(c, o, kind, slope, act, None if integer else got, mutate)
        if integer and got is not None:         # the statistics rows keep their bracket: from the kernel's (= the exact) tape
            r2, b2, _ = forward(c, o, kind, slope, act, got, mutate)
            for k in r2:
                if k[:2] in ("ct", "cr", "rm", "rv"):
                    ref[k], br[k] = r2[k], b2[k]
    else:
        ref, br, smax = backward(c, o, kind, slope, None if integer else got, mutate)
    if integer:
        assert smax < EXACT_LIMIT, "%s %s: integer data is not exact, largest S = %g" % (c.name, kind, smax)
    return ref, {k: v * SECOND_ORDER for k, v in br.items()}


BRACKETED_ON_INTEGERS = ("ct", "cr", "rm_t", "rv_t", "rm_r", "rv_r", "pcoef")


# ---- tables -------------------------------------------------------------------------------------------------------------------
def _table_a():
    out = []
    for gi, (Cin, C, Kp, Tc, Vc, V, rep, res, bn) in enumerate(GEOMETRIES):
        for N, groups in ((4, 2), (5, 1)):
            act = ACT_TANH if (not bn and res == 1) else ACT_LRELU           # the self-finishing last blocks end in tanh
            out.append(Case("g%d-N%dg%d" % (gi, N, groups), N, groups, Cin, C, Kp, Tc, Vc, V, rep, res, bn, act=act, rt=False))
    return out


TABLE_A = _table_a()

F, P, Bk, BP, I = "fwd", "pend", "bwd", "bwdprev", "infer"
VALU = lambda i, mv: {"mfma%d" % i: 0, "mv%d" % i: mv}        # noqa: E731
MFMA = lambda i: {"mfma%d" % i: 1, "mv%d" % i: 0}             # noqa: E731


def _both(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


TABLE_B = [
    # ---- head contraction rows: 16 (VALU-16) against 17 (matrix cores) below 64 columns; the tcn with C = 16 and Nf < 64
    Case("rows16", 3, 1, 16, 16, 1, 4, 5, 5, 2, 0, 1, expect={"fwd": _both(VALU(0, 16), VALU(1, 16)), "bwd": _both(VALU(0, 16), VALU(1, 16))}),
    Case("rows17", 3, 1, 16, 17, 1, 4, 5, 5, 2, 0, 1, expect={"fwd": _both(MFMA(0), VALU(1, 32)), "bwd": _both(VALU(0, 16), MFMA(1))}),
    # ---- head contraction columns: Nc = 63 / 64 at 4 and 12 rows
    Case("cols63-m4", 2, 1, 16, 4, 1, 9, 7, 7, 1, 0, 1, kinds=(F, Bk, I), expect={"fwd": VALU(0, 4), "infer": VALU(0, 4), "bwd": VALU(0, 16)}),
    Case("cols64-m4", 2, 1, 16, 4, 1, 8, 8, 8, 1, 0, 1, kinds=(F, Bk, I), expect={"fwd": MFMA(0), "infer": MFMA(0), "bwd": MFMA(0)}),
    Case("cols63-m12", 2, 1, 16, 4, 3, 9, 7, 7, 1, 0, 0, kinds=(F, Bk, I), expect={"fwd": VALU(0, 16), "bwd": VALU(0, 16)}),
    Case("cols64-m12", 2, 1, 16, 4, 2, 8, 8, 8, 1, 2, 1, kinds=(F, Bk, I), expect={"fwd": MFMA(0), "bwd": MFMA(0)}),
    # ---- head contraction depth: ragged K in the three VALU buckets, the bucket-32 edge K * 32 <= 2048, and the depths that are
    #      multiples of 16 (module docstring)
    Case("depth12-m4", 2, 1, 12, 4, 1, 3, 5, 5, 2, 0, 1, kinds=(F, P, Bk), expect={"fwd": VALU(0, 4)}),
    Case("depth20-m12", 2, 1, 20, 4, 3, 3, 5, 5, 2, 0, 1, kinds=(F, Bk), expect={"fwd": VALU(0, 16)}),
    Case("depth44-m20", 2, 1, 44, 20, 1, 3, 5, 5, 1, 0, 0, kinds=(F, Bk), expect={"fwd": VALU(0, 32), "bwd": MFMA(0)}),
    Case("depth60-m32", 2, 1, 60, 16, 1, 3, 5, 5, 1, 2, 0, kinds=(F, Bk), expect={"fwd": VALU(0, 32)}),
    Case("depth48-m20", 2, 1, 48, 20, 1, 3, 5, 5, 1, 0, 0, kinds=(F,), expect={"fwd": MFMA(0)}),
    Case("depth64-m32", 2, 1, 64, 16, 1, 3, 5, 5, 1, 2, 0, kinds=(F,), expect={"fwd": MFMA(0)}),
    Case("depth68-m20-refused", 2, 1, 68, 20, 1, 3, 5, 5, 1, 0, 0, kinds=(), reject=("fwd", "infer")),
    Case("rows33-ragged-refused", 2, 1, 12, 11, 3, 3, 5, 5, 1, 0, 0, kinds=(), reject=("fwd", "infer")),
    Case("tcn-c21-edge", 2, 1, 16, 21, 1, 2, 5, 5, 1, 0, 1, kinds=(F, Bk), expect={"fwd": VALU(1, 32)}),
    Case("tcn-c22-refused", 2, 1, 16, 22, 1, 2, 5, 5, 1, 0, 1, kinds=(), reject=("fwd", "infer")),
    # ---- tcn: C = 16 at Nf >= 64 (a matrix-core tile whose upper half-wave has no valid row), C = 3, C = 48 (second row tile ragged)
    Case("tcn-c16-nf70", 2, 1, 16, 16, 1, 7, 5, 5, 2, 1, 1, expect={"fwd": MFMA(1), "bwd": MFMA(1), "infer": MFMA(1)}),
    Case("tcn-c3-nf66", 2, 1, 8, 3, 3, 3, 11, 11, 2, 2, 1, act=ACT_TANH, expect={"fwd": VALU(1, 4), "bwd": MFMA(1)}),
    Case("tcn-c48", 2, 2, 16, 48, 1, 2, 5, 5, 1, 0, 1, kinds=(F, Bk, BP), expect={"fwd": MFMA(1), "bwd": MFMA(1)}),
    # ---- backward, transposed-operand form with a ragged / short K = Mh
    Case("at-mh8", 2, 1, 32, 8, 1, 3, 5, 5, 2, 0, 1, kinds=(Bk, BP), expect={"bwd": MFMA(0)}),
    Case("at-mh20", 2, 1, 32, 5, 3, 3, 5, 5, 2, 2, 1, kinds=(Bk, BP), expect={"bwd": MFMA(0)}),
    Case("at-mh3", 2, 1, 32, 3, 1, 3, 5, 5, 2, 0, 1, kinds=(Bk, BP), expect={"bwd": MFMA(0)}),
    # ---- columns Nc = Nf in {1, 21, 33, 65}
    Case("cols1", 3, 1, 16, 16, 2, 1, 1, 1, 1, 2, 1, kinds=(F, P, Bk, BP)),
    Case("cols21", 2, 1, 16, 16, 2, 3, 7, 7, 1, 2, 1),
    Case("cols33", 2, 1, 16, 16, 2, 3, 11, 11, 1, 2, 1),
    Case("cols65", 2, 1, 16, 16, 2, 5, 13, 13, 1, 2, 1, expect={"fwd": _both(MFMA(0), MFMA(1))}),
    # ---- the single-vertex block: Tc = Vc = V = 1, one acting partition, four repeated frames
    Case("single-vertex-rep4", 4, 2, 32, 32, 1, 1, 1, 1, 4, 2, 1, kinds=(F, P, Bk, BP)),
    # ---- 32 vertices with and without U; 33 is the error code
    Case("v32", 2, 1, 4, 4, 3, 2, 32, 32, 2, 1, 1),
    Case("v32-U", 2, 1, 8, 4, 3, 2, 32, 32, 2, 2, 0, up=True),
    Case("v33-error", 2, 1, 4, 4, 3, 2, 33, 33, 2, 1, 1, kinds=(), reject=("dims",)),
    # ---- rep 1 .. 4 (2 and 4 above), every residual kind with and without bn_t, both activations
    Case("rep3", 2, 1, 8, 8, 3, 2, 3, 5, 3, 1, 1, act=ACT_TANH),
    Case("res0-bn0", 2, 1, 8, 6, 3, 3, 3, 5, 1, 0, 0, act=ACT_TANH),
    Case("res0-bn1", 2, 1, 8, 6, 3, 3, 3, 5, 2, 0, 1),
    Case("res1-bn0", 2, 1, 6, 6, 3, 3, 3, 5, 2, 1, 0, act=ACT_TANH),
    Case("res1-bn1", 2, 1, 6, 6, 3, 3, 3, 5, 2, 1, 1),
    Case("res2-bn0", 2, 1, 8, 6, 3, 3, 3, 5, 2, 2, 0),
    Case("res2-bn1", 2, 1, 8, 6, 3, 3, 3, 5, 2, 2, 1, act=ACT_TANH),
    # ---- groups 1 / 2 / 4, one sample per batch, one sample in all
    Case("groups4-N8", 8, 4, 8, 6, 3, 3, 3, 5, 2, 2, 1, kinds=(F, P)),
    Case("groups4-N4", 4, 4, 8, 6, 3, 3, 3, 5, 2, 2, 1, kinds=(F, P)),
    Case("groups2-N2", 2, 2, 8, 6, 3, 3, 3, 5, 2, 2, 1, kinds=(F, P)),
    Case("N1", 1, 1, 8, 6, 3, 3, 3, 5, 2, 2, 1),
    # ---- the merge's chunk boundary: 32, 33 and 65 samples per batch (the tiniest geometry), and two batches of 32
    Case("h32", 32, 1, 4, 4, 1, 1, 2, 2, 1, 2, 1, kinds=(F, BP)),
    Case("h33", 33, 1, 4, 4, 1, 1, 2, 2, 1, 2, 1, kinds=(F, BP)),
    Case("h65", 65, 1, 4, 4, 1, 1, 2, 2, 1, 2, 1, kinds=(F, BP)),
    Case("h32-groups2", 64, 2, 4, 4, 1, 1, 2, 2, 1, 2, 1, kinds=(F, P)),
    # ---- the merge area: 4 groups C = 2048 is taken, one channel more is the error code
    Case("merge-area-2048", 8, 4, 16, 128, 1, 1, 1, 1, 2, 0, 1, kinds=(F,)),
    Case("merge-area-over", 8, 4, 16, 129, 1, 1, 1, 1, 2, 0, 1, kinds=(), reject=("fwd",)),
    # ---- the statistics rows: 2 C = 512 rows are reduced, 544 are refused (the single-pass row map of the partials)
    Case("statrows-512", 3, 1, 16, 256, 1, 1, 1, 1, 1, 2, 1, K=1, kinds=(F, P)),
    Case("statrows-544-refused", 3, 1, 16, 272, 1, 1, 1, 1, 1, 2, 1, K=1, kinds=(), reject=("fwd",)),
    # ---- backward with a previous block: 512 columns / 512 input channels are taken, 528 are the error code; the previous block
    #      with and without its BatchNorm layers and noise
    Case("prev-cols512", 2, 1, 2, 2, 1, 16, 32, 32, 1, 1, 0, kinds=(BP,)),
    Case("prev-cols528-refused", 2, 1, 2, 2, 1, 33, 16, 16, 1, 1, 0, kinds=(), reject=("bwdprev",)),
    Case("prev-cin512", 3, 1, 512, 16, 1, 1, 1, 1, 1, 0, 1, K=1, kinds=(BP,), expect={"bwd": MFMA(0)}),
    Case("prev-cin528-refused", 3, 1, 528, 16, 1, 1, 1, 1, 1, 0, 1, K=1, kinds=(), reject=("bwdprev",)),
    Case("prev-t", 3, 1, 8, 6, 3, 3, 3, 5, 2, 2, 1, kinds=(BP, P), prev="t", pend="t"),
    Case("prev-r", 3, 1, 8, 6, 3, 3, 3, 5, 2, 2, 1, kinds=(BP, P), prev="r", pend="r"),
    Case("prev-identity-noise", 3, 1, 8, 6, 3, 3, 3, 5, 2, 2, 1, kinds=(BP, P), prev="tin", pend="tin"),
    Case("prev-plain", 3, 1, 8, 6, 3, 3, 3, 5, 2, 2, 1, kinds=(BP, P), prev="", pend=""),
    # ---- the 150 KB of LDS: one shape just under and one just over, per direction (found with the layout rule; the CPU test
    #      asserts the byte counts)
    Case("lds-fwd-under", 2, 1, 16, 16, 3, 9, 25, 25, 2, 2, 1, kinds=(F, I)),
    Case("lds-fwd-over", 2, 1, 16, 16, 3, 10, 25, 25, 2, 2, 1, kinds=(), reject=("fwd", "infer")),
    Case("lds-bwd-under", 2, 1, 16, 16, 3, 7, 25, 25, 2, 2, 1, kinds=(Bk,)),
    Case("lds-bwd-over", 2, 1, 16, 16, 3, 8, 25, 25, 2, 2, 1, kinds=(), reject=("bwd",)),
]



def _eligible_kinds(c):
    """inference takes a block with T > 1 and at least 16 input-grid columns only (kg_genblock_infer_lds_bytes)"""
    ok = c.T > 1 and c.Tc * c.Vc >= 16
    return c._replace(kinds=tuple(k for k in c.kinds if k != "infer" or ok))


TABLE_A = [_eligible_kinds(c) for c in TABLE_A]
TABLE_B = [_eligible_kinds(c) for c in TABLE_B]
CASES = {c.name: c for c in TABLE_A + TABLE_B}
assert len(CASES) == len(TABLE_A) + len(TABLE_B)


def launches(table):
    """[(case name, kind)] of every launch of a table"""
    return [(c.name, k) for c in table for k in c.kinds]
