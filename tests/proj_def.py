"""The float64 definitions of kg_proj_loss / kg_proj_step (include/kgan_hip.h, "projection into W") in numpy, the
error brackets of their outputs, the same objective in torch (for autograd and for the reference loop), and the projection loop
itself on oracle.modules_ref.Generator.  Nothing here touches the GPU.

Objective of one sample, x (C, T, V) fp32 generated, y' (C, T, V) fp32 target, m (T, V) >= 0:
    d = fp32(x - y');  everything after it in float64 (differences of fp32 values are exact there)
    L_pos = sum m d^2 / (C sum m),  L_vel = sum mv (d[t+1] - d[t])^2 / (C sum mv),  L_bone = sum mb (s_x - s_y)^2 / sum mb
    L = (lp L_pos + lv L_vel) + lb L_bone;  a term with lambda 0 or weight sum 0 is 0; a weight that is not > 0 selects its
    entry away (np.where: the other branch may hold NaN, it is never added).
"""
import functools

import numpy as np
import torch

U = 2.0 ** -53
U32 = 2.0 ** -24
F32 = np.float32


def target(y, scale=1.0, shift=0.0):
    """y' = fp32(fp32(y * scale) + shift): two float32 operations"""
    return ((np.asarray(y, dtype=F32) * F32(scale)).astype(F32) + F32(shift)).astype(F32)


def _mask(m, n, T, V):
    if m is None:
        return np.ones((n, T, V))
    m = np.asarray(m, dtype=np.float64)
    return np.broadcast_to(m, (n, T, V)) if m.ndim == 2 else m


def loss_one(x, yp, m, bones, lambdas):
    """one sample: dict(L (4,) float64, g (C, T, V) float64 - the hand-written gradient -, eL (4,), eg (C, T, V): bounds on the
    absolute float64 evaluation error of BOTH evaluations (this one and the kernel's, whatever the order of their sums))"""
    lp, lv, lb = (float(v) for v in lambdas)
    C, T, V = x.shape
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(yp, dtype=np.float64)
    bones = np.asarray(bones, dtype=np.int64).reshape(-1, 2)
    B = len(bones)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(x, dtype=F32) - np.asarray(yp, dtype=F32)).astype(F32).astype(np.float64)
        on = m > 0
        # position
        tp = np.where(on[None], m[None] * d * d, 0.0)
        Wp = C * np.where(on, m, 0.0).sum()
        # velocity
        onv = on[:-1] & on[1:]
        mv = np.where(onv, m[:-1] * m[1:], 0.0)
        e = d[:, 1:] - d[:, :-1]
        tv = np.where(onv[None], mv[None] * e * e, 0.0)
        Wv = C * mv.sum()
        # bones
        a, c = bones[:, 0], bones[:, 1]
        onb = (m[:, a] > 0) & (m[:, c] > 0)                               # (T, B)
        mb = np.where(onb, m[:, a] * m[:, c], 0.0)
        ex, ey = x64[:, :, a] - x64[:, :, c], y64[:, :, a] - y64[:, :, c]   # (C, T, B), exact
        sx, sy = (ex * ex).sum(0), (ey * ey).sum(0)
        df = np.where(onb, sx - sy, 0.0)
        tb = mb * df * df
        Wb = mb.sum()
        onp_, onv_, onb_ = lp > 0 and Wp > 0, lv > 0 and Wv > 0, lb > 0 and Wb > 0
        Lp = tp.sum() / Wp if onp_ else 0.0
        Lv = tv.sum() / Wv if onv_ else 0.0
        Lb = tb.sum() / Wb if onb_ else 0.0
        L = (lp * Lp + lv * Lv) + lb * Lb
        # the hand-written gradient
        cp, cv, cb = (2 * lp / Wp if onp_ else 0.0), (2 * lv / Wv if onv_ else 0.0), (4 * lb / Wb if onb_ else 0.0)
        g = np.zeros((C, T, V))
        ag = np.zeros((C, T, V))                                          # sum of the absolute values of an element's terms
        if onp_:
            t = cp * np.where(on[None], m[None] * d, 0.0)
            g += t
            ag += np.abs(t)
        if onv_:
            t = cv * np.where(onv[None], mv[None] * e, 0.0)
            g[:, 1:] += t
            g[:, :-1] -= t
            ag[:, 1:] += np.abs(t)
            ag[:, :-1] += np.abs(t)
        edf = np.where(onb, (C + 3) * U * (sx + sy), 0.0)                 # absolute error of s_x - s_y
        ebg = np.zeros((C, T, V))
        if onb_:
            t = cb * (mb * df)[None] * ex                                 # (C, T, B)
            te = np.abs(cb * (mb * edf)[None] * ex)
            for b in range(B):
                if a[b] == c[b]:
                    continue
                g[:, :, a[b]] += t[:, :, b]
                g[:, :, c[b]] -= t[:, :, b]
                ag[:, :, a[b]] += np.abs(t[:, :, b])
                ag[:, :, c[b]] += np.abs(t[:, :, b])
                ebg[:, :, a[b]] += te[:, :, b]
                ebg[:, :, c[b]] += te[:, :, b]
        # brackets.  A sum of N non-negative terms, each with k roundings, has the relative error (N + k) u in any order; the
        # weight sums add (T V + 2) u, the division 1 u.  The bone term also carries the cancellation of s_x - s_y.
        eW = (T * max(V, B) + 4) * U
        eL = np.zeros(4)
        eL[1] = (C * T * V + 6) * U * Lp + eW * Lp
        eL[2] = (C * T * V + 8) * U * Lv + eW * Lv
        eL[3] = ((T * B + 8) * U + eW) * Lb + (2 * (mb * np.abs(df) * edf).sum() / Wb if onb_ else 0.0)
        eL[0] = lp * eL[1] + lv * eL[2] + lb * eL[3] + 4 * U * abs(L)
        eg = (eW + (B + 12) * U) * ag + ebg
    return dict(L=np.array([L, Lp, Lv, Lb]), g=g, eL=2.0 * eL, eg=2.0 * eg)


def loss_def(x, y, mask, bones, lambdas, scale=1.0, shift=0.0):
    """x, y (n, C, T, V) fp32; mask None, (T, V) or (n, T, V) -> dict(L64 (n, 4), loss (n, 4) fp32, g64, gx fp32 (n, C, T, V),
    eL, eg: the absolute float64 evaluation error bounds)"""
    x = np.asarray(x, dtype=F32)
    n, C, T, V = x.shape
    yp = target(y, scale, shift)
    m = _mask(mask, n, T, V)
    rows = [loss_one(x[i], yp[i], m[i], bones, lambdas) for i in range(n)]
    out = dict(L64=np.stack([r["L"] for r in rows]), g64=np.stack([r["g"] for r in rows]),
               eL=np.stack([r["eL"] for r in rows]), eg=np.stack([r["eg"] for r in rows]))
    with np.errstate(over="ignore", invalid="ignore"):
        out["loss"], out["gx"] = out["L64"].astype(F32), out["g64"].astype(F32)
    return out


def brackets_ok(ref):
    """the preconditions of the bracket, on the definition alone: the float64 evaluation error stays below 2^-30 of every loss
    word and below 2^-30 of a sample's largest gradient element"""
    L, eL = ref["L64"], ref["eL"]
    gmax = np.abs(ref["g64"]).reshape(len(L), -1).max(1)
    return bool((eL <= 2.0 ** -30 * np.abs(L)).all() and (ref["eg"].reshape(len(L), -1).max(1) <= 2.0 ** -30 * gmax).all())


def loss_torch(x, yp, m, bones, lambdas):
    """the same objective in torch, differentiable in x, in x's dtype: (n,) totals and the (n, 4) words.  m (n, T, V)."""
    lp, lv, lb = lambdas
    n, C, T, V = x.shape
    bones = torch.as_tensor(np.asarray(bones, dtype=np.int64).reshape(-1, 2))
    zero = x.new_zeros(())
    d = x - yp
    on = m > 0
    Wp = C * torch.where(on, m, zero).sum((1, 2))
    Sp = torch.where(on[:, None], m[:, None] * d * d, zero).sum((1, 2, 3))
    onv = on[:, :-1] & on[:, 1:]
    mv = torch.where(onv, m[:, :-1] * m[:, 1:], zero)
    e = d[:, :, 1:] - d[:, :, :-1]
    Sv = torch.where(onv[:, None], mv[:, None] * e * e, zero).sum((1, 2, 3))
    Wv = C * mv.sum((1, 2))
    a, c = bones[:, 0], bones[:, 1]
    onb = (m[:, :, a] > 0) & (m[:, :, c] > 0)
    mb = torch.where(onb, m[:, :, a] * m[:, :, c], zero)
    sx = ((x[:, :, :, a] - x[:, :, :, c]) ** 2).sum(1)
    sy = ((yp[:, :, :, a] - yp[:, :, :, c]) ** 2).sum(1)
    df = torch.where(onb, sx - sy, zero)
    Sb = (mb * df * df).sum((1, 2))
    Wb = mb.sum((1, 2))

    def term(S, W, lam):
        ok = (W > 0) & (lam > 0)
        return torch.where(ok, S / torch.where(ok, W, torch.ones_like(W)), torch.zeros_like(S))

    Lp, Lv, Lb = term(Sp, Wp, lp), term(Sv, Wv, lv), term(Sb, Wb, lb)
    L = (lp * Lp + lv * Lv) + lb * Lb
    return L, torch.stack([L, Lp, Lv, Lb], 1)


# ---- the step ----------------------------------------------------------------------------------------------------------------

def lr_at(s, S, lr, ramp_up=0, ramp_down=0):
    """the learning rate of the 1-based step s of S"""
    f = float(lr)
    if ramp_up > 0:
        f = f * min(1.0, s / ramp_up)
    if ramp_down > 0 and s > S - ramp_down:
        f = f * (0.5 * (1.0 + np.cos(np.pi * ((s - (S - ramp_down)) / ramp_down))))
    return f


def step_def(w, am, av, gw, wmean, labels, loss, s, best_obj, best_loss, best_w, nonfinite, hist, S, lr, b1, b2, eps, lambda_w=0.0,
             ramp_up=0, ramp_down=0):
    """kg_proj_step on numpy arrays; returns new arrays (the inputs are not modified): w, am, av as float64 (w64, am64, av64:
    unrounded) and float32, obj (n,) fp32, best_obj, best_loss, best_w, nonfinite, hist"""
    w, am, av, gw = (np.asarray(t, dtype=F32) for t in (w, am, av, gw))
    n, D = w.shape
    labels = np.asarray(labels, dtype=np.int64)
    K = len(wmean)
    lab_ok = (labels >= 0) & (labels < K)
    wm = np.asarray(wmean, dtype=np.float64)[np.where(lab_ok, labels, 0)]
    L = np.asarray(loss, dtype=F32)[:, 0]
    w64 = w.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if lambda_w > 0:
            prior = ((w64 - wm) ** 2).mean(1)
            obj = (L.astype(np.float64) + lambda_w * prior).astype(F32)
        else:
            obj = L.copy()
        ok = lab_ok & np.isfinite(obj) & np.isfinite(gw).all(1)
        out = dict(obj=obj, best_obj=np.array(best_obj, dtype=F32), best_loss=np.array(best_loss, dtype=F32),
                   best_w=np.array(best_w, dtype=F32), nonfinite=np.array(nonfinite, dtype=np.int32),
                   hist=None if hist is None else np.array(hist, dtype=F32))
        if out["hist"] is not None and 1 <= s <= S:
            out["hist"][s - 1] = obj
        out["nonfinite"] += (~ok).astype(np.int32)
        better = ok & (obj < out["best_obj"])
        out["best_obj"][better] = obj[better]
        out["best_loss"][better] = np.asarray(loss, dtype=F32)[better]
        out["best_w"][better] = w[better]
        g = gw.astype(np.float64)
        if lambda_w > 0:
            g = g + (2.0 * lambda_w / D) * (w64 - wm)
        m1 = b1 * am.astype(np.float64) + (1.0 - b1) * g
        v1 = b2 * av.astype(np.float64) + (1.0 - b2) * (g * g)
        sc = max(int(s), 1)
        up = (m1 / (1.0 - b1 ** sc)) / (np.sqrt(v1 / (1.0 - b2 ** sc)) + eps)
        w1 = w64 - lr_at(s, S, lr, ramp_up, ramp_down) * up
        k = ok[:, None]
        out["w64"], out["am64"], out["av64"] = np.where(k, w1, w64), np.where(k, m1, am), np.where(k, v1, av)
        out["w"] = np.where(k, w1.astype(F32), w)
        out["am"] = np.where(k, m1.astype(F32), am)
        out["av"] = np.where(k, v1.astype(F32), av)
    out["ok"] = ok
    return out


# ---- stand-ins for the two native wrappers on CPU tensors (tests/test_proj_cpu.py patches them in) -------------------------------

def emu_proj_loss(x, y, bones, lambdas, mask=None, scale=1.0, shift=0.0, loss=None, gx=None):
    ref = loss_def(x.detach().numpy(), y.detach().numpy(), None if mask is None else mask.numpy(), bones, lambdas, scale, shift)
    lo, g = torch.from_numpy(ref["loss"]), torch.from_numpy(ref["gx"])
    if loss is not None:
        loss.copy_(lo)
        lo = loss
    if gx is not None:
        gx.copy_(g.reshape(gx.shape))
        g = gx
    return lo, g


def emu_proj_step(w, am, av, gw, wmean, labels, loss, step_t, best_obj, best_loss, best_w, nonfinite, hist, S, lr, b1, b2, eps,
                  lambda_w=0.0, ramp_up=0, ramp_down=0):
    o = step_def(w.numpy(), am.numpy(), av.numpy(), gw.numpy(), wmean.numpy(), labels.numpy(), loss.numpy(), int(step_t.item()),
                 best_obj.numpy(), best_loss.numpy(), best_w.numpy(), nonfinite.numpy(), None if hist is None else hist.numpy(),
                 S, lr, b1, b2, eps, lambda_w, ramp_up, ramp_down)
    for name, t in (("w", w), ("am", am), ("av", av), ("best_obj", best_obj), ("best_loss", best_loss), ("best_w", best_w),
                    ("nonfinite", nonfinite), ("hist", hist)):
        if t is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(o[name])))


# ---- the reference loop ------------------------------------------------------------------------------------------------------------

def oracle_synth(Go, w):
    """oracle.modules_ref.Generator's blocks from w, as its forward iterates them, with zero noise planes"""
    x = w.view(*w.shape, 1, 1)
    zero = w.new_zeros(())
    for blk, imp in zip(Go.st_gcn_networks, Go.edge_importance):
        x, _ = blk(x, Go.A[blk.lvl].to(w.dtype) * imp, zero)
    return x


def oracle_loop(Go, y, labels, w_init, bones, steps, lr=0.05, betas=(0.9, 0.999), eps=1e-8, lambdas=(1.0, 1.0, 0.1), mask=None,
                dtype=torch.float64):
    """The projection loop (lambda_w = 0, no ramps) on the eval-mode oracle generator in ``dtype``: objective, autograd, Adam,
    best-keeping.  Returns dict(history (steps, n), w, best_w, best_obj) as float64 numpy arrays.  ``Go`` is used as it is (the
    caller has cast it)."""
    Go.eval()
    n = w_init.shape[0]
    w = w_init.detach().to(dtype).clone().requires_grad_(True)
    yp = y.detach().to(dtype)
    m = torch.ones((n,) + tuple(y.shape[2:]), dtype=dtype) if mask is None else mask.to(dtype).expand(n, *y.shape[2:])
    am, av = torch.zeros_like(w), torch.zeros_like(w)
    best_obj = torch.full((n,), float("inf"), dtype=dtype)
    best_w = w.detach().clone()
    hist = []
    b1, b2 = betas
    for s in range(1, steps + 1):
        L, _ = loss_torch(oracle_synth(Go, w), yp, m, bones, lambdas)
        g, = torch.autograd.grad(L.sum(), w)
        with torch.no_grad():
            hist.append(L.detach().clone())
            better = L < best_obj
            best_obj = torch.where(better, L.detach(), best_obj)
            best_w[better] = w.detach()[better]
            am.mul_(b1).add_(g, alpha=1 - b1)
            av.mul_(b2).addcmul_(g, g, value=1 - b2)
            w -= lr * (am / (1 - b1 ** s)) / ((av / (1 - b2 ** s)).sqrt() + eps)
    f = lambda t: t.detach().double().numpy()
    return dict(history=f(torch.stack(hist)), w=f(w), best_w=f(best_w), best_obj=f(best_obj))


# ---- the end-to-end case of tests/test_proj_cpu.py and tests/test_project_gpu.py ----------------------------------------------------

TINY = dict(latent=32, channels=2, classes=3, t_size=16, mlp=4, n=3, steps=20)
TINY_BONES = [(1, 2), (2, 3), (0, 1), (4, 5), (5, 6), (0, 4), (0, 7), (7, 8), (8, 9), (8, 10), (10, 11), (11, 12), (8, 13), (13, 14),
              (14, 15)]                                                   # H36M


def tiny_pair(device="cpu"):
    """(G on the HIP path, Go the oracle) with the same parameters: H36M graph, latent 32, 3 classes, t_size 16, mlp_dim 4"""
    from kinetic_gan_amd.generator import Generator
    from oracle import modules_ref as M
    from oracle.fill import fill_module
    G = Generator(TINY["latent"], TINY["channels"], TINY["classes"], TINY["t_size"], TINY["mlp"], dataset="h36m")
    Go = M.Generator(TINY["latent"], TINY["channels"], TINY["classes"], TINY["t_size"], TINY["mlp"], dataset="h36m")
    fill_module(G, seed=1)
    fill_module(Go, seed=1)
    return G.to(device), Go


def _case(Go, seed):
    """targets y = synth(w*), w* = 0.5 randn, and w_init = w* + 0.3 randn, from the float64 oracle"""
    g = torch.Generator().manual_seed(seed)
    D = TINY["latent"] + TINY["classes"]
    w_star = 0.5 * torch.randn(TINY["n"], D, generator=g, dtype=torch.float64)
    w_init = w_star + 0.3 * torch.randn(TINY["n"], D, generator=g, dtype=torch.float64)
    Go.double().eval()
    with torch.no_grad():
        y = oracle_synth(Go, w_star)
    return y.float(), w_init.float()


def _dev(a, b):
    return float(np.abs(a / b - 1.0).max())


@functools.lru_cache(maxsize=None)
def end_to_end_case():
    """dict(y, w_init, labels, r64 the float64 loop, E, dw, seed): the case of the issue with its two yardsticks - E, the largest
    relative deviation of the float32 oracle loop's objective curve from the float64 loop's, and dw, the float32 loop's largest
    deviation in best_w.

    The objective is only piecewise smooth: where the trajectory passes a LeakyReLU unit's kink, two runs that differ by
    round-off can take different sides, and Adam's normalised step then moves that latent element by a share of lr, not of the
    round-off.  A comparison against ONE float64 curve says something only where that curve answers linearly to perturbations of
    float32 size.  That is a property of the reference alone, and it is asserted on the reference alone: the float64 loop is run
    again from w_init moved by +-4 dw per element (three sign patterns), and each of these curves must stay within 16 E of the
    unperturbed one (four times the linear answer to a perturbation four times the float32 loop's).  The case is the first seed
    0, 1, 2, .. that passes; nothing of the code under test is looked at."""
    Go = tiny_pair()[1]
    labels = torch.zeros(TINY["n"], dtype=torch.int64)
    for seed in range(16):
        y, w_init = _case(Go, seed)
        r64 = oracle_loop(Go.double(), y, labels, w_init, TINY_BONES, TINY["steps"], dtype=torch.float64)
        r32 = oracle_loop(Go.float(), y, labels, w_init, TINY_BONES, TINY["steps"], dtype=torch.float32)
        Go.double()
        E, dw = _dev(r32["history"], r64["history"]), float(np.abs(r32["best_w"] - r64["best_w"]).max())
        g = torch.Generator().manual_seed(1000 + seed)
        ok = True
        for _ in range(3):
            sign = torch.randint(0, 2, w_init.shape, generator=g).double() * 2 - 1
            rp = oracle_loop(Go, y, labels, w_init.double() + 4 * dw * sign, TINY_BONES, TINY["steps"], dtype=torch.float64)
            ok = ok and _dev(rp["history"], r64["history"]) <= 16 * E
        if ok:
            return dict(y=y, w_init=w_init, labels=labels, r64=r64, E=E, dw=dw, seed=seed)
    raise AssertionError("no seed below 16 gives a float64 loop that is stable under perturbations of float32 size")
