"""Host definitions of the inference-only generation entry points (include/kgan_hip.h): the yardstick of
tests/test_sampler_cpu.py and tests/test_sampler_gpu.py, and their CPU emulations (``emulated_sampler_native``: installed on
top of tests/util.emulated_native by patching ``_native.<name>``).

    kg_bn_eval_coef   coef = [gamma rstd, beta - mean gamma rstd, mean, rstd], rstd = 1 / sqrt(running_var + eps)
    kg_genblock_infer the staged eval-mode block: head conv, U A_k expansion with residual, 3-tap tcn, affine + noise + act
    kg_sample_inputs  tests/train_def.py's Philox4x32-10 / Box-Muller streams with word 1 = 0x100 + (0 z, 1 noise, 2 t)
    kg_trunc_lerp     m = column means of t;  x <- m + truncation (x - m)
"""
import contextlib

import numpy as np
import torch

from kinetic_gan_amd import _native
from oracle import prim_ref
from tests import train_def
from tests.util import emulated_native

STREAM_SAMPLE = 0x100
S_Z, S_NOISE, S_T = STREAM_SAMPLE + 0, STREAM_SAMPLE + 1, STREAM_SAMPLE + 2


# ---- definitions -----------------------------------------------------------------------------------------------------

def bn_eval_coef_def(gamma, beta, running_mean, running_var, eps, dtype=np.float64):
    """(4, C) = [scale, shift, mean, rstd] in ``dtype`` (numpy arrays in, gamma / beta may be None)"""
    rm, rv = np.asarray(running_mean, dtype=dtype), np.asarray(running_var, dtype=dtype)
    rstd = dtype(1.0) / np.sqrt(rv + dtype(eps))
    scale = rstd if gamma is None else np.asarray(gamma, dtype=dtype) * rstd
    shift = -rm * scale if beta is None else np.asarray(beta, dtype=dtype) - rm * scale
    return np.stack([scale, shift, rm, rstd]).astype(dtype)


def sample_normals(n, seed, stream, step, dtype=np.float32):
    """the first n normals of sampler stream ``stream`` (S_Z, S_NOISE, S_T) of replay ``step``"""
    return train_def.normals(n, seed, stream, step, rank=0, dtype=dtype)


def trunc_lerp_def(x, t, truncation, dtype=np.float64):
    """m + truncation (x - m), m = column means of t, every operation in ``dtype``"""
    x, t = np.asarray(x, dtype=dtype), np.asarray(t, dtype=dtype)
    m = t.sum(0, dtype=dtype) / dtype(t.shape[0])
    return (m + dtype(truncation) * (x - m)).astype(dtype)


# ---- CPU emulations of the _native wrappers ---------------------------------------------------------------------------

def bn_eval_coef(jobs):
    for j in jobs:
        rstd = torch.rsqrt(j["running_var"] + j["eps"])
        scale = rstd if j.get("gamma") is None else j["gamma"] * rstd
        shift = -j["running_mean"] * scale if j.get("beta") is None else j["beta"] - j["running_mean"] * scale
        j["coef"].copy_(torch.stack([scale, shift, j["running_mean"], rstd]))


def genblock_infer_supported(d, n, wg, wr, wt):
    return d.T > 1 and d.Tc * d.Vc >= 16 and prim_ref._gb_lds_bytes(d, False, stats=False) >= 0


def genblock_infer(d, *, x, wg, wr=None, br=None, wt, bt=None, B, U=None, ct=None, cr=None, noise=None, nw=None, slope=0.2,
                   out=None):
    Mg = d.Kp * d.C
    yc = torch.einsum("mc,nctv->nmtv", prim_ref._gb_head_weight(d, wg, wr), x)
    rs = yc[:, Mg:] if d.res_kind == 2 else (x if d.res_kind == 1 else None)
    z, r = prim_ref.gen_expand(yc[:, :Mg], None, U, d.rep, d.C, rs=rs, rbias=br if d.res_kind == 2 else None, B=B)
    u = torch.nn.functional.conv2d(z, wt.reshape(d.C, d.C, 3, 1), bt, padding=(1, 0))
    res = prim_ref.affine_act(u, ct[0] if ct is not None else None, ct[1] if ct is not None else None, r,
                              cr[0] if cr is not None else None, cr[1] if cr is not None else None, noise,
                              None if nw is None else nw.reshape(-1), d.act, slope)
    if out is not None:
        out.copy_(res)
        return out
    return res


def sample_inputs(step, ticket, seed, z=None, noise=None, t=None):
    s = int(step.item())
    for buf, stream in ((z, S_Z), (noise, S_NOISE), (t, S_T)):
        if buf is not None:
            buf.copy_(torch.as_tensor(sample_normals(buf.numel(), seed, stream, s)).view(buf.shape))
    step.add_(1)


def trunc_lerp(x, t, truncation):
    m = t.mean(0, keepdim=True)
    x.copy_(m + truncation * (x - m))
    return x


NAMES = ["bn_eval_coef", "genblock_infer_supported", "genblock_infer", "sample_inputs", "trunc_lerp"]


@contextlib.contextmanager
def emulated_sampler_native():
    """tests/util.emulated_native plus the emulations above"""
    with emulated_native():
        saved = {k: getattr(_native, k) for k in NAMES}
        for k in NAMES:
            setattr(_native, k, globals()[k])
        try:
            yield
        finally:
            for k, f in saved.items():
                setattr(_native, k, f)
