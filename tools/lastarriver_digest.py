#!/usr/bin/env python3
"""sha256 digests of what the last-arriver kernels compute (csrc/kg_handoff.h), to compare two trees bit for bit on one GPU
(record: profiles/lastarriver_refactor.log).  The benchmark shapes do not reach every ticket site - kg_bn_bwd_many is on the
autograd route only, the tail statistics have one chunk per channel at the toy shapes - so each site runs here on a shape with
several arrivals per counter, from fixed seeds, twice where the second call reuses the counters:
  * bn_fwd_many: two jobs, two stacked batches each (coefficients, running statistics, batch counters);
  * bn_bwd_many: two jobs;
  * gen_tail_bwd: 50 chunks per channel (tanh, identity residual) and lrelu with a BatchNorm residual;
  * genblock_fwd (finished input and pending-tail input) and genblock_bwd with the previous block's tail statistics;
  * conv: a 4-way K-split completed in-kernel;
  * the step counters after kg_step_inputs / kg_sample_inputs;
  * the sum of the shared ticket counters afterwards (0).
One line per digest, "<name> <sha256>".
    python tools/lastarriver_digest.py [--root TREE]"""
import argparse
import hashlib
import os
import sys

os.environ["KG_CONV_PLAN"] = "4,4"      # (read when the library loads) tile 32 x 64, four workgroups along K
os.environ.pop("KG_CONV_INKERNEL", None)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package runs")
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.root))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd import _native as nv  # noqa: E402
from kinetic_gan_amd._native import TAP_TIME, Group, WView  # noqa: E402


def say(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        h.update(np.ascontiguousarray(a).tobytes())
    print("%-28s %s" % (name, h.hexdigest()), flush=True)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    assert kinetic_gan_amd.__file__.startswith(os.path.abspath(opt.root)), kinetic_gan_amd.__file__

    def plane(t):
        out = nv.new_plane(*t.shape, d)
        out.copy_(t)
        return out

    def stats(x, c, seed):
        return (rnd(c, seed=seed) + 1.5).to(d), x.mean((0, 2, 3)).to(d), torch.rsqrt(x.var((0, 2, 3), unbiased=False) + 1e-5).to(d)

    # ---- kg_bn_fwd_many
    jobs, state = [], []
    for i, (N, C, T, V) in enumerate([(4, 3, 32, 25), (64, 32, 16, 11)]):
        rm, rv = torch.zeros(C, device=d), torch.ones(C, device=d)
        nbt = torch.zeros((), dtype=torch.int64, device=d)
        jobs.append(dict(x=plane(rnd(N, C, T, V, seed=300 + i) * 2.0 + 3.0), gamma=rnd(C, seed=310 + i).to(d), beta=rnd(C, seed=320 + i).to(d),
                         running_mean=rm, running_var=rv, num_batches_tracked=nbt, momentum=0.1, eps=1e-5, groups=2))
        state += [rm, rv, nbt]
    for rounds in range(2):
        say("bn_fwd_many.coef.%d" % rounds, *nv.bn_fwd_many(jobs))
        say("bn_fwd_many.running.%d" % rounds, *state)

    # ---- kg_bn_bwd_many
    jobs = []
    for i, (N, C, T, V) in enumerate([(64, 32, 16, 11), (2, 3, 64, 25)]):
        x = rnd(N, C, T, V, seed=400 + i) * 1.5 + 0.3
        gam, mean, rstd = stats(x, C, 410 + i)
        jobs.append(dict(g=plane(rnd(N, C, T, V, seed=420 + i)), x=plane(x), gamma=gam, mean=mean, rstd=rstd, training=True))
    for rounds in range(2):
        say("bn_bwd_many.coef.%d" % rounds, *nv.bn_bwd_many(jobs))

    # ---- kg_gen_tail_stats + kg_gen_tail_apply
    for N, C, T, V, res, act in [(64, 3, 64, 25, "identity", nv.ACT_TANH), (64, 32, 16, 11, "bn", nv.ACT_LRELU)]:
        g, out = plane(rnd(N, C, T, V, seed=1)), plane(torch.tanh(rnd(N, C, T, V, seed=2)))
        r = rnd(N, C, T, V, seed=4)
        noise = rnd(N, 1, T, V, seed=5).to(d)
        names = ["nw"] + (["gamma_r", "beta_r"] if res == "bn" else [])
        for rounds in range(2):
            sinks = {k: torch.full((C,), 0.25, device=d) for k in names}
            du, dr = nv.gen_tail_bwd(g, out, act, r=plane(r), bn_r=stats(r, C, 6) if res == "bn" else None, noise=noise, sinks=sinks)
            say("gen_tail_bwd.%s.%d" % (res, rounds), du, dr, *[sinks[k] for k in names])

    # ---- kg_genblock_fwd / kg_genblock_bwd: the G3 geometry of tests/test_kernels_gpu.py (GENBLOCK_CASES[0])
    N, Cin, C, K, Tc, V, rep = 6, 128, 64, 3, 4, 5, 2
    T = Tc * rep
    dims = nv.GenBlockDims(Cin=Cin, C=C, K=K, Kp=K, Tc=Tc, Vc=V, T=T, V=V, rep=rep, res_kind=2, bn_t=True, act=nv.ACT_LRELU)
    w = dict(wg=(rnd(K * C, Cin, 1, 1, seed=2) / Cin ** 0.5).to(d), wr=(rnd(C, Cin, 1, 1, seed=3) / Cin ** 0.5).to(d),
             wt=(rnd(C, C, 3, 1, seed=5) / (3 * C) ** 0.5).to(d), B=torch.rand(K, V, V, generator=torch.Generator().manual_seed(1)).to(d))
    assert nv.genblock_supported(dims, N, w["wg"], w["wr"], w["wt"]) and nv.genblock_supported(dims, N, w["wg"], w["wr"], w["wt"], backward=True)

    def bn_layer(seed):
        g_ = torch.Generator().manual_seed(seed)
        return dict(gamma=(torch.rand(C, generator=g_) + 0.5).to(d), beta=torch.randn(C, generator=g_).to(d),
                    running_mean=torch.randn(C, generator=g_).to(d), running_var=(torch.rand(C, generator=g_) + 0.5).to(d),
                    num_batches_tracked=torch.tensor(3, dtype=torch.int64, device=d), momentum=0.1, eps=1e-5)

    pu, prr = rnd(N, Cin, Tc, V, seed=10), rnd(N, Cin, Tc, V, seed=11)
    pnoise = rnd(N, 1, Tc, V, seed=14).to(d)
    pend = dict(u=plane(pu), r=plane(prr), ct=(rnd(2, 4, Cin, seed=12) * 0.5).to(d), cr=(rnd(2, 4, Cin, seed=13) * 0.5).to(d), noise=pnoise,
                nw=(rnd(1, Cin, 1, 1, seed=15) * 0.2).to(d), act=nv.ACT_LRELU)
    for mode in ("x", "pend"):
        bt_, br_ = bn_layer(20), bn_layer(21)
        src = dict(x=plane(rnd(N, Cin, Tc, V, seed=9))) if mode == "x" else dict(pend=pend)
        got = nv.genblock_fwd(dims, bn_t=bt_, bn_r=br_, br=rnd(C, seed=4).to(d), bt=rnd(C, seed=6).to(d), groups=2, **src, **w)
        say("genblock_fwd.%s" % mode, *[got[k] for k in ("x", "yc", "z", "r", "u", "ct", "cr")])
        say("genblock_fwd.%s.running" % mode, *[bl[k] for bl in (bt_, br_) for k in ("running_mean", "running_var", "num_batches_tracked")])
    names = ["nw", "gamma_t", "beta_t", "gamma_r", "beta_r"]
    wb = {k: v for k, v in w.items()}
    for rounds in range(2):
        sinks = {k: torch.full((Cin,), 0.25, device=d) for k in names}
        prev = dict(x=plane(torch.tanh(rnd(N, Cin, Tc, V, seed=36))), u=plane(pu), r=plane(prr), noise=pnoise, act=nv.ACT_LRELU,
                    bn_t=stats(pu, Cin, 40), bn_r=stats(prr, Cin, 41), sinks=sinks)
        got = nv.genblock_bwd(dims, g=plane(rnd(N, C, T, V, seed=30)), out=plane(torch.tanh(rnd(N, C, T, V, seed=31))),
                              u=plane(rnd(N, C, T, V, seed=32) * 1.5 + 0.3), r=plane(rnd(N, C, T, V, seed=33)),
                              coef=rnd(6, C, seed=34).to(d), prev=prev, **wb)
        say("genblock_bwd.%d" % rounds, *[got[k] for k in ("du", "dr", "gyc", "zf", "gx", "pcoef")], *[sinks[k] for k in names])

    # ---- kg_conv: four workgroups along K, the last one of a tile to arrive sums the slabs
    N, Cin, M, T, V = 4, 512, 500, 8, 3
    cm = lambda t: t.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    grp = Group(cm(rnd(N, Cin, T, V, seed=2)).to(d), (rnd(M, Cin, 3, 1, seed=1) / (3 * Cin) ** 0.5).to(d), WView(1, Cin * 3, 3), Cin, 3,
                TAP_TIME, 2, False, None)
    kw = dict(bias0=rnd(M, seed=3).to(d), bias1=rnd(M, seed=5).to(d), add=cm(rnd(N, M, T // 2, V, seed=4)).to(d), act=nv.ACT_LRELU,
              mask=cm(rnd(N, M, T // 2, V, seed=6)).to(d))
    nv.last_conv_plan = []
    for rounds in range(2):
        say("conv.ksplit4.%d" % rounds, nv.conv([grp], N, M, T // 2, V, **kw))
    assert nv.last_conv_plan == [4, 4], nv.last_conv_plan
    nv.last_conv_plan = None

    # ---- kg_step_inputs / kg_sample_inputs: the last arriver advances the step counter
    step, ticket = torch.zeros(1, dtype=torch.int64, device=d), torch.zeros(1, dtype=torch.int32, device=d)
    z, alpha = torch.empty(8, 512, device=d), torch.empty(8, device=d)
    for rounds in range(3):
        nv.step_inputs(step, ticket, 11, 8, z=z, alpha=alpha)
    say("step_inputs", step, ticket, z, alpha)
    noise = torch.empty(5000, device=d)
    for rounds in range(3):
        nv.sample_inputs(step, ticket, 12, z=z, noise=noise)
    say("sample_inputs", step, ticket, z, noise)

    torch.cuda.synchronize()
    total = sum(int(b.sum().item()) for b in nv._sync_bufs.values())
    print("%-28s %d" % ("sync_buffer.sum", total), flush=True)
    assert total == 0


if __name__ == "__main__":
    main()
