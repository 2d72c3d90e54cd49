"""The inference-only generation path on the MI355X: its four entry points against their host definitions
(tests/sample_def.py), kg_genblock_infer against the reference's eval-mode block fixtures, Sampler.forward against the
reference's eval-mode outputs and the float64 oracle, replay / resume determinism, sampling between training replays,
and the command line.

Normals (kg_sample_inputs): the device evaluates Box-Muller in fp32; the reference is the definition in float64 from the
same integer draws.  The bound is 4 E with E the largest difference between the definition evaluated in numpy float32
and in float64 over exactly this file's draws (DRAW_CASES: seed 5, replays 0-2, streams z / noise / t of an h36m round
of 30 with 1000 x 522 truncation draws and of an ntu round of 7 with 1000 x 512): the largest is 1.786e-6, so
E = 1.8e-6 and the bound is 7.2e-6.

kg_trunc_lerp: the reference is the definition in float64; the bound is 4 S with S the largest difference between the
definition evaluated in numpy float32 (rows added in index order) and in float64 on this file's inputs (LERP_CASES):
the largest is 4.909e-7 (values up to 4.6), so S = 5.0e-7 and the bound is 2.0e-6.
"""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import gen_trunk as gt
from kinetic_gan_amd.sample import Sampler, sample_actions
from oracle.fill import block_input, fill_module, gen_block_in_shapes, rand_inputs, rand_noise
from tests import guard, sample_def, train_def
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)
from tests.util import build_pair, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
FWD_TOL = 1e-4          # as tests/test_parity_gpu.py
E_DEF = 1.8e-6
NORMAL_TOL = 4 * E_DEF
S_LERP = 5.0e-7
LERP_TOL = 4 * S_LERP
SEED = 5
# (layout, samples of a round, columns of the truncation draws)
DRAW_CASES = [("h36m", 30, 522), ("ntu", 7, 512)]
# (N, D, M, truncation, seed)
LERP_CASES = [(37, 572, 1000, 0.7, 1), (600, 512, 1000, 0.95, 2), (3, 70, 33, 0.5, 3)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _log(name, msg):
    """figures go to the tools' output folder (KG_OUT, default runs/) before the assertion that reads them"""
    out = os.path.join(ROOT, os.environ.get("KG_OUT", "runs"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, name), "a") as f:
        f.write(msg + "\n")
    print(msg)


def noise_len(layout, B):
    t_size, nodes = (64, (25, 11, 5, 1)) if layout == "ntu" else (32, (16, 7, 2, 1))
    from oracle.fill import gen_noise_shapes
    return sum(int(np.prod(s)) for s in gen_noise_shapes(B, t_size, nodes))


def lerp_inputs(case):
    N, D, M, trunc, seed = case
    return rnd(N, D, seed=100 + seed), rnd(M, D, seed=200 + seed) * 1.5 + 0.25, trunc


# ---- kg_bn_eval_coef ---------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_bn_eval_coef_against_definition_and_live_statistics():
    """eight layers in one launch against the float64 definition (the bound of the kg_bn_fwd coefficient test: 2e-5 of the
    largest value); an in-place change of the running statistics is picked up by the next launch"""
    cs = [512, 256, 128, 64, 32, 3, 2, 301]
    jobs, host = [], []
    for i, c in enumerate(cs):
        gamma, beta = rnd(c, seed=10 + i), rnd(c, seed=20 + i)
        rm, rv = rnd(c, seed=30 + i) * 0.3, torch.rand(c, generator=torch.Generator().manual_seed(40 + i)) + 0.5
        if i == 5:
            gamma = None
        if i == 6:
            beta = None
        host.append((gamma, beta, rm, rv))
        jobs.append(dict(gamma=None if gamma is None else gamma.to(DEV), beta=None if beta is None else beta.to(DEV),
                         running_mean=rm.to(DEV), running_var=rv.to(DEV), eps=1e-5,
                         coef=guard.full((4, c), float("nan"), device=DEV)))

    def check(tag):
        for j, c in zip(jobs, cs):
            want = sample_def.bn_eval_coef_def(None if j["gamma"] is None else j["gamma"].cpu().numpy(),
                                               None if j["beta"] is None else j["beta"].cpu().numpy(),
                                               j["running_mean"].cpu().numpy(), j["running_var"].cpu().numpy(), 1e-5)
            got = j["coef"].cpu().double().numpy()
            err = np.abs(got - want).max()
            assert err <= 2e-5 * np.abs(want).max(), (tag, c, err)
    nv.bn_eval_coef(jobs)
    check("first")
    before = [j["coef"].clone() for j in jobs]
    for j in jobs:                              # what a training replay does: in place, through the same pointers
        j["running_mean"].add_(0.5)
        j["running_var"].mul_(2.0)
    nv.bn_eval_coef(jobs)
    check("after the update")
    for b, j in zip(before, jobs):
        assert not torch.equal(b[1], j["coef"][1]) and not torch.equal(b[3], j["coef"][3])
    with pytest.raises(ValueError):
        nv.bn_eval_coef(jobs + jobs[:1])


# ---- kg_genblock_infer -------------------------------------------------------------------------------------------------

def _block_operands(G, meta, i, n):
    """parameters, adjacency product and eval-mode coefficients of block i"""
    params, bns = gt.collect_params(G)
    p = meta.block_params([q.detach() for q in params], i)
    g = meta.geoms[i]
    ae = torch.empty((g.K, g.V, g.V), device=DEV)
    b = torch.empty((g.K, g.Vc, g.V), device=DEV)
    nv.gen_adj_prepare([dict(a=g.A_fixed, imp=G.edge_importance[i].detach(), u=g.U, aeff=ae, b=b)])
    coefs, jobs = [None, None], []
    for k, bn in enumerate(bns[i]):
        if bn is not None:
            coefs[k] = torch.empty((4, g.cout), device=DEV)
            jobs.append(dict(gamma=bn.weight.detach(), beta=bn.bias.detach(), running_mean=bn.running_mean,
                             running_var=bn.running_var, eps=bn.eps, coef=coefs[k]))
    if jobs:
        nv.bn_eval_coef(jobs)
    return g, p, b[:g.Kp], coefs


def _run_block(g, p, B, coefs, x, noise, out=None):
    return nv.genblock_infer(g.dims, x=x, wg=p["wg"], wr=p["wr"], br=p["br"], wt=p["wt"], bt=p["bt"], B=B, U=g.U, ct=coefs[0],
                             cr=coefs[1], noise=noise, nw=p["nw"], slope=0.2, out=out)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("form", ["ct", "rt"])
@pytest.mark.parametrize("cfg", ["ntu", "h36m"])
def test_genblock_infer_vs_reference_golden(cfg, form, golden_dir, monkeypatch):
    """every block that takes the fused form against the reference's eval-mode block outputs (the inputs of
    test_blocks_vs_reference_golden), in the compile-time and the run-time geometry form; then at an odd N with
    non-contiguous planes against the contiguous N = 2 launch, sample by sample, bit for bit"""
    if form == "rt":
        monkeypatch.setenv("KG_GB_RT", "1")
    nv.reload_env()
    try:
        gold = np.load(os.path.join(golden_dir, f"ref_{cfg}.npz"))
        c, G, D, Go, Do = build_pair(cfg, DEV)
        nn_ = G.graph.num_node
        n = 2
        noise = rand_noise(n, c["t_size"], nn_, seed=5, device=DEV)
        gs = gen_block_in_shapes(n, c["latent"] + c["n_classes"], c["channels"], c["t_size"], nn_)
        meta = gt.GenTrunkMeta(G, torch.device(DEV))
        fused = []
        for i in range(meta.nb):
            g, p, B, coefs = _block_operands(G, meta, i, n)
            if not (g.T > 1 and nv.genblock_infer_supported(g.dims, n, p["wg"], p["wr"] if g.res == "conv" else None, p["wt"])):
                continue
            fused.append(i)
            x = block_input(gs[i], 200 + i).to(DEV)
            y = _run_block(g, p, B, coefs, x, noise[i])
            torch.cuda.synchronize()
            assert tuple(y.shape) == gold[f"G{i}_eval"].shape
            err = rel_err(y, torch.as_tensor(gold[f"G{i}_eval"]))
            _log("sampler_blocks.log", "%s %s G%d %s vs G%d_eval: %.3e" % (cfg, form, i, tuple(y.shape), i, err))
            assert err < FWD_TOL, (cfg, form, i, err)
            # N = 5: input and output are slices of wider tensors (sample and channel strides of a larger buffer)
            n5 = 5
            xs = torch.cat([x, block_input((3,) + tuple(gs[i][1:]), 900 + i).to(DEV)], 0)
            nz5 = torch.cat([noise[i], rnd(3, 1, g.T, g.V, seed=950 + i).to(DEV)], 0)
            wide = nv.new_plane(n5 + 2, g.cin + 3, g.Tc, g.Vc, torch.device(DEV)).zero_()
            xin = wide[1:1 + n5, 2:2 + g.cin]
            xin.copy_(xs)
            wide_o = nv.new_plane(n5 + 1, g.cout + 2, g.T, g.V, torch.device(DEV)).zero_()
            yo = wide_o[1:, 1:1 + g.cout]
            assert not xin.is_contiguous() and not yo.is_contiguous()
            _run_block(g, p, B, coefs, xin, nz5, out=yo)
            torch.cuda.synchronize()
            assert np.array_equal(bits(yo[:n]), bits(y)), (cfg, form, i)
            assert torch.isfinite(yo).all()
            assert float(wide_o[0].abs().max()) == 0.0 and float(wide_o[:, 0].abs().max()) == 0.0       # nothing outside the view
        assert fused == ([3, 4, 5, 6] if cfg == "ntu" else [5, 6]), fused
    finally:
        monkeypatch.undo()
        nv.reload_env()


# ---- kg_sample_inputs --------------------------------------------------------------------------------------------------

def check_normals(got, stream, step):
    n = got.numel()
    want = sample_def.sample_normals(n, SEED, stream, step, dtype=np.float64)
    e_def = np.abs(sample_def.sample_normals(n, SEED, stream, step) - want).max()
    err = np.abs(got.detach().cpu().double().numpy().reshape(-1) - want).max()
    _log("sampler_inputs.log", "normals stream 0x%x replay %d: n %d, device err %.3e, definition fp32 err %.3e, bound %.3e" % (
        stream, step, n, err, e_def, NORMAL_TOL))
    assert e_def <= E_DEF, e_def              # (the bound's premise holds for these draws)
    assert err <= NORMAL_TOL, err


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("layout,B,dt", DRAW_CASES)
def test_sample_inputs_against_definition(layout, B, dt):
    nl = noise_len(layout, B)
    step = guard.zeros(1, dtype=torch.int64, device=DEV)
    ticket = guard.zeros(1, dtype=torch.int32, device=DEV)
    z = guard.full((B, 512), float("nan"), device=DEV)
    noise = guard.full((nl,), float("nan"), device=DEV)
    t = guard.full((1000, dt), float("nan"), device=DEV)
    for s in range(3):
        nv.sample_inputs(step, ticket, SEED, z=z, noise=noise, t=t)
        assert int(step.item()) == s + 1 and int(ticket.item()) == 0
        check_normals(z, sample_def.S_Z, s)
        check_normals(noise, sample_def.S_NOISE, s)
        check_normals(t, sample_def.S_T, s)
    # z == NULL: the buffer is left alone, the other streams are what they were, the counter still advances
    z.fill_(7.0)
    n0, t0 = noise.clone(), t.clone()
    step.fill_(2)
    nv.sample_inputs(step, ticket, SEED, z=None, noise=noise, t=t)
    assert int(step.item()) == 3 and float(z.min()) == 7.0 == float(z.max())
    assert torch.equal(noise, n0) and torch.equal(t, t0)
    # the sampler's z stream is not the training z stream of the same seed and step
    zt = guard.zeros((B, 512), device=DEV)
    st = guard.full((1,), 2, dtype=torch.int64, device=DEV)
    nv.step_inputs(st, ticket, SEED, B, z=zt)
    nv.sample_inputs(step.fill_(2), ticket, SEED, z=z)
    assert not torch.equal(z, zt) and float((z == zt).float().mean()) < 0.01


def test_sample_inputs_replay_is_deterministic():
    B, dt = 12, 522
    nl = noise_len("h36m", B)

    def bufs():
        return guard.zeros((B, 512), device=DEV), guard.zeros(nl, device=DEV), guard.zeros((1000, dt), device=DEV)
    step = guard.zeros(1, dtype=torch.int64, device=DEV)
    ticket = guard.zeros(1, dtype=torch.int32, device=DEV)
    outs = {}
    for s in range(3):
        b = bufs()
        nv.sample_inputs(step, ticket, SEED, *b)
        outs[s] = b
    for k in range(3):
        assert not torch.equal(outs[0][k], outs[1][k]) and not torch.equal(outs[1][k], outs[2][k])
    z, nz, t = bufs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nv.sample_inputs(step, ticket, SEED, z, nz, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        nv.sample_inputs(step, ticket, SEED, z, nz, t)
    step.zero_()
    for s in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(step.item()) == s + 1
        for got, want in zip((z, nz, t), outs[s]):
            assert torch.equal(got, want), s


# ---- kg_trunc_lerp -----------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("case", LERP_CASES)
def test_trunc_lerp_against_definition(case):
    x, t, trunc = lerp_inputs(case)
    want = sample_def.trunc_lerp_def(x.numpy(), t.numpy(), trunc)
    s_def = np.abs(sample_def.trunc_lerp_def(x.numpy(), t.numpy(), trunc, dtype=np.float32).astype(np.float64) - want).max()
    xd, td = x.to(DEV), t.to(DEV)
    a = nv.trunc_lerp(xd.clone(), td, trunc)
    b = nv.trunc_lerp(xd.clone(), td, trunc)
    err = np.abs(a.cpu().double().numpy() - want).max()
    _log("sampler_inputs.log", "trunc_lerp %s: device err %.3e, definition fp32 spread %.3e, bound %.3e" % (case, err, s_def, LERP_TOL))
    assert s_def <= S_LERP, s_def             # (the bound's premise holds for these inputs)
    assert err <= LERP_TOL, err
    assert np.array_equal(bits(a), bits(b))
    # rows of wider matrices (leading dimensions)
    N, D = x.shape
    xw, tw = guard.zeros((N, D + 5), device=DEV), guard.zeros((t.shape[0], D + 3), device=DEV)
    xw[:, 2:2 + D], tw[:, 1:1 + D] = xd, td
    nv.trunc_lerp(xw[:, 2:2 + D], tw[:, 1:1 + D], trunc)
    assert np.array_equal(bits(xw[:, 2:2 + D]), bits(a)) and float(xw[:, :2].abs().max()) == 0.0 == float(xw[:, 2 + D:].abs().max())


# ---- Sampler.forward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["ntu", "h36m"])
def test_sampler_forward_vs_reference_golden(cfg, golden_dir):
    gold = np.load(os.path.join(golden_dir, f"ref_{cfg}.npz"))
    c, G, D, Go, Do = build_pair(cfg, DEV)
    nn_ = G.graph.num_node
    real, labels, z, alpha = rand_inputs(4, c["channels"], c["t_size"], nn_[0], c["n_classes"], c["latent"], seed=3, device=DEV)
    noise = rand_noise(4, c["t_size"], nn_, seed=6, device=DEV)
    sd0 = {k: v.clone() for k, v in G.state_dict().items()}
    out = Sampler(G, qtd=1, use_graph=False).forward(z, labels, noise)
    err = rel_err(out, torch.as_tensor(gold["G_out_eval"]))
    np.random.seed(77)
    t = torch.as_tensor(np.random.normal(0, 1, (1000, c["latent"] + c["n_classes"])), dtype=torch.float32)
    out_t = Sampler(G, qtd=1, trunc=0.7, trunc_mode="w", use_graph=False).forward(z, labels, noise, trunc_t=t)
    err_t = rel_err(out_t, torch.as_tensor(gold["G_out_eval_trunc"]))
    _log("sampler_blocks.log", "%s Sampler.forward vs G_out_eval %.3e, vs G_out_eval_trunc %.3e" % (cfg, err, err_t))
    assert err < FWD_TOL, err
    assert err_t < FWD_TOL, err_t
    assert G.training
    for k, v in G.state_dict().items():
        assert torch.equal(v, sd0[k]), k


def test_sampler_forward_full_size_margin():
    """ntu, 600 samples (one round of the reference's default run): the distance of Sampler.forward to the float64
    evaluation of the oracle generator (as tools/g_margin.py forms it) is at most twice the distance of the existing
    eval / no_grad forward to the same value - both are fp32 evaluation orders of one network whose last block
    amplifies round-off; the yardstick is the float64 oracle, not either path"""
    c, G, D, Go, Do = build_pair("ntu", DEV)
    nn_ = G.graph.num_node
    n = 600
    real, labels, z, alpha = rand_inputs(n, c["channels"], c["t_size"], nn_[0], c["n_classes"], c["latent"], seed=11)
    noise = rand_noise(n, c["t_size"], nn_, seed=12)
    Go64 = copy.deepcopy(Go).double().eval()
    Go64.A = [a.double() for a in Go64.A]
    with torch.no_grad():
        f64 = Go64(z.double(), labels, noise=[t.double() for t in noise])
    zd, ld, nd = z.to(DEV), labels.to(DEV), [t.to(DEV) for t in noise]
    G.eval()
    with torch.no_grad():
        own = G(zd, ld, noise=nd)
    G.train(True)
    out = Sampler(G, qtd=10, use_graph=False).forward(zd, ld, nd)
    d_s, d_o = rel_err(out, f64), rel_err(own, f64)
    msg = "ntu n=600: Sampler.forward vs float64 oracle %.3e | eval / no_grad forward vs float64 oracle %.3e | ratio %.2f" % (
        d_s, d_o, d_s / max(d_o, 1e-30))
    _log("sampler_margin.log", msg)
    assert d_s <= 2 * d_o, msg


# ---- next(): replay, resume, consistency -------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["-", "w", "z"])
def test_next_replay_equals_eager_and_resumes(mode):
    c, G, D, Go, Do = build_pair("h36m", DEV)
    kw = dict(qtd=3, seed=9, trunc=None if mode == "-" else 0.8, trunc_mode=mode, mean_size=200)
    sg, se = Sampler(G, use_graph=True, **kw), Sampler(G, use_graph=False, **kw)
    seq = []
    for r in range(3):
        a, b = sg.next(), se.next()
        torch.cuda.synchronize()
        assert int(sg.step_dev.item()) == r + 1 == int(se.step_dev.item())
        for x, y in zip(a, b):
            assert torch.equal(x, y), (mode, r)
        assert a[1].tolist() == [k for _ in range(3) for k in range(10)]
        seq.append([t.clone() for t in a])
        # the returned z, labels and images belong together: the schedule on them, with the replay's own noise planes
        # (and truncation draws), gives the images bit for bit
        z_in = _raw_z(sg, r) if mode == "z" else a[2]       # ('z' mode returns the truncated z: forward() takes the raw draw)
        again = se.forward(z_in, a[1], sg.noise, trunc_t=sg.t)
        if mode == "z":
            assert np.array_equal(bits(nv.trunc_lerp(z_in.clone(), sg.t, 0.8)), bits(a[2]))
        assert np.array_equal(bits(again), bits(a[0])), (mode, r)
    assert not torch.equal(seq[0][0], seq[1][0]) and not torch.equal(seq[0][2], seq[1][2])
    # a second Sampler with the same seed: the same sequence; resumed at counter 1: continues it
    s2 = Sampler(G, use_graph=True, **kw)
    for r in range(2):
        for x, y in zip(s2.next(), seq[r]):
            assert torch.equal(x, y)
    s3 = Sampler(G, use_graph=True, **dict(kw, seed=1))
    s3.next()
    s3.load_state_dict({"seed": 9, "step": 1})
    for r in (1, 2):
        for x, y in zip(s3.next(), seq[r]):
            assert torch.equal(x, y)
    assert s3.state_dict() == {"seed": 9, "step": 3}


def _raw_z(s, r):
    """the z draw of replay r as the device wrote it (before the in-place Z-space truncation)"""
    z = torch.empty_like(s.z)
    step = guard.full((1,), r, dtype=torch.int64, device=DEV)
    nv.sample_inputs(step, guard.zeros(1, dtype=torch.int32, device=DEV), s.seed, z=z)
    return z


def test_fixed_z_and_generate_order():
    c, G, D, Go, Do = build_pair("h36m", DEV)
    z0 = rnd(1, c["latent"], seed=4)
    s = Sampler(G, qtd=2, label=7, seed=3, fixed_z=z0, trunc=0.9, trunc_mode="z", mean_size=100)
    a = [t.clone() for t in s.next()]
    b = [t.clone() for t in s.next()]
    assert a[1].tolist() == [7, 7] and torch.equal(s.fixed_z, z0.to(DEV).repeat(2, 1))
    assert not torch.equal(a[0], b[0])                       # other noise, other truncation mean
    assert float((a[2] - b[2]).abs().max()) < 0.5            # the pinned point, pulled towards two estimates of the mean
    np.random.seed(5)
    G.eval()
    imgs0, labs0, zs0 = sample_actions(G, c["n_classes"], c["latent"], gen_qtd=5, qtd=3, keep_on_device=True)
    G.train(True)
    imgs, labs, zs = Sampler(G, qtd=3, seed=1).generate(5, keep_on_device=True)
    assert labs.tolist() == labs0.tolist() and imgs.shape == imgs0.shape and zs.shape == zs0.shape and imgs.is_cuda
    assert torch.isfinite(imgs).all()


# ---- train -> sample -> train -> sample ----------------------------------------------------------------------------------

def test_sampling_between_training_replays(tmp_path):
    """one captured Sampler between graph-replayed TrainLoop steps, no rebuild: every next() is what a freshly built
    Sampler computes from the same inputs on the current weights, lies within 1e-5 of G.eval()'s own forward, and
    leaves G's running statistics as the training step left them"""
    from kinetic_gan_amd.feeder import Feeder
    from kinetic_gan_amd.train import TrainLoop
    c, G, D, Go, Do = build_pair("h36m", DEV)
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 13, 2, 40, 16, 10, "h36m", seed=4)
    loop = TrainLoop(G, D, Feeder(dp, lp, dataset="h36m"), 4, c["t_size"], n_critic=2, seed=3)
    s = Sampler(G, qtd=2, seed=21, trunc=0.95, trunc_mode="w", mean_size=300)
    prev = None
    for rnd_ in range(3):
        for _ in range(2):
            loop.step()
        torch.cuda.synchronize()
        stats = {k: v.clone() for k, v in G.named_buffers()}
        flat = loop.trainer.fG.flat.clone()
        imgs, labels, z = s.next()
        torch.cuda.synchronize()
        for k, v in G.named_buffers():
            assert torch.equal(v, stats[k]), k
        assert torch.equal(loop.trainer.fG.flat, flat) and G.training
        fresh = Sampler(G, qtd=2, seed=0, trunc=0.95, trunc_mode="w", mean_size=300, use_graph=False)
        again = fresh.forward(z, labels, s.noise, trunc_t=s.t)
        assert np.array_equal(bits(again), bits(imgs)), rnd_
        G.eval()
        with torch.no_grad():
            w = G.mapping(z, labels)
            w = G.truncate(w, 300, 0.95, t=s.t)
            own = G.synthesis(w, s.noise)
        G.train(True)
        err = rel_err(imgs, own)
        _log("sampler_blocks.log", "train -> sample round %d: next() vs G.eval() forward %.3e" % (rnd_, err))
        assert err < 1e-5, err
        if prev is not None:
            assert not torch.equal(prev, imgs)
        prev = imgs.clone()
    assert loop.step_count == 6 and s.step_count == 3


# ---- command line ------------------------------------------------------------------------------------------------------

def test_cli_generate_then_mmd(tmp_path):
    """tools/generate.py on a filled h36m generator: the reference's file names and shapes; tools/mmd_actions.py reads
    them against a synthetic real set and prints a finite value"""
    from kinetic_gan_amd.generator import Generator
    G = Generator(512, 2, 10, 32, 4, dataset="h36m")
    fill_module(G, seed=1)
    model = str(tmp_path / "generator.pth")
    torch.save(G.state_dict(), model)
    out = str(tmp_path / "run")
    common = ["--dataset", "h36m", "--channels", "2", "--v_size", "16", "--t_size", "32", "--n_classes", "10", "--model", model,
              "--out", out, "--seed", "2"]
    cmd = [sys.executable, os.path.join(ROOT, "tools", "generate.py"), "--batch_size", "25", "--gen_qtd", "100"] + common
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    act = os.path.join(out, "actions")
    assert sorted(os.listdir(act)) == ["10_100_trunc0.95_gen_data.npy", "10_100_trunc0.95_gen_label.pkl", "10_100_trunc0.95_gen_z.npy"]
    data = np.load(os.path.join(act, "10_100_trunc0.95_gen_data.npy"))
    zs = np.load(os.path.join(act, "10_100_trunc0.95_gen_z.npy"))
    with open(os.path.join(act, "10_100_trunc0.95_gen_label.pkl"), "rb") as f:
        labels = pickle.load(f)
    assert data.shape == (1000, 2, 32, 16) and data.dtype == np.float32 and np.isfinite(data).all() and np.abs(data).max() <= 1.0
    assert zs.shape == (1000, 512) and labels.shape == (2, 1000) and np.array_equal(labels[0], labels[1])
    assert labels[0].tolist() == [k for _ in range(4) for _ in range(25) for k in range(10)]
    # a single label, no truncation, eager: the other spelling of the names
    cmd = [sys.executable, os.path.join(ROOT, "tools", "generate.py"), "--batch_size", "3", "--gen_qtd", "4", "--label", "7",
           "--trunc_mode", "-", "--stochastic", "--no-graph"] + common
    r2 = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-4000:]
    d2 = np.load(os.path.join(act, "7_4_stochastic_gen_data.npy"))
    z2 = np.load(os.path.join(act, "7_4_stochastic_gen_z.npy"))
    assert d2.shape == (6, 2, 32, 16) and z2.shape == (6, 512) and np.array_equal(z2[0], z2[5])
    # MMD against a synthetic real set with >= 100 samples of every class
    real_dir = tmp_path / "real"
    os.makedirs(real_dir)
    dp, lp = train_def.synthetic_dataset(str(real_dir), 1600, 2, 40, 16, 10, "h36m", seed=8)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "mmd_actions.py"), "--data_real", dp, "--labels_real", lp,
           "--data_fake", os.path.join(act, "10_100_trunc0.95_gen_data.npy"),
           "--labels_fake", os.path.join(act, "10_100_trunc0.95_gen_label.pkl"), "--mmd_mode", "avg", "--t_size", "32",
           "--dataset", "h36m"]
    r3 = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r3.returncode == 0, r3.stdout[-2000:] + r3.stderr[-4000:]
    value = float(r3.stdout.strip().splitlines()[-1])
    assert np.isfinite(value) and value > 0.0
