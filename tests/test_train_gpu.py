"""kg_step_inputs and the training loop on the MI355X: the kernel against the host definition (tests/train_def.py),
moments, determinism (also under graph replay), TrainLoop against the eagerly called Trainer.iteration, resume,
the streaming fallback and the command line.

Normals: the device evaluates Box-Muller in fp32 (logf / sqrtf / sincosf, each specified to a few ulp, like numpy's);
the reference is the definition in float64 from the same integer draws.  The bound is 4 E with E the largest
difference between the definition evaluated in numpy float32 and in float64 over this file's draws (seed 5, steps 0-2,
ranks 0 and 1, every normal stream, 2^18 values each; seed 1234, step 7, 2^20 values): the largest is 1.783e-6, so
E = 1.8e-6 and the bound is 7.2e-6.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd.feeder import Feeder
from kinetic_gan_amd.train import ResidentDataset, TrainLoop, norm_constants, update_pattern

import train_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)
from util import build_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_DEF = 1.8e-6
NORMAL_TOL = 4 * E_DEF
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_normals(got, seed, stream, step, rank=0):
    n = got.numel()
    want = train_def.normals(n, seed, stream, step, rank, dtype=np.float64)
    e_def = np.abs(train_def.normals(n, seed, stream, step, rank) - want).max()
    err = np.abs(got.detach().cpu().double().numpy().reshape(-1) - want).max()
    print("normals seed %d stream %d step %d rank %d: n %d, device err %.3e, definition fp32 err %.3e, bound %.3e" % (
        seed, stream, step, rank, n, err, e_def, NORMAL_TOL))
    assert e_def <= E_DEF, e_def              # (the bound's premise holds for these draws)
    assert err <= NORMAL_TOL, err


def plane_lens(layout, B):
    import kinetic_gan_amd.generator as KG
    G = KG.Generator(512, 3, 60, 64, 4, dataset="ntu") if layout == "ntu" else KG.Generator(512, 2, 10, 32, 4, dataset="h36m")
    shapes = train_def.plane_shapes(G, B)
    return shapes, [int(np.prod(s)) for s in shapes]


_SHAPES = {}


def shapes_of(layout, B):
    if (layout, B) not in _SHAPES:
        _SHAPES[(layout, B)] = plane_lens(layout, B)
    return _SHAPES[(layout, B)]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("layout,B,world", [("ntu", 64, 1), ("h36m", 64, 1), ("ntu", 5, 1), ("ntu", 8, 2)])
def test_kernel_against_definition(tmp_path, layout, B, world):
    """three consecutive iterations (the second epoch starts inside them): batch, labels and alpha bit for bit, normals
    within 4 E of the float64 definition, the counter at s + 1 after every launch"""
    seed = 5
    c, v, t_raw, t_size, latent = (3, 25, 80, 64, 512) if layout == "ntu" else (2, 16, 40, 32, 512)
    n = 2 * B * world + 3                     # two batches per epoch and rank, a dropped tail
    dp, lp = train_def.synthetic_dataset(str(tmp_path), n, c, t_raw, v, 7, layout, seed=1)
    f = Feeder(dp, lp, dataset=layout)
    res = ResidentDataset(f, t_size, DEV)
    assert res.fits and tuple(res.data.shape) == (n, c, t_size, v)
    bpe = (n // B) // world
    assert bpe == 2
    plen = bpe * world * B
    perm = torch.stack([torch.as_tensor(train_def.permutation(n, seed, e)[:plen]) for e in (0, 1)]).to(DEV)
    shapes, lens = shapes_of(layout, B)
    for rank in range(world):
        step = guard.zeros(1, dtype=torch.int64, device=DEV)
        ticket = guard.zeros(1, dtype=torch.int32, device=DEV)
        real = guard.full((B, c, t_size, v), float("nan"), device=DEV)
        labels = guard.full((B,), -1, dtype=torch.int64, device=DEV)
        z = guard.full((B, latent), float("nan"), device=DEV)
        alpha = guard.full((B,), float("nan"), device=DEV)
        noise = guard.full((2 * sum(lens),), float("nan"), device=DEV)
        nd, ng = nv.noise_views(noise, shapes)
        gather = nv.StepData(res.data, res.labels, perm, bpe, res.scale, res.shift, real, labels)
        for s in range(3):
            nv.step_inputs(step, ticket, seed, B, z=z, alpha=alpha, noise=noise, plane_len=lens, gather=gather,
                           rank=rank, world=world)
            assert int(step.item()) == s + 1 and int(ticket.item()) == 0
            w_real, w_labels = train_def.batch(f, B, t_size, seed, s, rank, world)
            assert np.array_equal(bits(real), bits(w_real)), (rank, s)
            assert np.array_equal(labels.cpu().numpy(), w_labels), (rank, s)
            assert np.array_equal(bits(alpha), bits(train_def.uniforms(B, seed, train_def.STREAM_ALPHA, s, rank))), (rank, s)
            check_normals(z, seed, train_def.STREAM_Z, s, rank)
            check_normals(torch.cat([p.reshape(-1) for p in nd]), seed, train_def.STREAM_NOISE_D, s, rank)
            check_normals(torch.cat([p.reshape(-1) for p in ng]), seed, train_def.STREAM_NOISE_G, s, rank)
            # the planes of one synthesis are consecutive runs of its stream
            w_planes = train_def.noise_planes(shapes, seed, train_def.STREAM_NOISE_D, s, rank, dtype=np.float64)
            for p, w in zip(nd, w_planes):
                assert tuple(p.shape) == w.shape and np.abs(p.cpu().double().numpy() - w).max() <= NORMAL_TOL


@pytest.mark.usefixtures("guarded")
def test_kernel_strided_source_and_random_only(tmp_path):
    """a source that is not row-contiguous (the uncropped 5-D NTU array read in place) takes the element-wise form with
    the same bits; data == NULL leaves the batch alone and still advances the counter"""
    seed, B, t_size = 5, 4, 8
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 11, 3, 12, 25, 5, "ntu", seed=2)
    f = Feeder(dp, lp, dataset="ntu")
    raw = torch.as_tensor(np.load(dp)).to(DEV)                # (N, C, T, V, M)
    view = raw[:, :, :t_size, :, 0]
    res_labels = torch.as_tensor(np.asarray(f.label, dtype=np.int64)).to(DEV)
    scale, shift = norm_constants(f)
    perm = torch.stack([torch.as_tensor(train_def.permutation(11, seed, e)[:8]) for e in (0, 1)]).to(DEV)
    step = guard.zeros(1, dtype=torch.int64, device=DEV)
    ticket = guard.zeros(1, dtype=torch.int32, device=DEV)
    real = guard.zeros((B, 3, t_size, 25), device=DEV)
    labels = guard.zeros(B, dtype=torch.int64, device=DEV)
    g = nv.StepData(view, res_labels, perm, 2, scale, shift, real, labels)
    for s in range(3):
        nv.step_inputs(step, ticket, seed, B, gather=g)
        w_real, w_labels = train_def.batch(f, B, t_size, seed, s)
        assert np.array_equal(bits(real), bits(w_real)) and np.array_equal(labels.cpu().numpy(), w_labels)
    keep = real.clone()
    z = guard.zeros((B, 16), device=DEV)
    nv.step_inputs(step, ticket, seed, B, z=z)
    assert int(step.item()) == 4 and torch.equal(real, keep)
    check_normals(z, seed, train_def.STREAM_Z, 3)


@pytest.mark.usefixtures("guarded")
def test_moments():
    """2^20 normals and 2^20 uniforms of one iteration: 5-sigma bounds from the sample size"""
    n = 1 << 20
    step = guard.full((1,), 7, dtype=torch.int64, device=DEV)
    ticket = guard.zeros(1, dtype=torch.int32, device=DEV)
    z = torch.empty((2048, 512), device=DEV)
    nv.step_inputs(step, ticket, 1234, 2048, z=z)
    x = z.double().reshape(-1)
    assert x.numel() == n and torch.isfinite(x).all()
    mean, var = x.mean().item(), x.var(unbiased=False).item()
    print("normals: mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e)" % (mean, 5 / n ** 0.5, var - 1, 5 * (2 / n) ** 0.5))
    assert abs(mean) <= 5 / n ** 0.5
    assert abs(var - 1) <= 5 * (2 / n) ** 0.5
    check_normals(z, 1234, train_def.STREAM_Z, 7)
    step.fill_(7)
    alpha = torch.empty(n, device=DEV)
    nv.step_inputs(step, ticket, 1234, n, alpha=alpha)
    u = alpha.double()
    print("uniforms: mean - 1/2 %.3e (bound %.3e)" % (u.mean().item() - 0.5, 5 / (12 * n) ** 0.5))
    assert u.min().item() >= 0.0 and u.max().item() < 1.0
    assert abs(u.mean().item() - 0.5) <= 5 / (12 * n) ** 0.5
    assert np.array_equal(bits(alpha), bits(train_def.uniforms(n, 1234, train_def.STREAM_ALPHA, 7)))


def test_determinism_and_graph_replay():
    """the same (seed, step) gives the same bits whatever ran before, eagerly and from a replayed graph; steps differ"""
    B, seed = 16, 5
    shapes, lens = shapes_of("ntu", B)

    def bufs():
        return (guard.zeros((B, 512), device=DEV), guard.zeros(B, device=DEV), guard.zeros(2 * sum(lens), device=DEV))
    step = guard.zeros(1, dtype=torch.int64, device=DEV)
    ticket = guard.zeros(1, dtype=torch.int32, device=DEV)
    outs = {}
    for s in (0, 1, 2):
        z, a, nz = bufs()
        nv.step_inputs(step, ticket, seed, B, z=z, alpha=a, noise=nz, plane_len=lens)
        outs[s] = (z, a, nz)
    for k in range(3):
        assert not torch.equal(outs[0][k], outs[1][k]) and not torch.equal(outs[1][k], outs[2][k])
    step.fill_(1)                              # again, out of order, into other buffers
    z, a, nz = bufs()
    nv.step_inputs(step, ticket, seed, B, z=z, alpha=a, noise=nz, plane_len=lens)
    for got, want in zip((z, a, nz), outs[1]):
        assert torch.equal(got, want)
    # graph: one capture, replayed from counter 0
    z, a, nz = bufs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nv.step_inputs(step, ticket, seed, B, z=z, alpha=a, noise=nz, plane_len=lens)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        nv.step_inputs(step, ticket, seed, B, z=z, alpha=a, noise=nz, plane_len=lens)
    step.zero_()
    for s in (0, 1, 2):
        g.replay()
        torch.cuda.synchronize()
        assert int(step.item()) == s + 1
        for got, want in zip((z, a, nz), outs[s]):
            assert torch.equal(got, want), s


# ---- the loop ------------------------------------------------------------------------------------------------------------

CFG, B_LOOP, SEED_LOOP, N_CRITIC = "h36m", 4, 3, 2


def loop_feeder(path):
    os.makedirs(path, exist_ok=True)
    dp, lp = train_def.synthetic_dataset(str(path), 3 * B_LOOP + 1, 2, 40, 16, 10, "h36m", seed=4)
    return Feeder(dp, lp, dataset="h36m")


def loop_state(loop_or_trainer, G, D):
    tr = getattr(loop_or_trainer, "trainer", loop_or_trainer)
    out = {}
    for name, f, m in (("G", tr.fG, G), ("D", tr.fD, D)):
        out[name + ".flat"], out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = f.flat, f.exp_avg, f.exp_avg_sq
        out[name + ".adam_step"] = f.step
        for k, b in m.named_buffers():
            out[name + ".buf." + k] = b
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def assert_same_state(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs (max |d| %.3e)" % (
            what, k, (a[k].double() - b[k].double()).abs().max().item())


def make_loop(path, **kw):
    c, G, D, _, _ = build_pair(CFG, DEV)
    loop = TrainLoop(G, D, loop_feeder(path), B_LOOP, c["t_size"], n_critic=N_CRITIC, seed=SEED_LOOP, **kw)
    return loop, G, D


@pytest.fixture(scope="module")
def six_steps(tmp_path_factory):
    """six iterations of the captured loop on a 3-batch dataset: state and loss record"""
    loop, G, D = make_loop(tmp_path_factory.mktemp("six"))
    assert loop.bpe == 3 and not loop.streaming
    for _ in range(6):
        loop.step()
    d, g = loop.losses()
    assert loop.step_count == 6 and int(loop.step_dev.item()) == 6 and loop.epoch == 2
    assert np.isfinite(d).all() and np.isfinite(g).all() and d.shape == g.shape == (6,)
    return loop_state(loop, G, D), d, g


def test_loop_matches_eager_iterations(six_steps, tmp_path):
    """TrainLoop (graphs, n_critic = 2, the epoch turns over after three batches) against Trainer.iteration called
    eagerly on the host definition's batch / labels / alpha and the kernel's own normals: bit for bit"""
    from kinetic_gan_amd.wgan_gp import Trainer
    state, d_rec, g_rec = six_steps
    c, G, D, _, _ = build_pair(CFG, DEV)
    f = loop_feeder(tmp_path)
    tr = Trainer(G, D, n_critic=N_CRITIC)
    shapes = train_def.plane_shapes(G, B_LOOP)
    lens = [int(np.prod(s)) for s in shapes]
    step = guard.zeros(1, dtype=torch.int64, device=DEV)
    ticket = guard.zeros(1, dtype=torch.int32, device=DEV)
    pattern = update_pattern(3, N_CRITIC, 6)
    assert pattern == [True, False, True, True, False, True]
    d_want, g_want, last_g = [], [], float("nan")
    for s in range(6):
        real, labels = train_def.batch(f, B_LOOP, c["t_size"], SEED_LOOP, s)
        alpha = train_def.uniforms(B_LOOP, SEED_LOOP, train_def.STREAM_ALPHA, s)
        z = torch.empty((B_LOOP, c["latent"]), device=DEV)
        noise = torch.empty(2 * sum(lens), device=DEV)
        step.fill_(s)
        nv.step_inputs(step, ticket, SEED_LOOP, B_LOOP, z=z, noise=noise, plane_len=lens)
        nd, ng = nv.noise_views(noise, shapes)
        d_loss, g_loss = tr.iteration(torch.as_tensor(real).to(DEV), torch.as_tensor(labels).to(DEV), z,
                                      torch.as_tensor(alpha).to(DEV).view(-1, 1, 1, 1), nd, ng if pattern[s] else None,
                                      with_g=pattern[s])
        d_want.append(d_loss.item())
        last_g = g_loss.item() if g_loss is not None else last_g
        g_want.append(last_g)
    assert_same_state(state, loop_state(tr, G, D), "graph loop vs eager iterations")
    assert np.array_equal(d_rec, np.array(d_want, dtype=np.float32)), (d_rec, d_want)
    assert np.array_equal(g_rec, np.array(g_want, dtype=np.float32)), (g_rec, g_want)


def test_eager_loop_matches_graph_loop(six_steps, tmp_path):
    loop, G, D = make_loop(tmp_path, use_graph=False)
    for _ in range(6):
        loop.step()
    d, g = loop.losses()
    assert_same_state(six_steps[0], loop_state(loop, G, D), "use_graph=False vs graphs")
    assert np.array_equal(d, six_steps[1]) and np.array_equal(g, six_steps[2])


@pytest.mark.parametrize("use_graph", [True, False])
def test_short_ring_wraps_and_flushes(six_steps, tmp_path, use_graph):
    """a ring of four rows under six iterations: the fifth - critic only, so kg_loss_append repeats the g_loss of the row
    before it, which lies across the wrap - is enqueued behind a flush in mid-run; run_ahead=2: the host waits at every
    iteration.  State and both loss arrays bit for bit those of the default loop"""
    loop, G, D = make_loop(tmp_path, ring_len=4, run_ahead=2, use_graph=use_graph)
    assert loop.ring_len == 4 and tuple(loop.ring.shape) == (4, 2) and loop.run_ahead == 2
    assert not loop.with_g(4)
    for _ in range(6):
        loop.step()
    d, g = loop.losses()
    assert_same_state(six_steps[0], loop_state(loop, G, D), "ring_len=4, run_ahead=2, use_graph=%s vs the default loop" % use_graph)
    assert np.array_equal(bits(d), bits(six_steps[1])) and np.array_equal(bits(g), bits(six_steps[2]))


@pytest.mark.parametrize("at", [3, 4])
def test_resume_is_bit_exact(six_steps, tmp_path, at):
    """``at`` iterations + state_dict through a file + the rest in a fresh loop == 6 iterations; at = 3 is an epoch boundary,
    4 lies inside an epoch: the first iteration uploads the current epoch's permutation and the next one's"""
    loop, G, D = make_loop(tmp_path / "a")
    for _ in range(at):
        loop.step()
    path = str(tmp_path / "loop_state.pth")
    sd = loop.state_dict()
    assert set(sd) == {"step", "epoch", "seed", "n_critic", "batch_size", "batches_per_epoch", "last_losses", "G", "D"}
    assert set(sd["G"]) == set(sd["D"]) == {"flat", "exp_avg", "exp_avg_sq", "adam_step", "buffers"}
    torch.save(sd, path)
    d0, g0 = loop.losses()
    del loop
    loop2, G2, D2 = make_loop(tmp_path / "b")
    with torch.no_grad():                      # a different starting point: everything must come from the file
        loop2.trainer.fG.flat.add_(0.25)
        loop2.trainer.fD.flat.mul_(0.5)
    loop2.load_state_dict(torch.load(path, weights_only=False))
    assert loop2.step_count == at and loop2.epoch == 1
    for k in range(6 - at):
        loop2.step()
        if k == 0:
            assert sorted(loop2._perm._epochs) == [1, 2]
    d1, g1 = loop2.losses()
    assert_same_state(six_steps[0], loop_state(loop2, G2, D2), "%d + resume + %d vs 6" % (at, 6 - at))
    assert np.array_equal(np.concatenate((d0, d1)), six_steps[1])
    assert np.array_equal(np.concatenate((g0, g1)), six_steps[2])


def test_streaming_fallback_is_bit_exact(six_steps, tmp_path):
    loop, G, D = make_loop(tmp_path, max_resident_bytes=0)
    assert loop.streaming and loop.resident.data is None
    for _ in range(6):
        loop.step()
    d, g = loop.losses()
    assert_same_state(six_steps[0], loop_state(loop, G, D), "streamed vs resident")
    assert np.array_equal(d, six_steps[1]) and np.array_equal(g, six_steps[2])


def test_cli_two_epochs(tmp_path):
    """tools/train.py on a tiny synthetic .npy / .pkl pair: actions, loss record, checkpoints the modules accept"""
    from scipy.io import loadmat
    from kinetic_gan_amd.discriminator import Discriminator
    from kinetic_gan_amd.generator import Generator
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 13, 2, 40, 16, 10, "h36m", seed=6)
    out = str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--n_epochs", "2", "--batch_size", "4", "--dataset", "h36m",
           "--channels", "2", "--v_size", "16", "--t_size", "32", "--n_classes", "10", "--n_critic", "2",
           "--sample_interval", "4", "--checkpoint_interval", "3", "--log_interval", "2", "--seed", "1",
           "--data_path", dp, "--label_path", lp, "--out", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[Epoch ")]
    assert len(lines) == 3 and lines[-1].startswith("[Epoch 1/2] [Batch 2/3] [D loss: "), r.stdout
    assert sorted(os.listdir(os.path.join(out, "actions"))) == ["0.npy", "4.npy"]
    acts = np.load(os.path.join(out, "actions", "4.npy"))
    assert acts.shape == (100, 2, 32, 16) and np.isfinite(acts).all()
    mat = loadmat(os.path.join(out, "plot_loss.mat"))
    assert mat["d_loss"].size == 6 and mat["g_loss"].size == 6 and np.isfinite(mat["d_loss"]).all()
    assert sorted(os.listdir(os.path.join(out, "models"))) == ["discriminator_0.pth", "discriminator_3.pth",
                                                               "generator_0.pth", "generator_3.pth"]
    G = Generator(512, 2, 10, 32, 4, dataset="h36m")
    D = Discriminator(2, 10, 32, 512, dataset="h36m")
    G.load_state_dict(torch.load(os.path.join(out, "models", "generator_3.pth")), strict=True)
    D.load_state_dict(torch.load(os.path.join(out, "models", "discriminator_3.pth")), strict=True)
    assert os.path.exists(os.path.join(out, "loop_state.pth"))
