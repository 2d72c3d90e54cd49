"""Generator weight averaging on the MI355X: kg_adam_step_ema against the host definition
(tests/ema_def.py) and against kg_adam_step(_fused) bit for bit, determinism and graph replay with a live step, the
captured training loop with the average, resume, sampling from the averaged module between replays, the commands.

Tolerance of the average (derived in tests/ema_def.py, not measured): per element and step
|e_device - e_def| <= 2^-21 max(|e_old|, |p_new|), e_def computed in float64 from the device's own e_old and p_new.
Across steps everything is compared one step at a time or bit for bit, so no accumulated tolerance is needed.
"""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd.feeder import Feeder
from kinetic_gan_amd.generator import Generator
from kinetic_gan_amd.sample import Sampler
from kinetic_gan_amd.train import TrainLoop, update_pattern
from kinetic_gan_amd.wgan_gp import FlatParams

import ema_def
import train_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)
from util import build_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-8


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.device == b.device and a.dtype == b.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return np.array_equal(bits(a), bits(b))


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------

_NTU_LEN = []


def ntu_flat_len():
    if not _NTU_LEN:
        f = FlatParams(Generator(512, 3, 60, 64, 4, dataset="ntu"))
        _NTU_LEN.append(int(f.flat.numel()))
        del f
    return _NTU_LEN[0]


def shifted(t, shift):
    """a copy of t whose first element lies `shift` floats behind a 16-byte boundary"""
    base = torch.empty(t.numel() + shift + 4, dtype=t.dtype, device=t.device)
    assert base.data_ptr() % 16 == 0
    out = base[shift:shift + t.numel()]
    out.copy_(t)
    assert out.data_ptr() % 16 == (4 * shift) % 16 and out.is_contiguous()
    return out


def kernel_inputs(n, seed):
    """parameters of mixed magnitude (1e-6 .. 1e2), an average that is partly far from them, partly within a few ulp, partly
    equal; gradients with zeros among them"""
    gen = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(n, generator=gen) * 8 - 6)
    p = torch.randn(n, generator=gen) * mag
    kind = torch.randint(0, 4, (n,), generator=gen)
    e = torch.where(kind == 0, p,
                    torch.where(kind == 1, p * (1 + 3e-7 * torch.randn(n, generator=gen)),
                                torch.where(kind == 2, p + mag * torch.randn(n, generator=gen), torch.randn(n, generator=gen))))
    g = torch.randn(n, generator=gen) * (torch.rand(n, generator=gen) > 0.1)
    m = 0.1 * torch.randn(n, generator=gen)
    v = 0.01 * torch.rand(n, generator=gen)
    return [t.to(DEV) for t in (p, g, m, v, e)]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("n", [1, 3, 1023, 4101, "ntu"])
def test_kernel_against_definition(n, shift):
    """p, m, v and the (cleared) g bit for bit what nv.adam_step gives on clones; e within 2^-21 max(|e_old|, |p_new|) of
    the float64 definition - for every step count, decay, warm-up and zero_grad of the issue's list, grad_scale 0.5"""
    n = ntu_flat_len() if n == "ntu" else n
    src = kernel_inputs(n, seed=11 + n % 97)
    step = guard.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for s in (1, 2, 9, 1000, 10 ** 6):
        step.fill_(s)
        for decay in (0.5, 0.999, 0.9999):
            for warmup in (0.0, 10.0):
                for zero in (False, True):
                    p, g, m, v, e = [shifted(t, shift) for t in src]
                    p2, g2, m2, v2 = [shifted(t, shift) for t in src[:4]]
                    if shift == 0:
                        assert all(t.data_ptr() % 16 == 0 for t in (p, g, m, v, e))
                    e_old = e.cpu().numpy().copy()
                    nv.adam_step_ema(p, g, m, v, e, LR, B1, B2, EPS, step, 0.5, zero, decay, warmup)
                    nv.adam_step(p2, g2, m2, v2, LR, B1, B2, EPS, step, 0.5, zero_grad=zero)
                    torch.cuda.synchronize()
                    what = (n, shift, s, decay, warmup, zero)
                    for a, b, name in ((p, p2, "p"), (m, m2, "m"), (v, v2, "v"), (g, g2, "g")):
                        assert same_bits(a, b), (name, what)
                    assert same_bits(g, torch.zeros_like(g) if zero else src[1]), what
                    p_new = p.cpu().numpy()
                    want = ema_def.update(e_old, p_new, s, decay, warmup)
                    err = np.abs(e.cpu().numpy().astype(np.float64) - want)
                    tol = ema_def.bound(e_old, p_new)
                    ratio = float((err / np.maximum(tol, 1e-300)).max())
                    worst = max(worst, ratio)
                    assert (err <= tol).all(), (what, ratio)
    print("kg_adam_step_ema n %d shift %d: largest |e - def| / bound %.3f (bound = 2^-21 max(|e_old|, |p_new|))" % (n, shift, worst))


def test_bad_arguments_raise():
    p, g, m, v, e = kernel_inputs(16, seed=1)
    step = guard.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="ema_decay"):
        nv.adam_step_ema(p, g, m, v, e, LR, B1, B2, EPS, step, 1.0, True, 1.0, 10.0)
    with pytest.raises(AssertionError):
        nv.adam_step_ema(p, g, m, v, e[:8], LR, B1, B2, EPS, step, 1.0, True, 0.9, 10.0)


# ---- 2. determinism and replay -------------------------------------------------------------------------------------------

def test_determinism_and_replay_follow_the_live_step():
    n = 4101
    src = kernel_inputs(n, seed=5)
    step = guard.zeros(1, dtype=torch.int32, device=DEV)

    def fresh():
        return [t.clone() for t in src]

    def eager(k):
        bufs = fresh()
        outs = []
        for s in range(1, k + 1):
            step.fill_(s)
            nv.adam_step_ema(*bufs, LR, B1, B2, EPS, step, 0.5, False, 0.999, 10.0)
            outs.append([t.clone() for t in bufs])
        torch.cuda.synchronize()
        return outs
    a, b = eager(3), eager(3)
    for x, y in zip(a, b):
        assert all(same_bits(s, t) for s, t in zip(x, y))
    assert not same_bits(a[0][4], a[1][4]) and not same_bits(a[1][4], a[2][4])
    # one captured launch, replayed three times with the step tensor advanced in between
    bufs = fresh()
    step.fill_(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nv.adam_step_ema(*bufs, LR, B1, B2, EPS, step, 0.5, False, 0.999, 10.0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        nv.adam_step_ema(*bufs, LR, B1, B2, EPS, step, 0.5, False, 0.999, 10.0)
    for t, s in zip(bufs, src):
        t.copy_(s)
    step.zero_()
    for k in range(3):
        step += 1
        graph.replay()
        torch.cuda.synchronize()
        assert int(step.item()) == k + 1
        for got, want, name in zip(bufs, a[k], "pgmve"):
            assert same_bits(got, want), (k, name)
    # the ramp moved: the third step's factor is not the first one's (beta_1 = 2/11, beta_3 = 4/13)
    assert ema_def.beta(1, 0.999, 10.0) != ema_def.beta(3, 0.999, 10.0)


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------

CFG, B_LOOP, SEED_LOOP, N_CRITIC, DECAY = "h36m", 4, 3, 2, 0.99


def loop_feeder(path):
    os.makedirs(path, exist_ok=True)
    dp, lp = train_def.synthetic_dataset(str(path), 3 * B_LOOP + 1, 2, 40, 16, 10, "h36m", seed=4)
    return Feeder(dp, lp, dataset="h36m")


def loop_state(loop, with_ema=True):
    tr = loop.trainer
    out = {}
    for name, f, m in (("G", tr.fG, loop.G), ("D", tr.fD, loop.D)):
        out[name + ".flat"], out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = f.flat, f.exp_avg, f.exp_avg_sq
        out[name + ".grad"], out[name + ".adam_step"] = f.grad, f.step
        for k, b in m.named_buffers():
            out[name + ".buf." + k] = b
    if with_ema and tr.fG.ema is not None:
        out["G.ema"] = tr.fG.ema
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def assert_same_state(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs (max |d| %.3e)" % (
            what, k, (a[k].double() - b[k].double()).abs().max().item())


def make_loop(path, **kw):
    c, G, D, _, _ = build_pair(CFG, DEV)
    return TrainLoop(G, D, loop_feeder(path), B_LOOP, c["t_size"], n_critic=N_CRITIC, seed=SEED_LOOP, **kw)


@pytest.fixture(scope="module")
def six_steps(tmp_path_factory):
    """six replays of the captured loop with the average: state (average included) after every iteration, loss record"""
    loop = make_loop(tmp_path_factory.mktemp("six"), ema_decay=DECAY)
    assert loop.bpe == 3 and not loop.streaming and loop.trainer.fD.ema is None
    f = loop.trainer.fG
    initial = f.flat.clone()
    assert same_bits(f.ema, initial) and f.ema.data_ptr() != f.flat.data_ptr()
    # after capture, before the first step: the warm-up iterations in front of a capture have left no trace
    loop._graph(True)
    loop._graph(False)
    torch.cuda.synchronize()
    assert same_bits(f.ema, initial) and same_bits(f.flat, initial) and int(f.step.item()) == 0
    states = []
    for _ in range(6):
        loop.step()
        states.append(loop_state(loop))
    d, g = loop.losses()
    assert loop.step_count == 6 and np.isfinite(d).all() and np.isfinite(g).all()
    return initial.cpu(), states, d, g


def test_loop_average_moves_with_generator_steps_only(six_steps):
    initial, states, _, _ = six_steps
    pattern = update_pattern(3, N_CRITIC, 6)
    assert pattern == [True, False, True, True, False, True]
    prev_e, s = initial, 0
    for k, (st, wg) in enumerate(zip(states, pattern)):
        if not wg:
            assert torch.equal(st["G.ema"], prev_e), k
        else:
            s += 1
            assert int(st["G.adam_step"].item()) == s
            want = ema_def.update(prev_e.numpy(), st["G.flat"].numpy(), s, DECAY, 10.0)
            err = np.abs(st["G.ema"].numpy().astype(np.float64) - want)
            assert (err <= ema_def.bound(prev_e.numpy(), st["G.flat"].numpy())).all(), k
            assert not torch.equal(st["G.ema"], prev_e) and not torch.equal(st["G.ema"], st["G.flat"])
        prev_e = st["G.ema"]
    assert s == 4


def test_replays_match_eager_iterations(six_steps, tmp_path):
    _, states, d_rec, g_rec = six_steps
    loop = make_loop(tmp_path, ema_decay=DECAY, use_graph=False)
    for k in range(6):
        loop.step()
        assert_same_state(states[k], loop_state(loop), "graph vs eager, iteration %d" % k)
    d, g = loop.losses()
    assert np.array_equal(bits(d), bits(d_rec)) and np.array_equal(bits(g), bits(g_rec))


def test_average_only_observes(six_steps, tmp_path):
    _, states, d_rec, g_rec = six_steps
    loop = make_loop(tmp_path)
    assert loop.trainer.fG.ema is None and "ema" not in loop.state_dict() and "ema" not in loop.state_dict()["G"]
    with pytest.raises(RuntimeError):
        loop.ema_generator()
    for k in range(6):
        loop.step()
        want = {key: v for key, v in states[k].items() if key != "G.ema"}
        assert_same_state(want, loop_state(loop), "with vs without the average, iteration %d" % k)
    d, g = loop.losses()
    assert np.array_equal(bits(d), bits(d_rec)) and np.array_equal(bits(g), bits(g_rec))


# ---- 4. resume -----------------------------------------------------------------------------------------------------------

def test_resume_is_bit_exact(six_steps, tmp_path):
    _, states, d_rec, g_rec = six_steps
    loop = make_loop(tmp_path / "a", ema_decay=DECAY)
    for _ in range(3):
        loop.step()
    sd = loop.state_dict()
    assert sd["ema"] == {"decay": DECAY, "warmup": 10.0} and same_bits(sd["G"]["ema"], states[2]["G.ema"])
    assert "ema" not in sd["D"]
    path = str(tmp_path / "loop_state.pth")
    torch.save(sd, path)
    d0, g0 = loop.losses()
    del loop
    loop2 = make_loop(tmp_path / "b", ema_decay=DECAY)
    with torch.no_grad():                      # a different starting point: everything must come from the file
        loop2.trainer.fG.flat.add_(0.25)
        loop2.trainer.fG.ema.mul_(0.5)
    loaded = torch.load(path, weights_only=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # (a state WITH the average: no warning)
        loop2.load_state_dict(loaded)
    assert_same_state(states[2], loop_state(loop2), "loaded state")
    for _ in range(3):
        loop2.step()
    d1, g1 = loop2.losses()
    assert_same_state(states[5], loop_state(loop2), "3 + resume + 3 vs 6")
    assert np.array_equal(np.concatenate((d0, d1)), d_rec) and np.array_equal(np.concatenate((g0, g1)), g_rec)
    # a loop without the average ignores the one in the state
    loop3 = make_loop(tmp_path / "c")
    loop3.load_state_dict(torch.load(path, weights_only=False))
    assert loop3.trainer.fG.ema is None
    assert_same_state({k: v for k, v in states[2].items() if k != "G.ema"}, loop_state(loop3), "state into a loop without")


def test_resume_without_average_and_mismatch(tmp_path):
    plain = make_loop(tmp_path / "a")
    for _ in range(3):
        plain.step()
    sd = plain.state_dict()
    assert "ema" not in sd
    loop = make_loop(tmp_path / "b", ema_decay=DECAY)
    with pytest.warns(UserWarning, match="average"):
        loop.load_state_dict(sd)
    f = loop.trainer.fG
    assert same_bits(f.ema, f.flat) and same_bits(f.flat, sd["G"]["flat"])
    sd2 = loop.state_dict()
    other = make_loop(tmp_path / "c", ema_decay=0.999)
    with pytest.raises(ValueError, match="decay"):
        other.load_state_dict(sd2)
    other = make_loop(tmp_path / "d", ema_decay=DECAY, ema_warmup=0.0)
    with pytest.raises(ValueError, match="warmup"):
        other.load_state_dict(sd2)


# ---- 5. sampling ---------------------------------------------------------------------------------------------------------

def test_sampler_over_the_average_follows_training(tmp_path):
    """a captured Sampler over ema_generator() against a Sampler with the same seed and counter on a freshly constructed
    Generator loaded from ema_generator().state_dict(): bit for bit, before and after four more training replays (the same
    captured Sampler, no rebuild); the live generator's samples differ.
    The fresh generator's parameters are laid into one flat buffer (FlatParams) like the averaged module's: the Sampler's
    launch sequence depends on the storage form - with the gcn and residual weights of a block in ONE buffer the head
    contraction is one launch over both row blocks (gen_trunk._head_conv), with separate tensors it is two - and the two
    forms round differently.  The difference to a fresh generator on per-tensor storage is printed (not asserted: it is a
    property of the Sampler's schedule, the same for the live generator)."""
    c, G, D, _, _ = build_pair(CFG, DEV)
    loop = TrainLoop(G, D, loop_feeder(tmp_path), B_LOOP, c["t_size"], n_critic=N_CRITIC, seed=SEED_LOOP, ema_decay=DECAY)
    for _ in range(3):
        loop.step()
    E = loop.ema_generator()
    assert loop.ema_generator() is E and not E.training and G.training
    assert list(E.state_dict().keys()) == list(G.state_dict().keys())
    lo = loop.trainer.fG.ema.data_ptr()
    for (k, p), off in zip(E.named_parameters(), loop.trainer.fG.offsets):
        assert p.data_ptr() == lo + 4 * off and not p.requires_grad, k
    for (k, b), (_, lb) in zip(E.named_buffers(), G.named_buffers()):
        assert b.data_ptr() == lb.data_ptr(), k
    s = Sampler(E, qtd=2, seed=7)
    live = Sampler(G, qtd=2, seed=7)
    assert s.use_graph

    def fresh_output(counter, flat=True):
        F = Generator(c["latent"], c["channels"], c["n_classes"], c["t_size"], c["mlp"], dataset="h36m").to(DEV)
        F.load_state_dict(E.state_dict(), strict=True)
        keep = FlatParams(F) if flat else None      # noqa: F841  (the buffer the parameters now live in)
        fs = Sampler(F, qtd=2, seed=7)
        fs.load_state_dict({"seed": 7, "step": counter})
        out, _, _ = fs.next()
        torch.cuda.synchronize()
        return out.clone()
    for rnd_ in range(2):
        stats = {k: v.clone() for k, v in G.named_buffers()}
        ema = loop.trainer.fG.ema.clone()
        want = fresh_output(rnd_)
        imgs, _, _ = s.next()
        imgs_live, _, _ = live.next()
        torch.cuda.synchronize()
        assert torch.isfinite(imgs).all()
        other = fresh_output(rnd_, flat=False)
        print("round %d: Sampler(ema_generator()) vs fresh generator, flat storage: max |d| %.3e; per-tensor storage: max |d| %.3e"
              % (rnd_, (imgs - want).abs().max().item(), (imgs - other).abs().max().item()))
        assert same_bits(imgs, want), rnd_
        assert not same_bits(imgs, imgs_live), rnd_
        assert same_bits(loop.trainer.fG.ema, ema) and all(torch.equal(v, stats[k]) for k, v in G.named_buffers())
        if rnd_ == 0:
            first = imgs.clone()
            for _ in range(4):                   # four more training replays; the SAME captured Sampler again
                loop.step()
            torch.cuda.synchronize()
            assert not same_bits(loop.trainer.fG.ema, ema)
        else:
            assert not same_bits(imgs, first)
    assert loop.step_count == 7 and s.step_count == 2


# ---- 6. commands ---------------------------------------------------------------------------------------------------------

def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_commands(tmp_path):
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 13, 2, 40, 16, 10, "h36m", seed=6)
    common = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--n_epochs", "2", "--batch_size", "4", "--dataset", "h36m",
              "--channels", "2", "--v_size", "16", "--t_size", "32", "--n_classes", "10", "--n_critic", "2",
              "--sample_interval", "4", "--checkpoint_interval", "3", "--log_interval", "2", "--seed", "1",
              "--data_path", dp, "--label_path", lp]
    out_e, out_p = str(tmp_path / "run_ema"), str(tmp_path / "run_plain")
    r = subprocess.run(common + ["--out", out_e, "--ema_decay", "0.99"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run(common + ["--out", out_p], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    today = ["actions/0.npy", "actions/4.npy", "config.txt", "loop_state.pth", "models/discriminator_0.pth",
             "models/discriminator_3.pth", "models/generator_0.pth", "models/generator_3.pth", "plot_loss.mat"]
    assert _tree(out_p) == today
    assert _tree(out_e) == sorted(today + ["actions_ema/0.npy", "actions_ema/4.npy", "models/generator_ema_0.pth",
                                           "models/generator_ema_3.pth"])
    # the live outputs of the two runs are the same files: the average only observes (actions draw from numpy's global
    # generator, unseeded, so those are compared by shape)
    for name in ("generator_0.pth", "generator_3.pth", "discriminator_3.pth"):
        a = torch.load(os.path.join(out_e, "models", name))
        b = torch.load(os.path.join(out_p, "models", name))
        assert list(a.keys()) == list(b.keys()) and all(torch.equal(a[k], b[k]) for k in a), name
    acts = np.load(os.path.join(out_e, "actions_ema", "4.npy"))
    assert acts.shape == (100, 2, 32, 16) and np.isfinite(acts).all()
    live3 = torch.load(os.path.join(out_e, "models", "generator_3.pth"))
    ema0 = torch.load(os.path.join(out_e, "models", "generator_ema_0.pth"))
    ema3 = torch.load(os.path.join(out_e, "models", "generator_ema_3.pth"))
    G = Generator(512, 2, 10, 32, 4, dataset="h36m")
    assert list(ema3.keys()) == list(G.state_dict().keys())
    G.load_state_dict(ema3, strict=True)
    k = "mlp.mlp.0.weight"
    assert not torch.equal(ema3[k], live3[k]) and not torch.equal(ema3[k], ema0[k])
    assert all(torch.equal(ema3[q], live3[q]) for q in ema3 if "running_" in q or "num_batches" in q)      # shared statistics
    # tools/generate.py takes the averaged checkpoint like any generator checkpoint
    gen_out = str(tmp_path / "gen")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "generate.py"), "--batch_size", "5", "--gen_qtd", "10", "--dataset", "h36m",
           "--channels", "2", "--v_size", "16", "--t_size", "32", "--n_classes", "10",
           "--model", os.path.join(out_e, "models", "generator_ema_0.pth"), "--out", gen_out, "--seed", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = sorted(os.listdir(os.path.join(gen_out, "actions")))
    assert len(files) == 3 and [f.split("_gen_")[1] for f in files] == ["data.npy", "label.pkl", "z.npy"], files
    data = np.load(os.path.join(gen_out, "actions", files[0]))
    assert data.shape == (100, 2, 32, 16) and np.isfinite(data).all()
