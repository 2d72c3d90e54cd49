"""project.Projector on the MI355X with the tiny generator of proj_def.tiny_pair (H36M graph, latent 32, 3 classes, t_size 16,
mlp_dim 4, oracle.fill.fill_module(seed=1), n = 3): the generator stands still, a replayed run equals an eager one bit for bit,
the best-so-far record is the running minimum of the history, the objective curve follows the float64 loop on the oracle
generator, masked-out target entries are never looked at, and metrics.reconstruction / tools/project_actions.py on top.

Against the float64 loop (proj_def.end_to_end_case: seed 4, the first whose float64 curve is stable under perturbations of
float32 size): E = 1.35e-5 and the float32 loop's deviation in best_w = 1.62e-6 on a CPU; the Projector under CPU emulation of the
generator's kernels stays at 0.65 E and 1.47 of that deviation (tests/test_proj_cpu.py); the GPU figures are printed by the
test and quoted in DESIGN.md 29."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, metrics
from kinetic_gan_amd.project import Projector

import proj_def

pytestmark = pytest.mark.gpu
N, STEPS = proj_def.TINY["n"], proj_def.TINY["steps"]
PLAIN = dict(dataset="h36m", steps=STEPS, lr=0.05, lambdas=(1.0, 1.0, 0.1), lambda_w=0.0, ramp_up=0.0, ramp_down=0.0, mean_size=64)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


@pytest.fixture(scope="module")
def G():
    return proj_def.tiny_pair("cuda")[0]


@pytest.fixture(scope="module")
def case():
    return proj_def.end_to_end_case()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def snapshot(G):
    return dict(state={k: v.clone() for k, v in G.state_dict().items()}, grads=[None if p.grad is None else p.grad.clone() for p in G.parameters()],
                req=[p.requires_grad for p in G.parameters()], training=[m.training for m in G.modules()])


def assert_stands_still(G, snap):
    for k, v in G.state_dict().items():
        assert v.dtype == snap["state"][k].dtype and torch.equal(v, snap["state"][k]), k
    for p, g, r in zip(G.parameters(), snap["grads"], snap["req"]):
        assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g)) and p.requires_grad == r
    assert [m.training for m in G.modules()] == snap["training"]


# ---- 1. the generator stands still ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_graph", [True, False])
def test_the_generator_stands_still(G, case, use_graph):
    G.train()
    G.st_gcn_networks[3].eval()                                           # a mixed set of flags must come back as it was
    params = list(G.parameters())
    params[0].grad = torch.full_like(params[0], 0.25)                     # one .grad present, the others None
    params[1].requires_grad_(False)
    try:
        snap = snapshot(G)
        p = Projector(G, N, use_graph=use_graph, lambda_w=0.01, dataset="h36m", steps=5, mean_size=64, noise="fixed")
        assert_stands_still(G, snap)
        out = p.project(case["y"], case["labels"])
        torch.cuda.synchronize()
        assert_stands_still(G, snap)
        assert torch.isfinite(out["history"]).all() and out["nonfinite"].tolist() == [0] * N
    finally:
        params[0].grad = None
        params[1].requires_grad_(True)
        G.train()


# ---- 2. replay = eager ------------------------------------------------------------------------------------------------------------

def test_replay_equals_eager(G, case):
    kw = dict(PLAIN, ramp_up=0.1, ramp_down=0.25, lambda_w=0.01)
    a = Projector(G, N, use_graph=True, **kw).project(case["y"], case["labels"], w_init=case["w_init"])
    b = Projector(G, N, use_graph=False, **kw).project(case["y"], case["labels"], w_init=case["w_init"])
    for k in ("w", "best_w", "history", "best_loss", "best_obj", "loss"):
        assert same_bits(a[k], b[k]), k
    assert torch.isfinite(a["history"]).all()
    # a second run on the same graph, from the class means this time: the captured iteration is reused
    p = Projector(G, N, use_graph=True, **kw)
    first = p.project(case["y"], case["labels"], w_init=case["w_init"])
    graph = p._graph
    again = p.project(case["y"], case["labels"])
    assert p._graph is graph and same_bits(first["history"], a["history"]) and not same_bits(again["history"], a["history"])
    assert same_bits(p.project(case["y"], case["labels"], w_init=case["w_init"])["best_w"], a["best_w"])


# ---- 3. best-keeping --------------------------------------------------------------------------------------------------------------

def test_best_keeping_step_by_step(G, case):
    p = Projector(G, N, use_graph=False, **PLAIN)
    rec = []

    def on_step(s):
        rec.append(dict(w=p.w.detach().clone(), obj=p.loss[:, 0].clone(), best_obj=p.best_obj.clone(), best_w=p.best_w.clone()))

    out = p.project(case["y"], case["labels"], w_init=case["w_init"], on_step=on_step)
    assert len(rec) == STEPS
    w_in = [case["w_init"].cuda()] + [r["w"] for r in rec[:-1]]          # the w that entered step s
    hist = out["history"]
    run_min = torch.full((N,), float("inf"), device="cuda")
    arg = [0] * N
    for s, r in enumerate(rec):
        assert same_bits(hist[s], r["obj"]), s                            # lambda_w = 0: the objective is the loss word
        for i in range(N):
            if hist[s, i] < run_min[i]:
                run_min[i], arg[i] = hist[s, i], s
        assert same_bits(r["best_obj"], run_min), s
        assert same_bits(r["best_w"], torch.stack([w_in[arg[i]][i] for i in range(N)])), s
    assert same_bits(out["best_obj"], hist.min(0).values) and same_bits(out["best_loss"][:, 0], out["best_obj"])


# ---- 4, 5. against the float64 loop; it inverts --------------------------------------------------------------------------------------

def test_against_the_float64_oracle_loop(G, case):
    out = Projector(G, N, use_graph=True, **PLAIN).project(case["y"], case["labels"], w_init=case["w_init"])
    hist = out["history"].double().cpu().numpy()
    E, dw, r64 = case["E"], case["dw"], case["r64"]
    dev = float(np.abs(hist / r64["history"] - 1.0).max())
    dwp = float(np.abs(out["best_w"].double().cpu().numpy() - r64["best_w"]).max())
    print("seed %d: E = %.3g, float32 loop's deviation in best_w = %.3g" % (case["seed"], E, dw))
    print("objective curve: deviation / E = %.3f;  best_w: deviation / float32 loop's = %.3f" % (dev / E, dwp / dw))
    assert dev <= 4 * E, (dev, E)
    assert dwp <= 4 * dw, (dwp, dw)
    # it actually inverts: every sample's best objective is at most half its first
    best, first = out["best_obj"].cpu().numpy(), hist[0]
    print("best / first objective:", (best / first).tolist(), " float64 loop:", (r64["best_obj"] / r64["history"][0]).tolist())
    assert (best <= 0.5 * first).all()
    assert out["nonfinite"].tolist() == [0] * N
    # recon is the synthesis of best_w: its objective is the best objective up to the difference of the two forward paths
    lo, _ = _native.proj_loss(out["recon"], case["y"].cuda(), proj_def.TINY_BONES, PLAIN["lambdas"])
    assert np.allclose(lo[:, 0].cpu().numpy(), best, rtol=1e-3)


# ---- 6. completion ------------------------------------------------------------------------------------------------------------------

def test_completion_never_looks_at_masked_entries(G, case):
    mask = torch.ones(16, 16)
    mask[4:12, [3, 6, 12]] = 0.0
    y0, yn = case["y"].clone(), case["y"].clone()
    y0[:, :, 4:12, [3, 6, 12]] = 0.0
    yn[:, :, 4:12, [3, 6, 12]] = float("nan")
    p = Projector(G, N, use_graph=True, **PLAIN)
    a = p.project(yn, case["labels"], mask=mask, w_init=case["w_init"])
    b = p.project(y0, case["labels"], mask=mask, w_init=case["w_init"])
    for k, v in a.items():
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(v, b[k]) if v.dtype != torch.float32 else same_bits(v, b[k]), k
    assert (a["best_obj"] <= 0.5 * a["history"][0]).all()
    full = p.project(case["y"], case["labels"], w_init=case["w_init"])
    assert not same_bits(full["history"], a["history"])                   # (the mask does change the objective)


# ---- 7. metrics.reconstruction --------------------------------------------------------------------------------------------------------

def test_metrics_reconstruction(G, case):
    g = torch.Generator().manual_seed(3)
    K, P = 3, 2
    real = torch.cat([case["y"], case["y"].flip(0) * 0.9])[torch.randperm(6, generator=g)]
    labels = np.array([0, 1, 2, 2, 0, 1])
    kw = dict(steps=10, lr=0.05, ramp_up=0.0, ramp_down=0.2, mean_size=64)
    out = metrics.reconstruction(G, real, labels, dataset="h36m", per_class=P, n=6, **kw)
    idx = np.stack([np.flatnonzero(labels == c)[:P] for c in range(K)]).reshape(-1)
    one = Projector(G, 6, dataset="h36m", **kw).project(real[idx], np.repeat(np.arange(K), P))
    assert out["per_sample"].shape == (K, P, 4) and out["values"].shape == (K, 3) and out["mean"].shape == (3,)
    assert same_bits(out["per_sample"], one["best_loss"].reshape(K, P, 4))
    assert same_bits(out["values"], one["best_loss"].reshape(K, P, 4)[:, :, 1:].mean(1))
    assert same_bits(out["mean"], out["values"].mean(0)) and (out["mean"] > 0).all()
    assert same_bits(out["best_w"].reshape(6, -1), one["best_w"]) and out["recon"].shape == (K, P, 2, 16, 16)
    assert metrics.RECON_NAMES == ("recon_pos", "recon_vel", "recon_bone")
    # batches of 4: the last one is filled up; the scores agree up to the batch size's effect on the generator's kernels
    four = metrics.reconstruction(G, real, labels, dataset="h36m", per_class=P, n=4, **kw)
    assert four["per_sample"].shape == (K, P, 4) and torch.allclose(four["per_sample"], out["per_sample"], rtol=5e-2)
    with pytest.raises(ValueError, match="per_class=3 needed"):
        metrics.reconstruction(G, real, labels, dataset="h36m", per_class=3)


# ---- 8. the tool --------------------------------------------------------------------------------------------------------------------

def test_project_actions_tool_end_to_end(G, case, tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import project_actions
    K, P, n = 3, 2, 12
    rng = np.random.RandomState(0)
    base = case["y"].numpy()
    real = np.concatenate([base * s for s in (1.0, 0.9, 0.8, 0.7)]).astype(np.float32)      # 12 samples in [-1, 1]
    real[0, 0, 0, 0], real[1, 0, 0, 0] = 1.0, -1.0                        # the feeder's normalisation is then the identity
    lab = rng.permutation(np.repeat(np.arange(K), n // K))
    np.save(tmp_path / "real.npy", real)
    with open(tmp_path / "real.pkl", "wb") as f:
        pickle.dump(([str(i) for i in range(n)], lab.tolist()), f)
    torch.save(G.state_dict(), tmp_path / "generator_0.pth")
    argv = ["--model", str(tmp_path / "generator_0.pth"), "--data_real", str(tmp_path / "real.npy"), "--labels_real",
            str(tmp_path / "real.pkl"), "--dataset", "h36m", "--latent_dim", "32", "--n_classes", "3", "--t_size", "16", "--per_class",
            str(P), "--steps", "10", "--mean_size", "64", "--batch", "6", "--out", str(tmp_path / "out")]
    res = project_actions.main(argv)
    text = capsys.readouterr().out
    loss, w, data = (np.load(tmp_path / "out" / f) for f in ("proj_loss.npy", "proj_w.npy", "proj_data.npy"))
    assert loss.shape == (K * P, 4) and w.shape == (K * P, 35) and data.shape == (K * P, 2, 16, 16) and np.isfinite(data).all()
    means = loss.reshape(K, P, 4)[:, :, 1:].astype(np.float64).mean(1).mean(0).tolist()
    assert [res[k] for k in metrics.RECON_NAMES] == means
    assert all(("%s %.6g" % (k, v)) in text for k, v in zip(metrics.RECON_NAMES, means)) and "held_out_pos" not in text
    with open(tmp_path / "out" / "proj_label.pkl", "rb") as f:
        assert np.asarray(pickle.load(f)).shape == (2, K * P)
    res2 = project_actions.main(argv + ["--mask_frames", "4:12", "--mask_joints", "3", "6", "12"])
    text2 = capsys.readouterr().out
    assert "held_out_pos" in text2 and np.isfinite(res2["held_out_pos"]) and res2["held_out_pos"] > 0
    assert res2["recon_pos"] != res["recon_pos"]
