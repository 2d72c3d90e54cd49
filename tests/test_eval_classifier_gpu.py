"""The action classifier's scores inside the Evaluator on the MI355X: the four new columns against their
composition (a twin Sampler round + metrics.classifier_scores), the untouched MMD / PRDC / Frechet columns, replay against
eager, the launch counts, the untouched classifier, selection by accuracy and by feature FD, resume, the training loop, the
command, and metrics.classifier_scores with the pair counts on against the float64 definition of kg_cls_scores.

Four classes, P = 3 samples per class, classifier_batch = 8: a round of 12 samples takes two ragged chunks (8 + 4)."""
import csv
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import metrics
from kinetic_gan_amd.classifier import Classifier
from kinetic_gan_amd.classify import ClassifierLoop
from kinetic_gan_amd.discriminator import Discriminator
from kinetic_gan_amd.evaluate import Evaluator
from kinetic_gan_amd.feeder import Feeder
from kinetic_gan_amd.generator import Generator
from kinetic_gan_amd.sample import Sampler
from kinetic_gan_amd.train import TrainLoop
from kinetic_gan_amd.wgan_gp import FlatParams

import cls_def
import eval_prdc_def
import train_def
from cls_scores_def import cls_scores_def

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K, C, T, V, LATENT, MLP = 4, 2, 32, 16, 512, 4
SEED_EV, P, CB, SD, SL = 5, 3, 8, 7, 2
CLS_KW = dict(classifier_per_class=P, classifier_batch=CB, diversity_pairs=SD, multimodality_pairs=SL)
NEW = ["%s/%s" % (g, q) for g in ("a", "b") for q in metrics.CLS_NAMES]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    x, y = bits(a), bits(b)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)


def assert_same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert same_bits(a[k], b[k]), "%s: %s differs" % (what, k)


def _write_set(path, x, y):
    os.makedirs(path, exist_ok=True)
    dp, lp = os.path.join(path, "data.npy"), os.path.join(path, "label.pkl")
    np.save(dp, x.numpy())
    with open(lp, "wb") as f:
        pickle.dump((["s%d" % i for i in range(len(y))], [int(v) for v in y]), f)
    return Feeder(dp, lp, norm=False, dataset="h36m")


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Classifier(2, 4, 32, latent=64, feat_dim=8) trained as in tests/test_classifier_gpu.py: torch's default initialisation
    under manual_seed(0), 100 replayed iterations of batch 16 on cls_def.synthetic_set"""
    x, y = cls_def.synthetic_set(10)
    feeder = _write_set(str(tmp_path_factory.mktemp("toy")), x, y)
    torch.manual_seed(0)
    clf = Classifier(C, K, T, latent=64, feat_dim=8, dataset="h36m").to(DEV)
    loop = ClassifierLoop(clf, feeder, 16, T, seed=0, lr=1e-3, b1=0.9, b2=0.999, use_graph=True)
    for _ in range(100):
        loop.step()
    torch.cuda.synchronize()
    return clf


def real_set():
    """eight samples per class of the toy distribution, shuffled: the Evaluator takes the first P of every class"""
    x, y = cls_def.synthetic_set(33, n_classes=K, per_class=8)
    perm = np.random.RandomState(1).permutation(len(y))
    return x[perm], y[perm].numpy()


def flat_generator(seed=1):
    torch.manual_seed(seed)
    G = Generator(LATENT, C, K, T, MLP, dataset="h36m").to(DEV)
    G._flat_keep = FlatParams(G)
    return G


def ev_state(ev):
    out = {"count": ev.count, "ring_val": ev.ring_val, "ring_iter": ev.ring_iter, "best_val": ev.best_val, "best_iter": ev.best_iter,
           "snap_flat": ev.snap_flat}
    for k, b in ev.snap_buffers.items():
        out["snap." + k] = b
    for name, group in (("step.", ev.samplers), ("prdc_step.", ev.prdc_samplers), ("frechet_step.", ev.frechet_samplers),
                        ("cls_step.", ev.cls_samplers)):
        for k, s in group.items():
            out[name + k] = s.step_dev
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def make_ev(gens, it=None, **kw):
    kw.setdefault("select", "a/avg")
    x, y = real_set()
    return Evaluator(gens, x, real_labels=y, pairs=2, seed=SEED_EV, iteration=it, ring_len=8, **kw)


# shared: the PRDC round (and with it the Frechet round) has the classifier's count and is read in place; own: it has not
KINDS = {"shared": dict(prdc_per_class=P, prdc_k=2, frechet_per_class=P), "own": dict(prdc_per_class=4, prdc_k=2)}


@pytest.fixture(scope="module")
def composed(trained):
    Ga, Gb = flat_generator(), flat_generator()
    before = [p.detach().clone() for p in trained.parameters()]
    mode = trained.training
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    evs = {}
    for kind, kw in KINDS.items():
        evs[kind] = make_ev({"a": Ga, "b": Gb}, it, classifier=trained, **CLS_KW, **kw)
        evs[kind + "/plain"] = make_ev({"a": Ga, "b": Gb}, it, **kw)
    assert all(e.use_graph for e in evs.values())
    states = {k: [] for k in evs}
    for k in range(3):
        for name, e in evs.items():
            e.evaluate()
            states[name].append(ev_state(e))
        it += 2
    return dict(Ga=Ga, Gb=Gb, clf=trained, before=before, mode=mode, evs=evs, states=states,
                recs={k: e.records() for k, e in evs.items()})


def twin_round(G, counter, qtd):
    s = Sampler(G, qtd=qtd, seed=SEED_EV, use_graph=False)
    s.load_state_dict({"seed": SEED_EV, "step": counter})
    out, _, _ = s.next()
    torch.cuda.synchronize()
    return out, s


@pytest.mark.parametrize("kind", list(KINDS))
def test_columns_equal_the_composition(composed, kind):
    ev, rec, plain = composed["evs"][kind], composed["recs"][kind], composed["recs"][kind + "/plain"]
    n_old = len(plain["names"])
    assert rec["names"] == plain["names"] + NEW and rec["scores"].shape == (3, n_old + 8)
    # the MMD, PRDC and Frechet columns do not move, and neither does what they decide
    assert same_bits(rec["scores"][:, :n_old], plain["scores"])
    assert same_bits(rec["improved"], plain["improved"]) and same_bits(rec["iteration"], plain["iteration"])
    assert ev.best() == composed["evs"][kind + "/plain"].best()
    last, last_plain = composed["states"][kind][-1], composed["states"][kind + "/plain"][-1]
    for key in last_plain:
        if key != "ring_val":
            assert same_bits(last[key], last_plain[key]), key
    # a shared round is not a Sampler of its own, and nothing is counted twice
    assert len(ev.cls_samplers) == (0 if kind == "shared" else 2)
    assert len(ev._all_samplers()) == len(set(map(id, ev._all_samplers()))) == (4 if kind == "shared" else 6)
    assert all(s.step_count == 3 for s in ev._all_samplers())
    # the real side: the first P samples of every class, class by class
    x, y = real_set()
    rows = np.concatenate([np.flatnonzero(y == c)[:P] for c in range(K)])
    real, lab_real = x[rows], y[rows]
    clf = composed["clf"]
    for k in range(3):
        out, s = twin_round(composed["Ga"], k, P)
        assert out.shape == (K * P, C, T, V) and s.labels_np.tolist() == list(range(K)) * P
        want = metrics.classifier_scores(clf, out, s.labels_np, real, lab_real, batch=CB, class_fd=False, diversity_pairs=SD,
                                         multimodality_pairs=SL, pair_seed=SEED_EV)
        cols = [np.float32(want["accuracy"]).reshape(1), want["feature_fd"].to(torch.float32).reshape(1),
                want["diversity"].to(torch.float32).reshape(1), want["multimodality"].to(torch.float32).reshape(1)]
        print("evaluation", k, dict(zip(metrics.CLS_NAMES, [float(np.asarray(c.cpu() if torch.is_tensor(c) else c)[0]) for c in cols])))
        for i, col in enumerate(cols):
            assert same_bits(rec["scores"][k, n_old + i:n_old + i + 1], col), (k, metrics.CLS_NAMES[i])
        if k == 0:
            cr = ev.classifier_real
            assert same_bits(cr["diversity"], want["diversity_real"]) and same_bits(cr["multimodality"], want["multimodality_real"])
            assert float(cr["accuracy"]) == want["accuracy_real"] and same_bits(cr["features"], want["features_real"])
            div, mm = metrics.cls_pair_tables(s.labels_np, K, SD, SL, SEED_EV)
            assert same_bits(ev._cls_tables[0], div) and same_bits(ev._cls_tables[1], mm)
    new = rec["scores"][:, n_old:]
    assert np.isfinite(new).all() and (new[:, [0, 4]] >= 0).all() and (new[:, [0, 4]] <= 1).all() and (new[:, [1, 2, 3, 5, 6, 7]] > 0).all()
    assert same_bits(new[:, :4], new[:, 4:])             # equal weights behind another Sampler
    state = ev.state_dict()
    assert state["classifier"] == {"per_class": P, "diversity_pairs": SD, "multimodality_pairs": SL}
    assert "classifier" not in composed["evs"][kind + "/plain"].state_dict() and state["names"] == plain["names"] + NEW
    assert not any("weight" in k for k in state)         # the classifier's weights are the caller's


@pytest.mark.parametrize("kind", list(KINDS))
def test_replays_equal_eager_evaluations(composed, kind):
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, it, use_graph=False, classifier=composed["clf"], **CLS_KW, **KINDS[kind])
    for k in range(3):
        ev.evaluate()
        it += 2
        assert_same(composed["states"][kind][k], ev_state(ev), "graph vs eager, evaluation %d" % k)
    a, b = ev.records(), composed["recs"][kind]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))


def test_launch_counts_for_two_generators(composed, monkeypatch):
    calls = {"cls_scores": [], "frechet_sets": [], "frechet_real": []}
    plain = {k: getattr(nv, k) for k in calls}
    monkeypatch.setattr(nv, "cls_scores", lambda feats, *a, **kw: (calls["cls_scores"].append(len(list(feats))), plain["cls_scores"](feats, *a, **kw))[1])
    monkeypatch.setattr(nv, "frechet_sets", lambda cache, fakes, *a, **kw: (calls["frechet_sets"].append(len(list(fakes))),
                                                                          plain["frechet_sets"](cache, fakes, *a, **kw))[1])
    monkeypatch.setattr(nv, "frechet_real", lambda *a, **kw: (calls["frechet_real"].append(1), plain["frechet_real"](*a, **kw))[1])
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, use_graph=False, classifier=composed["clf"], **CLS_KW)
    assert calls == {"cls_scores": [1], "frechet_sets": [], "frechet_real": [1]}      # the real side, once, at construction
    counted = {}
    nv.flop_count = counted
    try:
        for _ in range(2):
            for v in calls.values():
                del v[:]
            ev.evaluate()
            torch.cuda.synchronize()
            assert calls == {"cls_scores": [2], "frechet_sets": [2], "frechet_real": []}, calls
    finally:
        nv.flop_count = None
    assert "kg_cls_scores" in counted and "kg_frechet_real" not in counted


def test_classifier_untouched(composed):
    clf = composed["clf"]
    assert clf.training == composed["mode"]
    for p, q in zip(clf.parameters(), composed["before"]):
        assert same_bits(p, q)


# ---- selection -----------------------------------------------------------------------------------------------------------

# the scale factors of the weights, evaluation by evaluation.  An untrained generator is recognised at chance level whatever
# its label, so its accuracy moves in steps of 1/12 at most and mostly stays at 3/12: with the first list one MI355X recorded
# 0.25, 0.25, 0.25, 0.3333, 0.25, 0.25 - a second improvement at the fourth evaluation, behind equal scores and the NaN weights.
# The assertions below hold for whatever values are recorded.
SCALES_ACC = [1.0, 4.0, float("nan"), 8.0, 16.0, 4.0]
SCALES = [1.0, 0.9, float("nan"), 1.1, 0.8, 1.0]


@pytest.mark.parametrize("name,col,maximise,SCALES", [("live/accuracy", 2, True, SCALES_ACC), ("live/feature_fd", 3, False, SCALES)])
def test_selection(trained, name, col, maximise, SCALES):
    """the generator's weights are scaled between the evaluations, and once they are NaN; the improved flags and best() are the
    record definition's, fed with the device's scores; the snapshot holds the weights of the best evaluation"""
    G = flat_generator(3)
    flat = G._flat_keep.flat
    orig = flat.clone()
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    ev = make_ev({"live": G}, it, select=name, classifier=trained, **CLS_KW)
    worst = float("-inf") if maximise else float("inf")
    assert ev.maximise == maximise and ev.best() == {"value": worst, "iteration": -1}
    assert ev.names == ["live/avg", "live/joint"] + ["live/" + q for q in metrics.CLS_NAMES]
    weights = []
    for k, s in enumerate(SCALES):
        with torch.no_grad():
            flat.copy_(orig * s)
        weights.append(flat.detach().clone())
        it.fill_(10 * (k + 1))
        ev.evaluate()
    rec, best = ev.records(), ev.best()
    v = rec["scores"][:, col]
    print(name, "per evaluation:", v.tolist(), "improved:", rec["improved"].tolist(), "best:", best)
    ref = eval_prdc_def.Record2(6, col, 8, maximise=maximise)
    for k in range(len(SCALES)):
        ref.append(rec["scores"][k], rec["iteration"][k])
    assert rec["improved"].tolist() == ref.ring_iter[:len(SCALES), 1].astype(bool).tolist() and rec["improved"][0]
    assert best == {"value": float(ref.best_val), "iteration": int(ref.best_iter)}
    ok = np.isfinite(v)
    pick = (np.nanmax if maximise else np.nanmin)(v)
    first = int(np.flatnonzero(ok & (v == pick))[0])     # the FIRST best value: an equal score keeps the earlier snapshot
    assert best["value"] == float(pick) and best["iteration"] == 10 * (first + 1)
    assert same_bits(ev.snap_flat, weights[first])
    # exactly at the evaluations where the column improved: a strictly better value than every earlier one
    run = worst
    for k, x in enumerate(v.tolist()):
        better = (x > run) if maximise else (x < run)
        assert bool(rec["improved"][k]) == better, k
        run = x if better else run
    if not maximise:
        assert np.isnan(v[2]) and not rec["improved"][2] and len(set(v[ok].tolist())) > 1      # a NaN never wins


def test_select_rejection_resume_and_other_columns(composed):
    gens = {"a": composed["Ga"], "b": composed["Gb"]}
    clf = composed["clf"]
    for name in ("a/diversity", "b/multimodality"):
        with pytest.raises(ValueError, match="closer"):
            make_ev(gens, select=name, classifier=clf, **CLS_KW)
    # construction checks
    with pytest.raises(ValueError, match="diversity_pairs"):
        make_ev(gens, classifier=clf, **dict(CLS_KW, diversity_pairs=K * P + 1))
    with pytest.raises(ValueError, match="multimodality_pairs"):
        make_ev(gens, classifier=clf, **dict(CLS_KW, multimodality_pairs=P + 1))
    with pytest.raises(ValueError, match="classes"):
        make_ev(gens, classifier=Classifier(C, K + 1, T, latent=64, feat_dim=8, dataset="h36m").to(DEV), **CLS_KW)
    with pytest.raises(ValueError, match="frames"):
        make_ev(gens, classifier=Classifier(C, K, T // 2, latent=64, feat_dim=8, dataset="h36m").to(DEV), **CLS_KW)
    with pytest.raises(ValueError, match="is on"):
        make_ev(gens, classifier=Classifier(C, K, T, latent=64, feat_dim=8, dataset="h36m"), **CLS_KW)
    # state_dict -> load_state_dict continues bit for bit
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    first = make_ev(gens, it, classifier=clf, **CLS_KW, **KINDS["own"])
    first.evaluate()
    it += 2
    sd = first.state_dict()
    second = make_ev(gens, it, classifier=clf, **CLS_KW, **KINDS["own"])
    second.load_state_dict(sd)
    for k in (1, 2):
        second.evaluate()
        it += 2
        assert_same(composed["states"]["own"][k], ev_state(second), "1 + resume + %d" % k)
    a, b = second.records(), composed["recs"]["own"]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))
    # a state with other columns, or other pair counts, is rejected before anything is loaded
    for other in (make_ev(gens, it, **KINDS["own"]), make_ev(gens, it, classifier=clf, **dict(CLS_KW, diversity_pairs=SD - 1), **KINDS["own"])):
        keep = ev_state(other)
        with pytest.raises(ValueError, match="classifier"):
            other.load_state_dict(sd)
        assert_same(keep, ev_state(other), "a rejected state")
    with pytest.raises(ValueError, match="classifier"):
        second.load_state_dict(composed["evs"]["own/plain"].state_dict())
    sd2 = dict(sd, names=sd["names"][:-1] + ["b/other"])
    with pytest.raises(ValueError, match="names"):
        second.load_state_dict(sd2)


# ---- the training loop and the command -----------------------------------------------------------------------------------

B_LOOP, SEED_LOOP, N_CRITIC, DECAY = 4, 3, 2, 0.9
LOOP_NAMES = ["live/avg", "live/joint", "ema/avg", "ema/joint"] + ["%s/%s" % (g, q) for g in ("live", "ema") for q in metrics.CLS_NAMES]


def loop_feeder(path, n=80):
    os.makedirs(path, exist_ok=True)
    dp, lp = train_def.synthetic_dataset(str(path), n, C, 40, V, K, "h36m", seed=4)
    return Feeder(dp, lp, dataset="h36m")


def loop_state(loop):
    tr = loop.trainer
    out = {}
    for name, f, m in (("G", tr.fG, loop.G), ("D", tr.fD, loop.D)):
        out[name + ".flat"], out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = f.flat, f.exp_avg, f.exp_avg_sq
        out[name + ".grad"], out[name + ".adam_step"] = f.grad, f.step
        for k, b in m.named_buffers():
            out[name + ".buf." + k] = b
    out["G.ema"] = tr.fG.ema
    out["step_dev"] = loop.step_dev
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def make_loop(path, clf, **kw):
    torch.manual_seed(1)
    G = Generator(LATENT, C, K, T, MLP, dataset="h36m").to(DEV)
    torch.manual_seed(2)
    D = Discriminator(C, K, T, LATENT, dataset="h36m").to(DEV)
    return TrainLoop(G, D, loop_feeder(path), B_LOOP, T, n_critic=N_CRITIC, seed=SEED_LOOP, eval_pairs=2, ema_decay=DECAY,
                     eval_interval=2, eval_classifier=clf, eval_classifier_samples=P, eval_classifier_batch=CB,
                     eval_diversity_pairs=SD, eval_multimodality_pairs=SL, **kw)


def test_train_loop_writes_the_eight_columns_and_resumes(trained, tmp_path):
    loop = make_loop(tmp_path / "six", trained, eval_select="ema/feature_fd")
    ev = loop.evaluator
    assert ev.names == LOOP_NAMES and ev.select == "ema/feature_fd" and not ev.maximise and ev.use_graph
    states = []
    for k in range(6):
        loop.step()
        states.append(loop_state(loop))
    want_ev, rec, best = ev_state(ev), ev.records(), ev.best()
    print("loop scores", rec["scores"].tolist(), "best", best)
    assert rec["iteration"].tolist() == [2, 4, 6] and rec["scores"].shape == (3, 12) and np.isfinite(rec["scores"]).all()
    from kinetic_gan_amd.evaluate import write_metrics_csv
    write_metrics_csv(str(tmp_path / "metrics.csv"), rec)
    rows = list(csv.reader(open(tmp_path / "metrics.csv")))
    assert rows[0] == ["iteration"] + LOOP_NAMES + ["improved"] and len(rows) == 4
    # a second loop takes the same steps; its state after three of them goes to a file
    first = make_loop(tmp_path / "a", trained, eval_select="ema/feature_fd")
    for k in range(3):
        first.step()
        assert_same(states[k], loop_state(first), "a second loop, iteration %d" % k)
    sd = first.state_dict()
    assert sd["eval"]["count"] == 1 and sd["eval"]["classifier"] == {"per_class": P, "diversity_pairs": SD, "multimodality_pairs": SL}
    path = str(tmp_path / "loop_state.pth")
    torch.save(sd, path)
    del first
    second = make_loop(tmp_path / "b", trained, eval_select="ema/feature_fd")
    with torch.no_grad():                      # a different starting point: everything must come from the file
        second.trainer.fG.flat.add_(0.25)
        second.evaluator.snap_flat.fill_(3.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        second.load_state_dict(torch.load(path, weights_only=False))
    for _ in range(3):
        second.step()
    assert_same(states[5], loop_state(second), "3 + resume + 3 vs 6")
    assert_same(want_ev, ev_state(second.evaluator), "3 + resume + 3 vs 6, evaluator")
    got = second.evaluator.records()
    assert all(same_bits(got[k], rec[k]) for k in ("iteration", "scores", "improved")) and second.evaluator.best() == best


def test_train_command(tmp_path):
    """tools/train.py takes a checkpoint of tools/train_classifier.py and refuses one whose meta has another t_size"""
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 64, C, 40, V, K, "h36m", seed=4)
    cdir = str(tmp_path / "clf")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_classifier.py"), "--data_path", dp, "--label_path", lp, "--dataset", "h36m",
           "--t_size", str(T), "--batch_size", "16", "--n_epochs", "1", "--latent", "64", "--feat_dim", "8", "--n_classes", str(K),
           "--out", cdir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ckpt = sorted(f for f in os.listdir(cdir) if f.startswith("classifier_") and f.endswith(".pth"))
    assert ckpt, os.listdir(cdir)
    ckpt = os.path.join(cdir, ckpt[-1])
    out = str(tmp_path / "run")
    base = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--n_epochs", "1", "--batch_size", "8", "--dataset", "h36m",
            "--channels", str(C), "--v_size", str(V), "--t_size", str(T), "--n_classes", str(K), "--n_critic", "2",
            "--sample_interval", "100", "--checkpoint_interval", "100", "--log_interval", "4", "--seed", "1",
            "--data_path", dp, "--label_path", lp, "--ema_decay", "0.9", "--eval_interval", "4", "--eval_pairs", "2",
            "--eval_classifier_samples", str(P), "--eval_classifier_batch", str(CB), "--eval_diversity_pairs", str(SD),
            "--eval_multimodality_pairs", str(SL), "--eval_select", "live/accuracy"]
    r = subprocess.run(base + ["--out", out, "--eval_classifier", ckpt], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "[best live/accuracy: " in r.stdout
    rows = list(csv.reader(open(os.path.join(out, "metrics.csv"))))
    assert rows[0] == ["iteration"] + LOOP_NAMES + ["improved"] and len(rows) == 3
    state = torch.load(os.path.join(out, "loop_state.pth"), weights_only=False)["eval"]
    assert state["select"] == "live/accuracy" and state["names"] == LOOP_NAMES
    back = np.array([[float(v) for v in r_[1:13]] for r_ in rows[1:]], dtype=np.float32)
    assert same_bits(back, state["records"]["scores"]) and np.isfinite(back).all()
    assert os.path.exists(os.path.join(out, "models", "generator_best.pth"))
    # another t_size in the checkpoint's meta: refused before anything is trained
    sd = torch.load(ckpt, weights_only=False)
    sd["meta"] = dict(sd["meta"], t_size=T // 2)
    bad = str(tmp_path / "classifier_bad.pth")
    torch.save(sd, bad)
    out2 = str(tmp_path / "run2")
    r = subprocess.run(base + ["--out", out2, "--eval_classifier", bad], capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "t_size" in r.stderr and "--eval_classifier" in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert not os.path.exists(os.path.join(out2, "metrics.csv"))


# ---- metrics.classifier_scores ---------------------------------------------------------------------------------------------

def test_classifier_scores_new_keys(trained):
    xg, yg = cls_def.synthetic_set(21, n_classes=K, per_class=5)
    xr, yr = cls_def.synthetic_set(22, n_classes=K, per_class=6)
    plain = metrics.classifier_scores(trained, xg, yg, xr, yr, batch=CB)
    assert set(plain) == {"correct", "features_gen", "features_real", "accuracy", "correct_real", "accuracy_real", "feature_fd",
                          "feature_fd_class_mean", "feature_fd_per_class"}                       # the parent's key set
    s = metrics.classifier_scores(trained, xg, yg, xr, yr, batch=CB, diversity_pairs=9, multimodality_pairs=3, pair_seed=4)
    assert set(s) >= set(plain) | {"diversity", "multimodality", "correct_per_class", "count_per_class", "diversity_real",
                                   "multimodality_real"}
    for k in plain:                                      # what was there keeps its bits
        assert (same_bits(s[k], plain[k]) if torch.is_tensor(plain[k]) else s[k] == plain[k]), k
    for suffix, feat, pred, y in (("", s["features_gen"], s["pred_gen"], yg), ("_real", s["features_real"], s["pred_real"], yr)):
        div, mm = metrics.cls_pair_tables(y.numpy(), K, 9, 3, 4)
        d = cls_scores_def([feat.cpu().numpy()], [pred.cpu().numpy()], y.numpy(), div, mm, K)
        for name, q in (("diversity", 1), ("multimodality", 2)):
            got = s[name + suffix]
            assert got.dtype == torch.float64 and got.is_cuda and abs(float(got) - d["scores64"][0, q]) <= 1e-13 * d["scores64"][0, q]
        if not suffix:
            assert s["correct_per_class"].cpu().numpy().tolist() == d["correct_per_class"][0].tolist()
            assert s["count_per_class"].cpu().numpy().tolist() == d["count_per_class"].tolist() == [5] * K
            assert s["correct"] == int(d["correct"][0])
        else:
            assert s["correct_real"] == int(d["correct"][0])
    with pytest.raises(ValueError, match="both"):
        metrics.classifier_scores(trained, xg, yg, xr, yr, batch=CB, diversity_pairs=9)
