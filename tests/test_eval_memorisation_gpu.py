"""The memorisation columns inside the Evaluator on the MI355X: "<g>/authenticity" and "<g>/label_agreement"
against their composition (a twin Sampler round + metrics.memorisation / memorisation_features), the untouched other columns,
replay against eager, the call counts, the untouched classifier and training set, selection by label agreement, the refusal
of authenticity, resume, the training loop and the command.

The toy set-up of tests/test_eval_classifier_gpu.py: four classes, P = 3 samples per class, two generators, classifier_batch 8.
The training set is cls_def.synthetic_set plus PLANTED rows of generator "a"'s first round (which a twin Sampler reproduces):
  rows 0 .. 3  copies (raw space: + 1e-4 N(0, 1), as nn_def.planted; feature space: exact) - closer to their sources than to
               any other training sample: NOT authentic.  The copies of rows 2 and 3 carry each other's label: their sources'
               nearest training sample disagrees with the conditioning label, rows 0 and 1 agree.
  row 5        its copy stands TWICE in the training set: the two are each other's nearest training sample at distance 0, so
               row 5, whose nearest neighbour is one of them, is authentic by the >= of the definition (d2 >= 0).
So at evaluation 0 both tallies of "a" lie strictly between 0 and n = 12, whatever the untrained generators produce."""
import csv
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import metrics
from kinetic_gan_amd.discriminator import Discriminator
from kinetic_gan_amd.evaluate import Evaluator, write_metrics_csv
from kinetic_gan_amd.generator import Generator
from kinetic_gan_amd.train import TrainLoop

import cls_def
import train_def
from test_eval_classifier_gpu import (C, CB, CLS_KW, DEV, K, LATENT, MLP, P, SD, SEED_EV, SL, T, V, assert_same, ev_state,  # noqa: F401
                                      flat_generator, loop_feeder, make_ev, same_bits, trained, twin_round)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROUND = K * P
NEW = ["%s/%s" % (g, q) for g in ("a", "b") for q in metrics.MEMORISATION_NAMES]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def mem_state(ev):
    out = ev_state(ev)
    for k, s in ev.mem_samplers.items():
        out["mem_step." + k] = s.step_dev.detach().cpu().clone()
    return out


def training_set(Ga, space):
    """(train (N, C, T, V) fp32 on the device, labels (N,) numpy): the synthetic set and the planted rows of the docstring"""
    x, y = cls_def.synthetic_set(50, n_classes=K, per_class=8)
    out, s = twin_round(Ga, 0, P)
    rows = out.detach().cpu().contiguous()
    lab = np.asarray(s.labels_np)
    pick = [0, 1, 2, 3, 5, 5]
    planted = rows[pick].clone()
    if space == "raw":
        noise = 1e-4 * np.random.RandomState(9).randn(5, C, T, V)
        planted += torch.as_tensor(noise[[0, 1, 2, 3, 4, 4]], dtype=torch.float32)      # (row 5: the SAME noisy copy twice)
    lab_planted = lab[[0, 1, 3, 2, 5, 5]]
    train = torch.cat([x, planted]).to(DEV)
    return train, np.concatenate([y.numpy(), lab_planted])


def kind_kw(kind, clf, train, lab):
    mem = dict(memorisation_train=train, memorisation_train_labels=lab)
    if kind == "features":
        return dict(classifier=clf, **CLS_KW), dict(memorisation="features", **mem)
    return dict(prdc_per_class=P, prdc_k=2), dict(memorisation="raw", memorisation_per_class=P, **mem)      # the PRDC round is read


@pytest.fixture(scope="module")
def composed(trained):
    Ga, Gb = flat_generator(1), flat_generator(2)
    before = [p.detach().clone() for p in trained.parameters()]
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    evs, sets = {}, {}
    for kind in ("features", "raw"):
        train, lab = training_set(Ga, kind)
        sets[kind] = (train, lab, train.clone())
        base, mem = kind_kw(kind, trained, train, lab)
        evs[kind] = make_ev({"a": Ga, "b": Gb}, it, **base, **mem)
        evs[kind + "/plain"] = make_ev({"a": Ga, "b": Gb}, it, **base)
    assert all(e.use_graph for e in evs.values())
    states = {k: [] for k in evs}
    for k in range(3):
        for name, e in evs.items():
            e.evaluate()
            states[name].append(mem_state(e))
        it += 2
    return dict(Ga=Ga, Gb=Gb, clf=trained, before=before, mode=trained.training, evs=evs, sets=sets, states=states,
                recs={k: e.records() for k, e in evs.items()})


def features_of(ev, x):
    feat = torch.zeros((x.shape[0], int(ev.classifier.feat_dim)), dtype=torch.float32, device=DEV)
    pred = torch.zeros(x.shape[0], dtype=torch.int32, device=DEV)
    ev._classifier_features(x, feat, pred)
    return feat


@pytest.mark.parametrize("kind", ["features", "raw"])
def test_columns_equal_the_composition(composed, kind):
    ev, rec, plain = composed["evs"][kind], composed["recs"][kind], composed["recs"][kind + "/plain"]
    train, lab, _ = composed["sets"][kind]
    n_old = len(plain["names"])
    assert rec["names"] == plain["names"] + NEW and rec["scores"].shape == (3, n_old + 4)
    # every other column is that of an Evaluator without the option, and so is what they decide
    assert same_bits(rec["scores"][:, :n_old], plain["scores"])
    assert same_bits(rec["improved"], plain["improved"]) and same_bits(rec["iteration"], plain["iteration"])
    last, last_plain = composed["states"][kind][-1], composed["states"][kind + "/plain"][-1]
    for key in last_plain:
        if key != "ring_val":
            assert same_bits(last[key], last_plain[key]), key
    # no Sampler of its own: the classifier round's features / the PRDC round are read in place
    assert ev.mem_samplers == {} and len(ev._all_samplers()) == 4 and all(s.step_count == 3 for s in ev._all_samplers())
    loo = None
    tallies = []
    for k in range(3):
        for g, G in enumerate((composed["Ga"], composed["Gb"])):
            out, s = twin_round(G, k, P)
            if kind == "features":
                if loo is None:
                    train_feat = features_of(ev, train)
                    assert same_bits(train_feat, ev.memorisation_train_features)
                want = metrics.memorisation_features(features_of(ev, out), s.labels_np, train_feat, lab, train_loo=loo)
            else:
                want = metrics.memorisation(out, s.labels_np, train, lab, train_loo=loo)
            loo = want["train_loo_d2"]
            cols = [np.float32(want["authenticity"].item()).reshape(1), np.float32(want["label_agreement"].item()).reshape(1)]
            counts = want["counts"].tolist()
            print(kind, "evaluation", k, "generator", "ab"[g], "counts", counts, "of", N_ROUND)
            tallies.append(counts)
            for i, col in enumerate(cols):
                assert same_bits(rec["scores"][k, n_old + 2 * g + i:n_old + 2 * g + i + 1], col), (k, g, metrics.MEMORISATION_NAMES[i])
            if k == 0 and g == 0:
                # the planted rows: copies are found and are not authentic; the duplicated copy makes row 5 authentic at d2 >= 0
                n_syn = train.shape[0] - 6
                assert want["nn_index"][:4].tolist() == [n_syn, n_syn + 1, n_syn + 2, n_syn + 3] or kind == "features"
                assert not want["authentic"][:4].any() and want["authentic"][5]
                assert loo[n_syn + 4] == 0 and loo[n_syn + 5] == 0
    assert same_bits(ev._mem_loo, loo)
    # not vacuous: both tallies of generator "a" at evaluation 0 lie strictly between 0 and n
    assert 0 < tallies[0][0] < N_ROUND and 0 < tallies[0][1] < N_ROUND, tallies
    new = rec["scores"][:, n_old:]
    assert np.isfinite(new).all() and (new >= 0).all() and (new <= 1).all()
    state = ev.state_dict()
    assert state["memorisation"] == {"mode": kind, "per_class": P} and state["names"] == plain["names"] + NEW
    assert "memorisation" not in composed["evs"][kind + "/plain"].state_dict()
    # the real side's reference: the selected real samples as queries against the same training set
    real = ev.memorisation_real
    assert 0 <= float(real["authenticity"]) <= 1 and 0 <= float(real["label_agreement"]) <= 1
    assert real["counts"].dtype == torch.int64 and real["counts"].shape == (2,)


@pytest.mark.parametrize("kind", ["features", "raw"])
def test_replays_equal_eager_evaluations(composed, kind):
    train, lab, _ = composed["sets"][kind]
    base, mem = kind_kw(kind, composed["clf"], train, lab)
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, it, use_graph=False, **base, **mem)
    for k in range(3):
        ev.evaluate()
        it += 2
        assert_same(composed["states"][kind][k], mem_state(ev), "graph vs eager, evaluation %d" % k)
    a, b = ev.records(), composed["recs"][kind]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))


@pytest.mark.parametrize("kind", ["features", "raw"])
@pytest.mark.parametrize("gens", [("a",), ("a", "b")])
def test_three_new_launches_whatever_the_number_of_generators(composed, monkeypatch, kind, gens):
    """ONE kg_nn_sets (search + merge) and ONE kg_nn_scores per evaluation; the leave-one-out pass and the real side's scores
    run once, at construction"""
    calls = {"nn_sets": [], "nn_scores": [], "nn": []}
    plain = {k: getattr(nv, k) for k in calls}
    monkeypatch.setattr(nv, "nn_sets", lambda qs, *a, **kw: (calls["nn_sets"].append(len(list(qs))), plain["nn_sets"](qs, *a, **kw))[1])
    monkeypatch.setattr(nv, "nn_scores", lambda idx, *a, **kw: (calls["nn_scores"].append(idx.shape[0]), plain["nn_scores"](idx, *a, **kw))[1])
    monkeypatch.setattr(nv, "nn", lambda *a, **kw: (calls["nn"].append(1), plain["nn"](*a, **kw))[1])
    train, lab, _ = composed["sets"][kind]
    base, mem = kind_kw(kind, composed["clf"], train, lab)
    G = {"a": composed["Ga"], "b": composed["Gb"]}
    ev = make_ev({g: G[g] for g in gens}, use_graph=False, **base, **mem)
    assert calls == {"nn_sets": [1], "nn_scores": [1], "nn": [1]}          # the real side and the leave-one-out pass, once
    counted = {}
    nv.flop_count = counted
    try:
        for _ in range(2):
            for v in calls.values():
                del v[:]
            ev.evaluate()
            torch.cuda.synchronize()
            assert calls == {"nn_sets": [len(gens)], "nn_scores": [len(gens)], "nn": []}, calls
    finally:
        nv.flop_count = None
    assert "kg_nn_sets" in counted and "kg_nn_scores" in counted and "kg_nn" not in counted


def test_classifier_and_training_set_untouched(composed):
    clf = composed["clf"]
    assert clf.training == composed["mode"]
    for p, q in zip(clf.parameters(), composed["before"]):
        assert same_bits(p, q)
    for kind, (train, _, copy) in composed["sets"].items():
        assert same_bits(train, copy), kind


def test_raw_space_with_samplers_of_its_own_and_a_resident_dataset(composed):
    """memorisation_per_class = 2 matches no other round: two more Samplers; the training set as a ResidentDataset - the
    unnormalised array searched in place through (scale, shift) - gives the columns of the normalised tensor"""
    train, lab, _ = composed["sets"]["raw"]
    scale, shift = 0.4, -0.3
    raw = (train - shift) / scale
    norm = raw.clone().mul_(scale).add_(shift)
    ds = types.SimpleNamespace(fits=True, data=raw, labels=torch.as_tensor(lab).to(DEV), scale=scale, shift=shift)
    gens = {"a": composed["Ga"], "b": composed["Gb"]}
    kw = dict(memorisation="raw", memorisation_per_class=2)
    ev = make_ev(gens, memorisation_train=ds, **kw)
    ev2 = make_ev(gens, memorisation_train=norm, memorisation_train_labels=lab, **kw)
    assert ev._mem_bv.t.data_ptr() == raw.data_ptr() and ev._mem_ba == (scale, shift)          # in place
    assert len(ev.mem_samplers) == 2 and len(ev._all_samplers()) == 4
    for _ in range(2):
        ev.evaluate()
        ev2.evaluate()
    a, b = ev.records(), ev2.records()
    assert a["names"] == ["a/avg", "a/joint", "b/avg", "b/joint"] + NEW and same_bits(a["scores"], b["scores"])
    assert same_bits(ev._mem_loo, ev2._mem_loo)
    out, s = twin_round(composed["Ga"], 1, 2)
    want = metrics.memorisation(out, s.labels_np, ds)
    assert same_bits(a["scores"][1, 4:5], np.float32(want["authenticity"].item()).reshape(1))
    assert same_bits(a["scores"][1, 5:6], np.float32(want["label_agreement"].item()).reshape(1))
    assert all(s.step_count == 2 for s in ev._all_samplers())


def test_selection_by_label_agreement(composed):
    """select="b/label_agreement" (larger is better): the snapshot is taken on a strict improvement only"""
    train, lab, _ = composed["sets"]["raw"]
    G = flat_generator(3)
    flat = G._flat_keep.flat
    orig = flat.clone()
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": G}, it, select="b/label_agreement", memorisation="raw", memorisation_per_class=P,
                 memorisation_train=train, memorisation_train_labels=lab)
    assert ev.maximise and ev.best() == {"value": float("-inf"), "iteration": -1}
    col = ev.names.index("b/label_agreement")
    scales, weights = [1.0, 4.0, float("nan"), 0.25, 1.0, 16.0], []
    for k, s in enumerate(scales):
        with torch.no_grad():
            flat.copy_(orig * s)
        weights.append(flat.detach().clone())
        it.fill_(10 * (k + 1))
        ev.evaluate()
    rec, best = ev.records(), ev.best()
    v = rec["scores"][:, col]
    print("b/label_agreement per evaluation:", v.tolist(), "improved:", rec["improved"].tolist(), "best:", best)
    run = float("-inf")
    for k, x in enumerate(v.tolist()):
        better = x > run
        assert bool(rec["improved"][k]) == better, k
        run = x if better else run
    assert rec["improved"][0]
    first = int(np.flatnonzero(v == np.nanmax(v))[0])
    assert best == {"value": float(np.nanmax(v)), "iteration": 10 * (first + 1)}
    assert same_bits(ev.snap_flat, weights[first])


def test_rejections_and_resume(composed):
    gens = {"a": composed["Ga"], "b": composed["Gb"]}
    clf = composed["clf"]
    train, lab, _ = composed["sets"]["raw"]
    mem = dict(memorisation_train=train, memorisation_train_labels=lab)
    for name in ("a/authenticity", "b/authenticity"):
        with pytest.raises(ValueError, match="closer"):
            make_ev(gens, select=name, memorisation="raw", memorisation_per_class=P, **mem)
    with pytest.raises(ValueError, match="none of"):
        make_ev(gens, memorisation="pixels", **mem)
    with pytest.raises(ValueError, match="needs the training set"):
        make_ev(gens, memorisation="raw", memorisation_per_class=P)
    with pytest.raises(ValueError, match="classifier= and classifier_per_class"):
        make_ev(gens, memorisation="features", **mem)
    with pytest.raises(ValueError, match="memorisation_per_class=2 is for memorisation='raw'"):
        make_ev(gens, classifier=clf, **CLS_KW, memorisation="features", memorisation_per_class=2, **mem)
    with pytest.raises(ValueError, match="memorisation_per_class >= 1"):
        make_ev(gens, memorisation="raw", **mem)
    with pytest.raises(ValueError, match="memorisation_train_labels is needed"):
        make_ev(gens, memorisation="raw", memorisation_per_class=P, memorisation_train=train)
    with pytest.raises(ValueError, match=r"channels, frames, joints"):
        make_ev(gens, memorisation="raw", memorisation_per_class=P, memorisation_train=train[:, :, :T // 2], memorisation_train_labels=lab)
    with pytest.raises(ValueError, match="scores, at most"):
        Evaluator({"g%d" % i: composed["Ga"] for i in range(3)}, *_real(), pairs=2, prdc_per_class=P, prdc_k=2, frechet_per_class=P,
                  classifier=clf, **CLS_KW, memorisation="raw", memorisation_per_class=P, **mem)     # 3 x (2 + 4 + 2 + 4 + 2) = 42 > 32
    # state_dict -> load_state_dict continues bit for bit
    base, memkw = kind_kw("raw", clf, train, lab)
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    first = make_ev(gens, it, **base, **memkw)
    first.evaluate()
    it += 2
    sd = first.state_dict()
    second = make_ev(gens, it, **base, **memkw)
    second.load_state_dict(sd)
    for k in (1, 2):
        second.evaluate()
        it += 2
        assert_same(composed["states"]["raw"][k], mem_state(second), "1 + resume + %d" % k)
    a, b = second.records(), composed["recs"]["raw"]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))
    # a state from a run without the option - or with the other space - is refused before anything is loaded, and vice versa
    plain = make_ev(gens, it, **base)
    keep = mem_state(plain)
    with pytest.raises(ValueError, match="memorisation"):
        plain.load_state_dict(sd)
    assert_same(keep, mem_state(plain), "a rejected state")
    with pytest.raises(ValueError, match="memorisation"):
        second.load_state_dict(composed["evs"]["raw/plain"].state_dict())
    with pytest.raises(ValueError, match="memorisation"):
        second.load_state_dict(dict(sd, memorisation={"mode": "features", "per_class": P}))


def _real():
    from test_eval_classifier_gpu import real_set
    return real_set()


# ---- the training loop and the command -----------------------------------------------------------------------------------

LOOP_NAMES = ["live/avg", "live/joint", "ema/avg", "ema/joint"] + ["%s/%s" % (g, q) for g in ("live", "ema") for q in metrics.CLS_NAMES] \
    + ["%s/%s" % (g, q) for g in ("live", "ema") for q in metrics.MEMORISATION_NAMES]


def test_train_loop_writes_the_columns(trained, tmp_path):
    """the loop's own ResidentDataset (normalised by the Feeder's constants) is the training side, where it lies"""
    torch.manual_seed(1)
    G = Generator(LATENT, C, K, T, MLP, dataset="h36m").to(DEV)
    torch.manual_seed(2)
    D = Discriminator(C, K, T, LATENT, dataset="h36m").to(DEV)
    loop = TrainLoop(G, D, loop_feeder(tmp_path / "set"), 4, T, n_critic=2, seed=3, eval_pairs=2, ema_decay=0.9, eval_interval=2,
                     eval_classifier=trained, eval_classifier_samples=P, eval_classifier_batch=CB, eval_diversity_pairs=SD,
                     eval_multimodality_pairs=SL, eval_memorisation="features", eval_select="ema/label_agreement")
    ev = loop.evaluator
    assert ev.names == LOOP_NAMES and ev.maximise and ev.memorisation == "features" and ev.use_graph
    assert ev._mem_train.data_ptr() == loop.resident.data.data_ptr() and ev._mem_N == 80
    for _ in range(4):
        loop.step()
    rec = ev.records()
    assert rec["iteration"].tolist() == [2, 4] and rec["scores"].shape == (2, 16) and np.isfinite(rec["scores"]).all()
    assert ((rec["scores"][:, 12:] >= 0) & (rec["scores"][:, 12:] <= 1)).all()
    write_metrics_csv(str(tmp_path / "metrics.csv"), rec)
    rows = list(csv.reader(open(tmp_path / "metrics.csv")))
    assert rows[0] == ["iteration"] + LOOP_NAMES + ["improved"] and len(rows) == 3
    assert loop.state_dict()["eval"]["memorisation"] == {"mode": "features", "per_class": P}
    # the composition of the live generator's last columns: the loop's training set through its affine, chunk by chunk
    r = loop.resident
    norm = r.data * r.scale + r.shift
    assert same_bits(features_of(ev, norm), ev.memorisation_train_features)


def test_train_command_refuses_a_streamed_dataset(tmp_path):
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 64, C, 40, V, K, "h36m", seed=4)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--n_epochs", "1", "--batch_size", "8", "--dataset", "h36m",
           "--channels", str(C), "--v_size", str(V), "--t_size", str(T), "--n_classes", str(K), "--n_critic", "2", "--seed", "1",
           "--data_path", dp, "--label_path", lp, "--eval_interval", "4", "--eval_pairs", "2", "--out", str(tmp_path / "run"),
           "--eval_memorisation", "raw", "--eval_memorisation_samples", str(P), "--max_resident_bytes", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--eval_memorisation raw" in r.stderr and "streamed" in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert "searches the training set on the device" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path / "run"), "metrics.csv"))
