"""The kinematic columns inside the Evaluator on the MI355X: "<g>/bone_cv" .. "<g>/still" against their
composition (a twin Sampler round + metrics.kinematics), the untouched other columns, round sharing, replay against eager,
the call counts, all 40 columns through kg_eval_record3 with selection by jerk, the rejections, resume, the training loop
and the command.  Every comparison is on bits.

The toy set-up of tests/test_eval_classifier_gpu.py: four classes, C 2, T 32, V 16 (h36m), P = 3 samples per class, two
generators, pairs 2, ring_len 8, three evaluations.  still_eps is 0.05 here (tests/test_kin_gpu.py: a good share of the
steps is still), so that the option travels and the sixth column does not compare two sets without a still step."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import evaluate, metrics
from kinetic_gan_amd.discriminator import Discriminator
from kinetic_gan_amd.evaluate import Evaluator, write_metrics_csv
from kinetic_gan_amd.generator import Generator
from kinetic_gan_amd.train import TrainLoop

import cls_def
import train_def
from test_eval_classifier_gpu import (C, CLS_KW, DEV, K, LATENT, MLP, P, T, V, assert_same, ev_state, flat_generator,  # noqa: F401
                                      loop_feeder, make_ev, real_set, same_bits, trained, twin_round)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.05
KIN_KW = dict(kinematics_per_class=P, kinematics_dataset="h36m", kinematics_still_eps=EPS)
NEW = ["%s/%s" % (g, q) for g in ("a", "b") for q in metrics.KIN_NAMES]
# own: no other round has P samples per class - Samplers of its own; shared: the PRDC round is read in place
KINDS = {"own": dict(), "shared": dict(prdc_per_class=P, prdc_k=2)}
IT0 = 2 ** 24 + 3


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def kin_state(ev):
    out = ev_state(ev)
    for k, s in ev.kin_samplers.items():
        out["kin_step." + k] = s.step_dev.detach().cpu().clone()
    return out


def real_selected():
    """the first P real samples of every class, class by class, and their labels"""
    x, y = real_set()
    rows = evaluate.class_rows(y, K, P)
    return x[rows].to(DEV), np.repeat(np.arange(K), P)


@pytest.fixture(scope="module")
def composed():
    Ga, Gb = flat_generator(1), flat_generator(2)
    it = torch.full((1,), IT0, dtype=torch.int64, device=DEV)
    evs = {}
    for kind, kw in KINDS.items():
        evs[kind] = make_ev({"a": Ga, "b": Gb}, it, **KIN_KW, **kw)
        evs[kind + "/plain"] = make_ev({"a": Ga, "b": Gb}, it, **kw)
    assert all(e.use_graph for e in evs.values())
    states = {k: [] for k in evs}
    for k in range(3):
        for name, e in evs.items():
            e.evaluate()
            states[name].append(kin_state(e))
        it += 2
    return dict(Ga=Ga, Gb=Gb, evs=evs, states=states, recs={k: e.records() for k, e in evs.items()})


@pytest.mark.parametrize("kind", list(KINDS))
def test_columns_equal_the_composition(composed, kind):
    ev, rec, plain = composed["evs"][kind], composed["recs"][kind], composed["recs"][kind + "/plain"]
    n_old = len(plain["names"])
    assert rec["names"] == plain["names"] + NEW and rec["scores"].shape == (3, n_old + 12)
    # every other column is that of an Evaluator without the option, and so is what they decide
    assert same_bits(rec["scores"][:, :n_old], plain["scores"])
    assert same_bits(rec["improved"], plain["improved"]) and same_bits(rec["iteration"], plain["iteration"])
    assert rec["iteration"].tolist() == [IT0, IT0 + 2, IT0 + 4]
    last, last_plain = composed["states"][kind][-1], composed["states"][kind + "/plain"][-1]
    for key in last_plain:
        if key != "ring_val":
            assert same_bits(last[key], last_plain[key]), key
    real, lab_real = real_selected()
    for k in range(3):
        for g, G in enumerate((composed["Ga"], composed["Gb"])):
            out, s = twin_round(G, k, P)
            want = metrics.kinematics(out, real, s.labels_np, lab_real, dataset="h36m", still_eps=EPS)
            assert want["scores"].dtype == torch.float32 and want["scores"].shape == (6,)
            assert same_bits(rec["scores"][k, n_old + 6 * g:n_old + 6 * g + 6], want["scores"]), (kind, k, g)
            assert int(want["nonfinite"].sum()) == 0 and int(want["degenerate"].sum()) == 0
    new = rec["scores"][:, n_old:]
    print(kind, "kinematic columns", dict(zip(NEW, new[0].tolist())))
    assert np.isfinite(new).all() and (new > 0).all()
    assert not np.array_equal(new[:, :6], new[:, 6:])                  # the columns of a differ from those of b
    state = ev.state_dict()
    assert state["kinematics"]["per_class"] == P and state["kinematics"]["still_eps"] == EPS
    assert state["kinematics"]["bones"] == [list(b) for b in ev.kinematics_bones] and len(state["kinematics"]["bones"]) == V - 1
    assert state["kinematics"]["mirror"] == [list(p) for p in ev.kinematics_mirror] and state["names"] == plain["names"] + NEW
    assert "kinematics" not in composed["evs"][kind + "/plain"].state_dict()
    # the real side, once: the means of the descriptors metrics.kinematics computes for it
    ref = metrics.kinematics(real, real, lab_real, lab_real, dataset="h36m", still_eps=EPS, per_sample=True)
    kr = ev.kinematics_real
    assert same_bits(ev._kin_real_desc, ref["desc_real"]) and set(kr) == set(metrics.KIN_NAMES) | {"class_means", "degenerate", "nonfinite"}
    assert kr["class_means"].shape == (K, 6) and kr["degenerate"].tolist() == [0] * K and kr["nonfinite"].tolist() == [0] * K
    for i, q in enumerate(metrics.KIN_NAMES):
        assert float(kr[q]) == float(ref["desc_real"].double().mean(dim=1)[:, i].mean())
    assert composed["evs"][kind + "/plain"].kinematics_real is None


def test_round_sharing(composed):
    own, shared = composed["evs"]["own"], composed["evs"]["shared"]
    assert list(own.kin_samplers) == ["a", "b"] and own.round_owner["kinematics"] is None and len(own._all_samplers()) == 4
    assert all(s.step_count == 3 for s in own._all_samplers())
    assert [int(s.step_dev.item()) for s in own._all_samplers()] == [3] * 4                 # the counters advance in lock-step
    assert shared.kin_samplers == {} and shared.round_owner["kinematics"] == "prdc" and len(shared._all_samplers()) == 4
    assert len(composed["evs"]["shared/plain"]._all_samplers()) == 4                         # no Sampler was added
    # the same rounds either way (one seed, one counter): the same kinematic columns
    a, b = composed["recs"]["own"], composed["recs"]["shared"]
    assert same_bits(a["scores"][:, -12:], b["scores"][:, -12:])


@pytest.mark.parametrize("kind", list(KINDS))
def test_replays_equal_eager_evaluations(composed, kind):
    it = torch.full((1,), IT0, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, it, use_graph=False, **KIN_KW, **KINDS[kind])
    for k in range(3):
        ev.evaluate()
        it += 2
        assert_same(composed["states"][kind][k], kin_state(ev), "graph vs eager, evaluation %d" % k)
    a, b = ev.records(), composed["recs"][kind]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))


@pytest.mark.parametrize("gens", [("a",), ("a", "b")])
def test_three_new_launches_whatever_the_number_of_generators(composed, monkeypatch, gens):
    """ONE kg_kin_desc_sets and ONE kg_kin_scores (two launches) per evaluation; kg_kin_desc runs once, at construction"""
    calls = {"kin_desc_sets": [], "kin_scores": [], "kin_desc": []}
    plain = {k: getattr(nv, k) for k in calls}
    monkeypatch.setattr(nv, "kin_desc_sets", lambda xs, *a, **kw: (calls["kin_desc_sets"].append(len(list(xs))),
                                                                   plain["kin_desc_sets"](xs, *a, **kw))[1])
    monkeypatch.setattr(nv, "kin_scores", lambda real, fakes, *a, **kw: (calls["kin_scores"].append(len(list(fakes))),
                                                                         plain["kin_scores"](real, fakes, *a, **kw))[1])
    monkeypatch.setattr(nv, "kin_desc", lambda *a, **kw: (calls["kin_desc"].append(1), plain["kin_desc"](*a, **kw))[1])
    G = {"a": composed["Ga"], "b": composed["Gb"]}
    ev = make_ev({g: G[g] for g in gens}, use_graph=False, **KIN_KW)
    assert calls == {"kin_desc_sets": [], "kin_scores": [], "kin_desc": [1]}                 # the real side, once
    counted = {}
    nv.flop_count = counted
    try:
        for _ in range(2):
            for v in calls.values():
                del v[:]
            ev.evaluate()
            torch.cuda.synchronize()
            assert calls == {"kin_desc_sets": [len(gens)], "kin_scores": [len(gens)], "kin_desc": []}, calls
    finally:
        nv.flop_count = None
    assert "kg_kin_desc_sets" in counted and "kg_kin_scores" in counted and "kg_kin_desc" not in counted


def test_groups_of_one_set_leave_the_same_bits(composed, monkeypatch):
    monkeypatch.setattr(nv, "KIN_MAX_SETS", 1)
    it = torch.full((1,), IT0, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, it, **KIN_KW)
    assert ev._kin_desc.shape[0] == 1
    for k in range(3):
        ev.evaluate()
        it += 2
    a, b = ev.records(), composed["recs"]["own"]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))


def test_everything_on_is_40_columns_through_record3(trained, composed, monkeypatch):
    """live + ema with every option: 40 names, kg_eval_record3, select = "b/jerk" (smaller is better)"""
    used = []
    plain3 = nv.eval_record3
    monkeypatch.setattr(nv, "eval_record3", lambda scores, *a, **kw: (used.append(len(scores)), plain3(scores, *a, **kw))[1])
    monkeypatch.setattr(nv, "eval_record2", lambda *a, **kw: pytest.fail("kg_eval_record2 with the kinematic columns on"))
    train, lab = cls_def.synthetic_set(50, n_classes=K, per_class=8)
    G = flat_generator(3)
    flat = G._flat_keep.flat
    orig = flat.clone()
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": G}, it, select="b/jerk", prdc_per_class=P, prdc_k=2, frechet_per_class=P,
                 classifier=trained, **CLS_KW, memorisation="raw", memorisation_per_class=P, memorisation_train=train.to(DEV),
                 memorisation_train_labels=lab.numpy(), **KIN_KW)
    want = evaluate.score_names(("a", "b"), ("avg", "joint"), True, ("pose", "motion"), True, True, kinematics=True)
    assert ev.names == want and len(ev.names) == 40 and ev.names[-12:] == NEW and not ev.maximise
    assert ev.kin_samplers == {} and ev.round_owner["kinematics"] == "prdc" and len(ev._all_samplers()) == 4
    assert ev.best() == {"value": float("inf"), "iteration": -1}
    col = ev.names.index("b/jerk")
    scales, weights = [1.0, 4.0, float("nan"), 0.25, 1.0, 16.0], []
    for k, s in enumerate(scales):
        with torch.no_grad():
            flat.copy_(orig * s)
        weights.append(flat.detach().clone())
        it.fill_(10 * (k + 1))
        ev.evaluate()
    rec, best = ev.records(), ev.best()
    assert used and set(used) == {40} and rec["scores"].shape == (6, 40)
    v = rec["scores"][:, col]
    print("b/jerk per evaluation:", v.tolist(), "improved:", rec["improved"].tolist(), "best:", best)
    run = float("inf")
    for k, x in enumerate(v.tolist()):
        better = x < run                         # (False for a NaN: it never wins)
        assert bool(rec["improved"][k]) == better, k
        run = x if better else run
    assert rec["improved"][0] and np.isnan(v[2]) and np.isnan(rec["scores"][2, -6:]).any() and not rec["improved"][2]
    assert np.isfinite(rec["scores"][:, 28:34]).all()                  # generator "a" is untouched by b's NaN weights
    first = int(np.flatnonzero(v == np.nanmin(v))[0])
    assert best == {"value": float(np.nanmin(v)), "iteration": 10 * (first + 1)}
    assert same_bits(ev.snap_flat, weights[first])
    E = ev.best_generator()
    assert same_bits(torch.cat([p.detach().reshape(-1) for p in E.parameters()]), weights[first])


# prdc 3, frechet 3, classifier 4, kinematics 4, raw memorisation at 4 (a count others have) or 5 (a count nobody else has)
MIXED = dict(prdc_per_class=3, prdc_k=2, frechet_per_class=3, classifier_per_class=4, classifier_batch=8, diversity_pairs=7,
             multimodality_pairs=2, memorisation="raw", kinematics_per_class=4, kinematics_dataset="h36m", kinematics_still_eps=EPS)
ALONE = {"prdc": ("prdc_per_class", "prdc_k"), "frechet": ("frechet_per_class",),
         "classifier": ("classifier_per_class", "classifier_batch", "diversity_pairs", "multimodality_pairs"),
         "memorisation": ("memorisation", "memorisation_per_class"),
         "kinematics": ("kinematics_per_class", "kinematics_dataset", "kinematics_still_eps")}


@pytest.fixture(scope="module")
def alone(trained, composed):
    """{(family, count): the family's columns of an Evaluator with that family alone, three evaluations}: computed once"""
    train, lab = cls_def.synthetic_set(50, n_classes=K, per_class=8)
    train, lab, cache = train.to(DEV), lab.numpy(), {}

    def columns(family, kw):
        key = (family, kw[family + "_per_class"])
        if key not in cache:
            extra = {"classifier": dict(classifier=trained),
                     "memorisation": dict(memorisation_train=train, memorisation_train_labels=lab)}.get(family, {})
            it = torch.full((1,), IT0, dtype=torch.int64, device=DEV)
            ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, it, **{k: kw[k] for k in ALONE[family]}, **extra)
            assert list(ev.round_owner.values()) == [None] * 5 and len(ev._all_samplers()) == 4
            for _ in range(3):
                ev.evaluate()
                it += 2
            cache[key] = ev.records()["scores"][:, 4:]
        return cache[key]
    return dict(train=train, lab=lab, columns=columns)


@pytest.mark.parametrize("mem", [4, 5])
def test_every_family_on_with_mixed_counts(trained, composed, alone, mem):
    """one table, one round pool, one real side per count: who owns which round, how many Samplers there are, which real-side
    tensors are one, and every family's columns those of an Evaluator with that family alone (Samplers of one seed and count
    draw the same rounds)"""
    kw = dict(MIXED, memorisation_per_class=mem)
    it = torch.full((1,), IT0, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, it, classifier=trained, memorisation_train=alone["train"],
                 memorisation_train_labels=alone["lab"], **kw)
    owners = {"prdc": None, "frechet": "prdc", "classifier": None, "memorisation": "classifier" if mem == 4 else None,
              "kinematics": "classifier"}
    assert ev.round_owner == owners and list(ev.round_owner) == ["prdc", "frechet", "classifier", "memorisation", "kinematics"]
    n_owners = sum(o is None for o in owners.values())
    assert n_owners == (2 if mem == 4 else 3) and len(ev._all_samplers()) == 2 * (1 + n_owners)
    assert len({id(s) for s in ev._all_samplers()}) == len(ev._all_samplers())
    groups = dict(prdc=ev.prdc_samplers, frechet=ev.frechet_samplers, classifier=ev.cls_samplers, memorisation=ev.mem_samplers,
                  kinematics=ev.kin_samplers)
    for key, group in groups.items():
        assert list(group) == (["a", "b"] if owners[key] is None else []), key
        assert all(s.n == K * kw[key + "_per_class"] for s in group.values()), key
    for _ in range(3):
        ev.evaluate()
        it += 2
    assert all(s.step_count == 3 for s in ev._all_samplers())
    assert [int(s.step_dev.item()) for s in ev._all_samplers()] == [3] * len(ev._all_samplers())      # in lock-step
    # the real side: one tensor per count, which the families' attributes alias
    sides = ev._real_sides
    assert sorted(sides) == sorted({3, 4, mem}) and len({t.data_ptr() for t in sides.values()}) == len(sides)
    assert ev.prdc_real.data_ptr() == ev.frechet_real.data_ptr() == sides[3].data_ptr() != sides[4].data_ptr()
    x, y = real_set()
    for per, t in sides.items():
        assert same_bits(t, x[evaluate.class_rows(y, K, per)])
    # every family's columns against that family alone
    rec = ev.records()
    assert rec["names"] == evaluate.score_names(("a", "b"), ("avg", "joint"), True, ("pose", "motion"), True, True, kinematics=True)
    assert rec["scores"].shape == (3, 40) and ev._record == "eval_record3"
    lo = 4
    for f in evaluate.FAMILIES:
        want = alone["columns"](f.key, kw)
        got = rec["scores"][:, lo:lo + want.shape[1]]
        assert want.shape[1] == 2 * len(f.columns(f.on(ev))) and same_bits(got, want), f.key
        lo += want.shape[1]
    assert lo == 40 and np.isfinite(rec["scores"]).all()


def test_rejections(composed):
    gens = {"a": composed["Ga"], "b": composed["Gb"]}
    with pytest.raises(ValueError, match="kinematics_dataset"):
        make_ev(gens, kinematics_per_class=P)                                                # no dataset and no bones
    with pytest.raises(ValueError, match=r"bones name a joint outside \[0, V=16\)"):
        make_ev(gens, kinematics_per_class=P, kinematics_dataset="ntu")                      # a 25-joint skeleton on 16 joints
    x, y = real_set()
    with pytest.raises(ValueError, match="T=3 frames"):
        Evaluator(gens, x[:, :, :3], real_labels=y, pairs=2, **KIN_KW)
    with pytest.raises(ValueError, match="kinematics_per_class=-1"):
        make_ev(gens, kinematics_per_class=-1, kinematics_dataset="h36m")
    with pytest.raises(ValueError, match="above the cap of %d" % nv.KIN_MAX_POINTS):
        make_ev(gens, kinematics_per_class=nv.KIN_MAX_POINTS // 2 + 1, kinematics_dataset="h36m")
    with pytest.raises(ValueError, match="still_eps"):
        make_ev(gens, kinematics_per_class=P, kinematics_dataset="h36m", kinematics_still_eps=-1.0)
    # the caller's own skeleton: two bones, no mirror pairs - the asymmetry column is 0 on both sides, so its W1 is 0
    ev = make_ev(gens, kinematics_per_class=P, kinematics_bones=[(0, 1), (1, 2)])
    ev.evaluate()
    rec = ev.records()
    assert (rec["scores"][0, [5, 11]] == 0).all() and np.isfinite(rec["scores"]).all()
    assert ev.state_dict()["kinematics"]["mirror"] == [] and ev.state_dict()["kinematics"]["bones"] == [[0, 1], [1, 2]]


def test_resume(composed):
    gens = {"a": composed["Ga"], "b": composed["Gb"]}
    it = torch.full((1,), IT0, dtype=torch.int64, device=DEV)
    first = make_ev(gens, it, **KIN_KW)
    for _ in range(2):
        first.evaluate()
        it += 2
    sd = first.state_dict()
    assert sd["count"] == 2 and "kinematics_real" not in sd and not any("real" in k for k in sd["kinematics"])
    second = make_ev(gens, it, **KIN_KW)
    second.load_state_dict(sd)
    second.evaluate()
    assert_same(composed["states"]["own"][2], kin_state(second), "2 + resume + 1")
    a, b = second.records(), composed["recs"]["own"]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))
    # another still_eps or per_class is refused before anything is loaded; a state without the key needs the option off
    for other in (make_ev(gens, it, **dict(KIN_KW, kinematics_still_eps=0.01)), make_ev(gens, it, **dict(KIN_KW, kinematics_per_class=2)),
                  make_ev(gens, it)):
        keep = kin_state(other)
        with pytest.raises(ValueError, match="kinematics"):
            other.load_state_dict(sd)
        assert_same(keep, kin_state(other), "a rejected state")
    old = composed["evs"]["own/plain"].state_dict()
    assert "kinematics" not in old
    with pytest.raises(ValueError, match="kinematics"):
        second.load_state_dict(old)
    off = make_ev(gens, it)
    off.load_state_dict(old)                      # a state from before the option loads with the option off
    assert off.n_evals == 3


# ---- the training loop and the command -----------------------------------------------------------------------------------

LOOP_NAMES = ["live/avg", "live/joint", "ema/avg", "ema/joint"] + ["%s/%s" % (g, q) for g in ("live", "ema") for q in metrics.KIN_NAMES]


def test_train_loop_writes_the_columns(tmp_path):
    torch.manual_seed(1)
    G = Generator(LATENT, C, K, T, MLP, dataset="h36m").to(DEV)
    torch.manual_seed(2)
    D = Discriminator(C, K, T, LATENT, dataset="h36m").to(DEV)
    loop = TrainLoop(G, D, loop_feeder(tmp_path / "set"), 4, T, n_critic=2, seed=3, eval_pairs=2, ema_decay=0.9, eval_interval=2,
                     eval_kinematics=P, eval_kinematics_still_eps=EPS, eval_select="ema/jerk")
    ev = loop.evaluator
    assert ev.names == LOOP_NAMES and not ev.maximise and ev.use_graph and ev._record == "eval_record3"
    assert ev.kinematics_per_class == P and ev.kinematics_still_eps == EPS and len(ev.kinematics_bones) == V - 1
    for _ in range(4):
        loop.step()
    rec = ev.records()
    assert rec["iteration"].tolist() == [2, 4] and rec["scores"].shape == (2, 16) and np.isfinite(rec["scores"]).all()
    write_metrics_csv(str(tmp_path / "metrics.csv"), rec)
    rows = list(csv.reader(open(tmp_path / "metrics.csv")))
    assert rows[0] == ["iteration"] + LOOP_NAMES + ["improved"] and len(rows) == 3
    back = np.array([[float(v) for v in r[1:17]] for r in rows[1:]], dtype=np.float32)
    assert same_bits(back, rec["scores"])
    assert loop.state_dict()["eval"]["kinematics"]["per_class"] == P


def test_train_command(tmp_path):
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 64, C, 40, V, K, "h36m", seed=4)
    out = str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--n_epochs", "1", "--batch_size", "8", "--dataset", "h36m",
           "--channels", str(C), "--v_size", str(V), "--t_size", str(T), "--n_classes", str(K), "--n_critic", "2",
           "--sample_interval", "100", "--checkpoint_interval", "100", "--log_interval", "4", "--seed", "1",
           "--data_path", dp, "--label_path", lp, "--eval_interval", "4", "--eval_pairs", "2", "--out", out,
           "--eval_kinematics", "3", "--eval_select", "live/jerk"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "[best live/jerk: " in r.stdout
    names = ["live/avg", "live/joint"] + ["live/" + q for q in metrics.KIN_NAMES]
    rows = list(csv.reader(open(os.path.join(out, "metrics.csv"))))
    assert rows[0] == ["iteration"] + names + ["improved"] and len(rows) == 3           # 8 iterations: two intervals
    state = torch.load(os.path.join(out, "loop_state.pth"), weights_only=False)["eval"]
    assert state["select"] == "live/jerk" and state["names"] == names and state["kinematics"]["still_eps"] == 1e-3
    back = np.array([[float(v) for v in r_[1:9]] for r_ in rows[1:]], dtype=np.float32)
    assert same_bits(back, state["records"]["scores"]) and np.isfinite(back).all()
    assert os.path.exists(os.path.join(out, "models", "generator_best.pth"))
