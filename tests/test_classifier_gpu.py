"""The action classifier at model level on the MI355X, in the order a first visit runs them: block 0 of the
trunk without label channels, Classifier against the host oracle, ClassifierLoop (against the oracle's Adam loop, replay
against eager, resume, the gathered batches), learning on a toy set, metrics.classifier_scores."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import metrics
from kinetic_gan_amd.classifier import Classifier
from kinetic_gan_amd.classify import ClassifierLoop, evaluate
from kinetic_gan_amd.disc_trunk import BlockGeom, DiscTrunkFn, MaskedAdjacencyFn, TrunkMeta
from kinetic_gan_amd.discriminator import st_gcn
from kinetic_gan_amd.feeder import Feeder
from kinetic_gan_amd.graph import build_graph
from oracle import modules_ref as M
from oracle.fill import fill_module
from oracle.graph_tables import load_graph

import cls_def
import train_def
import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- 1. block 0 alone ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,C,T", [("h36m", 2, 32), ("ntu", 3, 64)])
def test_block0_without_label_channels(name, C, T):
    """st_gcn(C, 32, residual=False) through a trunk meta with const_channels = 0 (the gcn route with the plain spec_g, C_in = 2
    or 3) against the oracle's DiscBlock: forward <= 1e-4 max|b|, parameter gradients grad_close at 5e-3"""
    graph, ograph = build_graph(name), load_graph(name)
    As = [torch.tensor(a, dtype=torch.float32) for a in graph.As]
    ks = ([3 for _ in As], [a.size(0) for a in As])
    blk = st_gcn(C, 32, ks, 1, graph=graph, lvl=0, dw_s=True, dw_t=T, residual=False)
    ora = M.DiscBlock(C, 32, ks, 1, graph=ograph, lvl=0, dw_s=True, dw_t=T, residual=False)
    fill_module(blk, seed=3)
    fill_module(ora, seed=3)
    assert list(blk.state_dict()) == list(ora.state_dict())
    V = As[0].shape[1]
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, C, T, V, generator=g) * 2 - 1
    imp = torch.rand(As[0].shape, generator=g) + 0.5
    blk.to(DEV)
    geom = BlockGeom(blk, T, V, torch.device(DEV), const_channels=0)
    assert geom.cc == 0 and geom.res == "none" and geom.spec_g.Cin == C
    meta = TrunkMeta([geom], [As[0].to(DEV)], head=False, label_bias=False)
    imp_d = imp.to(DEV).requires_grad_()
    params = [blk.gcn.conv.weight, blk.tcn.weight, blk.tcn.bias]
    ak_all = MaskedAdjacencyFn.apply(meta, imp_d)
    (h,) = DiscTrunkFn.apply(meta, x.to(DEV), None, None, ak_all, *params)
    imp_o = imp.clone().requires_grad_()
    ho, _ = ora(x, As[0] * imp_o)
    r = torch.rand(ho.shape, generator=g) - 0.5
    (h * r.to(DEV)).sum().backward()
    (ho * r).sum().backward()
    torch.cuda.synchronize()
    print("block 0 forward", util.rel_err(h, ho))
    assert tuple(h.shape) == tuple(ho.shape) and util.rel_err(h, ho) <= 1e-4
    po = dict(ora.named_parameters())
    for k, p in blk.named_parameters():
        assert p.grad is not None and util.grad_close(p.grad, po[k].grad, 5e-3), (k, util.l2_rel(p.grad, po[k].grad))
    assert util.grad_close(imp_d.grad, imp_o.grad, 5e-3), util.l2_rel(imp_d.grad, imp_o.grad)


# ---- 2. Classifier against OracleClassifier -----------------------------------------------------------------------------

def _pair(name, C, L, T, seed=5, **kw):
    clf = Classifier(C, L, T, dataset=name, **kw)
    ora = cls_def.OracleClassifier(C, L, T, dataset=name, **kw)
    fill_module(clf, seed=seed)
    fill_module(ora, seed=seed)
    return clf.to(DEV), ora


@pytest.mark.parametrize("name,C,L,T,V,n", [("h36m", 2, 10, 32, 16, 4), ("ntu", 3, 60, 64, 25, 3)])
def test_classifier_against_oracle(name, C, L, T, V, n):
    clf, ora = _pair(name, C, L, T)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(n, C, T, V, generator=g) * 2 - 1
    y = torch.randint(0, L, (n,), generator=g)
    out = clf.classify(x.to(DEV), y.to(DEV))
    out["loss"].backward()
    with torch.no_grad():
        feat_ng = clf.features(x.to(DEV))
    lo = ora(x)
    loss_o = F.cross_entropy(lo, y)
    loss_o.backward()
    torch.cuda.synchronize()
    print("logits %.3e features %.3e loss %.3e" % (util.rel_err(out["logits"], lo), util.rel_err(out["features"], ora.features(x)),
                                                   util.rel_err(out["loss"], loss_o)))
    assert util.rel_err(out["logits"], lo) <= 1e-4
    assert util.rel_err(out["features"], ora.features(x)) <= 1e-4
    assert util.rel_err(out["loss"], loss_o) <= 1e-5
    assert np.array_equal(bits(feat_ng), bits(out["features"]))
    assert int(out["correct"]) == int((out["pred"].cpu().long() == y).sum())
    po = dict(ora.named_parameters())
    for k, p in clf.named_parameters():
        assert p.grad is not None and util.grad_close(p.grad, po[k].grad, 5e-3), (k, util.l2_rel(p.grad, po[k].grad))


# ---- 3. ClassifierLoop ---------------------------------------------------------------------------------------------------

def _fixture_feeder():
    return Feeder(os.path.join(GOLDEN, "feeder_h36m_data.npy"), os.path.join(GOLDEN, "feeder_h36m_label.pkl"), dataset="h36m")


def _loop(feeder, use_graph, seed_model=9, **kw):
    clf = Classifier(2, 4, 16, dataset="h36m")
    fill_module(clf, seed=seed_model)
    return ClassifierLoop(clf.to(DEV), feeder, 4, 16, seed=2, lr=1e-3, use_graph=use_graph, **kw)


def _state_bits(loop):
    f = loop.flat
    torch.cuda.synchronize()
    return [bits(t) for t in (f.flat, f.exp_avg, f.exp_avg_sq, f.step, loop.ring, loop.step_dev)]


def test_classifier_loop():
    feeder = _fixture_feeder()
    B, t, seed, lr = 4, 16, 2, 1e-3
    # (a) eager, against the host oracle's loop on the same batches
    eager = _loop(feeder, False)
    ora = cls_def.OracleClassifier(2, 4, 16, dataset="h36m")
    fill_module(ora, seed=9)
    opt = torch.optim.Adam(ora.parameters(), lr=lr, betas=(0.9, 0.999))
    gaps = []
    for s in range(6):
        eager.step()
        want_x, want_y = train_def.batch(feeder, B, t, seed, s)
        assert np.array_equal(bits(eager.real), want_x.view(np.uint32)), s          # the gather definition's rows
        assert np.array_equal(eager.labels.cpu().numpy(), want_y), s
        opt.zero_grad()
        lo = ora.loss(torch.as_tensor(want_x), torch.as_tensor(want_y))
        lo.backward()
        opt.step()
        loss = float(eager.losses()[0][-1])
        gaps.append(abs(loss - float(lo.detach())) / abs(float(lo.detach())))
    print("loss gaps to the oracle's Adam loop:", ["%.2e" % g for g in gaps])
    assert gaps[0] <= 1e-5 and gaps[5] <= 4e-3, gaps
    loss_e, acc_e = eager.losses()
    assert len(loss_e) == 6 and np.isfinite(loss_e).all() and ((acc_e >= 0) & (acc_e <= 1)).all()
    assert eager.step_count == 6 and int(eager.step_dev.item()) == 6
    want = _state_bits(eager)
    # (b) six replays: the same bits (parameters, moments, ring)
    replay = _loop(feeder, True)
    for _ in range(6):
        replay.step()
    for a, b in zip(_state_bits(replay), want):
        assert np.array_equal(a, b)
    # (b') a ring of four rows (it wraps, and is read in mid-run) and a host that waits at every iteration: the same record,
    # parameters and moments
    short = _loop(feeder, True, ring_len=4, run_ahead=2)
    assert short.ring_len == 4 and short.run_ahead == 2
    for _ in range(6):
        short.step()
    for a, b in zip(short.losses(), replay.losses()):
        assert len(a) == 6 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in zip(_state_bits(short)[:4], want[:4]):
        assert np.array_equal(a, b)
    assert np.array_equal(_state_bits(short)[5], want[5])
    # (c) resume: state after three iterations into a fresh loop, three more
    first = _loop(feeder, False)
    for _ in range(3):
        first.step()
    sd = first.state_dict()
    assert sd["step"] == 3 and set(sd) == {"step", "seed", "batch_size", "batches_per_epoch", "flat", "exp_avg", "exp_avg_sq",
                                           "adam_step", "last_losses"}
    second = _loop(feeder, True, seed_model=10)          # other initial weights: everything comes from the state
    second.load_state_dict(sd)
    for _ in range(3):
        second.step()
    got = _state_bits(second)
    for i, (a, b) in enumerate(zip(got, want)):
        if i == 4:          # the ring: a resumed run holds the last loss pair of the first half and its own rows
            assert np.array_equal(a[2:6], b[2:6])
        else:
            assert np.array_equal(a, b), i
    with pytest.raises(ValueError):
        _loop(feeder, False).load_state_dict(dict(sd, seed=3))


# ---- 4. it learns / 5. the scores -----------------------------------------------------------------------------------------

def _write_set(path, x, y):
    os.makedirs(path, exist_ok=True)
    dp, lp = os.path.join(path, "data.npy"), os.path.join(path, "label.pkl")
    np.save(dp, x.numpy())
    with open(lp, "wb") as f:
        pickle.dump((["s%d" % i for i in range(len(y))], [int(v) for v in y]), f)
    return Feeder(dp, lp, norm=False, dataset="h36m")


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Classifier(2, 4, 32, latent=64, feat_dim=16), torch's default initialisation under manual_seed(0), 100 replayed
    iterations of batch 16 on the toy set"""
    seed = 0
    x, y = cls_def.synthetic_set(10 + seed)
    feeder = _write_set(str(tmp_path_factory.mktemp("toy")), x, y)
    torch.manual_seed(seed)
    clf = Classifier(2, 4, 32, latent=64, feat_dim=16, dataset="h36m").to(DEV)
    loop = ClassifierLoop(clf, feeder, 16, 32, seed=seed, lr=1e-3, b1=0.9, b2=0.999, use_graph=True)
    for _ in range(100):
        loop.step()
    return clf, loop


def test_it_learns(trained):
    clf, loop = trained
    loss, acc = loop.losses()
    xv, yv = cls_def.synthetic_set(100 + 0)
    res = loop.evaluate(xv, yv)
    print("loss %.4f -> %.4f, batch accuracy %.2f -> %.2f, held-out accuracy %.3f" % (loss[0], loss[-1], acc[0], acc[-1],
                                                                                     res["accuracy"]))
    assert len(loss) == 100 and loss[-1] < loss[0]
    assert res["accuracy"] >= 0.9
    assert res["total"].tolist() == [8, 8, 8, 8] and res["correct"].sum() == round(res["accuracy"] * 32)
    assert evaluate(clf, xv, yv, batch=5)["correct"].tolist() == res["correct"].tolist()


def test_classifier_scores(trained):
    clf, _ = trained
    xg, yg = cls_def.synthetic_set(21, n_classes=3, per_class=12)
    xr, yr = cls_def.synthetic_set(22, n_classes=3, per_class=12)
    s = metrics.classifier_scores(clf, xg, yg, xr, yr, batch=16)
    with torch.no_grad():
        chunks = lambda x: torch.cat([clf.features(x[lo:lo + 16].to(DEV)) for lo in range(0, len(x), 16)], 0)      # noqa: E731
        fg, fr = chunks(xg), chunks(xr)
        logits = torch.cat([clf(xg[lo:lo + 16].to(DEV)) for lo in range(0, len(xg), 16)], 0).cpu().numpy()
    assert s["correct"] == int((cls_def.pred_rule(logits) == yg.numpy()).sum())
    assert s["accuracy"] == s["correct"] / 36.0 and 0.0 <= s["accuracy_real"] <= 1.0
    one = metrics.frechet_features(fg, fr)
    per = metrics.frechet_features(fg, fr, yg, yr, None)
    assert np.array_equal(s["feature_fd"].cpu().numpy(), one["mean"].cpu().numpy())
    assert np.array_equal(s["feature_fd_class_mean"].cpu().numpy(), per["mean"].cpu().numpy())
    assert np.array_equal(s["feature_fd_per_class"].cpu().numpy(), per["values"].cpu().numpy())
    assert np.isfinite(s["feature_fd"].item()) and tuple(s["feature_fd_per_class"].shape) == (3,)
    # per_class: the first samples of every class
    s8 = metrics.classifier_scores(clf, xg, yg, xr, yr, per_class=8, batch=16)
    per8 = metrics.frechet_features(fg, fr, yg, yr, 8)
    assert np.array_equal(s8["feature_fd_per_class"].cpu().numpy(), per8["values"].cpu().numpy())
    # labels rotated by one class: the generator "disobeys" every label
    rot = metrics.classifier_scores(clf, xg, (yg + 1) % 3, xr, batch=16)
    assert rot["accuracy"] == 0.0 and rot["correct"] == 0 and "accuracy_real" not in rot
