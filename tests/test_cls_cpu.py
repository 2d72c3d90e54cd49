"""The action classifier without a GPU: the head's entry points are declared, exported and reject bad
arguments on the host; its float64 definition (tests/cls_def.py) agrees with torch; classifier.Classifier under emulation
agrees with the host oracle; both command-line tools parse their flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd.classifier import Classifier
from kinetic_gan_amd.discriminator import Discriminator
from oracle.fill import fill_module

import abi_layout
import cls_def
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("kg_cls_head_workspace_bytes", "kg_cls_head_fwd", "kg_cls_head_bwd", "kg_cls_head_wgrad")
# (N, C, T', V', F, L) of tests/test_cls_gpu.py
GPU_SHAPES = [(1, 8, 1, 1, 1, 2), (5, 72, 2, 1, 16, 10), (7, 512, 4, 1, 64, 60), (33, 512, 2, 3, 96, 120), (64, 64, 1, 1, 16, 4)]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def test_entry_points_declared_and_exported(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kgan_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(raw, name) and name in _native.EXPORTS
    assert "kg_cls.hip" in build.SOURCES
    abi_layout.assert_mirror("KgClsHeadArgs")
    assert lib.kg_abi_version() == 9
    assert _native.EXPORTS["kg_cls_head_workspace_bytes"][0] is ctypes.c_int64


def _good_args():
    a = _native._ClsHeadArgs()
    a.N, a.C, a.T, a.V, a.F, a.L, a.slope = 4, 16, 2, 1, 8, 5, 0.2
    a.h_sN, a.h_sC = 2, 8
    for f in ("h", "w1", "b1", "w2", "b2", "labels", "pooled", "feat", "logits", "loss_per_sample", "pred", "loss", "correct",
              "gtop", "g", "dw1", "db1", "dw2", "db2", "ws"):
        setattr(a, f, 0x1000)          # never dereferenced: every call below is rejected on the host
    a.ws_bytes = 4 * 4 * (5 + 8)
    return a


def test_invalid_arguments_are_rejected_without_gpu(lib):
    calls = [(n, getattr(lib, n)) for n in ENTRIES[1:]]

    def rejected(a, name, fn):
        assert fn(ctypes.byref(a), None) < 0, name
        assert name.encode() in lib.kg_last_error(), (name, lib.kg_last_error())

    for name, fn in calls:
        assert fn(None, None) < 0 and name.encode() in lib.kg_last_error()
        for field, bad in (("F", 97), ("F", 0), ("L", 0), ("N", 0), ("C", 0), ("T", 0)):
            a = _good_args()
            setattr(a, field, bad)
            rejected(a, name, fn)
    assert lib.kg_cls_head_workspace_bytes(None) < 0 and b"kg_cls_head_workspace_bytes" in lib.kg_last_error()
    for field, bad in (("F", 97), ("L", 0), ("N", 0)):
        a = _good_args()
        setattr(a, field, bad)
        assert lib.kg_cls_head_workspace_bytes(ctypes.byref(a)) < 0 and b"kg_cls_head_workspace_bytes" in lib.kg_last_error()
    # NULL operands
    for name, fields in (("kg_cls_head_fwd", ("h", "w1", "b1", "w2", "b2", "pooled", "feat", "logits", "pred", "loss", "correct",
                                              "loss_per_sample")),
                         ("kg_cls_head_bwd", ("w1", "w2", "labels", "feat", "logits", "gtop", "g", "ws")),
                         ("kg_cls_head_wgrad", ("pooled", "feat", "dw1", "db1", "dw2", "db2", "ws"))):
        for f in fields:
            a = _good_args()
            setattr(a, f, None)
            rejected(a, name, getattr(lib, name))
    a = _good_args()
    a.masked, a.h = 1, None          # the mask is read from h
    rejected(a, "kg_cls_head_bwd", lib.kg_cls_head_bwd)
    # a workspace that is too small
    for name in ("kg_cls_head_bwd", "kg_cls_head_wgrad"):
        a = _good_args()
        a.ws_bytes -= 4
        rejected(a, name, getattr(lib, name))
        assert b"ws_bytes" in lib.kg_last_error()


def test_workspace_formula(lib):
    for (N, C, T, V, F_, L) in GPU_SHAPES:
        assert _native.cls_head_workspace_bytes(N, C, T, V, F_, L) == cls_def.workspace_bytes(N, F_, L) == 4 * N * (L + F_)


@pytest.mark.parametrize("shape", GPU_SHAPES[:4] + [(6, 24, 2, 2, 12, 7)])
@pytest.mark.parametrize("masked", [False, True])
def test_definition_against_torch_float64(shape, masked):
    """cls_def.head_def in float64 against F.cross_entropy + autograd in float64: every output and gradient to 1e-12"""
    N, C, T, V, F_, L = shape
    rs = np.random.RandomState(sum(shape))
    h = rs.randn(N, C, T, V)
    w1, b1, w2, b2 = rs.randn(F_, C) / np.sqrt(C), rs.randn(F_) * 0.1, rs.randn(L, F_) / np.sqrt(F_), rs.randn(L) * 0.1
    y = rs.randint(0, L, N)
    gtop = 0.7
    d = cls_def.head_def(h, w1, b1, w2, b2, y, 0.2, gtop=gtop, masked=masked)
    slope = float(np.float32(0.2))
    # with `masked` h is the LeakyReLU output of a pre-activation u; the gradient the definition returns is d / d u
    u = torch.tensor(np.where(h > 0, h, h / slope) if masked else h, requires_grad=True)
    ht = F.leaky_relu(u, slope) if masked else u
    tw1, tb1, tw2, tb2 = (torch.tensor(t, requires_grad=True) for t in (w1, b1, w2, b2))
    pooled = ht.mean(dim=(2, 3))
    pooled.retain_grad()
    feat = F.leaky_relu(F.linear(pooled, tw1, tb1), slope)
    feat.retain_grad()
    logits = F.linear(feat, tw2, tb2)
    logits.retain_grad()
    loss = F.cross_entropy(logits, torch.tensor(y))
    lps = F.cross_entropy(logits, torch.tensor(y), reduction="none")
    (loss * gtop).backward()

    def close(a, b, what):
        b = b.detach().numpy()
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (what, np.abs(a - b).max())

    close(d["pooled"], pooled, "pooled")
    close(d["feat"], feat, "feat")
    close(d["logits"], logits, "logits")
    close(d["loss_per_sample"], lps, "loss_per_sample")
    close(np.asarray(d["loss"]), loss, "loss")
    assert (d["pred"] == logits.argmax(1).numpy()).all()
    assert d["correct"] == int((logits.argmax(1).numpy() == y).sum())
    close(d["dlogits"], logits.grad, "dlogits")
    close(d["g"], u.grad, "g")
    close(d["dw1"], tw1.grad, "dw1")
    close(d["db1"], tb1.grad, "db1")
    close(d["dw2"], tw2.grad, "dw2")
    close(d["db2"], tb2.grad, "db2")
    # dfeat is the gradient at fc1's output (in front of the LeakyReLU)
    close(d["dfeat"], feat.grad * torch.where(feat > 0, 1.0, slope), "dfeat")


def test_definition_rules():
    """ties go to the lowest index, NaN never wins, a bad label gives NaN for its sample alone and is never correct"""
    lg = np.array([[1.0, 3.0, 3.0, 2.0], [np.nan, 5.0, 1.0, 0.0], [2.0, np.nan, 7.0, 7.0], [0.0, 0.0, 0.0, 0.0]])
    assert cls_def.pred_rule(lg).tolist() == [1, 0, 2, 0]
    rs = np.random.RandomState(0)
    h, w1, b1, w2, b2 = rs.randn(3, 4, 1, 1), rs.randn(5, 4), rs.randn(5), rs.randn(6, 5), rs.randn(6)
    good = cls_def.head_def(h, w1, b1, w2, b2, [1, 2, 3], gtop=1.0)
    bad = cls_def.head_def(h, w1, b1, w2, b2, [1, -1, 3], gtop=1.0)
    assert np.isnan(bad["loss_per_sample"][1]) and np.isnan(bad["loss"])
    assert (bad["loss_per_sample"][[0, 2]] == good["loss_per_sample"][[0, 2]]).all()
    assert np.isnan(bad["dlogits"][1]).all() and (bad["dlogits"][[0, 2]] == good["dlogits"][[0, 2]]).all()
    hit = cls_def.head_def(h, w1, b1, w2, b2, good["pred"].tolist())
    assert hit["correct"] == 3
    assert cls_def.head_def(h, w1, b1, w2, b2, [int(good["pred"][0]), -1, 99])["correct"] == 1


CASES = {"h36m": dict(channels=2, n_classes=10, T=32, V=16, n=4), "ntu": dict(channels=3, n_classes=60, T=64, V=25, n=4)}


def _pair(name, feat_dim=64):
    c = CASES[name]
    clf = Classifier(c["channels"], c["n_classes"], c["T"], dataset=name, feat_dim=feat_dim)
    ora = cls_def.OracleClassifier(c["channels"], c["n_classes"], c["T"], dataset=name, feat_dim=feat_dim)
    fill_module(clf, seed=5)
    fill_module(ora, seed=5)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(c["n"], c["channels"], c["T"], c["V"], generator=g) * 2 - 1
    y = torch.randint(0, c["n_classes"], (c["n"],), generator=g)
    return clf, ora, x, y


@pytest.mark.parametrize("name", ["h36m", "ntu"])
def test_classifier_against_oracle_emulated(name):
    """Both sides fp32 torch on the CPU: logits within 1e-5 of max, every parameter gradient within 1e-5 relative L2"""
    clf, ora, x, y = _pair(name)
    assert list(clf.state_dict()) == list(ora.state_dict())
    with cls_def.emulated_native():
        out = clf.classify(x, y)
        out["loss"].backward()
        with torch.no_grad():
            feat_ng = clf.features(x)
            logits_fw = clf(x)
    lo = ora(x)
    F.cross_entropy(lo, y).backward()
    print("logits", util.rel_err(out["logits"], lo))
    assert util.rel_err(out["logits"], lo) <= 1e-5
    assert util.rel_err(out["features"], ora.features(x)) <= 1e-5
    assert util.rel_err(out["loss"], F.cross_entropy(lo, y)) <= 1e-5
    assert torch.equal(feat_ng, out["features"]) and torch.equal(logits_fw, out["logits"])
    assert out["pred"].tolist() == lo.argmax(1).tolist()
    assert int(out["correct"]) == int((lo.argmax(1) == y).sum())
    po = dict(ora.named_parameters())
    worst = 0.0
    for k, p in clf.named_parameters():
        assert p.grad is not None, k
        worst = max(worst, util.l2_rel(p.grad, po[k].grad))
        assert util.l2_rel(p.grad, po[k].grad) <= 1e-5, (k, util.l2_rel(p.grad, po[k].grad))
    print("worst parameter gradient", worst)


def test_state_dict_keys_and_limits():
    clf = Classifier(3, 60, 64, dataset="ntu")
    D = Discriminator(3, 60, 64, 512, dataset="ntu")
    want = [k for k in D.state_dict() if k != "label_emb.weight" and not k.startswith("fcn.")]
    want += ["fc1.weight", "fc1.bias", "fcn.weight", "fcn.bias"]
    assert list(clf.state_dict()) == want
    assert not hasattr(clf, "label_emb")
    assert clf.st_gcn_networks[0].in_channels == 3 and clf.st_gcn_networks[0].res_kind == "none"
    assert tuple(clf.fc1.weight.shape) == (64, 512) and tuple(clf.fcn.weight.shape) == (60, 64)
    with pytest.raises(ValueError):
        Classifier(3, 60, 64, feat_dim=97)
    Classifier(3, 60, 64, feat_dim=_native.FRECHET_MAX_DIM)


def test_head_gradients_go_through_the_parameter_sink():
    """with a flat gradient bucket the head's four gradients are added into it (autograd sees None), like every layer's"""
    from kinetic_gan_amd.wgan_gp import FlatParams
    clf, ora, x, y = _pair("h36m", feat_dim=16)
    with cls_def.emulated_native():
        flat = FlatParams(clf)
        flat.zero_grad()
        clf.classify(x, y)["loss"].backward()
        flat.gather_grads()
    F.cross_entropy(ora(x), y).backward()
    po = dict(ora.named_parameters())
    for k, p in clf.named_parameters():
        assert util.l2_rel(p.grad, po[k].grad) <= 1e-5, k
    flat.release() if hasattr(flat, "release") else None


@pytest.mark.parametrize("tool", ["train_classifier.py", "classify_actions.py"])
def test_tools_parse_their_flags(tool):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    flags = {"train_classifier.py": ["--data_path", "--label_path", "--dataset", "--t_size", "--batch_size", "--n_epochs", "--lr",
                                     "--seed", "--feat_dim", "--val_data_path", "--val_label_path", "--eval_interval",
                                     "--checkpoint_interval", "--out", "--no-graph"],
             "classify_actions.py": ["--model", "--data_real", "--labels_real", "--data_fake", "--labels_fake", "--per_class",
                                     "--per_class_table"]}[tool]
    for f in flags:
        assert f in r.stdout, f
