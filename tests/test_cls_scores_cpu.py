"""kg_cls_scores and what is built on it, without a GPU: the float64 definition on a hand-computed case, the
pair tables, the record's column names and senses, the entry point's host-side rejections and layout, the tools' flags."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build, evaluate, metrics

import abi_layout
from cls_scores_def import cls_scores_def, in_order_means

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


# ---- the definition ----------------------------------------------------------------------------------------------------

def test_definition_on_a_hand_computed_case():
    """three rows (0, 0), (3, 4), (6, 8): distances 5, 10, 5, 0; labels (0, 1, 1), predictions (0, 1, 0)"""
    x = np.array([[0, 0], [3, 4], [6, 8]], dtype=np.float32)
    d = cls_scores_def([x], [[0, 1, 0]], [0, 1, 1], div_pairs=[[0, 1], [0, 2]], mm_pairs=[[0, 0], [1, 2]], n_classes=2)
    assert d["dist"].tolist() == [[5.0, 10.0, 0.0, 5.0]]
    assert d["correct_per_class"].tolist() == [[1, 1]] and d["count_per_class"].tolist() == [1, 2]
    assert d["correct"].tolist() == [2]
    assert d["scores64"].tolist() == [[2.0 / 3.0, 7.5, 2.5]]
    assert d["scores"].dtype == np.float32 and d["scores"].tolist() == [[float(np.float32(2.0 / 3.0)), 7.5, 2.5]]
    # a label outside [0, K) is counted nowhere; a pair index outside [0, N) gives NaN
    e = cls_scores_def([x], [[0, 1, 0]], [0, 5, -1], [[0, 3]], [[0, 0], [-1, 1]], 2)
    assert e["count_per_class"].tolist() == [1, 0] and e["correct"].tolist() == [1]
    assert np.isnan(e["dist"][0, 0]) and e["dist"][0, 1] == 0.0 and np.isnan(e["dist"][0, 2])
    assert in_order_means([1.0, 2.0, 4.0], 2) == (1.5, 4.0)


# ---- the pair tables ---------------------------------------------------------------------------------------------------

def restated_tables(lab, K, Sd, Sl, seed):
    """the documented draw order, written again"""
    r = np.random.RandomState(seed)
    a, b = r.choice(len(lab), Sd, replace=False), r.choice(len(lab), Sd, replace=False)
    mm = []
    for c in range(K):
        rows = np.array([i for i, y in enumerate(lab) if y == c])
        p, q = r.choice(len(rows), Sl, replace=False), r.choice(len(rows), Sl, replace=False)
        mm += list(zip(rows[p], rows[q]))
    return np.array(list(zip(a, b))), np.array(mm)


@pytest.mark.parametrize("K,P,Sd,Sl,seed", [(1, 1, 1, 1, 0), (3, 4, 12, 4, 1), (10, 6, 33, 3, 7), (60, 3, 100, 2, 123)])
def test_pair_tables(K, P, Sd, Sl, seed):
    lab = np.random.RandomState(seed + 1).permutation(np.repeat(np.arange(K), P))
    div, mm = metrics.cls_pair_tables(lab, K, Sd, Sl, seed)
    assert div.dtype == np.int32 and mm.dtype == np.int32 and div.shape == (Sd, 2) and mm.shape == (K * Sl, 2)
    for t in (div, mm):
        assert t.min() >= 0 and t.max() < lab.size
    want_div, want_mm = restated_tables(lab.tolist(), K, Sd, Sl, seed)
    assert np.array_equal(div, want_div) and np.array_equal(mm, want_mm)
    assert np.array_equal(lab[mm], np.repeat(np.arange(K), Sl)[:, None] * np.ones((1, 2), dtype=np.int64))   # class-major
    for col in (div[:, 0], div[:, 1]):                   # without replacement inside a draw
        assert np.unique(col).size == Sd
    again = metrics.cls_pair_tables(lab, K, Sd, Sl, seed)
    assert np.array_equal(again[0], div) and np.array_equal(again[1], mm)
    if lab.size > 2:
        other = metrics.cls_pair_tables(lab, K, Sd, Sl, seed + 1)
        assert not (np.array_equal(other[0], div) and np.array_equal(other[1], mm))


def test_pair_tables_value_errors():
    lab = [0, 0, 1, 1, 1]
    metrics.cls_pair_tables(lab, 2, 5, 2, 0)
    with pytest.raises(ValueError, match="diversity_pairs"):
        metrics.cls_pair_tables(lab, 2, 6, 2, 0)
    with pytest.raises(ValueError, match="class 0"):
        metrics.cls_pair_tables(lab, 2, 5, 3, 0)
    with pytest.raises(ValueError, match="class 2"):
        metrics.cls_pair_tables(lab, 3, 5, 1, 0)       # a class without members
    for bad in ([0, 2, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match="outside"):
            metrics.cls_pair_tables(bad, 2, 1, 1, 0)


# ---- the record's columns ----------------------------------------------------------------------------------------------

def test_score_names_and_sense():
    assert metrics.CLS_NAMES == ("accuracy", "feature_fd", "diversity", "multimodality")
    plain = evaluate.score_names(["live", "ema"], ["avg"], True, ("pose",))
    assert evaluate.score_names(["live", "ema"], ["avg"], True, ("pose",), classifier=False) == plain
    names = evaluate.score_names(["live", "ema"], ["avg"], True, ("pose",), classifier=True)
    assert names[:len(plain)] == plain
    assert names[len(plain):] == ["%s/%s" % (g, q) for g in ("live", "ema") for q in metrics.CLS_NAMES]
    assert evaluate.score_sense("live/accuracy") == "max" and evaluate.score_sense("ema/feature_fd") == "min"
    assert evaluate.score_sense("live/coverage") == "max" and evaluate.score_sense("live/avg") == "min"
    assert evaluate.score_sense("live/pose_fd") == "min"
    for name in ("live/diversity", "ema/multimodality"):
        with pytest.raises(ValueError):
            evaluate.score_sense(name)


def test_evaluator_signature():
    p = inspect.signature(evaluate.Evaluator.__init__).parameters
    got = {k: p[k].default for k in ("classifier", "classifier_per_class", "classifier_batch", "diversity_pairs",
                                     "multimodality_pairs")}
    assert got == dict(classifier=None, classifier_per_class=0, classifier_batch=512, diversity_pairs=200, multimodality_pairs=20)
    from kinetic_gan_amd.train import TrainLoop
    p = inspect.signature(TrainLoop.__init__).parameters
    got = {k: p[k].default for k in ("eval_classifier", "eval_classifier_samples", "eval_classifier_batch", "eval_diversity_pairs",
                                     "eval_multimodality_pairs")}
    assert got == dict(eval_classifier=None, eval_classifier_samples=0, eval_classifier_batch=512, eval_diversity_pairs=200,
                       eval_multimodality_pairs=20)


def test_classifier_scores_signature_defaults():
    p = inspect.signature(metrics.classifier_scores).parameters
    assert list(p)[:8] == ["clf", "gen", "labels_gen", "real", "labels_real", "per_class", "batch", "class_fd"]
    assert (p["labels_real"].default, p["per_class"].default, p["batch"].default, p["class_fd"].default) == (None, None, 512, True)
    assert (p["diversity_pairs"].default, p["multimodality_pairs"].default, p["pair_seed"].default) == (0, 0, 0)
    p = inspect.signature(_native.cls_head_fwd).parameters
    assert p["feat_out"].default is None and p["pred_out"].default is None


def test_the_select_rejection_needs_no_gpu():
    """the column exists and is refused before anything touches a device"""
    for name in ("live/diversity", "live/multimodality"):
        with pytest.raises(ValueError, match="closer"):
            evaluate.Evaluator({"live": object()}, None, classifier=object(), classifier_per_class=3, select=name)
    with pytest.raises(ValueError, match="none of"):     # without the classifier the column does not exist
        evaluate.Evaluator({"live": object()}, None, select="live/accuracy")


def test_check_classifier_meta():
    from kinetic_gan_amd.classifier import check_classifier_meta, load_classifier  # noqa: F401
    run = dict(dataset="ntu", n_classes=60, in_channels=3, t_size=64, scale=0.25, shift=-1.0)
    check_classifier_meta(dict(run, latent=512, feat_dim=64), run)
    for k, v in (("dataset", "h36m"), ("n_classes", 10), ("in_channels", 2), ("t_size", 32), ("scale", 0.5), ("shift", 0.0)):
        with pytest.raises(ValueError, match=k):
            check_classifier_meta(dict(run, **{k: v}), run)


# ---- the entry point ---------------------------------------------------------------------------------------------------

def test_entry_point_declared_exported_and_laid_out(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kgan_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert re.search(r"\bkg_cls_scores\s*\(", txt) and hasattr(raw, "kg_cls_scores") and "kg_cls_scores" in _native.EXPORTS
    abi_layout.assert_mirror("KgClsScoresArgs")
    assert abi_layout.header_constants()["KG_CLS_MAX_SETS"] == _native.CLS_MAX_SETS == 4
    assert lib.kg_abi_version() == 9


OPERANDS = ("labels", "div_pairs", "mm_pairs", "dist", "scores64", "scores", "correct", "correct_per_class", "count_per_class")


def _good_args():
    a = _native._ClsScoresArgs()
    a.nsets, a.N, a.F, a.K, a.Sd, a.Sl, a.feat_ld = 2, 7, 16, 3, 5, 2, 16
    for s in range(2):
        a.feat[s], a.pred[s] = 0x1000, 0x1000          # never dereferenced: every call below is rejected on the host
    for f in OPERANDS:
        setattr(a, f, 0x1000)
    return a


def test_invalid_arguments_are_rejected_without_gpu(lib):
    def rejected(a):
        assert lib.kg_cls_scores(ctypes.byref(a), None) < 0
        assert b"kg_cls_scores" in lib.kg_last_error(), lib.kg_last_error()

    assert lib.kg_cls_scores(None, None) < 0 and b"kg_cls_scores" in lib.kg_last_error()
    for field, bad in (("nsets", 0), ("nsets", 5), ("N", 0), ("F", 0), ("F", 97), ("K", 0), ("K", 1025), ("Sd", 0), ("Sl", 0),
                       ("feat_ld", 15), ("N", -1), ("Sd", -3)):
        a = _good_args()
        setattr(a, field, bad)
        rejected(a)
        assert field.encode() in lib.kg_last_error()
    for f in OPERANDS:
        a = _good_args()
        setattr(a, f, None)
        rejected(a)
    for arr in ("feat", "pred"):
        for s in range(2):
            a = _good_args()
            getattr(a, arr)[s] = None
            rejected(a)
    a = _good_args()                                     # the sets beyond nsets are not looked at
    a.nsets = 1
    a.feat[1] = a.pred[1] = None
    a.N = 0
    rejected(a)
    assert b"N=0" in lib.kg_last_error()


# ---- the tools ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tool,flags", [
    ("classify_actions.py", ("--diversity_pairs", "--multimodality_pairs", "--pair_seed", "--per_class_table")),
    ("train.py", ("--eval_classifier", "--eval_classifier_samples", "--eval_classifier_batch", "--eval_diversity_pairs",
                  "--eval_multimodality_pairs")),
    ("time_eval.py", ("--classifier",))])
def test_tools_list_their_new_flags(tool, flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for f in flags:
        assert f in r.stdout, (tool, f)
