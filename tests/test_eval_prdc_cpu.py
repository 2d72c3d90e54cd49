"""Precision / recall / density / coverage inside the Evaluator, without a GPU: declaration / export / ctypes
mirrors of kg_prdc_radii, kg_prdc_sets and kg_eval_record2, their host-side rejections, the workspace formula, the
definitions of tests/eval_prdc_def.py on hand-worked examples, score names and senses, the csv writer with 12 columns, the
Evaluator's argument errors and the command line's flags."""
import csv
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build, evaluate, metrics

import abi_layout
import eval_def
import eval_prdc_def
import prdc_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = [3, 2, 2, float("nan"), 5, 1, float("inf"), 1, 0.5, float("-inf"), 7, 7]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


# ---- declaration, export, mirrors ----------------------------------------------------------------------------------------

def test_header_declares_and_library_exports(lib):
    txt = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, arg, nargs in (("kg_prdc_radii", "KgPrdcRadiiArgs", 2), ("kg_prdc_sets", "KgPrdcSetsArgs", 2),
                             ("kg_prdc_sets_workspace_bytes", "KgPrdcSetsArgs", 1), ("kg_eval_record2", "KgEvalRecord2Args", 2)):
        assert re.search(r"\b%s\s*\(\s*const %s\*" % (name, arg), code), "%s is not declared in kgan_hip.h" % name
        assert hasattr(ctypes.CDLL(_native.LIB_PATH), name) and getattr(lib, name) is not None
        assert len(_native.EXPORTS[name][1]) == nargs
    assert "#define KG_PRDC_MAX_SETS 4" in txt and _native.PRDC_MAX_SETS == 4
    assert "#define KG_EVAL2_MAX_SCORES 32" in txt and _native.EVAL2_MAX_SCORES == 32
    assert "#define KG_EVAL_MAX_SCORES 8" in txt and _native.EVAL_MAX_SCORES == 8          # (the existing record is untouched)
    assert all(callable(getattr(_native, f)) for f in ("prdc_radii", "prdc_sets", "prdc_sets_workspace_bytes", "eval_record2"))


def test_abi_version_unchanged(lib):
    assert lib.kg_abi_version() == 9


@pytest.mark.parametrize("cname,mirror", [("KgPrdcRadiiArgs", "_PrdcRadiiArgs"), ("KgPrdcSetsArgs", "_PrdcSetsArgs"),
                                          ("KgEvalRecord2Args", "_EvalRecord2Args"), ("KgPrdcArgs", "_PrdcArgs"),
                                          ("KgEvalRecordArgs", "_EvalRecordArgs")])
def test_structs_match_header(cname, mirror):
    assert abi_layout.mirrors()[cname] is getattr(_native, mirror)
    abi_layout.assert_mirror(cname)


# ---- rejections without a GPU call ---------------------------------------------------------------------------------------

def _sets_args(nsets=2):
    a = _native._PrdcSetsArgs()
    a.real = 0x1000
    for g in range(nsets):
        a.fake[g] = 0x2000 + 0x100 * g
    a.r_sc, a.r_sp, a.r_so = 100 * 4800, 4800, 0
    a.f_sc, a.f_sp, a.f_so = 1600, 60 * 1600, 6000 * 1600
    a.nsets, a.n, a.m, a.d_outer, a.d_inner, a.classes, a.k = nsets, 100, 90, 3, 1600, 60, 5
    a.radii_real, a.counts, a.values, a.ws = 0x3000, 0x4000, 0x5000, 0x6000
    return a


@pytest.mark.parametrize("field,value,needle", [
    ("real", None, b"null pointer real"), ("fake1", None, b"null pointer fake[1]"), ("radii_real", None, b"null pointer radii_real"),
    ("counts", None, b"null pointer counts"), ("values", None, b"null pointer values"), ("ws", None, b"null pointer ws"),
    ("nsets", 0, b"nsets=0"), ("nsets", 5, b"nsets=5"), ("n", 0, b"n=0"), ("m", 0, b"m=0"), ("classes", 0, b"classes=0"),
    ("d_outer", 0, b"d_outer=0"), ("d_inner", 0, b"d_inner=0"), ("k", 0, b"k=0"), ("k", 33, b"k=33"),
    ("m", 4, b"k=5 > min(n=100, m=4) - 1"), ("n", 5, b"k=5 > min(n=5, m=90) - 1"), ("ws_bytes", 64, b"ws_bytes=64"),
    ("n", _native.PRDC_MAX_POINTS + 1, b"n=%d above the cap" % (_native.PRDC_MAX_POINTS + 1)),
    ("m", _native.PRDC_MAX_POINTS + 1, b"m=%d above the cap" % (_native.PRDC_MAX_POINTS + 1))])
def test_kg_prdc_sets_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _sets_args()
    need = lib.kg_prdc_sets_workspace_bytes(ctypes.byref(a))
    assert need == 4 * 2 * 60 * (2 * 90 + 100)
    a.ws_bytes = need
    if field == "fake1":
        a.fake[1] = None
    else:
        setattr(a, field, value)
    if field in ("nsets", "n", "m", "classes", "d_outer", "d_inner", "k"):
        assert lib.kg_prdc_sets_workspace_bytes(ctypes.byref(a)) < 0
        assert needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_prdc_sets(ctypes.byref(a), None) < 0
    assert b"kg_prdc_sets" in lib.kg_last_error() and needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_prdc_sets(None, None) < 0 and lib.kg_prdc_sets_workspace_bytes(None) < 0


def test_workspace_formula_and_launch_limit(lib):
    """4 nsets classes (2 m + n): fake radii, hit words, per-set flag words; linear in everything, no n x m term"""
    f = _native.prdc_sets_workspace_bytes
    for nsets in (1, 2, 4):
        for c in (1, 7, 60):
            for n, m in ((6, 33), (100, 100), (1000, 4096)):
                assert f(nsets, n, m, 3, 1600, c, 5) == 4 * nsets * c * (2 * m + n)
    assert f(1, 20, 20, 1, 7, 1, 19) == 4 * 60
    with pytest.raises(RuntimeError, match="k=20"):
        f(1, 20, 20, 1, 7, 1, 20)
    with pytest.raises(RuntimeError, match="nsets=5"):
        f(5, 20, 20, 1, 7, 1, 3)
    # a launch stays below 2^24 workgroups: 4 sets x 15 classes x 512 x 512 cross tiles of 64 pass, 16 classes are 2^24
    big = _native.PRDC_MAX_POINTS
    assert f(4, big, big, 1, 7, 15, 5) == 4 * 4 * 15 * 3 * big
    with pytest.raises(RuntimeError, match=r"nsets=4 x classes=16 .* 16777216 workgroups"):
        f(4, big, big, 1, 7, 16, 5)


def _radii_args():
    a = _native._PrdcRadiiArgs()
    a.x, a.sc, a.sp, a.so = 0x1000, 100 * 4800, 4800, 0
    a.n, a.d_outer, a.d_inner, a.classes, a.k, a.radii = 100, 3, 1600, 60, 5, 0x2000
    return a


@pytest.mark.parametrize("field,value,needle", [
    ("x", None, b"null pointer x"), ("radii", None, b"null pointer radii"), ("n", 0, b"n=0"), ("classes", 0, b"classes=0"),
    ("d_outer", 0, b"d_outer=0"), ("d_inner", -1, b"d_inner=-1"), ("k", 0, b"k=0"), ("k", 33, b"k=33"), ("n", 5, b"k=5 > n=5 - 1"),
    ("n", _native.PRDC_MAX_POINTS + 1, b"n=%d above the cap" % (_native.PRDC_MAX_POINTS + 1)),
    ("classes", 1 << 24, b"fewer than 16777216")])
def test_kg_prdc_radii_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _radii_args()
    setattr(a, field, value)
    assert lib.kg_prdc_radii(ctypes.byref(a), None) < 0
    assert b"kg_prdc_radii" in lib.kg_last_error() and needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_prdc_radii(None, None) < 0


def _record2_args(nscores=1, select=0, ring_len=4, null=None):
    a = _native._EvalRecord2Args()
    p = 0x1000
    for i in range(min(nscores, _native.EVAL2_MAX_SCORES)):
        a.scores[i] = p
    a.nscores, a.select, a.ring_len, a.maximise = nscores, select, ring_len, 1
    a.iter = a.count = a.ring_val = a.ring_iter = a.best_val = a.best_iter = a.flag = p
    if null == "score":
        a.scores[nscores - 1] = None
    elif null:
        setattr(a, null, None)
    return a


def test_kg_eval_record2_rejects_bad_arguments_without_gpu(lib):
    for kw, word in ((dict(nscores=0), b"nscores=0"), (dict(nscores=33), b"nscores=33"), (dict(nscores=12, select=12), b"select=12"),
                     (dict(select=-1), b"select"), (dict(ring_len=0), b"ring_len"), (dict(null="count"), b"null"),
                     (dict(null="flag"), b"null"), (dict(null="best_val"), b"null"), (dict(nscores=32, null="score"), b"null score 31")):
        assert lib.kg_eval_record2(ctypes.byref(_record2_args(**kw)), None) < 0, kw
        assert b"kg_eval_record2" in lib.kg_last_error() and word in lib.kg_last_error(), (kw, lib.kg_last_error())
    assert lib.kg_eval_record2(None, None) < 0


# ---- the definitions -----------------------------------------------------------------------------------------------------

def test_given_radii_hand_worked_example():
    """The example of tests/test_prdc_cpu.py: 1-D, R = 0, 0, 2, 5, F = 1, 3, 4, 10, k = 1; rho_F = 4, 1, 1, 36.
    d2 rows: [1 9 16 100] twice, [1 1 4 64], [16 4 1 25].  Q (<= rho_F, columns): {0, 1, 2}, {2}, {3}, {3} whatever rho_R is.
    With the true rho_R = 0, 0, 4, 9: P rows none, none, {0, 1, 2}, {1, 2} -> the counts of prdc_def.
    With rho_R halved = 0, 0, 2, 4.5: P rows none, none, {0, 1}, {1, 2} (4 <= 4.5, 1 <= 4.5; 16 is not): hits 1, 2, 1, 0,
    cP = 3, cD = 4, cC = 2; recall does not move."""
    R = torch.tensor([[0.0], [0.0], [2.0], [5.0]])
    F = torch.tensor([[1.0], [3.0], [4.0], [10.0]])
    full = prdc_def.one_class(R, F, 1)
    out = eval_prdc_def.given_radii_one_class(R, F, full["radii_real"], 1)
    for key in ("counts", "fake_hits", "real_flags", "radii_fake"):
        assert torch.equal(out[key], full[key]), key
    half = eval_prdc_def.given_radii_one_class(R, F, [0.0, 0.0, 2.0, 4.5], 1)
    assert half["radii_fake"].tolist() == [4.0, 1.0, 1.0, 36.0]
    assert half["fake_hits"].tolist() == [1, 2, 1, 0]
    assert half["real_flags"].tolist() == [1, 1, 3, 3]
    assert half["counts"].tolist() == [3, 4, 4, 2]
    # radii of zero: only exact hits count (none here), recall still as before
    zero = eval_prdc_def.given_radii_one_class(R, F, [0.0] * 4, 1)
    assert zero["counts"].tolist() == [0, 4, 0, 0] and zero["real_flags"].tolist() == [1, 1, 1, 1]
    both = eval_prdc_def.given_radii(torch.stack([R, R]), torch.stack([F, F]), torch.tensor([[0.0, 0.0, 4.0, 9.0], [0.0, 0.0, 2.0, 4.5]]), 1)
    assert both["counts"].tolist() == [[3, 4, 5, 2], [3, 4, 4, 2]]


def test_record2_both_senses():
    lo, hi = eval_prdc_def.Record2(1, 0, 4, maximise=False), eval_prdc_def.Record2(1, 0, 4, maximise=True)
    old = eval_def.Record(1, 0, 4)
    assert math.isinf(lo.best_val) and lo.best_val > 0 and math.isinf(hi.best_val) and hi.best_val < 0
    got_lo = [lo.append([s], 10 * (i + 1)) for i, s in enumerate(SEQ)]
    got_hi = [hi.append([s], 10 * (i + 1)) for i, s in enumerate(SEQ)]
    got_old = [old.append([s], 10 * (i + 1)) for i, s in enumerate(SEQ)]
    #                 3     2      2      nan    5      1     inf    1      0.5   -inf   7      7
    assert got_lo == [True, True, False, False, False, True, False, False, True, True, False, False] == got_old
    assert got_hi == [True, False, False, False, True, False, True, False, False, False, False, False]
    assert lo.best_val == -np.inf and lo.best_iter == 100 and hi.best_val == np.inf and hi.best_iter == 70
    assert np.array_equal(lo.ring_val, old.ring_val, equal_nan=True) and np.array_equal(lo.ring_iter, old.ring_iter)
    assert hi.ring_iter.tolist() == [[90, 0], [100, 0], [110, 0], [120, 0]] and hi.count == 12
    # a NaN never wins against the -inf start, and -inf is not above it
    r = eval_prdc_def.Record2(12, 11, 3, maximise=True)
    assert not r.append([0.0] * 11 + [float("nan")]) and not r.append([0.0] * 11 + [float("-inf")]) and r.best_iter == -1
    assert r.append([9.0] * 11 + [0.25], 2 ** 24 + 1) and r.best_iter == 2 ** 24 + 1 and r.best_val == np.float32(0.25)
    assert not r.append([9.0] * 11 + [0.25], 5) and r.best_iter == 2 ** 24 + 1              # equal: the earlier one stays


# ---- names, senses, files ------------------------------------------------------------------------------------------------

def test_score_names_and_senses():
    names = evaluate.score_names(["live", "ema"], ("avg", "joint"), prdc=True)
    assert names == ["live/avg", "live/joint", "ema/avg", "ema/joint",
                     "live/precision", "live/recall", "live/density", "live/coverage",
                     "ema/precision", "ema/recall", "ema/density", "ema/coverage"]
    assert evaluate.score_names(["live", "ema"], ("avg", "joint")) == names[:4]
    assert [evaluate.score_sense(n) for n in names] == ["min"] * 4 + ["max"] * 8
    assert evaluate.score_sense("g/avg") == "min" and evaluate.score_sense("coverage/joint") == "min"
    assert metrics.PRDC_NAMES == ("precision", "recall", "density", "coverage")


def test_class_rows():
    labels = [2, 0, 1, 1, 0, 2, 2, 0, 1]
    assert evaluate.class_rows(labels, 3, 2).tolist() == [1, 4, 2, 3, 0, 5]
    assert evaluate.class_rows(labels, 3, 3).tolist() == [1, 4, 7, 2, 3, 8, 0, 5, 6]
    with pytest.raises(ValueError, match="class 0 has 3 samples, 4 needed"):
        evaluate.class_rows(labels, 3, 4)


def test_csv_writer_with_12_columns_round_trips_bit_for_bit(tmp_path):
    names = evaluate.score_names(["live", "ema"], ("avg", "joint"), prdc=True)
    rng = np.random.RandomState(0)
    scores = rng.rand(5, 12).astype(np.float32)
    scores[1, 4], scores[2, 11], scores[3, 6], scores[4, 0] = np.nan, np.inf, 1.25, 1e-30
    scores[0, 7] = np.float32(1) / np.float32(3)
    rec = {"names": names, "iteration": np.array([2, 4, 6, 8, 2 ** 24 + 1], dtype=np.int64), "scores": scores,
           "improved": np.array([True, False, True, False, False])}
    path = str(tmp_path / "metrics.csv")
    evaluate.write_metrics_csv(path, rec)
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["iteration"] + names + ["improved"] and len(rows) == 6 and all(len(r) == 14 for r in rows)
    assert [int(r[0]) for r in rows[1:]] == rec["iteration"].tolist() and [int(r[13]) for r in rows[1:]] == [1, 0, 1, 0, 0]
    back = np.array([[float(v) for v in r[1:13]] for r in rows[1:]], dtype=np.float32)
    assert np.array_equal(back.view(np.uint32), scores.view(np.uint32))


def test_evaluator_argument_errors_without_device():
    gens = {"a": object()}
    with pytest.raises(ValueError, match="prdc_per_class=-1"):
        evaluate.Evaluator(gens, None, prdc_per_class=-1)
    for k in (0, 8, 33):
        with pytest.raises(ValueError, match="prdc_k=%d" % k):
            evaluate.Evaluator(gens, None, prdc_per_class=8, prdc_k=k)
    with pytest.raises(ValueError, match="above the cap"):
        evaluate.Evaluator(gens, None, prdc_per_class=_native.PRDC_MAX_POINTS + 1)
    with pytest.raises(ValueError, match="36 scores, at most 32"):
        evaluate.Evaluator({str(i): object() for i in range(6)}, None, prdc_per_class=8, prdc_k=3)
    with pytest.raises(ValueError, match="10 scores, at most 8"):                            # off: the limit of kg_eval_record
        evaluate.Evaluator({str(i): object() for i in range(5)}, None)
    with pytest.raises(ValueError, match="select 'a/coverage' is none of"):                  # a PRDC name with PRDC off
        evaluate.Evaluator(gens, None, select="a/coverage")
    with pytest.raises(ValueError, match="select 'b/coverage' is none of"):
        evaluate.Evaluator(gens, None, select="b/coverage", prdc_per_class=8, prdc_k=3)


def test_bindings_refuse_cpu_tensors_and_wrong_dtypes():
    x = torch.zeros(2, 10, 6)
    v = _native.PrdcView(x, 60, 6, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.prdc_radii(v, 10, 1, 6, 2, 3)
    with pytest.raises(TypeError, match="fp32 only"):
        _native.prdc_radii(_native.PrdcView(x.double(), 60, 6, 0), 10, 1, 6, 2, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.prdc_sets(v, [x, x], 60, 6, 0, torch.zeros(2, 10), 10, 10, 1, 6, 2, 3)
    with pytest.raises(TypeError, match="fp32 only"):
        _native.prdc_sets(v, [x.double()], 60, 6, 0, torch.zeros(2, 10), 10, 10, 1, 6, 2, 3)
    with pytest.raises(RuntimeError, match="nsets=5"):
        _native.prdc_sets(v, [x] * 5, 60, 6, 0, torch.zeros(2, 10), 10, 10, 1, 6, 2, 3)


def test_synthetic_set_of_the_gpu_tests_has_11_samples_of_every_class(tmp_path):
    """tests/test_eval_prdc_gpu.py selects 8 per class from index 1 on (metrics.select_reference_samples)"""
    import train_def
    from kinetic_gan_amd.feeder import Feeder
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 200, 2, 40, 16, 10, "h36m", seed=4)
    lab = np.asarray(Feeder(dp, lp, dataset="h36m").label)
    assert min(int((lab[1:] == c).sum()) for c in range(10)) >= 11
    data, labels, _ = metrics.select_reference_samples(Feeder(dp, lp, dataset="h36m"), np.arange(10), 32, per_class=8)
    assert data.shape == (80, 2, 32, 16) and labels.tolist() == np.repeat(np.arange(10), 8).tolist()


def test_train_command_flags():
    spec = importlib.util.spec_from_file_location("kg_tools_train", os.path.join(ROOT, "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opt = mod.parse_args(["--data_path", "d", "--label_path", "l"])
    assert opt.eval_prdc == 0 and opt.eval_prdc_k == 5                  # off by default
    opt = mod.parse_args(["--data_path", "d", "--label_path", "l", "--eval_interval", "100", "--eval_prdc", "100", "--eval_prdc_k", "3",
                          "--eval_select", "ema/coverage"])
    assert (opt.eval_prdc, opt.eval_prdc_k, opt.eval_select) == (100, 3, "ema/coverage")
