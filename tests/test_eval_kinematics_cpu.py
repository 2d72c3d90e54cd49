"""The kinematic columns inside the Evaluator, without a GPU: declaration / export / ctypes mirrors of
kg_kin_desc_sets and kg_eval_record3, their host-side rejections and the workspace formula, score names and senses, the csv
writer with 40 columns, the Evaluator's argument errors, the state check and the command line's flags."""
import csv
import ctypes
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build, evaluate, metrics
from kinetic_gan_amd.graph import Graph_h36m, graph_ntu

import abi_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIN12 = ["%s/%s" % (g, q) for g in ("live", "ema") for q in ("bone_cv", "asymmetry", "speed", "accel", "jerk", "still")]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


# ---- declaration, export, mirrors ----------------------------------------------------------------------------------------

def test_header_declares_and_library_exports(lib):
    txt = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, arg, nargs in (("kg_kin_desc_sets", "KgKinDescSetsArgs", 2), ("kg_kin_desc_sets_workspace_bytes", "KgKinDescSetsArgs", 1),
                             ("kg_kin_desc_sets_lds_bytes", "KgKinDescSetsArgs", 1), ("kg_eval_record3", "KgEvalRecord3Args", 2)):
        assert re.search(r"\b%s\s*\(\s*const %s\*" % (name, arg), code), "%s is not declared in kgan_hip.h" % name
        assert hasattr(ctypes.CDLL(_native.LIB_PATH), name) and getattr(lib, name) is not None
        assert len(_native.EXPORTS[name][1]) == nargs
    assert "#define KG_EVAL3_MAX_SCORES 64" in txt and _native.EVAL3_MAX_SCORES == 64
    assert "#define KG_EVAL2_MAX_SCORES 32" in txt and _native.EVAL2_MAX_SCORES == 32        # (the existing records are untouched)
    assert "#define KG_EVAL_MAX_SCORES 8" in txt and _native.EVAL_MAX_SCORES == 8
    assert "#define KG_KIN_MAX_SETS 4" in txt and _native.KIN_MAX_SETS == 4
    assert all(callable(getattr(_native, f)) for f in ("kin_desc_sets", "kin_desc_sets_workspace_bytes", "kin_desc_sets_lds_bytes",
                                                       "eval_record3"))
    assert lib.kg_abi_version() == 9 and _native.ABI_VERSION == 9


@pytest.mark.parametrize("cname,mirror", [("KgKinDescSetsArgs", "_KinDescSetsArgs"), ("KgEvalRecord3Args", "_EvalRecord3Args")])
def test_structs_match_header(cname, mirror):
    assert abi_layout.mirrors()[cname] is getattr(_native, mirror)
    abi_layout.assert_mirror(cname)


# ---- rejections without a GPU call ---------------------------------------------------------------------------------------

def _sets_args(nsets=2, **kw):
    """a valid h36m call (K 3, n 5, T 8) on made-up device addresses; the keywords overwrite fields, ``null`` clears one"""
    bones, mirror = list(Graph_h36m.bones), list(Graph_h36m.mirror_bones)
    tb = (ctypes.c_int32 * (2 * len(bones)))(*[int(v) for b in bones for v in b])
    tm = (ctypes.c_int32 * (2 * len(mirror)))(*[int(v) for p in mirror for v in p])
    a = _native._KinDescSetsArgs()
    for g in range(min(max(nsets, 0), _native.KIN_MAX_SETS)):
        a.x[g] = 0x10000 + 0x1000 * g
        a.desc[g] = 0x20000 + 0x1000 * g
    a.nsets, a.n, a.T, a.C, a.V, a.classes = nsets, 5, 8, 2, 16, 3
    a.sc, a.ss, a.sf, a.so = 256, 768, 16, 128
    a.B, a.M = len(bones), len(mirror)
    a.bones, a.mirror = ctypes.cast(tb, ctypes.c_void_p), ctypes.cast(tm, ctypes.c_void_p)
    a.still_eps = 1e-3
    a.degenerate, a.ws, a.counters, a.counters_len = 0x30000, 0x40000, 0x50000, 1
    a.ws_bytes = 4 * max(nsets, 1) * 3 * 5
    null = kw.pop("null", None)
    for k, v in kw.items():
        setattr(a, k, v)
    if null in ("x", "desc"):
        getattr(a, null)[nsets - 1] = None
    elif null:
        setattr(a, null, None)
    return a, (tb, tm)


def test_workspace_and_lds_formulas(lib):
    for nsets in (1, 2, 3, 4):
        a, keep = _sets_args(nsets)
        assert lib.kg_kin_desc_sets_workspace_bytes(ctypes.byref(a)) == 4 * nsets * 3 * 5
        one = _native._KinDescArgs()
        for f in ("n", "T", "C", "V", "classes", "B", "M", "bones", "mirror", "still_eps"):
            setattr(one, f, getattr(a, f))
        assert lib.kg_kin_desc_sets_lds_bytes(ctypes.byref(a)) == lib.kg_kin_desc_lds_bytes(ctypes.byref(one)) > 4 * 2 * 8 * 16
    bones, mirror = list(graph_ntu.bones), list(graph_ntu.mirror_bones)
    assert _native.kin_desc_sets_workspace_bytes(4, 100, 64, 3, 25, 60, bones, mirror) == 4 * 4 * 60 * 100
    assert _native.kin_desc_sets_lds_bytes(4, 100, 64, 3, 25, 60, bones, mirror) == _native.kin_desc_lds_bytes(100, 64, 3, 25, 60, bones, mirror)


def test_kg_kin_desc_sets_rejects_bad_arguments_without_gpu(lib):
    cases = [(dict(nsets=0), b"nsets=0"), (dict(nsets=5), b"nsets=5"), (dict(nsets=-1), b"nsets=-1"),
             (dict(nsets=2, null="x"), b"null pointer x[1]"), (dict(nsets=3, null="desc"), b"null pointer desc[2]"),
             (dict(nsets=1, null="x"), b"null pointer x[0]"),
             (dict(nsets=4, classes=1 << 11, n=1 << 11, ws_bytes=1 << 40), b"nsets * classes * n"),
             (dict(classes=0), b"classes=0"), (dict(n=0), b"n=0"), (dict(classes=1 << 12, n=1 << 12), b"classes * n"),
             (dict(C=4), b"C=4"), (dict(V=33), b"V=33"), (dict(B=0), b"B=0"), (dict(B=33), b"B=33"), (dict(M=17), b"M=17"),
             (dict(T=3), b"T=3"), (dict(T=2048), b"C*T*V"), (dict(sc=-1), b"negative stride"), (dict(still_eps=float("nan")), b"still_eps"),
             (dict(still_eps=-1.0), b"still_eps"), (dict(null="bones"), b"bones"), (dict(null="mirror"), b"mirror"),
             (dict(V=15), b"bones["), (dict(B=3), b"mirror["), (dict(null="degenerate"), b"degenerate"), (dict(null="ws"), b"ws"),
             (dict(null="counters"), b"counters"), (dict(counters_len=0), b"counters_len"), (dict(nsets=2, ws_bytes=4 * 2 * 15 - 4), b"ws_bytes")]
    for kw, word in cases:
        a, keep = _sets_args(**kw)
        assert lib.kg_kin_desc_sets(ctypes.byref(a), None) < 0, kw
        assert b"kg_kin_desc_sets" in lib.kg_last_error() and word in lib.kg_last_error(), (kw, lib.kg_last_error())
    assert lib.kg_kin_desc_sets(None, None) < 0 and lib.kg_kin_desc_sets_workspace_bytes(None) < 0
    a, keep = _sets_args(5)
    assert lib.kg_kin_desc_sets_workspace_bytes(ctypes.byref(a)) < 0 and b"nsets=5" in lib.kg_last_error()
    assert lib.kg_kin_desc_sets_lds_bytes(ctypes.byref(a)) < 0 and b"nsets=5" in lib.kg_last_error()
    # the one-set entry point keeps its own messages
    one = _native._KinDescArgs()
    assert lib.kg_kin_desc(ctypes.byref(one), None) < 0 and b"kg_kin_desc: classes=0" in lib.kg_last_error()


def _record3_args(nscores=1, select=0, ring_len=4, null=None):
    a = _native._EvalRecord3Args()
    p = 0x1000
    for i in range(min(nscores, _native.EVAL3_MAX_SCORES)):
        a.scores[i] = p
    a.nscores, a.select, a.ring_len, a.maximise = nscores, select, ring_len, 1
    a.iter = a.count = a.ring_val = a.ring_iter = a.best_val = a.best_iter = a.flag = p
    if null == "score":
        a.scores[nscores - 1] = None
    elif null:
        setattr(a, null, None)
    return a


def test_kg_eval_record3_rejects_bad_arguments_without_gpu(lib):
    for kw, word in ((dict(nscores=0), b"nscores=0"), (dict(nscores=65), b"nscores=65"), (dict(nscores=40, select=40), b"select=40"),
                     (dict(select=-1), b"select"), (dict(ring_len=0), b"ring_len"), (dict(null="count"), b"null"),
                     (dict(null="flag"), b"null"), (dict(null="best_val"), b"null"), (dict(nscores=64, null="score"), b"null score 63")):
        assert lib.kg_eval_record3(ctypes.byref(_record3_args(**kw)), None) < 0, kw
        assert b"kg_eval_record3" in lib.kg_last_error() and word in lib.kg_last_error(), (kw, lib.kg_last_error())
    assert lib.kg_eval_record3(None, None) < 0


# ---- names, senses, the csv writer ---------------------------------------------------------------------------------------

def test_score_names_and_senses():
    names = evaluate.score_names(("live", "ema"), ("avg", "joint"), True, ("pose", "motion"), True, True, kinematics=True)
    today = evaluate.score_names(("live", "ema"), ("avg", "joint"), True, ("pose", "motion"), True, True)
    assert len(today) == 28 and len(names) == 40 <= _native.EVAL3_MAX_SCORES
    assert names[:28] == today and names[28:] == KIN12
    assert metrics.KIN_NAMES == ("bone_cv", "asymmetry", "speed", "accel", "jerk", "still")
    assert evaluate.score_sense("ema/jerk") == "min"
    assert [evaluate.score_sense(n) for n in KIN12] == ["min"] * 12
    assert evaluate.score_names(["a"], ("avg",), kinematics=True) == ["a/avg"] + ["a/" + q for q in metrics.KIN_NAMES]
    assert evaluate.score_names(["a"], ("avg",)) == ["a/avg"]
    assert evaluate.NO_SENSE == ("diversity", "multimodality", "authenticity")


def test_write_metrics_csv_round_trips_40_columns(tmp_path):
    names = evaluate.score_names(("live", "ema"), ("avg", "joint"), True, ("pose", "motion"), True, True, kinematics=True)
    rng = np.random.RandomState(0)
    scores = rng.standard_normal((3, 40)).astype(np.float32)
    scores[1, 33] = np.nan                       # a generator that emitted a non-finite value
    scores[2, 39] = np.float32(1e-30)
    rec = {"names": names, "iteration": np.array([2 ** 24 + 3, 2 ** 24 + 5, 2 ** 24 + 7]), "scores": scores,
           "improved": np.array([True, False, True])}
    path = str(tmp_path / "metrics.csv")
    evaluate.write_metrics_csv(path, rec)
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["iteration"] + names + ["improved"] and len(rows) == 4
    back = np.array([[float(v) for v in r[1:41]] for r in rows[1:]], dtype=np.float32)
    assert np.array_equal(back.view(np.uint32)[~np.isnan(scores)], scores.view(np.uint32)[~np.isnan(scores)])
    assert np.array_equal(np.isnan(back), np.isnan(scores))
    assert [int(r[0]) for r in rows[1:]] == rec["iteration"].tolist() and [r[-1] for r in rows[1:]] == ["1", "0", "1"]


# ---- the Evaluator's argument errors and the state ------------------------------------------------------------------------

def test_evaluator_argument_errors_without_device():
    gens = {"a": object()}
    with pytest.raises(ValueError, match="kinematics_per_class=-1"):
        evaluate.Evaluator(gens, None, kinematics_per_class=-1, kinematics_dataset="h36m")
    with pytest.raises(ValueError, match="kinematics_dataset"):
        evaluate.Evaluator(gens, None, kinematics_per_class=3)
    with pytest.raises(ValueError, match="kinematics_dataset.*undefined dataset 'kinetics'"):
        evaluate.Evaluator(gens, None, kinematics_per_class=3, kinematics_dataset="kinetics")
    with pytest.raises(ValueError, match="kinematics_per_class=%d.*above the cap of %d" % (_native.KIN_MAX_POINTS // 2 + 1, _native.KIN_MAX_POINTS)):
        evaluate.Evaluator(gens, None, kinematics_per_class=_native.KIN_MAX_POINTS // 2 + 1, kinematics_dataset="h36m")
    with pytest.raises(ValueError, match="select 'a/jerk' is none of"):                      # a kinematic name with the option off
        evaluate.Evaluator(gens, None, select="a/jerk")
    with pytest.raises(ValueError, match="70 scores, at most 64"):                           # kg_eval_record3's room
        evaluate.Evaluator({str(i): object() for i in range(10)}, None, modes=("avg",), kinematics_per_class=3, kinematics_dataset="h36m")
    with pytest.raises(ValueError, match="40 scores, at most 32"):                           # off: the limits of today
        evaluate.Evaluator({str(i): object() for i in range(5)}, None, prdc_per_class=8, prdc_k=3, frechet_per_class=8)


def _stub(kin=0, still_eps=1e-3, old=False):
    """what Evaluator.check_compatible reads of an Evaluator; ``old``: an object of before the kinematic columns"""
    names = evaluate.score_names(["a"], ("avg",), kinematics=bool(kin))
    ns = types.SimpleNamespace(prdc_per_class=0, prdc_k=3, frechet_per_class=0, frechet_modes=(), pairs=2, select="a/avg",
                               modes=("avg",), names=names, ring_val=torch.zeros(8, len(names)), snap_flat=torch.zeros(5),
                               snap_buffers={"b": torch.zeros(1)})
    if not old:
        bones, mirror = metrics._kin_tables("h36m", None, None, "stub")
        ns.kinematics_per_class, ns.kinematics_still_eps = kin, still_eps
        ns.kinematics_bones, ns.kinematics_mirror = (bones, mirror) if kin else (None, None)
    return ns


def _state(stub):
    sd = {"pairs": 2, "select": "a/avg", "modes": ["avg"], "names": list(stub.names), "ring_val": torch.zeros(8, len(stub.names)),
          "snapshot": {"flat": torch.zeros(5), "buffers": {"b": torch.zeros(1)}}}
    if getattr(stub, "kinematics_per_class", 0):
        sd["kinematics"] = evaluate._kinematics_state(stub)
    return sd


def test_state_check():
    on, off, old = _stub(3), _stub(0), _stub(0, old=True)
    check = evaluate.Evaluator.check_compatible
    sd_on, sd_off = _state(on), _state(off)
    assert sd_on["kinematics"]["per_class"] == 3 and sd_on["kinematics"]["still_eps"] == 1e-3
    assert sd_on["kinematics"]["bones"] == [list(b) for b in Graph_h36m.bones] and "kinematics" not in sd_off
    check(on, sd_on)
    check(off, sd_off)
    check(old, sd_off)                          # a state without the key loads into an Evaluator with the option off
    for ev, sd in ((off, sd_on), (old, sd_on), (on, sd_off), (_stub(4), sd_on), (_stub(3, still_eps=2e-3), sd_on)):
        with pytest.raises(ValueError, match="kinematics"):
            check(ev, dict(sd, names=list(ev.names), ring_val=torch.zeros(8, len(ev.names))))
    flipped = dict(sd_on, kinematics=dict(sd_on["kinematics"], mirror=sd_on["kinematics"]["mirror"][:-1]))
    with pytest.raises(ValueError, match="kinematics"):
        check(on, flipped)


# ---- the command line -----------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_command_flags(capsys):
    tool = _tool("train")
    base = ["--data_path", "d.npy", "--label_path", "l.pkl"]
    opt = tool.parse_args(base)
    assert opt.eval_kinematics == 0 and opt.eval_kinematics_still_eps == 1e-3
    opt = tool.parse_args(base + ["--eval_kinematics", "100", "--eval_kinematics_still_eps", "0.01", "--eval_select", "ema/jerk"])
    assert opt.eval_kinematics == 100 and opt.eval_kinematics_still_eps == 0.01 and opt.eval_select == "ema/jerk"
    with pytest.raises(SystemExit):
        tool.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "<bone_cv|asymmetry|speed|accel|jerk|still>" in text and "--eval_kinematics" in text
