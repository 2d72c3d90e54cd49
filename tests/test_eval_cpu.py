"""Scoring during training without a GPU: the record's definition (tests/eval_def.py) against hand-worked
sequences, the entry points' declaration / export / host-side rejection, the row order of the real side, the sample
selection on a dataset too small for it, the csv writer, the default of ``eval_select``, the command line's flags."""
import csv
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build, evaluate, metrics
from kinetic_gan_amd.feeder import Feeder

import abi_layout
import eval_def
import train_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = [3, 2, 2, float("nan"), 5, 1, float("inf"), 1, 0.5]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


# ---- the definition ------------------------------------------------------------------------------------------------------

def test_definition_strict_less_nan_inf_and_wrap():
    r = eval_def.Record(1, 0, 4)
    assert math.isinf(r.best_val) and r.best_val > 0 and r.best_iter == -1 and r.count == 0
    got = [r.append([s], 10 * (i + 1)) for i, s in enumerate(SEQ)]
    #       3     2     2 (equal) nan    5      1     inf    1 (equal) 0.5
    assert got == [True, True, False, False, False, True, False, False, True]
    assert r.best_val == np.float32(0.5) and r.best_iter == 90 and r.count == 9 and r.flag == 1
    # ring of 4: evaluations 8 (slot 0), 5, 6, 7 (slots 1..3) are what is left
    assert r.ring_iter.tolist() == [[90, 1], [60, 1], [70, 0], [80, 0]]
    assert r.ring_val[:, 0].tolist() == [0.5, 1.0, float("inf"), 1.0]


def test_definition_nan_never_wins_and_inf_start():
    r = eval_def.Record(2, 1, 3)
    assert not r.append([0.0, float("nan")]) and r.best_iter == -1 and math.isinf(r.best_val)
    assert not r.append([0.0, float("inf")])            # +inf is not below the +inf start
    assert r.ring_iter[:2].tolist() == [[-1, 0], [-1, 0]]           # an absent iteration is -1
    assert r.append([7.0, 4.0], 2 ** 24 + 1) and r.best_iter == 2 ** 24 + 1 and r.best_val == 4.0
    assert not r.append([1.0, float("nan")], 5) and r.best_val == 4.0          # the select column decides, not column 0
    assert r.ring_iter[0].tolist() == [5, 0] and np.isnan(r.ring_val[0, 1])    # wrapped


def test_definition_select_column():
    a, b = eval_def.Record(4, 0, 4), eval_def.Record(4, 3, 4)
    for i, s in enumerate(SEQ):
        row = [s, 100.0 - i, -float(i), 9.0 - s if s == s else s]
        a.append(row, i)
        b.append(row, i)
    assert a.best_val == 0.5 and a.best_iter == 8
    assert b.best_iter == 6 and b.best_val == -np.inf   # column 3 = 9 - s: 6, 7, 7, nan, 4, 8, -inf, 8, 8.5
    assert b.ring_iter.tolist() == [[8, 0], [5, 0], [6, 1], [7, 0]]
    assert np.array_equal(a.ring_val, b.ring_val, equal_nan=True)


# ---- the entry points ----------------------------------------------------------------------------------------------------

def test_entry_points_declared_exported_bound(lib):
    txt = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("kg_eval_record", 2), ("kg_copy_if", 4)):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), "%s is not declared in kgan_hip.h" % name
        assert hasattr(ctypes.CDLL(_native.LIB_PATH), name)
        restype, argtypes = _native.EXPORTS[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
    assert "kg_eval.hip" in build.SOURCES
    assert lib.kg_abi_version() == 9
    assert callable(_native.eval_record) and callable(_native.copy_if)


def test_struct_sizes_match_header():
    for cname in ("KgEvalRecordArgs", "KgCopyJob"):
        abi_layout.assert_mirror(cname)
    consts = abi_layout.header_constants()
    assert [consts["KG_EVAL_MAX_SCORES"], consts["KG_COPY_IF_MAX_JOBS"]] == [_native.EVAL_MAX_SCORES, _native.COPY_IF_MAX_JOBS]
    assert _native.COPY_IF_MAX_JOBS >= 32


FIELDS = ("scores", "nscores", "select", "iter", "count", "ring_val", "ring_iter", "ring_len", "best_val", "best_iter", "flag")


@pytest.mark.parametrize("cls, size, offsets", [
    ("_EvalRecordArgs", 136, (0, 64, 68, 72, 80, 88, 96, 104, 112, 120, 128)),
    ("_EvalRecord2Args", 336, (0, 256, 260, 264, 272, 280, 288, 296, 304, 312, 320, 328)),
    ("_EvalRecord3Args", 592, (0, 512, 516, 520, 528, 536, 544, 552, 560, 568, 576, 584))])
def test_record_structs_keep_their_layout(cls, size, offsets):
    """the three structs come from one field list: the sizes and offsets of the three hand-written classes before it"""
    S = getattr(_native, cls)
    names = FIELDS + (("maximise",) if len(offsets) == 12 else ())
    assert issubclass(S, ctypes.Structure) and S.__name__ == cls and ctypes.sizeof(S) == size
    assert tuple(n for n, _ in S._fields_) == names and tuple(getattr(S, n).offset for n in names) == offsets
    types = dict(S._fields_)
    assert ctypes.sizeof(types["scores"]) == offsets[1] and types["scores"]._type_ is ctypes.c_void_p
    assert [types[n] for n in ("nscores", "select", "ring_len")] == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
    assert all(types[n] is ctypes.c_void_p for n in ("iter", "count", "ring_val", "ring_iter", "best_val", "best_iter", "flag"))
    assert types.get("maximise", ctypes.c_int32) is ctypes.c_int32


# ---- the sharing rule and the state normaliser ---------------------------------------------------------------------------

ORDER = ("prdc", "frechet", "classifier", "memorisation", "kinematics")


def _owners_by_the_four_chains(n):
    """the rule as it was written before ``round_owners``, family by family (``group``: the family has Samplers of its own)"""
    group = {"prdc": bool(n["prdc"])}
    owner = {"prdc": None}
    # frechet: a bool
    shared = bool(n["frechet"]) and n["prdc"] == n["frechet"]
    owner["frechet"] = "prdc" if shared else None
    group["frechet"] = bool(n["frechet"]) and not shared
    # classifier: if / elif over two names
    owner["classifier"] = None
    if n["classifier"]:
        if n["prdc"] == n["classifier"]:
            owner["classifier"] = "prdc"
        elif n["frechet"] == n["classifier"]:
            owner["classifier"] = "frechet"
    group["classifier"] = bool(n["classifier"]) and owner["classifier"] is None
    # memorisation, kinematics: for / else over the families before them
    for key, before in (("memorisation", ORDER[:3]), ("kinematics", ORDER[:4])):
        owner[key] = None
        if n[key]:
            for kind in before:
                if n[kind] == n[key] and group[kind]:      # (a round that is itself shared has no Samplers: its owner came first)
                    owner[key] = kind
                    break
        group[key] = bool(n[key]) and owner[key] is None
    return owner, group


def test_round_owners_is_the_rule_of_the_four_chains():
    import itertools
    cases = list(itertools.product((0, 3, 4), repeat=5))
    assert len(cases) == 243
    for case in cases:
        n = dict(zip(ORDER, case))
        got = evaluate.round_owners(n)
        want, group = _owners_by_the_four_chains(n)
        assert got == want and list(got) == list(ORDER), (n, got, want)
        for key, owner in got.items():
            if owner is not None:
                assert got[owner] is None and n[owner] == n[key] != 0 and ORDER.index(owner) < ORDER.index(key), (n, got)
            if n[key] == 0:
                assert owner is None and key not in got.values(), (n, got)
        assert {k for k in ORDER if n[k] and got[k] is None} == {k for k in ORDER if group[k]}      # who builds Samplers
    assert [f.key for f in evaluate.FAMILIES] == list(ORDER)


def test_plain_state_is_idempotent_and_keeps_what_differs():
    plain = evaluate.plain_state
    back = {"per_class": np.int64(8), "modes": ("pose", "motion"), "still_eps": np.float64(1e-3), "mode": "raw",
            "bones": np.array([[0, 1], [1, 2]], dtype=np.int32), "mirror": [(0, 1)], "none": None}
    once = plain(back)
    assert once == {"per_class": 8, "modes": ["pose", "motion"], "still_eps": 1e-3, "mode": "raw", "bones": [[0, 1], [1, 2]],
                    "mirror": [[0, 1]], "none": None}
    assert plain(once) == once and plain(plain(np.int64(8))) == 8 and type(plain(np.int64(8))) is int
    assert type(once["per_class"]) is int and type(once["still_eps"]) is float and type(once["bones"][0][0]) is int
    assert plain({"per_class": np.int64(8), "modes": ("pose", "motion")}) == {"per_class": 8, "modes": ["pose", "motion"]}
    assert plain({"still_eps": 2e-3}) != plain({"still_eps": 1e-3}) and plain({"mode": "raw"}) != plain({"mode": "features"})
    assert plain(None) is None and plain("pose") == "pose"


def _record_args(nscores=1, select=0, ring_len=4, null=None):
    a = _native._EvalRecordArgs()
    p = 0x1000
    for i in range(min(nscores, _native.EVAL_MAX_SCORES)):
        a.scores[i] = p
    a.nscores, a.select, a.ring_len = nscores, select, ring_len
    a.iter = a.count = a.ring_val = a.ring_iter = a.best_val = a.best_iter = a.flag = p
    if null:
        setattr(a, null, None)
    return a


def test_bad_arguments_are_rejected_without_gpu(lib):
    """every rejection happens on the host side of the C call, in front of the launch"""
    for kw, word in ((dict(nscores=0), b"nscores"), (dict(nscores=9), b"nscores"), (dict(nscores=2, select=2), b"select"),
                     (dict(select=-1), b"select"), (dict(ring_len=0), b"ring_len"), (dict(null="count"), b"null"),
                     (dict(null="flag"), b"null"), (dict(null="best_val"), b"null")):
        assert lib.kg_eval_record(ctypes.byref(_record_args(**kw)), None) < 0, kw
        assert b"kg_eval_record" in lib.kg_last_error() and word in lib.kg_last_error(), (kw, lib.kg_last_error())
    assert lib.kg_eval_record(None, None) < 0
    J = _native._CopyJob

    def jobs(*t):
        arr = (J * len(t))()
        for i, (s, d, n) in enumerate(t):
            arr[i].src, arr[i].dst, arr[i].nwords = s, d, n
        return arr
    flag = 0x1000
    for arr, n, word in ((jobs((0x2000, 0x2010, 5)), 1, b"overlap"),            # dst starts inside src
                         (jobs((0x2010, 0x2000, 5)), 1, b"overlap"),            # src starts inside dst
                         (jobs((0x2000, 0x2000, 1)), 1, b"overlap"),
                         (jobs((0x2000, 0x3000, 4), (0x4000, 0x4004, 2)), 2, b"overlap"),
                         (jobs((None, 0x3000, 4)), 1, b"null"), (jobs((0x2000, None, 4)), 1, b"null"),
                         (jobs((0x2000, 0x3000, 0)), 1, b"nwords"), (jobs((0x2002, 0x3000, 4)), 1, b"aligned"),
                         (jobs((0x2000, 0x3000, 4)), 0, b"njobs"), (jobs((0x2000, 0x3000, 4)), 33, b"njobs")):
        assert lib.kg_copy_if(flag, arr, n, None) < 0, word
        assert b"kg_copy_if" in lib.kg_last_error() and word in lib.kg_last_error(), (word, lib.kg_last_error())
    assert lib.kg_copy_if(None, jobs((0x2000, 0x3000, 4)), 1, None) < 0
    assert lib.kg_copy_if(flag, None, 1, None) < 0


# ---- the real side -------------------------------------------------------------------------------------------------------

def test_pair_rows_against_a_hand_made_example():
    labels = [2, 0, 1, 1, 0, 2, 2, 0, 1]
    # class 0: 1, 4, 7; class 1: 2, 3, 8; class 2: 0, 5, 6 -> row j*3 + c
    assert evaluate.pair_rows(labels, 3, 2).tolist() == [1, 2, 0, 4, 3, 5] == eval_def.pair_rows(labels, 3, 2)
    assert evaluate.pair_rows(labels, 3, 3).tolist() == [1, 2, 0, 4, 3, 5, 7, 8, 6]
    assert evaluate.pair_rows(labels, 3, 1).tolist() == [1, 2, 0]
    with pytest.raises(ValueError):
        evaluate.pair_rows(labels, 3, 4)
    with pytest.raises(ValueError):
        evaluate.pair_rows(labels, 4, 1)
    # the output of select_reference_samples (labels = repeat(arange(K), pairs)): sample c*pairs + j -> row j*K + c
    K, pairs = 4, 3
    rows = evaluate.pair_rows(np.repeat(np.arange(K), pairs), K, pairs)
    assert rows.tolist() == [c * pairs + j for j in range(pairs) for c in range(K)]
    rng = np.random.RandomState(0)
    lab = rng.randint(0, 5, 60)
    assert evaluate.pair_rows(lab, 5, 4).tolist() == eval_def.pair_rows(lab.tolist(), 5, 4)


def test_selection_needs_two_samples_of_every_class(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    dp, lp = train_def.synthetic_dataset(str(a), 64, 2, 40, 16, 10, "h36m", seed=4)
    f = Feeder(dp, lp, dataset="h36m")
    lab = np.asarray(f.label)
    assert [int((lab[1:] == c).sum()) for c in range(10)] == [5, 2, 9, 6, 6, 8, 6, 8, 6, 7]
    data, labels, index = metrics.select_reference_samples(f, np.arange(10), 32, per_class=2)
    assert data.shape == (20, 2, 32, 16) and labels.tolist() == np.repeat(np.arange(10), 2).tolist()
    rows = evaluate.pair_rows(labels, 10, 2)
    assert [int(lab[index[r]]) for r in rows] == list(range(10)) * 2
    with pytest.raises(ValueError):
        metrics.select_reference_samples(f, np.arange(10), 32, per_class=3)
    dp, lp = train_def.synthetic_dataset(str(b), 40, 2, 40, 16, 10, "h36m", seed=4)
    f40 = Feeder(dp, lp, dataset="h36m")
    assert min(int((np.asarray(f40.label)[1:] == c).sum()) for c in range(10)) == 1
    with pytest.raises(ValueError, match="select_reference_samples"):
        metrics.select_reference_samples(f40, np.arange(10), 32, per_class=2)


# ---- host helpers --------------------------------------------------------------------------------------------------------

def test_csv_writer_round_trips_bit_for_bit(tmp_path):
    rec = {"names": ["live/avg", "live/joint"], "iteration": np.array([2, 4, 2 ** 24 + 1], dtype=np.int64),
           "scores": np.array([[0.1, 3.0], [np.nan, np.inf], [1e-30, 16777217.0]], dtype=np.float32),
           "improved": np.array([True, False, True])}
    path = str(tmp_path / "metrics.csv")
    evaluate.write_metrics_csv(path, rec)
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["iteration", "live/avg", "live/joint", "improved"] and len(rows) == 4
    assert [int(r[0]) for r in rows[1:]] == [2, 4, 2 ** 24 + 1] and [int(r[3]) for r in rows[1:]] == [1, 0, 1]
    back = np.array([[float(v) for v in r[1:3]] for r in rows[1:]], dtype=np.float32)
    assert np.array_equal(back.view(np.uint32), rec["scores"].view(np.uint32))
    evaluate.write_metrics_csv(path, {"names": ["a/avg"], "iteration": np.zeros(0, np.int64), "scores": np.zeros((0, 1), np.float32),
                                      "improved": np.zeros(0, bool)})
    assert list(csv.reader(open(path))) == [["iteration", "a/avg", "improved"]]


def test_default_of_eval_select():
    assert evaluate.default_select(["live", "ema"], ("avg", "joint")) == "ema/avg"
    assert evaluate.default_select(["live"], ("avg", "joint")) == "live/avg"
    assert evaluate.default_select(["live", "ema"], ("joint",)) == "ema/joint"
    assert evaluate.default_select(["g"], ("joint", "avg")) == "g/avg"


def test_train_command_flags():
    spec = importlib.util.spec_from_file_location("kg_tools_train", os.path.join(ROOT, "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opt = mod.parse_args(["--data_path", "d", "--label_path", "l"])
    assert opt.eval_interval == 0 and opt.eval_pairs == 10 and opt.eval_select is None and opt.eval_trunc is None
    assert opt.eval_trunc_mode == "-" and opt.eval_data_path is None and opt.eval_label_path is None
    opt = mod.parse_args(["--data_path", "d", "--label_path", "l", "--eval_interval", "100", "--eval_pairs", "2", "--eval_select",
                          "live/joint", "--eval_trunc", "0.9", "--eval_trunc_mode", "w", "--eval_data_path", "e", "--eval_label_path", "f"])
    assert (opt.eval_interval, opt.eval_pairs, opt.eval_select, opt.eval_trunc, opt.eval_trunc_mode, opt.eval_data_path,
            opt.eval_label_path) == (100, 2, "live/joint", 0.9, "w", "e", "f")
