"""kg_nn_sets / kg_nn_scores and what is built on them, without a GPU: the header and the exports, the ctypes
mirrors, every argument check, the workspace formula and the plan rule (the sets count as row tiles), the definition of the
score words on a hand-worked example, the argument errors of metrics.memorisation_features / memorisation_sets, and the
Evaluator's names and senses for the two new columns."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd import metrics
from kinetic_gan_amd.evaluate import NO_SENSE, score_names, score_sense

import abi_layout
from nn_sets_def import nn_scores_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def test_header_declares_and_library_exports(lib):
    header = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    for sym, struct in (("kg_nn_sets_workspace_bytes", "KgNnSetsArgs"), ("kg_nn_sets", "KgNnSetsArgs"),
                        ("kg_nn_scores", "KgNnScoresArgs")):
        assert "%s(const %s* a" % (sym, struct) in header
        assert getattr(lib, sym) is not None and sym in _native.EXPORTS
    assert "#define KG_NN_MAX_SETS 4" in header and _native.NN_MAX_SETS == 4
    assert "#define KG_NN_SCORES_MAX_CLASSES %d" % _native.NN_SCORES_MAX_CLASSES in header
    assert abi_layout.header_constants()["KG_NN_SCORES_MAX_CLASSES"] == _native.NN_SCORES_MAX_CLASSES


def test_abi_version_unchanged(lib):
    assert lib.kg_abi_version() == 9 and _native.ABI_VERSION == 9
    assert abi_layout.header_constants()["KG_ABI_VERSION"] == 9


@pytest.mark.parametrize("name", ["KgNnSetsArgs", "KgNnScoresArgs", "KgNnArgs"])
def test_structs_match_header(name):
    abi_layout.assert_mirror(name)


def _valid_sets(nsets=3):
    a = _native._NnSetsArgs()
    for g in range(nsets):
        a.query[g] = 0x1000 * (g + 1)
    a.nsets = nsets
    a.base = 0x9000
    a.q_sc, a.q_sp, a.q_so = 0, 4800, 0
    a.b_sc, a.b_sp, a.b_so = 0, 4800, 0
    a.Q, a.N, a.d_outer, a.d_inner, a.classes, a.k = 100, 90, 3, 1600, 2, 5
    a.tile, a.split = 32, 4
    a.idx, a.d2, a.ws = 0xa000, 0xb000, 0xc000
    return a


POINTERS = ("query0", "query2", "base", "idx", "d2", "ws", "ws_bytes")


@pytest.mark.parametrize("field,value,needle", [
    ("query0", None, b"null pointer query[0]"), ("query2", None, b"null pointer query[2]"), ("base", None, b"null pointer base"),
    ("idx", None, b"null pointer idx"), ("d2", None, b"null pointer d2"), ("ws", None, b"null pointer ws"),
    ("ws_bytes", 64, b"ws_bytes=64"),
    ("nsets", 0, b"nsets=0"), ("nsets", 5, b"nsets=5"), ("nsets", -1, b"nsets=-1"),
    ("Q", 0, b"Q=0"), ("N", 0, b"N=0"), ("N", -3, b"N=-3"), ("classes", 0, b"classes=0"), ("d_outer", 0, b"d_outer=0"),
    ("d_inner", 0, b"d_inner=0"), ("k", 0, b"k=0"), ("k", 33, b"k=33"), ("N", 4, b"k=5 > N=4"),
    ("tile", 16, b"tile=16"), ("tile", -1, b"tile=-1"), ("split", -1, b"split=-1"),
    ("split", _native.NN_MAX_SPLIT + 1, b"split=%d" % (_native.NN_MAX_SPLIT + 1)),
    ("Q", _native.NN_MAX_POINTS + 1, b"Q=%d above the cap" % (_native.NN_MAX_POINTS + 1)),
    ("N", _native.NN_MAX_POINTS + 1, b"N=%d above the cap" % (_native.NN_MAX_POINTS + 1))])
def test_kg_nn_sets_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _valid_sets()
    need = lib.kg_nn_sets_workspace_bytes(ctypes.byref(a))
    assert need == 3 * 2 * 100 * 4 * 5 * 8
    a.ws_bytes = need
    if field.startswith("query"):
        a.query[int(field[5:])] = None
    else:
        setattr(a, field, value)
    if field not in POINTERS:
        assert lib.kg_nn_sets_workspace_bytes(ctypes.byref(a)) < 0
        assert needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_nn_sets(ctypes.byref(a), None) < 0
    assert needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_last_error().startswith(b"kg_nn_sets")


def test_a_null_set_beyond_nsets_is_not_looked_at(lib):
    """query[g] for g >= nsets may hold anything; with k = N (no "self" to leave out) the shape passes"""
    a = _valid_sets(2)
    a.k = a.N = 7
    a.split = 0
    assert lib.kg_nn_sets_workspace_bytes(ctypes.byref(a)) > 0
    assert lib.kg_nn_sets(ctypes.byref(a), None) < 0 and b"ws_bytes=0" in lib.kg_last_error()     # the pointers passed


def test_grid_bounds_count_the_sets(lib):
    """search: nsets * classes * row tiles * split workgroups; merge: ceil(nsets * classes * Q / 4): both below 2^24"""
    big, f = _native.NN_MAX_POINTS, _native.nn_sets_workspace_bytes
    assert f(1, big, 100, 1, 7, 3, 1, tile=64, split=1) == 3 * big * 8
    assert f(3, big, 100, 1, 7, 1, 1, tile=64, split=1) == 3 * big * 8
    with pytest.raises(RuntimeError, match=r"nsets=4 x classes=1 x Q=16777216 x split=1 make 16777216 workgroups"):
        f(4, big, 100, 1, 7, 1, 1, tile=64, split=1)                # the merge launch
    with pytest.raises(RuntimeError, match=r"nsets=2 x classes=1 x Q=16777216 x split=32 make \d+ workgroups"):
        f(2, big, 100, 1, 7, 1, 1, tile=64, split=32)               # the search launch: 2 * 2^18 * 32
    assert f(2, big, 100, 1, 7, 1, 1, tile=64, split=16) == 2 * big * 16 * 8


def test_workspace_formula_and_the_plan_counts_sets_as_row_tiles(lib):
    f, one = _native.nn_sets_workspace_bytes, _native.nn_workspace_bytes
    for nsets, classes, Q, N, k, split in ((1, 1, 40, 40, 3, 3), (3, 3, 53, 37, 5, 5), (4, 2, 150, 300, 5, 2), (2, 1, 6000, 40000, 1, 6)):
        assert f(nsets, Q, N, 3, 1600, classes, k, split=split) == nsets * classes * Q * split * k * 8
        assert f(nsets, Q, N, 3, 1600, classes, k, tile=64, split=split) == f(nsets, Q, N, 3, 1600, classes, k, tile=32, split=split)
    auto = lambda g, Q, N, c=1, k=1, d=96: f(g, Q, N, 1, d, c, k) // (g * c * Q * k * 8)      # noqa: E731  (the plan's split)
    # one set is kg_nn's plan
    for Q, N, c in ((6000, 40000, 1), (70, 40000, 1), (40, 40, 1), (100, 100, 60), (1200, 4000, 1)):
        assert auto(1, Q, N, c) == one(Q, N, 1, 96, c, 1) // (c * Q * 8)
    # 94 row tiles of 64 want ceil(512 / 94) = 6 chunks -> 7 of 104 column tiles; two sets are 188 row tiles: 3 chunks wanted ->
    # 4 of 208 column tiles; four sets 376: 2 wanted -> 3 of 312
    assert auto(1, 6000, 40000) == 7 and auto(2, 6000, 40000) == 4 and auto(4, 6000, 40000) == 3
    assert auto(2, 6000, 40000) < auto(1, 6000, 40000)
    # the tile edge counts the sets too: Q = 900 is 15 row tiles of 64, x 32 chunks = 480 < 512 -> the 32-tile for one set (29
    # row tiles want 18 chunks: 21 of 6 column tiles); four sets are 1920 >= 512 -> the 64-tile, 60 row tiles want 9 chunks:
    # 9 of 7 column tiles (with the 32-tile it would be 116 row tiles and 5 chunks)
    assert auto(1, 900, 4000) == 21 and auto(4, 900, 4000) == 9


def _valid_scores():
    a = _native._NnScoresArgs()
    a.nsets, a.Q, a.N, a.n_classes, a.ld = 2, 10, 20, 4, 1
    a.idx, a.d2, a.query_labels, a.base_labels, a.base_loo = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.counts, a.counts_per_class, a.scores64, a.scores = 0x6000, None, 0x7000, 0x8000
    return a


@pytest.mark.parametrize("field,value,needle", [
    ("idx", None, b"null pointer idx"), ("d2", None, b"null pointer d2"), ("query_labels", None, b"null pointer query_labels"),
    ("base_labels", None, b"null pointer base_labels"), ("base_loo", None, b"null pointer base_loo"),
    ("counts", None, b"null pointer counts"), ("scores64", None, b"null pointer scores64"), ("scores", None, b"null pointer scores"),
    ("Q", 0, b"Q=0"), ("N", 0, b"N=0"), ("n_classes", 0, b"n_classes=0"), ("nsets", 0, b"nsets=0"), ("nsets", 5, b"nsets=5"),
    ("ld", 0, b"ld=0"),
    ("Q", _native.NN_MAX_POINTS + 1, b"Q=%d above the cap" % (_native.NN_MAX_POINTS + 1)),
    ("N", _native.NN_MAX_POINTS + 1, b"N=%d above the cap" % (_native.NN_MAX_POINTS + 1)),
    ("n_classes", _native.NN_SCORES_MAX_CLASSES + 1, b"n_classes=%d outside [1, %d]" % (
        _native.NN_SCORES_MAX_CLASSES + 1, _native.NN_SCORES_MAX_CLASSES))])
def test_kg_nn_scores_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _valid_scores()
    setattr(a, field, value)
    assert lib.kg_nn_scores(ctypes.byref(a), None) < 0
    assert needle in lib.kg_last_error() and lib.kg_last_error().startswith(b"kg_nn_scores"), lib.kg_last_error()


def test_scores_definition_hand_worked_example():
    """5 base points with leave-one-out distances 1, 4, 0.25, 9, 2 and labels 0 1 0 1 2; 4 queries labelled 0 1 2 0.
    set 0: neighbours 0 1 2 4 at d2 = 1 (== loo: authentic), 3.9999998 (one ulp below 4: a copy), 0.25 (==), 2.5
           -> authentic 3; labels 0 1 0 2 against 0 1 2 0 -> agreeing 2
    set 1: neighbours 3 3 3 3 at d2 = 0 -> authentic 0; labels 1 1 1 1 -> agreeing 1"""
    loo = np.array([1, 4, 0.25, 9, 2], dtype=np.float32)
    below = np.nextafter(np.float32(4), np.float32(0))
    assert below < np.float32(4) and repr(float(below)) == "3.999999761581421"
    idx = np.array([[0, 1, 2, 4], [3, 3, 3, 3]])
    d2 = np.array([[1, below, 0.25, 2.5], [0, 0, 0, 0]], dtype=np.float32)
    out = nn_scores_def(idx, d2, [0, 1, 2, 0], [0, 1, 0, 1, 2], loo, 3)
    assert out["counts"].tolist() == [[3, 2], [0, 1]] and out["counts"].dtype == np.int64
    assert out["counts_per_class"].tolist() == [[[2, 1], [0, 1], [1, 0]], [[0, 0], [0, 1], [0, 0]]]
    assert out["scores64"].tolist() == [[0.75, 0.5], [0.0, 0.25]] and out["scores"].dtype == np.float32
    assert out["scores"].tolist() == [[0.75, 0.5], [0.0, 0.25]]
    # the one rounding: 1 / 3 in float64, then to float32 - what metrics._share produces
    third = nn_scores_def(np.zeros((1, 3), int), np.array([[5, 0, 0]], np.float32), [0, 0, 0], [0], [1.0], 1)
    assert third["scores64"][0, 0] == 1 / 3 and third["scores"][0, 0] == np.float32(1 / 3)
    assert third["scores"][0, 0] == metrics._share(torch.tensor(1), 3).item()


def test_metrics_argument_errors_without_gpu():
    f = torch.zeros(12, 8)
    lab = np.arange(12) % 3
    with pytest.raises(ValueError, match=r"feat_gen is a \(n, d\) feature matrix"):
        metrics.memorisation_features(torch.zeros(12, 2, 3, 4), lab, f, lab)
    with pytest.raises(ValueError, match=r"feat_train is a \(n, d\) feature matrix"):
        metrics.memorisation_features(f, lab, torch.zeros(12), lab)
    with pytest.raises(ValueError, match="labels_train is needed"):
        metrics.memorisation_features(f, lab, f, None)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.memorisation_features(f, lab, torch.zeros(12, 7), lab)
    with pytest.raises(ValueError, match="11 labels_gen for 12 samples"):
        metrics.memorisation_features(f, lab[:11], f, lab)
    with pytest.raises(ValueError, match="labels_heldout is needed"):
        metrics.memorisation_features(f, lab, f, lab, feat_heldout=f)
    with pytest.raises(ValueError, match="at least 2 training samples"):
        metrics.memorisation_features(f, lab, f[:1], lab[:1])
    with pytest.raises(ValueError, match=r"train_loo must be the \(12,\) fp32"):
        metrics.memorisation_features(f, lab, f, lab, train_loo=torch.zeros(11))
    x = torch.zeros(12, 2, 3, 4)
    for bad in ([], [x] * 5, x):
        with pytest.raises(ValueError, match="a list of 1 to 4"):
            metrics.memorisation_sets(bad, lab, x, lab)
    with pytest.raises(ValueError, match="the sets differ in shape"):
        metrics.memorisation_sets([x, x[:11]], lab, x, lab)
    with pytest.raises(ValueError, match="labels_train is needed"):
        metrics.memorisation_sets([x], lab, x)
    with pytest.raises(ValueError, match="labels is needed"):
        metrics.memorisation_sets([x], None, x, lab)
    with pytest.raises(ValueError, match="set 0 samples .* and train samples .* differ in shape"):
        metrics.memorisation_sets([x, x], lab, torch.zeros(12, 2, 3, 5), lab)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.memorisation_sets([f], lab, torch.zeros(12, 7), lab)
    with pytest.raises(ValueError, match="11 labels for 12 samples"):
        metrics.memorisation_sets([x], lab[:11], x, lab)
    with pytest.raises(ValueError, match="at least 2 training samples"):
        metrics.memorisation_sets([x], lab, x[:1], lab[:1])
    with pytest.raises(ValueError, match=r"train_loo must be the \(12,\) fp32"):
        metrics.memorisation_sets([x], lab, x, lab, train_loo=torch.zeros(12, dtype=torch.float64))


def test_score_names_and_senses():
    assert metrics.MEMORISATION_NAMES == ("authenticity", "label_agreement")
    plain = score_names(["live", "ema"], ["avg", "joint"], prdc=True, frechet=("pose", "motion"), classifier=True)
    names = score_names(["live", "ema"], ["avg", "joint"], prdc=True, frechet=("pose", "motion"), classifier=True, memorisation=True)
    assert names[:len(plain)] == plain and len(plain) == 24
    assert names[24:] == ["live/authenticity", "live/label_agreement", "ema/authenticity", "ema/label_agreement"]
    assert len(names) == 28 <= _native.EVAL2_MAX_SCORES
    assert score_names(["g"], ["avg"], memorisation=True) == ["g/avg", "g/authenticity", "g/label_agreement"]
    assert score_names(["g"], ["avg"]) == ["g/avg"]
    assert score_sense("ema/label_agreement") == "max" and "authenticity" in NO_SENSE
    with pytest.raises(ValueError, match="closer"):
        score_sense("live/authenticity")
    assert score_sense("live/avg") == "min" and score_sense("live/accuracy") == "max"
