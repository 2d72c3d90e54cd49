"""kg_nn_gram without a GPU: exports and struct layout against the header, every rejection with the field named,
the workspace formula with the automatic cand, and the argument errors of metrics' ``method=``."""
import ctypes
import os

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd import metrics

import abi_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def test_header_declares_and_library_exports(lib):
    header = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    for sym in ("kg_nn_gram_workspace_bytes", "kg_nn_gram", "kg_nn_norms"):
        assert "%s(const KgNnGramArgs* a" % sym in header
        assert getattr(lib, sym) is not None and sym in _native.EXPORTS
    assert "#define KG_NN_NORM_PARTS 64" in header and _native.NN_NORM_PARTS == 64
    assert "kg_nn_gram.hip" in build.SOURCES
    assert lib.kg_abi_version() == 9            # additive


def test_struct_matches_header():
    abi_layout.assert_mirror("KgNnGramArgs")


def _valid_args():
    a = _native._NnGramArgs()
    a.query[0], a.base = 0x1000, 0x2000
    a.nsets = 1
    a.q_sc, a.q_sp, a.q_so = 0, 4800, 0
    a.b_sc, a.b_sp, a.b_so = 0, 4800, 0
    a.Q, a.N, a.d_outer, a.d_inner, a.classes, a.k = 100, 90, 3, 1600, 2, 5
    a.tile, a.split = 32, 4
    a.b_norms, a.b_norm_parts = 0x6000, 0x7000
    a.idx, a.d2, a.stats, a.ws = 0x3000, 0x4000, 0x8000, 0x5000
    return a


POINTERS = ("query", "base", "idx", "d2", "ws", "ws_bytes", "b_norms", "b_norm_parts", "stats")


@pytest.mark.parametrize("field,value,needle", [
    ("query", None, b"null pointer query[0]"), ("base", None, b"null pointer base"), ("idx", None, b"null pointer idx"),
    ("d2", None, b"null pointer d2"), ("ws", None, b"null pointer ws"), ("b_norms", None, b"null pointer b_norms"),
    ("b_norm_parts", None, b"null pointer b_norm_parts"), ("stats", None, b"null pointer stats"),
    ("nsets", 0, b"nsets=0"), ("nsets", 5, b"nsets=5"),
    ("Q", 0, b"Q=0"), ("N", 0, b"N=0"), ("N", -3, b"N=-3"), ("classes", 0, b"classes=0"), ("d_outer", 0, b"d_outer=0"),
    ("d_inner", 0, b"d_inner=0"), ("k", 0, b"k=0"), ("k", 33, b"k=33"), ("N", 4, b"k=5 > N=4"),
    ("k", 32, b"k=32 leaves no cand"), ("cand", 5, b"cand=5"), ("cand", 3, b"cand=3"), ("cand", 33, b"cand=33"), ("cand", -1, b"cand=-1"),
    ("tile", 16, b"tile=16"), ("split", -1, b"split=-1"),
    ("split", _native.NN_MAX_SPLIT + 1, b"split=%d" % (_native.NN_MAX_SPLIT + 1)),
    ("ws_bytes", 64, b"ws_bytes=64"),
    ("Q", _native.NN_MAX_POINTS + 1, b"Q=%d above the cap" % (_native.NN_MAX_POINTS + 1)),
    ("N", _native.NN_MAX_POINTS + 1, b"N=%d above the cap" % (_native.NN_MAX_POINTS + 1))])
def test_kg_nn_gram_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _valid_args()
    need = lib.kg_nn_gram_workspace_bytes(ctypes.byref(a))
    assert need == 2 * (100 * (8 * 13 * 5 + 8) + 4)
    a.ws_bytes = need
    if field == "query":
        a.query[0] = None
    else:
        setattr(a, field, value)
    if field not in POINTERS:
        assert lib.kg_nn_gram_workspace_bytes(ctypes.byref(a)) < 0
        assert needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_nn_gram(ctypes.byref(a), None) < 0
    assert needle in lib.kg_last_error(), lib.kg_last_error()


def test_second_query_set_and_exclude_self_rules(lib):
    a = _valid_args()
    a.ws_bytes = 1 << 30
    a.nsets = 2
    assert lib.kg_nn_gram(ctypes.byref(a), None) < 0 and b"null pointer query[1]" in lib.kg_last_error()
    a.exclude_self = 1
    assert lib.kg_nn_gram_workspace_bytes(ctypes.byref(a)) < 0 and b"exclude_self=1 needs nsets=2 to be 1" in lib.kg_last_error()
    f = _native.nn_gram_workspace_bytes
    with pytest.raises(RuntimeError, match=r"k=21 > N=21 - 1 neighbours \(exclude_self=1\)"):
        f(1, 21, 21, 1, 7, 1, 21, exclude_self=True)
    assert f(1, 21, 21, 1, 7, 1, 20, exclude_self=True, split=1) == 21 * (8 * 32 * 2 + 8) + 4


@pytest.mark.parametrize("field,value,needle", [
    ("base", None, b"null pointer base"), ("N", 0, b"N=0"), ("classes", 0, b"classes=0"), ("d_outer", 0, b"d_outer=0"),
    ("d_inner", -1, b"d_inner=-1"), ("N", _native.NN_MAX_POINTS + 1, b"above the cap")])
def test_kg_nn_norms_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _valid_args()
    setattr(a, field, value)
    assert lib.kg_nn_norms(ctypes.byref(a), 0x1000, 0x2000, None) < 0
    assert needle in lib.kg_last_error(), lib.kg_last_error()
    a = _valid_args()
    assert lib.kg_nn_norms(ctypes.byref(a), None, 0x2000, None) < 0 and b"null pointer norms" in lib.kg_last_error()
    assert lib.kg_nn_norms(ctypes.byref(a), 0x1000, None, None) < 0 and b"null pointer parts" in lib.kg_last_error()


def test_workspace_formula_and_automatic_cand(lib):
    """nsets * classes * (Q * (8 * cand * (split + 1) + 8) + 4): the chunk lists and the merged candidates (cand (key, j) each),
    a flag and a list entry per row, a list length per (set, class); cand = min(32, max(k + 8, 2 k)); the plan is kg_nn_sets'"""
    f = _native.nn_gram_workspace_bytes
    for nsets, classes, Q, N, k, split, cand in ((1, 1, 40, 40, 3, 3, 11), (2, 3, 53, 37, 5, 5, 13), (4, 2, 150, 300, 10, 2, 20),
                                                 (1, 1, 600, 4000, 20, 6, 32), (1, 1, 20, 33, 31, 4, 32)):
        want = nsets * classes * (Q * (8 * cand * (split + 1) + 8) + 4)
        assert f(nsets, Q, N, 3, 1600, classes, k, split=split) == want
        assert f(nsets, Q, N, 3, 1600, classes, k, split=split, tile=64) == want
        assert f(nsets, Q, N, 3, 1600, classes, k, split=split, cand=cand) == want
    assert f(1, 40, 40, 1, 7, 1, 3, split=1, cand=4) == 40 * (8 * 4 * 2 + 8) + 4
    # the automatic split is that of kg_nn_sets on the same shape
    for nsets, Q, N in ((1, 6000, 40000), (2, 6000, 40000), (1, 70, 40000), (1, 40000, 40000)):
        split = _native.nn_sets_workspace_bytes(nsets, Q, N, 1, 75, 1, 1) // (nsets * Q * 8)
        assert f(nsets, Q, N, 1, 75, 1, 1) == nsets * (Q * (8 * 9 * (split + 1) + 8) + 4)


def test_metrics_argument_errors_without_gpu():
    x = torch.zeros(12, 2, 4, 3)
    lab = [0, 1] * 6
    for call in (lambda m: metrics.nearest(x, x, method=m), lambda m: metrics.memorisation(x, lab, x, lab, method=m),
                 lambda m: metrics.memorisation_sets([x], lab, x, lab, method=m), lambda m: metrics.nn_two_sample(x, x, method=m),
                 lambda m: metrics.memorisation_features(x.reshape(12, -1), lab, x.reshape(12, -1), lab, method=m)):
        with pytest.raises(ValueError, match="method='cdist' is none of 'exact', 'gram'"):
            call("cdist")
    assert metrics.NN_METHODS == ("exact", "gram")
    big = torch.zeros(40, 1, 1, 2)
    with pytest.raises(ValueError, match="k=32 must be below 32"):
        metrics.nearest(big, big, k=32, method="gram")
    with pytest.raises(ValueError, match="k=33 outside"):
        metrics.nearest(big, big, k=33, method="gram")
    with pytest.raises(ValueError, match="differ in shape"):       # the checks of the exact path come first, unchanged
        metrics.nearest(x, torch.zeros(12, 2, 5, 3), method="gram")
