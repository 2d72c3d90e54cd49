"""Precision / recall / density / coverage without a GPU: the float64 definition (tests/prdc_def.py) on a hand-worked
example, the argument checks of kg_prdc and metrics.prdc, the workspace size and the ctypes mirror of KgPrdcArgs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd import metrics

import abi_layout
import prdc_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def test_header_declares_and_library_exports(lib):
    header = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    for sym in ("kg_prdc_workspace_bytes", "kg_prdc"):
        assert "%s(const KgPrdcArgs* a" % sym in header
        assert getattr(lib, sym) is not None
    assert "#define KG_PRDC_MAX_K 32" in header and _native.PRDC_MAX_K == 32
    assert "#define KG_PRDC_MAX_POINTS %d" % _native.PRDC_MAX_POINTS in header and _native.PRDC_MAX_POINTS >= 4096


def test_abi_version_unchanged(lib):
    assert lib.kg_abi_version() == 9


def test_prdc_struct_matches_header():
    abi_layout.assert_mirror("KgPrdcArgs")


def _valid_args():
    a = _native._PrdcArgs()
    a.real, a.fake = 0x1000, 0x2000
    a.r_sc, a.r_sp, a.r_so = 100 * 4800, 4800, 0
    a.f_sc, a.f_sp, a.f_so = 100 * 4800, 4800, 0
    a.n, a.m, a.d_outer, a.d_inner, a.classes, a.k = 100, 90, 3, 1600, 60, 5
    a.counts, a.values, a.ws = 0x3000, 0x4000, 0x5000
    return a


@pytest.mark.parametrize("field,value,needle", [
    ("real", None, b"null pointer real"), ("fake", None, b"null pointer fake"), ("counts", None, b"null pointer counts"),
    ("values", None, b"null pointer values"), ("ws", None, b"null pointer ws"),
    ("n", 0, b"n=0"), ("m", 0, b"m=0"), ("m", -3, b"m=-3"), ("classes", 0, b"classes=0"), ("d_outer", 0, b"d_outer=0"),
    ("d_inner", 0, b"d_inner=0"), ("k", 0, b"k=0"), ("k", 33, b"k=33"), ("m", 4, b"k=5 > min(n=100, m=4) - 1"),
    ("n", 5, b"k=5 > min(n=5, m=90) - 1"), ("ws_bytes", 64, b"ws_bytes=64"),
    ("n", _native.PRDC_MAX_POINTS + 1, b"n=%d above the cap" % (_native.PRDC_MAX_POINTS + 1)),
    ("m", _native.PRDC_MAX_POINTS + 1, b"m=%d above the cap" % (_native.PRDC_MAX_POINTS + 1))])
def test_kg_prdc_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _valid_args()
    need = lib.kg_prdc_workspace_bytes(ctypes.byref(a))
    assert need == 8 * 60 * (100 + 90)
    a.ws_bytes = need
    setattr(a, field, value)
    if field in ("n", "m", "classes", "d_outer", "d_inner", "k"):
        assert lib.kg_prdc_workspace_bytes(ctypes.byref(a)) < 0
        assert needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_prdc(ctypes.byref(a), None) < 0
    assert needle in lib.kg_last_error(), lib.kg_last_error()


def test_limits_are_valid(lib):
    """k = min(n, m) - 1, k = 32 and the largest supported set pass the shape checks"""
    for n, m, k in ((20, 20, 19), (40, 33, 32), (_native.PRDC_MAX_POINTS, 4096, 5)):
        assert _native.prdc_workspace_bytes(n, m, 1, 7, 1, k) == 8 * (n + m)
    with pytest.raises(RuntimeError, match="k=20"):
        _native.prdc_workspace_bytes(20, 20, 1, 7, 1, 20)


def test_launches_of_2_to_24_workgroups_are_rejected(lib):
    """a tile launch stays below 2^24 workgroups of 256 threads (the runtime refuses 2^32 threads in x): 63 classes of
    32768 x 32768 points are 63 * 512 * 512 cross tiles of 64 and pass, 64 classes are 2^24 and are refused by name"""
    big = _native.PRDC_MAX_POINTS
    assert big == 32768
    assert _native.prdc_workspace_bytes(big, big, 1, 7, 63, 5) == 8 * 63 * 2 * big
    with pytest.raises(RuntimeError, match=r"classes=64 .* 16777216 workgroups"):
        _native.prdc_workspace_bytes(big, big, 1, 7, 64, 5)


def test_workspace_is_linear_and_monotone(lib):
    """no n x m term: monotone in n, m and classes, below 64 classes (n + m) bytes (there are no tile partials)"""
    f = lambda n, m, c: _native.prdc_workspace_bytes(n, m, 3, 1600, c, 5)      # noqa: E731
    sizes = (6, 33, 100, 1000, 4096)
    for c in (1, 7, 60):
        for n in sizes:
            for m in sizes:
                b = f(n, m, c)
                assert 0 < b <= 64 * c * (n + m)
                assert f(n + 1, m, c) >= b and f(n, m + 1, c) >= b and f(n, m, c + 1) >= b
    assert f(4096, 4096, 1) < 4096 * 4096


def test_definition_hand_worked_example():
    """1-D, 4 + 4 points, k = 1.  R = 0, 0, 2, 5 (a duplicate: radius 0), F = 1, 3, 4, 10.
    rho_R = 0, 0, 4, 9; rho_F = 4, 1, 1, 36.  d2 rows: [1 9 16 100] twice, [1 1 4 64], [16 4 1 25].
    P (<= rho_R, rows): none, none, {0, 1, 2} (4 <= 4: a tie), {1, 2};  Q (<= rho_F, columns): {0, 1, 2}, {2} (1 <= 1: a
    tie), {3}, {3}."""
    R = torch.tensor([[0.0], [0.0], [2.0], [5.0]])
    F = torch.tensor([[1.0], [3.0], [4.0], [10.0]])
    out = prdc_def.one_class(R, F, 1)
    assert out["radii_real"].tolist() == [0.0, 0.0, 4.0, 9.0]
    assert out["radii_fake"].tolist() == [4.0, 1.0, 1.0, 36.0]
    assert out["fake_hits"].tolist() == [1, 2, 2, 0]
    assert out["real_flags"].tolist() == [1, 1, 3, 3]
    assert out["counts"].tolist() == [3, 4, 5, 2]
    v = prdc_def.values_of(out["counts"][None], 4, 4, 1)[0].tolist()
    assert v == [0.75, 1.0, 1.25, 0.5]
    # a strict '<' anywhere, or leaving the duplicate out by value, changes the counts
    out2 = prdc_def.one_class(R, F, 2)
    assert out2["radii_real"].tolist() == [4.0, 4.0, 4.0, 25.0]


def test_bracket_contains_exact_and_is_narrow_on_the_generator():
    """the generator's data in float64: lo <= exact <= hi, and the bracket is narrow at a shape of the verified list"""
    R, F = prdc_def.make_data(0, 2, 100, 100, 75)
    ref = prdc_def.reference(R, F, 5, prdc_def.tau(75))
    assert (ref["counts_lo"] <= ref["counts"]).all() and (ref["counts"] <= ref["counts_hi"]).all()
    ok, width = prdc_def.bracket_is_narrow(ref)
    assert ok, width
    c = ref["counts"][0].tolist()
    assert c == [100, 72, 543, 83]              # recall and coverage mid-range, precision != recall (the collapsed quarter)


def test_metrics_prdc_argument_errors_without_gpu():
    x = torch.zeros(12, 2, 4, 3)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.prdc(x, torch.zeros(12, 2, 5, 3))
    with pytest.raises(ValueError, match=r"\(N, C, T, V\)"):
        metrics.prdc(x[0], x)
    ragged = [0] * 5 + [1] * 7
    with pytest.raises(ValueError, match="class 1 has 7 real samples"):
        metrics.prdc(x, x, labels_gen=[0] * 6 + [1] * 6, labels_real=ragged)
    with pytest.raises(ValueError, match="class 0 has 5 fake samples, per_class=6"):
        metrics.prdc(x, x, labels_gen=ragged, labels_real=[0] * 6 + [1] * 6, per_class=6)
    with pytest.raises(ValueError, match="class 2 has 0 real samples"):
        metrics.prdc(x, x, labels_gen=np.eye(3)[[0, 1, 2] * 4], labels_real=[0, 1] * 6, per_class=4)
    with pytest.raises(ValueError, match="11 labels_gen for 12 samples"):
        metrics.prdc(x, x, labels_gen=[0] * 11)
    with pytest.raises(ValueError, match="k=12 outside"):
        metrics.prdc(x, x, k=12)
    assert metrics.PRDC_NAMES == ("precision", "recall", "density", "coverage")
