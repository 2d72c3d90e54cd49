"""Kinematic plausibility scores without a GPU: the float64 definition's closed forms (tests/kin_def.py), the W1 hand values,
the mirror tables of graph.py derived again from joint-level pairs, exports and struct layout, every rejection of kg_kin_desc /
kg_kin_scores (none of them reaches the GPU) and the argument errors of metrics.kinematics."""
import ctypes

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build, metrics
from kinetic_gan_amd.graph import Graph_h36m, graph_ntu

import abi_layout
import kin_def


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


int_skeleton = kin_def.int_skeleton


# ---- closed forms of the definition ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ntu", "h36m"])
def test_rigid_translation_mirrored_constant_velocity(name):
    # T = 8: the mean of 8 equal lengths is exact in every tree of pairs (a sum of 9 equal irrational lengths need not be)
    x, bones, mirror = int_skeleton(name, 8)
    x = x + (np.arange(8, dtype=np.float32) * 3)[None, :, None]          # a rigid integer translation, constant velocity
    d, degen, _ = kin_def.descriptors64(x, bones, mirror)
    assert not degen
    assert d[0] == 0.0                                                   # bone_cv
    assert d[1] == 0.0                                                   # asymmetry: a mirrored skeleton
    assert d[3] == 0.0 and d[4] == 0.0                                   # accel, jerk
    s = kin_def.lengths(x, bones).mean()
    C = x.shape[0]
    assert d[2] == pytest.approx(np.sqrt(C * 9.0) / s, rel=1e-14) and d[5] == 0.0


def test_asymmetric_skeleton_has_asymmetry():
    x, bones, mirror = int_skeleton("ntu", 4)
    x[:, :, 7] += 5                                                      # one hand further out: two bones change
    assert kin_def.descriptors64(x, bones, mirror)[0][1] > 0


@pytest.mark.parametrize("name", ["ntu", "h36m"])
def test_frozen_and_all_zero(name):
    x, bones, mirror = int_skeleton(name, 6)
    d, degen, count = kin_def.descriptors64(x, bones, mirror)
    assert not degen and d[5] == 1.0 and d[2] == 0.0 and count == 5 * x.shape[2]
    d, degen, _ = kin_def.descriptors64(np.zeros_like(x), bones, mirror)
    assert degen and np.array_equal(d, np.zeros(6))
    out = kin_def.descriptors(np.stack([x, np.zeros_like(x)])[None], bones, mirror)
    assert out["degenerate"].tolist() == [1] and out["nonfinite"].tolist() == [0]


def test_no_mirror_pairs_gives_zero_asymmetry():
    x = kin_def.make_data(0, 1, 1, 3, 8, 25)[0, 0]
    assert kin_def.descriptors64(x, kin_def.NTU_BONES, [])[0][1] == 0.0


def test_descriptors_are_invariant_under_scale_and_shift():
    """x * scale + shift in float64 before the one cast: the descriptors move only by roundoff"""
    a = kin_def.make_data(3, 1, 2, 3, 16, 25)
    b = kin_def.make_data(3, 1, 2, 3, 16, 25, scale=0.25, shift=-0.5)
    C, V, bones, mirror = kin_def.skeleton("ntu")
    da, db = kin_def.descriptors(a, bones, mirror), kin_def.descriptors(b, bones, mirror)
    assert np.allclose(da["d64"], db["d64"], rtol=1e-3, atol=0)


def test_test_data_is_well_conditioned():
    """what the GPU test asserts again before reading the kernel: bone_cv >= 1e-3 and no step near the threshold"""
    for name, T in (("ntu", 4), ("ntu", 64), ("h36m", 5)):
        C, V, bones, mirror = kin_def.skeleton(name)
        x = kin_def.make_data(1, 2, 5, C, T, V)
        ref = kin_def.descriptors(x, bones, mirror)
        assert ref["d64"][..., 0].min() >= 1e-3
        for k in range(2):
            for i in range(5):
                assert kin_def.threshold_margin(x[k, i], bones) >= 1e-6
                err = kin_def.eval_error(x[k, i], bones, mirror, ref["d64"][k, i])
                assert (err[:5] <= 2.0 ** -30).all(), err


# ---- W1 ---------------------------------------------------------------------------------------------------------------------

def test_w1_hand_values():
    assert kin_def.w1([0, 1], [0, 0.5, 1]) == 1.0 / 6.0
    rng = np.random.RandomState(0)
    a = rng.normal(size=40).astype(np.float32)
    assert kin_def.w1(a, a + np.float32(0.5)) == pytest.approx(0.5, rel=1e-6)
    b = (np.arange(16) // 2).astype(np.float32)                          # 0 0 1 1 2 2 ..
    assert kin_def.w1(b, b + 0.5) == 0.5
    c = np.array([1, 1, 2, 3, 3, 3, 5, -0.0, 0.0, 7], dtype=np.float32)
    assert kin_def.w1(c, rng.permutation(c)) == 0.0                      # two permutations of one multiset with ties
    assert np.isnan(kin_def.w1([0, np.inf], [1, 2])) and np.isnan(kin_def.w1([0, 1], [np.nan]))


def test_w1_against_sorted_quantile_form():
    """n == m: W1 = mean |sorted real - sorted fake|, an independent formula"""
    rng = np.random.RandomState(5)
    a, b = rng.normal(size=50).astype(np.float32), rng.normal(0.3, 2.0, size=50).astype(np.float32)
    want = np.abs(np.sort(a).astype(np.float64) - np.sort(b).astype(np.float64)).mean()
    assert kin_def.w1(a, b) == pytest.approx(want, rel=1e-12)


def test_w1_does_not_depend_on_the_order_of_ties_bit_for_bit():
    rng = np.random.RandomState(1)
    real = rng.randint(0, 6, size=37).astype(np.float32) / 4
    fake = rng.randint(0, 6, size=50).astype(np.float32) / 4
    base = kin_def.w1(real, fake)
    assert base > 0
    for _ in range(5):
        got = kin_def.w1(rng.permutation(real), rng.permutation(fake))
        assert np.float64(got).view(np.int64) == np.float64(base).view(np.int64)


def test_tree_sum_shape():
    assert kin_def.tree_sum([1.0]) == 1.0 and kin_def.tree_sum([1.0, 2.0, 4.0]) == 7.0
    t = np.array([1e16, 1.0, -1e16, 1.0, 1.0])                           # (t0 + t4) + t2 first, then (t1 + t3)
    assert kin_def.tree_sum(t) == ((1e16 + 1.0) + (-1e16 + 0.0)) + ((1.0 + 0.0) + (1.0 + 0.0))


# ---- the mirror tables ------------------------------------------------------------------------------------------------------

def test_mirror_tables_derive_from_joint_pairs():
    for g, pairs in ((graph_ntu, kin_def.NTU_JOINT_PAIRS), (Graph_h36m, kin_def.H36M_JOINT_PAIRS)):
        want = kin_def.mirror_from_joints(g.bones, pairs)
        assert sorted((min(p), max(p)) for p in g.mirror_bones) == want
        assert len({i for p in g.mirror_bones for i in p}) == 2 * len(g.mirror_bones)       # no bone in two pairs
    assert len(graph_ntu.mirror_bones) == 10 and len(Graph_h36m.mirror_bones) == 6
    assert [tuple(b) for b in graph_ntu.bones] == kin_def.NTU_BONES and [tuple(b) for b in Graph_h36m.bones] == kin_def.H36M_BONES


# ---- ABI --------------------------------------------------------------------------------------------------------------------

def test_exports_layout_and_constants(lib):
    for name in ("kg_kin_desc_workspace_bytes", "kg_kin_desc_lds_bytes", "kg_kin_desc", "kg_kin_scores_lds_bytes", "kg_kin_scores"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    abi_layout.assert_mirror("KgKinDescArgs")
    abi_layout.assert_mirror("KgKinScoresArgs")
    consts = abi_layout.header_constants()
    assert consts["KG_KIN_DESC"] == _native.KIN_DESC == len(metrics.KIN_NAMES) == 6
    assert metrics.KIN_NAMES == kin_def.KIN_NAMES
    assert (consts["KG_KIN_MAX_JOINTS"], consts["KG_KIN_MAX_BONES"], consts["KG_KIN_MAX_MIRROR"]) == (32, 32, 16)
    assert (consts["KG_KIN_MIN_FRAMES"], consts["KG_KIN_MAX_ELEMS"]) == (4, 32768)
    assert (consts["KG_KIN_MAX_SETS"], consts["KG_KIN_MAX_POINTS"]) == (4, 16384)
    assert lib.kg_abi_version() == 9


def desc_args(**over):
    """a complete, valid KgKinDescArgs (NTU, 2 classes x 3 samples, T 8) with fake device addresses; nothing launches in these
    tests because every call below is rejected first"""
    C, V, bones, mirror = kin_def.skeleton("ntu")
    kw = dict(n=3, T=8, C=C, V=V, classes=2, bones=bones, mirror=mirror, still_eps=1e-3)
    ptr = dict(x=0x1000, desc=0x2000, degenerate=0x3000, ws=0x4000, counters=0x5000)
    fields = dict(sc=3 * C * 8 * V, ss=C * 8 * V, sf=V, so=8 * V, ws_bytes=4 * 6, counters_len=1)
    for k, v in over.items():
        (kw if k in kw else ptr if k in ptr else fields)[k] = v
    a, keep = _native._kin_desc_shape(kw["n"], kw["T"], kw["C"], kw["V"], kw["classes"], kw["bones"], kw["mirror"], kw["still_eps"])
    for k, v in list(ptr.items()) + list(fields.items()):
        setattr(a, k, v)
    return a, keep


def test_desc_queries_accept_the_valid_shape(lib):
    a, keep = desc_args()
    assert lib.kg_kin_desc_workspace_bytes(ctypes.byref(a)) == 4 * 6
    lds = lib.kg_kin_desc_lds_bytes(ctypes.byref(a))
    assert 4 * 3 * 8 * 25 < lds <= 4 * 3 * 8 * 25 + 4096
    assert _native.kin_desc_lds_bytes(100, 256, 3, 25, 60, *kin_def.skeleton("ntu")[2:]) <= 160 * 1024       # NTU at T 256
    assert _native.kin_desc_lds_bytes(100, 1024, 2, 16, 10, *kin_def.skeleton("h36m")[2:]) <= 160 * 1024     # H36M at T 1024


BAD_BONE = list(kin_def.NTU_BONES)
BAD_BONE[5] = (3, 25)
NEG_BONE = list(kin_def.NTU_BONES)
NEG_BONE[0] = (-1, 2)
DESC_REJECTS = [
    (dict(x=None), b"null pointer x"), (dict(desc=None), b"null pointer desc"), (dict(degenerate=None), b"null pointer degenerate"),
    (dict(ws=None), b"null pointer ws"), (dict(counters=None), b"null pointer counters"), (dict(counters_len=0), b"counters_len"),
    (dict(ws_bytes=20), b"ws_bytes"),
    (dict(classes=0), b"classes=0"), (dict(n=0), b"n=0"), (dict(n=1 << 23), b"classes * n"),
    (dict(C=1), b"C=1"), (dict(C=4), b"C=4"), (dict(V=33, bones=[(0, 1)], mirror=[]), b"V=33"), (dict(V=0), b"V=0"),
    (dict(bones=[]), b"B=0"), (dict(bones=[(0, 1)] * 33, mirror=[]), b"B=33"), (dict(mirror=[(0, 1)] * 17), b"M=17"),
    (dict(T=3), b"T=3"), (dict(T=437), b"C*T*V"),
    (dict(sf=-1), b"negative stride"),
    (dict(bones=BAD_BONE), b"bones[5][1]=25"), (dict(bones=NEG_BONE), b"bones[0][0]=-1"),
    (dict(mirror=[(0, 24)]), b"mirror[0][1]=24"), (dict(mirror=[(0, 1), (-2, 3)]), b"mirror[1][0]=-2"),
    (dict(still_eps=-1e-3), b"still_eps"), (dict(still_eps=float("nan")), b"still_eps"), (dict(still_eps=float("inf")), b"still_eps"),
]


@pytest.mark.parametrize("over,msg", DESC_REJECTS, ids=[m.decode().replace(" ", "_") + str(i) for i, (_, m) in enumerate(DESC_REJECTS)])
def test_desc_rejections_name_the_field(lib, over, msg):
    a, keep = desc_args(**over)
    assert lib.kg_kin_desc(ctypes.byref(a), None) < 0
    err = lib.kg_last_error()
    assert b"kg_kin_desc" in err and msg in err, err


def test_desc_null_tables(lib):
    a, keep = desc_args()
    a.bones = None
    assert lib.kg_kin_desc(ctypes.byref(a), None) < 0 and b"null pointer bones" in lib.kg_last_error()
    a, keep = desc_args()
    a.mirror = None
    assert lib.kg_kin_desc(ctypes.byref(a), None) < 0 and b"null pointer mirror" in lib.kg_last_error()
    assert lib.kg_kin_desc(None, None) < 0 and b"null args" in lib.kg_last_error()
    with pytest.raises(RuntimeError, match="T=3"):
        _native.kin_desc_lds_bytes(3, 3, 3, 25, 2, *kin_def.skeleton("ntu")[2:])


def scores_args(**over):
    a = _native._kin_scores_shape(over.pop("nsets", 2), over.pop("n", 5), over.pop("m", 7), over.pop("classes", 3))
    a.real, a.mean_real, a.mean_fake, a.w1, a.w1_mean, a.scores, a.nonfinite = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    for g in range(4):
        a.fake[g] = 0x8000 + 0x1000 * g
    for k, v in over.items():
        setattr(a, k, v)
    return a


SCORES_REJECTS = [
    (dict(real=None), b"null pointer real"), (dict(mean_real=None), b"null pointer mean_real"),
    (dict(mean_fake=None), b"null pointer mean_fake"), (dict(w1=None), b"null pointer w1"),
    (dict(w1_mean=None), b"null pointer w1_mean"), (dict(scores=None), b"null pointer scores"),
    (dict(nonfinite=None), b"null pointer nonfinite"),
    (dict(classes=0), b"classes=0"), (dict(n=0), b"n=0"), (dict(m=0), b"m=0"),
    (dict(n=8192, m=8193), b"n + m = 16385"), (dict(n=16384, m=1), b"n + m = 16385"),
    (dict(nsets=0), b"nsets=0"), (dict(nsets=5), b"nsets=5"),
]


@pytest.mark.parametrize("over,msg", SCORES_REJECTS, ids=[m.decode().replace(" ", "_") for _, m in SCORES_REJECTS[:-3]] + ["cap_b", "nsets0", "nsets5"])
def test_scores_rejections_name_the_field(lib, over, msg):
    a = scores_args(**dict(over))
    assert lib.kg_kin_scores(ctypes.byref(a), None) < 0
    err = lib.kg_last_error()
    assert b"kg_kin_scores" in err and msg in err, err


def test_scores_null_set_and_queries(lib):
    a = scores_args(nsets=3)
    a.fake[2] = None
    assert lib.kg_kin_scores(ctypes.byref(a), None) < 0 and b"null pointer fake[2]" in lib.kg_last_error()
    a = scores_args(nsets=2)
    a.fake[3] = None                                                     # beyond nsets: not looked at ... but nothing may launch here
    assert lib.kg_kin_scores_lds_bytes(ctypes.byref(a)) == 8 * 16 + 4 * 256 + 16
    assert _native.kin_scores_lds_bytes(4, 8192, 8192, 1) == 8 * 16384 + 4 * 1024 + 16 <= 160 * 1024
    assert _native.kin_scores_lds_bytes(1, 6000, 6000, 1) == 8 * 16384 + 4 * 1024 + 16
    assert _native.kin_scores_lds_bytes(1, 1024, 1024, 60) == 8 * 2048 + 4 * 256 + 16
    with pytest.raises(RuntimeError, match="n \\+ m = 16385"):
        _native.kin_scores_lds_bytes(1, 8192, 8193, 1)
    assert lib.kg_kin_scores(None, None) < 0 and b"null args" in lib.kg_last_error()


# ---- metrics.kinematics: argument errors (raised before anything touches a GPU) -------------------------------------------------

def test_metrics_kinematics_argument_errors():
    ok = torch.zeros(4, 3, 8, 25)
    k = metrics.kinematics
    with pytest.raises(ValueError, match="gen samples are \\(N, C, T, V\\)"):
        k(torch.zeros(4, 3, 8), ok)
    with pytest.raises(ValueError, match="gen has C=4"):
        k(torch.zeros(4, 4, 8, 25), torch.zeros(4, 4, 8, 25))
    with pytest.raises(ValueError, match="T=3 frames"):
        k(torch.zeros(4, 3, 3, 25), torch.zeros(4, 3, 3, 25))
    with pytest.raises(ValueError, match="C\\*T\\*V"):
        k(torch.zeros(1, 3, 500, 25), torch.zeros(1, 3, 500, 25))
    with pytest.raises(ValueError, match="differ in shape"):
        k(torch.zeros(4, 3, 9, 25), ok)
    with pytest.raises(ValueError, match="undefined dataset"):
        k(ok, ok, dataset="kinetics")
    with pytest.raises(ValueError, match="bones name a joint outside \\[0, V=16\\)"):
        k(torch.zeros(4, 2, 8, 16), torch.zeros(4, 2, 8, 16), dataset="ntu")
    with pytest.raises(ValueError, match="mirror names a bone"):
        k(ok, ok, bones=[(0, 1), (1, 2)], mirror=[(0, 2)])
    with pytest.raises(ValueError, match="33 bones"):
        k(ok, ok, bones=[(0, 1)] * 33)
    with pytest.raises(ValueError, match="17 mirror pairs"):
        k(ok, ok, mirror=[(0, 1)] * 17)
    with pytest.raises(ValueError, match="still_eps"):
        k(ok, ok, still_eps=-1.0)
    with pytest.raises(ValueError, match="3 labels_gen for 4 samples"):
        k(ok, ok, labels_gen=[0, 1, 0], labels_real=[0, 1, 0, 1])
    with pytest.raises(ValueError, match="ragged classes"):
        k(ok, ok, labels_gen=[0, 1, 0, 1], labels_real=[0, 1, 1, 1])
    with pytest.raises(ValueError, match="per_class=3 needed"):
        k(ok, ok, labels_gen=[0, 1, 0, 1], labels_real=[0, 1, 0, 1], per_class=3)
    with pytest.raises(ValueError, match="n \\+ m = 8192 \\+ 8193"):
        k(torch.zeros(8193, 2, 4, 1), torch.zeros(8192, 2, 4, 1), bones=[(0, 0)])
    with pytest.raises(ValueError, match="5 sets"):
        metrics.kinematics_sets([ok] * 5, torch.zeros(1, 4, 6))
    with pytest.raises(ValueError, match="real_desc is the"):
        metrics.kinematics_sets([ok], torch.zeros(1, 4, 5))
    with pytest.raises(ValueError, match="labels name 2 classes, real_desc has 1"):
        metrics.kinematics_sets([ok], torch.zeros(1, 4, 6), labels=[0, 1, 0, 1])
