"""The Frechet pose / motion distance without a GPU: the float64 definition (tests/frechet_def.py) against the reference's
recorded results and against closed forms, the caps on the tolerances of the shapes the GPU tests use, the argument checks of
kg_frechet and metrics.frechet, and the ctypes mirror of KgFrechetArgs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd import metrics

import abi_layout
import frechet_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frechet_ref.npz")

# ((classes, n, m, t, C, V), seeds, modes) of frechet_def.make_data in tests/test_frechet_gpu.py: the stage shapes, the
# rank-deficient and P = 2 shapes, the metrics.frechet case
BOTH = ("pose", "motion")
GPU_CASES = [((3, 5, 7, 9, 3, 25), (1, 2), BOTH), ((1, 40, 36, 8, 3, 4), (1, 2), BOTH), ((2, 6, 6, 5, 3, 1), (1, 2), BOTH),
             ((1, 30, 30, 4, 1, 1), (1, 2), BOTH), ((1, 48, 48, 8, 3, 32), (1, 2), BOTH), ((1, 37, 29, 64, 3, 25), (1, 2), BOTH),
             ((1, 1, 1, 20, 3, 25), (1,), BOTH), ((2, 1, 1, 2, 3, 4), (1,), ("pose",)), ((1, 2, 2, 1, 3, 4), (1,), ("pose",)),
             ((1, 1, 1, 3, 3, 4), (1,), ("motion",)), ((4, 10, 10, 16, 3, 25), (1,), BOTH)]
GPU_CLOSED_FORMS = [(40, 8, 3, 4), (20, 16, 3, 25)]         # (n, t, C, V) of frechet_def.closed_form_pairs there


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


# ---- the definition ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ntu", "h36m", "small", "max"])
def test_definition_against_the_reference(name):
    """the recorded calculate_frechet_distance of full-rank sets (P >= 4 d); the bracket is the trace term's: the solver's
    delta_eig carried through the square roots"""
    z = np.load(GOLDEN)
    R = (z[name + "_real_q"].astype(np.float32) / np.float32(127)).astype(np.float64)
    F = (z[name + "_fake_q"].astype(np.float32) / np.float32(127)).astype(np.float64)
    d = R.shape[1]
    assert frechet_def.full_rank(R.shape[0], F.shape[0], d)
    ref = frechet_def.one_class(R, F)
    tol = frechet_def.tol_tr(ref["e"], frechet_def.delta_eig(d, ref["e"].max()))
    want = float(z[name + "_fd"])
    print(name, ref["fd"], want, abs(ref["fd"] - want), tol)
    assert tol <= 1e-8 * ref["scale"] and want > 0.01 * ref["scale"]
    assert abs(ref["fd"] - want) <= tol


def test_closed_form_one_dimension():
    g = np.random.RandomState(0)
    R, F = g.randn(50, 1) * 0.7 + 0.2, g.randn(40, 1) * 0.3 - 0.1
    s1, s2 = R.std(ddof=1), F.std(ddof=1)
    want = (R.mean() - F.mean()) ** 2 + (s1 - s2) ** 2
    assert abs(frechet_def.one_class(R, F)["fd"] - want) <= 1e-14


def _cloud(seed, P, d):
    g = np.random.RandomState(seed)
    return g.randn(P, d) @ (g.randn(d, d) / np.sqrt(d)) + g.randn(d)


def test_closed_form_identical_shift_scale():
    R = _cloud(1, 200, 12)
    ref = frechet_def.one_class(R, R.copy())
    assert abs(ref["fd"]) <= 1e-12 * ref["scale"]
    b = np.linspace(-0.5, 0.5, 12)
    assert abs(frechet_def.one_class(R, R + b)["fd"] - b @ b) <= 1e-12 * ref["scale"]
    mu, S = frechet_def.moments(R)
    for s in (0.5, 1.7):
        want = (1 - s) ** 2 * (mu @ mu + np.trace(S))
        assert abs(frechet_def.one_class(R, s * R)["fd"] - want) <= 1e-12 * ref["scale"]


def test_definition_decomposes_the_real_covariance():
    """rank-deficient real set against a full-rank fake set and the other way round give the same T up to the null
    eigenvalues' round-off - and the definition takes the route through S_r"""
    R, F = _cloud(2, 6, 10), _cloud(3, 80, 10)
    a, b = frechet_def.one_class(R, F), frechet_def.one_class(F, R)
    assert abs(a["terms"][3] - b["terms"][3]) <= 1e-6 * a["scale"]
    assert a["lam_r"] == pytest.approx(np.linalg.eigvalsh(a["cov_real"]).max())


def test_points_pose_and_motion():
    x = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5) ** 2
    p = frechet_def.points(x, "pose")
    assert p.shape == (8, 15) and np.array_equal(p[5], x[1, :, 1, :].reshape(-1))
    q = frechet_def.points(x, "motion")
    assert q.shape == (6, 15) and np.array_equal(q[4], (x[1, :, 2, :].astype(np.float64) - x[1, :, 1, :]).reshape(-1))


def test_generator_is_exact_in_fp32():
    real, fake = frechet_def.make_data(1, 2, 3, 4, 3, 5, 7)
    assert real.shape == (2, 3, 3, 5, 7) and fake.shape == (2, 4, 3, 5, 7) and real.dtype == np.float32
    for x in (real, fake):
        q = np.round(x.astype(np.float64) * 127)
        assert np.array_equal((q.astype(np.float32) / np.float32(127)), x) and np.abs(q).max() <= 127


def _assert_caps(real, fake, mode, what):
    """real (K, n, C, t, V), fake (K, m, C, t, V): the tolerances of every class stay below the caps"""
    K, n, C, t, V = real.shape
    m = fake.shape[1]
    fr = t - (mode == "motion")
    per, _ = frechet_def.reference(real, fake, mode)
    xmax = max(np.abs(frechet_def.points(x.reshape((-1,) + x.shape[2:]), mode)).max() for x in (real, fake))
    for ref in per:
        tol = frechet_def.tolerances(ref, n * fr, m * fr, C * V, xmax)
        cap_b, cap_e = frechet_def.caps(n * fr, m * fr, C * V, ref["scale"])
        print(what, mode, "b %.3g / %.3g  e2e %.3g / %.3g" % (tol["b"], cap_b, tol["e2e"], cap_e))
        assert tol["b"] <= cap_b and tol["e2e"] <= cap_e
    return per


@pytest.mark.parametrize("shape,seeds,modes", GPU_CASES)
def test_tolerance_caps_on_the_gpu_shapes(shape, seeds, modes):
    """the brackets of tests/test_frechet_gpu.py hide nothing: stage (b) <= 1e-8 scale and end to end <= 1e-5 scale on
    full-rank sets (P >= 4 d in both), <= 1e-4 scale on the others - on the generator's data of every shape, seed and mode
    used there (its bounds() asserts the same caps on whatever it is given, the tool test's data included)"""
    K, n, m, t, C, V = shape
    for seed in seeds:
        real, fake = frechet_def.make_data(seed, K, n, m, C, t, V)
        for mode in modes:
            for ref in _assert_caps(real, fake, mode, (shape, seed)):
                assert ref["fd"] > 1e-3 * ref["scale"]          # (the two sets do differ: FD is not round-off)


@pytest.mark.parametrize("n,t,C,V", GPU_CLOSED_FORMS)
def test_tolerance_caps_on_the_closed_form_sets(n, t, C, V):
    """the dyadic sets of its closed-form test: F = R + b and F = 1.5 R hold exactly in fp32, and the caps hold"""
    R, b, sets = frechet_def.closed_form_pairs(n, t, C, V)
    R64 = R.astype(np.float64)
    assert np.array_equal(sets["identical"], R) and np.array_equal(sets["shift"].astype(np.float64), R64 + b)
    assert np.array_equal(sets["scale"].astype(np.float64), 1.5 * R64)
    for name, F in sets.items():
        for mode in BOTH:
            _assert_caps(R[None], F[None], mode, (n, t, C, V, name))


# ---- ABI ---------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports(lib):
    header = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    for sym in ("kg_frechet_workspace_bytes", "kg_frechet"):
        assert "%s(const KgFrechetArgs* a" % sym in header
        assert getattr(lib, sym) is not None
    assert len(_native.EXPORTS["kg_frechet_workspace_bytes"][1]) == 1 and len(_native.EXPORTS["kg_frechet"][1]) == 2
    assert "#define KG_FRECHET_MAX_DIM %d" % _native.FRECHET_MAX_DIM in header and _native.FRECHET_MAX_DIM == 96
    assert lib.kg_abi_version() == 9


def test_frechet_struct_matches_header():
    abi_layout.assert_mirror("KgFrechetArgs")


def _valid_args():
    a = _native._FrechetArgs()
    a.real, a.fake = 0x1000, 0x2000
    a.r_sc, a.r_ss, a.r_sf, a.r_so = 100 * 4800, 4800, 25, 1600
    a.f_sc, a.f_ss, a.f_sf, a.f_so = 100 * 4800, 4800, 25, 1600
    a.n, a.m, a.frames, a.diff, a.d_outer, a.d_inner, a.classes = 100, 90, 64, 1, 3, 25, 60
    a.values, a.terms, a.sweeps, a.ws = 0x3000, 0x4000, 0x5000, 0x6000
    return a


@pytest.mark.parametrize("fields,needle", [
    (dict(real=None), b"null pointer real"), (dict(fake=None), b"null pointer fake"),
    (dict(values=None), b"null pointer values"), (dict(terms=None), b"null pointer terms"),
    (dict(sweeps=None), b"null pointer sweeps"), (dict(ws=None), b"null pointer ws"),
    (dict(n=0), b"n=0"), (dict(m=-2), b"m=-2"), (dict(classes=0), b"classes=0"), (dict(d_outer=0), b"d_outer=0"),
    (dict(d_inner=0), b"d_inner=0"), (dict(diff=2), b"diff=2"),
    (dict(d_inner=33), b"d_outer=3 x d_inner=33 above KG_FRECHET_MAX_DIM"), (dict(d_outer=1, d_inner=97), b"d_inner=97"),
    (dict(frames=1), b"frames=1"), (dict(frames=0, diff=0), b"frames=0"),
    (dict(n=1, frames=2), b"n=1 gives P=1"), (dict(m=1, frames=1, diff=0), b"m=1 gives P=1"),
    (dict(n=1 << 20, frames=18), b"n=1048576 x frames=18"), (dict(m=(1 << 24) + 1, frames=1, diff=0), b"m=16777217 x frames=1"),
    (dict(classes=1 << 23), b"classes=8388608 make"),
    (dict(ws_bytes=64), b"ws_bytes=64"), (dict(ws=0x6004), b"ws is not 8-byte aligned")])
def test_kg_frechet_rejects_bad_arguments_without_gpu(lib, fields, needle):
    """every rejection happens before any GPU call, with the field named"""
    a = _valid_args()
    need = lib.kg_frechet_workspace_bytes(ctypes.byref(a))
    assert need > 0
    a.ws_bytes = need
    for k, v in fields.items():
        setattr(a, k, v)
    if not set(fields) & {"real", "fake", "values", "terms", "sweeps", "ws", "ws_bytes"}:
        assert lib.kg_frechet_workspace_bytes(ctypes.byref(a)) < 0
        assert needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_frechet(ctypes.byref(a), None) < 0
    assert needle in lib.kg_last_error(), lib.kg_last_error()


def test_workspace_holds_partials_and_moments(lib):
    """chunk partials + mu and S of both sets; the limits pass: d = 96, P = 2, P = 2^24"""
    d = 75
    need = _native.frechet_workspace_bytes(100, 100, 64, False, 3, 25, 60)
    assert need % 8 == 0 and need >= 8 * 60 * 2 * (d + d * d)
    assert need <= 8 * (1024 + 2 * 60) * 2 * (d + d * d)           # about 1024 chunk workgroups, never per point
    assert _native.frechet_workspace_bytes(2, 2, 1, False, 1, 96, 1) == 8 * 4 * (96 + 96 * 96)
    assert _native.frechet_workspace_bytes(1, 1, 3, True, 3, 32, 1) > 0
    assert _native.frechet_workspace_bytes(1 << 24, 2, 1, False, 1, 4, 1) > 0
    with pytest.raises(RuntimeError, match="above 2\\^24"):
        _native.frechet_workspace_bytes((1 << 24) + 1, 2, 1, False, 1, 4, 1)
    with pytest.raises(RuntimeError, match="frames=1"):
        _native.frechet_workspace_bytes(10, 10, 1, True, 3, 25, 1)


# ---- metrics.frechet ---------------------------------------------------------------------------------------------------

def test_metrics_frechet_argument_errors_without_gpu():
    x = torch.zeros(12, 2, 4, 3)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.frechet(x, torch.zeros(12, 2, 4, 5))
    with pytest.raises(ValueError, match=r"\(N, C, T, V\)"):
        metrics.frechet(x[0], x)
    ragged = [0] * 5 + [1] * 7
    with pytest.raises(ValueError, match="class 1 has 7 real samples"):
        metrics.frechet(x, x, labels_gen=[0] * 6 + [1] * 6, labels_real=ragged)
    with pytest.raises(ValueError, match="class 0 has 5 fake samples, per_class=6"):
        metrics.frechet(x, x, labels_gen=ragged, labels_real=[0] * 6 + [1] * 6, per_class=6)
    with pytest.raises(ValueError, match="d = C\\*V = 100 above 96"):
        metrics.frechet(torch.zeros(4, 4, 3, 25), torch.zeros(4, 4, 3, 25))
    with pytest.raises(ValueError, match="T=1 frames, mode 'motion' needs 2"):
        metrics.frechet(torch.zeros(8, 2, 1, 3), torch.zeros(8, 2, 1, 3), mode="motion")
    with pytest.raises(ValueError, match="either set needs two points"):
        metrics.frechet(torch.zeros(8, 2, 1, 3), torch.zeros(8, 2, 1, 3), per_class=1)
    with pytest.raises(ValueError, match="undefined mode"):
        metrics.frechet(x, x, mode="joint")
    with pytest.raises(ValueError, match=r"\(N, d\)"):
        metrics.frechet_features(x, x)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.frechet_features(torch.zeros(8, 5), torch.zeros(8, 6))
    with pytest.raises(ValueError, match="d = C\\*V = 97 above 96"):
        metrics.frechet_features(torch.zeros(8, 97), torch.zeros(8, 97))
    with pytest.raises(ValueError, match="class 1 has 7 real samples"):
        metrics.frechet_features(torch.zeros(12, 5), torch.zeros(12, 5), labels_gen=[0] * 6 + [1] * 6, labels_real=ragged)
    assert metrics.FRECHET_TERMS == ("dmu2", "tr_real", "tr_fake", "tr_sqrt") == frechet_def.TERMS
