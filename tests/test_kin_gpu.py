"""kg_kin_desc / kg_kin_scores on the MI355X against the float64 definition (tests/kin_def.py), in two stages so that a loose
end-to-end bound cannot hide an error:
  (a) desc against the definition inside a derived bracket: one fp32 rounding, 2^-24 |def|, plus the fp64 evaluation error of
      kin_def.eval_error, which must come out under 2^-30 |def| on the test data - asserted, with bone_cv >= 1e-3 and "no step
      within 1e-6 relative of the still threshold", BEFORE the kernel's output is read; `still` is an exact count and must
      equal the definition's single rounding exactly;
  (b) mean_*, w1, w1_mean and scores against the definition evaluated on the KERNEL'S OWN desc, bit for bit.
Then the closed forms on the device, NaN and all-zero samples, strided inputs, determinism, graph capture, metrics.kinematics /
kinematics_sets and the command-line tool.  Outputs start poisoned and red-zoned (tests/guard.py)."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native
from kinetic_gan_amd import metrics

import kin_def
import mmd_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)

pytestmark = pytest.mark.gpu
SCORE_KEYS = ("mean_real", "mean_fake", "w1", "w1_mean", "scores", "nonfinite")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


def view(x):
    """(K, n, C, T, V) tensor (any strides, joints contiguous) -> FrechetView"""
    return _native.FrechetView(x, x.stride(0), x.stride(1), x.stride(3), x.stride(2))


def run_desc(x, bones, mirror, still_eps=1e-3):
    K, n, C, T, V = x.shape
    desc, degenerate = _native.kin_desc(view(x), n, T, C, V, K, bones, mirror, still_eps)
    guard.assert_no_poison(desc, "desc")
    guard.assert_no_poison(degenerate, "degenerate")
    return desc, degenerate


@functools.lru_cache(maxsize=None)
def case(name, seed, K, n, T, mirrored=True, still_eps=1e-3):
    """(x numpy, bones, mirror, the definition with its brackets): computed once; nothing of the kernel is read here"""
    C, V, bones, mirror = kin_def.skeleton(name)
    if not mirrored:
        mirror = []
    x = kin_def.make_data(seed, K, n, C, T, V)
    ref = kin_def.descriptors(x, bones, mirror, still_eps)
    ref["err"] = np.stack([[kin_def.eval_error(x[k, i], bones, mirror, ref["d64"][k, i]) for i in range(n)] for k in range(K)])
    # the conditions of the bracket, on the definition alone
    assert ref["d64"][..., 0].min() >= 1e-3, "bone_cv of the test data cancels"
    assert min(kin_def.threshold_margin(x[k, i], bones, still_eps) for k in range(K) for i in range(n)) >= 1e-6
    assert (ref["err"][..., :5] <= 2.0 ** -30).all(), "the fp64 evaluation error is too large to test anything"
    return x, tuple(bones), tuple(mirror), ref


def check_desc(desc, degenerate, ref, rows=None):
    """stage (a) for every sample (or the (k, i) in rows)"""
    got = desc.cpu().numpy().astype(np.float64)
    K, n = got.shape[:2]
    worst = 0.0
    for k in range(K):
        for i in range(n):
            if rows is not None and (k, i) not in rows:
                continue
            d = ref["d64"][k, i]
            tol = (kin_def.U32 + ref["err"][k, i][:5]) * np.abs(d[:5])
            err = np.abs(got[k, i, :5] - d[:5])
            worst = max(worst, (err / np.maximum(tol, 1e-300)).max())
            assert (err <= tol).all(), (k, i, got[k, i], d, err, tol)
            assert np.float32(got[k, i, 5]) == ref["desc"][k, i, 5], (k, i, got[k, i, 5], ref["desc"][k, i, 5])     # exact count
    print("stage (a): worst error / bracket %.3f" % worst)
    if rows is None:
        assert degenerate.cpu().tolist() == ref["degenerate"].tolist()


# ---- stage (a) ---------------------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("n", [1, 5, 40])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("T", [4, 5, 64])
@pytest.mark.parametrize("name", ["ntu", "h36m"])
def test_descriptors_against_the_definition(name, T, K, n):
    x, bones, mirror, ref = case(name, 1, K, n, T)
    desc, degenerate = run_desc(torch.from_numpy(x).cuda(), bones, mirror)
    assert desc.shape == (K, n, 6) and desc.dtype == torch.float32 and degenerate.dtype == torch.int32
    check_desc(desc, degenerate, ref)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("name", ["ntu", "h36m"])
def test_still_counts_with_a_wide_threshold(name):
    """still_eps = 0.05: a good share of the steps is still, and the count is the definition's exactly"""
    x, bones, mirror, ref = case(name, 2, 2, 7, 33, True, 0.05)
    assert ref["still"].min() >= 1 and ref["still"].max() > 20
    desc, degenerate = run_desc(torch.from_numpy(x).cuda(), bones, mirror, 0.05)
    check_desc(desc, degenerate, ref)


@pytest.mark.usefixtures("guarded")
def test_crop_class_stride_and_no_mirror():
    x, bones, mirror, ref = case("ntu", 3, 3, 5, 9)
    K, n, C, T, V = x.shape
    g = torch.Generator(device="cuda").manual_seed(0)
    # a crop in T, read in place
    long = torch.randn((K, n, C, T + 5, V), device="cuda", generator=g)
    long[:, :, :, 2:2 + T] = torch.from_numpy(x).cuda()
    crop = long[:, :, :, 2:2 + T]
    assert not crop.is_contiguous() and crop.stride(3) == V and crop.stride(2) == (T + 5) * V
    check_desc(*run_desc(crop, bones, mirror), ref)
    # a class stride that is not n * the sample stride
    wide = torch.randn((K, n + 3, C, T, V), device="cuda", generator=g)
    wide[:, :n] = torch.from_numpy(x).cuda()
    part = wide[:, :n]
    assert part.stride(0) == (n + 3) * part.stride(1)
    check_desc(*run_desc(part, bones, mirror), ref)
    # M = 0
    x0, bones0, mirror0, ref0 = case("ntu", 3, 3, 5, 9, False)
    assert mirror0 == () and (ref0["d64"][..., 1] == 0).all()
    desc, degenerate = run_desc(torch.from_numpy(x0).cuda(), bones0, mirror0)
    check_desc(desc, degenerate, ref0)
    assert (desc[..., 1] == 0).all()
    # strides that reach outside the tensor are refused before the launch
    with pytest.raises(ValueError, match="reach outside"):
        _native.kin_desc(_native.FrechetView(part, part.stride(0), part.stride(1), part.stride(3), part.stride(2)), n + 4, T, C,
                         V, K, bones, mirror)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("name", ["ntu", "h36m"])
def test_closed_forms_on_the_device(name):
    """rigid integer translation at constant velocity of a mirrored skeleton (T = 8: the mean of 8 equal lengths is exact in
    every tree of pairs); a frozen sample; an all-zero sample"""
    x, bones, mirror = kin_def.int_skeleton(name, 8)
    C = x.shape[0]
    moving = x + (np.arange(8, dtype=np.float32) * 3)[None, :, None]
    batch = np.stack([moving, x, np.zeros_like(x)])[None]               # (1, 3, C, 8, V)
    desc, degenerate = run_desc(torch.from_numpy(batch).cuda(), bones, mirror)
    d = desc.cpu().numpy()[0]
    s = kin_def.lengths(x, bones).mean()
    assert d[0, 0] == 0 and d[0, 1] == 0 and d[0, 3] == 0 and d[0, 4] == 0 and d[0, 5] == 0
    assert d[0, 2] == pytest.approx(np.sqrt(C * 9.0) / s, rel=2.0 ** -23)
    assert d[1, 0] == 0 and d[1, 1] == 0 and d[1, 2] == 0 and d[1, 5] == 1
    assert (d[2] == 0).all() and not np.signbit(d[2]).any()
    assert degenerate.cpu().tolist() == [1]


@pytest.mark.usefixtures("guarded")
def test_nan_and_zero_samples_inside_an_ordinary_class():
    x, bones, mirror, ref = case("ntu", 4, 3, 6, 12)
    x = x.copy()
    x[1, 2, 1, 3, 7] = np.nan                                           # one coordinate of one joint in one frame
    x[1, 4] = 0.0
    x[2, 0] = 5.0                                                       # a constant, non-zero sample collapses as well
    desc, degenerate = run_desc(torch.from_numpy(x).cuda(), bones, mirror)
    touched = {(1, 2), (1, 4), (2, 0)}
    check_desc(desc, degenerate, ref, rows={(k, i) for k in range(3) for i in range(6)} - touched)        # every other row
    want = kin_def.descriptors(x, bones, mirror)
    got = desc.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want["desc"]))
    assert np.isnan(got[1, 2, [0, 2, 3, 4]]).all() and got[1, 2, 5] == 0
    assert (got[1, 4] == 0).all() and (got[2, 0] == 0).all()
    assert degenerate.cpu().tolist() == [0, 1, 1] == want["degenerate"].tolist()
    out = _native.kin_scores(desc, [desc.flip(1).contiguous()])
    assert out["nonfinite"].cpu().tolist() == [[0, 1, 0], [0, 1, 0]]
    check_scores(out, desc, [desc.flip(1).contiguous()])
    w1 = out["w1"].cpu().numpy()[0]
    assert np.isnan(w1[1, [0, 2, 3, 4]]).all() and w1[1, 5] == 0 and (w1[[0, 2]] == 0).all()       # a set against its permutation
    assert np.isnan(out["scores"].cpu().numpy()[0, 0])


# ---- stage (b) ---------------------------------------------------------------------------------------------------------------

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def check_scores(out, real_desc, fake_descs):
    """the definition on the kernel's own descriptors, bit for bit (NaN: NaN in the same places)"""
    for k in SCORE_KEYS:
        guard.assert_no_poison(out[k], k)
    want = kin_def.scores(real_desc.cpu().numpy(), [f.cpu().numpy() for f in fake_descs])
    for k in SCORE_KEYS:
        g, w = out[k].cpu().numpy(), want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype.kind == "f":
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), k
            g, w = np.where(nan, 0, g), np.where(nan, 0, w)
        assert np.array_equal(bits(g), bits(w)), (k, g, w)


def same_bits(a, b, keys=SCORE_KEYS):
    for k in keys:
        assert torch.equal(a[k].view(torch.int64) if a[k].dtype == torch.float64 else a[k],
                           b[k].view(torch.int64) if b[k].dtype == torch.float64 else b[k]), k


@functools.lru_cache(maxsize=None)
def device_desc(seed, K, cnt, name="ntu", T=4):
    """the kernel's own descriptors of make_data samples (stage (a) has checked them), on the device"""
    C, V, bones, mirror = kin_def.skeleton(name)
    x = torch.from_numpy(kin_def.make_data(seed, K, cnt, C, T, V)).cuda()
    return _native.kin_desc(view(x), cnt, T, C, V, K, bones, mirror)[0]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("K,n,m", [(3, 1, 1), (3, 5, 7), (3, 100, 100), (3, 37, 50), (2, 33, 32), (1, 1024, 1000), (1, 1025, 1024),
                                   (1, 8192, 8192)],
                         ids=["1+1", "5+7", "100+100", "37+50", "pow2+1", "2024", "2049", "cap"])
def test_scores_on_the_kernels_own_descriptors_bit_for_bit(K, n, m):
    real, fake = device_desc(11, K, n), device_desc(12, K, m)
    out = _native.kin_scores(real, [fake])
    assert out["w1"].shape == (1, K, 6) and out["w1"].dtype == torch.float64 and out["scores"].dtype == torch.float32
    check_scores(out, real, [fake])
    w1 = out["w1"].cpu().numpy()
    assert np.isfinite(w1).all() and (w1 >= 0).all()
    if n > 1:
        assert (w1[..., :5] > 0).all()


@pytest.mark.usefixtures("guarded")
def test_scores_with_duplicates_across_and_within_the_sides():
    rng = np.random.RandomState(3)
    real = (rng.randint(-3, 6, size=(2, 37, 6)) / 4).astype(np.float32)
    fake = (rng.randint(-3, 6, size=(2, 50, 6)) / 4).astype(np.float32)
    real[0, :4, 0], fake[0, :4, 0] = [-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 0.0, 0.0]
    fake[1, :37] = real[1]                                              # the real class again, plus 13 more
    rt, ft = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    out = _native.kin_scores(rt, [ft])
    check_scores(out, rt, [ft])
    perm = torch.from_numpy(rng.permutation(37)).cuda()
    same = _native.kin_scores(rt, [rt[:, perm].contiguous()])           # two permutations of one multiset with ties
    assert (same["w1"] == 0).all() and (same["scores"] == 0).all()
    shifted = _native.kin_scores(rt, [rt + 0.5])
    assert (shifted["w1"] == 0.5).all()                                 # quarters: every gap and product is exact
    a = torch.tensor([0.0, 1.0], device="cuda").repeat(6, 1).t().reshape(1, 2, 6).contiguous()
    b = torch.tensor([0.0, 0.5, 1.0], device="cuda").repeat(6, 1).t().reshape(1, 3, 6).contiguous()
    assert (_native.kin_scores(a, [b])["w1"] == 1.0 / 6.0).all()


@pytest.mark.usefixtures("guarded")
def test_sets_equal_their_one_set_calls():
    real = device_desc(11, 3, 37)
    fakes = [device_desc(20 + g, 3, 50) for g in range(4)]
    ones = [_native.kin_scores(real, [f]) for f in fakes]
    for nsets in (1, 2, 3, 4):
        out = _native.kin_scores(real, fakes[:nsets])
        check_scores(out, real, fakes[:nsets])
        assert out["w1"].shape == (nsets, 3, 6) and out["nonfinite"].shape == (nsets + 1, 3)
        for g in range(nsets):
            for k in ("mean_fake", "w1", "w1_mean", "scores"):
                assert np.array_equal(bits(out[k][g].cpu().numpy()), bits(ones[g][k][0].cpu().numpy())), (nsets, g, k)
            assert torch.equal(out["mean_real"].view(torch.int64), ones[g]["mean_real"].view(torch.int64))
            assert torch.equal(out["nonfinite"][g + 1], ones[g]["nonfinite"][1])


def test_cap_is_enforced():
    real, fake = torch.zeros((1, 8193, 6), device="cuda"), torch.zeros((1, 8192, 6), device="cuda")
    with pytest.raises(RuntimeError, match="n \\+ m = 16385"):
        _native.kin_scores(real, [fake])
    with pytest.raises(RuntimeError, match="nsets=5"):
        _native.kin_scores(fake, [fake] * 5)
    with pytest.raises(ValueError, match="share classes and m"):
        _native.kin_scores(fake, [fake, real])


# ---- launch properties -----------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_two_calls_give_the_same_bits():
    x, bones, mirror, _ = case("ntu", 1, 3, 40, 64)
    xt = torch.from_numpy(x).cuda()
    a, da = run_desc(xt, bones, mirror)
    b, db = run_desc(xt, bones, mirror)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(da, db)
    fake = device_desc(12, 3, 50, T=64)
    same_bits(_native.kin_scores(a, [fake, fake]), _native.kin_scores(b, [fake, fake]))


def _batches(seed, K=3, n=8, m=6, T=12, name="ntu"):
    C, V, _, _ = kin_def.skeleton(name)
    real = torch.from_numpy(kin_def.make_data(seed, K, n, C, T, V)).cuda().reshape(K * n, C, T, V)
    gen = torch.from_numpy(kin_def.make_data(seed + 100, K, m, C, T, V, scale=0.25, shift=-0.3)).cuda().reshape(K * m, C, T, V)
    return real, gen, np.repeat(np.arange(K), n), np.repeat(np.arange(K), m)


def test_graph_capture_replays_on_new_inputs():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    real, gen, lab_r, lab_g = _batches(2)
    real2, gen2, _, _ = _batches(5)
    before = metrics.kinematics(gen, real, lab_g, lab_r)["w1"].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.kinematics(gen, real, lab_g, lab_r, per_sample=True)    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = metrics.kinematics(gen, real, lab_g, lab_r, per_sample=True)
    real.copy_(real2)
    gen.copy_(gen2)
    g.replay()
    torch.cuda.synchronize()
    eager = metrics.kinematics(gen2, real2, lab_g, lab_r, per_sample=True)
    for k in eager:
        x, y = cap[k], eager[k]
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32),
                           y.view(torch.int64) if y.dtype == torch.float64 else y.view(torch.int32)), k
    assert not torch.equal(eager["w1"], before)                         # (the two inputs do score differently)


@pytest.mark.usefixtures("guarded")
def test_metrics_kinematics_against_the_definition():
    """labels, per_class, numpy inputs, a value scale that differs between the sides; then kinematics_sets against four
    kinematics calls, bit for bit"""
    K, n, m, T = 3, 8, 6, 12
    real, gen, lab_r, lab_g = _batches(2, K, n, m, T)
    C, V, bones, mirror = kin_def.skeleton("ntu")
    out = metrics.kinematics(gen, real, lab_g, np.eye(K)[lab_r], per_sample=True)
    assert out["w1_mean"].shape == (6,) and out["w1"].shape == (K, 6) and out["nonfinite"].shape == (2, K)
    assert out["desc_real"].shape == (K, n, 6) and out["desc_fake"].shape == (K, m, 6)
    assert out["degenerate"].cpu().tolist() == [0] * K == out["degenerate_real"].cpu().tolist()
    for key, x, cnt in (("desc_real", real, n), ("desc_fake", gen, m)):
        xn = x.cpu().numpy().reshape(K, cnt, C, T, V)
        ref = kin_def.descriptors(xn, bones, mirror)
        ref["err"] = np.stack([[kin_def.eval_error(xn[k, i], bones, mirror, ref["d64"][k, i]) for i in range(cnt)] for k in range(K)])
        assert ref["d64"][..., 0].min() >= 1e-3 and (ref["err"][..., :5] <= 2.0 ** -30).all()
        assert min(kin_def.threshold_margin(xn[k, i], bones) for k in range(K) for i in range(cnt)) >= 1e-6
        check_desc(out[key], out["degenerate"], ref)
    want = kin_def.scores(out["desc_real"].cpu().numpy(), [out["desc_fake"].cpu().numpy()])
    for key in ("w1_mean", "scores", "w1", "mean_fake"):
        assert np.array_equal(bits(out[key].cpu().numpy()), bits(want[key][0])), key
    assert np.array_equal(bits(out["mean_real"].cpu().numpy()), bits(want["mean_real"]))
    # classes interleaved, per_class, numpy input: the same samples, the same bits
    perm_r, perm_g = np.argsort(np.tile(np.arange(n), K), kind="stable"), np.argsort(np.tile(np.arange(m), K), kind="stable")
    mixed = metrics.kinematics(gen[torch.as_tensor(perm_g).cuda()].cpu().numpy(), real[torch.as_tensor(perm_r).cuda()], lab_g[perm_g],
                               lab_r[perm_r], per_sample=True)
    for key in out:
        assert torch.equal(mixed[key], out[key]), key
    four = metrics.kinematics(gen, real, lab_g, lab_r, per_class=4, per_sample=True)
    assert torch.equal(four["desc_real"], out["desc_real"][:, :4]) and torch.equal(four["desc_fake"], out["desc_fake"][:, :4])
    # sets
    sets = [gen, gen.flip(2), gen * 2 + 1, gen.roll(1, 0).contiguous()]
    cache, deg_r = metrics.kinematics_real(real, lab_r, with_degenerate=True)
    assert torch.equal(cache, out["desc_real"]) and torch.equal(deg_r, out["degenerate_real"])
    both = metrics.kinematics_sets(sets, cache, lab_g)
    assert both["w1_mean"].shape == (4, 6) and both["scores"].shape == (4, 6) and both["desc"].shape == (4, K, m, 6)
    for g, s in enumerate(sets):
        one = metrics.kinematics(s, real, lab_g, lab_r, per_sample=True)
        for key in ("w1_mean", "scores", "w1", "mean_fake", "degenerate"):
            assert torch.equal(both[key][g], one[key]), (g, key)
        assert torch.equal(both["mean_real"], one["mean_real"]) and torch.equal(both["desc"][g], one["desc_fake"])
        assert torch.equal(both["nonfinite"][[0, g + 1]], one["nonfinite"])
    assert not torch.equal(both["w1"][0], both["w1"][3])


def test_kinematics_actions_tool_end_to_end(tmp_path, capsys):
    """tools/kinematics_actions.py on a small H36M-shaped .npy / .pkl quadruple: selection, normalisation, metrics.kinematics"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kinematics_actions
    n, C, T, V = 400, 2, 12, 16
    rng = np.random.RandomState(0)
    lab = rng.permutation(np.repeat(np.arange(10), n // 10))
    real = np.ascontiguousarray(kin_def.make_data(7, 1, n, C, T, V)[0])
    lo, hi = real.min(), real.max()
    fake = kin_def.make_data(8, 1, n, C, T, V)[0]
    fake = np.ascontiguousarray(((2 * ((fake - fake.min()) / (fake.max() - fake.min())) - 1) * 0.9).astype(np.float32))
    fake_lab = lab[::-1].copy()
    for nm, d, lb in (("real", real, lab), ("fake", fake, fake_lab)):
        np.save(tmp_path / (nm + ".npy"), d)
        with open(tmp_path / (nm + ".pkl"), "wb") as f:
            pickle.dump(([str(i) for i in range(n)], lb.tolist()), f)
    argv = ["--data_real", str(tmp_path / "real.npy"), "--labels_real", str(tmp_path / "real.pkl"),
            "--data_fake", str(tmp_path / "fake.npy"), "--labels_fake", str(tmp_path / "fake.pkl"),
            "--t_size", "8", "--dataset", "h36m", "--per_class", "20", "--still_eps", "0.002", "--per_class_table"]
    got = kinematics_actions.main(argv)
    r_idx = mmd_def.select_scan(lab, list(range(10)), per_class=20)
    f_idx = mmd_def.select_scan(fake_lab, list(range(10)), per_class=20)
    sel_real = (2 * ((real[r_idx][:, :, :8] - lo) / (hi - lo)) - 1).astype(np.float32)
    sel_fake = fake[f_idx][:, :, :8]
    labels = np.repeat(np.arange(10), 20)
    want = metrics.kinematics(sel_fake, sel_real, labels, labels, dataset="h36m", still_eps=0.002)
    assert got == tuple(want["w1_mean"].cpu().tolist())
    assert len(got) == 6 and all(np.isfinite(v) and v >= 0 for v in got) and all(v > 0 for v in got[:5])
    text = capsys.readouterr().out
    assert "w1_bone_cv" in text and "mean_real bone_cv" in text and "mean_fake bone_cv" in text and text.count("\n") > 14
    one = kinematics_actions.main(argv[:-1] + ["--unconditional"])
    want1 = metrics.kinematics(sel_fake, sel_real, dataset="h36m", still_eps=0.002)
    assert one == tuple(want1["w1_mean"].cpu().tolist())
