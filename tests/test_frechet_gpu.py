"""kg_frechet on the MI355X against the float64 definition (tests/frechet_def.py), in three stages so that a loose end-to-end
bound cannot hide a solver error:
  (a) the kernel's mu and S against the definition within tol_mu / tol_S;
  (b) the kernel's T against the DEFINITION evaluated (numpy float64, host) on the kernel's own S_r, S_f within
      tol_tr(e, delta_eig);
  (c) FD = |dmu|^2 + tr S_r + tr S_f - 2 T recomputed in float64 from the outputs within 8 eps scale;
  end to end from raw data within 2 tol_tr(e, delta_eig + delta_mom) + 2 d tol_S + 2 sqrt(d) |dmu| tol_mu.
The brackets are capped on the float64 definition BEFORE the kernel's output is read (frechet_def.caps).  Then rank-deficient
and degenerate sets, closed forms, strided inputs, determinism, workspace reuse, graph capture, metrics.frechet and the
command-line tool."""
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

import frechet_def
import mmd_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)

pytestmark = pytest.mark.gpu
EPS = frechet_def.EPS
MOMENTS = ("mu_real", "mu_fake", "cov_real", "cov_fake")
ALL_KEYS = ("values", "terms", "sweeps", "mean") + MOMENTS
MODES = ("pose", "motion")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


def bounds(real, fake, mode):
    """the definition, its tolerances and the caps on them, per class: nothing of the kernel is read here"""
    K, n, C, t, V = real.shape
    m = fake.shape[1]
    fr, d = t - (mode == "motion"), C * V
    per, mean = frechet_def.reference(real, fake, mode)
    xmax = max(np.abs(frechet_def.points(x.reshape((-1,) + x.shape[2:]), mode)).max() for x in (real, fake))
    for ref in per:
        ref["tol"] = frechet_def.tolerances(ref, n * fr, m * fr, d, xmax)
        cap_b, cap_e = frechet_def.caps(n * fr, m * fr, d, ref["scale"])
        assert ref["tol"]["b"] <= cap_b and ref["tol"]["e2e"] <= cap_e, ("the bracket is too wide to test anything", ref["tol"])
    return per, mean


class _Refs(dict):
    def __init__(self, real, fake):
        super().__init__()
        self.data = (real, fake)

    def __missing__(self, mode):
        self[mode] = bounds(*self.data, mode)
        return self[mode]


@functools.lru_cache(maxsize=None)
def case(seed, K, n, m, t, C, V):
    """(real, fake) float32 numpy and on the GPU, and the float64 reference of a mode on request; each computed once"""
    real, fake = frechet_def.make_data(seed, K, n, m, C, t, V)
    return real, fake, torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda(), _Refs(real, fake)


def view(x):
    """(K, n, C, t, V) tensor -> FrechetView"""
    return _native.FrechetView(x, x.stride(0), x.stride(1), x.stride(3), x.stride(2))


def run(real, fake, mode, moments=True, ws=None):
    K, n, C, t, V = real.shape
    return _native.frechet(view(real), view(fake), n, fake.shape[1], t, mode == "motion", C, V, K, want_mean=True,
                           moments=moments, ws=ws)


def same_bits(a, b, keys=ALL_KEYS):
    for key in keys:
        x, y = a[key], b[key]
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), key


def check_stages(out, per, mean, P_r, P_f, d):
    o = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(np.isfinite(o[k]).all() for k in ALL_KEYS)
    assert (o["sweeps"] >= 1).all() and (o["sweeps"] < 40).all(), o["sweeps"]
    for c, ref in enumerate(per):
        tol = ref["tol"]
        # (a) moments
        for key, tl in (("mu_real", tol["tol_mu"]), ("mu_fake", tol["tol_mu"]), ("cov_real", tol["tol_S"]), ("cov_fake", tol["tol_S"])):
            err = np.abs(o[key][c] - ref[key]).max()
            print("class %d (a) %s err %.3g tol %.3g" % (c, key, err, tl))
            assert err <= tl, (key, err, tl)
        for key in ("cov_real", "cov_fake"):
            assert np.array_equal(o[key][c], o[key][c].T)              # symmetric bit for bit
        # (b) the trace term on the kernel's own covariances
        own = frechet_def.from_moments(o["mu_real"][c], o["cov_real"][c], o["mu_fake"][c], o["cov_fake"][c])
        tol_b = frechet_def.tol_tr(own["e"], frechet_def.delta_eig(d, max(own["e"].max(), 0.0)))
        assert tol_b <= frechet_def.caps(P_r, P_f, d, own["scale"])[0]
        err = abs(o["terms"][c, 3] - own["terms"][3])
        print("class %d (b) T err %.3g tol %.3g" % (c, err, tol_b))
        assert err <= tol_b
        # (c) assembly: the four terms, then FD from them
        scale = own["scale"]
        assert np.abs(o["terms"][c, :3] - own["terms"][:3]).max() <= d * EPS * scale     # a sum of d terms in another order
        t = o["terms"][c]
        assert abs(o["values"][c] - ((t[0] + t[1] + t[2]) - 2.0 * t[3])) <= 8 * EPS * (t[0] + t[1] + t[2])
        # end to end
        err = abs(o["values"][c] - ref["fd"])
        print("class %d e2e FD %.12g def %.12g err %.3g tol %.3g" % (c, o["values"][c], ref["fd"], err, tol["e2e"]))
        assert err <= tol["e2e"]
    s = 0.0
    for v in o["values"]:
        s += v
    assert o["mean"] == s / len(per)
    assert abs(o["mean"] - mean) <= max(r["tol"]["e2e"] for r in per)


STAGE_SHAPES = [(3, 5, 7, 9, 3, 25), (1, 40, 36, 8, 3, 4), (2, 6, 6, 5, 3, 1), (1, 30, 30, 4, 1, 1), (1, 48, 48, 8, 3, 32),
                (1, 37, 29, 64, 3, 25)]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("K,n,m,t,C,V", STAGE_SHAPES)
def test_stages(K, n, m, t, C, V, seed, mode):
    """d = 75 (odd: one idle index) with unequal sets, 12, 3, 1, the LDS maximum 96, and 2368 + 1856 points (pose) /
    2331 + 1827 (motion: a ragged last chunk) in several moment chunks"""
    _, _, real, fake, refs = case(seed, K, n, m, t, C, V)
    fr = t - (mode == "motion")
    out = run(real, fake, mode)
    check_stages(out, *refs[mode], n * fr, m * fr, C * V)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
def test_one_dimension_closed_form(mode):
    real, fake, real_g, fake_g, refs = case(1, 1, 30, 30, 4, 1, 1)
    out = run(real_g, fake_g, mode)
    R, F = frechet_def.points(real[0], mode), frechet_def.points(fake[0], mode)
    want = (R.mean() - F.mean()) ** 2 + (R.std(ddof=1) - F.std(ddof=1)) ** 2
    assert abs(out["values"].item() - want) <= refs[mode][0][0]["tol"]["e2e"]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("K,n,m,t,C,V,mode", [(1, 1, 1, 20, 3, 25, "pose"), (1, 1, 1, 20, 3, 25, "motion"),
                                                (2, 1, 1, 2, 3, 4, "pose"), (1, 2, 2, 1, 3, 4, "pose"), (1, 1, 1, 3, 3, 4, "motion")])
def test_rank_deficient(K, n, m, t, C, V, mode):
    """P = 20 (motion: 19) < d = 75, and P = 2: one sample of two frames, two samples of one frame, one sample of two
    frame differences"""
    _, _, real, fake, refs = case(1, K, n, m, t, C, V)
    fr = t - (mode == "motion")
    check_stages(run(real, fake, mode), *refs[mode], n * fr, m * fr, C * V)


def test_one_point_is_rejected():
    _, _, real, fake, _ = case(1, 2, 1, 1, 2, 3, 4)
    with pytest.raises(RuntimeError, match="n=1 gives P=1 < 2 real points"):
        run(real, fake, "motion")


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
def test_constant_real_set(mode):
    """every real point of class 1 is the same: S_r = 0 exactly, T = 0, FD = |dmu|^2 + tr S_f, no NaN"""
    real, fake, _, _, _ = case(1, 3, 5, 7, 9, 3, 25)
    real = real.copy()
    if mode == "pose":
        real[1] = real[1, 0, :, 0][None, :, None, :]
    else:                                                   # a constant velocity: every frame difference is 1 / 128
        real[1] = (np.arange(9, dtype=np.float32) / np.float32(128))[None, None, :, None]
    out = run(torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda(), mode)
    o = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(np.isfinite(o[k]).all() for k in ALL_KEYS)
    assert not o["cov_real"][1].any() and o["terms"][1, 1] == 0 and o["terms"][1, 3] == 0
    assert o["sweeps"][1].tolist() == [1, 1]
    R, F = frechet_def.points(real[1], mode), frechet_def.points(fake[1], mode)
    assert np.array_equal(o["mu_real"][1], R[0])
    mu_f, S_f = frechet_def.moments(F)
    want = ((R[0] - mu_f) ** 2).sum() + np.trace(S_f)
    assert abs(o["values"][1] - want) <= 1e-12 * want
    assert o["values"][1] == (o["terms"][1, 0] + o["terms"][1, 1]) + o["terms"][1, 2]
    per, _ = frechet_def.reference(real[[0, 2]], fake[[0, 2]], mode)          # the neighbours are untouched
    for c, ref in zip((0, 2), per):
        assert abs(o["values"][c] - ref["fd"]) <= 1e-4 * ref["scale"]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("n,t,C,V", [(40, 8, 3, 4), (20, 16, 3, 25)])
def test_closed_forms_on_the_device(n, t, C, V):
    """identical sets: 0; F = R + b: |b|^2; F = s R: (1 - s)^2 (|mu|^2 + tr S) - the expected values come from np.mean /
    np.cov alone, not from the definition's eigen route; the tolerance is the end-to-end bracket of each pair"""
    R, b, sets = frechet_def.closed_form_pairs(n, t, C, V)
    forms = {"identical": lambda mu, S: 0.0, "shift": lambda mu, S: float((b.astype(np.float64) ** 2).sum()),
             "scale": lambda mu, S: 0.25 * (mu @ mu + np.trace(S))}
    for name, F in sets.items():
        closed = forms[name]
        for mode in MODES:
            if name == "shift" and mode == "motion":
                closed_m = lambda mu, S: 0.0                # noqa: E731  (a constant shift has no motion)
            else:
                closed_m = closed
            per, _ = bounds(R[None], F[None], mode)
            mu, S = frechet_def.moments(frechet_def.points(R, mode))
            want = closed_m(mu, S)
            out = run(torch.from_numpy(R[None]).cuda(), torch.from_numpy(F[None]).cuda(), mode)
            got = out["values"].item()
            print(name, mode, got, want, per[0]["tol"]["e2e"])
            assert abs(got - want) <= per[0]["tol"]["e2e"]
            assert (out["sweeps"] < 40).all()


def _batches(K=3, n=8, m=6, C=3, T=6, V=5, seed=3):
    real, fake = frechet_def.make_data(seed, K, n, m, C, T, V)
    return torch.from_numpy(real.reshape(K * n, C, T, V)).cuda(), torch.from_numpy(fake.reshape(K * m, C, T, V)).cuda(), \
        np.repeat(np.arange(K), n), np.repeat(np.arange(K), m)


def _interleave(labels, seed):
    """positions that spread the classes unevenly over the batch but keep every class's samples in their order"""
    mixed = np.random.RandomState(seed).permutation(labels)
    src = np.empty(labels.size, dtype=np.int64)
    for c in np.unique(labels):
        src[np.flatnonzero(mixed == c)] = np.flatnonzero(labels == c)
    return src, mixed


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
def test_strided_inputs(mode, monkeypatch):
    """a crop in T of a longer tensor (read in place), classes interleaved by a label permutation (gathered once), evenly
    spaced samples (read in place), numpy / CPU inputs: all give the bits of the contiguous call"""
    real, gen, lab_r, lab_g = _batches()
    seen = []
    plain = _native.frechet

    def spy(rv, gv, *args, **kw):
        seen.append((rv, gv, args))
        return plain(rv, gv, *args, **kw)

    monkeypatch.setattr(_native, "frechet", spy)
    base = metrics.frechet(gen, real, lab_g, lab_r, mode=mode, moments=True)
    rv, gv, args = seen[-1]
    assert rv.t.data_ptr() == real.data_ptr() and gv.t.data_ptr() == gen.data_ptr()         # grouped: no copy
    assert args[:7] == (8, 6, 6, mode == "motion", 3, 5, 3)
    g = torch.Generator(device="cuda").manual_seed(0)
    long_r = torch.randn((real.shape[0], 3, 9, 5), device="cuda", generator=g)
    long_g = torch.randn((gen.shape[0], 3, 9, 5), device="cuda", generator=g)
    long_r[:, :, 2:8], long_g[:, :, :6] = real, gen
    out = metrics.frechet(long_g[:, :, :6], long_r[:, :, 2:8], lab_g, lab_r, mode=mode, moments=True)
    rv, gv, _ = seen[-1]
    assert rv.t.data_ptr() == long_r[:, :, 2:8].data_ptr() and gv.t.data_ptr() == long_g.data_ptr()    # cropped: no copy
    assert rv.so == 9 * 5 and rv.sf == 5 and rv.ss == 3 * 9 * 5
    same_bits(out, base)
    # classes interleaved unevenly: gathered
    src_r, mix_r = _interleave(lab_r, 3)
    src_g, mix_g = _interleave(lab_g, 4)
    out = metrics.frechet(gen[torch.as_tensor(src_g).cuda()], real[torch.as_tensor(src_r).cuda()], mix_g, np.eye(3)[mix_r],
                          mode=mode, moments=True)
    rv, gv, _ = seen[-1]
    assert rv.ss == 3 * 6 * 5 and rv.sc == 8 * rv.ss and gv.sc == 6 * gv.ss
    same_bits(out, base)
    # per_class: the first 4 of each class, classes interleaved evenly: read in place
    il_r = real.reshape(3, 8, 3, 6, 5).transpose(0, 1).reshape(-1, 3, 6, 5).contiguous()
    il_g = gen.reshape(3, 6, 3, 6, 5).transpose(0, 1).reshape(-1, 3, 6, 5).contiguous()
    out = metrics.frechet(il_g, il_r, np.tile(np.arange(3), 6), np.tile(np.arange(3), 8), mode=mode, per_class=4, moments=True)
    rv, gv, args = seen[-1]
    assert rv.t.data_ptr() == il_r.data_ptr() and gv.t.data_ptr() == il_g.data_ptr() and args[0:2] == (4, 4)
    assert rv.ss == 3 * 90 and rv.sc == 90
    want = metrics.frechet(gen.reshape(3, 6, 3, 6, 5)[:, :4].reshape(-1, 3, 6, 5), real.reshape(3, 8, 3, 6, 5)[:, :4]
                           .reshape(-1, 3, 6, 5), np.repeat(np.arange(3), 4), np.repeat(np.arange(3), 4), mode=mode, moments=True)
    same_bits(out, want)
    # numpy / CPU inputs and id labels on the device
    out = metrics.frechet(gen.cpu().numpy(), real.cpu(), torch.as_tensor(lab_g).cuda(), lab_r, mode=mode, moments=True)
    same_bits(out, base)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
def test_deterministic_and_workspace_contents_do_not_matter(mode):
    """two calls give the same bits; a reused workspace filled with either guard pattern (a NaN word, zeros) too"""
    _, _, real, fake, _ = case(1, 1, 37, 29, 64, 3, 25)
    a, b = run(real, fake, mode), run(real, fake, mode)
    same_bits(a, b)
    words = _native.frechet_workspace_bytes(37, 29, 64, mode == "motion", 3, 25, 1) // 4
    for fill in (guard.PATTERN_A, 0):
        ws = guard.full((words,), fill, dtype=torch.int32, device="cuda").view(torch.float64)     # red-zoned like the outputs
        same_bits(run(real, fake, mode, ws=ws), a)
        same_bits(run(real, fake, mode, ws=ws), a)                                              # and what the call itself left
    _, _, real3, fake3, _ = case(1, 3, 5, 7, 9, 3, 25)
    same_bits(run(real3, fake3, mode), run(real3, fake3, mode))


def test_graph_capture_replays_on_new_inputs():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    real, gen, lab_r, lab_g = _batches(K=4, n=10, m=9, seed=2)
    real2, gen2, _, _ = _batches(K=4, n=10, m=9, seed=5)
    before = metrics.frechet(gen, real, lab_g, lab_r, mode="pose")["values"].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.frechet(gen, real, lab_g, lab_r, mode="both", moments=True)                # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = metrics.frechet(gen, real, lab_g, lab_r, mode="both", moments=True)
    real.copy_(real2)
    gen.copy_(gen2)
    g.replay()
    torch.cuda.synchronize()
    eager = metrics.frechet(gen2, real2, lab_g, lab_r, mode="both", moments=True)
    for mode in MODES:
        same_bits(cap[mode], eager[mode])
    assert not torch.equal(eager["pose"]["values"], before)           # (the two inputs do score differently)


@pytest.mark.usefixtures("guarded")
def test_metrics_frechet_both_and_features():
    """4 classes x 10 samples, T 16, V 25 as (N, C, T, V) batches with labels, against the definition; the frames handed
    over as an (N T, 75) feature matrix give the pose result bit for bit"""
    K, n, C, T, V = 4, 10, 3, 16, 25
    real, fake, real_g, fake_g, refs = case(1, K, n, n, T, C, V)
    lab = np.repeat(np.arange(K), n)
    out = metrics.frechet(fake_g.reshape(K * n, C, T, V), real_g.reshape(K * n, C, T, V), lab, np.eye(K)[lab], mode="both",
                          moments=True)
    assert sorted(out) == ["motion", "pose"]
    for mode in MODES:
        fr = T - (mode == "motion")
        check_stages(out[mode], *refs[mode], n * fr, n * fr, C * V)
        assert out[mode]["mean"].shape == () and out[mode]["values"].shape == (K,) and out[mode]["terms"].shape == (K, 4)
        assert out[mode]["sweeps"].shape == (K, 2) and out[mode]["cov_real"].shape == (K, 75, 75)
    assert out["pose"]["values"].dtype == torch.float64 and out["pose"]["sweeps"].dtype == torch.int32
    feat_r = real_g.permute(0, 1, 3, 2, 4).reshape(K * n * T, C * V)
    feat_f = fake_g.permute(0, 1, 3, 2, 4).reshape(K * n * T, C * V)
    flab = np.repeat(np.arange(K), n * T)
    feat = metrics.frechet_features(feat_f, feat_r, flab, flab, moments=True)
    same_bits(feat, out["pose"])
    plain = metrics.frechet_features(feat_f, feat_r, flab, flab)
    assert sorted(plain) == ["mean", "sweeps", "terms", "values"]
    same_bits(plain, out["pose"], ("values", "terms", "sweeps", "mean"))


def test_frechet_actions_tool_end_to_end(tmp_path):
    """tools/frechet_actions.py on a small H36M-shaped .npy / .pkl quadruple: selection, normalisation, metrics.frechet"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import frechet_actions
    rng = np.random.RandomState(0)
    n, C, T, V = 400, 3, 12, 16
    lab = rng.permutation(np.repeat(np.arange(10), n // 10))
    latent = rng.normal(size=(n, T, 6)) + lab[:, None, None]
    mix = rng.normal(size=(6, C * V))
    real = (latent @ mix + 0.3 * rng.normal(size=(n, T, C * V))).reshape(n, T, C, V).transpose(0, 2, 1, 3)
    real = np.ascontiguousarray(real.astype(np.float32))
    lo, hi = real.min(), real.max()
    fake = (2 * ((real - lo) / (hi - lo)) - 1)[::-1] * 0.9 + rng.normal(0, 0.02, size=real.shape)
    fake, fake_lab = np.ascontiguousarray(fake.astype(np.float32)), lab[::-1].copy()
    for nm, d, lb in (("real", real, lab), ("fake", fake, fake_lab)):
        np.save(tmp_path / (nm + ".npy"), d)
        with open(tmp_path / (nm + ".pkl"), "wb") as f:
            pickle.dump(([str(i) for i in range(n)], lb.tolist()), f)
    argv = ["--data_real", str(tmp_path / "real.npy"), "--labels_real", str(tmp_path / "real.pkl"),
            "--data_fake", str(tmp_path / "fake.npy"), "--labels_fake", str(tmp_path / "fake.pkl"),
            "--t_size", "8", "--dataset", "h36m", "--per_class", "20", "--per_class_table"]
    got = frechet_actions.main(argv)
    r_idx = mmd_def.select_scan(lab, list(range(10)), per_class=20)
    f_idx = mmd_def.select_scan(fake_lab, list(range(10)), per_class=20)
    sel_real = (2 * ((real[r_idx][:, :, :8] - lo) / (hi - lo)) - 1).astype(np.float32)
    sel_fake = fake[f_idx][:, :, :8]
    labels = np.repeat(np.arange(10), 20)
    want = metrics.frechet(sel_fake, sel_real, labels, labels, mode="both")
    assert got == (float(want["pose"]["mean"].cpu()), float(want["motion"]["mean"].cpu()))
    assert len(got) == 2 and all(np.isfinite(v) and v > 0 for v in got)
    for mode in MODES:
        per, mean = bounds(sel_real.reshape(10, 20, C, 8, V), sel_fake.reshape(10, 20, C, 8, V), mode)
        assert abs(float(want[mode]["mean"].cpu()) - mean) <= max(p["tol"]["e2e"] for p in per)
    one = frechet_actions.main(argv[:-1] + ["--unconditional"])
    want1 = metrics.frechet(sel_fake, sel_real, mode="both")
    assert one == (float(want1["pose"]["mean"].cpu()), float(want1["motion"]["mean"].cpu()))
