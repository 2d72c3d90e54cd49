"""kg_mmd on the MI355X: MMD^2 of every (group, bandwidth) against the float64 definition (tests/mmd_def.py) in both
kernel regimes, strided inputs, the finishing rules, the reference fixtures (tests/golden/mmd_ref.npz), determinism
and graph capture."""
import os

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native
from kinetic_gan_amd import metrics

import mmd_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)

pytestmark = pytest.mark.gpu
BWS = mmd_def.BANDWIDTHS


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


def check_mmd2(got, x, y, bws=BWS):
    """got (G, nbw) kernel MMD^2; x, y (G, m, dim): |hip - f64| <= 1e-5 sum_{i != j}(kxx + kyy + 2 kxy)_f64 / (m (m-1)),
    plus the part no fp32 distance avoids far in the kernel's tail (d / bw >> 1): 4 eps32 sqrt(dim) x the distance
    sensitivity (mmd_def.pair_sums_batched); where d / bw <= 1 the first term is the larger one"""
    m, dim = x.shape[1], x.shape[2]
    S, A, B = mmd_def.pair_sums_batched(x, y, bws, with_tail=True)
    want = S / (m * (m - 1))
    tol = (1e-5 * A + 4 * mmd_def.EPS32 * dim ** 0.5 * B) / (m * (m - 1)) + 1e-37
    err = (got.double() - want).abs()
    assert torch.isfinite(got).all()
    bad = err > tol
    if bad.any():
        g, b = (int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError("group %d bw %g: got %g want %g tol %g" % (g, bws[b], got[g, b].item(), want[g, b].item(),
                                                                        tol[g, b].item()))
    return want, tol


def check_frame_mean(got, want, tol):
    """got (K, nbw) kernel MMD; want / tol (K, F, nbw) float64 MMD^2 and its tolerance: the mean over frames of sqrt,
    compared where the sign of every frame's MMD^2 is decided (|MMD^2| > 10 tol): NaN exactly where one is negative"""
    sure = (want.abs() > 10 * tol).all(1)
    per = torch.where(want >= 0, want.clamp_min(0).sqrt(), torch.full_like(want, float("nan"))).mean(1)
    got = got.double()
    assert sure.any()
    assert torch.equal(torch.isnan(got)[sure], torch.isnan(per)[sure])
    fin = sure & torch.isfinite(per)
    assert ((got - per).abs()[fin] <= 1e-4 * per[fin] + 1e-6).all()


def nctv_groups(t, mode):
    """(K, C, T, V) -> (K*T, V, C) avg groups or (K, V, C*T) joint groups (float64, the definition's layout)"""
    K, C, T, V = t.shape
    if mode == "avg":
        return t.permute(0, 2, 3, 1).reshape(K * T, V, C).double()
    return t.permute(0, 3, 1, 2).reshape(K, V, C * T).double()


def run_nctv(x, y, mode, bws=BWS):
    K, C, T, V = x.shape
    views = []
    for t in (x, y):
        if mode == "avg":
            views.append(_native.MmdView(t, t.stride(3), t.stride(1), t.stride(2), t.stride(0)))
        else:
            views.append(_native.MmdView(t, t.stride(3), t.stride(2), 0, t.stride(0)))
    dim, groups = (C, T) if mode == "avg" else (C * T, 1)
    return _native.mmd(views[0], views[1], V, V, dim, groups, K, bws, want_mean=True)


def rand_pair(shape, seed, spread=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(shape, device="cuda", generator=g) * 2 - 1
    y = (x * 1.15 + 0.1 * torch.randn(shape, device="cuda", generator=g)) * spread
    return x, y


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("K,C,T,V,mode", [(10, 2, 32, 16, "avg"), (60, 3, 64, 25, "avg"), (60, 3, 64, 25, "joint"),
                                          (3, 3, 1024, 16, "avg")])
def test_protocol_shapes_against_f64(K, C, T, V, mode):
    """regime (a): the reference protocol read straight from (N, C, T, V) (m = 16 / 25, dim = C or C*T)"""
    x, y = rand_pair((K, C, T, V), seed=K + T)
    out = run_nctv(x, y, mode)
    torch.cuda.synchronize()
    want, tol = check_mmd2(out["mmd2"], nctv_groups(x, mode), nctv_groups(y, mode))
    groups = T if mode == "avg" else 1
    check_frame_mean(out["mmd"], want.reshape(K, groups, len(BWS)), tol.reshape(K, groups, len(BWS)))


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("m,dim,G", [(1000, 75, 64), (1000, 4800, 1), (777, 33, 3)])
def test_sample_sets_against_f64(m, dim, G):
    """regime (b): few large groups, (N, L, D) sample sets: groups = frames (avg) or the flattened set (G = 1)"""
    x, y = rand_pair((m, G, dim), seed=m + dim, spread=1.0)
    scale = 1.0 / dim      # keep some bandwidths of the sweep away from both saturation ends
    x, y = x * scale ** 0.5 * 4, y * scale ** 0.5 * 4
    xv = _native.MmdView(x, x.stride(0), x.stride(2), x.stride(1), 0)
    yv = _native.MmdView(y, y.stride(0), y.stride(2), y.stride(1), 0)
    out = _native.mmd(xv, yv, m, m, dim, G, 1, BWS)
    torch.cuda.synchronize()
    check_mmd2(out["mmd2"], x.permute(1, 0, 2), y.permute(1, 0, 2))


@pytest.mark.usefixtures("guarded")
def test_strided_inputs():
    """non-contiguous operands: a permuted (L, N, D) storage, every other point of a larger set, a sliced frame range"""
    base_x, base_y = rand_pair((40, 2 * 90, 7), seed=3)          # (L, 2N, D)
    x = base_x.permute(1, 0, 2)[::2]                             # (N=90, L=40, D=7), point stride 2*7, frame stride 2*90*7
    y = base_y.permute(1, 0, 2)[1::2]
    assert not x.is_contiguous()
    got = metrics.mmd_sweep(x, y, BWS, "avg")
    S, A = mmd_def.pair_sums_batched(x.permute(1, 0, 2), y.permute(1, 0, 2), BWS)
    check_frame_mean(got[None], (S / (90 * 89))[None], (1e-5 * A / (90 * 89))[None])
    # feeder tensor cropped in time (a view: frame stride V, channel stride T_full*V)
    full_x, full_y = rand_pair((10, 3, 50, 16), seed=4)
    cx, cy = full_x[:, :, :32], full_y[:, :, :32]
    out = run_nctv(cx, cy, "avg")
    check_mmd2(out["mmd2"], nctv_groups(cx, "avg"), nctv_groups(cy, "avg"))


@pytest.mark.usefixtures("guarded")
def test_finish_rules():
    """a negative MMD^2 frame makes its bandwidth NaN; a class with NaN at every bandwidth scores 0; m = 1 is NaN"""
    a, b = [0.0, 0.0], [1.0, 0.0]
    # class 0: frame 0 has Y = X swapped (MMD^2 < 0), frame 1 an ordinary pair; class 1: both frames swapped
    x = torch.tensor([[a, b], [a, b], [a, b], [a, b]], device="cuda")                    # (class*frame, m=2, dim=2)
    y = torch.tensor([[b, a], [[5.0, 5.0], [6.0, 5.0]], [b, a], [b, a]], device="cuda")
    x, y = x.reshape(2, 2, 2, 2), y.reshape(2, 2, 2, 2)                                   # (class, frame, point, dim)
    bws = [0.1, 1.0, 10.0]
    views = [_native.MmdView(t, t.stride(2), t.stride(3), t.stride(1), t.stride(0)) for t in (x, y)]
    out = _native.mmd(views[0], views[1], 2, 2, 2, 2, 2, bws, want_mean=True)
    torch.cuda.synchronize()
    mmd2 = out["mmd2"].reshape(2, 2, 3)
    assert (mmd2[0, 0] < 0).all() and (mmd2[1] < 0).all() and (mmd2[0, 1] > 0).all()
    assert torch.isnan(out["mmd"]).all()
    assert out["result"].tolist() == [0.0, 0.0] and out["mean"].item() == 0.0
    # class 0 with only the ordinary frame: its best bandwidth wins
    y2 = y.clone()
    y2[0, 0] = y[0, 1]
    x2 = x.clone()
    views = [_native.MmdView(t, t.stride(2), t.stride(3), t.stride(1), t.stride(0)) for t in (x2, y2)]
    out = _native.mmd(views[0], views[1], 2, 2, 2, 2, 2, bws, want_mean=True)
    r = out["result"].tolist()
    assert r[0] == pytest.approx(float(np.nanmax(out["mmd"][0].cpu().numpy()))) and r[0] > 0 and r[1] == 0.0
    assert out["mean"].item() == pytest.approx(r[0] / 2, rel=1e-6)
    # m = 1: 0 / 0
    one = guard.zeros(1, 1, 3, device="cuda")
    assert np.isnan(metrics.mmd_sweep(one, one + 1, bws, "avg").cpu().numpy()).all()
    assert metrics.calculate_mmd(torch.zeros(2, 3, 4, 1), torch.ones(2, 3, 4, 1), [0, 1], "avg").item() == 0.0


def _fixture(golden_dir, name):
    d = np.load(os.path.join(golden_dir, "mmd_ref.npz"))
    real = d[name + "_real_q"].astype(np.float32) / np.float32(127)
    lab = d[name + "_labels"]
    fake = (real * d[name + "_fake_scale"][lab][:, None, None, None]
            + d[name + "_fake_shift"][lab][:, None, None, None]).astype(np.float32)
    return fake, real, lab, d


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("name", ["h36m", "ntu"])
@pytest.mark.parametrize("mode", ["avg", "joint"])
def test_reference_fixtures(golden_dir, name, mode):
    """calculate_mmd and MMD.compute_sequence_mmd against the reference's own outputs: rel 1e-4 on the final value and
    on every bandwidth where the reference's fp32 value is >= 100 x its roundoff"""
    fake, real, lab, d = _fixture(golden_dir, name)
    ref_seq, ref_calc = d["%s_seq_%s" % (name, mode)], float(d["%s_calc_%s" % (name, mode)])
    mean, result, per_bw = metrics.calculate_mmd(torch.tensor(fake).cuda(), torch.tensor(real).cuda(), lab, mode,
                                                 per_class=True)
    assert abs(mean.item() - ref_calc) <= 1e-4 * ref_calc, (mean.item(), ref_calc)
    one_hot = np.eye(ref_seq.shape[0])[lab]
    assert metrics.calculate_mmd(fake, real, one_hot, mode).item() == mean.item()      # the reference's label form
    per_bw = per_bw.cpu().numpy()
    mm = metrics.MMD(mode)
    checked = 0
    for c in range(ref_seq.shape[0]):
        i = int(np.flatnonzero(lab == c)[0])
        g0 = torch.tensor(fake[i]).permute(2, 1, 0)
        r0 = torch.tensor(real[i]).permute(2, 1, 0)
        err = mmd_def.sequence_roundoff(g0, r0, BWS, mode)
        ok = np.abs(ref_seq[c]) > 100 * err
        for b in np.flatnonzero(ok):
            assert abs(per_bw[c, b] - ref_seq[c, b]) <= 1e-4 * abs(ref_seq[c, b]), (c, b, per_bw[c, b], ref_seq[c, b])
            checked += 1
        b = int(np.nanargmax(ref_seq[c]))
        v = mm.compute_sequence_mmd(g0.cuda(), r0.cuda(), BWS[b])
        assert isinstance(v, float) and abs(v - ref_seq[c, b]) <= 1e-4 * ref_seq[c, b]
        assert result[c].item() == float(np.nanmax(per_bw[c]))
    assert checked >= 2 * ref_seq.shape[0]


def test_sorted_batch_reads_in_place_and_agrees(golden_dir):
    """a batch ordered class by class (the selection's layout) is read in place and gives the gathered result's bits"""
    fake, real, lab, _ = _fixture(golden_dir, "h36m")
    order = np.argsort(lab, kind="stable")
    a = metrics.calculate_mmd(torch.tensor(fake).cuda(), torch.tensor(real).cuda(), lab, "avg")
    b = metrics.calculate_mmd(torch.tensor(fake[order]).cuda(), torch.tensor(real[order]).cuda(), lab[order], "avg")
    assert a.item() == b.item()


@pytest.mark.usefixtures("guarded")
def test_rkhs_mmd_matches_definition():
    x, y = rand_pair((50, 6), seed=9)
    v = metrics.MMD("avg").rkhs_mmd(x, y, 1.0)
    want = mmd_def.mmd2(x, y, [1.0]).item()
    assert abs(v - want ** 0.5) <= 1e-5 * want ** 0.5


def test_deterministic():
    for shape, mode in (((60, 3, 64, 25), "avg"), ((4, 3, 64, 1000), "joint")):
        x, y = rand_pair(shape, seed=11)
        a, b = run_nctv(x, y, mode), run_nctv(x, y, mode)
        torch.cuda.synchronize()
        for k in ("mmd2", "mmd", "result", "mean"):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_graph_capture_replays_same_bits(golden_dir):
    fake, real, lab, _ = _fixture(golden_dir, "ntu")
    gen, rl = torch.tensor(fake).cuda(), torch.tensor(real).cuda()
    seq1, seq2 = rand_pair((1000, 8, 75), seed=12)
    eager = (metrics.calculate_mmd(gen, rl, lab, "avg"), metrics.mmd_sweep(seq1, seq2, BWS, "joint"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.calculate_mmd(gen, rl, lab, "avg")                  # warm-up on the capture stream
        metrics.mmd_sweep(seq1, seq2, BWS, "joint")
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = (metrics.calculate_mmd(gen, rl, lab, "avg"), metrics.mmd_sweep(seq1, seq2, BWS, "joint"))
    g.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, cap):
        assert torch.equal(e.view(torch.int32), c.view(torch.int32))


def test_unequal_sets_raise():
    x, y = rand_pair((20, 4, 3), seed=13)
    with pytest.raises(ValueError, match="m=20 != n=19"):
        metrics.mmd_sweep(x, y[:19], BWS, "avg")
    xv = _native.MmdView(x, x.stride(0), x.stride(2), x.stride(1), 0)
    with pytest.raises(RuntimeError, match="m=20 != n=19"):
        _native.mmd(xv, xv, 20, 19, 3, 4, 1, BWS)


def test_mmd_actions_tool_end_to_end(tmp_path):
    """tools/mmd_actions.py on a small H36M-shaped .npy / .pkl pair: selection, normalisation and the one-call score"""
    import pickle
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mmd_actions
    rng = np.random.RandomState(0)
    n, C, T, V = 1050, 3, 12, 16
    lab = rng.permutation(np.repeat(np.arange(10), n // 10))
    real = rng.uniform(-3, 5, size=(n, C, T, V)).astype(np.float32)
    fake = np.clip(real / 4 + rng.normal(0, 0.1, size=real.shape), -1, 1).astype(np.float32)
    for nm, d in (("real", real), ("fake", fake)):
        np.save(tmp_path / (nm + ".npy"), d)
        with open(tmp_path / (nm + ".pkl"), "wb") as f:
            pickle.dump(([str(i) for i in range(n)], lab.tolist()), f)
    argv = ["--data_real", str(tmp_path / "real.npy"), "--labels_real", str(tmp_path / "real.pkl"),
            "--data_fake", str(tmp_path / "fake.npy"), "--labels_fake", str(tmp_path / "fake.pkl"),
            "--mmd_mode", "avg", "--t_size", "8", "--dataset", "h36m"]
    got = mmd_actions.main(argv)
    # the same score from the scan-order selection and the float64 definition
    r_idx = mmd_def.select_scan(lab, list(range(10)))
    sel_real = 2 * ((real[r_idx][:, :, :8] - real.min()) / (real.max() - real.min())) - 1
    sel_fake = fake[r_idx][:, :, :8]
    want, _, _ = mmd_def.calculate_mmd(torch.tensor(sel_fake).double(), torch.tensor(sel_real).double(),
                                       lab[r_idx], "avg")
    assert abs(got - want) <= 1e-4 * want, (got, want)
