"""kg_prdc on the MI355X: counts, per-point flags / hits and radii against the float64 definition (tests/prdc_def.py) -
exactly on integer data, inside the derived bracket on real-valued data -, the protocol shapes through metrics.prdc,
strided inputs, determinism, workspace reuse, graph capture and the command-line tool.

Error model (prdc_def): tau_D = (D + 3) 2^-24 bounds the relative error of every fp32 distance and radius; the counts
under the tight and the loose predicate are `lo` and `hi`, and `hi - lo <= max(1, 0.01 exact)` is asserted on the float64
definition BEFORE the kernel's output is looked at."""
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

import mmd_def
import prdc_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)

pytestmark = pytest.mark.gpu
PER_POINT = ("radii_real", "radii_fake", "fake_hits", "real_flags")
ALL_KEYS = ("counts", "values", "mean") + PER_POINT


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


@functools.lru_cache(maxsize=None)
def case(seed, classes, n, m, D, k, integer=False):
    """(R, F) fp32 on the GPU and their float64 reference (with the bracket unless the data is integer); computed once"""
    R, F = (t.cuda() for t in prdc_def.make_data(seed, classes, n, m, D, integer=integer))
    ref = prdc_def.reference(R, F, k, 0.0 if integer else prdc_def.tau(D))
    return R, F, ref


def run_sets(R, F, k, per_point=True, ws=None):
    """R (K, n, D), F (K, m, D) contiguous -> the output dict of _native.prdc"""
    K, n, D = R.shape
    m = F.shape[1]
    return _native.prdc(_native.PrdcView(R, R.stride(0), R.stride(1), 0), _native.PrdcView(F, F.stride(0), F.stride(1), 0),
                        n, m, 1, D, K, k, want_mean=True, per_point=per_point, ws=ws)


def same_bits(a, b, keys):
    for key in keys:
        x, y = a[key], b[key]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), key


def check_exact(out, ref):
    assert torch.equal(out["counts"].long(), ref["counts"])
    assert torch.equal(out["fake_hits"].long(), ref["fake_hits"])
    assert torch.equal(out["real_flags"], ref["real_flags"])
    assert torch.equal(out["radii_real"].double(), ref["radii_real"])
    assert torch.equal(out["radii_fake"].double(), ref["radii_fake"])


def check_bracket(out, ref, D, k):
    ok, width = prdc_def.bracket_is_narrow(ref)
    assert ok, "the bracket is too wide at this shape and seed to test anything: hi - lo = %s" % width.tolist()
    got = out["counts"].long()
    print("counts", got.tolist(), "lo", ref["counts_lo"].tolist(), "hi", ref["counts_hi"].tolist())
    assert (ref["counts_lo"] <= got).all() and (got <= ref["counts_hi"]).all()
    hits = out["fake_hits"].long()
    assert (ref["fake_hits_lo"] <= hits).all() and (hits <= ref["fake_hits_hi"]).all()      # equal wherever lo == hi
    fl, lo, hi = out["real_flags"], ref["real_flags_lo"], ref["real_flags_hi"]
    assert ((fl & lo) == lo).all() and ((fl | hi) == hi).all()                              # equal wherever lo == hi
    t = prdc_def.tau(D)
    for key in ("radii_real", "radii_fake"):
        err = (out[key].double() - ref[key]).abs()
        assert (err <= t * ref[key] + 1e-30).all(), (key, (err / ref[key]).max().item(), t)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("classes,n,m,D,k", [(1, 40, 40, 6, 3), (3, 37, 53, 75, 5), (1, 20, 20, 3, 19), (1, 130, 70, 48, 4)])
def test_exact_on_integer_data(classes, n, m, D, k):
    """integer coordinates in [-8, 8], D * 256 < 2^24: every fp32 distance and comparison is exact, '<=' ties abound"""
    R, F, ref = case(0, classes, n, m, D, k, integer=True)
    out = run_sets(R, F, k)
    check_exact(out, ref)


@pytest.mark.usefixtures("guarded")
def test_exact_duplicate_real_and_fake_on_a_real():
    """real sample 1 duplicates real sample 0 and fake 0 equals them: radius 0 (the duplicate is a neighbour: left out by
    index, not by value) and the pair counts through 0 <= 0"""
    R, F, _ = case(0, 1, 40, 40, 6, 3, integer=True)
    R, F = R.clone(), F.clone()
    R[0, 1] = R[0, 0]
    F[0, 0] = R[0, 0]
    ref = prdc_def.reference(R, F, 1)
    assert ref["radii_real"][0, 0] == 0 and ref["radii_real"][0, 1] == 0 and ref["fake_hits"][0, 0] >= 2
    out = run_sets(R, F, 1)
    check_exact(out, ref)


def tile_edges(classes, n, m):
    """(radii, cross) tile edges by the rule of prdc_plan in csrc/kg_prdc.hip: a launch takes the 64-tile once that alone
    makes 512 workgroups - one per ROW tile of either set for the radii, one per tile of R x F for the cross launch"""
    c64 = lambda v: -(-v // 64)      # noqa: E731
    return (64 if classes * (c64(n) + c64(m)) >= 512 else 32), (64 if classes * c64(n) * c64(m) >= 512 else 32)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("classes,n,m,D,k,edges", [(24, 700, 650, 6, 5, (64, 64)), (1, 1500, 1400, 48, 4, (32, 64))])
def test_exact_on_integer_data_64_tiles(classes, n, m, D, k, edges):
    """the shapes above all run on 32-tiles (2 x 2 pairs per thread).  These select the 64-tile kernels (4 x 4 pairs, four
    ranking threads per row): 24 x (700 + 650) in both launches (528 row tiles, 2904 tiles), 1 x (1500 + 1400) in the cross
    launch only (46 row tiles, 528 tiles).  Ragged last tiles in both (700 = 10 * 64 + 60, 1500 = 23 * 64 + 28: two waves
    of the last row tile have no row); integer data, so counts, hits, flags and radii are compared with no tolerance"""
    assert tile_edges(classes, n, m) == edges
    R, F, ref = case(0, classes, n, m, D, k, integer=True)
    assert len(torch.unique(ref["radii_real"])) > 3 and 0 < ref["counts"][:, 1].min() and ref["counts"][:, 1].max() < n
    out = run_sets(R, F, k)
    check_exact(out, ref)


@pytest.mark.usefixtures("guarded")
def test_bracket_64_tiles():
    """real-valued data on the 64-tile kernels of both launches: 24 classes of 700 + 650 points"""
    assert tile_edges(24, 700, 650) == (64, 64)
    R, F, ref = case(0, 24, 700, 650, 33, 5)
    check_bracket(run_sets(R, F, 5), ref, 33, 5)


BRACKET_SHAPES = [(37, 53, 7, 3), (37, 53, 75, 5), (64, 64, 33, 1), (100, 100, 75, 5), (300, 260, 75, 5), (33, 47, 1536, 3),
                  (100, 100, 4800, 5)]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n,m,D,k", BRACKET_SHAPES)
def test_bracket(n, m, D, k, seed):
    R, F, ref = case(seed, 1, n, m, D, k)
    check_bracket(run_sets(R, F, k), ref, D, k)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("classes,n,m,D,k", [(3, 100, 100, 4800, 5), (1, 1000, 900, 75, 5)])
def test_bracket_classes_and_multi_tile(classes, n, m, D, k):
    R, F, ref = case(0, classes, n, m, D, k)
    check_bracket(run_sets(R, F, k), ref, D, k)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("K,C,T,V,seed", [(60, 3, 64, 25, 35), (10, 2, 32, 16, 0)])
def test_protocol_shapes_through_metrics(K, C, T, V, seed):
    """the evaluation protocol's 100 + 100 samples per class, as (N, C, T, V) batches with labels, through metrics.prdc.
    Class c draws from seed + c; base seed 35 for the 60 classes because the float64 definition alone says that class seed
    34 has a bracket of 2 on cR (the cap is 1) while 35 .. 94 are all inside the cap"""
    D = C * T * V
    R, F, ref = case(seed, K, 100, 100, D, 5)
    lab = np.repeat(np.arange(K), 100)
    out = metrics.prdc(F.reshape(K * 100, C, T, V), R.reshape(K * 100, C, T, V), lab, np.eye(K)[lab], k=5, per_point=True)
    check_bracket(out, ref, D, 5)
    assert out["mean"].shape == (4,) and out["values"].shape == (K, 4) and out["counts"].shape == (K, 4)


@pytest.mark.usefixtures("guarded")
def test_values_and_mean():
    """values = counts / denominators to 1 ulp; mean = the class mean of values to 1e-6 relative"""
    R, F, _ = case(0, 3, 37, 53, 75, 5)
    out = run_sets(R, F, 5, per_point=False)
    want = prdc_def.values_of(out["counts"], 37, 53, 5)
    v = out["values"]
    ulp = torch.maximum(torch.nextafter(v, v + 1) - v, v - torch.nextafter(v, v - 1)).double()
    assert ((v.double() - want).abs() <= ulp).all()
    mean = v.double().mean(0)
    assert ((out["mean"].double() - mean).abs() <= 1e-6 * mean).all()
    assert (v[:, 2].double() * 5 * 53 - out["counts"][:, 2].double()).abs().max() < 1e-3        # density = cD / (k m)


def _batches(K=3, n=24, m=20, C=3, T=6, V=5, seed=1):
    R, F = prdc_def.make_data(seed, K, n, m, C * T * V)
    return R.reshape(K * n, C, T, V).cuda(), F.reshape(K * m, C, T, V).cuda(), np.repeat(np.arange(K), n), \
        np.repeat(np.arange(K), m)


@pytest.mark.usefixtures("guarded")
def test_strided_inputs(monkeypatch):
    """a crop in T of a longer array (d_outer = C, read in place), grouped classes (read in place) and classes shuffled in
    the batch (gathered once) give the bits of the contiguous call"""
    real, gen, lab_r, lab_g = _batches()
    seen = []
    plain = _native.prdc

    def spy(rv, gv, *args, **kw):
        seen.append((rv, gv, args))
        return plain(rv, gv, *args, **kw)

    monkeypatch.setattr(_native, "prdc", spy)
    base = metrics.prdc(gen, real, lab_g, lab_r, k=4, per_point=True)
    rv, gv, args = seen[-1]
    assert rv.t.data_ptr() == real.data_ptr() and gv.t.data_ptr() == gen.data_ptr()         # grouped: no copy
    assert args[2:4] == (1, 3 * 6 * 5)
    # the same samples as the first 6 frames of longer arrays
    g = torch.Generator(device="cuda").manual_seed(0)
    long_r = torch.randn((real.shape[0], 3, 9, 5), device="cuda", generator=g)
    long_g = torch.randn((gen.shape[0], 3, 9, 5), device="cuda", generator=g)
    long_r[:, :, :6], long_g[:, :, :6] = real, gen
    out = metrics.prdc(long_g[:, :, :6], long_r[:, :, :6], lab_g, lab_r, k=4, per_point=True)
    rv, gv, args = seen[-1]
    assert rv.t.data_ptr() == long_r.data_ptr() and gv.t.data_ptr() == long_g.data_ptr()    # cropped: no copy
    assert args[2:4] == (3, 6 * 5) and rv.so == 9 * 5
    same_bits(out, base, ALL_KEYS)
    # one side cropped, the other contiguous
    same_bits(metrics.prdc(gen, long_r[:, :, :6], lab_g, lab_r, k=4, per_point=True), base, ALL_KEYS)
    # classes shuffled in the batch: gathered
    pr, pg = np.random.RandomState(3).permutation(real.shape[0]), np.random.RandomState(4).permutation(gen.shape[0])
    out = metrics.prdc(gen[torch.as_tensor(pg).cuda()], real[torch.as_tensor(pr).cuda()], lab_g[pg], lab_r[pr], k=4)
    rv, gv, _ = seen[-1]
    assert rv.sp == 3 * 6 * 5 and rv.sc == 24 * rv.sp
    # (the shuffle reorders the samples inside a class: the per-class results are permutation-invariant, the per-point
    # arrays are not compared)
    same_bits(out, base, ("counts", "values", "mean"))
    # per_class: the first 10 of each class, classes interleaved (evenly spaced: read in place)
    il_r = real.reshape(3, 24, 3, 6, 5).transpose(0, 1).reshape(-1, 3, 6, 5).contiguous()
    il_g = gen.reshape(3, 20, 3, 6, 5).transpose(0, 1).reshape(-1, 3, 6, 5).contiguous()
    out = metrics.prdc(il_g, il_r, np.tile(np.arange(3), 20), np.tile(np.arange(3), 24), k=4, per_class=10, per_point=True)
    rv, gv, args = seen[-1]
    assert rv.t.data_ptr() == il_r.data_ptr() and args[0:2] == (10, 10)
    want = metrics.prdc(gen.reshape(3, 20, 3, 6, 5)[:, :10].reshape(-1, 3, 6, 5), real.reshape(3, 24, 3, 6, 5)[:, :10]
                        .reshape(-1, 3, 6, 5), np.repeat(np.arange(3), 10), np.repeat(np.arange(3), 10), k=4, per_point=True)
    same_bits(out, want, ALL_KEYS)
    # numpy / CPU inputs and id labels on the device
    out = metrics.prdc(gen.cpu().numpy(), real.cpu(), torch.as_tensor(lab_g).cuda(), lab_r, k=4, per_point=True)
    same_bits(out, base, ALL_KEYS)


@pytest.mark.usefixtures("guarded")
def test_deterministic_and_workspace_cleared_by_the_call():
    """two calls give the same bits; a call that reuses the workspace of a call on OTHER data is unaffected by what that
    call left there (the radii launch clears what the cross launch accumulates into)"""
    R, F, _ = case(0, 3, 100, 100, 4800, 5)
    a, b = run_sets(R, F, 5), run_sets(R, F, 5)
    same_bits(a, b, ALL_KEYS)
    R2, F2, _ = case(1, 3, 100, 100, 4800, 5)
    words = _native.prdc_workspace_bytes(100, 100, 1, 4800, 3, 5) // 4
    ws = guard.full((words,), 0x7FC0BEEF, dtype=torch.int32, device="cuda")             # red-zoned like the outputs
    first = run_sets(R2[:, :, :75].contiguous(), F2[:, :, :75].contiguous(), 5, ws=ws)       # every row hit many times
    torch.cuda.synchronize()
    assert first["counts"][:, 2].min() > 0 and (ws != 0x7FC0BEEF).all()
    same_bits(run_sets(R, F, 5, ws=ws), a, ALL_KEYS)
    R3, F3, _ = case(0, 1, 1000, 900, 75, 5)
    same_bits(run_sets(R3, F3, 5), run_sets(R3, F3, 5), ALL_KEYS)
    R4, F4, _ = case(0, 24, 700, 650, 6, 5, integer=True)                                  # 64-tiles in both launches
    same_bits(run_sets(R4, F4, 5), run_sets(R4, F4, 5), ALL_KEYS)


def test_graph_capture_replays_on_new_inputs():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    real, gen, lab_r, lab_g = _batches(K=4, n=40, m=36, seed=2)
    real2, gen2, _, _ = _batches(K=4, n=40, m=36, seed=5)
    before = metrics.prdc(gen, real, lab_g, lab_r, k=5)["counts"].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.prdc(gen, real, lab_g, lab_r, k=5, per_point=True)                # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = metrics.prdc(gen, real, lab_g, lab_r, k=5, per_point=True)
    real.copy_(real2)
    gen.copy_(gen2)
    g.replay()
    torch.cuda.synchronize()
    eager = metrics.prdc(gen2, real2, lab_g, lab_r, k=5, per_point=True)
    same_bits(cap, eager, ALL_KEYS)
    assert not torch.equal(eager["counts"], before)           # (the two inputs do score differently)


@pytest.mark.usefixtures("guarded")
def test_meaning_identical_sets_and_collapsed_fakes():
    real, _, lab_r, _ = _batches(K=3, n=24, m=24)
    out = metrics.prdc(real.clone(), real, lab_r, lab_r, k=5)
    assert out["values"][:, [0, 1, 3]].eq(1).all() and out["mean"][[0, 1, 3]].eq(1).all()
    # every fake of class 1 is real sample 0 of class 1: precision 1, recall <= (k + 1) / n
    fake = real.clone()
    fake[24:48] = real[24]
    v = metrics.prdc(fake, real, lab_r, lab_r, k=5)["values"]
    assert v[1, 0].item() == 1.0 and 0 < v[1, 1].item() <= (5 + 1) / 24
    assert v[[0, 2]][:, [0, 1, 3]].eq(1).all()


def test_prdc_actions_tool_end_to_end(tmp_path):
    """tools/prdc_actions.py on a small H36M-shaped .npy / .pkl quadruple: selection, normalisation, one metrics.prdc call"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import prdc_actions
    rng = np.random.RandomState(0)
    n, C, T, V = 400, 3, 12, 16
    lab = rng.permutation(np.repeat(np.arange(10), n // 10))
    latent = rng.normal(size=(n, 4)) + lab[:, None]
    mix = rng.normal(size=(4, C * T * V))
    real = (latent @ mix).reshape(n, C, T, V).astype(np.float32)
    lo, hi = real.min(), real.max()
    fake = (2 * ((real - lo) / (hi - lo)) - 1)[::-1] * 0.9 + rng.normal(0, 0.02, size=real.shape)
    fake, fake_lab = np.ascontiguousarray(fake.astype(np.float32)), lab[::-1].copy()
    for nm, d, lb in (("real", real, lab), ("fake", fake, fake_lab)):
        np.save(tmp_path / (nm + ".npy"), d)
        with open(tmp_path / (nm + ".pkl"), "wb") as f:
            pickle.dump(([str(i) for i in range(n)], lb.tolist()), f)
    argv = ["--data_real", str(tmp_path / "real.npy"), "--labels_real", str(tmp_path / "real.pkl"),
            "--data_fake", str(tmp_path / "fake.npy"), "--labels_fake", str(tmp_path / "fake.pkl"),
            "--t_size", "8", "--dataset", "h36m", "--k", "3", "--per_class", "20", "--per_class_table"]
    got = prdc_actions.main(argv)
    r_idx = mmd_def.select_scan(lab, list(range(10)), per_class=20)
    f_idx = mmd_def.select_scan(fake_lab, list(range(10)), per_class=20)
    sel_real = 2 * ((real[r_idx][:, :, :8] - lo) / (hi - lo)) - 1
    sel_fake = fake[f_idx][:, :, :8]
    labels = np.repeat(np.arange(10), 20)
    want = metrics.prdc(sel_fake, sel_real, labels, labels, k=3)
    assert got == tuple(float(v) for v in want["mean"].cpu())
    assert len(got) == 4 and all(0 < v <= 1 for v in (got[0], got[1], got[3])) and got[2] > 0
    ref = prdc_def.reference(torch.tensor(sel_real).reshape(10, 20, -1), torch.tensor(sel_fake).reshape(10, 20, -1), 3,
                             prdc_def.tau(C * 8 * V))
    c = want["counts"].cpu().long()
    assert (ref["counts_lo"] <= c).all() and (c <= ref["counts_hi"]).all()
    one = prdc_actions.main(argv[:-1] + ["--unconditional"])
    assert one == tuple(float(v) for v in metrics.prdc(sel_fake, sel_real, k=3)["mean"].cpu())
