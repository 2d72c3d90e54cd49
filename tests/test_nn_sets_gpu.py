"""kg_nn_sets and kg_nn_scores on the MI355X: every set bit for bit what kg_nn writes for it - under every
(tile, split) plan of either call, through an affine, for column slices of wider matrices and for a crop in T -, exact
against the float64 definition on integer data, determinism under two poison fills, graph capture; the score words against
the integer definition of tests/nn_sets_def.py; metrics.memorisation_sets / memorisation_features against one
metrics.memorisation call per set; tools/nearest_actions.py --classifier.

kg_nn (tests/test_nn_gpu.py pins it against the definition) is the reference of the main check, so it needs no tolerance."""
import functools
import types

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native
from kinetic_gan_amd import metrics

import nn_def
import prdc_def
from nn_sets_def import nn_scores_def, nn_sets_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 40, 40, 6, 3), (3, 53, 37, 75, 5), (1, 20, 33, 3, 32), (1, 70, 130, 48, 4), (1, 70, 130, 8, 1)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


@functools.lru_cache(maxsize=None)
def case(classes, Q, N, D, nsets=4, integer=False):
    """(queries: nsets tensors (K, Q, D), b (K, N, D)) fp32 on the GPU; set g is the query side of prdc_def.make_data(seed g),
    the base that of seed 0; computed once and never written"""
    b = prdc_def.make_data(0, classes, N, Q, D, integer=integer)[0].cuda()
    qs = tuple(prdc_def.make_data(g, classes, N, Q, D, integer=integer)[1].cuda() for g in range(nsets))
    return qs, b


def view(x):
    return _native.PrdcView(x, x.stride(0), x.stride(1), 0)


def run_sets(qs, b, k, **kw):
    """qs: (K, Q, D) contiguous tensors, b (K, N, D) -> (idx, d2) (nsets, K, Q, k) of _native.nn_sets"""
    K, Q, D = qs[0].shape
    return _native.nn_sets(list(qs), qs[0].stride(0), qs[0].stride(1), 0, view(b), Q, b.shape[1], 1, D, K, k, **kw)


def run_one(q, b, k, **kw):
    K, Q, D = q.shape
    return _native.nn(view(q), view(b), Q, b.shape[1], 1, D, K, k, **kw)


def same_bits(a, b):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape
    assert torch.equal(a[0], b[0]), "idx"
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "d2"


def per_set(qs, b, k, **kw):
    outs = [run_one(q, b, k, **kw) for q in qs]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def splits_for(N):
    """forced splits under which N spans at least three chunks with a ragged last one (tests/test_nn_gpu.py)"""
    return [s for s in range(3, min(N, _native.NN_MAX_SPLIT) + 1) if N % s and -(-N // s) * (s - 1) < N][:2]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("nsets", [1, 2, 3, 4])
@pytest.mark.parametrize("classes,Q,N,D,k", SHAPES)
def test_every_set_has_the_bits_of_kg_nn(classes, Q, N, D, k, nsets):
    """the automatic plan of both calls, then both tiles x forced splits (ragged chunks; split = N: chunks of one point, short
    lists; k = 32 > a chunk of 33 / 4 points) against kg_nn under its automatic plan: the plans of the two calls differ"""
    qs, b = case(classes, Q, N, D)
    qs = qs[:nsets]
    want = per_set(qs, b, k)
    same_bits(run_sets(qs, b, k), want)
    splits = splits_for(N)
    assert len(splits) == 2
    for tile in (32, 64):
        for split in splits + [1, min(N, _native.NN_MAX_SPLIT)]:
            same_bits(run_sets(qs, b, k, tile=tile, split=split), want)
    # and kg_nn under a forced plan against the sets under the automatic one
    same_bits(run_sets(qs, b, k), per_set(qs, b, k, tile=64, split=splits[0]))


@pytest.mark.usefixtures("guarded")
def test_empty_chunks():
    """N = 33 in 32 chunks of ceil(33 / 32) = 2 points: chunks 17 .. 31 start beyond N and hold nothing"""
    qs, b = case(1, 20, 33, 3)
    same_bits(run_sets(qs[:3], b, 32, tile=32, split=32), per_set(qs[:3], b, 32))


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("classes,Q,N,D,k", SHAPES[:3])
def test_exact_on_integer_data(classes, Q, N, D, k):
    """integer coordinates in [-8, 8]: every fp32 distance is exact and ties abound - idx and d2 of three sets equal the
    float64 definition with no tolerance"""
    qs, b = case(classes, Q, N, D, integer=True)
    qs = qs[:3]
    ref = nn_sets_def(list(qs), b, k)
    assert (ref["d2"][..., 1:] == ref["d2"][..., :-1]).any() or k == 1
    for tile, split in ((0, 0), (32, splits_for(N)[0]), (64, splits_for(N)[1])):
        idx, d2 = run_sets(qs, b, k, tile=tile, split=split)
        assert torch.equal(idx.long(), ref["idx"]) and torch.equal(d2.double(), ref["d2"])


@pytest.mark.usefixtures("guarded")
def test_base_read_through_an_affine():
    """the resident-array case: the unnormalised base with (scale, shift), the queries normalised; and both sides"""
    qs, b = case(2, 150, 300, 75, nsets=3)
    scale, shift = 2.0 / 7.3, -2.0 * -3.1 / 7.3 - 1.0
    raw_b = (b - shift) / scale
    norm_b = raw_b.clone().mul_(scale).add_(shift)
    raw_q = [(q - shift) / scale for q in qs]
    norm_q = [r.clone().mul_(scale).add_(shift) for r in raw_q]
    want = per_set(norm_q, norm_b, 5)
    same_bits(run_sets(norm_q, raw_b, 5, b_affine=(scale, shift)), want)
    same_bits(run_sets(norm_q, raw_b, 5, b_affine=(scale, shift), tile=64, split=3), want)
    same_bits(run_sets(raw_q, raw_b, 5, q_affine=(scale, shift), b_affine=(scale, shift)), want)
    same_bits(run_sets(norm_q, raw_b, 5, b_affine=(scale, shift)), per_set(norm_q, raw_b, 5, b_affine=(scale, shift)))


@pytest.mark.usefixtures("guarded")
def test_queries_as_column_slices_of_wider_matrices():
    """q_sp > D: the feature columns 3 .. 11 of (Q, 16) matrices, read in place"""
    qs, b = case(1, 70, 130, 8, nsets=3)
    g = torch.Generator(device="cuda").manual_seed(1)
    wide = [torch.randn((70, 16), device="cuda", generator=g) for _ in qs]
    for w, q in zip(wide, qs):
        w[:, 3:11] = q[0]
    cols = [w[:, 3:11] for w in wide]
    assert all(c.data_ptr() == w.data_ptr() + 12 and c.stride(0) == 16 for c, w in zip(cols, wide))
    out = _native.nn_sets(cols, 0, 16, 0, view(b), 70, 130, 1, 8, 1, 1)
    same_bits(out, per_set(qs, b, 1))
    with pytest.raises(ValueError, match="query set 2 reach outside"):
        _native.nn_sets(cols[:2] + [cols[2][:69].clone()], 0, 16, 0, view(b), 70, 130, 1, 8, 1, 1)


@pytest.mark.usefixtures("guarded")
def test_d_outer_with_a_crop_in_t():
    """D = 3 * 8 * 5 as d_outer = 3, d_inner = 8 * 5: the first 8 of 12 frames of longer arrays on both sides, read in place"""
    qs, b = case(1, 70, 130, 120, nsets=2)
    g = torch.Generator(device="cuda").manual_seed(2)
    long_q = [torch.randn((70, 3, 12, 5), device="cuda", generator=g) for _ in qs]
    long_b = torch.randn((130, 3, 12, 5), device="cuda", generator=g)
    for lq, q in zip(long_q, qs):
        lq[:, :, :8] = q.reshape(70, 3, 8, 5)
    long_b[:, :, :8] = b.reshape(130, 3, 8, 5)
    out = _native.nn_sets(long_q, 0, 180, 60, _native.PrdcView(long_b, 0, 180, 60), 70, 130, 3, 40, 1, 4)
    same_bits(out, per_set(qs, b, 4))


@pytest.mark.usefixtures("guarded")
def test_deterministic_under_two_poison_fills():
    qs, b = case(2, 150, 300, 75, nsets=3)
    want = per_set(qs, b, 5)
    words = _native.nn_sets_workspace_bytes(3, 150, 300, 1, 75, 2, 5, split=5) // 4
    assert words == 3 * 2 * 150 * 5 * 5 * 2
    for fill in (0x7FC0BEEF, 0):
        ws = guard.full((words,), fill, dtype=torch.int32, device="cuda")
        out = run_sets(qs, b, 5, split=5, ws=ws)
        same_bits(out, want)
        torch.cuda.synchronize()
        assert (ws != 0x7FC0BEEF).all()
        same_bits(run_sets(qs, b, 5, split=5, ws=ws), want)            # the workspace now holds an earlier search's lists
    with pytest.raises(ValueError, match="at least"):
        run_sets(qs, b, 5, split=5, ws=ws[:-1])


def test_graph_capture_replays_on_new_inputs():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    qs, b = case(1, 150, 300, 75, nsets=3)
    qs2 = [q.flip(1).contiguous() for q in qs[::-1]]
    b2 = b.flip(1).contiguous()
    qs, b = [q.clone() for q in qs], b.clone()
    lab_q = torch.arange(150, dtype=torch.int32, device="cuda") % 4
    lab_b = torch.arange(300, dtype=torch.int32, device="cuda") % 4
    loo = torch.full((300,), 0.5, device="cuda")

    def both():
        idx, d2 = run_sets(qs, b, 5)
        return idx, d2, _native.nn_scores(idx, d2, lab_q, lab_b, loo, 4, per_class=True)     # column 0 of the k = 5 lists

    before = both()[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()                                              # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = both()
    for q, q2 in zip(qs, qs2):
        q.copy_(q2)
    b.copy_(b2)
    g.replay()
    torch.cuda.synchronize()
    want = per_set(qs2, b2, 5)
    same_bits(cap[:2], want)
    eager = _native.nn_scores(want[0], want[1], lab_q, lab_b, loo, 4, per_class=True)
    for key in eager:
        assert torch.equal(cap[2][key].view(torch.uint8), eager[key].view(torch.uint8)), key
    assert not torch.equal(cap[0], before)


# ---- kg_nn_scores --------------------------------------------------------------------------------------------------------

def scores_case(nsets, Q, K, N=97, seed=0):
    """random neighbours, distances and labels; planted: queries 0 / 1 point at base 0 / N - 1, query 0 has d2 == loo
    (authentic) and agrees in its label, query 1 disagrees, the last query has d2 one ulp below (a copy); class K - 1 is
    carried by no query when K > 1"""
    g = np.random.RandomState(seed + 17 * Q + K)
    idx = g.randint(0, N, size=(nsets, Q)).astype(np.int32)
    loo = (g.rand(N).astype(np.float32) + np.float32(0.25))
    d2 = (g.rand(nsets, Q).astype(np.float32) * np.float32(1.5))
    ql = g.randint(0, max(K - 1, 1), size=Q).astype(np.int32)
    bl = g.randint(0, K, size=N).astype(np.int32)
    idx[:, 0] = 0
    d2[:, 0] = loo[0]
    bl[0] = ql[0]                                           # query 0 agrees with its neighbour
    if Q > 1:
        idx[:, 1] = N - 1
        bl[N - 1] = (ql[1] + 1) % K                         # query 1 does not (K > 1)
        d2[:, -1] = np.nextafter(loo[idx[:, -1]], np.float32(0))
    return idx, d2, ql, bl, loo


def check_scores(out, want):
    for key in ("counts", "counts_per_class", "scores64", "scores"):
        got = out[key].cpu().numpy()
        assert got.dtype == want[key].dtype and got.shape == want[key].shape, key
        assert np.array_equal(got.view(np.uint8), want[key].view(np.uint8)), (key, got, want[key])


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("K", [1, 4, 120])
@pytest.mark.parametrize("nsets", [1, 4])
@pytest.mark.parametrize("Q", [1, 255, 257, 1000])
def test_scores_equal_the_definition(Q, nsets, K):
    idx, d2, ql, bl, loo = scores_case(nsets, Q, K)
    want = nn_scores_def(idx, d2, ql, bl, loo, K)
    if Q > 1:
        assert (d2[:, 0] == loo[idx[:, 0]]).all() and (d2[:, -1] < loo[idx[:, -1]]).all()
        assert (idx[:, 0] == 0).all() and (idx[:, 1] == 96).all()
    if K > 1:
        assert (want["counts_per_class"][:, K - 1] == 0).all() and (ql != K - 1).all()
    dev = [torch.as_tensor(a).cuda() for a in (idx, d2, ql, bl, loo)]
    out = _native.nn_scores(*dev, K, per_class=True)
    check_scores(out, want)
    if Q >= 255:
        assert (0 < want["counts"][:, 0]).all() and (want["counts"][:, 0] < Q).all()
        assert K == 1 or ((0 < want["counts"][:, 1]).all() and (want["counts"][:, 1] < Q).all())
    again = _native.nn_scores(*dev, K, per_class=True)
    check_scores(again, want)
    bare = _native.nn_scores(*dev, K)                       # counts_per_class = NULL
    assert "counts_per_class" not in bare
    assert torch.equal(bare["counts"], out["counts"]) and torch.equal(bare["scores"], out["scores"])


@pytest.mark.usefixtures("guarded")
def test_scores_read_column_0_of_a_k5_result():
    idx, d2, ql, bl, loo = scores_case(3, 257, 4)
    want = nn_scores_def(idx, d2, ql, bl, loo, 4)
    g = torch.Generator(device="cuda").manual_seed(3)
    idx5 = torch.randint(0, 97, (3, 1, 257, 5), device="cuda", generator=g, dtype=torch.int32)
    d25 = torch.rand((3, 1, 257, 5), device="cuda", generator=g)
    idx5[:, 0, :, 0] = torch.as_tensor(idx).cuda()
    d25[:, 0, :, 0] = torch.as_tensor(d2).cuda()
    rest = [torch.as_tensor(a).cuda() for a in (ql, bl, loo)]
    check_scores(_native.nn_scores(idx5, d25, *rest, 4, per_class=True), want)
    check_scores(_native.nn_scores(idx5[:, 0], d25[:, 0], *rest, 4, per_class=True), want)
    with pytest.raises(ValueError, match="query_labels"):
        _native.nn_scores(idx5, d25, rest[0].long(), rest[1], rest[2], 4)


@pytest.mark.usefixtures("guarded")
def test_scores_skip_an_index_outside_the_base():
    """outside the definition, documented: such a query is skipped - nothing is read for it and it counts nowhere"""
    idx, d2, ql, bl, loo = scores_case(2, 255, 4)
    bad = idx.copy()
    bad[0, 5], bad[1, 7], bad[1, 9] = -1, 97, 2 ** 31 - 1
    keep = np.ones((2, 255), bool)
    keep[0, 5] = keep[1, 7] = keep[1, 9] = False
    out = _native.nn_scores(*[torch.as_tensor(a).cuda() for a in (bad, d2, ql, bl, loo)], 4, per_class=True)
    for g in range(2):
        auth = (d2[g] >= loo[idx[g]]) & keep[g]
        agree = (bl[idx[g]] == ql) & keep[g]
        assert out["counts"][g].tolist() == [int(auth.sum()), int(agree.sum())]
        assert out["scores"][g, 0].item() == np.float32(np.float64(auth.sum()) / 255)


# ---- metrics -------------------------------------------------------------------------------------------------------------

def _resident(train, lab, scale, shift):
    """what train.ResidentDataset holds: the unnormalised samples and the labels on the device, and the affine"""
    raw = ((torch.as_tensor(train) - shift) / scale).cuda()
    return types.SimpleNamespace(fits=True, data=raw, labels=torch.as_tensor(lab).cuda(), scale=scale, shift=shift)


def planted_sets():
    """nn_def.planted (rows 0 .. 9 of the generated set are near-copies) and two more sets on the same labels: set 1 with rows
    10 .. 29 near-copies as well (noise 1e-4), set 2 exact copies of training rows 40 .. 79"""
    train, lab_t, gen, lab_g, copied = nn_def.planted(0, 120, 40, 3, 5, 5, 4)
    g1, g2 = gen.copy(), train[40:80].copy()
    g1[10:30] = train[20:40] + np.float32(1e-4) * np.random.RandomState(5).randn(20, 3, 5, 5).astype(np.float32)
    return train, lab_t, [gen, g1, g2], lab_g


KEYS = ("nn_index", "nn_d2", "counts", "authenticity", "label_agreement")


def check_against_memorisation(out, sets, lab_g, train, lab_t, one):
    want_counts = []
    for g, x in enumerate(sets):
        want = one(x, lab_g, train, lab_t)
        for key in KEYS:
            assert out[key][g].dtype == want[key].dtype, key
            assert torch.equal(out[key][g].reshape(-1).view(torch.uint8), want[key].reshape(-1).view(torch.uint8)), (g, key)
        assert torch.equal(out["train_loo_d2"].view(torch.int32), want["train_loo_d2"].view(torch.int32))
        want_counts.append(want["counts"].tolist())
    return want_counts


@pytest.mark.usefixtures("guarded")
def test_memorisation_sets_equals_one_memorisation_call_per_set(monkeypatch):
    train, lab_t, sets, lab_g = planted_sets()
    calls = []
    for name in ("nn_sets", "nn_scores", "nn"):
        plain = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _n=name, _p=plain, **kw: (calls.append(_n), _p(*a, **kw))[1])
    out = metrics.memorisation_sets(sets, lab_g, train, lab_t)
    assert calls == ["nn", "nn_sets", "nn_scores"]            # the leave-one-out pass, then ONE search and ONE finishing launch
    del calls[:]
    again = metrics.memorisation_sets(sets, lab_g, train, lab_t, train_loo=out["train_loo_d2"])
    assert calls == ["nn_sets", "nn_scores"]
    counts = check_against_memorisation(out, sets, lab_g, train, lab_t, metrics.memorisation)
    assert counts[0][0] == 30 and counts[1][0] == 10 and counts[2][0] == 0          # 10, 30 and 40 of 40 are copies
    assert out["nn_index"][2].tolist() == list(range(40, 80)) and out["nn_d2"][2].eq(0).all()
    for key in KEYS:
        assert torch.equal(again[key], out[key])
    per_class = out["counts_per_class"].cpu().numpy()
    assert per_class.shape == (3, 4, 2) and (per_class.sum(1) == out["counts"].cpu().numpy()).all()
    # the training side as a ResidentDataset read in place through its affine
    ds = _resident(train, lab_t, 0.4, -0.3)
    seen = []
    plain = _native.nn_sets
    monkeypatch.setattr(_native, "nn_sets", lambda qs, sc, sp, so, bv, *a, **kw: (seen.append((bv, kw)), plain(qs, sc, sp, so, bv, *a, **kw))[1])
    res = metrics.memorisation_sets(sets, lab_g, ds)
    bv, kw = seen[-1]
    assert bv.t.data_ptr() == ds.data.data_ptr() and kw["b_affine"] == (0.4, -0.3)
    check_against_memorisation(res, sets, lab_g, ds, None, lambda x, lg, t, lt: metrics.memorisation(x, lg, t))
    assert res["counts"][:, 0].tolist() == [30, 10, 0]


@pytest.mark.usefixtures("guarded")
def test_memorisation_features_on_planted_duplicate_rows():
    """feature rows: 60 training rows, 24 generated ones of which rows 0 .. 7 ARE training rows 10 .. 17 (distance 0: copies
    whatever the leave-one-out distance, unless that is 0 too - training rows 16 and 17 are duplicates of each other, so a copy
    of either is at 0 >= 0: authentic by the >= of the definition)"""
    g = np.random.RandomState(0)
    ft = g.randn(60, 8).astype(np.float32)
    ft[17] = ft[16]
    fg = (g.randn(24, 8) + 6).astype(np.float32)
    fg[:8] = ft[10:18]
    lab_t, lab_g = np.arange(60) % 4, np.arange(24) % 4
    lab_g[:8] = lab_t[10:18]
    out = metrics.memorisation_features(fg, lab_g, ft, lab_t)
    assert out["nn_index"][:8].tolist() == [10, 11, 12, 13, 14, 15, 16, 16]         # the tie at 0 goes to the lower index
    assert out["nn_d2"][:8].eq(0).all() and out["train_loo_d2"][16:18].eq(0).all()
    assert out["authentic"].tolist() == [False] * 6 + [True] * 18 and out["counts"][0].item() == 18
    assert out["authenticity"].item() == np.float32(18 / 24)
    # against the definition: one global class, k = 1
    ref = nn_def.reference(torch.as_tensor(fg)[None].cuda(), torch.as_tensor(ft)[None].cuda(), 1)
    assert torch.equal(out["nn_index"], ref["idx"].reshape(-1))
    # and the sets form on the same matrices, wider matrices read as column slices included
    wide = torch.zeros((24, 12), device="cuda")
    wide[:, 2:10] = torch.as_tensor(fg).cuda()
    sets = metrics.memorisation_sets([fg, wide[:, 2:10]], lab_g, ft, lab_t)
    for s in range(2):
        for key in KEYS:
            assert torch.equal(sets[key][s].reshape(-1), out[key].reshape(-1)), key
    held = metrics.memorisation_features(fg, lab_g, ft, lab_t, feat_heldout=ft[:5], labels_heldout=lab_t[:5])
    assert held["heldout_nn_index"].tolist() == [0, 1, 2, 3, 4] and held["heldout_authenticity"].item() == 0.0


def test_nearest_actions_tool_with_a_classifier(tmp_path):
    """tools/nearest_actions.py --classifier: the four feature-space scores next to the raw ones, from a checkpoint in the
    format of tools/train_classifier.py (untrained weights: the scores need not mean anything); fake = the normalised training
    set, so in feature space every generated sample finds itself at distance 0 - authenticity 0, label agreement 1 - unless
    two training samples share their features; a checkpoint with another normalisation is refused"""
    import os
    import pickle
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import nearest_actions
    from kinetic_gan_amd.classifier import Classifier
    from kinetic_gan_amd.feeder import Feeder
    from kinetic_gan_amd.train import norm_constants
    rng = np.random.RandomState(0)
    n, C, T, V = 100, 3, 40, 16
    lab = rng.permutation(np.repeat(np.arange(10), n // 10))
    train = rng.normal(size=(n, C, T, V)).astype(np.float32) + lab[:, None, None, None].astype(np.float32)
    lo, hi = train.min(), train.max()
    sets = {"train": train, "real": np.clip(rng.normal(size=(n, C, T, V)).astype(np.float32) + lab[:, None, None, None], lo, hi)}
    sets["real"][0].flat[0], sets["real"][1].flat[0] = lo, hi           # (the two Feeders then normalise alike)
    sets["fake"] = (2 * ((train - lo) / (hi - lo)) - 1).astype(np.float32)
    for nm, d in sets.items():
        np.save(tmp_path / (nm + ".npy"), d.astype(np.float32))
        with open(tmp_path / (nm + ".pkl"), "wb") as f:
            pickle.dump(([str(i) for i in range(n)], lab.tolist()), f)
    scale, shift = norm_constants(Feeder(str(tmp_path / "train.npy"), str(tmp_path / "train.pkl"), norm=True, dataset="h36m"))
    torch.manual_seed(0)
    clf = Classifier(C, 10, 32, latent=64, feat_dim=8, dataset="h36m")
    sd = clf.state_dict()
    sd["meta"] = dict(dataset="h36m", in_channels=C, n_classes=10, t_size=32, latent=64, feat_dim=8, scale=scale, shift=shift)
    torch.save(sd, tmp_path / "classifier_1.pth")
    argv = sum((["--data_" + nm, str(tmp_path / (nm + ".npy")), "--labels_" + nm, str(tmp_path / (nm + ".pkl"))]
                for nm in ("real", "fake", "train")), [])
    argv += ["--t_size", "32", "--dataset", "h36m", "--per_class", "5", "--classifier_batch", "16"]
    got = nearest_actions.main(argv + ["--classifier", str(tmp_path / "classifier_1.pth")])
    new = {"feature_authenticity", "feature_label_agreement", "real_feature_authenticity", "real_feature_label_agreement"}
    assert new < set(got) and all(0.0 <= got[k] <= 1.0 for k in new)
    print({k: got[k] for k in sorted(new)})
    assert got["authenticity"] <= 0.1 and got["feature_authenticity"] <= 0.1 and got["feature_label_agreement"] >= 0.9
    sd["meta"] = dict(sd["meta"], scale=scale * 2)
    torch.save(sd, tmp_path / "classifier_2.pth")
    with pytest.raises(SystemExit, match="--classifier .*scale"):
        nearest_actions.main(argv + ["--classifier", str(tmp_path / "classifier_2.pth")])
