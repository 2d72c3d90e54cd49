"""kg_nn on the MI355X: indices and distances against the float64 definition (tests/nn_def.py) - exactly on integer data,
inside the error model on real-valued data -, the same bits under every (tile, split) plan, exclude_self, the affine,
determinism, workspace reuse, graph capture, and metrics.nearest / memorisation / nn_two_sample and the command-line tool.

Error model (nn_def): tau_D = (D + 3) 2^-24 bounds the relative error of every fp32 distance.  A query whose first k + 1
reference distances are separated by more than that is DECIDED and must return the reference list in order; that at most
5 % of the queries are undecided at these shapes is asserted on the definition alone (tests/test_nn_cpu.py)."""
import functools
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native
from kinetic_gan_amd import metrics

import nn_def
import prdc_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


@functools.lru_cache(maxsize=None)
def case(seed, classes, Q, N, D, k, integer=False, exclude_self=False):
    """(q (K, Q, D), b (K, N, D)) fp32 on the GPU and their float64 reference (with `decided` unless the data is integer);
    computed once"""
    b, q = (t.cuda() for t in prdc_def.make_data(seed, classes, N, Q, D, integer=integer))
    ref = nn_def.reference(q, b, k, exclude_self, 0.0 if integer else nn_def.tau(D))
    return q, b, ref


def view(x):
    return _native.PrdcView(x, x.stride(0), x.stride(1), 0)


def run(q, b, k, **kw):
    """q (K, Q, D), b (K, N, D) contiguous -> (idx, d2) of _native.nn"""
    K, Q, D = q.shape
    return _native.nn(view(q), view(b), Q, b.shape[1], 1, D, K, k, **kw)


def same_bits(a, b):
    assert torch.equal(a[0], b[0]), "idx"
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "d2"


def check_exact(out, ref):
    assert torch.equal(out[0].long(), ref["idx"])
    assert torch.equal(out[1].double(), ref["d2"])


def check_model(out, ref, D, k):
    """decided queries: the reference list in order; every query: each distance within tau_D of the float64 distance of its
    index, a non-decreasing list of distinct indices, and no index left out closer than the k-th by more than the bound"""
    t = nn_def.tau(D)
    idx, d2, dist = out[0].long(), out[1].double(), ref["dist"]
    dec = ref["decided"]
    print("decided %d of %d queries" % (int(dec.sum()), dec.numel()))
    assert dec.double().mean() >= 0.95
    assert torch.equal(idx[dec], ref["idx"][dec])
    true = torch.gather(dist, 2, idx)
    err = (d2 - true).abs()
    assert (err <= t * true + 1e-30).all(), ((err / true).max().item(), t)
    assert (d2[..., 1:] >= d2[..., :-1]).all()
    assert (idx.sort(-1).values.diff(dim=-1) > 0).all()
    rest = dist.scatter(2, idx, float("inf")).min(-1).values          # the closest base point that was NOT returned
    assert (rest * (1 + t) >= d2[..., -1] * (1 - t)).all()


def splits_for(N):
    """forced splits under which N spans at least three chunks with a ragged last one"""
    return [s for s in range(3, min(N, _native.NN_MAX_SPLIT) + 1) if N % s and -(-N // s) * (s - 1) < N][:2]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("classes,Q,N,D,k", [(1, 40, 40, 6, 3), (3, 53, 37, 75, 5), (1, 20, 33, 3, 32), (1, 70, 130, 48, 4)])
def test_exact_on_integer_data(classes, Q, N, D, k, tile):
    """integer coordinates in [-8, 8], D * 256 < 2^24: every fp32 distance is exact and ties abound - idx and d2 equal the
    definition with no tolerance, N cut into >= 3 chunks with a ragged last one (k = 32 > a chunk of 33 / 4 points: short
    partial lists), both tiles"""
    q, b, ref = case(0, classes, Q, N, D, k, integer=True)
    assert (ref["d2"][..., 1:] == ref["d2"][..., :-1]).any()            # (ties are there)
    splits = splits_for(N)
    assert len(splits) == 2
    for split in splits:
        check_exact(run(q, b, k, tile=tile, split=split), ref)


@pytest.mark.usefixtures("guarded")
def test_same_bits_under_every_plan():
    q, b, ref = case(0, 2, 150, 300, 75, 5)
    auto = run(q, b, 5)
    check_model(auto, ref, 75, 5)
    for tile in (32, 64):
        for split in (1, 2, 5):
            same_bits(run(q, b, 5, tile=tile, split=split), auto)
    same_bits(run(q, b, 5, split=32), auto)
    same_bits(run(q, b, 5, tile=64, split=7), auto)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("Q,N,D,k", [(200, 300, 75, 5), (65, 257, 48, 32), (128, 1000, 2048, 8)])
def test_real_valued_data(Q, N, D, k, seed):
    q, b, ref = case(seed, 1, Q, N, D, k)
    check_model(run(q, b, k), ref, D, k)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("Q,N,step", [(70, 130, 2), (300, 700, 1)])
def test_real_valued_data_cropped_in_place(Q, N, step):
    """D = 4800 as d_outer = 3, d_inner = 64 * 25: the first 64 of 80 frames of every `step`-th sample of longer arrays, read
    in place"""
    q, b, ref = case(0, 1, Q, N, 4800, 5)
    g = torch.Generator(device="cuda").manual_seed(1)
    long_q = torch.randn((Q * step, 3, 80, 25), device="cuda", generator=g)
    long_b = torch.randn((N * step, 3, 80, 25), device="cuda", generator=g)
    long_q[::step, :, :64] = q.reshape(Q, 3, 64, 25)
    long_b[::step, :, :64] = b.reshape(N, 3, 64, 25)
    sp, so = step * 3 * 80 * 25, 80 * 25
    out = _native.nn(_native.PrdcView(long_q, 0, sp, so), _native.PrdcView(long_b, 0, sp, so), Q, N, 3, 64 * 25, 1, 5)
    check_model(out, ref, 4800, 5)
    same_bits(out, run(q, b, 5))


@pytest.mark.usefixtures("guarded")
def test_exclude_self_with_a_planted_duplicate():
    """one tensor searched against itself, point 7 a copy of point 3: the neighbour at 0 is the twin, never the point
    itself; k = N - 1 passes with exclude_self, k = N without"""
    x = case(0, 1, 40, 40, 6, 3, integer=True)[1][:, :32].clone()
    x[0, 7] = x[0, 3]
    N = 32
    for k, excl in ((1, True), (N - 1, True), (N, False), (5, False)):
        ref = nn_def.reference(x, x, k, excl)
        for tile, split in ((32, 1), (64, 4), (0, 0)):
            out = run(x, x, k, exclude_self=excl, tile=tile, split=split)
            check_exact(out, ref)
            if excl:
                assert (out[0][0] != torch.arange(N, device="cuda")[:, None]).all()
                assert out[0][0, 7, 0] == 3 and out[0][0, 3, 0] == 7 and out[1][0, 7, 0] == 0
            else:
                assert out[0][0, 7, :2].tolist() == [3, 7] and out[1][0, 7, :2].tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="k=32 > N=32 - 1"):
        run(x, x, N, exclude_self=True)


@pytest.mark.usefixtures("guarded")
def test_affine_gives_the_bits_of_two_stock_launches():
    """the unnormalised set with (scale, shift) = the set normalised by mul_ then add_, on either side and on both; D = 75 is
    no multiple of the 32 staged dimensions and N no multiple of the tile, so padding turned into `shift` would show"""
    q, b, _ = case(1, 2, 150, 300, 75, 5)
    scale, shift = 2.0 / 7.3, -2.0 * -3.1 / 7.3 - 1.0
    raw_q, raw_b = (q - shift) / scale, (b - shift) / scale
    norm_q, norm_b = raw_q.clone().mul_(scale).add_(shift), raw_b.clone().mul_(scale).add_(shift)
    want = run(norm_q, norm_b, 5)
    for tile, split in ((0, 0), (64, 3)):
        same_bits(run(norm_q, raw_b, 5, b_affine=(scale, shift), tile=tile, split=split), want)
        same_bits(run(raw_q, norm_b, 5, q_affine=(scale, shift), tile=tile, split=split), want)
        same_bits(run(raw_q, raw_b, 5, q_affine=(scale, shift), b_affine=(scale, shift), tile=tile, split=split), want)
    assert want[1].min() > 0 and torch.isfinite(want[1]).all()


@pytest.mark.usefixtures("guarded")
def test_deterministic_and_workspace_contents_do_not_matter():
    q, b, _ = case(0, 2, 150, 300, 75, 5)
    a = run(q, b, 5, split=5)
    same_bits(run(q, b, 5, split=5), a)
    words = _native.nn_workspace_bytes(150, 300, 1, 75, 2, 5, split=5) // 4
    assert words == 2 * 150 * 5 * 5 * 2
    ws = guard.full((words,), 0x7FC0BEEF, dtype=torch.int32, device="cuda")             # poisoned, red-zoned
    same_bits(run(q, b, 5, split=5, ws=ws), a)
    torch.cuda.synchronize()
    assert (ws != 0x7FC0BEEF).all()
    q2, b2, _ = case(1, 2, 150, 300, 75, 5)
    other = run(q2, b2, 5, split=5, ws=ws)                  # the workspace now holds another search's lists
    assert not torch.equal(other[0], a[0])
    same_bits(run(q, b, 5, split=5, ws=ws), a)
    with pytest.raises(ValueError, match="at least"):
        run(q, b, 5, split=5, ws=ws[:-1])


def test_graph_capture_replays_on_new_inputs():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    q, b, _ = case(0, 2, 150, 300, 75, 5)
    q2, b2, _ = case(1, 2, 150, 300, 75, 5)
    q, b = q.clone(), b.clone()
    before = run(q, b, 5)[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(q, b, 5)                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run(q, b, 5)
    q.copy_(q2)
    b.copy_(b2)
    g.replay()
    torch.cuda.synchronize()
    same_bits(cap, run(q2, b2, 5))
    assert not torch.equal(cap[0], before)                 # (the two inputs do differ in their neighbours)


def _resident(train, lab, scale, shift):
    """what train.ResidentDataset holds: the unnormalised samples and the labels on the device, and the affine"""
    raw = ((torch.as_tensor(train) - shift) / scale).cuda()
    return types.SimpleNamespace(fits=True, data=raw, labels=torch.as_tensor(lab).cuda(), scale=scale, shift=shift)


@pytest.mark.usefixtures("guarded")
def test_metrics_nearest_reads_a_resident_dataset_in_place(monkeypatch):
    train, lab_t, gen, lab_g, copied = nn_def.planted(0, 120, 40, 3, 5, 5, 4)
    ds = _resident(train, lab_t, 0.4, -0.3)
    seen = []
    plain = _native.nn

    def spy(qv, bv, *args, **kw):
        seen.append((qv, bv, args, kw))
        return plain(qv, bv, *args, **kw)

    monkeypatch.setattr(_native, "nn", spy)
    gen_d = torch.as_tensor(gen).cuda()
    out = metrics.nearest(gen_d, ds, k=3)
    qv, bv, args, kw = seen[-1]
    assert bv.t.data_ptr() == ds.data.data_ptr() and qv.t.data_ptr() == gen_d.data_ptr()        # no copy
    assert kw["b_affine"] == (0.4, -0.3) and args[:5] == (40, 120, 1, 75, 1)
    assert out["index"][0, :10, 0].tolist() == copied.tolist()
    norm = ds.data.clone().mul_(0.4).add_(-0.3)
    want = metrics.nearest(gen_d, norm, k=3)
    assert torch.equal(out["idx"], want["idx"]) and torch.equal(out["d2"], want["d2"])
    # a crop in T of a longer resident array, class by class with the dataset's own labels
    long = torch.randn((120, 3, 8, 5), device="cuda")
    long[:, :, :5] = ds.data
    ds2 = types.SimpleNamespace(fits=True, data=long[:, :, :5], labels=ds.labels, scale=0.4, shift=-0.3)
    out = metrics.nearest(gen_d, ds2, labels_query=lab_g, per_class=6)
    qv, bv, args, kw = seen[-1]
    assert bv.t.data_ptr() == long.data_ptr() and args[2:4] == (3, 25) and bv.so == 40
    want = metrics.nearest(gen_d, norm, labels_query=lab_g, labels_base=lab_t, per_class=6)
    assert torch.equal(out["index"], want["index"]) and torch.equal(out["d2"], want["d2"])
    assert (lab_t[out["index"].cpu().numpy()[:, :, 0]] == np.arange(4)[:, None]).all()


@pytest.mark.usefixtures("guarded")
def test_memorisation_on_the_planted_case():
    train, lab_t, gen, lab_g, copied = nn_def.planted(0, 120, 40, 3, 5, 5, 4)
    held, lab_h, _, _, _ = nn_def.planted(7, 30, 4, 3, 5, 5, 4)
    ds = _resident(train, lab_t, 0.4, -0.3)
    out = metrics.memorisation(gen, lab_g, ds, heldout=held, labels_heldout=lab_h)
    assert out["authentic"].tolist() == [False] * 10 + [True] * 30 and out["authenticity"].item() == 0.75
    assert out["nn_index"][:10].tolist() == copied.tolist()
    agree = int((lab_t[out["nn_index"].cpu().numpy()] == lab_g).sum())
    assert out["counts"].tolist() == [30, agree] and out["label_agreement"].item() == np.float32(agree / 40)
    assert out["train_loo_d2"].shape == (120,) and out["heldout_nn_index"].shape == (30,)
    again = metrics.memorisation(gen, lab_g, ds, train_loo=out["train_loo_d2"])
    assert torch.equal(again["authentic"], out["authentic"]) and torch.equal(again["nn_d2"], out["nn_d2"])


@pytest.mark.usefixtures("guarded")
def test_nn_two_sample_against_the_definition():
    """integer data: the four searches are exact, so the counts equal the definition's"""
    R, F = prdc_def.make_data(3, 3, 40, 40, 30, integer=True)
    lab = np.repeat(np.arange(3), 40)
    out = metrics.nn_two_sample(F.reshape(120, 2, 3, 5), R.reshape(120, 2, 3, 5), lab, lab)
    want = [list(nn_def.two_sample(F[c], R[c])) for c in range(3)]
    assert out["counts"].tolist() == want
    tot = np.sum(want, 0)
    assert out["acc_real"].tolist() == [np.float32(w[0] / 40) for w in want]
    assert out["mean"].tolist() == [np.float32(tot[0] / 120), np.float32(tot[1] / 120), np.float32(tot.sum() / 240)]
    same = metrics.nn_two_sample(R.reshape(120, 2, 3, 5), R.reshape(120, 2, 3, 5), lab, lab)
    assert same["acc_fake"].eq(0).all()                     # copies: every fake's twin is a real at distance 0


def test_nearest_actions_tool_end_to_end(tmp_path):
    """tools/nearest_actions.py on small H36M-shaped .npy / .pkl files: a fake set whose class 0 is copied from the training
    set, scores, and the pairs file"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import nearest_actions
    rng = np.random.RandomState(0)
    n, C, T, V = 200, 3, 12, 16
    lab = rng.permutation(np.repeat(np.arange(10), n // 10))
    mix = rng.normal(size=(4, C * T * V))
    sets = {}
    for nm in ("train", "real"):
        sets[nm] = ((rng.normal(size=(n, 4)) + lab[:, None]) @ mix).reshape(n, C, T, V).astype(np.float32)
    lo, hi = sets["train"].min(), sets["train"].max()
    sets["real"] = np.clip(sets["real"], lo, hi)            # (the two Feeders then normalise alike: same min and max)
    sets["real"][0].flat[0], sets["real"][1].flat[0] = lo, hi
    fake = (2 * ((sets["train"] - lo) / (hi - lo)) - 1).astype(np.float32)
    fake[lab != 0] += rng.normal(0, 0.5, size=fake[lab != 0].shape).astype(np.float32)
    sets["fake"] = fake
    for nm, d in sets.items():
        np.save(tmp_path / (nm + ".npy"), d)
        with open(tmp_path / (nm + ".pkl"), "wb") as f:
            pickle.dump(([str(i) for i in range(n)], lab.tolist()), f)
    argv = sum((["--data_" + nm, str(tmp_path / (nm + ".npy")), "--labels_" + nm, str(tmp_path / (nm + ".pkl"))]
                for nm in ("real", "fake", "train")), [])
    argv += ["--t_size", "8", "--dataset", "h36m", "--k", "2", "--per_class", "10", "--pairs_out", str(tmp_path / "pairs.npy")]
    got = nearest_actions.main(argv)
    assert set(got) == {"authenticity", "label_agreement", "real_authenticity", "real_label_agreement", "nn_acc_real",
                        "nn_acc_fake", "nn_acc"}
    assert got["authenticity"] == np.float32(0.9) and got["label_agreement"] >= 0.1      # class 0: 10 of 100 are copies
    pairs = np.load(tmp_path / "pairs.npy")
    assert pairs.shape == (200, 3)
    sel = np.flatnonzero(lab == 0)[:10]
    assert pairs[0:20:2, 0].tolist() == sel.tolist() and pairs[0:20:2, 1].tolist() == sel.tolist()    # each copy finds its source
    assert (pairs[0:20:2, 2] < 1e-8).all() and (pairs[1::2, 2] >= pairs[0::2, 2]).all()
