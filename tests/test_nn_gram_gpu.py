"""kg_nn_gram on the MI355X: the matrix-core pre-filter with exact re-score and fallback returns the bits of
kg_nn.  The yardstick throughout is _native.nn on the same tensors (same_bits), and the float64 definition (tests/nn_def.py)
where it is exact: integer data.  stats (sets, classes, 2) = certified rows, fallback rows.

Data that decides whether the certificate is sound:
  cancelling   coordinates 32768 + e: the rounding unit of the Gram sum exceeds every distance - nothing may be certified;
  planted      integer centres far apart, keys exact - everything must be certified;
  mixed        cand + 1 identical copies of the nearest point - the tie reaches past the candidates, exactly those rows fall back."""
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
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


@functools.lru_cache(maxsize=None)
def data(seed, classes, Q, N, D, integer=False):
    b, q = (t.cuda() for t in prdc_def.make_data(seed, classes, N, Q, D, integer=integer))
    return q, b


def view(x):
    return _native.PrdcView(x, x.stride(0), x.stride(1), 0)


def exact(q, b, k, **kw):
    """q (K, Q, D), b (K, N, D) contiguous -> (idx, d2) of _native.nn"""
    K, Q, D = q.shape
    return _native.nn(view(q), view(b), Q, b.shape[1], 1, D, K, k, **kw)


def gram(qs, b, k, **kw):
    """qs: a list of (K, Q, D) sets, b (K, N, D) -> (idx, d2, stats) of _native.nn_gram"""
    K, Q, D = qs[0].shape
    return _native.nn_gram(qs, qs[0].stride(0), qs[0].stride(1), 0, view(b), Q, b.shape[1], 1, D, K, k, **kw)


def same_bits(out, ref, g=0):
    assert torch.equal(out[0][g], ref[0]), "idx"
    assert torch.equal(out[1][g].view(torch.int32), ref[1].view(torch.int32)), "d2"


def whole(out, Q):
    """every row is certified or falls back; returns the (sets, classes) fallback counts"""
    st = out[2]
    assert st.dtype == torch.int32 and (st.sum(-1) == Q).all() and (st >= 0).all()
    return st[..., 1]


def check_exact(out, ref, g=0):
    assert torch.equal(out[0][g].long(), ref["idx"])
    assert torch.equal(out[1][g].double(), ref["d2"])


def splits_for(N):
    """forced splits under which N spans at least three chunks with a ragged last one"""
    return [s for s in range(3, min(N, _native.NN_MAX_SPLIT) + 1) if N % s and -(-N // s) * (s - 1) < N][:2]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("classes,Q,N,D,k", [(1, 40, 40, 6, 3), (3, 53, 37, 75, 5), (1, 20, 33, 3, 31), (1, 70, 130, 48, 4)])
def test_integer_shapes_against_kg_nn_and_the_definition(classes, Q, N, D, k, tile):
    """the integer shapes of test_nn_gpu.py (ties abound; k = 31 is the largest k with a cand): ragged forced splits, both tiles"""
    q, b = data(0, classes, Q, N, D, True)
    want, ref = exact(q, b, k), nn_def.reference(q, b, k)
    splits = splits_for(N)
    assert len(splits) == 2
    for split in splits:
        out = gram([q], b, k, tile=tile, split=split)
        same_bits(out, want)
        check_exact(out, ref)
        print("fallback", (classes, Q, N, D, k), tile, split, whole(out, Q).tolist())


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("Q,N,D,k", [(200, 300, 75, 5), (65, 257, 48, 31), (128, 1000, 2048, 8), (100, 200, 600, 5)])
def test_real_valued_shapes(Q, N, D, k):
    """the real-valued shapes; D = 600 is two full 256-blocks of the pre-filter's chain and a remainder"""
    q, b = data(0, 1, Q, N, D)
    out = gram([q], b, k)
    same_bits(out, exact(q, b, k))
    print("fallback", (Q, N, D, k), whole(out, Q).tolist())


@pytest.mark.usefixtures("guarded")
def test_exclude_self_with_a_planted_duplicate():
    x = data(0, 1, 40, 40, 6, True)[1][:, :32].clone()
    x[0, 7] = x[0, 3]
    N = 32
    for k in (1, 5, N - 1):                     # (k = N - 1 = 31: 31 admissible points, cand = 32 holds them all)
        ref = nn_def.reference(x, x, k, True)
        for tile, split in ((32, 1), (64, 4), (0, 0)):
            out = gram([x], x, k, exclude_self=True, tile=tile, split=split)
            same_bits(out, exact(x, x, k, exclude_self=True))
            check_exact(out, ref)
            assert (out[0][0, 0] != torch.arange(N, device="cuda")[:, None]).all()
            assert out[0][0, 0, 7, 0] == 3 and out[0][0, 0, 3, 0] == 7 and out[1][0, 0, 7, 0] == 0
            whole(out, N)
    with pytest.raises(RuntimeError, match="k=32 > N=32 - 1"):
        gram([x], x, N, exclude_self=True)
    with pytest.raises(RuntimeError, match="exclude_self=1 needs nsets=2 to be 1"):
        gram([x, x], x, 1, exclude_self=True)


@pytest.mark.usefixtures("guarded")
def test_affine_on_either_side():
    q, b = data(1, 2, 150, 300, 75)
    scale, shift = 2.0 / 7.3, -2.0 * -3.1 / 7.3 - 1.0
    raw_q, raw_b = (q - shift) / scale, (b - shift) / scale
    norm_q, norm_b = raw_q.clone().mul_(scale).add_(shift), raw_b.clone().mul_(scale).add_(shift)
    want = exact(norm_q, norm_b, 5)
    for tile, split in ((0, 0), (64, 3)):
        same_bits(gram([norm_q], raw_b, 5, b_affine=(scale, shift), tile=tile, split=split), want)
        same_bits(gram([raw_q], norm_b, 5, q_affine=(scale, shift), tile=tile, split=split), want)
        same_bits(gram([raw_q], raw_b, 5, q_affine=(scale, shift), b_affine=(scale, shift), tile=tile, split=split), want)


@pytest.mark.usefixtures("guarded")
def test_crop_in_t_read_in_place():
    """D = 90 as d_outer = 3, d_inner = 6 * 5: the first 6 of 8 frames of every second sample of longer arrays"""
    Q, N, step = 70, 130, 2
    g = torch.Generator(device="cuda").manual_seed(1)
    long_q = torch.randn((Q * step, 3, 8, 5), device="cuda", generator=g)
    long_b = torch.randn((N * step, 3, 8, 5), device="cuda", generator=g)
    sp, so = step * 3 * 8 * 5, 8 * 5
    qv, bv = _native.PrdcView(long_q, 0, sp, so), _native.PrdcView(long_b, 0, sp, so)
    want = _native.nn(qv, bv, Q, N, 3, 30, 1, 5)
    out = _native.nn_gram([long_q], 0, sp, so, bv, Q, N, 3, 30, 1, 5)
    same_bits(out, want)
    flat_q = long_q[::step, :, :6].reshape(1, Q, 90).contiguous()
    flat_b = long_b[::step, :, :6].reshape(1, N, 90).contiguous()
    same_bits(out, exact(flat_q, flat_b, 5))
    norms = _native.nn_norms(bv, N, 3, 30, 1)
    flat = _native.nn_norms(view(flat_b), N, 1, 90, 1)
    assert torch.equal(norms[0], flat[0]) and torch.equal(norms[1], flat[1])
    assert torch.equal(norms[1].amax(1), norms[0].amax(1))
    assert torch.allclose(norms[0], flat_b.double().pow(2).sum(-1).float(), rtol=1e-5)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("nsets", [1, 2, 3, 4])
def test_one_to_four_sets(nsets):
    b = data(0, 2, 150, 300, 75)[1]
    qs = [data(s, 2, 150, 300, 75)[0] for s in range(nsets)]
    out = gram(qs, b, 5)
    assert out[0].shape == (nsets, 2, 150, 5) and out[2].shape == (nsets, 2, 2)
    for g, q in enumerate(qs):
        same_bits(out, exact(q, b, 5), g)
    whole(out, 150)


@pytest.mark.usefixtures("guarded")
def test_base_no_larger_than_cand_is_certified_by_count():
    q, b = data(0, 1, 40, 40, 6, True)
    for N, k, cand in ((10, 3, 0), (12, 3, 12), (11, 10, 0)):
        out = gram([q], b[:, :N].contiguous(), k, cand=cand)
        same_bits(out, exact(q, b[:, :N].contiguous(), k))
        assert out[2].tolist() == [[[40, 0]]]


def cancelling(seed, Q, N, D=64):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n: (32768.0 + torch.randint(-1, 2, (1, n, D), generator=g).float()).cuda()     # noqa: E731
    return mk(Q), mk(N)


@pytest.mark.usefixtures("guarded")
def test_cancelling_data_is_never_certified():
    """|x|^2 ~ 64 * 2^30: one rounding of the Gram sum is 4096, the largest distance 4 * 64 = 256"""
    q, b = cancelling(0, 50, 200)
    want, ref = exact(q, b, 5), nn_def.reference(q, b, 5)
    assert ref["d2"].max() <= 256
    for tile, split in ((0, 0), (64, 3)):
        out = gram([q], b, 5, tile=tile, split=split)
        assert out[2].tolist() == [[[0, 50]]]
        same_bits(out, want)
        check_exact(out, ref)


def planted(seed, Q, k, D=16, copies=0, tied=0):
    """Q integer centres 64 * {0..3}^D (pairwise d2 >= 4096, asserted), the queries; per centre k base points centre + e,
    e in {-1, 0, 1}^D distinct - but for the first `tied` centres `copies` identical copies of one such point.  The base is
    shuffled.  Every value and every sum of the Gram form stays below 2^24: keys are exact."""
    g = np.random.RandomState(seed)
    cen = 64.0 * g.randint(0, 4, size=(Q, D))
    d = ((cen[:, None] - cen[None]) ** 2).sum(-1) + 1e9 * np.eye(Q)
    assert d.min() >= 4096
    pts = []
    for c in range(Q):
        es = set()
        while len(es) < k:
            es.add(tuple(g.randint(-1, 2, size=D)))
        es = np.array(sorted(es), dtype=np.float64)
        pts.append(np.repeat(cen[c] + es[:1], copies, 0) if c < tied else cen[c] + es)
    base = np.concatenate(pts)
    base = base[g.permutation(len(base))]
    assert (base ** 2).sum(-1).max() * 4 < 2 ** 24
    f = lambda x: torch.tensor(x, dtype=torch.float32).unsqueeze(0).cuda()      # noqa: E731
    return f(cen), f(base)


@pytest.mark.usefixtures("guarded")
def test_planted_data_is_always_certified():
    q, b = planted(0, 40, 5)
    ref = nn_def.reference(q, b, 5)
    assert ref["d2"].max() <= 16
    for tile, split in ((0, 0), (32, 3)):
        out = gram([q], b, 5, tile=tile, split=split)
        assert out[2].tolist() == [[[40, 0]]]
        same_bits(out, exact(q, b, 5))
        check_exact(out, ref)


@pytest.mark.usefixtures("guarded")
def test_mixed_data_exactly_the_tied_rows_fall_back():
    """the first 20 centres carry cand + 1 = 14 identical copies of their nearest point: k of the 14 are the answer (the
    lowest indices), and the 14th has the key of the 13th - no certificate can be strict.  The halves as two query sets
    show WHICH rows fell back; the partial compaction list is also run with a second, cancelling class"""
    k, cand, Q = 5, 13, 40
    q, b = planted(1, Q, k, copies=cand + 1, tied=Q // 2)
    want, ref = exact(q, b, k), nn_def.reference(q, b, k)
    assert (ref["d2"][0, :Q // 2, 0] == ref["d2"][0, :Q // 2, -1]).all()
    for tile, split in ((0, 0), (64, 3), (32, 7)):
        out = gram([q], b, k, cand=cand, tile=tile, split=split)
        assert out[2].tolist() == [[[Q // 2, Q // 2]]]
        same_bits(out, want)
        check_exact(out, ref)
    halves = [q[:, :Q // 2].contiguous(), q[:, Q // 2:].contiguous()]
    out = gram(halves, b, k, cand=cand)
    assert out[2].tolist() == [[[0, Q // 2]], [[Q // 2, 0]]]
    for g in range(2):
        same_bits(out, exact(halves[g], b, k), g)
    # every second row tied: the list is scattered over the row tiles
    order = torch.arange(Q).reshape(2, Q // 2).t().reshape(-1).cuda()
    out = gram([q[:, order].contiguous()], b, k, cand=cand, tile=32)
    assert out[2].tolist() == [[[Q // 2, Q // 2]]]
    same_bits(out, exact(q[:, order].contiguous(), b, k))
    # two classes: planted (all certified) and cancelling (none)
    cq, cb = cancelling(2, Q, b.shape[1], D=16)
    q2, b2 = torch.cat([q, cq]).contiguous(), torch.cat([b, cb]).contiguous()
    for order2 in ((0, 1), (1, 0)):
        qq, bb = q2[list(order2)].contiguous(), b2[list(order2)].contiguous()
        out = gram([qq], bb, k, cand=cand)
        st = [[Q // 2, Q // 2], [0, Q]]
        assert out[2].tolist() == [[st[order2[0]], st[order2[1]]]]
        same_bits(out, exact(qq, bb, k))


@pytest.mark.usefixtures("guarded")
def test_offset_sweep():
    """real-valued data moved away from the origin by 4^p: the Gram form loses a digit per step, the bits stay those of kg_nn"""
    q, b = data(0, 1, 200, 300, 75)
    counts = []
    for p in range(8):
        qo, bo = q + 4.0 ** p, b + 4.0 ** p
        out = gram([qo], bo, 5)
        same_bits(out, exact(qo, bo, 5))
        counts.append(int(whole(out, 200)[0, 0]))
    print("offset sweep: fallback rows of 200 at 4^0 .. 4^7:", counts)
    assert counts[-1] >= counts[0]


@pytest.mark.usefixtures("guarded")
def test_same_bits_and_stats_under_every_plan():
    q, b = data(0, 2, 150, 300, 75)
    want = exact(q, b, 5)
    for cand in (0, 6, 13, 32):
        stats = None
        for tile, split in ((0, 0), (32, 1), (32, 5), (64, 2), (64, 7), (0, 32)):
            out = gram([q], b, 5, cand=cand, tile=tile, split=split)
            same_bits(out, want)
            whole(out, 150)
            stats = out[2] if stats is None else stats
            assert torch.equal(out[2], stats), (cand, tile, split)
        print("cand", cand, "fallback", stats[..., 1].tolist())


@pytest.mark.usefixtures("guarded")
def test_deterministic_and_workspace_contents_do_not_matter():
    q, b = data(0, 2, 150, 300, 75)
    a = gram([q], b, 5, split=5)
    words = _native.nn_gram_workspace_bytes(1, 150, 300, 1, 75, 2, 5, split=5) // 4
    assert words * 4 == 2 * (150 * (8 * 13 * 6 + 8) + 4)
    ws = guard.full((words,), 0x7FC0BEEF, dtype=torch.int32, device="cuda")
    norms = _native.nn_norms(view(b), 300, 1, 75, 2)
    for _ in range(2):
        out = gram([q], b, 5, split=5, ws=ws, base_norms=norms)
        same_bits(out, (a[0][0], a[1][0]))
        assert torch.equal(out[2], a[2])
    q2, b2 = data(1, 2, 150, 300, 75)
    gram([q2], b2, 5, split=5, ws=ws)           # the workspace now holds another search's lists and flags
    ws[-2:] = 150                               # (and list lengths that are not this call's)
    same_bits(gram([q], b, 5, split=5, ws=ws, base_norms=norms), (a[0][0], a[1][0]))
    with pytest.raises(ValueError, match="at least"):
        gram([q], b, 5, split=5, ws=ws[:-1])


def test_graph_capture_replays_on_new_inputs():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)  The replay's inputs are the
    mixed case: certified rows and a fallback list that the captured launches have not seen"""
    k, cand, Q = 5, 13, 40
    q2, b2 = planted(1, Q, k, copies=cand + 1, tied=Q // 2)
    q, b = planted(0, Q, k)
    pad = b2.shape[1] - b.shape[1]
    b = torch.cat([b, b[:, :pad] + 1000.0], 1).contiguous()           # (the same N; the extra points lie far away)
    q, b = q.clone(), b.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gram([q], b, k, cand=cand)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        norms = _native.nn_norms(view(b), b.shape[1], 1, 16, 1)
        cap = gram([q], b, k, cand=cand, base_norms=norms)
    g.replay()
    torch.cuda.synchronize()
    assert cap[2].tolist() == [[[Q, 0]]]
    q.copy_(q2)
    b.copy_(b2)
    g.replay()
    torch.cuda.synchronize()
    assert cap[2].tolist() == [[[Q // 2, Q // 2]]]
    same_bits(cap, exact(q2, b2, k))


def _resident(train, lab, scale, shift):
    raw = ((torch.as_tensor(train) - shift) / scale).cuda()
    return types.SimpleNamespace(fits=True, data=raw, labels=torch.as_tensor(lab).cuda(), scale=scale, shift=shift)


@pytest.mark.usefixtures("guarded")
def test_metrics_with_method_gram_equal_the_exact_results(monkeypatch):
    train, lab_t, gen, lab_g, copied = nn_def.planted(0, 120, 40, 3, 5, 5, 4)
    held, lab_h, _, _, _ = nn_def.planted(7, 30, 4, 3, 5, 5, 4)
    ds = _resident(train, lab_t, 0.4, -0.3)
    seen = []
    plain = _native.nn_gram
    monkeypatch.setattr(_native, "nn_gram", lambda qs, sc, sp, so, bv, *a, **kw: (seen.append((qs, bv, kw)), plain(qs, sc, sp, so, bv, *a, **kw))[1])
    gen_d = torch.as_tensor(gen).cuda()
    out = metrics.nearest(gen_d, ds, k=3, method="gram")
    qs, bv, kw = seen[-1]
    assert bv.t.data_ptr() == ds.data.data_ptr() and qs[0].data_ptr() == gen_d.data_ptr() and kw["b_affine"] == (0.4, -0.3)
    want = metrics.nearest(gen_d, ds, k=3)
    assert all(torch.equal(out[key], want[key]) for key in ("idx", "d2", "index"))
    assert out["index"][0, :10, 0].tolist() == copied.tolist()
    assert (out["certified"] + out["fallback"]).tolist() == [40] and "certified" not in want
    per = metrics.nearest(gen_d, ds, labels_query=lab_g, per_class=6, method="gram")
    want = metrics.nearest(gen_d, ds, labels_query=lab_g, per_class=6)
    assert torch.equal(per["index"], want["index"]) and torch.equal(per["d2"], want["d2"]) and per["fallback"].shape == (4,)
    a = metrics.memorisation(gen, lab_g, ds, heldout=held, labels_heldout=lab_h, method="gram")
    e = metrics.memorisation(gen, lab_g, ds, heldout=held, labels_heldout=lab_h)
    for key, v in e.items():
        assert torch.equal(a[key], v), key
    assert int(a["certified"] + a["fallback"]) == 40 and int(a["train_loo_certified"] + a["train_loo_fallback"]) == 120
    a = metrics.memorisation_sets([gen, gen[::-1].copy()], lab_g, ds, method="gram")
    e = metrics.memorisation_sets([gen, gen[::-1].copy()], lab_g, ds)
    for key, v in e.items():
        assert torch.equal(a[key], v), key
    assert (a["certified"] + a["fallback"]).tolist() == [40, 40]
    R, F = prdc_def.make_data(3, 3, 40, 40, 30, integer=True)
    lab = np.repeat(np.arange(3), 40)
    a = metrics.nn_two_sample(F.reshape(120, 2, 3, 5), R.reshape(120, 2, 3, 5), lab, lab, method="gram")
    e = metrics.nn_two_sample(F.reshape(120, 2, 3, 5), R.reshape(120, 2, 3, 5), lab, lab)
    for key, v in e.items():
        assert torch.equal(a[key], v), key
    assert (a["certified"] + a["fallback"]).tolist() == [160] * 3


def test_nearest_actions_tool_with_method_gram(tmp_path, capsys):
    """tools/nearest_actions.py --method gram on the small H36M-shaped files of test_nn_gpu.py's tool test: the scores and the
    pairs file are those of the exact run, and the row counts are printed"""
    import os
    import pickle
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import nearest_actions
    rng = np.random.RandomState(0)
    n, C, T, V = 200, 3, 12, 16
    lab = rng.permutation(np.repeat(np.arange(10), n // 10))
    mix = rng.normal(size=(4, C * T * V))
    sets = {nm: ((rng.normal(size=(n, 4)) + lab[:, None]) @ mix).reshape(n, C, T, V).astype(np.float32) for nm in ("train", "real")}
    lo, hi = sets["train"].min(), sets["train"].max()
    sets["real"] = np.clip(sets["real"], lo, hi)
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
    argv += ["--t_size", "8", "--dataset", "h36m", "--k", "2", "--per_class", "10"]
    want = nearest_actions.main(argv + ["--pairs_out", str(tmp_path / "exact.npy")])
    capsys.readouterr()
    got = nearest_actions.main(argv + ["--pairs_out", str(tmp_path / "gram.npy"), "--method", "gram"])
    assert got == want and got["authenticity"] == np.float32(0.9)
    assert "kg_nn_gram rows (certified, fallback): fake -> train" in capsys.readouterr().out
    assert np.array_equal(np.load(tmp_path / "gram.npy"), np.load(tmp_path / "exact.npy"))
