"""kg_cls_scores on the MI355X (csrc/kg_cls.hip) against its float64 definition (tests/cls_scores_def.py), every
call inside a guard.Guard scope: poisoned outputs, red zones on both sides of every buffer.

Tolerance.  The integer outputs are bit exact.  A distance is a square root of an fp64 sum of F <= 96 squares: a differently
ordered (lanes first, then a shuffle tree) or contracted (fma) sum is within 2 F 2^-53 = 2.2e-14 of the definition's, relative;
the square root halves that.  The bound is 1e-13 relative: a factor five over it.  Everything downstream of dist is pinned
bit for bit against the device's OWN dist: the two means (in-order fp64 sum, one division), accuracy = correct / N, and
scores = the fp32 rounding of scores64."""
import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import metrics

import guard
from cls_scores_def import cls_scores_def, in_order_means

pytestmark = pytest.mark.gpu

# (S, N, F, K, Sd, Sl): the smallest case; two sets, F below a wave; four sets, F at the limit of 96 (two lane strides), N no
# multiple of anything; K*Sl + Sd pairs over more than one workgroup and K near a wave
SHAPES = [(1, 2, 1, 1, 1, 1), (2, 7, 16, 3, 5, 2), (4, 60, 96, 10, 33, 3), (3, 130, 64, 60, 100, 2)]
DIST_RTOL = 1e-13
INTS = ("correct", "correct_per_class", "count_per_class")


def _inputs(shape, seed=0):
    S, N, F, K, Sd, Sl = shape
    rs = np.random.RandomState(2000 + sum(shape) + seed)
    lab = np.tile(np.arange(K), -(-N // K))[:N]
    rs.shuffle(lab)
    if np.bincount(lab, minlength=K).min() < Sl:         # (N < K * Sl: every class still needs Sl members)
        lab = np.tile(np.arange(K), Sl)[:N]
    div, mm = metrics.cls_pair_tables(lab, K, Sd, Sl, seed)
    feats = [rs.randn(N, F).astype(np.float32) * (1 + s) for s in range(S)]
    preds = [np.where(rs.rand(N) < 0.6, lab, rs.randint(0, K, N)).astype(np.int32) for _ in range(S)]
    return dict(feats=feats, preds=preds, labels=lab.astype(np.int64), div=div, mm=mm, K=K)


def _run(i, ld=None):
    """one nv.cls_scores call on guarded buffers; everything as numpy on the host.  ``ld``: the sets are column slices of
    wider (N, ld) matrices (feat_ld > F)"""
    dev = torch.device("cuda")
    feats = []
    for f in i["feats"]:
        n, d = f.shape
        wide = guard.empty((n, ld or d), dtype=torch.float32, device=dev)      # (the columns beyond F stay poisoned)
        wide[:, :d].copy_(torch.as_tensor(f))
        feats.append(wide[:, :d])
    preds = [guard.empty(p.shape, dtype=torch.int32, device=dev).copy_(torch.as_tensor(p)) for p in i["preds"]]
    up = lambda a, dt: guard.empty(np.shape(a), dtype=dt, device=dev).copy_(torch.as_tensor(a))      # noqa: E731
    out = nv.cls_scores(feats, preds, up(i["labels"], torch.int64), up(i["div"], torch.int32), up(i["mm"], torch.int32), i["K"])
    for k, v in out.items():
        guard.assert_no_poison(v, k)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b, keys=None):
    for k in (keys or a):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def _check(r, i):
    """the device's result r of inputs i against the definition; returns the worst relative distance error"""
    d = cls_scores_def(i["feats"], i["preds"], i["labels"], i["div"], i["mm"], i["K"])
    S, N, Sd = len(i["feats"]), i["labels"].size, np.shape(i["div"])[0]
    for k in INTS:
        assert r[k].dtype == np.int32 and r[k].tobytes() == d[k].tobytes(), k
    assert r["dist"].shape == d["dist"].shape and r["dist"].dtype == np.float64
    fin = np.isfinite(d["dist"])
    assert np.array_equal(np.isnan(r["dist"]), ~fin)
    err = np.abs(r["dist"][fin] - d["dist"][fin]) / np.maximum(d["dist"][fin], 1e-300)
    err[d["dist"][fin] == 0] = np.abs(r["dist"][fin])[d["dist"][fin] == 0]          # identical rows: exactly 0
    worst = float(err.max()) if err.size else 0.0
    print("dist: worst relative error %.3e (bound %.1e)" % (worst, DIST_RTOL))
    assert worst <= DIST_RTOL
    assert (r["dist"][d["dist"] == 0] == 0).all()
    for s in range(S):
        div, mm = in_order_means(r["dist"][s], Sd)
        want = np.array([np.float64(int(r["correct"][s])) / np.float64(N), div, mm])
        assert r["scores64"][s].tobytes() == want.tobytes(), (s, r["scores64"][s], want)
    assert r["scores"].dtype == np.float32 and r["scores"].tobytes() == r["scores64"].astype(np.float32).tobytes()
    return d


@pytest.mark.parametrize("shape", SHAPES)
def test_against_definition(shape):
    i = _inputs(shape)
    i["div"][0] = (i["div"][0, 0], i["div"][0, 0])       # a pair that holds the same row twice: exactly 0
    with guard.Guard("A"):
        r = _run(i)
    d = _check(r, i)
    assert r["dist"][:, 0].tolist() == [0.0] * shape[0] and d["dist"][:, 0].tolist() == [0.0] * shape[0]


def test_row_stride_empty_class_and_bad_label():
    """feat_ld > F (the columns beyond F hold the poison word and are never read), a class without members and one label
    outside [0, K): counted nowhere"""
    S, N, F, K, Sd, Sl = 2, 21, 24, 4, 9, 2
    rs = np.random.RandomState(5)
    lab = np.tile(np.arange(3), 7)                       # class 3 has no member
    div, mm3 = metrics.cls_pair_tables(lab, 3, Sd, Sl, 1)
    i = dict(feats=[rs.randn(N, F).astype(np.float32) for _ in range(S)],
             preds=[rs.randint(0, K, N).astype(np.int32) for _ in range(S)], labels=lab.astype(np.int64), div=div,
             mm=np.concatenate([mm3, mm3[:Sl]]), K=K)    # (class 3's pairs: any valid rows - the kernel takes the table as it is)
    i["labels"][4] = K                                   # outside [0, K)
    i["labels"][10] = -1
    i["preds"][0][4] = K
    with guard.Guard("A"):
        r = _run(i, ld=40)
        plain = _run(i)
    d = _check(r, i)
    assert d["count_per_class"][3] == 0 and r["count_per_class"].sum() == N - 2
    _same_bits(r, plain)


def test_integer_case_is_bit_exact():
    """rows (3 k_i, 4 k_i, 0, ...): every distance is 5 |k_i - k_j| - exact whatever the order of the sum"""
    S, N, F, K, Sd, Sl = 3, 40, 70, 5, 25, 4
    rs = np.random.RandomState(11)
    lab = np.repeat(np.arange(K), N // K)
    div, mm = metrics.cls_pair_tables(lab, K, Sd, Sl, 3)
    feats = []
    for s in range(S):
        k = rs.randint(-20, 21, N).astype(np.float32)
        f = np.zeros((N, F), dtype=np.float32)
        f[:, 0], f[:, 65] = 3 * k, 4 * k                 # (the two columns in different lane strides)
        feats.append(f)
    i = dict(feats=feats, preds=[rs.randint(0, K, N).astype(np.int32) for _ in range(S)], labels=lab.astype(np.int64), div=div,
             mm=mm, K=K)
    with guard.Guard("A"):
        r = _run(i)
    d = cls_scores_def(i["feats"], i["preds"], i["labels"], i["div"], i["mm"], K)
    pairs = np.concatenate([div, mm])
    for s in range(S):
        k = feats[s][:, 0] / 3
        assert d["dist"][s].tolist() == (5 * np.abs(k[pairs[:, 0]] - k[pairs[:, 1]])).tolist()
    _same_bits(r, {k: d[k] for k in r})


def test_determinism_graph_replay_and_guard_patterns():
    """two calls, a graph replay, and poison pattern A against B: the same bits; red zones intact"""
    shape = SHAPES[3]
    i = _inputs(shape)
    with guard.Guard("A"):
        a1 = _run(i)
        a2 = _run(i)
    with guard.Guard("B"):
        b = _run(i)
    _same_bits(a1, a2)
    _same_bits(a1, b)
    dev = torch.device("cuda")
    feats = [torch.as_tensor(f).to(dev) for f in i["feats"]]
    preds = [torch.as_tensor(p).to(dev) for p in i["preds"]]
    lab, div, mm = (torch.as_tensor(i[k]).to(dev) for k in ("labels", "div", "mm"))
    keep = {}

    def step():
        keep.update(nv.cls_scores(feats, preds, lab, div, mm, i["K"]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in keep.values():
        t.view(torch.uint8).fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(a1, {k: v.cpu().numpy() for k, v in keep.items()})
    # the replay follows its operands: other features, other predictions
    j = _inputs(shape, seed=1)
    for t, f in zip(feats, j["feats"]):
        t.copy_(torch.as_tensor(f))
    for t, p in zip(preds, j["preds"]):
        t.copy_(torch.as_tensor(p))
    graph.replay()
    torch.cuda.synchronize()
    with guard.Guard("A"):
        want = _run(dict(i, feats=j["feats"], preds=j["preds"]))
    _same_bits(want, {k: v.cpu().numpy() for k, v in keep.items()})


def test_binding_rejects_what_the_kernel_cannot_read():
    dev = torch.device("cuda")
    i = _inputs(SHAPES[1])
    feats = [torch.as_tensor(f).to(dev) for f in i["feats"]]
    preds = [torch.as_tensor(p).to(dev) for p in i["preds"]]
    lab, div, mm = (torch.as_tensor(i[k]).to(dev) for k in ("labels", "div", "mm"))
    with pytest.raises(ValueError):
        nv.cls_scores(feats * 3, preds * 3, lab, div, mm, i["K"])                    # five sets and more
    with pytest.raises(ValueError):
        nv.cls_scores(feats, preds[:1], lab, div, mm, i["K"])
    with pytest.raises(ValueError):
        nv.cls_scores([feats[0], feats[1].t().contiguous().t()], preds, lab, div, mm, i["K"])      # another row stride
    with pytest.raises(ValueError):
        nv.cls_scores(feats, preds, lab.to(torch.int32), div, mm, i["K"])
    with pytest.raises(ValueError):
        nv.cls_scores(feats, preds, lab, div, mm[:-1], i["K"])                       # no whole number of pairs per class
    with pytest.raises(RuntimeError, match="kg_cls_scores"):
        nv.cls_scores(feats, preds, lab, div[:0], mm, i["K"])                        # Sd = 0: the library's message


def test_head_fwd_writes_row_slices():
    """cls_head_fwd(feat_out=, pred_out=) over three ragged chunks: the bits of three plain calls in the right rows, every
    other row untouched"""
    dev = torch.device("cuda")
    N, C, T, V, F, L = 11, 40, 2, 3, 24, 7
    rs = np.random.RandomState(9)
    f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev)      # noqa: E731
    h = f32(rs.randn(N, C, T, V))
    w1, b1, w2, b2 = f32(rs.randn(F, C) * 0.2), f32(rs.randn(F) * 0.1), f32(rs.randn(L, F) * 0.3), f32(rs.randn(L) * 0.1)
    chunks = [(1, 5), (5, 6), (6, 10)]                   # rows 0 and 10 belong to no chunk
    with guard.Guard("A"):
        feat = guard.full((N, F), -7.0, dtype=torch.float32, device=dev)
        pred = guard.full((N,), -7, dtype=torch.int32, device=dev)
        plain = []
        for lo, hi in chunks:
            out = nv.cls_head_fwd(h[lo:hi], w1, b1, w2, b2, None, feat_out=feat[lo:hi], pred_out=pred[lo:hi])
            assert out["feat"].data_ptr() == feat[lo:hi].data_ptr() and out["pred"].data_ptr() == pred[lo:hi].data_ptr()
            plain.append(nv.cls_head_fwd(h[lo:hi], w1, b1, w2, b2, None))
            assert torch.equal(out["logits"], plain[-1]["logits"])
        for (lo, hi), p in zip(chunks, plain):
            assert feat[lo:hi].cpu().numpy().tobytes() == p["feat"].cpu().numpy().tobytes()
            assert pred[lo:hi].cpu().numpy().tobytes() == p["pred"].cpu().numpy().tobytes()
        for row in (0, 10):
            assert (feat[row] == -7.0).all() and int(pred[row]) == -7
        with pytest.raises(ValueError):
            nv.cls_head_fwd(h[0:4], w1, b1, w2, b2, None, feat_out=feat[0:3])
        with pytest.raises(ValueError):
            nv.cls_head_fwd(h[0:4], w1, b1, w2, b2, None, feat_out=feat[0:4, :F].t().contiguous().t())
        with pytest.raises(ValueError):
            nv.cls_head_fwd(h[0:4], w1, b1, w2, b2, None, pred_out=pred[0:8:2])
