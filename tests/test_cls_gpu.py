"""The action classifier's head on the MI355X (csrc/kg_cls.hip) against its float64 definition (tests/cls_def.py), every
call inside a guard.Guard scope: poisoned outputs, red zones on both sides of every buffer.

Tolerance.  The definition is also evaluated in numpy float32, every sum in the definition's own (index) order; E is its
largest distance to the float64 value over the cases below, per output kind, as max|a - b| / max|b| of a case.  The device
is allowed 4 E - the rule DESIGN.md 11 uses for the normals: the kernels add in another order (lanes first) and their
exp / log are a few ulp from numpy's.  The test prints E and the device's figure per kind.  E, and the worst figure one MI355X
gave over all cases:
    pooled 9.98e-08 / 9.98e-08      feat 1.02e-06 / 2.05e-07      logits 4.87e-07 / 1.41e-07
    loss_per_sample 1.97e-07 / 1.70e-07      loss 5.37e-08 / 1.70e-07 (the one-sample case: 3.2 E)
    dlogits 2.27e-07 / 1.26e-07     dfeat 5.64e-07 / 5.84e-07     g 3.66e-07 / 3.28e-07
    dw1 2.84e-07 / 2.68e-07   db1 1.95e-07 / 1.87e-07   dw2 7.65e-07 / 2.19e-07   db2 2.03e-07 / 1.97e-07
"""
import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv

import cls_def
import guard

pytestmark = pytest.mark.gpu

# (N, C, T', V', F, L): one sample / a ragged last tile of samples; C no multiple of 64; pools of 1, 2, 4, 6 elements; F at 1
# and at the limit of 96; L below and above one wave
SHAPES = [(1, 8, 1, 1, 1, 2), (5, 72, 2, 1, 16, 10), (7, 512, 4, 1, 64, 60), (33, 512, 2, 3, 96, 120), (64, 64, 1, 1, 16, 4)]
FWD = ("pooled", "feat", "logits", "loss_per_sample", "loss")
BWD = ("dlogits", "dfeat", "g", "dw1", "db1", "dw2", "db2")
GTOP = 0.75


def _inputs(shape):
    N, C, T, V, F_, L = shape
    rs = np.random.RandomState(1000 + sum(shape))
    f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731
    u = rs.randn(N, C, T, V)
    return dict(h=f32(np.where(u > 0, u, 0.2 * u)),
                w1=f32(rs.uniform(-1, 1, (F_, C)) * 1.4 * np.sqrt(3.0 / C)), b1=f32(rs.uniform(-0.2, 0.2, F_)),
                w2=f32(rs.uniform(-1, 1, (L, F_)) * 2.0 * np.sqrt(3.0 / F_)), b2=f32(rs.uniform(-0.2, 0.2, L)),
                y=rs.randint(0, L, N).astype(np.int64))


_DEFS = {}


def _defs(shape, masked):
    """(float64 definition, float32 definition) of a case, computed once"""
    key = (shape, masked)
    if key not in _DEFS:
        i = _inputs(shape)
        args = (i["h"], i["w1"], i["b1"], i["w2"], i["b2"], i["y"], 0.2)
        _DEFS[key] = (cls_def.head_def(*args, gtop=GTOP, masked=masked, dtype=np.float64),
                      cls_def.head_def(*args, gtop=GTOP, masked=masked, dtype=np.float32))
    return _DEFS[key]


def _dist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


_E = {}


def _bound():
    """E per output kind over all shapes (and both `masked` settings for g)"""
    if not _E:
        for kind in FWD + BWD:
            _E[kind] = max(_dist(d32[kind], d64[kind]) for s in SHAPES for m in (False, True) for d64, d32 in [_defs(s, m)])
    return _E


def _device_h(h, layout, dev):
    """h on the device: channel-major planes (sN = T'V', sC = N T'V') or NCHW"""
    t = torch.as_tensor(h)
    if layout == "nchw":
        out = guard.empty(t.shape, dtype=torch.float32, device=dev)
    else:
        n, c, tt, v = t.shape
        out = guard.empty((c, n, tt, v), dtype=torch.float32, device=dev).permute(1, 0, 2, 3)
    out.copy_(t)
    return out


def _run(shape, layout, masked, with_labels, labels=None, slope=0.2, inputs=None, accumulate=None):
    """fwd (+ bwd + wgrad with labels) of one case; everything as numpy on the host"""
    dev = torch.device("cuda")
    i = inputs if inputs is not None else _inputs(shape)
    h = _device_h(i["h"], layout, dev)
    w1, b1, w2, b2 = (torch.as_tensor(i[k]).to(dev) for k in ("w1", "b1", "w2", "b2"))
    y = None
    if with_labels:
        y = torch.as_tensor(i["y"] if labels is None else labels, dtype=torch.int64).to(dev)
    out = nv.cls_head_fwd(h, w1, b1, w2, b2, y, slope)
    for k in ("pooled", "feat", "logits", "pred"):
        guard.assert_no_poison(out[k], k)
    res = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    if not with_labels:
        assert out["loss"] is None and out["loss_per_sample"] is None and out["correct"] is None
        return res
    gtop = torch.full((1,), GTOP, dtype=torch.float32, device=dev)
    g, ws = nv.cls_head_bwd(gtop, h, w1, w2, y, out["feat"], out["logits"], masked=masked, slope=slope)
    N, L, F_ = shape[0], shape[5], shape[4]
    assert ws.numel() * 4 == cls_def.workspace_bytes(N, F_, L)
    if accumulate is None:
        dws = [guard.empty(p.numel(), dtype=torch.float32, device=dev) for p in (w1, b1, w2, b2)]
        nv.cls_head_wgrad(ws, out["pooled"], out["feat"], L, *dws, accumulate=False)
    else:
        dws = [guard.empty(p.numel(), dtype=torch.float32, device=dev).copy_(torch.as_tensor(a).reshape(-1)) for p, a in
               zip((w1, b1, w2, b2), accumulate)]
        nv.cls_head_wgrad(ws, out["pooled"], out["feat"], L, *dws, accumulate=True)
    res.update(g=g.cpu().numpy(), dlogits=ws[:N * L].view(N, L).cpu().numpy(), dfeat=ws[N * L:].view(N, F_).cpu().numpy())
    for k, t, p in zip(("dw1", "db1", "dw2", "db2"), dws, (w1, b1, w2, b2)):
        res[k] = t.view(p.shape).cpu().numpy()
    return res


def _same_bits(a, b, keys=None):
    for k in (keys or a):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("layout", ["planes", "nchw"])
@pytest.mark.parametrize("shape", SHAPES)
def test_head_against_definition(shape, layout):
    E = _bound()
    worst = {}
    with guard.Guard("A"):
        for masked in (False, True):
            d64, _ = _defs(shape, masked)
            r = _run(shape, layout, masked, True)
            for kind in FWD + BWD:
                worst[kind] = max(worst.get(kind, 0.0), _dist(r[kind], d64[kind]))
            # pred: the rule applied to the device's own logits, and the definition's wherever its top two logits are apart
            assert (r["pred"] == cls_def.pred_rule(r["logits"])).all()
            top2 = np.sort(d64["logits"], 1)[:, -2:]
            clear = (top2[:, 1] - top2[:, 0]) > 8 * E["logits"] * np.abs(d64["logits"]).max() if shape[5] > 1 else np.ones(shape[0], bool)
            assert (r["pred"][clear] == d64["pred"][clear]).all()
            assert int(r["correct"]) == int((r["pred"] == _inputs(shape)["y"]).sum())
            # the finishing launch: fp64 sum in sample order, rounded once
            assert np.float32(cls_def.mean_in_order(r["loss_per_sample"])).tobytes() == np.float32(r["loss"]).tobytes()
        # labels = NULL: features, logits and predictions only, the same bits
        r0 = _run(shape, layout, False, False)
        _same_bits(r0, r, ("pooled", "feat", "logits", "pred"))
    for kind in FWD + BWD:
        print("%-16s E %.3e  device %.3e" % (kind, E[kind], worst[kind]))
    for kind in FWD + BWD:
        assert worst[kind] <= 4 * E[kind], (kind, worst[kind], E[kind])


def _integer_inputs():
    N, C, T, V, F_, L = 6, 16, 2, 2, 8, 10
    rs = np.random.RandomState(7)
    w2 = rs.randint(-1, 2, (L, F_)).astype(np.float32)
    b2 = rs.randint(-2, 3, L).astype(np.float32)
    for l in (3, 7, 9):                                # classes 3, 7 and 9 tie on the largest logit of every sample
        w2[l], b2[l] = w2[3], 4096.0
    i = dict(h=rs.randint(-3, 4, (N, C, T, V)).astype(np.float32), w1=rs.randint(-2, 3, (F_, C)).astype(np.float32),
             b1=rs.randint(-2, 3, F_).astype(np.float32), w2=w2, b2=b2, y=np.array([3, 7, 3, 0, 9, 3], dtype=np.int64))
    return (N, C, T, V, F_, L), i


@pytest.mark.parametrize("layout", ["planes", "nchw"])
def test_integer_case_is_bit_exact(layout):
    """small integers, T'V' = 4, slope 1/4: every value of the forward pass is exact in fp32"""
    shape, i = _integer_inputs()
    d = cls_def.head_def(i["h"], i["w1"], i["b1"], i["w2"], i["b2"], i["y"], 0.25)
    with guard.Guard("A"):
        r = _run(shape, layout, False, True, slope=0.25, inputs=i)
    for k in ("pooled", "feat", "logits"):
        assert d[k].astype(np.float32).astype(np.float64).tobytes() == d[k].tobytes()          # exact in fp32 indeed
        assert r[k].tobytes() == d[k].astype(np.float32).tobytes(), k
    assert d["pred"].tolist() == [3] * 6 and r["pred"].tolist() == d["pred"].tolist()
    assert int(r["correct"]) == d["correct"] == 3


def test_bad_label():
    """a label outside [0, L): NaN loss for that sample alone, never counted correct, the other samples keep their bits"""
    shape = SHAPES[2]
    L = shape[5]
    with guard.Guard("A"):
        good = _run(shape, "planes", True, True)
        y = good["pred"].astype(np.int64).copy()          # every sample correct ...
        ref = _run(shape, "planes", True, True, labels=y)
        y_bad = y.copy()
        y_bad[1], y_bad[5] = L, -1                         # ... but for two labels out of range
        bad = _run(shape, "planes", True, True, labels=y_bad)
    assert int(ref["correct"]) == shape[0] and int(bad["correct"]) == shape[0] - 2
    ok = np.ones(shape[0], bool)
    ok[[1, 5]] = False
    assert np.isnan(bad["loss_per_sample"][~ok]).all() and np.isnan(bad["loss"])
    _same_bits(bad, ref, ("pooled", "feat", "logits", "pred"))
    for k in ("loss_per_sample", "dlogits", "dfeat", "g"):
        assert bad[k][ok].tobytes() == ref[k][ok].tobytes(), k
        assert np.isnan(bad[k][~ok]).all(), k


def test_determinism_and_guard_patterns():
    """two calls, a graph replay of fwd + bwd + wgrad, and poison pattern A against B: the same bits; red zones intact"""
    shape = SHAPES[3]
    with guard.Guard("A"):
        a1 = _run(shape, "planes", True, True)
        a2 = _run(shape, "planes", True, True)
    with guard.Guard("B"):
        b = _run(shape, "planes", True, True)
    _same_bits(a1, a2)
    _same_bits(a1, b)
    # replay: static operands, the three launches captured once
    dev = torch.device("cuda")
    i = _inputs(shape)
    N, C, T, V, F_, L = shape
    h = _device_h(i["h"], "planes", dev)
    w1, b1, w2, b2 = (torch.as_tensor(i[k]).to(dev) for k in ("w1", "b1", "w2", "b2"))
    y = torch.as_tensor(i["y"]).to(dev)
    gtop = torch.full((1,), GTOP, dtype=torch.float32, device=dev)
    dws = [torch.zeros(p.numel(), dtype=torch.float32, device=dev) for p in (w1, b1, w2, b2)]
    keep = {}

    def step():
        out = nv.cls_head_fwd(h, w1, b1, w2, b2, y, 0.2)
        g, ws = nv.cls_head_bwd(gtop, h, w1, w2, y, out["feat"], out["logits"], masked=True)
        nv.cls_head_wgrad(ws, out["pooled"], out["feat"], L, *dws, accumulate=False)
        keep.update(out, g=g, ws=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in dws:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    r = {k: keep[k].cpu().numpy() for k in ("pooled", "feat", "logits", "pred", "loss_per_sample", "loss", "correct", "g")}
    r.update(dlogits=keep["ws"][:N * L].view(N, L).cpu().numpy(), dfeat=keep["ws"][N * L:].view(N, F_).cpu().numpy())
    for k, t, p in zip(("dw1", "db1", "dw2", "db2"), dws, (w1, b1, w2, b2)):
        r[k] = t.view(p.shape).cpu().numpy()
    _same_bits(a1, r)


def test_accumulate():
    """accumulate=True adds to what the gradient buffers held, False overwrites (poisoned buffers: test above)"""
    shape = SHAPES[1]
    N, C, T, V, F_, L = shape
    rs = np.random.RandomState(3)
    pre = [rs.randn(*s).astype(np.float32) for s in ((F_, C), (F_,), (L, F_), (L,))]
    with guard.Guard("A"):
        plain = _run(shape, "nchw", False, True)
        acc = _run(shape, "nchw", False, True, accumulate=pre)
    for k, p in zip(("dw1", "db1", "dw2", "db2"), pre):
        assert acc[k].tobytes() == (p + plain[k]).astype(np.float32).tobytes(), k
