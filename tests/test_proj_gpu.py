"""kg_proj_loss / kg_proj_step on the MI355X against the float64 definition (tests/proj_def.py).  The loss words and gx must lie
inside a derived bracket - one fp32 rounding, 2^-24 |def|, plus the float64 evaluation error bound of proj_def.loss_one, which
must itself stay below 2^-30 of the value it belongs to: asserted on the definition BEFORE the kernel's output is read.  Then
integer data bit for bit, masks, NaN behind a zero weight, strides and the affine read, the step against its definition, frozen
samples, determinism and graph capture.  Outputs start poisoned and red-zoned (tests/guard.py)."""
import functools

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native

import kin_def
import proj_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)

pytestmark = pytest.mark.gpu
LAM = (1.0, 1.0, 0.1)
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    _native.load_library()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def case(name, n, T, mask="weights", seed=1):
    """(x, y, m, bones, the definition): computed once; nothing of the kernel is read here.  mask: None, "weights" (n, T, V) in
    [0.2, 2) with a fifth of the entries 0, "shared" (T, V) of 0 / 1"""
    C, V, bones, _ = kin_def.skeleton(name)
    x = kin_def.make_data(seed, 1, n, C, T, V)[0]
    y = kin_def.make_data(seed + 50, 1, n, C, T, V, scale=0.9, shift=0.1)[0]
    rng = np.random.RandomState(seed + 7)
    m = None
    if mask == "weights":
        m = (rng.uniform(0.2, 2.0, size=(n, T, V)) * (rng.uniform(size=(n, T, V)) > 0.2)).astype(F32)
    elif mask == "shared":
        m = (rng.uniform(size=(T, V)) > 0.3).astype(F32)
    ref = proj_def.loss_def(x, y, m, bones, LAM)
    assert proj_def.brackets_ok(ref), "the float64 evaluation error is too large to test anything"
    return x, y, m, tuple(bones), ref


def run_loss(x, y, bones, lam=LAM, mask=None, **kw):
    dev = lambda t: None if t is None else (torch.from_numpy(t).cuda() if isinstance(t, np.ndarray) else t)
    loss, gx = _native.proj_loss(dev(x), dev(y), bones, lam, mask=dev(mask), **kw)
    guard.assert_no_poison(loss, "loss")
    guard.assert_no_poison(gx, "gx")
    return loss, gx


def check_loss(loss, gx, ref):
    got_l, got_g = loss.cpu().numpy().astype(np.float64), gx.cpu().numpy().astype(np.float64)
    tol_l = proj_def.U32 * np.abs(ref["L64"]) + ref["eL"]
    tol_g = proj_def.U32 * np.abs(ref["g64"]) + ref["eg"]
    err_l, err_g = np.abs(got_l - ref["L64"]), np.abs(got_g - ref["g64"])
    print("loss: worst error / bracket %.3f;  gx: %.3f" % ((err_l / np.maximum(tol_l, 1e-300)).max(), (err_g / np.maximum(tol_g, 1e-300)).max()))
    assert (err_l <= tol_l).all(), (got_l, ref["L64"])
    assert (err_g <= tol_g).all(), float((err_g / np.maximum(tol_g, 1e-300)).max())


# ---- 1. against the definition ------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("T", [1, 2, 5, 64])
@pytest.mark.parametrize("name", ["ntu", "h36m"])
def test_loss_against_the_definition(name, T, n):
    x, y, m, bones, ref = case(name, n, T)
    loss, gx = run_loss(x, y, bones, mask=m)
    assert loss.shape == (n, 4) and gx.shape == x.shape and loss.dtype == gx.dtype == torch.float32
    check_loss(loss, gx, ref)
    if T == 1:
        assert (loss[:, 2] == 0).all()                                    # the velocity term is off


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("T", [33, 97])
def test_loss_over_several_chunks_without_mask(T):
    """T = 33: one frame in the second chunk; 97: four chunks, the last of one frame"""
    x, y, m, bones, ref = case("ntu", 3, T, None)
    check_loss(*run_loss(x, y, bones), ref)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("name,T", [("ntu", 64), ("h36m", 5), ("h36m", 1)])
def test_integer_data_bit_for_bit(name, T):
    C, V, bones, _ = kin_def.skeleton(name)
    rng = np.random.RandomState(3)
    x = rng.randint(-9, 10, size=(5, C, T, V)).astype(F32)
    y = rng.randint(-9, 10, size=(5, C, T, V)).astype(F32)
    m = (rng.uniform(size=(5, T, V)) > 0.25).astype(F32)
    ref = proj_def.loss_def(x, y, m, bones, LAM)
    loss, gx = run_loss(x, y, bones, mask=m)
    assert np.array_equal(bits(loss.cpu().numpy()), bits(ref["loss"])), (loss.cpu().numpy(), ref["loss"])
    check_loss(loss, gx, ref)
    same, g0 = run_loss(x, x, bones, mask=m)
    assert (same == 0).all() and (g0 == 0).all()
    off, _ = run_loss(x + 3, x, bones)
    assert (off[:, 0] == 9).all() and (off[:, 1] == 9).all() and (off[:, 2] == 0).all() and (off[:, 3] == 0).all()


# ---- 2. masks ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_masks():
    x, y, m, bones, ref = case("ntu", 5, 12, "shared")
    loss, gx = run_loss(x, y, bones, mask=m)
    check_loss(loss, gx, ref)
    per = np.broadcast_to(m, (5,) + m.shape).copy()
    l2, g2 = run_loss(x, y, bones, mask=per)                             # the same weights through the sample stride
    assert same_bits(loss, l2) and same_bits(gx, g2)
    assert (gx.cpu().numpy()[:, :, m == 0] == 0).all()
    l0, g0 = run_loss(x, y, bones, mask=np.zeros_like(m))
    assert (l0 == 0).all() and (g0 == 0).all() and not torch.signbit(g0).any()
    # NaN behind a zero weight: the bits of the call with those entries zeroed
    y0, yn = y.copy(), y.copy()
    y0[:, :, m == 0] = 0.0
    yn[:, :, m == 0] = np.nan
    la, ga = run_loss(x, y0, bones, mask=m)
    lb, gb = run_loss(x, yn, bones, mask=m)
    assert same_bits(la, lb) and same_bits(ga, gb) and same_bits(la, loss) and torch.isfinite(lb).all()
    # lambdas switch terms off
    l1, g1 = run_loss(x, y, bones, lam=(0.0, 2.0, 0.0), mask=m)
    r1 = proj_def.loss_def(x, y, m, bones, (0.0, 2.0, 0.0))
    check_loss(l1, g1, r1)
    assert (l1[:, 1] == 0).all() and (l1[:, 3] == 0).all() and (l1[:, 2] > 0).all()
    lnb, gnb = run_loss(x, y, (), mask=m)                                 # B = 0
    check_loss(lnb, gnb, proj_def.loss_def(x, y, m, [], LAM))


# ---- 3. strides and the affine read ----------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_crop_in_t_through_scale_and_shift_and_plane_strides():
    x, y, m, bones, _ = case("ntu", 5, 40)
    n, C, T, V = x.shape
    g = torch.Generator(device="cuda").manual_seed(0)
    raw = torch.randn((n, C, T + 9, V), device="cuda", generator=g) * 3
    crop = raw[:, :, 3:3 + T]
    assert not crop.is_contiguous() and crop.stride(2) == V
    scale, shift = 0.37, -0.21
    made = (crop * scale + shift).contiguous()
    xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    la, ga = run_loss(xt, crop, bones, mask=mt, scale=scale, shift=shift)
    lb, gb = run_loss(xt, made, bones, mask=mt)
    assert same_bits(la, lb) and same_bits(ga, gb)
    check_loss(la, ga, proj_def.loss_def(x, raw.cpu().numpy()[:, :, 3:3 + T], m, bones, LAM, scale, shift))
    # x channel-major, as the generator's planes are laid out
    plane = _native.new_plane(n, C, T, V, xt.device)
    plane.copy_(xt)
    assert plane.stride(1) == n * T * V and plane.stride(0) == T * V
    lc, gc = run_loss(plane, made, bones, mask=mt)
    assert same_bits(lc, lb) and same_bits(gc, gb) and gc.is_contiguous()
    with pytest.raises(ValueError, match="joints of y must be contiguous"):
        _native.proj_loss(xt, made.transpose(2, 3).contiguous().transpose(2, 3), bones, LAM)


# ---- 4. the step ----------------------------------------------------------------------------------------------------------------

def step_state(n, D, K, seed=0, S=20):
    rng = np.random.RandomState(seed)
    f = lambda *s: rng.normal(size=s).astype(F32)
    st = dict(w=f(n, D), am=0.01 * f(n, D), av=(0.01 * f(n, D)) ** 2, gw=0.1 * f(n, D), wmean=f(K, D),
              labels=rng.randint(0, K, size=n).astype(np.int64), loss=rng.uniform(0.5, 2.0, size=(n, 4)).astype(F32),
              best_obj=rng.uniform(1.0, 1.5, size=n).astype(F32), best_loss=f(n, 4), best_w=f(n, D), nonfinite=np.zeros(n, dtype=np.int32))
    return st


def run_step(st, s, S, hp):
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in st.items()}
    hist = guard.empty((S, st["w"].shape[0]), dtype=torch.float32, device="cuda")
    step_t = torch.full((1,), s, dtype=torch.int32, device="cuda")
    _native.proj_step(dev["w"], dev["am"], dev["av"], dev["gw"], dev["wmean"], dev["labels"], dev["loss"], step_t, dev["best_obj"],
                      dev["best_loss"], dev["best_w"], dev["nonfinite"], hist, S, **hp)
    assert int(step_t) == s                                               # the launch does not advance the counter
    return dev, hist


def ulp32(v):
    return np.spacing(np.abs(v).astype(F32)).astype(np.float64)


def check_step(st, dev, hist, s, S, hp):
    ref = proj_def.step_def(st["w"], st["am"], st["av"], st["gw"], st["wmean"], st["labels"], st["loss"], s, st["best_obj"],
                            st["best_loss"], st["best_w"], st["nonfinite"], None, S, hp["lr"], hp["b1"], hp["b2"], hp["eps"],
                            hp["lambda_w"], hp["ramp_up"], hp["ramp_down"])
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    ok = ref["ok"]
    for k in ("w", "am", "av"):
        err = np.abs(got[k].astype(np.float64) - ref[k + "64"])
        assert (err[ok] <= ulp32(ref[k + "64"])[ok]).all(), (k, float((err / ulp32(ref[k + "64"]))[ok].max()))
        assert np.array_equal(bits(got[k][~ok]), bits(st[k][~ok])), k     # frozen: the entering bits
    row = hist[s - 1].cpu().numpy()
    guard.assert_no_poison(hist[s - 1], "hist row")
    assert guard.poison_count(hist) == (S - 1) * hist.shape[1]           # and no other row was touched
    if hp["lambda_w"] == 0:
        assert np.array_equal(bits(row), bits(ref["obj"]))
    else:
        fin = np.isfinite(ref["obj"])
        assert np.array_equal(np.isfinite(row), fin) and (np.abs(row[fin].astype(np.float64) - ref["obj"][fin]) <= ulp32(ref["obj"][fin])).all()
    better = ok & (row < st["best_obj"])
    assert better.any() and ((~better).any() or len(better) == 1)
    assert np.array_equal(bits(got["best_obj"]), bits(np.where(better, row, st["best_obj"])))
    assert np.array_equal(bits(got["best_w"]), bits(np.where(better[:, None], st["w"], st["best_w"])))
    assert np.array_equal(bits(got["best_loss"]), bits(np.where(better[:, None], st["loss"], st["best_loss"])))
    assert got["nonfinite"].tolist() == (st["nonfinite"] + (~ok)).tolist() == ref["nonfinite"].tolist()
    for k in ("gw", "wmean", "loss"):
        assert np.array_equal(bits(got[k]), bits(st[k])), k               # inputs stay


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("lambda_w", [0.0, 0.01])
@pytest.mark.parametrize("s", [1, 2, 17, 20])
@pytest.mark.parametrize("n,D", [(1, 35), (5, 572), (70, 35)])
def test_step_against_the_definition(n, D, s, lambda_w):
    """S = 20, ramp_up 4, ramp_down 5: step 1 and 2 lie on the rising ramp (and carry the largest bias corrections), 17 on the
    cosine, 20 is its end (lr_s = 0 up to cos(pi) + 1)"""
    S, hp = 20, dict(lr=0.05, b1=0.9, b2=0.999, eps=1e-8, lambda_w=lambda_w, ramp_up=4, ramp_down=5)
    st = step_state(n, D, 3, seed=n + s)
    st["best_obj"][0] = 100.0                                             # sample 0 improves,
    if n > 1:
        st["best_obj"][1] = -1.0                                          # sample 1 does not
    dev, hist = run_step(st, s, S, hp)
    check_step(st, dev, hist, s, S, hp)


@pytest.mark.usefixtures("guarded")
def test_step_without_ramps_and_without_history():
    S, hp = 7, dict(lr=0.1, b1=0.0, b2=0.5, eps=1e-3, lambda_w=0.0, ramp_up=0, ramp_down=0)
    st = step_state(4, 33, 2, seed=5)
    st["best_obj"][0], st["best_obj"][1] = 100.0, -1.0
    dev, hist = run_step(st, 7, S, hp)
    check_step(st, dev, hist, 7, S, hp)
    d2 = {k: torch.from_numpy(v.copy()).cuda() for k, v in st.items()}
    _native.proj_step(d2["w"], d2["am"], d2["av"], d2["gw"], d2["wmean"], d2["labels"], d2["loss"], torch.full((1,), 7, dtype=torch.int32, device="cuda"),
                      d2["best_obj"], d2["best_loss"], d2["best_w"], d2["nonfinite"], None, S, **hp)
    for k in ("w", "am", "av", "best_obj", "best_w"):
        assert same_bits(d2[k], dev[k]), k


@pytest.mark.usefixtures("guarded")
def test_frozen_samples_and_their_neighbours():
    S, hp = 20, dict(lr=0.05, b1=0.9, b2=0.999, eps=1e-8, lambda_w=0.01, ramp_up=0, ramp_down=0)
    st = step_state(6, 70, 3, seed=9)
    st["best_obj"][:] = 100.0
    st["best_obj"][5] = -1.0
    st["gw"][1, 69] = np.nan                                              # a NaN gradient word, in the last element
    st["loss"][3, 0] = np.nan                                             # a NaN loss
    st["gw"][4, 0] = np.inf
    st["nonfinite"][3] = 2
    dev, hist = run_step(st, 3, S, hp)
    check_step(st, dev, hist, 3, S, hp)
    assert dev["nonfinite"].cpu().tolist() == [0, 1, 0, 3, 1, 0]
    assert np.isnan(hist[2, 3].item()) and np.isfinite(hist[2, 1].item())
    # a label outside [0, K) freezes its sample instead of reading outside wmean
    st2 = step_state(3, 40, 2, seed=2)
    st2["best_obj"][:] = [100.0, -1.0, 100.0]
    st2["labels"][:] = [0, 1, 2]
    dev2, hist2 = run_step(st2, 1, S, hp)
    check_step(st2, dev2, hist2, 1, S, hp)
    assert dev2["nonfinite"].cpu().tolist() == [0, 0, 1]


# ---- 5. launch properties -----------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_two_calls_give_the_same_bits():
    x, y, m, bones, _ = case("ntu", 70, 64)
    la, ga = run_loss(x, y, bones, mask=m)
    lb, gb = run_loss(x, y, bones, mask=m)
    assert same_bits(la, lb) and same_bits(ga, gb)
    S, hp = 20, dict(lr=0.05, b1=0.9, b2=0.999, eps=1e-8, lambda_w=0.01, ramp_up=4, ramp_down=5)
    st = step_state(70, 572, 3, seed=1)
    a, ha = run_step(st, 2, S, hp)
    b, hb = run_step(st, 2, S, hp)
    for k in a:
        assert torch.equal(a[k], b[k]) if a[k].dtype != torch.float32 else same_bits(a[k], b[k]), k
    assert same_bits(ha[1], hb[1])


def test_graph_capture_replays_on_new_inputs():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    x, y, m, bones, _ = case("h36m", 5, 64)
    x2, y2, m2, _, _ = case("h36m", 5, 64, "weights", 4)
    xt, yt, mt = (torch.from_numpy(t).cuda() for t in (x, y, m))
    S, hp = 20, dict(lr=0.05, b1=0.9, b2=0.999, eps=1e-8, lambda_w=0.01, ramp_up=4, ramp_down=5)
    st = step_state(5, 40, 3, seed=3)
    st["best_obj"][:] = 100.0
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in st.items()}
    hist = torch.full((S, 5), float("nan"), device="cuda")
    step_t = torch.ones(1, dtype=torch.int32, device="cuda")
    loss, gx = torch.zeros((5, 4), device="cuda"), torch.zeros_like(xt)

    def fn():
        _native.proj_loss(xt, yt, bones, LAM, mask=mt, loss=loss, gx=gx)
        _native.proj_step(dev["w"], dev["am"], dev["av"], dev["gw"], dev["wmean"], dev["labels"], loss, step_t, dev["best_obj"],
                          dev["best_loss"], dev["best_w"], dev["nonfinite"], hist, S, **hp)
        step_t.add_(1)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    # new inputs, state back at the start: the replay must equal two eager calls on them
    for t, v in ((xt, x2), (yt, y2), (mt, m2)):
        t.copy_(torch.from_numpy(v))
    for k, v in st.items():
        dev[k].copy_(torch.from_numpy(v))
    hist.fill_(float("nan"))
    step_t.fill_(1)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    want = {k: torch.from_numpy(v.copy()).cuda() for k, v in st.items()}
    whist = torch.full((S, 5), float("nan"), device="cuda")
    for k in (1, 2):
        l2, _ = _native.proj_loss(torch.from_numpy(x2).cuda(), torch.from_numpy(y2).cuda(), bones, LAM, mask=torch.from_numpy(m2).cuda())
        _native.proj_step(want["w"], want["am"], want["av"], want["gw"], want["wmean"], want["labels"], l2,
                          torch.full((1,), k, dtype=torch.int32, device="cuda"), want["best_obj"], want["best_loss"], want["best_w"],
                          want["nonfinite"], whist, S, **hp)
    assert int(step_t) == 3 and same_bits(loss, l2)
    for k in ("w", "am", "av", "best_obj", "best_w", "best_loss"):
        assert same_bits(dev[k], want[k]), k
    assert same_bits(hist[:2], whist[:2]) and torch.isnan(hist[2:]).all()
    assert not same_bits(want["w"], torch.from_numpy(st["w"]).cuda())
