"""Projection into W without a GPU: the float64 definition (tests/proj_def.py) against torch.autograd and central differences,
its closed forms, the schedule, every rejection of kg_proj_loss / kg_proj_step (none reaches the GPU), the struct mirrors, and
``Projector(use_graph=False)`` on CPU tensors - the generator's kernels emulated by the oracle, the two new launches by
proj_def - against the float64 loop on the oracle generator."""
import ctypes

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd.project import Projector

import abi_layout
import kin_def
import proj_def
from tests import util


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def data(name, n, T, seed=0):
    """values on the grid 2^-12 below 8 in magnitude: x - y is exact in float32, so the definition's d = fp32(x - y) is the
    float64 difference that torch forms"""
    C, V, bones, _ = kin_def.skeleton(name)
    grid = lambda a: (np.round(np.clip(a, -7, 7) * 4096) / 4096).astype(np.float32)
    x = grid(kin_def.make_data(seed, 1, n, C, T, V)[0])
    y = grid(kin_def.make_data(seed + 50, 1, n, C, T, V, scale=0.9, shift=0.1)[0])
    rng = np.random.RandomState(seed + 7)
    m = rng.uniform(0.2, 2.0, size=(n, T, V)) * (rng.uniform(size=(n, T, V)) > 0.2)
    return x, y, m.astype(np.float32), bones


# ---- 1. the hand-written gradient --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,T", [("ntu", 5), ("h36m", 2), ("h36m", 1)])
def test_hand_gradient_equals_autograd_and_central_differences(name, T):
    x, y, m, bones = data(name, 2, T)
    lam = (1.0, 0.7, 0.1)
    ref = proj_def.loss_def(x, y, m, bones, lam)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    L, words = proj_def.loss_torch(xt, torch.from_numpy(y).double(), torch.from_numpy(m).double(), bones, lam)
    g, = torch.autograd.grad(L.sum(), xt)
    assert np.allclose(words.detach().numpy(), ref["L64"], rtol=1e-12, atol=0)
    scale = np.abs(ref["g64"]).max()
    assert np.abs(g.numpy() - ref["g64"]).max() <= 1e-12 * scale
    # central differences on a handful of elements (the step is exact in float32: x +- h are float32 values)
    rng = np.random.RandomState(1)
    h = 2.0 ** -10
    for _ in range(12):
        i, c, t, v = (rng.randint(k) for k in x.shape)
        xp, xm = x.copy(), x.copy()
        xp[i, c, t, v] += np.float32(h)
        xm[i, c, t, v] -= np.float32(h)
        step = float(xp[i, c, t, v]) - float(xm[i, c, t, v])
        fd = (proj_def.loss_def(xp, y, m, bones, lam)["L64"][i, 0] - proj_def.loss_def(xm, y, m, bones, lam)["L64"][i, 0]) / step
        assert abs(fd - ref["g64"][i, c, t, v]) <= 1e-4 * scale, (fd, ref["g64"][i, c, t, v])
    assert proj_def.brackets_ok(ref)


# ---- 2. closed forms ------------------------------------------------------------------------------------------------------------

def test_closed_forms():
    x, y, m, bones = data("ntu", 3, 6)
    same = proj_def.loss_def(x, x, None, bones, (1, 1, 0.1))
    assert (same["loss"] == 0).all() and (same["gx"] == 0).all()
    xi = np.round(x * 8).astype(np.float32)                              # small integers: every sum below is exact
    off = proj_def.loss_def(xi + 3, xi, None, bones, (1, 1, 0.1))
    assert (off["L64"][:, 1] == 9.0).all() and (off["L64"][:, 2] == 0).all() and (off["L64"][:, 3] == 0).all()
    assert (off["L64"][:, 0] == 9.0).all()
    # a masked-out NaN target entry changes nothing
    mask = (m > 0).astype(np.float32)
    y0, yn = y.copy(), y.copy()
    y0[:, :, mask[0] == 0] = 0.0
    yn[:, :, mask[0] == 0] = np.nan
    a, b = proj_def.loss_def(x, y0, mask[0], bones, (1, 1, 0.1)), proj_def.loss_def(x, yn, mask[0], bones, (1, 1, 0.1))
    assert (mask[0] == 0).sum() > 5
    for k in ("loss", "gx"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert np.isfinite(b["loss"]).all()
    # switched-off terms
    off = proj_def.loss_def(x[:, :, :1], y[:, :, :1], None, bones, (1, 1, 0.1))            # T = 1
    assert (off["L64"][:, 2] == 0).all() and (off["L64"][:, 1] > 0).all()
    nob = proj_def.loss_def(x, y, None, [], (1, 1, 0.1))
    assert (nob["L64"][:, 3] == 0).all()
    zero = proj_def.loss_def(x, y, np.zeros_like(m), bones, (1, 1, 0.1))
    assert (zero["loss"] == 0).all() and (zero["gx"] == 0).all()


# ---- 3. the schedule ------------------------------------------------------------------------------------------------------------

def test_schedule_end_points():
    S, lr = 200, 0.05
    assert proj_def.lr_at(1, S, lr, 10, 50) == lr * (1 / 10) and proj_def.lr_at(10, S, lr, 10, 50) == lr
    assert proj_def.lr_at(150, S, lr, 10, 50) == lr                      # the last full-rate step
    assert proj_def.lr_at(175, S, lr, 10, 50) == pytest.approx(lr / 2, rel=1e-12)
    assert abs(proj_def.lr_at(S, S, lr, 10, 50)) <= 1e-18                # cos(pi) = -1
    assert proj_def.lr_at(1, S, lr) == lr and proj_def.lr_at(S, S, lr) == lr
    assert all(proj_def.lr_at(s + 1, S, lr, 10, 50) <= proj_def.lr_at(s, S, lr, 10, 50) for s in range(150, S))
    assert proj_def.lr_at(1, 1, lr, 1, 1) == 0.0 * lr or abs(proj_def.lr_at(1, 1, lr, 1, 1)) <= 1e-18


def test_step_definition_freezes_and_keeps_the_best():
    rng = np.random.RandomState(0)
    n, D, K = 4, 7, 3
    w, gw = rng.normal(size=(n, D)).astype(np.float32), rng.normal(size=(n, D)).astype(np.float32)
    loss = rng.uniform(1, 2, size=(n, 4)).astype(np.float32)
    gw[1, 3] = np.nan
    loss[2, 0] = np.nan
    z = np.zeros((n, D), dtype=np.float32)
    best = np.array([np.inf, np.inf, np.inf, 0.5], dtype=np.float32)
    o = proj_def.step_def(w, z, z, gw, rng.normal(size=(K, D)), [0, 1, 2, 0], loss, 1, best, np.zeros((n, 4)), z, np.zeros(n), np.zeros((3, n)),
                          3, 0.05, 0.9, 0.999, 1e-8)
    assert o["nonfinite"].tolist() == [0, 1, 1, 0] and o["ok"].tolist() == [True, False, False, True]
    assert np.array_equal(o["w"][1:3], w[1:3]) and (o["am"][1:3] == 0).all()
    assert o["best_obj"][0] == loss[0, 0] and np.array_equal(o["best_w"][0], w[0]) and o["best_obj"][3] == 0.5 and (o["best_w"][3] == 0).all()
    # the first Adam step moves every element by lr against the sign of its gradient
    assert np.allclose(o["w64"][0], w[0].astype(np.float64) - 0.05 * np.sign(gw[0]), atol=1e-6)
    assert np.array_equal(o["hist"][0][[0, 3]], loss[[0, 3], 0]) and np.isnan(o["hist"][0][2])


# ---- 4. rejected arguments ------------------------------------------------------------------------------------------------------

def loss_args(**over):
    C, V, bones, _ = kin_def.skeleton("ntu")
    kw = dict(n=3, C=C, T=8, V=V, bones=bones, lambdas=(1.0, 1.0, 0.1), scale=1.0, shift=0.0)
    fields = dict(x=0x1000, y=0x2000, m=0x3000, loss=0x4000, gx=0x5000, x_sn=8 * V, x_sc=3 * 8 * V, x_st=V, y_sn=C * 8 * V, y_sc=8 * V,
                  y_st=V, sm=0)
    for k, v in over.items():
        (kw if k in kw else fields)[k] = v
    a, keep = _native._proj_loss_shape(kw["n"], kw["C"], kw["T"], kw["V"], kw["bones"], kw["lambdas"], kw["scale"], kw["shift"])
    for k, v in fields.items():
        setattr(a, k, v)
    return a, keep


BAD_BONE = list(kin_def.NTU_BONES)
BAD_BONE[5] = (3, 25)
LOSS_REJECTS = [
    (dict(x=None), b"null pointer x"), (dict(y=None), b"null pointer y"), (dict(loss=None), b"null pointer loss"),
    (dict(gx=None), b"null pointer gx"), (dict(n=0), b"n=0"), (dict(C=0), b"C=0"), (dict(C=4), b"C=4"), (dict(T=0), b"T=0"),
    (dict(V=0, bones=[]), b"V=0"), (dict(V=33, bones=[]), b"V=33"), (dict(bones=[(0, 1)] * 33), b"B=33"),
    (dict(bones=BAD_BONE), b"bones[5][1]=25"), (dict(bones=[(-1, 2)]), b"bones[0][0]=-1"),
    (dict(x_st=-1), b"negative stride of x"), (dict(y_sn=-5), b"negative stride of y"), (dict(sm=-1), b"sm=-1"),
    (dict(lambdas=(-1.0, 1, 1)), b"lambda_pos"), (dict(lambdas=(1, -0.5, 1)), b"lambda_vel"), (dict(lambdas=(1, 1, float("nan"))), b"lambda_bone"),
    (dict(scale=float("inf")), b"scale"), (dict(shift=float("nan")), b"shift"),
]


@pytest.mark.parametrize("over,msg", LOSS_REJECTS, ids=[m.decode().replace(" ", "_") + str(i) for i, (_, m) in enumerate(LOSS_REJECTS)])
def test_loss_rejections_name_the_field(lib, over, msg):
    a, keep = loss_args(**over)
    assert lib.kg_proj_loss(ctypes.byref(a), None) < 0
    err = lib.kg_last_error()
    assert b"kg_proj_loss" in err and msg in err, err


def step_args(**over):
    kw = dict(n=3, D=40, K=5, S=20, lr=0.05, b1=0.9, b2=0.999, eps=1e-8, lambda_w=0.0, ramp_up=1, ramp_down=5)
    ptr = dict(w=0x1000, am=0x2000, av=0x3000, gw=0x4000, wmean=0x5000, labels=0x6000, loss=0x7000, step=0x8000, best_obj=0x9000,
               best_loss=0xa000, best_w=0xb000, hist=0xc000, nonfinite=0xd000)
    for k, v in over.items():
        (kw if k in kw else ptr)[k] = v
    a = _native._proj_step_shape(**kw)
    for k, v in ptr.items():
        setattr(a, k, v)
    return a


STEP_REJECTS = [(dict([(k, None)]), ("null pointer " + k).encode()) for k in
                ("w", "am", "av", "gw", "wmean", "labels", "loss", "step", "best_obj", "best_loss", "best_w", "nonfinite")] + [
    (dict(n=0), b"n=0"), (dict(D=0), b"D=0"), (dict(K=0), b"K=0"), (dict(S=0, ramp_up=0, ramp_down=0), b"S=0"),
    (dict(ramp_up=21), b"ramp_up=21"), (dict(ramp_up=-1), b"ramp_up=-1"), (dict(ramp_down=21), b"ramp_down=21"),
    (dict(ramp_down=-2), b"ramp_down=-2"), (dict(lambda_w=-1.0), b"lambda_w"), (dict(lr=-0.1), b"lr="), (dict(lr=float("nan")), b"lr="),
    (dict(b1=1.0), b"b1=1"), (dict(b1=-0.1), b"b1=-0.1"), (dict(b2=1.0), b"b2=1"), (dict(b2=float("nan")), b"b2="), (dict(eps=-1.0), b"eps="),
]


@pytest.mark.parametrize("over,msg", STEP_REJECTS, ids=[m.decode().replace(" ", "_") + str(i) for i, (_, m) in enumerate(STEP_REJECTS)])
def test_step_rejections_name_the_field(lib, over, msg):
    a = step_args(**over)
    assert lib.kg_proj_step(ctypes.byref(a), None) < 0
    err = lib.kg_last_error()
    assert b"kg_proj_step" in err and msg in err, err


def test_null_args_and_null_table(lib):
    assert lib.kg_proj_loss(None, None) < 0 and b"kg_proj_loss: null args" in lib.kg_last_error()
    assert lib.kg_proj_step(None, None) < 0 and b"kg_proj_step: null args" in lib.kg_last_error()
    a, keep = loss_args()
    a.bones = None
    assert lib.kg_proj_loss(ctypes.byref(a), None) < 0 and b"null pointer bones with B=24" in lib.kg_last_error()


# ---- 5. the ABI -------------------------------------------------------------------------------------------------------------------

def test_exports_layout_and_constants(lib):
    for name in ("kg_proj_loss", "kg_proj_step"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    abi_layout.assert_mirror("KgProjLossArgs")
    abi_layout.assert_mirror("KgProjStepArgs")
    consts = abi_layout.header_constants()
    assert (consts["KG_PROJ_MAX_CHANNELS"], consts["KG_PROJ_MAX_JOINTS"], consts["KG_PROJ_CHUNK_FRAMES"]) == (3, 32, 32)
    assert (_native.PROJ_MAX_CHANNELS, _native.PROJ_MAX_JOINTS, _native.PROJ_CHUNK_FRAMES) == (3, 32, 32)
    assert lib.kg_abi_version() == 9                                      # additive: the version stands


# ---- 6. the Projector's host logic against the float64 loop --------------------------------------------------------------------

def test_projector_host_logic_against_the_float64_loop(monkeypatch):
    G, _ = proj_def.tiny_pair()
    case = proj_def.end_to_end_case()
    y, w_init, r64, E, dw = case["y"], case["w_init"], case["r64"], case["E"], case["dw"]
    print("seed %d: E = %.3g, float32 loop's deviation in best_w = %.3g" % (case["seed"], E, dw))
    assert 0 < E < 1e-3 and 0 < dw < 1e-3
    state = {k: v.clone() for k, v in G.state_dict().items()}
    flags = [m.training for m in G.modules()]
    with util.emulated_native():
        monkeypatch.setattr(_native, "proj_loss", proj_def.emu_proj_loss)
        monkeypatch.setattr(_native, "proj_step", proj_def.emu_proj_step)
        p = Projector(G, 3, dataset="h36m", steps=20, lr=0.05, lambdas=(1.0, 1.0, 0.1), lambda_w=0.0, ramp_up=0.0, ramp_down=0.0,
                      mean_size=16, use_graph=False)
        out = p.project(y, [0, 0, 0], w_init=w_init)
    hist = out["history"].double().numpy()
    dev = float(np.abs(hist / r64["history"] - 1.0).max())
    dwp = float(np.abs(out["best_w"].double().numpy() - r64["best_w"]).max())
    print("objective curve: deviation / E = %.3f;  best_w: deviation / float32 loop's = %.3f" % (dev / E, dwp / dw))
    assert dev <= 4 * E and dwp <= 4 * dw
    assert (hist.min(0) <= 0.5 * hist[0]).all()
    assert torch.equal(out["best_obj"], out["history"].min(0).values) and out["nonfinite"].tolist() == [0, 0, 0]
    assert out["recon"].shape == y.shape and out["best_loss"].shape == (3, 4)
    # the generator stands still
    assert [m.training for m in G.modules()] == flags and all(p_.requires_grad and p_.grad is None for p_ in G.parameters())
    for k, v in G.state_dict().items():
        assert torch.equal(v, state[k]), k


def test_projector_argument_errors():
    G, _ = proj_def.tiny_pair()
    with pytest.raises(ValueError, match="undefined dataset"):
        Projector(G, 3, dataset="kinetics")
    with pytest.raises(ValueError, match="noise must be"):
        Projector(G, 3, dataset="h36m", noise="learned")
    with pytest.raises(ValueError, match="lambdas are three numbers"):
        Projector(G, 3, dataset="h36m", lambdas=(1.0, -1.0, 0.0))
    with pytest.raises(ValueError, match="fractions of steps"):
        Projector(G, 3, dataset="h36m", ramp_down=1.5)
    with pytest.raises(ValueError, match="outside \\[0, V=16\\)"):
        Projector(G, 3, dataset="ntu")
