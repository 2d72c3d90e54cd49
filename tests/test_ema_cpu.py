"""Generator weight averaging without a GPU: the entry point's declaration / export / binding, the host
definition (tests/ema_def.py) against closed forms, the host logic of Trainer / FlatParams with the native entry points
emulated (``_native.adam_step_ema`` replaced by the definition), the averaged module, the command line's flags."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd.wgan_gp import Trainer
from oracle.fill import rand_inputs, rand_noise
from tests.util import build_pair, emulated_native

import ema_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def test_entry_point_declared_exported_bound(lib):
    txt = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+kg_adam_step_ema\s*\(", txt), "kg_adam_step_ema is not declared in kgan_hip.h"
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "kg_adam_step_ema")
    assert "kg_adam_step_ema" in _native.EXPORTS
    restype, argtypes = _native.EXPORTS["kg_adam_step_ema"]
    assert restype is ctypes.c_int and len(argtypes) == 16            # the header's sixteen arguments
    assert lib.kg_adam_step_ema.argtypes == argtypes
    assert callable(_native.adam_step_ema)


def test_abi_version_is_still_9(lib):
    assert lib.kg_abi_version() == 9


def test_bad_arguments_are_rejected_without_gpu(lib):
    assert lib.kg_adam_step_ema(None, None, None, None, None, 4, 2e-4, 0.5, 0.999, 1e-8, None, 1.0, 1, 0.9, 10.0, None) < 0
    assert b"kg_adam_step_ema" in lib.kg_last_error()
    a = 0x1000
    assert lib.kg_adam_step_ema(a, a, a, a, a, 4, 2e-4, 0.5, 0.999, 1e-8, a, 1.0, 1, 1.0, 10.0, None) < 0
    assert b"ema_decay" in lib.kg_last_error()
    assert lib.kg_adam_step_ema(a, a, a, a, a, 4, 2e-4, 0.5, 0.999, 1e-8, a, 1.0, 1, 0.9, -1.0, None) < 0
    assert b"ema_warmup" in lib.kg_last_error()


def test_definition_against_closed_forms():
    # the ramp: beta_1 = 2 / 11, beta_s = decay from the first s with (1 + s) / (10 + s) >= decay
    assert ema_def.beta(1, 0.999, 10.0) == 2.0 / 11.0
    assert ema_def.beta(2, 0.999, 10.0) == 3.0 / 12.0
    d = float(np.float32(0.9))
    first = next(s for s in range(1, 1000) if (1.0 + s) / (10.0 + s) >= d)
    assert first == 80                                                 # (1 + s) / (10 + s) >= 0.9 <=> s >= 80
    for s in range(1, 200):
        want = d if s >= first else (1.0 + s) / (10.0 + s)
        assert ema_def.beta(s, 0.9, 10.0) == want, s
    assert ema_def.beta(1, 0.9, 0.0) == d and ema_def.beta(10 ** 6, 0.9999, 0.0) == float(np.float32(0.9999))
    # constant p: e_K - p = (e_0 - p) prod beta_s
    rng = np.random.RandomState(0)
    p = rng.randn(257).astype(np.float32)
    e0 = rng.randn(257).astype(np.float32)
    for decay, warmup in ((0.5, 0.0), (0.99, 10.0), (0.9999, 10.0)):
        e, prod = e0.astype(np.float64), 1.0
        for s in range(1, 41):
            e = ema_def.update(e, p, s, decay, warmup)
            prod *= ema_def.beta(s, decay, warmup)
        np.testing.assert_allclose(e - p, (e0.astype(np.float64) - p) * prod, rtol=0, atol=1e-13)
    # the bound is 2^-21 of the larger magnitude
    assert ema_def.bound(np.float32(-4.0), np.float32(1.0)) == 4.0 * 2.0 ** -21


# ---- host logic --------------------------------------------------------------------------------------------------------

N = 2
SEQUENCE = "dgddgdg"            # critic / generator steps: two critic steps in a row, a generator step at the end


def _inputs(c, G):
    nn_ = G.graph.num_node
    real, labels, z, alpha = rand_inputs(N, c["channels"], c["t_size"], nn_[0], c["n_classes"], c["latent"], seed=3)
    return real, labels, z, alpha, rand_noise(N, c["t_size"], nn_, seed=6)


def _state(tr):
    out = {}
    for name, f, m in (("G", tr.fG, tr.G), ("D", tr.fD, tr.D)):
        for k in ("flat", "grad", "exp_avg", "exp_avg_sq", "step"):
            out[name + "." + k] = getattr(f, k).detach().clone()
        for k, b in m.named_buffers():
            out[name + ".buf." + k] = b.detach().clone()
    return out


def test_average_only_observes(monkeypatch):
    """two trainers from the same seeds, one with ema_decay = 0.9, through the same d_step / g_step sequence: every live
    parameter, moment and buffer identical; the average is the recurrence over the generator's recorded parameters and
    does not move on critic steps; the trainer without a decay never calls adam_step_ema"""
    calls = []

    def counted(*a, **k):
        calls.append(int(a[9].item()))                    # (step_t)
        return ema_def.adam_step_ema(*a, **k)
    with emulated_native():
        monkeypatch.setattr(_native, "adam_step_ema", counted)
        c, G0, D0, _, _ = build_pair("h36m")
        _, G1, D1, _, _ = build_pair("h36m")
        plain = Trainer(G0, D0, n_critic=2)
        avg = Trainer(G1, D1, n_critic=2, ema_decay=0.9)
        assert plain.fG.ema is None and plain.fD.ema is None and avg.fD.ema is None
        assert avg.fG.ema is not None and avg.fG.ema.data_ptr() != avg.fG.flat.data_ptr()
        assert torch.equal(avg.fG.ema, avg.fG.flat)        # e_0: the initial weights
        real, labels, z, alpha, noise = _inputs(c, G0)
        want = avg.fG.flat.detach().numpy().astype(np.float64)
        s = 0
        for kind in SEQUENCE:
            before = avg.fG.ema.clone()
            n_calls = len(calls)
            if kind == "d":
                plain.d_step(real, labels, z, alpha, noise)
                assert len(calls) == n_calls                # the plain trainer: never
                avg.d_step(real, labels, z, alpha, noise)
                assert len(calls) == n_calls                # critic steps: not the average's launch either
                assert torch.equal(avg.fG.ema, before)
            else:
                plain.g_step(labels, z, noise)
                assert len(calls) == n_calls
                avg.g_step(labels, z, noise)
                s += 1
                assert calls[n_calls:] == [s]               # one launch, s counts generator steps
                want = ema_def.update(want.astype(np.float32), avg.fG.flat.detach().numpy(), s, 0.9, 10.0)
                assert np.array_equal(avg.fG.ema.numpy(), want.astype(np.float32))
                assert not torch.equal(avg.fG.ema, before) and not torch.equal(avg.fG.ema, avg.fG.flat)
            a, b = _state(plain), _state(avg)
            assert set(a) == set(b)
            for k in a:
                assert torch.equal(a[k], b[k]), (kind, k)
        assert s == 3 and int(avg.fG.step.item()) == 3 and int(avg.fD.step.item()) == 4


def test_off_means_off_and_flatten_is_required():
    with emulated_native():
        c, G, D, _, _ = build_pair("h36m")
        for decay in (None, 0, 0.0):
            tr = Trainer(G, D, flatten=False, ema_decay=decay)
            assert tr.fG is None
        with pytest.raises(ValueError, match="flatten"):
            Trainer(G, D, flatten=False, ema_decay=0.9)
        tr = Trainer(G, D, ema_decay=0.0)
        assert tr.fG.ema is None
        with pytest.raises(RuntimeError, match="average is off"):
            tr.ema_generator()
        with pytest.raises(ValueError, match="decay"):
            tr.fG.enable_ema(1.0)


@pytest.mark.parametrize("cfg", ["h36m", "ntu"])
def test_ema_generator_module(cfg):
    with emulated_native():
        c, G, D, Go, _ = build_pair(cfg)
        rng_state = torch.get_rng_state()
        tr = Trainer(G, D, ema_decay=0.99, ema_warmup=0.0)
        E = tr.ema_generator()
        assert tr.ema_generator() is E                      # cached
        assert torch.equal(torch.get_rng_state(), rng_state)
        assert type(E) is type(G) and E is not G and not E.training
        sd, live, ref = E.state_dict(), G.state_dict(), Go.state_dict()
        assert list(sd.keys()) == list(live.keys()) == list(ref.keys())
        assert all(sd[k].shape == live[k].shape for k in sd)
        f = tr.fG
        lo, hi = f.ema.data_ptr(), f.ema.data_ptr() + 4 * f.ema.numel()
        mine = list(E.named_parameters())
        assert len(mine) == len(f.offsets)
        for (k, p), (_, q), off in zip(mine, G.named_parameters(), f.offsets):
            assert p.data_ptr() == lo + 4 * off and p.data_ptr() + 4 * p.numel() <= hi, k
            assert p.untyped_storage().data_ptr() == f.ema.untyped_storage().data_ptr(), k
            assert not p.requires_grad and q.requires_grad, k
            assert torch.equal(p, q), k                     # e_0 = the initial weights
        bufs, live_bufs = dict(E.named_buffers()), dict(G.named_buffers())
        assert list(bufs) == list(live_bufs) and len(bufs) > 0
        for k, b in bufs.items():
            assert b.data_ptr() == live_bufs[k].data_ptr() and b is live_bufs[k], k
            assert not b.requires_grad
        # the module reads the average: move it and the live weights apart
        with torch.no_grad():
            f.ema.mul_(0.5)
        k0, p0 = mine[0]
        assert torch.equal(p0, dict(G.named_parameters())[k0] * 0.5)
        # not registered with the parameter sinks: the live bucket's registrations are the only ones
        from kinetic_gan_amd import ops
        for (k, p), (_, q) in zip(mine, G.named_parameters()):
            assert ops._sink_of(q) is not None and ops._sink_of(p) is None, k
        assert all(p.grad is None for _, p in mine)


def test_train_cli_flags():
    spec = importlib.util.spec_from_file_location("kg_tools_train", os.path.join(ROOT, "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--data_path", "d.npy", "--label_path", "l.pkl"]
    opt = mod.parse_args(base)
    assert opt.ema_decay == 0.0 and opt.ema_warmup == 10.0
    opt = mod.parse_args(base + ["--ema_decay", "0.999", "--ema_warmup", "0"])
    assert opt.ema_decay == 0.999 and opt.ema_warmup == 0.0
