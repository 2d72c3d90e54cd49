"""The inference-only generation path without a GPU: C layouts and argument checks of its entry points, the eligibility
rule of kg_genblock_infer, and the host logic of sample.Sampler on emulated kernels (tests/sample_def.py) against the
reference's eval-mode fixtures."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build

import abi_layout
from oracle.fill import rand_inputs, rand_noise
from tests import sample_def, train_def
from tests.util import build_pair, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_TOL = 1e-4          # as tests/test_parity_gpu.py
# Cin, C, Kp, Tc, Vc, V, rep, residual kind: the compile-time geometries of kg_genblock.hip (GB_GEOMETRIES)
GEOMETRIES = [(128, 64, 3, 4, 5, 5, 2, 2), (64, 32, 3, 8, 5, 11, 2, 2), (32, 3, 3, 16, 11, 11, 2, 2), (3, 3, 3, 32, 11, 25, 2, 1),
              (32, 2, 3, 8, 7, 7, 2, 2), (2, 2, 3, 16, 7, 16, 2, 1)]
# blocks G0-G2 of the ntu and h36m generators (Cin, C, Kp, Tc, Vc, V, rep, residual kind)
FRONT = [(572, 512, 1, 1, 1, 1, 1, 0), (512, 256, 1, 1, 1, 1, 4, 2), (256, 128, 3, 4, 1, 5, 1, 2),
         (522, 512, 1, 1, 1, 1, 1, 0), (512, 256, 1, 1, 1, 1, 2, 2), (256, 128, 3, 2, 1, 7, 1, 2)]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def test_new_struct_sizes_match_header():
    for cname in ("KgBnEvalJob", "KgGenBlockInferArgs", "KgSampleInputsArgs"):
        abi_layout.assert_mirror(cname)


def _infer_args(geo, aligned=True):
    a = _native._GenBlockInferArgs()
    a.N = 2
    a.Cin, a.C, a.Kp, a.Tc, a.Vc, a.V, a.rep, a.res_kind = geo
    a.K, a.T = 3, a.Tc * a.rep
    a.wg = a.wr = a.wt = 0x10000 if aligned else 0x10004
    return a


def test_entry_points_reject_invalid_arguments_without_gpu(lib):
    """every new entry point checks its arguments before any launch and names itself in kg_last_error()"""
    assert lib.kg_bn_eval_coef(None, 0, None) < 0 and b"kg_bn_eval_coef" in lib.kg_last_error()
    jobs = (_native._BnEvalJob * 2)()
    assert lib.kg_bn_eval_coef(jobs, 0, None) < 0 and b"njobs" in lib.kg_last_error()
    assert lib.kg_bn_eval_coef(jobs, 9, None) < 0 and b"njobs" in lib.kg_last_error()
    assert lib.kg_bn_eval_coef(jobs, 2, None) < 0 and b"kg_bn_eval_coef" in lib.kg_last_error()        # C = 0
    jobs[0].C = jobs[1].C = 4
    assert lib.kg_bn_eval_coef(jobs, 2, None) < 0 and b"running statistics" in lib.kg_last_error()

    assert lib.kg_genblock_infer(None, None) < 0 and b"kg_genblock_infer" in lib.kg_last_error()
    a = _native._GenBlockInferArgs()
    assert lib.kg_genblock_infer(ctypes.byref(a), None) < 0 and b"kg_genblock_infer" in lib.kg_last_error()
    assert lib.kg_genblock_infer_lds_bytes(ctypes.byref(a)) < 0 and b"kg_genblock_infer_lds_bytes" in lib.kg_last_error()
    a = _infer_args(FRONT[0])
    assert lib.kg_genblock_infer(ctypes.byref(a), None) < 0 and b"does not fit" in lib.kg_last_error()
    a = _infer_args(GEOMETRIES[0])
    a.wg = a.wr = a.wt = None
    assert lib.kg_genblock_infer_lds_bytes(ctypes.byref(a)) >= 0
    assert lib.kg_genblock_infer(ctypes.byref(a), None) < 0 and b"null weight" in lib.kg_last_error()

    assert lib.kg_sample_inputs(None, None) < 0 and b"kg_sample_inputs" in lib.kg_last_error()
    s = _native._SampleInputsArgs()
    assert lib.kg_sample_inputs(ctypes.byref(s), None) < 0 and b"null step" in lib.kg_last_error()
    s.step, s.ticket = 0x1000, 0x2000
    assert lib.kg_sample_inputs(ctypes.byref(s), None) < 0 and b"nothing to write" in lib.kg_last_error()
    s.z = 0x3000
    assert lib.kg_sample_inputs(ctypes.byref(s), None) < 0 and b"latent" in lib.kg_last_error()
    s.z, s.noise = None, 0x3000
    assert lib.kg_sample_inputs(ctypes.byref(s), None) < 0 and b"noise_len" in lib.kg_last_error()

    assert lib.kg_trunc_lerp(None, 0, 0, 0, None, 0, 0, 0.5, None) < 0 and b"kg_trunc_lerp" in lib.kg_last_error()
    assert lib.kg_trunc_lerp(0x1000, 8, 0, 8, 0x2000, 8, 4, 0.5, None) < 0 and b"N=0" in lib.kg_last_error()
    assert lib.kg_trunc_lerp(0x1000, 4, 2, 8, 0x2000, 8, 4, 0.5, None) < 0 and b"x_ld" in lib.kg_last_error()


def test_genblock_infer_eligibility(lib):
    """the six compile-time geometries fit; the weight-bound front blocks G0-G2 do not; a misaligned weight row rules
    out the 16-byte operand loads exactly as for the training forward"""
    for geo in GEOMETRIES:
        assert lib.kg_genblock_infer_lds_bytes(ctypes.byref(_infer_args(geo))) >= 0, geo
    for geo in FRONT:
        assert lib.kg_genblock_infer_lds_bytes(ctypes.byref(_infer_args(geo))) == -1, geo
    assert lib.kg_genblock_infer_lds_bytes(ctypes.byref(_infer_args(GEOMETRIES[0], aligned=False))) == -1
    # the emulation's rule agrees
    for geo, want in [(g, True) for g in GEOMETRIES] + [(g, False) for g in FRONT]:
        cin, c, kp, tc, vc, v, rep, res = geo
        d = _native.GenBlockDims(Cin=cin, C=c, K=3, Kp=kp, Tc=tc, Vc=vc, T=tc * rep, V=v, rep=rep, res_kind=res, bn_t=False, act=1)
        assert sample_def.genblock_infer_supported(d, 2, None, None, None) is want, geo


def _pair_inputs(cfg="h36m"):
    c, G, D, Go, Do = build_pair(cfg)
    nn_ = G.graph.num_node
    real, labels, z, alpha = rand_inputs(4, c["channels"], c["t_size"], nn_[0], c["n_classes"], c["latent"], seed=3)
    noise = rand_noise(4, c["t_size"], nn_, seed=6)
    return c, G, z, labels, noise


def _snapshot(G):
    return G.training, {k: v.clone() for k, v in G.state_dict().items()}


def _assert_untouched(G, snap):
    training, sd = snap
    assert G.training is training
    now = G.state_dict()
    assert list(now) == list(sd)
    for k, v in sd.items():
        assert torch.equal(now[k], v), k


def test_sampler_forward_matches_reference_eval_fixtures(golden_dir):
    from kinetic_gan_amd.sample import Sampler
    gold = np.load(os.path.join(golden_dir, "ref_h36m.npz"))
    c, G, z, labels, noise = _pair_inputs()
    snap = _snapshot(G)                      # (training mode: the Sampler must not need, or leave behind, eval())
    with sample_def.emulated_sampler_native():
        fused = []
        f0 = _native.genblock_infer
        _native.genblock_infer = lambda *a, **k: (fused.append(1), f0(*a, **k))[1]
        try:
            out = Sampler(G, qtd=1, use_graph=False).forward(z, labels, noise)
        finally:
            _native.genblock_infer = f0
        assert len(fused) == 2               # h36m: the last two blocks take the one-launch form
        err = rel_err(out, torch.as_tensor(gold["G_out_eval"]))
        print("Sampler.forward vs G_out_eval: %.3e" % err)
        assert err < FWD_TOL
        # W-space truncation with the fixture's draws (tests/golden/make_fixtures.py: numpy's global generator, seed 77)
        np.random.seed(77)
        t = torch.as_tensor(np.random.normal(0, 1, (1000, c["latent"] + c["n_classes"])), dtype=torch.float32)
        out_t = Sampler(G, qtd=1, trunc=0.7, trunc_mode="w", use_graph=False).forward(z, labels, noise, trunc_t=t)
        err_t = rel_err(out_t, torch.as_tensor(gold["G_out_eval_trunc"]))
        print("Sampler.forward vs G_out_eval_trunc: %.3e" % err_t)
        assert err_t < FWD_TOL
        _assert_untouched(G, snap)
        # G's own eval / no_grad forward (the folded path): the bound of the folded-vs-unfolded tests
        G.eval()
        with torch.no_grad():
            own = G(z, labels, noise=noise)
        G.train(True)
        err_o = rel_err(out, own)
        print("Sampler.forward vs G.eval() forward: %.3e" % err_o)
        assert err_o < 1e-5
        # Z-space truncation is generator.truncate_z with the same draws
        from kinetic_gan_amd.generator import truncate_z
        tz = t[:, :c["latent"]].contiguous()
        out_z = Sampler(G, qtd=1, trunc=0.7, trunc_mode="z", use_graph=False).forward(z, labels, noise, trunc_t=tz)
        G.eval()
        with torch.no_grad():
            own_z = G(truncate_z(z, 1000, 0.7, t=tz), labels, noise=noise)
        G.train(True)
        assert rel_err(out_z, own_z) < 1e-5


@pytest.mark.parametrize("label", [-1, 7])
def test_generate_order_and_generator_untouched(label):
    from kinetic_gan_amd.sample import Sampler, sample_actions
    c, G, z, labels, noise = _pair_inputs()
    with sample_def.emulated_sampler_native():
        np.random.seed(5)
        G.eval()
        imgs0, labs0, zs0 = sample_actions(G, c["n_classes"], c["latent"], gen_qtd=5, qtd=3, label=label)
        G.train(True)
        snap = _snapshot(G)
        s = Sampler(G, qtd=3, label=label, seed=11, use_graph=False)
        imgs, labs, zs = s.generate(5)
        _assert_untouched(G, snap)
    assert labs.tolist() == labs0.tolist()
    assert tuple(imgs.shape) == tuple(imgs0.shape) and tuple(zs.shape) == tuple(zs0.shape)
    assert torch.isfinite(imgs).all()
    # two rounds of draws: replay counters 0 and 1 of the z stream
    n = s.n
    for r in range(2):
        want = sample_def.sample_normals(n * c["latent"], 11, sample_def.S_Z, r).reshape(n, c["latent"])
        assert np.array_equal(zs[r * n:(r + 1) * n].numpy(), want)
    assert s.state_dict() == {"seed": 11, "step": 2}
    # resumed from the counter: the same next round
    with sample_def.emulated_sampler_native():
        a = s.next()[0].clone()
        s2 = Sampler(G, qtd=3, label=label, seed=3, use_graph=False)
        s2.load_state_dict({"seed": 11, "step": 2})
        assert torch.equal(s2.next()[0], a)


def test_sampler_streams_differ_from_training_streams():
    """counter word 1 of the sampler (0x100 + k) against the training streams' (k + 4 rank): for one seed and step none of
    the three sampler streams repeats one of the four training streams"""
    seed, step, n = 1234567, 3, 64
    train = [train_def.words(n, seed, k, step) for k in (train_def.STREAM_Z, train_def.STREAM_ALPHA, train_def.STREAM_NOISE_D,
                                                          train_def.STREAM_NOISE_G)]
    samp = [train_def.words(n, seed, k, step) for k in (sample_def.S_Z, sample_def.S_NOISE, sample_def.S_T)]
    for i, a in enumerate(samp):
        for b in train + samp[:i]:
            assert not np.array_equal(a, b) and (a == b).mean() < 0.05
    assert _native.STREAM_SAMPLE == sample_def.STREAM_SAMPLE == 0x100


def test_sampler_is_a_package_name():
    from kinetic_gan_amd.sample import Sampler
    assert kinetic_gan_amd.Sampler is Sampler
