"""Frechet pose / motion distance inside the Evaluator on the MI355X: kg_frechet_real + kg_frechet_sets against
kg_frechet set by set (bit for bit) and against the float64 definition (tests/frechet_def.py, within its own bracket), the
cache as the only thing read of the real side, the Sampler's layout, determinism and output coverage on poisoned, red-zoned
buffers, capture; then the Evaluator's new columns against their composition (a twin Sampler + metrics.frechet), the
untouched MMD / PRDC columns, replay against eager, the call count, selection by a Frechet score, the real side from arrays,
resume, the training loop and the command."""
import csv
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import metrics
from kinetic_gan_amd.evaluate import Evaluator
from kinetic_gan_amd.feeder import Feeder
from kinetic_gan_amd.generator import Generator
from kinetic_gan_amd.sample import Sampler
from kinetic_gan_amd.train import TrainLoop
from kinetic_gan_amd.wgan_gp import FlatParams

import eval_frechet_def
import eval_prdc_def
import train_def
from eval_frechet_def import MODES, SEED
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)
from util import build_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SET_KEYS = ("values", "terms", "sweeps", "mean", "mean32")
CACHE_KEYS = ("mu_real", "tr_real", "G", "sweeps_real")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    x, y = bits(a), bits(b)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)


# ---- 1. kg_frechet_sets against kg_frechet, set by set -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(nsets, K, n, m, t, C, V):
    """(real, fakes) float32 numpy and on the GPU; each made once"""
    real, fakes = eval_frechet_def.make_sets(SEED, nsets, K, n, m, C, t, V)
    return real, fakes, torch.from_numpy(real).to(DEV), [torch.from_numpy(f).to(DEV) for f in fakes]


def view(x):
    """(K, n, C, t, V) tensor -> FrechetView"""
    return nv.FrechetView(x, x.stride(0), x.stride(1), x.stride(3), x.stride(2))


def run_single(real, fake, mode):
    K, n, C, t, V = real.shape
    return nv.frechet(view(real), view(fake), n, fake.shape[1], t, mode == "motion", C, V, K, want_mean=True)


def run_real(real, mode):
    K, n, C, t, V = real.shape
    return nv.frechet_real(view(real), n, t, mode == "motion", C, V, K)


def run_sets(cache, fakes, mode, ws=None):
    K, m, C, t, V = fakes[0].shape
    f = view(fakes[0])
    if ws is None:
        ws = guard.empty(nv.frechet_sets_workspace_bytes(len(fakes), m, t, mode == "motion", C, V, K) // 8, dtype=torch.float64, device=DEV)
    return nv.frechet_sets(cache, fakes, f.sc, f.ss, f.sf, f.so, m, t, mode == "motion", C, V, K, ws=ws)


def assert_sets_equal_single_calls(out, cache, singles):
    for g, one in enumerate(singles):
        assert same_bits(out["values"][g], one["values"]), g
        assert same_bits(out["terms"][g], one["terms"]), g
        assert same_bits(out["sweeps"][g], one["sweeps"][:, 1]), g
        assert same_bits(out["mean"][g], one["mean"]), g
        assert same_bits(cache["sweeps_real"], one["sweeps"][:, 0]), g
        assert same_bits(cache["tr_real"], one["terms"][:, 1]), g
    assert same_bits(out["mean32"], out["mean"].to(torch.float32))           # the fp32 rounding of mean, exactly


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nsets,K,n,m,t,C,V", eval_frechet_def.SHAPES)
def test_sets_equal_kg_frechet_set_by_set(nsets, K, n, m, t, C, V, mode):
    _, _, real, fakes = case(nsets, K, n, m, t, C, V)
    d = C * V
    e = d + (d & 1)
    singles = [run_single(real, f, mode) for f in fakes]
    cache = run_real(real, mode)
    assert cache["mu_real"].shape == (K, d) and cache["tr_real"].shape == (K,) and cache["G"].shape == (K, e, e)
    assert cache["sweeps_real"].shape == (K,) and cache["sweeps_real"].dtype == torch.int32
    if d & 1:                                                 # the padding row and column are zero
        assert not cache["G"][:, d, :].any() and not cache["G"][:, :, d].any()
    out = run_sets(cache, fakes, mode)
    assert out["values"].shape == (nsets, K) and out["terms"].shape == (nsets, K, 4) and out["sweeps"].shape == (nsets, K)
    assert out["mean"].shape == (nsets,) and out["mean32"].shape == (nsets,) and out["mean32"].dtype == torch.float32
    assert_sets_equal_single_calls(out, cache, singles)
    moments = nv.frechet(view(real), view(fakes[0]), n, m, t, mode == "motion", C, V, K, moments=True)
    assert same_bits(cache["mu_real"], moments["mu_real"])
    if nsets > 1:
        assert not same_bits(out["values"][0], out["values"][1])              # (the sets do score differently)


# ---- 2. independence from kg_frechet: the float64 definition ---------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nsets,K,n,m,t,C,V", eval_frechet_def.DEF_SHAPES)
def test_sets_against_the_float64_definition(nsets, K, n, m, t, C, V, mode):
    """d = 15, 75 and 96; the bound is the definition's own end-to-end bracket, capped on the definition before the kernel's
    output is read"""
    real_np, fakes_np, real, fakes = case(nsets, K, n, m, t, C, V)
    refs = eval_frechet_def.reference_sets(real_np, fakes_np, mode)
    out = run_sets(run_real(real, mode), fakes, mode)
    o = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(np.isfinite(o[k]).all() for k in SET_KEYS)
    assert (o["sweeps"] >= 1).all() and (o["sweeps"] < 40).all(), o["sweeps"]
    for g, (per, mean) in enumerate(refs):
        for c, ref in enumerate(per):
            err = abs(o["values"][g, c] - ref["fd"])
            print("set %d class %d FD %.12g def %.12g err %.3g tol %.3g" % (g, c, o["values"][g, c], ref["fd"], err, ref["tol"]["e2e"]))
            assert err <= ref["tol"]["e2e"]
        assert abs(o["mean"][g] - mean) <= max(r["tol"]["e2e"] for r in per)
        assert o["mean32"][g] == np.float32(o["mean"][g])


# ---- 3. the cache is what is read ----------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
def test_the_cache_is_what_is_read(mode):
    _, _, real, fakes = case(2, 3, 5, 4, 8, 3, 5)
    real = guard.empty(real.shape, dtype=torch.float32, device=DEV).copy_(real)
    cache = run_real(real, mode)
    before = run_sets(cache, fakes, mode)
    real.fill_(float("nan"))                                  # the real data is gone: nothing may change
    after = run_sets(cache, fakes, mode)
    for key in SET_KEYS:
        assert same_bits(before[key], after[key]), key
    swapped = {k: v.clone() for k, v in cache.items()}
    swapped["G"][1] = cache["G"][0]                           # class 1 against the factor of class 0
    out = run_sets(swapped, fakes, mode)
    assert same_bits(out["terms"][:, :, :3], before["terms"][:, :, :3])
    for c in (0, 2):
        assert same_bits(out["terms"][:, c], before["terms"][:, c]) and same_bits(out["values"][:, c], before["values"][:, c])
        assert same_bits(out["sweeps"][:, c], before["sweeps"][:, c])
    assert (out["terms"][:, 1, 3] != before["terms"][:, 1, 3]).all() and (out["values"][:, 1] != before["values"][:, 1]).all()


# ---- 4. the Sampler's layout ---------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [3, 1])
def test_fakes_in_a_plane_buffer(C, mode):
    """the fakes as a Sampler round leaves them: a channel-major plane, row j*K + c = sample j of class c, frame stride V,
    outer stride T*V per channel of the whole batch (C > 1) - against contiguous class-major copies"""
    K, P, T, V = 3, 6, 7, 5
    gen = torch.Generator().manual_seed(3)
    planes = []
    for g in range(2):
        pl = nv.new_plane(P * K, C, T, V, DEV)
        pl.copy_(torch.randn((P * K, C, T, V), generator=gen).to(DEV))
        assert pl.stride(0) == T * V and (C == 1 or pl.stride(1) == P * K * T * V)
        planes.append(pl)
    real = torch.randn((K, P, C, T, V), generator=gen).to(DEV)
    cache = run_real(real, mode)
    sn, sc = nv._sn_sc(planes[0])
    ws = guard.empty(nv.frechet_sets_workspace_bytes(2, P, T, mode == "motion", C, V, K) // 8, dtype=torch.float64, device=DEV)
    out = nv.frechet_sets(cache, planes, sn, K * sn, V, sc if C > 1 else 0, P, T, mode == "motion", C, V, K, ws=ws)
    copies = [pl.reshape(P, K, C, T, V).transpose(0, 1).contiguous() for pl in planes]          # class-major
    want = run_sets(cache, copies, mode)
    for key in SET_KEYS:
        assert same_bits(out[key], want[key]), key
    assert_sets_equal_single_calls(out, cache, [run_single(real, f, mode) for f in copies])
    short = guard.empty(planes[1].numel() // 2, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="fake set 1 reach outside"):
        nv.frechet_sets(cache, [planes[0], short], sn, K * sn, V, sc if C > 1 else 0, P, T, mode == "motion", C, V, K, ws=ws)


# ---- 5. determinism and output coverage ----------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("mode", MODES)
def test_deterministic_on_poisoned_workspaces_and_every_word_written(mode):
    nsets, K, n, m, t, C, V = 2, 2, 5, 9, 16, 3, 5             # several chunks per set: the merge has something to sum
    _, _, real, fakes = case(nsets, K, n, m, t, C, V)
    diff = mode == "motion"
    caches = []
    for fill in (guard.PATTERN_A, 0):
        words = nv.frechet_real_workspace_bytes(n, t, diff, C, V, K) // 4
        ws = guard.full((words,), fill, dtype=torch.int32, device=DEV).view(torch.float64)
        caches.append(nv.frechet_real(view(real), n, t, diff, C, V, K, ws=ws))
    for key in CACHE_KEYS:
        assert same_bits(caches[0][key], caches[1][key]), key
        guard.assert_no_poison(caches[0][key], key)
    outs = []
    for fill in (guard.PATTERN_A, 0):
        words = nv.frechet_sets_workspace_bytes(nsets, m, t, diff, C, V, K) // 4
        ws = guard.full((words,), fill, dtype=torch.int32, device=DEV).view(torch.float64)
        outs.append(run_sets(caches[0], fakes, mode, ws=ws))
        outs.append(run_sets(caches[0], fakes, mode, ws=ws))                  # and on what the call itself left there
    for other in outs[1:]:
        for key in SET_KEYS:
            assert same_bits(outs[0][key], other[key]), key
    for key in SET_KEYS:
        guard.assert_no_poison(outs[0][key], key)
    fewer = run_sets(caches[0], fakes[1:], mode, ws=ws)                       # fewer sets on the same workspace
    assert_sets_equal_single_calls(fewer, caches[0], [run_single(real, fakes[1], mode)])


# ---- 6. capture ----------------------------------------------------------------------------------------------------------

def test_graph_capture_follows_fakes_and_cache():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    mode = "motion"
    real_np, fakes_np = eval_frechet_def.make_sets(2, 2, 3, 6, 5, 3, 6, 5)
    real2_np, fakes2_np = eval_frechet_def.make_sets(5, 2, 3, 6, 5, 3, 6, 5)
    real, real2 = torch.from_numpy(real_np).to(DEV), torch.from_numpy(real2_np).to(DEV)
    fakes = [torch.from_numpy(f).to(DEV) for f in fakes_np]
    cache = run_real(real, mode)
    ws = torch.empty(nv.frechet_sets_workspace_bytes(2, 5, 6, True, 3, 5, 3) // 8, dtype=torch.float64, device=DEV)
    before = {k: v.clone() for k, v in run_sets(cache, fakes, mode, ws=ws).items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run_sets(cache, fakes, mode, ws=ws)                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run_sets(cache, fakes, mode, ws=ws)
    g.replay()
    torch.cuda.synchronize()
    for key in SET_KEYS:
        assert same_bits(cap[key], before[key]), key
    for f, f2 in zip(fakes, fakes2_np):                       # new fake contents
        f.copy_(torch.from_numpy(f2))
    g.replay()
    torch.cuda.synchronize()
    eager = run_sets({k: v.clone() for k, v in cache.items()}, fakes, mode)
    for key in SET_KEYS:
        assert same_bits(cap[key], eager[key]), key
    assert not same_bits(eager["values"], before["values"])
    other = run_real(real2, mode)                             # another real set's cache, written over the first in place
    for key in CACHE_KEYS:
        cache[key].copy_(other[key])
    g.replay()
    torch.cuda.synchronize()
    eager2 = run_sets(other, fakes, mode)
    for key in SET_KEYS:
        assert same_bits(cap[key], eager2[key]), key
    assert not same_bits(eager2["values"], eager["values"])
    assert_sets_equal_single_calls(eager2, other, [run_single(real2, f, mode) for f in fakes])


# ---- 7. the Evaluator's columns ------------------------------------------------------------------------------------------

CFG, SEED_EV, PER, KNN, PER_OWN = "h36m", 5, 8, 3, 6
OLD = ["a/avg", "a/joint", "b/avg", "b/joint"] + ["%s/%s" % (g, q) for g in ("a", "b") for q in metrics.PRDC_NAMES]
NEW = ["a/pose_fd", "a/motion_fd", "b/pose_fd", "b/motion_fd"]


def eval_feeder(path, n=200):
    os.makedirs(path, exist_ok=True)
    dp, lp = train_def.synthetic_dataset(str(path), n, 2, 40, 16, 10, "h36m", seed=4)
    return Feeder(dp, lp, dataset="h36m")


def flat_generator():
    c, G, _, _, _ = build_pair(CFG, DEV)
    G._flat_keep = FlatParams(G)             # the buffer the parameters now live in
    return c, G


def ev_state(ev):
    out = {"count": ev.count, "ring_val": ev.ring_val, "ring_iter": ev.ring_iter, "best_val": ev.best_val, "best_iter": ev.best_iter,
           "snap_flat": ev.snap_flat}
    for k, b in ev.snap_buffers.items():
        out["snap." + k] = b
    for name, group in (("step.", ev.samplers), ("prdc_step.", ev.prdc_samplers), ("frechet_step.", ev.frechet_samplers)):
        for k, s in group.items():
            out[name + k] = s.step_dev
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def assert_same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert same_bits(a[k], b[k]), "%s: %s differs" % (what, k)


def make_ev(gens, feeder, it=None, **kw):
    kw.setdefault("select", "a/avg")
    return Evaluator(gens, feeder, pairs=2, seed=SEED_EV, iteration=it, ring_len=8, **kw)


KINDS = {"shared": dict(prdc_per_class=PER, prdc_k=KNN, frechet_per_class=PER),           # the PRDC round is read
         "own": dict(prdc_per_class=PER, prdc_k=KNN, frechet_per_class=PER_OWN)}          # a third round per generator


@pytest.fixture(scope="module")
def composed(tmp_path_factory):
    """two generators with the same weights, pairs = 2, 8 samples per class for PRDC with k = 3; Frechet on 8 per class (the
    PRDC round) and on 6 per class (rounds of its own): three replayed evaluations each, next to an Evaluator with PRDC alone"""
    feeder = eval_feeder(tmp_path_factory.mktemp("ev"))
    c, Ga = flat_generator()
    _, Gb = flat_generator()
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    evs = {k: make_ev({"a": Ga, "b": Gb}, feeder, it, **kw) for k, kw in KINDS.items()}
    evs["prdc"] = make_ev({"a": Ga, "b": Gb}, feeder, it, prdc_per_class=PER, prdc_k=KNN)
    assert all(e.use_graph for e in evs.values())
    states = {k: [] for k in evs}
    for k in range(3):
        for name, e in evs.items():
            e.evaluate()
            states[name].append(ev_state(e))
        it += 2
    return dict(feeder=feeder, c=c, Ga=Ga, Gb=Gb, evs=evs, states=states, recs={k: e.records() for k, e in evs.items()})


def twin_round(G, counter, qtd):
    s = Sampler(G, qtd=qtd, seed=SEED_EV, use_graph=False)
    s.load_state_dict({"seed": SEED_EV, "step": counter})
    out, _, _ = s.next()
    torch.cuda.synchronize()
    return out, s


@pytest.mark.parametrize("kind,per", [("shared", PER), ("own", PER_OWN)])
def test_columns_equal_the_composition(composed, kind, per):
    ev, rec, plain = composed["evs"][kind], composed["recs"][kind], composed["recs"]["prdc"]
    assert rec["names"] == OLD + NEW and rec["scores"].shape == (3, 16) and plain["names"] == OLD
    # the MMD and PRDC columns do not move: bit for bit those of the Evaluator without Frechet, and so does what they decide
    assert same_bits(rec["scores"][:, :12], plain["scores"])
    assert same_bits(rec["improved"], plain["improved"]) and same_bits(rec["iteration"], plain["iteration"])
    assert ev.best() == composed["evs"]["prdc"].best()
    for key in ("count", "ring_iter", "best_val", "best_iter", "snap_flat", "step.a", "step.b", "prdc_step.a", "prdc_step.b"):
        assert same_bits(composed["states"][kind][-1][key], composed["states"]["prdc"][-1][key]), key
    # a shared round is not a Sampler of its own, and nothing is counted twice
    assert len(ev.frechet_samplers) == (0 if kind == "shared" else 2)
    assert len(ev._all_samplers()) == len(set(map(id, ev._all_samplers()))) == (4 if kind == "shared" else 6)
    assert all(s.step_count == 3 for s in ev._all_samplers())
    # the real side: the protocol's selection, class by class
    data, labels, _ = metrics.select_reference_samples(composed["feeder"], np.arange(10), 32, per_class=per)
    assert same_bits(ev.frechet_real, data) and sorted(ev.frechet_cache) == ["motion", "pose"]
    real = torch.as_tensor(data).to(DEV)
    # the FD columns: metrics.frechet of a twin Sampler round against that selection, its fp64 mean rounded to fp32
    for k in range(3):
        out, s = twin_round(composed["Ga"], k, per)
        assert out.shape == (10 * per, 2, 32, 16) and s.labels_np.tolist() == list(range(10)) * per
        for i, mode in enumerate(MODES):
            want = metrics.frechet(out, real, s.labels_np, labels, mode=mode)
            print("evaluation", k, mode, "FD", float(want["mean"]))
            assert same_bits(rec["scores"][k, 12 + i:13 + i], want["mean"].to(torch.float32).reshape(1)), (k, mode)
            if k == 0:
                assert same_bits(ev.frechet_cache[mode]["sweeps_real"], want["sweeps"][:, 0])
                assert same_bits(ev.frechet_cache[mode]["tr_real"], want["terms"][:, 1])
    assert np.isfinite(rec["scores"]).all() and (rec["scores"][:, 12:] > 0).all()
    assert same_bits(rec["scores"][:, 12:14], rec["scores"][:, 14:16])        # equal weights behind another Sampler
    state = ev.state_dict()
    assert state["frechet"] == {"per_class": per, "modes": ["pose", "motion"]} and "frechet" not in composed["evs"]["prdc"].state_dict()
    assert state["prdc"] == {"per_class": PER, "k": KNN} and state["names"] == OLD + NEW
    assert not any(k.startswith("frechet_") for k in state)


@pytest.mark.parametrize("kind", ["shared", "own"])
def test_replays_equal_eager_evaluations(composed, kind):
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, composed["feeder"], it, use_graph=False, **KINDS[kind])
    for k in range(3):
        ev.evaluate()
        it += 2
        assert_same(composed["states"][kind][k], ev_state(ev), "graph vs eager, evaluation %d" % k)
    a, b = ev.records(), composed["recs"][kind]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))


def test_frechet_alone_and_one_mode(composed):
    """without PRDC the record still goes through kg_eval_record2; one mode: one column per generator"""
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, composed["feeder"], frechet_per_class=PER, frechet_modes=("motion",),
                 select="b/motion_fd")
    assert ev.names == OLD[:4] + ["a/motion_fd", "b/motion_fd"] and not ev.maximise and not ev.prdc_samplers
    ev.evaluate()
    rec = ev.records()
    assert same_bits(rec["scores"][0, :4], composed["recs"]["prdc"]["scores"][0, :4])
    assert same_bits(rec["scores"][0, 4:], composed["recs"]["shared"]["scores"][0, [13, 15]])
    assert rec["improved"].tolist() == [True] and ev.best()["value"] == float(rec["scores"][0, 5])


def test_one_kg_frechet_sets_call_per_mode_for_two_generators(composed, monkeypatch):
    calls, reals = [], []
    plain_sets, plain_real = nv.frechet_sets, nv.frechet_real
    monkeypatch.setattr(nv, "frechet_sets", lambda cache, fakes, *a, **kw: (calls.append(len(list(fakes))), plain_sets(cache, fakes, *a, **kw))[1])
    monkeypatch.setattr(nv, "frechet_real", lambda *a, **kw: (reals.append(1), plain_real(*a, **kw))[1])
    for kind in KINDS:
        ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, composed["feeder"], use_graph=False, **KINDS[kind])
        assert reals == [1, 1] and calls == []                # the real side: once per mode, at construction
        ev.evaluate()
        torch.cuda.synchronize()
        assert calls == [2, 2] and reals == [1, 1], (kind, calls, reals)       # one call per mode, both generators in it
        del calls[:], reals[:]


def test_real_side_from_arrays(composed):
    """``real`` / ``real_labels``: the first 8 samples of every class in index order, class by class - handed the samples the
    Feeder route selects (in index order), it builds the same real side, the same cache and the same columns"""
    feeder = composed["feeder"]
    _, _, index = metrics.select_reference_samples(feeder, np.arange(10), 32, per_class=PER)
    idx = np.sort(index)
    data = np.stack([np.asarray(feeder[int(i)][0], dtype=np.float32)[:, :32] for i in idx])
    lab = np.asarray(feeder.label)[idx]
    ev = make_ev({"a": composed["Ga"]}, torch.as_tensor(data), real_labels=lab, frechet_per_class=PER, use_graph=False)
    rows = np.concatenate([np.flatnonzero(lab == c)[:PER] for c in range(10)])
    ref = composed["evs"]["shared"]
    assert same_bits(ev.frechet_real, data[rows]) and same_bits(ev.frechet_real, ref.frechet_real)
    for mode in MODES:
        for key in CACHE_KEYS:
            assert same_bits(ev.frechet_cache[mode][key], ref.frechet_cache[mode][key]), (mode, key)
    ev.evaluate()
    assert same_bits(ev.records()["scores"][0, 2:], composed["recs"]["shared"]["scores"][0, 12:14])
    with pytest.raises(ValueError, match="class_rows"):
        make_ev({"a": composed["Ga"]}, torch.as_tensor(data[:60]), real_labels=lab[:60], frechet_per_class=PER)


# ---- 8. selection by a Frechet score -------------------------------------------------------------------------------------

SCALES = [1.0, 0.9, float("nan"), 1.1, 0.8, 1.0]


def test_selection_by_motion_fd(composed):
    """the generator's weights are scaled between the evaluations so that the score moves, and once they are NaN; the improved
    flags and best() are the definition's, fed with the device's scores; the snapshot holds the weights of the evaluation with
    the smallest value, and the NaN evaluation never wins"""
    _, G = flat_generator()
    flat = G._flat_keep.flat
    orig = flat.clone()
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    ev = make_ev({"ema": G}, composed["feeder"], it, select="ema/motion_fd", frechet_per_class=PER)
    assert not ev.maximise and ev.best() == {"value": float("inf"), "iteration": -1}
    assert ev.names == ["ema/avg", "ema/joint", "ema/pose_fd", "ema/motion_fd"]
    weights = []
    for k, s in enumerate(SCALES):
        with torch.no_grad():
            flat.copy_(orig * s)
        weights.append(flat.detach().clone())
        it.fill_(10 * (k + 1))
        ev.evaluate()
    rec, best = ev.records(), ev.best()
    fd = rec["scores"][:, 3]
    print("ema/motion_fd per evaluation:", fd.tolist(), "improved:", rec["improved"].tolist(), "best:", best)
    assert np.isnan(fd[2]) and np.isfinite(np.delete(fd, 2)).all() and len(set(np.delete(fd, 2).tolist())) > 1
    ref = eval_prdc_def.Record2(4, 3, 8, maximise=False)
    for k in range(len(SCALES)):
        ref.append(rec["scores"][k], rec["iteration"][k])
    assert rec["improved"].tolist() == ref.ring_iter[:len(SCALES), 1].astype(bool).tolist() and rec["improved"][0]
    assert not rec["improved"][2]                                                             # a NaN never wins
    assert best == {"value": float(ref.best_val), "iteration": int(ref.best_iter)}
    assert best["value"] == float(np.nanmin(fd)) and best["iteration"] == 10 * (int(np.nanargmin(fd)) + 1)     # the FIRST minimum
    k_best = best["iteration"] // 10 - 1
    assert k_best != 2 and same_bits(ev.snap_flat, weights[k_best])
    B = ev.best_generator()
    c = composed["c"]
    F = Generator(c["latent"], c["channels"], c["n_classes"], c["t_size"], c["mlp"], dataset="h36m")
    assert list(B.state_dict().keys()) == list(F.state_dict().keys())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev.reset()
    assert ev.best() == {"value": float("inf"), "iteration": -1} and all(int(s.step_dev.item()) == 0 for s in ev._all_samplers())


# ---- 9. resume, the training loop and the command ------------------------------------------------------------------------

B_LOOP, SEED_LOOP, N_CRITIC, DECAY = 4, 3, 2, 0.9
LOOP_NAMES = ["live/avg", "live/joint", "ema/avg", "ema/joint"] + ["%s/%s" % (g, q) for g in ("live", "ema") for q in metrics.PRDC_NAMES] \
    + ["live/pose_fd", "live/motion_fd", "ema/pose_fd", "ema/motion_fd"]


def loop_state(loop):
    tr = loop.trainer
    out = {}
    for name, f, m in (("G", tr.fG, loop.G), ("D", tr.fD, loop.D)):
        out[name + ".flat"], out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = f.flat, f.exp_avg, f.exp_avg_sq
        out[name + ".grad"], out[name + ".adam_step"] = f.grad, f.step
        for k, b in m.named_buffers():
            out[name + ".buf." + k] = b
    out["G.ema"] = tr.fG.ema
    out["step_dev"] = loop.step_dev
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def make_loop(path, **kw):
    c, G, D, _, _ = build_pair(CFG, DEV)
    kw.setdefault("ema_decay", DECAY)
    return TrainLoop(G, D, eval_feeder(path), B_LOOP, c["t_size"], n_critic=N_CRITIC, seed=SEED_LOOP, eval_pairs=2, **kw)


# PRDC on 8 and Frechet on 6 samples per class: the Frechet rounds have Samplers - and counters - of their own
FD_KW = dict(eval_interval=2, eval_prdc=PER, eval_prdc_k=KNN, eval_frechet=PER_OWN, eval_select="ema/motion_fd")


@pytest.fixture(scope="module")
def six_steps(tmp_path_factory):
    loop = make_loop(tmp_path_factory.mktemp("six"), **FD_KW)
    ev = loop.evaluator
    assert ev is not None and ev.use_graph and ev.select == "ema/motion_fd" and not ev.maximise and ev.names == LOOP_NAMES
    assert len(ev._all_samplers()) == 6
    states, evs = [], {}
    for k in range(6):
        loop.step()
        states.append(loop_state(loop))
        if (k + 1) % 2 == 0:
            evs[k + 1] = ev_state(ev)
    d, g = loop.losses()
    return dict(loop=loop, states=states, evs=evs, d=d, g=g, rec=ev.records(), best=ev.best())


def test_resume_is_bit_exact(six_steps, tmp_path):
    rec = six_steps["rec"]
    print("loop scores", rec["scores"].tolist(), "best", six_steps["best"])
    assert rec["iteration"].tolist() == [2, 4, 6] and rec["scores"].shape == (3, 16) and np.isfinite(rec["scores"]).all()
    loop = make_loop(tmp_path / "a", **FD_KW)
    for _ in range(3):
        loop.step()
    sd = loop.state_dict()
    assert sd["eval"]["count"] == 1 and sd["eval"]["step"] == 1
    assert sd["eval"]["frechet"] == {"per_class": PER_OWN, "modes": ["pose", "motion"]}
    path = str(tmp_path / "loop_state.pth")
    torch.save(sd, path)
    del loop
    loop2 = make_loop(tmp_path / "b", **FD_KW)
    with torch.no_grad():                      # a different starting point: everything must come from the file
        loop2.trainer.fG.flat.add_(0.25)
        loop2.evaluator.snap_flat.fill_(3.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loop2.load_state_dict(torch.load(path, weights_only=False))
    assert_same(six_steps["states"][2], loop_state(loop2), "loaded state")
    for _ in range(3):
        loop2.step()
    assert_same(six_steps["states"][5], loop_state(loop2), "3 + resume + 3 vs 6")
    assert_same(six_steps["evs"][6], ev_state(loop2.evaluator), "3 + resume + 3 vs 6, evaluator")
    got = loop2.evaluator.records()
    assert all(same_bits(got[k], rec[k]) for k in ("iteration", "scores", "improved"))
    assert loop2.evaluator.best() == six_steps["best"]
    assert len(loop2.evaluator._all_samplers()) == 6 and all(s.step_count == 3 for s in loop2.evaluator._all_samplers())
    # a differing frechet entry, and a state without one, raise before anything is loaded
    state = torch.load(path, weights_only=False)
    for kw in (dict(eval_frechet=PER_OWN + 1), dict(eval_frechet_modes=("motion",)), dict(eval_frechet=0, eval_select="ema/avg")):
        args = dict(FD_KW, use_graph=False)
        args.update(kw)
        other = make_loop(tmp_path / "c", **args)
        flat = other.trainer.fG.flat.clone()
        with pytest.raises(ValueError, match="frechet"):
            other.load_state_dict(state)
        assert same_bits(flat, other.trainer.fG.flat)
    # the parent's format: no "frechet" key; it loads into a loop without the option and not into one with it
    old_kw = dict(eval_interval=2, eval_prdc=PER, eval_prdc_k=KNN, eval_select="ema/coverage", use_graph=False)
    plain = make_loop(tmp_path / "d", **old_kw)
    plain.step()
    plain.step()
    old = plain.state_dict()
    assert "frechet" not in old["eval"] and old["eval"]["count"] == 1
    again = make_loop(tmp_path / "e", **old_kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again.load_state_dict(old)
    assert_same(ev_state(plain.evaluator), ev_state(again.evaluator), "a state of the parent's format")
    other = make_loop(tmp_path / "f", use_graph=False, **FD_KW)
    with pytest.raises(ValueError, match="frechet"):
        other.load_state_dict(old)


def test_evaluation_with_frechet_only_observes(six_steps, tmp_path):
    loop = make_loop(tmp_path)
    assert loop.evaluator is None
    for k in range(6):
        loop.step()
        assert_same(six_steps["states"][k], loop_state(loop), "with vs without evaluation, iteration %d" % k)
    d, g = loop.losses()
    assert same_bits(d, six_steps["d"]) and same_bits(g, six_steps["g"])
    # the record against the definition: the averaged generator's motion distance decides, smaller is better
    rec, ev = six_steps["rec"], six_steps["loop"].evaluator
    ref = eval_prdc_def.Record2(16, 15, ev.ring_len, maximise=False)
    for k in range(3):
        ref.append(rec["scores"][k], rec["iteration"][k])
    assert six_steps["best"] == {"value": float(ref.best_val), "iteration": int(ref.best_iter)}
    assert rec["improved"].tolist() == ref.ring_iter[:3, 1].astype(bool).tolist()


def test_train_command_end_to_end(tmp_path):
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 200, 2, 40, 16, 10, "h36m", seed=4)
    out = str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--n_epochs", "1", "--batch_size", "8", "--dataset", "h36m",
           "--channels", "2", "--v_size", "16", "--t_size", "32", "--n_classes", "10", "--n_critic", "2",
           "--sample_interval", "10", "--checkpoint_interval", "10", "--log_interval", "5", "--seed", "1",
           "--data_path", dp, "--label_path", lp, "--ema_decay", "0.9", "--out", out, "--eval_interval", "5", "--eval_pairs", "2",
           "--eval_frechet", str(PER), "--eval_select", "live/motion_fd"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "[best live/motion_fd: " in r.stdout
    names = LOOP_NAMES[:4] + LOOP_NAMES[12:]
    rows = list(csv.reader(open(os.path.join(out, "metrics.csv"))))
    assert rows[0] == ["iteration"] + names + ["improved"] and len(rows) == 6
    state = torch.load(os.path.join(out, "loop_state.pth"), weights_only=False)["eval"]
    assert state["frechet"] == {"per_class": PER, "modes": ["pose", "motion"]} and "prdc" not in state
    assert state["select"] == "live/motion_fd" and state["names"] == names
    rec = state["records"]
    assert [int(r_[0]) for r_ in rows[1:]] == rec["iteration"].tolist() == [5, 10, 15, 20, 25]
    back = np.array([[float(v) for v in r_[1:9]] for r_ in rows[1:]], dtype=np.float32)
    assert same_bits(back, rec["scores"]) and np.isfinite(back).all()
    assert [int(r_[9]) for r_ in rows[1:]] == rec["improved"].astype(int).tolist()
    ref = eval_prdc_def.Record2(8, 5, 1024, maximise=False)
    for k in range(5):
        ref.append(rec["scores"][k], rec["iteration"][k])
    assert int(state["best_iter"].item()) == int(ref.best_iter) and rec["improved"].tolist() == ref.ring_iter[:5, 1].astype(bool).tolist()
    model = os.path.join(out, "models", "generator_best.pth")
    best = torch.load(model)
    F = Generator(512, 2, 10, 32, 4, dataset="h36m")
    assert list(best.keys()) == list(F.state_dict().keys())
    F.load_state_dict(best, strict=True)
    gen_out = str(tmp_path / "gen")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "generate.py"), "--batch_size", "10", "--gen_qtd", "10", "--dataset", "h36m",
           "--channels", "2", "--v_size", "16", "--t_size", "32", "--n_classes", "10", "--model", model, "--out", gen_out, "--seed", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert any(f.endswith("_gen_data.npy") for f in os.listdir(os.path.join(gen_out, "actions")))
