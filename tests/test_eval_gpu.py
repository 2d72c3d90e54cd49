"""Scoring the generator during training on the MI355X: kg_eval_record and kg_copy_if against the host
definition (tests/eval_def.py) on poisoned, red-zoned buffers, the Evaluator against its composition (a twin Sampler +
metrics.calculate_mmd) and against the float64 definition of the MMD protocol, the captured training loop with
evaluation, resume, the commands.

Everything is compared bit for bit; the one comparison with float64 (tests/mmd_def.py) uses the rule of
tests/test_mmd_gpu.py (check_mmd2 / check_frame_mean) unchanged.
"""
import csv
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
from kinetic_gan_amd.checkpoint import AsyncCheckpointWriter
from kinetic_gan_amd.evaluate import Evaluator
from kinetic_gan_amd.feeder import Feeder
from kinetic_gan_amd.generator import Generator
from kinetic_gan_amd.sample import Sampler
from kinetic_gan_amd.train import TrainLoop
from kinetic_gan_amd.wgan_gp import FlatParams

import eval_def
import mmd_def
import train_def
from test_mmd_gpu import check_frame_mean, check_mmd2, nctv_groups, run_nctv
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)
from util import build_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SEQ = [3, 2, 2, float("nan"), 5, 1, float("inf"), 1, 0.5]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    x, y = bits(a), bits(b)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)


# ---- 1. kg_eval_record ---------------------------------------------------------------------------------------------------

def guarded_from(a):
    """a guarded device buffer holding the numpy array a"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return guard.empty(t.shape, dtype=t.dtype, device=DEV).copy_(t)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("it0", [None, 2 ** 24 + 1], ids=["iter-null", "iter-above-2^24"])
@pytest.mark.parametrize("nscores,select", [(1, 0), (4, 0), (4, 3)])
def test_record_against_definition(nscores, select, it0):
    """the issue's score sequence in the deciding column (other columns: values that would decide differently); ring of 4
    (it wraps); every ring row, flag, best_val, best_iter and count after every call, bit for bit"""
    ref = eval_def.Record(nscores, select, 4)
    scores = [guard.empty(1, dtype=torch.float32, device=DEV) for _ in range(nscores)]
    it = guard.empty(1, dtype=torch.int64, device=DEV) if it0 is not None else None
    count = guarded_from(np.zeros(1, np.int64))
    ring_val, ring_iter = guarded_from(ref.ring_val), guarded_from(ref.ring_iter)
    best_val, best_iter = guarded_from(np.array([np.inf], np.float32)), guarded_from(np.array([-1], np.int64))
    flag = guard.empty(1, dtype=torch.int32, device=DEV)          # (poison: every call must write it)
    for k, s in enumerate(SEQ):
        row = [np.float32(s) if i == select else np.float32(100.0 - 7 * k + i if (k + i) % 3 else np.nan) for i in range(nscores)]
        for t, v in zip(scores, row):
            t.fill_(float(v))
        itk = None if it0 is None else it0 + 3 * k
        if it is not None:
            it.fill_(itk)
        nv.eval_record(scores, select, it, count, ring_val, ring_iter, best_val, best_iter, flag)
        improved = ref.append(row, itk)
        torch.cuda.synchronize()
        what = (nscores, select, it0, k)
        assert same_bits(ring_val, ref.ring_val), what
        assert np.array_equal(ring_iter.cpu().numpy(), ref.ring_iter), what
        assert int(flag.item()) == int(improved) == int(ref.flag), what
        assert same_bits(best_val, np.array([ref.best_val], np.float32)), what
        assert int(best_iter.item()) == int(ref.best_iter) and int(count.item()) == ref.count == k + 1, what
    assert ref.best_val == np.float32(0.5) and int(best_iter.item()) == (-1 if it0 is None else it0 + 24)
    if it0 is not None:
        assert float(np.float32(it0 + 24)) != it0 + 24            # (an fp32 record could not hold this iteration)


# ---- 2. kg_copy_if -------------------------------------------------------------------------------------------------------

LENGTHS = [1, 3, 4, 5, 1023, 4099]


def shifted_empty(n, shift, dtype=torch.int32):
    """guarded, poisoned buffer of n elements whose first element lies `shift` elements behind a 16-byte boundary"""
    base = guard.empty(n + shift + 4, dtype=dtype, device=DEV)
    assert base.data_ptr() % 16 == 0
    out = base[shift:shift + n]
    assert out.is_contiguous() and out.data_ptr() % 16 == (shift * base.element_size()) % 16
    return base, out


def poisoned(t):
    return guard.poison_count(t) == t.numel() * t.element_size() // 4


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("dst_shift", [0, 1, 2])
@pytest.mark.parametrize("src_shift", [0, 1, 2])
def test_copy_if(src_shift, dst_shift):
    gen = torch.Generator().manual_seed(17 + 3 * src_shift + dst_shift)
    jobs, bases = [], []
    for n in LENGTHS:
        _, s = shifted_empty(n, src_shift)
        s.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32))
        b, d = shifted_empty(n, dst_shift)
        jobs.append((s.view(torch.float32), d.view(torch.float32)))         # (fp32 views: NaN payloads must survive too)
        bases.append(b)
    # an int64 tensor: two words per element (shifted by whole elements: 8 bytes, off the 16-byte grid when odd)
    _, s64 = shifted_empty(7, src_shift % 2, torch.int64)
    s64.copy_(torch.randint(-2 ** 62, 2 ** 62, (7,), generator=gen, dtype=torch.int64))
    b64, d64 = shifted_empty(7, dst_shift % 2, torch.int64)
    jobs.append((s64, d64))
    bases.append(b64)
    if src_shift == dst_shift == 0:
        assert all(s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0 for s, d in jobs)
    flag = guard.zeros(1, dtype=torch.int32, device=DEV)
    nv.copy_if(flag, jobs)
    torch.cuda.synchronize()
    for b in bases:                          # flag 0: nothing at all is written - the whole backing buffer keeps its poison
        assert poisoned(b)
    flag.fill_(1)
    nv.copy_if(flag, jobs)
    torch.cuda.synchronize()
    for (s, d), b in zip(jobs, bases):
        assert torch.equal(s.view(torch.int32), d.view(torch.int32)), (s.numel(), src_shift, dst_shift)
        words = d.numel() * d.element_size() // 4
        assert guard.poison_count(b) >= b.numel() * b.element_size() // 4 - words       # the slack around dst is untouched
    # the copy reads through pointers: new source values, the same call again
    for s, _ in jobs:
        s.view(torch.int32).add_(12345)
    flag.fill_(2)                            # any non-zero value
    nv.copy_if(flag, jobs)
    torch.cuda.synchronize()
    for s, d in jobs:
        assert torch.equal(s.view(torch.int32), d.view(torch.int32))


def test_copy_if_more_jobs_than_one_launch_and_replay():
    """40 jobs (two launches) inside a captured graph: the replay follows the flag and the sources"""
    src = [torch.full((i + 1,), float(i), device=DEV) for i in range(40)]
    dst = [torch.full((i + 1,), -1.0, device=DEV) for i in range(40)]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    jobs = list(zip(src, dst))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nv.copy_if(flag, jobs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        nv.copy_if(flag, jobs)
    graph.replay()
    torch.cuda.synchronize()
    assert all((d == -1).all() for d in dst)
    flag.fill_(1)
    for s in src:
        s.add_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(s, d) and (d == i + 0.5).all() for i, (s, d) in enumerate(jobs))


# ---- 3. bad arguments ----------------------------------------------------------------------------------------------------

def test_bad_arguments_raise():
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)      # noqa: E731
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)        # noqa: E731
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    t = f32(16)
    with pytest.raises(RuntimeError, match="overlap"):
        nv.copy_if(flag, [(t[0:8], t[4:12])])
    with pytest.raises(RuntimeError, match="overlap"):
        nv.copy_if(flag, [(f32(4), f32(4)), (t[4:12], t[0:8])])
    with pytest.raises(TypeError):
        nv.copy_if(flag.to(torch.int64), [(t[0:4], t[8:12])])
    with pytest.raises(TypeError):
        nv.copy_if(flag, [(t[0:4], i64(4))])
    with pytest.raises(TypeError):
        nv.copy_if(flag, [(t[0:4].half(), t[8:12].half())])
    with pytest.raises(ValueError):
        nv.copy_if(flag, [(t[0:4], t[8:13])])
    assert (t == 0).all()

    def rec(nscores=1, select=0, ring_len=4, **kw):
        a = dict(scores=[f32(1) for _ in range(nscores)], select=select, iteration=i64(1), count=i64(1),
                 ring_val=f32(ring_len, nscores), ring_iter=i64(ring_len, 2), best_val=f32(1), best_iter=i64(1), flag=flag)
        a.update(kw)
        nv.eval_record(**a)
    rec()                                    # (the arguments the cases below vary are otherwise fine)
    for kw, word in ((dict(nscores=2, select=2), "select"), (dict(nscores=4, select=7), "select"), (dict(nscores=0), "nscores"),
                     (dict(nscores=9), "nscores"), (dict(ring_len=0), "ring_len")):
        with pytest.raises(RuntimeError, match=word):
            rec(**kw)
    for kw in (dict(scores=[i64(1)]), dict(scores=[f32(2)]), dict(iteration=f32(1)), dict(count=torch.zeros(1, dtype=torch.int32, device=DEV)),
               dict(ring_val=f32(4, 1).double()), dict(ring_iter=torch.zeros(4, 2, dtype=torch.int32, device=DEV)),
               dict(best_val=i64(1)), dict(best_iter=f32(1)), dict(flag=i64(1))):
        with pytest.raises(TypeError):
            rec(**kw)
    with pytest.raises(ValueError):
        rec(ring_val=f32(4, 2))
    torch.cuda.synchronize()


# ---- 4. the Evaluator against its composition -----------------------------------------------------------------------------

CFG, SEED_EV = "h36m", 5


def eval_feeder(path, n=64):
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
    for k, s in ev.samplers.items():
        out["step." + k] = s.step_dev
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def assert_same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert same_bits(a[k], b[k]), "%s: %s differs" % (what, k)


def module_state(G):
    torch.cuda.synchronize()
    out = {"p." + k: p.detach().cpu().clone() for k, p in G.named_parameters()}
    out.update({"b." + k: b.detach().cpu().clone() for k, b in G.named_buffers()})
    return out


@pytest.fixture(scope="module")
def composed(tmp_path_factory):
    """two generators with the same weights behind one Evaluator, pairs = 2, both modes: three replayed evaluations"""
    feeder = eval_feeder(tmp_path_factory.mktemp("ev"))
    c, Ga = flat_generator()
    _, Gb = flat_generator()
    Ga.train()
    before = module_state(Ga), module_state(Gb)
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    ev = Evaluator({"a": Ga, "b": Gb}, feeder, pairs=2, select="a/avg", seed=SEED_EV, iteration=it, ring_len=8)
    assert ev.use_graph and ev.names == ["a/avg", "a/joint", "b/avg", "b/joint"] and ev.n == 20
    assert len(ev._jobs) == 25               # the flat parameters + (running_mean, running_var, num_batches_tracked) x 8 layers
    states = []
    for k in range(3):
        ev.evaluate()
        it += 2
        states.append(ev_state(ev))
    return dict(feeder=feeder, c=c, Ga=Ga, Gb=Gb, ev=ev, states=states, before=before, rec=ev.records(), best=ev.best())


def twin_round(G, counter, qtd=2):
    s = Sampler(G, qtd=qtd, seed=SEED_EV, use_graph=False)
    s.load_state_dict({"seed": SEED_EV, "step": counter})
    out, _, _ = s.next()
    torch.cuda.synchronize()
    return out.contiguous(), s


def test_scores_equal_the_composition(composed):
    ev, rec = composed["ev"], composed["rec"]
    assert rec["iteration"].tolist() == [2 ** 24 + 3, 2 ** 24 + 5, 2 ** 24 + 7] and rec["scores"].shape == (3, 4)
    assert np.isfinite(rec["scores"]).all() and (rec["scores"] > 0).all()
    assert ev.real.shape == (20, 2, 32, 16)
    for k in range(3):
        out, _ = twin_round(composed["Ga"], k)
        assert out.shape == (20, 2, 32, 16)
        for j, mode in enumerate(("avg", "joint")):
            want = metrics.calculate_mmd(out, ev.real, np.arange(20), mode)
            assert same_bits(rec["scores"][k, j], want.cpu().numpy()), (k, mode)
    # paired draws: the same weights behind another Sampler get the same scores
    assert same_bits(rec["scores"][:, :2], rec["scores"][:, 2:])
    assert not same_bits(rec["scores"][0], rec["scores"][1])                  # (another round, another draw)
    # the record against the definition, fed with the device's scores
    ref = eval_def.Record(4, 0, 8)
    for k in range(3):
        ref.append(rec["scores"][k], rec["iteration"][k])
    assert rec["improved"].tolist() == ref.ring_iter[:3, 1].astype(bool).tolist() and rec["improved"][0]
    assert composed["best"] == {"value": float(ref.best_val), "iteration": int(ref.best_iter)}
    assert same_bits(composed["states"][-1]["ring_val"], ref.ring_val)


def test_real_side_is_the_reordered_selection(composed, tmp_path):
    ev, feeder = composed["ev"], composed["feeder"]
    data, labels, _ = metrics.select_reference_samples(feeder, np.arange(10), 32, per_class=2)
    rows = eval_def.pair_rows(labels.tolist(), 10, 2)
    assert same_bits(ev.real, data[rows])
    with pytest.raises(ValueError, match="select_reference_samples"):      # the 40-sample variant: a class with one sample
        Evaluator({"a": composed["Ga"]}, eval_feeder(tmp_path, 40), pairs=2)


def test_against_float64_definition(composed):
    """one case against tests/mmd_def.py under the rule of tests/test_mmd_gpu.py: MMD^2 of every (pair, frame, bandwidth)
    and the per-pair frame means of the kg_mmd call whose mean IS the recorded score"""
    ev, rec = composed["ev"], composed["rec"]
    out, _ = twin_round(composed["Ga"], 0)
    for j, mode in enumerate(("avg", "joint")):
        res = run_nctv(out, ev.real, mode)
        torch.cuda.synchronize()
        assert same_bits(res["mean"].reshape(1), rec["scores"][0, j:j + 1])
        want, tol = check_mmd2(res["mmd2"], nctv_groups(out, mode), nctv_groups(ev.real, mode))
        groups = 32 if mode == "avg" else 1
        check_frame_mean(res["mmd"], want.reshape(20, groups, -1), tol.reshape(20, groups, -1))
        # the per-pair maximum over the bandwidths, on the kernel's own per-(pair, bandwidth) values (exact)
        per = [mmd_def.class_value(r) for r in res["mmd"].double().cpu().tolist()]
        assert same_bits(res["result"], np.array(per, np.float32))


def test_pairs_1_is_calculate_mmd_of_the_round(composed):
    G = composed["Ga"]
    ev = Evaluator({"g": G}, composed["feeder"], pairs=1, seed=SEED_EV, use_graph=False)
    assert ev.select == "g/avg"
    ev.evaluate()
    rec = ev.records()
    out, s = twin_round(G, 0, qtd=1)
    assert s.labels_np.tolist() == list(range(10)) and out.shape[0] == 10
    for j, mode in enumerate(("avg", "joint")):
        want = metrics.calculate_mmd(out, ev.real, s.labels_np, mode)
        assert same_bits(rec["scores"][0, j], want.cpu().numpy()), mode
    assert rec["iteration"].tolist() == [-1]             # no iteration tensor: recorded as -1


def test_replays_equal_eager_evaluations(composed):
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    ev = Evaluator({"a": composed["Ga"], "b": composed["Gb"]}, composed["feeder"], pairs=2, select="a/avg", seed=SEED_EV,
                   iteration=it, ring_len=8, use_graph=False)
    for k in range(3):
        ev.evaluate()
        it += 2
        assert_same(composed["states"][k], ev_state(ev), "graph vs eager, evaluation %d" % k)
    a, b = ev.records(), composed["rec"]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))


def test_evaluator_only_observes_and_snapshots_the_selected_generator(composed, tmp_path):
    Ga, Gb, ev = composed["Ga"], composed["Gb"], composed["ev"]
    for G, before in zip((Ga, Gb), composed["before"]):
        assert_same(before, module_state(G), "generator after three evaluations")
    assert Ga.training and Gb.training
    assert same_bits(ev.snap_flat, Ga._flat_keep.flat)
    B = ev.best_generator()
    assert ev.best_generator() is B and not B.training
    sd, want = B.state_dict(), Ga.state_dict()
    assert list(sd.keys()) == list(want.keys()) and all(torch.equal(sd[k], want[k]) for k in sd)
    lo = ev.snap_flat.data_ptr()
    assert all(lo <= p.data_ptr() < lo + 4 * ev.snap_flat.numel() and not p.requires_grad for p in B.parameters())
    assert all(b.data_ptr() == ev.snap_buffers[k].data_ptr() for k, b in B.named_buffers())
    # through the checkpoint writer into a fresh Generator, strictly
    w = AsyncCheckpointWriter()
    path = str(tmp_path / "generator_best.pth")
    w.save(B, path)
    w.close()
    c = composed["c"]
    F = Generator(c["latent"], c["channels"], c["n_classes"], c["t_size"], c["mlp"], dataset="h36m")
    loaded = torch.load(path)
    F.load_state_dict(loaded, strict=True)
    assert list(loaded.keys()) == list(sd.keys()) and all(torch.equal(loaded[k], sd[k].cpu()) for k in sd)
    # state_dict / load_state_dict continue bit for bit
    state = ev.state_dict()
    ev.evaluate()
    want_state, want_rec = ev_state(ev), ev.records()
    ev2 = Evaluator({"a": Ga, "b": Gb}, composed["feeder"], pairs=2, select="a/avg", seed=SEED_EV, iteration=ev.iteration, ring_len=8)
    ev2.load_state_dict(state)
    ev2.evaluate()
    assert_same(want_state, ev_state(ev2), "load_state_dict + one evaluation")
    got = ev2.records()
    assert all(same_bits(got[k], want_rec[k]) for k in ("iteration", "scores", "improved")) and len(got["iteration"]) == 4
    other = Evaluator({"a": Ga}, composed["feeder"], pairs=2, seed=SEED_EV, use_graph=False)
    with pytest.raises(ValueError):
        other.load_state_dict(state)


# ---- 5. in the loop ------------------------------------------------------------------------------------------------------

B_LOOP, SEED_LOOP, N_CRITIC, DECAY = 4, 3, 2, 0.9


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


@pytest.fixture(scope="module")
def six_steps(tmp_path_factory):
    loop = make_loop(tmp_path_factory.mktemp("six"), eval_interval=2)
    ev = loop.evaluator
    assert ev is not None and ev.use_graph and ev.select == "ema/avg" and ev.names == ["live/avg", "live/joint", "ema/avg", "ema/joint"]
    assert ev.iteration is loop.step_dev and loop.bpe == 16
    states, clones, evs = [], {}, {}
    for k in range(6):
        loop.step()
        states.append(loop_state(loop))
        if (k + 1) % 2 == 0:
            clones[k + 1] = {"ema": states[-1]["G.ema"], "buf": {q: b.detach().cpu().clone() for q, b in loop.G.named_buffers()}}
            evs[k + 1] = ev_state(ev)
    d, g = loop.losses()
    return dict(loop=loop, states=states, clones=clones, evs=evs, d=d, g=g, rec=ev.records(), best=ev.best())


def test_loop_records_and_snapshot(six_steps):
    rec, best, clones, ev = six_steps["rec"], six_steps["best"], six_steps["clones"], six_steps["loop"].evaluator
    assert rec["iteration"].tolist() == [2, 4, 6] and rec["scores"].shape == (3, 4) and np.isfinite(rec["scores"]).all()
    assert rec["improved"][0] and ev.n_evals == 3
    ref = eval_def.Record(4, 2, ev.ring_len)
    for k in range(3):
        ref.append(rec["scores"][k], rec["iteration"][k])
    assert best == {"value": float(ref.best_val), "iteration": int(ref.best_iter)} and best["iteration"] in (2, 4, 6)
    assert rec["improved"].tolist() == ref.ring_iter[:3, 1].astype(bool).tolist()
    # the snapshot is the averaged weights and the statistics AT the best evaluation, and not those of another one
    hit = clones[best["iteration"]]
    assert same_bits(ev.snap_flat, hit["ema"])
    assert set(ev.snap_buffers) == set(hit["buf"]) and all(torch.equal(ev.snap_buffers[k].cpu(), hit["buf"][k]) for k in hit["buf"])
    for itn, other in clones.items():
        if itn != best["iteration"]:
            assert not same_bits(ev.snap_flat, other["ema"]), itn
            assert any(not torch.equal(ev.snap_buffers[k].cpu(), other["buf"][k]) for k in other["buf"]), itn
    # the live and the averaged generator are different weights, scored on the same draws
    assert not same_bits(rec["scores"][:, :2], rec["scores"][:, 2:])
    sd = six_steps["loop"].state_dict()
    assert "eval" in sd and sd["eval"]["count"] == 3 and sd["eval"]["select"] == "ema/avg"


def test_evaluation_only_observes(six_steps, tmp_path):
    loop = make_loop(tmp_path)
    assert loop.evaluator is None and "eval" not in loop.state_dict()
    for k in range(6):
        loop.step()
        assert_same(six_steps["states"][k], loop_state(loop), "with vs without evaluation, iteration %d" % k)
    d, g = loop.losses()
    assert same_bits(d, six_steps["d"]) and same_bits(g, six_steps["g"])


def test_loop_replays_equal_eager_iterations(six_steps, tmp_path):
    loop = make_loop(tmp_path, eval_interval=2, use_graph=False)
    assert not loop.evaluator.use_graph
    for k in range(6):
        loop.step()
        assert_same(six_steps["states"][k], loop_state(loop), "graph vs eager, iteration %d" % k)
        if (k + 1) % 2 == 0:
            assert_same(six_steps["evs"][k + 1], ev_state(loop.evaluator), "graph vs eager, evaluation at %d" % (k + 1))
    d, g = loop.losses()
    assert same_bits(d, six_steps["d"]) and same_bits(g, six_steps["g"])
    rec = loop.evaluator.records()
    assert all(same_bits(rec[k], six_steps["rec"][k]) for k in ("iteration", "scores", "improved"))


# ---- 6. resume -----------------------------------------------------------------------------------------------------------

def test_resume_is_bit_exact(six_steps, tmp_path):
    loop = make_loop(tmp_path / "a", eval_interval=2)
    for _ in range(3):
        loop.step()
    sd = loop.state_dict()
    assert sd["eval"]["count"] == 1 and sd["eval"]["records"]["iteration"].tolist() == [2]
    path = str(tmp_path / "loop_state.pth")
    torch.save(sd, path)
    d0, g0 = loop.losses()
    del loop
    loop2 = make_loop(tmp_path / "b", eval_interval=2)
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
    rec = loop2.evaluator.records()
    assert all(same_bits(rec[k], six_steps["rec"][k]) for k in ("iteration", "scores", "improved"))
    assert loop2.evaluator.best() == six_steps["best"]
    d1, g1 = loop2.losses()
    assert same_bits(np.concatenate((d0, d1)), six_steps["d"]) and same_bits(np.concatenate((g0, g1)), six_steps["g"])
    # a loop without evaluation ignores the record in the state
    loop3 = make_loop(tmp_path / "c")
    loop3.load_state_dict(torch.load(path, weights_only=False))
    assert loop3.evaluator is None
    assert_same(six_steps["states"][2], loop_state(loop3), "state into a loop without evaluation")


def test_resume_mismatch_and_missing_record(tmp_path):
    loop = make_loop(tmp_path / "a", eval_interval=2)
    for _ in range(2):
        loop.step()
    sd = loop.state_dict()
    for kw, word in ((dict(eval_pairs=1), "pairs"), (dict(eval_select="live/avg"), "select"), (dict(eval_modes=("avg",)), "modes")):
        c, G, D, _, _ = build_pair(CFG, DEV)
        args = dict(n_critic=N_CRITIC, seed=SEED_LOOP, ema_decay=DECAY, eval_interval=2, eval_pairs=2, use_graph=False)
        args.update(kw)
        other = TrainLoop(G, D, loop.feeder, B_LOOP, c["t_size"], **args)
        flat = other.trainer.fG.flat.clone()
        with pytest.raises(ValueError, match=word):
            other.load_state_dict(sd)
        assert same_bits(flat, other.trainer.fG.flat)         # (raised before anything was loaded)
    plain = {k: v for k, v in sd.items() if k != "eval"}
    fresh = make_loop(tmp_path / "b", eval_interval=2, use_graph=False)
    fresh.evaluator.evaluate()
    with pytest.warns(UserWarning, match="record"):
        fresh.load_state_dict(plain)
    ev = fresh.evaluator
    assert ev.n_evals == 0 and len(ev.records()["iteration"]) == 0 and ev.best() == {"value": float("inf"), "iteration": -1}
    assert int(ev.count.item()) == 0 and all(int(s.step_dev.item()) == 0 for s in ev.samplers.values())
    assert fresh.step_count == 2


# ---- 7. commands ---------------------------------------------------------------------------------------------------------

def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_commands(tmp_path):
    dp, lp = train_def.synthetic_dataset(str(tmp_path), 64, 2, 40, 16, 10, "h36m", seed=4)
    common = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--n_epochs", "1", "--batch_size", "8", "--dataset", "h36m",
              "--channels", "2", "--v_size", "16", "--t_size", "32", "--n_classes", "10", "--n_critic", "2",
              "--sample_interval", "4", "--checkpoint_interval", "3", "--log_interval", "2", "--seed", "1",
              "--data_path", dp, "--label_path", lp, "--ema_decay", "0.9"]
    out_e, out_p = str(tmp_path / "run_eval"), str(tmp_path / "run_plain")
    r = subprocess.run(common + ["--out", out_e, "--eval_interval", "2", "--eval_pairs", "2"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "[best ema/avg: " in r.stdout
    r = subprocess.run(common + ["--out", out_p], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "[best " not in r.stdout
    plain = _tree(out_p)
    assert "metrics.csv" not in plain and "models/generator_best.pth" not in plain
    assert _tree(out_e) == sorted(plain + ["metrics.csv", "models/generator_best.pth"])
    state = torch.load(os.path.join(out_e, "loop_state.pth"), weights_only=False)
    assert "eval" not in torch.load(os.path.join(out_p, "loop_state.pth"), weights_only=False)
    ev = state["eval"]
    rec = ev["records"]
    assert rec["iteration"].tolist() == [2, 4, 6, 8]
    rows = list(csv.reader(open(os.path.join(out_e, "metrics.csv"))))
    assert rows[0] == ["iteration", "live/avg", "live/joint", "ema/avg", "ema/joint", "improved"] and len(rows) == 5
    assert [int(r_[0]) for r_ in rows[1:]] == rec["iteration"].tolist()
    assert [int(r_[5]) for r_ in rows[1:]] == rec["improved"].astype(int).tolist()
    back = np.array([[float(v) for v in r_[1:5]] for r_ in rows[1:]], dtype=np.float32)
    assert same_bits(back, rec["scores"])
    # the live outputs of the two runs are the same files: evaluation only observes
    for name in ("generator_3.pth", "generator_ema_3.pth", "discriminator_3.pth"):
        a = torch.load(os.path.join(out_e, "models", name))
        b = torch.load(os.path.join(out_p, "models", name))
        assert list(a.keys()) == list(b.keys()) and all(torch.equal(a[k], b[k]) for k in a), name
    # generator_best.pth: the snapshot, with the reference's keys, loadable strictly
    best = torch.load(os.path.join(out_e, "models", "generator_best.pth"))
    F = Generator(512, 2, 10, 32, 4, dataset="h36m")
    assert list(best.keys()) == list(F.state_dict().keys())
    F.load_state_dict(best, strict=True)
    fp = FlatParams(F)
    snap = ev["snapshot"]
    for (k, p), off in zip(F.named_parameters(), fp.offsets):
        assert same_bits(best[k], snap["flat"][off:off + p.numel()].view(p.shape)), k
    for k, b in snap["buffers"].items():
        assert torch.equal(best[k], b), k
    assert int(ev["best_iter"].item()) in (2, 4, 6, 8)
    gen_out = str(tmp_path / "gen")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "generate.py"), "--batch_size", "5", "--gen_qtd", "10", "--dataset", "h36m",
           "--channels", "2", "--v_size", "16", "--t_size", "32", "--n_classes", "10",
           "--model", os.path.join(out_e, "models", "generator_best.pth"), "--out", gen_out, "--seed", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = sorted(os.listdir(os.path.join(gen_out, "actions")))
    assert len(files) == 3 and [f.split("_gen_")[1] for f in files] == ["data.npy", "label.pkl", "z.npy"], files
    data = np.load(os.path.join(gen_out, "actions", files[0]))
    assert data.shape == (100, 2, 32, 16) and np.isfinite(data).all()
