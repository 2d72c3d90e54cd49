"""Precision / recall / density / coverage inside the Evaluator on the MI355X: kg_prdc_sets against kg_prdc set
by set, kg_prdc_radii, the given radii, strided input, determinism, capture, kg_eval_record2 against its definition
(tests/eval_prdc_def.py) - on poisoned, red-zoned buffers -, then the Evaluator's new columns against their composition (a
twin Sampler + metrics.prdc), selection by a maximised score, the launch count, resume, the training loop and the command.

Every comparison is bit for bit; no tolerance appears anywhere."""
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
from kinetic_gan_amd.evaluate import Evaluator
from kinetic_gan_amd.feeder import Feeder
from kinetic_gan_amd.generator import Generator
from kinetic_gan_amd.sample import Sampler
from kinetic_gan_amd.train import TrainLoop
from kinetic_gan_amd.wgan_gp import FlatParams

import eval_def
import eval_prdc_def
import prdc_def
import train_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers for the kernel tests below)
from util import build_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SET_KEYS = ("counts", "values", "mean", "radii_fake", "fake_hits", "real_flags")


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


# ---- 1. kg_prdc_sets against kg_prdc, set by set --------------------------------------------------------------------------

def make_sets(nsets, classes, n, m, D, integer=False):
    """R (K, n, D) and nsets fake sets (K, m, D) on the GPU: the generator of tests/prdc_def.py asked for nsets * m fakes per
    class, dealt out to the sets in turn - every set is drawn around the same real set and has its collapsed quarter"""
    R, F = prdc_def.make_data(0, classes, n, nsets * m, D, integer=integer)
    return R.cuda(), [F[:, g::nsets].contiguous().cuda() for g in range(nsets)]


def view(X):
    return nv.PrdcView(X, X.stride(0), X.stride(1), 0)


def run_prdc(R, F, k):
    K, n, D = R.shape
    return nv.prdc(view(R), view(F), n, F.shape[1], 1, D, K, k, want_mean=True, per_point=True)


def run_sets(R, Fs, k, radii, ws=None):
    K, n, D = R.shape
    m = Fs[0].shape[1]
    if ws is None:
        ws = guard.empty(nv.prdc_sets_workspace_bytes(len(Fs), n, m, 1, D, K, k) // 4, dtype=torch.int32, device=DEV)
    return nv.prdc_sets(view(R), Fs, Fs[0].stride(0), Fs[0].stride(1), 0, radii, n, m, 1, D, K, k, want_mean=True, per_point=True,
                        ws=ws)


def sets_tile_edges(nsets, classes, n, m):
    """(fake radii, cross) tile edges by the rule of prdc_sets_plan in csrc/kg_prdc.hip: a launch takes the 64-tile once that
    alone makes 512 workgroups - one per row tile of every fake (set, class), one per tile of every (set, class)"""
    c64 = lambda v: -(-v // 64)      # noqa: E731
    g = nsets * classes
    return (64 if g * c64(m) >= 512 else 32), (64 if g * c64(n) * c64(m) >= 512 else 32)


def assert_sets_equal_single_calls(out, singles):
    for g, one in enumerate(singles):
        for key in SET_KEYS:
            assert same_bits(out[key][g], one[key]), (g, key)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("nsets,classes,n,m,D,k,edges", [
    (1, 1, 40, 40, 6, 3, (32, 32)), (2, 3, 37, 53, 75, 5, (32, 32)), (3, 1, 130, 70, 48, 4, (32, 32)),
    (4, 2, 20, 20, 3, 19, (32, 32)), (4, 8, 260, 260, 6, 5, (32, 64)), (4, 26, 260, 260, 6, 5, (64, 64))])
def test_sets_equal_kg_prdc_set_by_set(nsets, classes, n, m, D, k, edges):
    """ragged tiles, several classes, a partial 32-dimension chunk, several row tiles, k = n - 1; the last two shapes take the
    cross launch and then also the fake-radii launch on the 64-tile kernels.  Float data: the equality is one of bits"""
    assert sets_tile_edges(nsets, classes, n, m) == edges
    R, Fs = make_sets(nsets, classes, n, m, D)
    singles = [run_prdc(R, F, k) for F in Fs]
    radii = nv.prdc_radii(view(R), n, 1, D, classes, k)
    assert radii.shape == (classes, n) and same_bits(radii, singles[0]["radii_real"])
    out = run_sets(R, Fs, k, radii)
    assert out["counts"].shape == (nsets, classes, 4) and out["mean"].shape == (nsets, 4)
    assert out["fake_hits"].shape == (nsets, classes, m) and out["real_flags"].shape == (nsets, classes, n)
    assert_sets_equal_single_calls(out, singles)
    if nsets > 1:
        assert not same_bits(out["counts"][0], out["counts"][1])          # (the sets do score differently)


# ---- 2. the given radii are read, not recomputed -------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_given_radii_are_read():
    """integer coordinates, 256 D < 2^24: everything is exact.  Real 1 duplicates real 0 and fake 0 of set 0 sits on them;
    radii_real = HALF the true radii (exact in fp32): counts, flags and hits are those of the definition fed with the halved
    radii - and not those of the true ones"""
    R, Fs = make_sets(2, 2, 40, 40, 6, integer=True)
    R, Fs = R.clone(), [F.clone() for F in Fs]
    R[0, 1] = R[0, 0]
    Fs[0][0, 0] = R[0, 0]
    true = nv.prdc_radii(view(R), 40, 1, 6, 2, 3)
    assert torch.equal(true.double().cpu(), torch.stack([prdc_def.radii(R[c].cpu(), 3) for c in range(2)]))
    half = guard.empty(true.shape, dtype=torch.float32, device=DEV).copy_(true * 0.5)
    assert torch.equal(half.double() * 2, true.double())
    out, full = run_sets(R, Fs, 3, half), run_sets(R, Fs, 3, true)
    for g, F in enumerate(Fs):
        ref = eval_prdc_def.given_radii(R.cpu(), F.cpu(), half.cpu(), 3)
        assert torch.equal(out["counts"][g].long().cpu(), ref["counts"]), g
        assert torch.equal(out["fake_hits"][g].long().cpu(), ref["fake_hits"]), g
        assert torch.equal(out["real_flags"][g].cpu(), ref["real_flags"]), g
        assert torch.equal(out["radii_fake"][g].double().cpu(), ref["radii_fake"]), g
        want = eval_prdc_def.given_radii(R.cpu(), F.cpu(), true.cpu(), 3)
        assert torch.equal(full["counts"][g].long().cpu(), want["counts"]) and not torch.equal(ref["counts"], want["counts"]), g
        assert torch.equal(ref["counts"][:, 1], want["counts"][:, 1])         # recall rests on the fake radii alone
    assert out["fake_hits"][0, 0, 0] >= 2                                     # 0 <= 0 / 2: the pair on the duplicate counts twice


# ---- 3. strided input ----------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_strided_fakes_in_a_plane_buffer():
    """the fakes as a Sampler round leaves them: a channel-major plane, row j*K + c = sample j of class c, cropped in T"""
    K, P, C, T, V, t, k = 3, 12, 2, 6, 5, 4, 4
    gen = torch.Generator().manual_seed(3)
    planes = []
    for g in range(2):
        pl = nv.new_plane(P * K, C, T, V, DEV)
        pl.copy_(torch.randn((P * K, C, T, V), generator=gen).to(DEV))
        assert pl.stride(1) == P * K * T * V and pl.stride(0) == T * V
        planes.append(pl)
    R = torch.randn((K, P, C * t * V), generator=gen).to(DEV)
    radii = nv.prdc_radii(view(R), P, 1, C * t * V, K, k)
    ws = guard.empty(nv.prdc_sets_workspace_bytes(2, P, P, C, t * V, K, k) // 4, dtype=torch.int32, device=DEV)
    rv = nv.PrdcView(R, R.stride(0), R.stride(1), t * V)
    sn, sc = planes[0].stride(0), planes[0].stride(1)
    out = nv.prdc_sets(rv, planes, sn, K * sn, sc, radii, P, P, C, t * V, K, k, want_mean=True, per_point=True, ws=ws)
    copies = [pl[:, :, :t].reshape(P, K, C * t * V).transpose(0, 1).contiguous() for pl in planes]        # class-major
    want = run_sets(R, copies, k, radii)
    for key in SET_KEYS:
        assert same_bits(out[key], want[key]), key
    assert_sets_equal_single_calls(out, [run_prdc(R, F, k) for F in copies])
    short = guard.empty(planes[1].numel() // 2, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="fake set 1 reach outside"):
        nv.prdc_sets(rv, [planes[0], short], sn, K * sn, sc, radii, P, P, C, t * V, K, k, ws=ws)


# ---- 4. determinism and the workspace -------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_deterministic_on_a_poisoned_workspace_and_every_word_written():
    R, Fs = make_sets(3, 3, 100, 90, 75)
    radii = nv.prdc_radii(view(R), 100, 1, 75, 3, 5)
    guard.assert_no_poison(radii, "radii")
    words = nv.prdc_sets_workspace_bytes(3, 100, 90, 1, 75, 3, 5) // 4
    assert words == 3 * 3 * (2 * 90 + 100)
    ws = guard.full((words,), guard.PATTERN_A, dtype=torch.int32, device=DEV)
    a = run_sets(R, Fs, 5, radii, ws=ws)
    torch.cuda.synchronize()
    assert guard.poison_count(ws) == 0                    # radii, hit words and flag words: all of it is written
    b = run_sets(R, Fs, 5, radii, ws=ws)                  # on what the first call left there (every row hit many times)
    assert a["counts"][:, :, 2].min() > 0
    for key in SET_KEYS:
        assert same_bits(a[key], b[key]), key
        guard.assert_no_poison(a[key], key)
    other = run_sets(R, [Fs[2], Fs[0]], 5, radii, ws=ws)    # fewer sets on the same workspace, another order
    assert_sets_equal_single_calls(other, [run_prdc(R, Fs[2], 5), run_prdc(R, Fs[0], 5)])


# ---- 5. capture ----------------------------------------------------------------------------------------------------------

def test_graph_capture_follows_fakes_and_radii():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    R, Fs = make_sets(2, 3, 40, 36, 90)
    _, Fs2 = make_sets(4, 3, 40, 36, 90)
    radii = nv.prdc_radii(view(R), 40, 1, 90, 3, 5)
    ws = torch.empty(nv.prdc_sets_workspace_bytes(2, 40, 36, 1, 90, 3, 5) // 4, dtype=torch.int32, device=DEV)
    before = {k: v.clone() for k, v in run_sets(R, Fs, 5, radii, ws=ws).items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run_sets(R, Fs, 5, radii, ws=ws)                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run_sets(R, Fs, 5, radii, ws=ws)
    g.replay()
    torch.cuda.synchronize()
    for key in SET_KEYS:
        assert same_bits(cap[key], before[key]), key
    for F, F2 in zip(Fs, Fs2[2:]):                        # new fake contents
        F.copy_(F2)
    g.replay()
    torch.cuda.synchronize()
    eager = run_sets(R, Fs, 5, radii.clone())
    for key in SET_KEYS:
        assert same_bits(cap[key], eager[key]), key
    assert not same_bits(eager["counts"], before["counts"])
    radii.mul_(0.25)                                      # new contents of radii_real
    g.replay()
    torch.cuda.synchronize()
    eager2 = run_sets(R, Fs, 5, radii.clone())
    for key in SET_KEYS:
        assert same_bits(cap[key], eager2[key]), key
    assert not same_bits(eager2["counts"], eager["counts"]) and same_bits(eager2["radii_fake"], eager["radii_fake"])


# ---- 6. kg_eval_record2 --------------------------------------------------------------------------------------------------

SEQ = [3, 2, 2, float("nan"), 5, 1, float("inf"), 1, 0.5, float("-inf"), 7, 7, float("inf")]


def guarded_from(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return guard.empty(t.shape, dtype=t.dtype, device=DEV).copy_(t)


def record_buffers(ref):
    return dict(count=guarded_from(np.zeros(1, np.int64)), ring_val=guarded_from(ref.ring_val), ring_iter=guarded_from(ref.ring_iter),
                best_val=guarded_from(np.array([ref.best_val], np.float32)), best_iter=guarded_from(np.array([-1], np.int64)),
                flag=guard.empty(1, dtype=torch.int32, device=DEV))          # (poison: every call must write it)


def seq_row(nscores, select, k, s):
    return [np.float32(s) if i == select else np.float32(100.0 - 7 * k + i if (k + i) % 3 else np.nan) for i in range(nscores)]


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("it0", [None, 2 ** 24 + 1], ids=["iter-null", "iter-above-2^24"])
@pytest.mark.parametrize("maximise", [False, True], ids=["minimise", "maximise"])
@pytest.mark.parametrize("nscores,select", [(1, 0), (12, 7), (32, 31)])
def test_record2_against_definition(nscores, select, maximise, it0):
    """NaN, +-inf and repeated values in the deciding column (other columns: values that would decide differently); ring of 4
    (it wraps); every ring row, flag, best_val, best_iter and count after every call, bit for bit"""
    ref = eval_prdc_def.Record2(nscores, select, 4, maximise)
    scores = [guard.empty(1, dtype=torch.float32, device=DEV) for _ in range(nscores)]
    it = guard.empty(1, dtype=torch.int64, device=DEV) if it0 is not None else None
    b = record_buffers(ref)
    for k, s in enumerate(SEQ):
        row = seq_row(nscores, select, k, s)
        for t, v in zip(scores, row):
            t.fill_(float(v))
        itk = None if it0 is None else it0 + 3 * k
        if it is not None:
            it.fill_(itk)
        nv.eval_record2(scores, select, it, b["count"], b["ring_val"], b["ring_iter"], b["best_val"], b["best_iter"], b["flag"],
                        maximise=maximise)
        improved = ref.append(row, itk)
        torch.cuda.synchronize()
        what = (nscores, select, maximise, it0, k)
        assert same_bits(b["ring_val"], ref.ring_val), what
        assert np.array_equal(b["ring_iter"].cpu().numpy(), ref.ring_iter), what
        assert int(b["flag"].item()) == int(improved) == int(ref.flag), what
        assert same_bits(b["best_val"], np.array([ref.best_val], np.float32)), what
        assert int(b["best_iter"].item()) == int(ref.best_iter) and int(b["count"].item()) == ref.count == k + 1, what
    want = (np.float32(np.inf), 18) if maximise else (np.float32(-np.inf), 27)
    assert ref.best_val == want[0] and int(b["best_iter"].item()) == (-1 if it0 is None else it0 + want[1])


@pytest.mark.usefixtures("guarded")
def test_record2_minimising_leaves_the_bits_of_kg_eval_record():
    refs = [eval_prdc_def.Record2(4, 2, 4, False), eval_def.Record(4, 2, 4)]
    bufs = [record_buffers(r) for r in refs]
    scores = [guard.empty(1, dtype=torch.float32, device=DEV) for _ in range(4)]
    it = guard.empty(1, dtype=torch.int64, device=DEV)
    for k, s in enumerate(SEQ):
        for t, v in zip(scores, seq_row(4, 2, k, s)):
            t.fill_(float(v))
        it.fill_(2 ** 24 + k)
        b = bufs[0]
        nv.eval_record2(scores, 2, it, b["count"], b["ring_val"], b["ring_iter"], b["best_val"], b["best_iter"], b["flag"])
        b = bufs[1]
        nv.eval_record(scores, 2, it, b["count"], b["ring_val"], b["ring_iter"], b["best_val"], b["best_iter"], b["flag"])
    torch.cuda.synchronize()
    for key in bufs[0]:
        assert same_bits(bufs[0][key], bufs[1][key]), key


def test_record2_bad_arguments_raise():
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)      # noqa: E731
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)        # noqa: E731
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def rec(nscores=1, select=0, ring_len=4, **kw):
        a = dict(scores=[f32(1) for _ in range(nscores)], select=select, iteration=i64(1), count=i64(1),
                 ring_val=f32(ring_len, nscores), ring_iter=i64(ring_len, 2), best_val=f32(1), best_iter=i64(1), flag=flag, maximise=True)
        a.update(kw)
        nv.eval_record2(**a)
    rec()
    rec(nscores=32, select=31)
    for kw, word in ((dict(nscores=2, select=2), "select"), (dict(nscores=12, select=12), "select"), (dict(nscores=0), "nscores"),
                     (dict(nscores=33), "nscores"), (dict(ring_len=0), "ring_len")):
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


# ---- 7. the Evaluator's columns ------------------------------------------------------------------------------------------

CFG, SEED_EV, PER, KNN = "h36m", 5, 8, 3
OLD = ["a/avg", "a/joint", "b/avg", "b/joint"]
NEW = ["%s/%s" % (g, q) for g in ("a", "b") for q in ("precision", "recall", "density", "coverage")]


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
    for k, s in ev.samplers.items():
        out["step." + k] = s.step_dev
    for k, s in ev.prdc_samplers.items():
        out["prdc_step." + k] = s.step_dev
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def assert_same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert same_bits(a[k], b[k]), "%s: %s differs" % (what, k)


def make_ev(gens, feeder, it=None, **kw):
    kw.setdefault("select", "a/avg")
    return Evaluator(gens, feeder, pairs=2, seed=SEED_EV, iteration=it, ring_len=8, **kw)


@pytest.fixture(scope="module")
def composed(tmp_path_factory):
    """two generators with the same weights, pairs = 2, 8 samples per class for PRDC with k = 3: three replayed evaluations,
    next to an Evaluator without PRDC on the same seed"""
    feeder = eval_feeder(tmp_path_factory.mktemp("ev"))
    c, Ga = flat_generator()
    _, Gb = flat_generator()
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": Ga, "b": Gb}, feeder, it, prdc_per_class=PER, prdc_k=KNN)
    plain = make_ev({"a": Ga, "b": Gb}, feeder, it)
    assert ev.use_graph and ev.names == OLD + NEW and plain.names == OLD
    states = []
    for k in range(3):
        ev.evaluate()
        plain.evaluate()
        it += 2
        states.append(ev_state(ev))
    return dict(feeder=feeder, c=c, Ga=Ga, Gb=Gb, ev=ev, plain=plain, states=states, rec=ev.records(), rec_plain=plain.records(),
                plain_state=ev_state(plain))


def twin_round(G, counter, qtd):
    s = Sampler(G, qtd=qtd, seed=SEED_EV, use_graph=False)
    s.load_state_dict({"seed": SEED_EV, "step": counter})
    out, _, _ = s.next()
    torch.cuda.synchronize()
    return out, s


def test_columns_equal_the_composition(composed):
    ev, rec, plain = composed["ev"], composed["rec"], composed["rec_plain"]
    assert rec["names"] == OLD + NEW and rec["scores"].shape == (3, 12) and plain["scores"].shape == (3, 4)
    # the MMD columns do not move: bit for bit those of the Evaluator without PRDC, and so does everything they decide
    assert same_bits(rec["scores"][:, :4], plain["scores"])
    assert same_bits(rec["improved"], plain["improved"]) and same_bits(rec["iteration"], plain["iteration"])
    assert ev.best() == composed["plain"].best()
    for key in ("best_val", "best_iter", "snap_flat", "step.a", "step.b"):
        assert same_bits(composed["states"][-1][key], composed["plain_state"][key]), key
    # the real side: the protocol's selection, class by class, and its radii
    data, labels, _ = metrics.select_reference_samples(composed["feeder"], np.arange(10), 32, per_class=PER)
    assert same_bits(ev.prdc_real, data) and ev.prdc_radii.shape == (10, PER)
    real = torch.as_tensor(data).to(DEV)
    # the PRDC columns: metrics.prdc of a twin Sampler round of 8 per class against that selection
    for k in range(3):
        out, s = twin_round(composed["Ga"], k, PER)
        assert out.shape == (10 * PER, 2, 32, 16) and s.labels_np.tolist() == list(range(10)) * PER
        want = metrics.prdc(out, real, s.labels_np, labels, k=KNN, per_point=True)
        print("evaluation", k, "precision / recall / density / coverage", want["mean"].tolist())
        assert same_bits(rec["scores"][k, 4:8], want["mean"]), k
        if k == 0:
            assert same_bits(ev.prdc_radii, want["radii_real"])
    assert np.isfinite(rec["scores"]).all() and (rec["scores"][:, 4:] >= 0).all()
    # equal weights behind another Sampler: equal columns
    assert same_bits(rec["scores"][:, 4:8], rec["scores"][:, 8:12])
    state = ev.state_dict()
    assert state["prdc"] == {"per_class": PER, "k": KNN} and "prdc" not in composed["plain"].state_dict()
    assert state["names"] == OLD + NEW and "prdc_radii" not in state


def test_replays_equal_eager_evaluations(composed):
    it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": composed["Ga"], "b": composed["Gb"]}, composed["feeder"], it, prdc_per_class=PER, prdc_k=KNN, use_graph=False)
    for k in range(3):
        ev.evaluate()
        it += 2
        assert_same(composed["states"][k], ev_state(ev), "graph vs eager, evaluation %d" % k)
    a, b = ev.records(), composed["rec"]
    assert all(same_bits(a[k], b[k]) for k in ("iteration", "scores", "improved"))


def test_real_side_from_arrays(composed):
    """``real`` / ``real_labels``: the first 8 samples of every class in index order, class by class"""
    feeder = composed["feeder"]
    idx = np.arange(1, 200)
    data = np.stack([np.asarray(feeder[int(i)][0], dtype=np.float32)[:, :32] for i in idx])
    lab = np.asarray(feeder.label)[idx]
    ev = make_ev({"a": composed["Ga"]}, torch.as_tensor(data), real_labels=lab, prdc_per_class=PER, prdc_k=KNN, use_graph=False)
    rows = np.concatenate([np.flatnonzero(lab == c)[:PER] for c in range(10)])
    assert same_bits(ev.prdc_real, data[rows])
    with pytest.raises(ValueError, match="class_rows"):
        make_ev({"a": composed["Ga"]}, torch.as_tensor(data[:60]), real_labels=lab[:60], prdc_per_class=PER, prdc_k=KNN)


# ---- 8. selection by a maximised score -----------------------------------------------------------------------------------

SCALES = [1.0, 0.9, 1.1, 1.0, 1.25, 0.8]


def test_selection_by_coverage(composed):
    """the generator's weights are scaled between the evaluations so that the score moves; the improved flags and best() are
    the definition's, fed with the device's scores, and the snapshot holds the weights of the best evaluation"""
    _, G = flat_generator()
    flat = G._flat_keep.flat
    orig = flat.clone()
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    ev = make_ev({"a": G}, composed["feeder"], it, select="a/coverage", prdc_per_class=PER, prdc_k=KNN)
    assert ev.maximise and ev.best() == {"value": float("-inf"), "iteration": -1}
    assert ev.names == ["a/avg", "a/joint", "a/precision", "a/recall", "a/density", "a/coverage"]
    weights = []
    for k, s in enumerate(SCALES):
        with torch.no_grad():
            flat.copy_(orig * s)
        weights.append(flat.detach().clone())
        it.fill_(10 * (k + 1))
        ev.evaluate()
    rec, best = ev.records(), ev.best()
    cov = rec["scores"][:, 5]
    print("a/coverage per evaluation:", cov.tolist(), "improved:", rec["improved"].tolist(), "best:", best)
    assert len(set(cov.tolist())) > 1, "the score did not move: the test decides nothing"
    ref = eval_prdc_def.Record2(6, 5, 8, maximise=True)
    for k in range(len(SCALES)):
        ref.append(rec["scores"][k], rec["iteration"][k])
    assert rec["improved"].tolist() == ref.ring_iter[:len(SCALES), 1].astype(bool).tolist() and rec["improved"][0]
    assert best == {"value": float(ref.best_val), "iteration": int(ref.best_iter)}
    assert best["value"] == float(cov.max()) and best["iteration"] == 10 * (int(np.argmax(cov)) + 1)     # the FIRST maximum
    k_best = best["iteration"] // 10 - 1
    assert same_bits(ev.snap_flat, weights[k_best])
    for k, w in enumerate(weights):
        if not same_bits(w, weights[k_best]):
            assert not same_bits(ev.snap_flat, w), k
    B = ev.best_generator()
    c = composed["c"]
    F = Generator(c["latent"], c["channels"], c["n_classes"], c["t_size"], c["mlp"], dataset="h36m")
    assert list(B.state_dict().keys()) == list(F.state_dict().keys())
    # minimising the same column picks another evaluation: the sense is what decides
    ref_min = eval_prdc_def.Record2(6, 5, 8, maximise=False)
    for k in range(len(SCALES)):
        ref_min.append(rec["scores"][k], rec["iteration"][k])
    assert float(ref_min.best_val) == float(cov.min()) != best["value"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev.reset()
    assert ev.best() == {"value": float("-inf"), "iteration": -1} and all(int(s.step_dev.item()) == 0 for s in ev.prdc_samplers.values())


# ---- 9. launch count -----------------------------------------------------------------------------------------------------

def count_calls(monkeypatch, ev):
    calls = []
    plain = nv._count
    monkeypatch.setattr(nv, "_count", lambda kind, flops: (calls.append(kind), plain(kind, flops))[1])
    ev.evaluate()
    torch.cuda.synchronize()
    monkeypatch.setattr(nv, "_count", plain)
    return calls


def test_one_kg_prdc_sets_call_whatever_the_number_of_generators(composed, monkeypatch):
    """every launch of the bindings passes through _native._count once per call; kg_prdc_sets is three launches per call
    (csrc/kg_prdc.hip): an evaluation adds the second Sampler rounds and exactly ONE kg_prdc_sets call - three kernel
    launches - for one generator and for two, no kg_prdc and no kg_prdc_radii (the real radii are computed at construction)"""
    Ga, Gb, feeder = composed["Ga"], composed["Gb"], composed["feeder"]
    per_round = None
    for gens in ({"a": Ga}, {"a": Ga, "b": Gb}):
        on = count_calls(monkeypatch, make_ev(gens, feeder, prdc_per_class=PER, prdc_k=KNN, use_graph=False))
        off = count_calls(monkeypatch, make_ev(gens, feeder, use_graph=False))
        prdc = [k for k in on if k.startswith("kg_prdc")]
        assert prdc == ["kg_prdc_sets"], prdc
        rest = [k for k in on if not k.startswith("kg_prdc")]
        extra = len(rest) - len(off)
        assert extra % len(gens) == 0 and extra > 0         # the PRDC Sampler rounds: the same launches per generator
        per_round = extra // len(gens) if per_round is None else per_round
        assert extra // len(gens) == per_round


# ---- 10. resume ----------------------------------------------------------------------------------------------------------

B_LOOP, SEED_LOOP, N_CRITIC, DECAY = 4, 3, 2, 0.9
LOOP_NAMES = ["live/avg", "live/joint", "ema/avg", "ema/joint"] + ["%s/%s" % (g, q) for g in ("live", "ema") for q in metrics.PRDC_NAMES]


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


PRDC_KW = dict(eval_interval=2, eval_prdc=PER, eval_prdc_k=KNN, eval_select="ema/coverage")


@pytest.fixture(scope="module")
def six_steps(tmp_path_factory):
    loop = make_loop(tmp_path_factory.mktemp("six"), **PRDC_KW)
    ev = loop.evaluator
    assert ev is not None and ev.use_graph and ev.select == "ema/coverage" and ev.maximise and ev.names == LOOP_NAMES
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
    assert rec["iteration"].tolist() == [2, 4, 6] and rec["scores"].shape == (3, 12) and np.isfinite(rec["scores"]).all()
    loop = make_loop(tmp_path / "a", **PRDC_KW)
    for _ in range(3):
        loop.step()
    sd = loop.state_dict()
    assert sd["eval"]["count"] == 1 and sd["eval"]["prdc"] == {"per_class": PER, "k": KNN} and sd["eval"]["step"] == 1
    path = str(tmp_path / "loop_state.pth")
    torch.save(sd, path)
    del loop
    loop2 = make_loop(tmp_path / "b", **PRDC_KW)
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
    assert all(s.step_count == 3 for s in loop2.evaluator._all_samplers())
    # a differing prdc entry, and a state without one, raise before anything is loaded
    state = torch.load(path, weights_only=False)
    for kw, word in ((dict(eval_prdc_k=2), "prdc"), (dict(eval_prdc=9), "prdc"), (dict(eval_prdc=0, eval_select="ema/avg"), "prdc")):
        args = dict(PRDC_KW, use_graph=False)
        args.update(kw)
        other = make_loop(tmp_path / "c", **args)
        flat = other.trainer.fG.flat.clone()
        with pytest.raises(ValueError, match=word):
            other.load_state_dict(state)
        assert same_bits(flat, other.trainer.fG.flat)
    plain = make_loop(tmp_path / "d", eval_interval=2, use_graph=False)
    old = plain.state_dict()
    assert "prdc" not in old["eval"]
    other = make_loop(tmp_path / "e", use_graph=False, **PRDC_KW)
    with pytest.raises(ValueError, match="prdc"):
        other.load_state_dict(old)


# ---- 11. the training loop and the command -------------------------------------------------------------------------------

def test_evaluation_with_prdc_only_observes(six_steps, tmp_path):
    loop = make_loop(tmp_path)
    assert loop.evaluator is None
    for k in range(6):
        loop.step()
        assert_same(six_steps["states"][k], loop_state(loop), "with vs without evaluation, iteration %d" % k)
    d, g = loop.losses()
    assert same_bits(d, six_steps["d"]) and same_bits(g, six_steps["g"])
    # the record against the definition: the averaged generator's coverage decides, larger is better
    rec, ev = six_steps["rec"], six_steps["loop"].evaluator
    ref = eval_prdc_def.Record2(12, 11, ev.ring_len, maximise=True)
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
           "--eval_prdc", str(PER), "--eval_prdc_k", str(KNN), "--eval_select", "live/coverage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "[best live/coverage: " in r.stdout
    rows = list(csv.reader(open(os.path.join(out, "metrics.csv"))))
    assert rows[0] == ["iteration"] + LOOP_NAMES + ["improved"] and len(rows) == 6
    state = torch.load(os.path.join(out, "loop_state.pth"), weights_only=False)["eval"]
    assert state["prdc"] == {"per_class": PER, "k": KNN} and state["select"] == "live/coverage" and state["names"] == LOOP_NAMES
    rec = state["records"]
    assert [int(r_[0]) for r_ in rows[1:]] == rec["iteration"].tolist() == [5, 10, 15, 20, 25]
    back = np.array([[float(v) for v in r_[1:13]] for r_ in rows[1:]], dtype=np.float32)
    assert same_bits(back, rec["scores"])
    assert [int(r_[13]) for r_ in rows[1:]] == rec["improved"].astype(int).tolist()
    ref = eval_prdc_def.Record2(12, 7, 1024, maximise=True)
    for k in range(5):
        ref.append(rec["scores"][k], rec["iteration"][k])
    assert int(state["best_iter"].item()) == int(ref.best_iter) and rec["improved"].tolist() == ref.ring_iter[:5, 1].astype(bool).tolist()
    best = torch.load(os.path.join(out, "models", "generator_best.pth"))
    F = Generator(512, 2, 10, 32, 4, dataset="h36m")
    assert list(best.keys()) == list(F.state_dict().keys())
    F.load_state_dict(best, strict=True)
