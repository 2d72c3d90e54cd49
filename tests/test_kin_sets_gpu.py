"""kg_kin_desc_sets and kg_eval_record3 on the MI355X.  Every equality is on bits: a set's descriptors and
degenerate counts against the kg_kin_desc call of that set (whose values tests/test_kin_gpu.py pins against the float64
definition), the record against the definition of tests/eval_def.py.  Outputs and workspaces start poisoned and red-zoned
(tests/guard.py); the guard also finds the ticket counter back at zero."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv

import eval_def
import eval_prdc_def
import kin_def
from tests import guard
from tests.guard import guarded  # noqa: F401  (fixture: poisoned, red-zoned buffers)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def view(x):
    """(K, n, C, T, V) tensor (any strides, joints contiguous) -> FrechetView"""
    return nv.FrechetView(x, x.stride(0), x.stride(1), x.stride(3), x.stride(2))


@functools.lru_cache(maxsize=None)
def sets_data(name, nsets, K, n, T):
    """nsets distinct (K, n, C, T, V) host arrays (another seed, scale and shift per set), the bones, the mirror pairs"""
    C, V, bones, mirror = kin_def.skeleton(name)
    xs = tuple(kin_def.make_data(30 + g, K, n, C, T, V, scale=1.0 / (1 + g), shift=0.1 * g) for g in range(nsets))
    return xs, tuple(bones), tuple(mirror)


def one_by_one(xs, bones, mirror, still_eps=1e-3):
    """[(desc, degenerate)] of one kg_kin_desc call per set"""
    out = []
    for x in xs:
        K, n, C, T, V = x.shape
        out.append(nv.kin_desc(view(x), n, T, C, V, K, bones, mirror, still_eps))
    return out


def run_sets(xs, bones, mirror, still_eps=1e-3):
    K, n, C, T, V = xs[0].shape
    desc, degenerate = nv.kin_desc_sets([view(x) for x in xs], 0, 0, 0, 0, n, T, C, V, K, bones, mirror, still_eps)
    guard.assert_no_poison(desc, "desc")
    guard.assert_no_poison(degenerate, "degenerate")
    assert desc.shape == (len(xs), K, n, 6) and desc.dtype == torch.float32
    assert degenerate.shape == (len(xs), K) and degenerate.dtype == torch.int32
    return desc, degenerate


def counters_zero():
    torch.cuda.synchronize()
    return all(int(b.abs().sum()) == 0 for b in nv._sync_bufs.values())


# ---- per-set equality -------------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("T", [4, 5, 32])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", ["ntu", "h36m"])
@pytest.mark.parametrize("nsets", [1, 2, 4])
def test_every_set_has_the_bits_of_its_own_call(nsets, name, K, n, T):
    host, bones, mirror = sets_data(name, nsets, K, n, T)
    xs = [torch.from_numpy(x).to(DEV) for x in host]
    assert all(not np.array_equal(host[0], h) for h in host[1:])
    desc, degenerate = run_sets(xs, bones, mirror)
    assert counters_zero()
    for g, (d1, g1) in enumerate(one_by_one(xs, bones, mirror)):
        assert same_bits(desc[g], d1), (nsets, name, K, n, T, g)
        assert torch.equal(degenerate[g], g1), (nsets, name, K, n, T, g)
        assert torch.isfinite(d1).all() and (d1[..., :5] > 0).all()          # (an ordinary sample: nothing vanishes)
    for g in range(1, nsets):
        assert not same_bits(desc[0], desc[g])                               # the sets do differ


@pytest.mark.usefixtures("guarded")
def test_the_samplers_layout_with_a_crop_in_time():
    """rows j*K + c of a (P*K, C, 40, V) parent read as T = 32: class stride = one sample, sample stride = K samples"""
    K, P, C, V, Tp, T = 3, 4, 2, 16, 40, 32
    _, _, bones, mirror = kin_def.skeleton("h36m")
    parents = [torch.from_numpy(kin_def.make_data(50 + g, P, K, C, Tp, V).reshape(P * K, C, Tp, V)).to(DEV) for g in range(3)]
    sn = C * Tp * V
    desc, degenerate = nv.kin_desc_sets(parents, sn, K * sn, V, Tp * V, P, T, C, V, K, bones, mirror)
    guard.assert_no_poison(desc, "desc")
    assert counters_zero()
    for g, x in enumerate(parents):
        rows = x.reshape(P, K, C, Tp, V).permute(1, 0, 2, 3, 4)[:, :, :, :T]        # (K, P, C, T, V), a view of the parent
        d1, g1 = nv.kin_desc(view(rows), P, T, C, V, K, bones, mirror)
        d2, _ = nv.kin_desc(view(rows.contiguous()), P, T, C, V, K, bones, mirror)
        assert same_bits(desc[g], d1) and same_bits(d1, d2) and torch.equal(degenerate[g], g1)
    # frame 32.. of the parent is not read: another tail, the same bits
    for x in parents:
        x[:, :, T:] = 7.0
    again, _ = nv.kin_desc_sets(parents, sn, K * sn, V, Tp * V, P, T, C, V, K, bones, mirror)
    assert same_bits(again, desc)
    with pytest.raises(ValueError, match="reach outside"):
        nv.kin_desc_sets(parents, sn, K * sn, V, Tp * V, P + 1, T, C, V, K, bones, mirror)


@pytest.mark.usefixtures("guarded")
def test_degenerate_and_nonfinite_samples_stay_in_their_sets_row():
    host, bones, mirror = sets_data("ntu", 3, 3, 5, 8)
    host = [h.copy() for h in host]
    host[1][0, 2] = 0.0                          # set 1: an all-zero sample in class 0 ...
    host[1][2, 4, 1, 3, 7] = np.nan              # ... and a NaN sample in class 2
    host[0][1, 0] = 0.0                          # set 0: two all-zero samples in class 1
    host[0][1, 3] = 0.0
    xs = [torch.from_numpy(h).to(DEV) for h in host]
    desc, degenerate = run_sets(xs, bones, mirror)
    assert degenerate.cpu().tolist() == [[0, 2, 0], [1, 0, 0], [0, 0, 0]]
    ones = one_by_one(xs, bones, mirror)
    for g, (d1, g1) in enumerate(ones):
        assert same_bits(desc[g], d1) and torch.equal(degenerate[g], g1)
    got = desc.cpu().numpy()
    assert (got[1, 0, 2] == 0).all() and (got[0, 1, 0] == 0).all() and (got[0, 1, 3] == 0).all()
    assert np.isnan(got[1, 2, 4, [0, 2, 3, 4]]).all() and np.isnan(got).sum() == np.isnan(got[1, 2, 4]).sum()
    # no other set's row moves: set 2 is what it is without the planted samples next to it
    clean, _, _ = sets_data("ntu", 3, 3, 5, 8)
    d_clean, g_clean = nv.kin_desc(view(torch.from_numpy(clean[2]).to(DEV)), 5, 8, 3, 25, 3, bones, mirror)
    assert same_bits(desc[2], d_clean) and torch.equal(degenerate[2], g_clean)
    out = nv.kin_scores(desc[2].contiguous(), [desc[0].contiguous(), desc[1].contiguous()])
    assert out["nonfinite"].cpu().tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 1]]
    assert np.isnan(out["scores"].cpu().numpy()[1, [0, 2, 3, 4]]).all() and torch.isfinite(out["scores"][0]).all()


@pytest.mark.usefixtures("guarded")
def test_w1_of_the_real_set_against_itself_is_zero():
    """still_eps = 0.05 (tests/test_kin_gpu.py: a good share of the steps is still), so that the sixth descriptor varies too"""
    host, bones, mirror = sets_data("h36m", 3, 3, 5, 32)
    xs = [torch.from_numpy(h).to(DEV) for h in host]
    real = xs[1]
    real_desc, _ = nv.kin_desc(view(real), 5, 32, 2, 16, 3, bones, mirror, 0.05)
    desc, _ = run_sets(xs, bones, mirror, 0.05)
    out = nv.kin_scores(real_desc, [desc[g] for g in range(3)])
    scores = out["scores"].cpu().numpy()
    print("w1 against set 1:", scores.tolist())
    assert (bits(scores[1]) == 0).all() and (bits(out["w1"][1]) == 0).all()                  # exactly +0.0
    assert np.isfinite(scores[[0, 2]]).all() and (scores[[0, 2]] > 0).all()


# ---- launch properties -----------------------------------------------------------------------------------------------------

@pytest.mark.usefixtures("guarded")
def test_two_calls_give_the_same_bits():
    host, bones, mirror = sets_data("ntu", 4, 3, 5, 32)
    xs = [torch.from_numpy(h).to(DEV) for h in host]
    a, da = run_sets(xs, bones, mirror)
    b, db = run_sets(xs, bones, mirror)
    assert same_bits(a, b) and torch.equal(da, db) and counters_zero()


def test_graph_capture_replays_on_new_inputs():
    """(not under the guard: allocations made while a stream captures pass through it unchanged)"""
    host, bones, mirror = sets_data("h36m", 2, 3, 5, 32)
    new, _, _ = sets_data("h36m", 4, 3, 5, 32)
    xs = [torch.from_numpy(h).to(DEV) for h in host]
    before = nv.kin_desc_sets([view(x) for x in xs], 0, 0, 0, 0, 5, 32, 2, 16, 3, bones, mirror)[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nv.kin_desc_sets([view(x) for x in xs], 0, 0, 0, 0, 5, 32, 2, 16, 3, bones, mirror)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap, cap_deg = nv.kin_desc_sets([view(x) for x in xs], 0, 0, 0, 0, 5, 32, 2, 16, 3, bones, mirror)
    fresh = [new[2].copy(), new[3].copy()]
    fresh[1][2, 1] = 0.0
    for x, h in zip(xs, fresh):
        x.copy_(torch.from_numpy(h))
    g.replay()
    torch.cuda.synchronize()
    eager, eager_deg = nv.kin_desc_sets([view(x) for x in xs], 0, 0, 0, 0, 5, 32, 2, 16, 3, bones, mirror)
    assert same_bits(cap, eager) and torch.equal(cap_deg, eager_deg) and cap_deg.cpu().tolist() == [[0, 0, 0], [0, 0, 1]]
    assert not same_bits(eager, before)


def test_workspace_bytes():
    for name in ("ntu", "h36m"):
        C, V, bones, mirror = kin_def.skeleton(name)
        for nsets, K, n in ((1, 1, 1), (2, 3, 5), (4, 60, 100), (3, 7, 11)):
            assert nv.kin_desc_sets_workspace_bytes(nsets, n, 32, C, V, K, bones, mirror) == 4 * nsets * K * n
        assert nv.kin_desc_sets_lds_bytes(4, 5, 32, C, V, 3, bones, mirror) == nv.kin_desc_lds_bytes(5, 32, C, V, 3, bones, mirror)


@pytest.mark.usefixtures("guarded")
def test_rejections_launch_nothing():
    host, bones, mirror = sets_data("h36m", 2, 3, 5, 8)
    xs = [torch.from_numpy(h).to(DEV) for h in host]
    out = guard.empty((2, 3, 5, 6), dtype=torch.float32, device=DEV)
    ws = guard.empty(2 * 3 * 5, dtype=torch.float32, device=DEV)
    def call(sets=xs, **kw):
        a = dict(n=5, T=8, Cc=2, V=16, classes=3, bones=bones, mirror=mirror, still_eps=1e-3)
        a.update(kw)
        nv.kin_desc_sets([view(x) for x in sets], 0, 0, 0, 0, a["n"], a["T"], a["Cc"], a["V"], a["classes"], a["bones"],
                         a["mirror"], a["still_eps"], out=out if len(sets) == 2 else None, ws=ws)
    cases = [(dict(sets=[]), "nsets=0"), (dict(sets=[xs[0]] * 5), "nsets=5"), (dict(classes=0), "classes=0"), (dict(n=0), "n=0"),
             (dict(Cc=4), "C=4"), (dict(V=33), "V=33"), (dict(T=3), "T=3"), (dict(T=2048), r"C\*T\*V"),
             (dict(bones=[]), "B=0"), (dict(bones=list(bones) + [(0, 16)]), r"bones\[%d\]\[1\]=16" % len(bones)),
             (dict(mirror=list(mirror) + [(0, len(bones))]), r"mirror\[%d\]\[1\]=%d" % (len(mirror), len(bones))),
             (dict(mirror=[(0, 1)] * 17), "M=17"),
             (dict(still_eps=-1.0), "still_eps"), (dict(still_eps=float("inf")), "still_eps"),
             (dict(classes=1 << 12, n=1 << 12), r"classes \* n"), (dict(classes=1 << 12, n=1 << 11), r"nsets \* classes \* n")]
    for kw, word in cases:
        with pytest.raises(RuntimeError, match="kg_kin_desc_sets.*" + word):
            call(**kw)
    with pytest.raises(ValueError, match="ws"):
        nv.kin_desc_sets([view(x) for x in xs], 0, 0, 0, 0, 5, 8, 2, 16, 3, bones, mirror, out=out, ws=ws.double())
    with pytest.raises(ValueError, match="out must be"):
        nv.kin_desc_sets([view(x) for x in xs], 0, 0, 0, 0, 5, 8, 2, 16, 3, bones, mirror, out=out[:1], ws=ws)
    with pytest.raises(RuntimeError, match="ws_bytes=116 < 120"):
        nv.kin_desc_sets([view(x) for x in xs], 0, 0, 0, 0, 5, 8, 2, 16, 3, bones, mirror, out=out, ws=ws[:-1])
    with pytest.raises(ValueError, match="differ in their strides"):
        nv.kin_desc_sets([view(xs[0]), view(xs[1].permute(1, 0, 2, 3, 4).contiguous().permute(1, 0, 2, 3, 4))], 0, 0, 0, 0, 5, 8, 2, 16,
                         3, bones, mirror, out=out, ws=ws)
    with pytest.raises(TypeError, match="fp32"):
        nv.kin_desc_sets([xs[0].double()], 16 * 8 * 2 * 5, 16 * 8 * 2, 16, 16 * 8, 5, 8, 2, 16, 3, bones, mirror)
    # a null x[g] / desc[g]: the library itself, with the binding's struct (nothing is launched: the call returns first)
    a, keep = nv._kin_desc_sets_shape(2, 5, 8, 2, 16, 3, bones, mirror, 1e-3)
    deg = guard.empty((2, 3), dtype=torch.int32, device=DEV)
    sync = nv._sync_buffer(torch.device(DEV))
    a.sc, a.ss, a.sf, a.so = xs[0].stride(0), xs[0].stride(1), xs[0].stride(3), xs[0].stride(2)
    a.degenerate, a.ws, a.ws_bytes, a.counters, a.counters_len = deg.data_ptr(), ws.data_ptr(), 120, sync.data_ptr(), sync.numel()
    lib = nv.load_library()
    for null, word in (("x", b"null pointer x[1]"), ("desc", b"null pointer desc[1]")):
        for g in range(2):
            a.x[g], a.desc[g] = xs[g].data_ptr(), out[g].data_ptr()
        getattr(a, null)[1] = None
        assert lib.kg_kin_desc_sets(ctypes.byref(a), None) < 0 and word in lib.kg_last_error()
    torch.cuda.synchronize()
    n_out, n_ws, n_deg = out.numel(), ws.numel(), deg.numel()
    assert guard.poison_count(out) == n_out and guard.poison_count(ws) == n_ws and guard.poison_count(deg) == n_deg      # untouched
    assert counters_zero()


# ---- kg_eval_record3 ---------------------------------------------------------------------------------------------------------

class Record3(eval_prdc_def.Record2):
    """the record of tests/eval_def.py (through its twin with a sense, tests/eval_prdc_def.py) with room for 64 scores"""

    def __init__(self, nscores, select, ring_len, maximise=False):
        assert 1 <= nscores <= 64
        eval_prdc_def.Record2.__init__(self, min(nscores, 32), min(select, min(nscores, 32) - 1), ring_len, maximise)
        self.nscores, self.select = nscores, select
        self.ring_val = np.full((ring_len, nscores), np.nan, dtype=np.float32)


SEQ = [3, 2, 2, float("nan"), 5]                 # ring_len 3, 5 evaluations: the ring wraps; a repeat and a NaN in the deciding column
IT0 = 2 ** 24 + 3


def guarded_from(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return guard.empty(t.shape, dtype=t.dtype, device=DEV).copy_(t)


def record_buffers(ref):
    return dict(count=guarded_from(np.zeros(1, np.int64)), ring_val=guarded_from(ref.ring_val), ring_iter=guarded_from(ref.ring_iter),
                best_val=guarded_from(np.array([ref.best_val], np.float32)), best_iter=guarded_from(np.array([-1], np.int64)),
                flag=guard.empty(1, dtype=torch.int32, device=DEV))          # (poison: every call must write it)


def seq_row(nscores, select, k, s):
    """the deciding column takes SEQ; the other columns hold values that would decide differently, and some NaNs"""
    return [np.float32(s) if i == select else np.float32(100.0 - 7 * k + i if (k + i) % 3 else np.nan) for i in range(nscores)]


def test_record3_definition_agrees_with_eval_def_on_its_own_ground():
    """(host only) Record3, minimising with 8 scores, is tests/eval_def.py's Record step by step"""
    a, b = Record3(8, 5, 3), eval_def.Record(8, 5, 3)
    for k, s in enumerate(SEQ + [1, 1, float("-inf")]):
        row = seq_row(8, 5, k, s)
        assert a.append(row, IT0 + k) == b.append(row, IT0 + k)
        assert same_bits(a.ring_val, b.ring_val) and np.array_equal(a.ring_iter, b.ring_iter)
        assert same_bits(np.float32(a.best_val), np.float32(b.best_val)) and a.best_iter == b.best_iter and a.count == b.count


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("maximise", [False, True], ids=["minimise", "maximise"])
@pytest.mark.parametrize("nscores,select", [(1, 0), (33, 0), (40, 0), (40, 39), (64, 0), (64, 39), (64, 63)])
def test_record3_against_definition(nscores, select, maximise):
    ref = Record3(nscores, select, 3, maximise)
    scores = [guard.empty(1, dtype=torch.float32, device=DEV) for _ in range(nscores)]
    it = guard.empty(1, dtype=torch.int64, device=DEV)
    b = record_buffers(ref)
    flags = []
    for k, s in enumerate(SEQ):
        row = seq_row(nscores, select, k, s)
        for t, v in zip(scores, row):
            t.fill_(float(v))
        it.fill_(IT0 + 2 * k)
        nv.eval_record3(scores, select, it, b["count"], b["ring_val"], b["ring_iter"], b["best_val"], b["best_iter"], b["flag"],
                        maximise=maximise)
        improved = ref.append(row, IT0 + 2 * k)
        torch.cuda.synchronize()
        what = (nscores, select, maximise, k)
        assert same_bits(b["ring_val"], ref.ring_val), what
        assert np.array_equal(b["ring_iter"].cpu().numpy(), ref.ring_iter), what
        assert int(b["flag"].item()) == int(improved) == int(ref.flag), what
        assert same_bits(b["best_val"], np.array([ref.best_val], np.float32)), what
        assert int(b["best_iter"].item()) == int(ref.best_iter) and int(b["count"].item()) == ref.count == k + 1, what
        flags.append(improved)
    # 3, 2, 2, NaN, 5: the equal score keeps the earlier best, the NaN never wins; above 2^24 the iteration keeps its last bits
    assert flags == ([True, False, False, False, True] if maximise else [True, True, False, False, False])
    assert int(b["best_iter"].item()) == (IT0 + 8 if maximise else IT0 + 2)


@pytest.mark.usefixtures("guarded")
@pytest.mark.parametrize("maximise", [False, True], ids=["minimise", "maximise"])
@pytest.mark.parametrize("nscores", [8, 32])
def test_record3_leaves_the_bits_of_kg_eval_record2(nscores, maximise):
    refs = [Record3(nscores, nscores - 1, 3, maximise), eval_prdc_def.Record2(nscores, nscores - 1, 3, maximise)]
    bufs = [record_buffers(r) for r in refs]
    scores = [guard.empty(1, dtype=torch.float32, device=DEV) for _ in range(nscores)]
    it = guard.empty(1, dtype=torch.int64, device=DEV)
    for k, s in enumerate(SEQ):
        for t, v in zip(scores, seq_row(nscores, nscores - 1, k, s)):
            t.fill_(float(v))
        it.fill_(IT0 + k)
        for fn, b in zip((nv.eval_record3, nv.eval_record2), bufs):
            fn(scores, nscores - 1, it, b["count"], b["ring_val"], b["ring_iter"], b["best_val"], b["best_iter"], b["flag"],
               maximise=maximise)
    torch.cuda.synchronize()
    for key in bufs[0]:
        assert same_bits(bufs[0][key], bufs[1][key]), key
    assert int(bufs[0]["count"].item()) == 5


def test_record3_bad_arguments_raise():
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)      # noqa: E731
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)        # noqa: E731
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def rec(nscores=1, select=0, ring_len=4, **kw):
        a = dict(scores=[f32(1) for _ in range(nscores)], select=select, iteration=i64(1), count=i64(1),
                 ring_val=f32(ring_len, nscores), ring_iter=i64(ring_len, 2), best_val=f32(1), best_iter=i64(1), flag=flag, maximise=True)
        a.update(kw)
        nv.eval_record3(**a)
    rec()
    rec(nscores=64, select=63)
    for kw, word in ((dict(nscores=40, select=40), "select"), (dict(nscores=0), "nscores"), (dict(nscores=65), "nscores=65"),
                     (dict(ring_len=0), "ring_len")):
        with pytest.raises(RuntimeError, match="kg_eval_record3.*" + word):
            rec(**kw)
    with pytest.raises(TypeError):
        rec(scores=[i64(1)])
