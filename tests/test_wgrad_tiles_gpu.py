"""-m gpu: every tile body of csrc/kg_wgrad.hip - five variants, fp32 and bf16-split (KG_WGRAD_SPLIT=1) - and every split
class of kg_wgrad_many against the float64 definition of tests/wgrad_def.py, on poisoned, red-zoned buffers.

Every test asserts, through `_native.last_wgrad_plan` (kg_wgrad_many_plan / kg_wgrad_plan_info), the tile variant and the
split class it is named after: the launches and their expectations are the table `wgrad_def.LAUNCHES`, which
tests/test_wgrad_def_cpu.py plans on the host as well.  Comparisons: bit equality on integer data (wgrad_def: every fp32
partial sum is exact in every order), the derived per-element bracket on seeded normal data with at most 512 columns."""
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from tests import guard
from tests import wgrad_def as wd
from tests.guard import guard_all  # noqa: F401  (autouse: every test of this module runs on poisoned, red-zoned buffers)
from tests.util import ReloadingEnv

pytestmark = pytest.mark.gpu
FORMS = {"fp32": {}, "bf16split": {"KG_WGRAD_SPLIT": "1"}}
LEAD = 7                    # floats in front of every destination inside its parent buffer
SENTINEL = -12345.0


@pytest.fixture
def monkeypatch(monkeypatch):
    """the environment through tests/util.ReloadingEnv: every change is followed by kg_reload_env()"""
    env = ReloadingEnv(monkeypatch)
    yield env
    env.undo()


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def stored(t, layout):
    """the logical (N, C, T, V) tensor on the device, NCHW or channel-major ("plane") storage"""
    if layout == "plane":
        t = t.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    out = t.to(dev())
    assert out.stride() == t.stride()
    return out


class Job:
    """one layer of a call: operands on the device, its destination at offset LEAD of a parent buffer, its definition"""

    def __init__(self, case, seed, integer, layout, accumulate):
        self.case, self.integer, self.accumulate = case, integer, accumulate
        pairs, base = wd.operands(case, seed, integer)
        self.ref, self.S, self.K = wd.reference(case, pairs, base if accumulate else None)
        wv, numel = case.view()
        self.wv, self.numel = nv.WView(wv.sT, wv.sO, wv.sI), numel
        self.parent = guard.empty(LEAD + numel, dtype=torch.float32, device=dev())
        self.parent[:LEAD] = SENTINEL
        if accumulate:
            self.parent[LEAD:] = base.to(dev())
        self.out = self.parent[LEAD:]
        self.pairs = [(stored(g, layout), stored(x, layout)) for g, x in pairs]
        self.vmap = None if case.vmap is None else torch.tensor(case.vmap, dtype=torch.int32, device=dev())

    def as_dict(self):
        c = self.case
        return dict(g=self.pairs[0][0], x=self.pairs[0][1], Cin=c.Cin, taps=c.taps, tap_mode=c.mode, t_stride=c.stride, vmap=self.vmap,
                    wv=self.wv, out=self.out, accumulate=self.accumulate, extra=self.pairs[1:])

    def check(self, split, what):
        """-> max err / bracket (0 on integer data, where equality is asserted)"""
        got = self.parent.cpu()
        assert (got[:LEAD] == SENTINEL).all(), what + ": wrote in front of its destination"
        out = got[LEAD:].double()
        guard.assert_no_poison(got[LEAD:], what)
        if self.integer:
            bad = (out != self.ref).nonzero().reshape(-1)
            assert bad.numel() == 0, "%s: %d of %d elements differ from the exact result, first at %d: %r != %r" % (
                what, bad.numel(), out.numel(), int(bad[0]), float(out[bad[0]]), float(self.ref[bad[0]]))
            return 0.0
        assert self.K <= wd.K_FLOAT_MAX
        r = wd.worst_ratio(out, self.ref, self.S, self.K, split=split)
        assert r <= 1.0, "%s: outside the bracket, max err / bracket = %.3f" % (what, r)
        return r


def run_many(monkeypatch, launch, form, integer, layout="plane", accumulate=None, seed=0, check=True):
    """one kg_wgrad_many call of the launch's cases under its switches; asserts the reported plan, then every result.
    accumulate None: jobs alternate between write and accumulate.  -> (plan, jobs, max err / bracket)"""
    for k, v in {**launch.env, **FORMS[form]}.items():
        monkeypatch.setenv(k, v)
    jobs = [Job(c, seed + 10 * i, integer, layout, (i % 2 == 0) if accumulate is None else accumulate) for i, c in enumerate(launch.cases)]
    plan = []
    monkeypatch.setattr(nv, "last_wgrad_plan", plan)
    nv.wgrad_many([j.as_dict() for j in jobs])
    monkeypatch.setattr(nv, "last_wgrad_plan", None)
    launch.check(launch.cases, plan)
    worst = 0.0
    for i, j in enumerate(jobs):
        if check:
            worst = max(worst, j.check(form == "bf16split", "%s job %d (%s), tile %s x %d splits" % (
                form, i, j.case.name, nv.WGRAD_TILE_NAMES[plan[i][0]], plan[i][1])))
    return plan, jobs, worst


def report(name, form, worst):
    print("wgrad_tiles_err %-9s %-60s max(err / bracket) = %.4f" % (form, name, worst))


def test_variant_numbers_are_the_headers():
    assert (nv.WGRAD_TILE_128x128, nv.WGRAD_TILE_64x64, nv.WGRAD_TILE_64x32, nv.WGRAD_TILE_32x64, nv.WGRAD_TILE_32x32) == (
        wd.T128, wd.T6464, wd.T6432, wd.T3264, wd.T3232) and nv.WGRAD_MAX_SPLITS == wd.MAX_SPLITS


# ---- the 128 x 128 tile -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["default plan, 128x128, 4096 columns", "default plan, 128x128, three pairs"])
def test_big_tile_default_plan_is_exact(name, form, monkeypatch):
    """M = Cin = 128, 3 taps, 4096 columns: the tile the default plan gives the wide layers, no tuning switch set"""
    for accumulate in (False, True):
        plan, _, _ = run_many(monkeypatch, wd.LAUNCHES[name], form, integer=True, accumulate=accumulate, seed=3)
        assert plan[0][0] == nv.WGRAD_TILE_128x128 and plan[0][1] > 1


BIG_NAMES = ["forced 128x128: " + c.name for c in wd.BIG_CASES]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", BIG_NAMES)
def test_big_tile_forced_at_small_column_counts(name, form, monkeypatch):
    """KG_WGRAD_BIGCOLS=0: full and ragged 128-row tiles, ragged chunks, one column, stride 2, channel blocks, a vertex map
    with dropped entries; both storages, write and accumulate, integer (exact) and float (bracket) data"""
    worst = 0.0
    for layout in ("plane", "nchw"):
        for accumulate in (False, True):
            for integer in (True, False):
                plan, _, r = run_many(monkeypatch, wd.LAUNCHES[name], form, integer, layout, accumulate, seed=5)
                assert plan[0][0] == nv.WGRAD_TILE_128x128
                worst = max(worst, r)
    report(name, form, worst)


@pytest.mark.parametrize("form", list(FORMS))
def test_big_tile_forced_all_shapes_in_one_call(form, monkeypatch):
    name = "forced 128x128, all shapes in one call"
    run_many(monkeypatch, wd.LAUNCHES[name], form, integer=True, seed=7)
    _, _, worst = run_many(monkeypatch, wd.LAUNCHES[name], form, integer=False, seed=8)
    report(name, form, worst)


# ---- the four smaller tiles through kg_wgrad_many --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("i", range(len(wd.SMALL_CASES)), ids=["%s-%s" % (nv.WGRAD_TILE_NAMES[v], c.name) for v, c in zip(wd.SMALL_VARIANTS, wd.SMALL_CASES)])
def test_small_tiles_one_job_each(i, form, monkeypatch):
    """the twelve edge shapes of test_wgrad and the vertex-gather shape, each alone in a kg_wgrad_many call: exact on integer
    data at the full shape, inside the bracket on float data at the shortened one"""
    v, c = wd.SMALL_VARIANTS[i], wd.SMALL_CASES[i]
    for accumulate in (False, True):
        plan, _, _ = run_many(monkeypatch, wd.LAUNCHES["small tile %d: %s" % (v, c.name)], form, True, "nchw", accumulate, seed=20 + i)
        assert plan[0][0] == v
    name = "small tile %d: short %s" % (v, c.name)
    plan, _, worst = run_many(monkeypatch, wd.LAUNCHES[name], form, False, "plane", True, seed=40 + i)
    assert plan[0][0] == v
    report(name, form, worst)


@pytest.mark.parametrize("form", list(FORMS))
def test_small_tiles_all_in_one_call(form, monkeypatch):
    """all thirteen in one call: each of the four variants occurs, one-split jobs next to jobs with 2 - 7 and with 13 splits"""
    plan, _, _ = run_many(monkeypatch, wd.LAUNCHES["small tiles, all shapes in one call"], form, integer=True, seed=60)
    assert {v for v, _ in plan} == {nv.WGRAD_TILE_64x64, nv.WGRAD_TILE_64x32, nv.WGRAD_TILE_32x64, nv.WGRAD_TILE_32x32}
    name = "small tiles, short float shapes in one call"
    plan, _, worst = run_many(monkeypatch, wd.LAUNCHES[name], form, integer=False, seed=61)
    assert {v for v, _ in plan} == {nv.WGRAD_TILE_64x64, nv.WGRAD_TILE_64x32, nv.WGRAD_TILE_32x64, nv.WGRAD_TILE_32x32}
    report(name, form, worst)


# ---- split classes ---------------------------------------------------------------------------------------------------------------
SPLIT_LAUNCHES = ["one split", "every job several splits", "small tiles, all shapes in one call", "128 splits",
                  "128 splits next to a small job", "short last split", "short last split, 128x128"]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", SPLIT_LAUNCHES)
def test_split_classes(name, form, monkeypatch):
    """a job the tile kernel writes itself; a launch of slab jobs only; a mixed one; 2 - 7 splits; more than 8 with a
    remainder modulo 8 (both branches of the XCD-aware order); the cap of 128; a pair whose last split is shorter - each
    asserted from the reported plan (Launch.check), exact on integer data"""
    launch = wd.LAUNCHES[name]
    assert launch.classes
    for accumulate in (False, True):
        run_many(monkeypatch, launch, form, integer=True, accumulate=accumulate, seed=70)


# ---- single-layer kg_wgrad on the bf16-split tile -------------------------------------------------------------------------------
def _single(case, seed, integer, accumulate, defer=None):
    j = Job(case, seed, integer, "plane", accumulate)
    d = j.as_dict()
    nv.wgrad(d["g"], d["x"], d["Cin"], d["taps"], d["tap_mode"], d["t_stride"], d["vmap"], j.numel, j.wv, out=j.out,
             accumulate=accumulate, extra=d["extra"], defer=defer)
    return j


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("i", range(len(wd.SMALL_CASES)), ids=[c.name for c in wd.SMALL_CASES])
def test_single_layer_kernel(i, form, monkeypatch):
    """kg_wgrad (always the 64 x 64 tile: kg_wgrad_bs_kernel with KG_WGRAD_SPLIT=1) on every edge shape, with one and with
    three operand pairs, finished at once and through kg_wgrad_reduce_many"""
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    plan = []
    monkeypatch.setattr(nv, "last_wgrad_plan", plan)
    c = wd.SMALL_CASES[i]
    c3 = c._replace(Ns=(c.Ns[0], c.Ns[0] + 1, 1))
    worst = 0.0
    for case, integer in ((c, True), (c3, True), (c.short(), False), (c3.short(), False)):
        j = _single(case, 80 + i, integer, accumulate=integer)
        assert plan == [(nv.WGRAD_TILE_64x64, plan[0][1])] and 1 <= plan[0][1] <= nv.WGRAD_MAX_SPLITS + 2
        worst = max(worst, j.check(form == "bf16split", "%s kg_wgrad %s" % (form, case.name)))
    deferred = []
    jobs = [_single(case, 90 + i, True, accumulate=acc, defer=deferred) for case, acc in ((c, False), (c3, True))]
    assert len(deferred) == 2 and deferred[0]["splits"] >= 1
    nv.wgrad_reduce_many(deferred)
    for j in jobs:
        j.check(form == "bf16split", "%s kg_wgrad deferred %s" % (form, j.case.name))
    monkeypatch.setattr(nv, "last_wgrad_plan", None)
    report("kg_wgrad " + c.name, form, worst)


# ---- determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["default plan, 128x128, three pairs", "forced 128x128, all shapes in one call",
                                  "small tiles, short float shapes in one call", "short last split"])
def test_three_runs_give_the_same_bits(name, form, monkeypatch, guard_all):
    """float data, three calls on the same operands: bit-identical results (fixed-order slab reduction, no atomics).  The
    call owns no ticket counter and no word outside its workspace and destinations: every counter of the binding is still
    zero and every red zone intact after the three runs"""
    launch = wd.LAUNCHES[name]
    bracketed = max(c.K for c in launch.cases) <= wd.K_FLOAT_MAX        # (beyond: the runs are compared with each other only)
    runs = []
    for _ in range(3):
        _, jobs, _ = run_many(monkeypatch, launch, form, integer=False, seed=95, check=bracketed)
        torch.cuda.synchronize()
        runs.append([j.parent.cpu().view(torch.int32) for j in jobs])
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))
    guard_all.check()
    for buf in nv._sync_bufs.values():
        assert not buf.any()
