"""-m gpu: every kernel form of csrc/kg_agg.hip and csrc/kg_aggconv.hip - frame, stream and matrix-core expand / reduce with
their sub-tile, grid and epilogue variants, both outer forms, kg_agg_outer_many across its launch boundaries, the four tile
plans and the tiny form of kg_aggconv with and without the label bias - against the float64 definitions of tests/agg_def.py,
on poisoned, red-zoned buffers.

Every test asserts, through `_native.last_agg_plan` / `_native.last_aggconv_plan` (kg_agg_plan_info, kg_agg_outer_many_plan,
kg_aggconv_plan_info), that the form and instantiation it is named after ran: the launches and their expectations are the
tables of agg_def (AGG_CASES, MANY, CONV_CASES), which tests/test_agg_def_cpu.py plans on the host as well.  Comparisons: bit
equality on integer data (agg_def: every fp32 operation is exact in every order), the derived per-element bracket on seeded
normal data; no poison word left in a result; sentinels intact in front of destinations inside a parent buffer."""
import os

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from tests import agg_def as ad
from tests import guard
from tests.guard import guard_all  # noqa: F401  (autouse: every test of this module runs on poisoned, red-zoned buffers)
from tests.util import ReloadingEnv

pytestmark = pytest.mark.gpu
LEAD = 7                    # floats in front of every destination inside its parent buffer
SENTINEL = -12345.0
ERR_LOG = os.environ.get("KG_AGG_FORMS_ERR_LOG")        # append the observed max(err / bracket) per form (profiles/agg_forms_err.log)
worst_by_form = {}


@pytest.fixture
def monkeypatch(monkeypatch):
    """the environment through tests/util.ReloadingEnv: every change is followed by kg_reload_env()"""
    env = ReloadingEnv(monkeypatch)
    yield env
    env.undo()


@pytest.fixture(scope="module", autouse=True)
def err_log():
    yield
    if ERR_LOG and worst_by_form:
        with open(ERR_LOG, "a") as f:
            for form in sorted(worst_by_form):
                f.write("agg_forms_err %-24s max(err / bracket) = %.4f over %d float cases\n" % ((form,) + worst_by_form[form]))


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


def adjacency(A, transposed):
    """on the device; `transposed`: the (K, V, W) view of a contiguous (K, W, V) tensor (what the adjoint passes hand over)"""
    return A.transpose(1, 2).contiguous().to(dev()).transpose(1, 2) if transposed else A.to(dev())


def report(form, name, r):
    print("agg_forms_err %-18s %-52s max(err / bracket) = %.4f" % (form, name, r))
    w, n = worst_by_form.get(form, (0.0, 0))
    worst_by_form[form] = (max(w, r), n + 1)


def compare(got, ref, S, n, b, integer, what):
    """-> max err / bracket (0 on integer data, where equality is asserted)"""
    got = got.detach().cpu()
    guard.assert_no_poison(got, what)
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    if integer:
        g, r = got.double().reshape(-1), ref.reshape(-1)
        bad = ((g != r) & ~(g.isnan() & r.isnan())).nonzero().reshape(-1)
        assert bad.numel() == 0, "%s: %d of %d elements differ from the exact result, first at %d: %r != %r" % (
            what, bad.numel(), g.numel(), int(bad[0]), float(g[bad[0]]), float(r[bad[0]]))
        return 0.0
    r = ad.worst_ratio(got, ref, S, n, b)
    assert r <= 1.0, "%s: outside the bracket, max err / bracket = %.3f" % (what, r)
    return r


def check_plan(c, p):
    bad = {k: (v, p[k]) for k, v in c.expect.items() if p[k] != v}
    assert not bad, "%s: (expected, reported) plan differs at %s: %r" % (c.name, bad, p)


def outer_dest(K, V, W):
    """a (K, V, W) destination LEAD floats inside its parent, sentinels in front"""
    parent = guard.empty(LEAD + K * V * W, dtype=torch.float32, device=dev())
    parent[:LEAD] = SENTINEL
    return parent, parent[LEAD:].view(K, V, W)


def launch_agg(c, o, integer):
    """one launch of the case on the device -> (result, parent buffer or None)"""
    slope = ad.SLOPE_EXACT if integer else ad.SLOPE_FLOAT
    if c.op == "expand":
        return nv.agg_expand(stored(o["x"], c.layout), adjacency(o["A"], c.a_tr), c.rep), None
    if c.op == "reduce":
        res = stored(o["res"], c.layout) if "res" in o else None
        inv = o["inv"].to(dev()) if o.get("inv") is not None else None
        mask = stored(o["mask"], c.layout) if "mask" in o else None
        if c.name.startswith("mfma reduce mask rows"):
            # the 128-bit mask path of the matrix-core epilogue: rows that line up with the output's, from the tensor itself
            fits = mask.stride(0) == c.T * c.W and mask.stride(1) % 4 == 0 and mask.data_ptr() % 16 == 0
            assert fits == ("unaligned" not in c.name), (c.name, mask.stride(), mask.data_ptr() % 16)
        return nv.agg_reduce(stored(o["y"], c.layout), adjacency(o["A"], c.a_tr), c.rep, res=res, res_tstride=c.res[0] if c.res else 1,
                             res_inv=inv, mask=mask, slope=slope), None
    parent, out = outer_dest(c.K, c.V, c.W)
    nv.agg_outer(stored(o["x"], c.layout), stored(o["y"], c.layout), c.K, c.rep, out=out)
    return out, parent


def run_agg(c, monkeypatch, integer, seed):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    o = c.operands(seed, integer)
    ref, S = c.reference(o, integer)
    plan = []
    monkeypatch.setattr(nv, "last_agg_plan", plan)
    got, parent = launch_agg(c, o, integer)
    monkeypatch.setattr(nv, "last_agg_plan", None)
    assert len(plan) == 1 and plan[0]["op"] == c.op, plan
    check_plan(c, plan[0])
    if parent is not None:
        assert bool((parent[:LEAD].cpu() == SENTINEL).all()), c.name + ": wrote in front of its destination"
    return compare(got, ref, S, c.n, c.b, integer, "%s (%s)" % (c.name, "integer" if integer else "float")), plan[0]


@pytest.mark.parametrize("name", list(ad.AGG))
def test_agg_case(name, monkeypatch):
    """one launch of the table: the reported form / instantiation / geometry is the one the case is named after; exact on
    integer data, inside the bracket on float data (cases too long for the mutation check are exact-only)"""
    c = ad.AGG[name]
    _, p = run_agg(c, monkeypatch, True, 21)
    if c.is_float:
        r, p = run_agg(c, monkeypatch, False, ad.DATA_SEED)
        report(ad.FORM_NAMES[p["form"]] + " " + c.op, name, r)


def test_agg_hook_is_off_by_default():
    assert nv.last_agg_plan is None and nv.last_aggconv_plan is None


# ---- kg_agg_outer_many -----------------------------------------------------------------------------------------------------------
def run_many(m, monkeypatch, integer, seed):
    """one kg_agg_outer_many call, every destination a slice of ONE packed buffer -> (packed buffer on the host, worst ratio)"""
    for k, v in m.env.items():
        monkeypatch.setenv(k, v)
    sizes = [j.K * j.V * j.W for j in m.jobs]
    packed = guard.empty(LEAD + sum(sizes), dtype=torch.float32, device=dev())
    packed[:LEAD] = SENTINEL
    ops = [j.operands(seed + 10 * i, integer) for i, j in enumerate(m.jobs)]
    plan, defer, off = [], [], LEAD
    monkeypatch.setattr(nv, "last_agg_plan", plan)
    for j, o, n in zip(m.jobs, ops, sizes):
        nv.agg_outer(stored(o["x"], j.layout), stored(o["y"], j.layout), j.K, j.rep, out=packed[off:off + n].view(j.K, j.V, j.W), defer=defer)
        off += n
    nv.agg_outer_finish(defer)
    monkeypatch.setattr(nv, "last_agg_plan", None)
    assert len(plan) == 1 and plan[0]["op"] == "outer_many" and plan[0]["launch"] == m.launch, (plan, m.launch)
    host = packed.cpu()
    assert bool((host[:LEAD] == SENTINEL).all()), "wrote in front of the packed buffer"
    worst, off = 0.0, LEAD
    for i, (j, o, n) in enumerate(zip(m.jobs, ops, sizes)):
        ref, S = j.reference(o, integer)
        worst = max(worst, compare(host[off:off + n].view(j.K, j.V, j.W), ref, S, j.n, j.b, integer, "job %d of %d" % (i, len(m.jobs))))
        off += n
    return host, worst, plan[0], ops


@pytest.mark.parametrize("name", list(ad.MANY))
def test_outer_many(name, monkeypatch):
    """1, 8, 9, 17 jobs, shared and one-by-one jobs interleaved across the 8- and 16-job boundaries, a small budget: the
    reported launch of every job is the table's; exact on integer data; on float data inside the bracket, as is the
    single-launch result of every job; three runs give identical bits"""
    m = ad.MANY[name]
    run_many(m, monkeypatch, True, 31)
    runs = [run_many(m, monkeypatch, False, 32) for _ in range(3)]
    assert all(torch.equal(runs[0][0].view(torch.int32), r[0].view(torch.int32)) for r in runs[1:])
    _, worst, plan, ops = runs[0]
    if name == "budget 6":
        assert plan["slabs"][2] < 80 and plan["slabs"][0] == 1
    for j, o in zip(m.jobs, ops):
        ref, S = j.reference(o, False)
        _, out = outer_dest(j.K, j.V, j.W)
        nv.agg_outer(stored(o["x"], j.layout), stored(o["y"], j.layout), j.K, j.rep, out=out)
        worst = max(worst, compare(out, ref, S, j.n, j.b, False, "single launch of " + j.name))
    report("outer_many", name, worst)


# ---- kg_aggconv / kg_aggconv_label -----------------------------------------------------------------------------------------------
def run_conv(c, monkeypatch, integer, seed):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    o = c.operands(seed, integer)
    ref, xa_ref, S, Sxa = c.reference(o, integer)
    d = dev()
    J = c.label[1] if c.label else 0
    wfull = o["wfull"].to(d)
    wview = wfull.reshape(-1)[c.cc + J:]                       # addressed inside its parent
    assert wview.data_ptr() == wfull.data_ptr() + 4 * (c.cc + J)
    wv = nv.WView(*o["wv"])
    plan = []
    monkeypatch.setattr(nv, "last_aggconv_plan", plan)
    x, A, nbr = stored(o["x"], c.layout), o["A"].to(d), o["nbr"].to(d)
    if c.label:
        out, xa = nv.aggconv_label(x, A, nbr, o["pcount"], wview, wv, c.M, o["labels"].to(d), o["emb"].to(d), wfull.reshape(-1, c.Cin + J, 1, 1),
                                   c.Cin + J, J, want_xa=c.xa)
    else:
        add = o["add"].to(d) if "add" in o else None
        out, xa = nv.aggconv(x, A, nbr, o["pcount"], wview, wv, c.M, add=add, add_tstride=c.add if c.add is not None else 1, want_xa=c.xa)
    monkeypatch.setattr(nv, "last_aggconv_plan", None)
    assert len(plan) == 1, plan
    check_plan(c, plan[0])
    what = "%s (%s)" % (c.name, "integer" if integer else "float")
    r = compare(out, ref, S, c.n(o["pcount"]), c.b, integer, what)
    assert (xa is not None) == c.xa
    if c.xa:
        r = max(r, compare(xa, xa_ref, Sxa, max(o["pcount"]), ad.B_EXPAND, integer, what + " xa"))
    if c.label:                                                # a label outside [0, L) poisons its sample, and only it
        L = c.label[0]
        nan = out.detach().cpu().isnan().reshape(c.N, -1)
        for n, lab in enumerate(c.label[2]):
            assert bool(nan[n].all()) == (not 0 <= lab < L) and bool(nan[n].any()) == (not 0 <= lab < L), (c.name, n, lab)
    return r, plan[0]


@pytest.mark.parametrize("name", list(ad.CONV))
def test_aggconv_case(name, monkeypatch):
    """the four tile plans (narrow and wide source spans, with and without the aggregated planes, lean and general epilogue),
    an invalid plan value, the unforced rule; the tiny form for both row tiles, 1 / 2 / 4 threads per column, with `add` and
    with the label bias (labels outside [0, L) included): the reported plan is the one the case is named after"""
    c = ad.CONV[name]
    run_conv(c, monkeypatch, True, 41)
    r, p = run_conv(c, monkeypatch, False, ad.DATA_SEED)
    report("aggconv tiny" if p["tiny"] else "aggconv tile %d%d" % (p["BM"], p["KS"]), name, r)
