"""-m gpu: every kernel form of csrc/kg_conv.hip - the 110 instantiations of the direct kernel (six tiles, both weight
orientations, FAST 0 / 1 / 2, the lean epilogue, both K-split completion forms), the shared kg_conv_many launch, the bf16-split
column and window forms, the tiny kernel, the weight-pack and split-K epilogue helpers - and the logical edges of the
operation, against the float64 definition of tests/conv_def.py, on poisoned, red-zoned buffers.

Every test asserts, through `_native.last_conv_form` (kg_conv_form_info / kg_conv_many_form on the arguments of the launch), that
the family and instantiation it is named after ran: the launches and their expectations are the tables of conv_def (TABLE_A,
TABLE_B, MANY), which tests/test_conv_def_cpu.py plans on the host as well.  Comparisons: bit equality on integer data
(conv_def: every fp32 operation is exact in every order), the derived per-element bracket on seeded normal data; no poison
word left in a result; frames the launch does not own still hold what the caller put there; sentinels intact in front of
destinations inside a parent buffer."""
import os

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from tests import conv_def as cd
from tests import guard
from tests.guard import guard_all  # noqa: F401  (autouse: every test of this module runs on poisoned, red-zoned buffers)
from tests.util import ReloadingEnv

pytestmark = pytest.mark.gpu
LEAD = 7                    # floats in front of every destination inside its parent buffer
SENTINEL = -54321.0
ERR_LOG = os.environ.get("KG_CONV_FORMS_ERR_LOG")       # append the observed max(err / bracket) per family (profiles/conv_forms_err.log)
worst_by_family = {}


@pytest.fixture
def monkeypatch(monkeypatch):
    """the environment through tests/util.ReloadingEnv: every change is followed by kg_reload_env()"""
    env = ReloadingEnv(monkeypatch)
    yield env
    env.undo()


@pytest.fixture(scope="module", autouse=True)
def err_log():
    yield
    if ERR_LOG and worst_by_family:
        with open(ERR_LOG, "a") as f:
            for fam in sorted(worst_by_family):
                f.write("conv_forms_err %-8s max(err / bracket) = %.4f over %d float launches\n" % ((fam,) + worst_by_family[fam]))


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def report(fam, name, r):
    print("conv_forms_err %-8s %-48s max(err / bracket) = %.4f" % (fam, name, r))
    w, n = worst_by_family.get(fam, (0.0, 0))
    worst_by_family[fam] = (max(w, r), n + 1)


def put(t, layout="nchw", off=0):
    """the tensor in a guarded device buffer of its own, `off` floats inside it; (N, C, T, V) tensors NCHW or channel-major"""
    flat = guard.empty(t.numel() + off, dtype=t.dtype, device=dev())
    if t.dim() == 4 and layout == "plane":
        n, c, tt, v = t.shape
        view = flat[off:].view(c, n, tt, v).permute(1, 0, 2, 3)
    else:
        view = flat[off:].view(t.shape)
    view.copy_(t)
    return view


def conv_kwargs(c, o, integer):
    """conv()'s arguments for the case on the device -> (kwargs, parent buffer of a caller's `out` or None)"""
    groups = []
    for i, g in enumerate(c.groups):
        wv = o["wv"][i]
        x = put(o["x"][i], c.layout, g.x_off)
        assert (x.data_ptr() % 16 == 0) == (g.x_off == 0)
        vmap = None if o["vmap"][i] is None else put(o["vmap"][i])
        groups.append(nv.Group(x, put(o["w"][i])[wv.off:], nv.WView(wv.sT, wv.sO, wv.sI, wv.sMB, wv.MB), g.Cin, g.taps, g.tap_mode,
                               g.t_stride, g.transposed, vmap))
    kw = dict(groups=groups, N=c.N, M=c.M, T_out=c.T_out, V_out=c.V_out, act=c.act_for(integer), slope=c.slope(integer))
    for key in ("bias0", "bias1"):
        if key in o:
            kw[key] = put(o[key])
    if "add" in o:
        kw["add"], kw["add_tstride"] = put(o["add"], c.layout), c.add
    if "mask" in o:
        kw["mask"] = put(o["mask"], c.layout)
    parent = None
    if c.out is not None:
        t0, ots, T_total = c.out
        shape = (c.N, c.M, T_total, c.V_out)
        parent = guard.empty(LEAD + c.N * c.M * T_total * c.V_out, dtype=torch.float32, device=dev())
        parent[:LEAD] = SENTINEL
        parent[LEAD:] = cd.BASE
        body = parent[LEAD:]
        out = body.view(c.M, c.N, T_total, c.V_out).permute(1, 0, 2, 3) if c.layout == "plane" else body.view(shape)
        kw.update(out=out, out_t0=t0, out_tstride=ots)
    return kw, parent


def compare(c, got, o, integer, nsplit, what):
    """-> max err / bracket (0 on integer data, where equality is asserted)"""
    where = dev() if c.big else "cpu"
    ref, br = cd.reference(c, o, integer, nsplit, device=where)
    got = got.detach().to(where)
    guard.assert_no_poison(got, what)
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    if integer:
        bad = (got.double() != ref).nonzero()
        assert bad.numel() == 0, "%s: %d of %d elements differ from the exact result, first at %r: %r != %r" % (
            what, bad.shape[0], ref.numel(), tuple(bad[0].tolist()), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))
        return 0.0
    r = cd.worst_ratio(got, ref, br)
    assert r <= 1.0, "%s: outside the bracket, max err / bracket = %.3f" % (what, r)
    return r


def check_form(name, expect, f):
    bad = {k: (v, f[k]) for k, v in expect.items() if f[k] != v}
    assert not bad, "%s: (expected, reported) form differs at %s: %r" % (name, bad, f)


def run_case(c, monkeypatch, integer, seed):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    o = c.operands(seed, integer)
    kw, parent = conv_kwargs(c, o, integer)
    if c.wpack:
        kw["wpack"] = nv.conv_pack(kw["groups"], c.N, c.M, c.T_out, c.V_out)
        assert kw["wpack"] is not None and kw["wpack"].data_ptr() % 16 == 0
    form = []
    monkeypatch.setattr(nv, "last_conv_form", form)
    got = nv.conv(**kw)
    monkeypatch.setattr(nv, "last_conv_form", None)
    assert len(form) == 1, form
    check_form(c.name, c.expect or cd.DEFAULT_FORMS[c.name], form[0])
    if parent is not None:
        assert bool((parent[:LEAD].cpu() == SENTINEL).all()), c.name + ": wrote in front of its destination"
    return compare(c, got, o, integer, form[0]["nsplit"], "%s (%s)" % (c.name, "integer" if integer else "float")), form[0]


@pytest.mark.parametrize("name", [c.name for c in cd.TABLE_A])
def test_instantiation(name, monkeypatch):
    """Table A, one launch per reachable instantiation: the reported form is the one the case is named after; exact on integer
    data, inside the bracket on float data"""
    c = cd.CASES[name]
    run_case(c, monkeypatch, True, 21)
    r, f = run_case(c, monkeypatch, False, cd.DATA_SEED)
    report(f["family"], name, r)


@pytest.mark.parametrize("name", [c.name for c in cd.TABLE_B])
def test_edge(name, monkeypatch):
    """Table B, the logical edges on the default plan and on a forced direct tile with partial K-slices"""
    c = cd.CASES[name]
    run_case(c, monkeypatch, True, 22)
    r, f = run_case(c, monkeypatch, False, cd.DATA_SEED)
    report(f["family"], name, r)


def run_many(name, monkeypatch, integer, seed):
    _, jobs, env, expect = cd.MANY[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ops = [j.operands(seed + 10 * i, integer) for i, j in enumerate(jobs)]
    kws, parents = zip(*[conv_kwargs(j, o, integer) for j, o in zip(jobs, ops)])
    form = []
    monkeypatch.setattr(nv, "last_conv_form", form)
    outs = nv.conv_many([dict(k) for k in kws])
    monkeypatch.setattr(nv, "last_conv_form", None)
    assert form and form[0]["family"] == "many", form
    check_form(name, expect, form[0])
    # a shared launch is one record; a call that falls back records the single launch of every job behind it
    assert len(form) == (1 if form[0]["tile"] >= 0 else 1 + len(jobs)), form
    worst = 0.0
    for i, (j, o, got, parent) in enumerate(zip(jobs, ops, outs, parents)):
        if parent is not None:
            assert bool((parent[:LEAD].cpu() == SENTINEL).all()), "%s job %d: wrote in front of its destination" % (name, i)
        nsplit = 1 if form[0]["tile"] >= 0 else form[1 + i]["nsplit"]
        worst = max(worst, compare(j, got, o, integer, nsplit, "%s job %d (%s)" % (name, i, "integer" if integer else "float")))
    return worst


@pytest.mark.parametrize("name", list(cd.MANY))
def test_many(name, monkeypatch):
    """kg_conv_many: the twelve instantiations of the shared launch, an XCD-grouped job between plain ones, and calls that fall
    back to one launch per job: the reported shared tile, instantiation and per-job workgroup ranges are the table's"""
    run_many(name, monkeypatch, True, 31)
    report("many", name, run_many(name, monkeypatch, False, 32))


def test_hook_is_off_by_default():
    assert nv.last_conv_form is None
