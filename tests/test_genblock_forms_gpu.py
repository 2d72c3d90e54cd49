"""-m gpu: every kernel form of csrc/kg_genblock.hip - the six compile-time geometries and the run-time form of the forward,
backward and inference kernels, both contraction paths with the three VALU row buckets, both operand orientations, the three
residual kinds with and without BatchNorm, the finished-input and pending-tail entries, both last-arriver reductions - and
the logical edges of the operation, against the float64 definition of tests/genblock_def.py, on poisoned, red-zoned buffers.

Every test asserts, through `_native.last_genblock_form` (kg_genblock_form on the arguments of the launch), that the
instantiation and the contraction paths it is named after ran: the launches and their expectations are the tables of
genblock_def (TABLE_A, TABLE_B), which tests/test_genblock_def_cpu.py plans on the host as well.  Every plane operand is a
channel slice of a wider channel-major parent with sentinels in front; every result is a plane view behind a lead that must
still hold the poison word.  Comparisons: bit equality on integer data (genblock_def: every fp32 operation is exact in every
order; the rows behind a division or rsqrt keep their bracket), the derived per-element bracket on seeded normal data, each
stage against the definition applied to the kernel's own taped input of that stage; no poison word left in a result; on
Table A the compile-time and the run-time form bit-equal on integer data."""
import os

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from tests import genblock_def as gd
from tests import guard
from tests.guard import guard_all  # noqa: F401  (autouse: every test of this module runs on poisoned, red-zoned buffers)
from tests.util import ReloadingEnv

pytestmark = pytest.mark.gpu
LEAD = 7                    # floats in front of every operand inside its parent buffer
SENTINEL = -54321.0
FILL = -12345.0             # the channels of a parent that are not the operand's
ERR_LOG = os.environ.get("KG_GENBLOCK_FORMS_ERR_LOG")   # append the observed max(err / bracket) per direction and form
worst_by_form = {}                                      # (profiles/genblock_forms_err.log)


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
            for key in sorted(worst_by_form):
                w, what, n = worst_by_form[key]
                f.write("genblock_forms_err %-6s %-4s max(err / bracket) = %.4f (%s) over %d float launches\n" % (key + (w, what, n)))
            f.write("genblock_forms_err every bracket term is derived (tests/genblock_def.py); none was measured\n")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def report(direction, form, name, r, what):
    print("genblock_forms_err %-6s %-4s %-40s max(err / bracket) = %.4f (%s)" % (direction, form, name, r, what))
    w, ww, n = worst_by_form.get((direction, form), (0.0, "-", 0))
    worst_by_form[(direction, form)] = (r, what, n + 1) if r > w else (w, ww, n + 1)


def dims_of(c, act):
    return nv.GenBlockDims(Cin=c.Cin, C=c.C, K=c.K, Kp=c.Kp, Tc=c.Tc, Vc=c.Vc, T=c.T, V=c.V, rep=c.rep, res_kind=c.res, bn_t=bool(c.bn_t),
                           act=act)


class Parents:
    """the parent buffers of a launch's plane operands: sentinels and filler channels are checked after the launch"""

    def __init__(self):
        self.items = []

    def plane(self, t):
        """(N, C, T, V) as channels 1 .. C of a channel-major (C + 2, N, T, V) parent that starts LEAD floats inside its buffer"""
        n, c, tt, v = t.shape
        flat = guard.empty(LEAD + (c + 2) * n * tt * v, dtype=torch.float32, device=dev())
        flat[:LEAD] = SENTINEL
        flat[LEAD:] = FILL
        parent = flat[LEAD:].view(c + 2, n, tt, v)
        view = parent[1:c + 1].permute(1, 0, 2, 3)
        view.copy_(t)
        assert nv.is_plane(view) and (not view.is_contiguous() or n == 1 or c == 1 or tt * v == 1)
        self.items.append((flat, parent, c))
        return view

    def check(self, what):
        for flat, parent, c in self.items:
            assert bool((flat[:LEAD] == SENTINEL).all()), what + ": wrote in front of an operand"
            assert bool((parent[0] == FILL).all()) and bool((parent[c + 1] == FILL).all()), what + ": wrote into a neighbouring channel"


def flat(t):
    """a contiguous operand (weights, vectors) in a guarded buffer of its own: 16-byte aligned"""
    if t is None:
        return None
    out = guard.empty(t.shape, dtype=t.dtype, device=dev())
    out.copy_(t)
    assert out.data_ptr() % 16 == 0
    return out


def lead_intact(t, what):
    """a result of the binding is a plane view PLANE_LEAD floats inside its buffer: the lead still holds the poison word"""
    base = t._base if t._base is not None else t
    if base.numel() > t.numel():
        assert guard.poison_count(base.reshape(-1)[:nv.PLANE_LEAD]) == nv.PLANE_LEAD, what + ": wrote in front of its destination"


def launch(c, kind, o, integer):
    """one launch of `kind` on the device -> ({name: CPU tensor} named as genblock_def names them, the form record)"""
    act, slope = c.act_for(integer, kind), gd.slope_of(integer)
    dims = dims_of(c, act)
    par = Parents()
    w = dict(wg=flat(o["wg"]), wr=flat(o.get("wr")), wt=flat(o["wt"]), B=flat(o["B"]), U=flat(o.get("U")))
    form = []
    nv.last_genblock_form = form
    try:
        got = {}
        if kind in ("fwd", "pend"):
            layers = {}
            for key in ("t", "r"):
                L = o.get("bn_" + key)
                layers[key] = None if L is None else {k: (flat(v) if torch.is_tensor(v) else v) for k, v in L.items()}
            kw = dict(br=flat(o.get("br")), bt=flat(o["bt"]), bn_t=layers["t"], bn_r=layers["r"], groups=c.groups, noise=flat(o["noise"]),
                      nw=flat(o["nw"]), slope=slope, **w)
            if kind == "fwd":
                res = nv.genblock_fwd(dims, x=par.plane(o["x"]), **kw)
            else:
                p = o["pend"]
                pend = dict(u=par.plane(p["u"]), r=None if p.get("r") is None else par.plane(p["r"]), ct=flat(p.get("ct")), cr=flat(p.get("cr")),
                            noise=flat(p.get("noise")), nw=flat(p.get("nw")), act=p["act"])
                res = nv.genblock_fwd(dims, pend=pend, **kw)
                got["x"] = res["x"]
            for k in ("yc", "z", "r", "u", "ct", "cr", "out"):
                if res[k] is not None:
                    got[k] = res[k]
            for key in ("t", "r"):
                if layers[key] is not None:
                    got["rm_" + key], got["rv_" + key] = layers[key]["running_mean"], layers[key]["running_var"]
                    assert int(layers[key]["num_batches_tracked"]) == 3 + c.groups
        elif kind == "infer":
            n, C, T, V = c.N, c.C, c.T, c.V
            dst = par.plane(torch.full((n, C, T, V), FILL))
            obuf = par.items[-1]
            obuf[1][1:C + 1].view(torch.int32).fill_(guard.PATTERN_A)                # the destination itself: poisoned
            res = nv.genblock_infer(dims, x=par.plane(o["x"]), br=flat(o.get("br")), bt=flat(o["bt"]), ct=flat(o.get("ict")), cr=flat(o.get("icr")),
                                    noise=flat(o["noise"]), nw=flat(o["nw"]), slope=slope, out=dst, **w)
            assert res is dst
            got["out"] = res
        else:
            prev = None
            sinks = None
            if kind == "bwdprev":
                p = o["prev"]
                sinks = {k: flat(v) for k, v in p["sinks"].items()}
                prev = dict(x=par.plane(p["x"]), act=p["act"], sinks=sinks,
                            u=None if p.get("u") is None else par.plane(p["u"]), r=None if p.get("r") is None else par.plane(p["r"]),
                            noise=flat(p.get("noise")),
                            bn_t=None if p.get("bn_t") is None else tuple(flat(t) for t in p["bn_t"]),
                            bn_r=None if p.get("bn_r") is None else tuple(flat(t) for t in p["bn_r"]))
            res = nv.genblock_bwd(dims, g=par.plane(o["g"]), out=par.plane(o["out"]), u=par.plane(o["u"]) if c.bn_t else None,
                                  r=par.plane(o["r"]) if c.res == 2 else None, coef=flat(o["coef"]), prev=prev, slope=slope, **w)
            for k in ("du", "dr", "gyc", "zf", "gx", "pcoef"):
                if res[k] is not None:
                    got[k] = res[k]
            if sinks is not None:
                got.update({"sink_" + k: v for k, v in sinks.items()})
    finally:
        nv.last_genblock_form = None
    assert len(form) == 1, form
    what = "%s %s" % (c.name, kind)
    out = {}
    for k, v in got.items():
        if v.dim() == 4 and kind != "infer":
            lead_intact(v, what + " " + k)
        out[k] = v.detach().cpu().contiguous()
        guard.assert_no_poison(out[k], what + " " + k)
    par.check(what)
    return out, form[0]


def check_form(c, kind, rt, f):
    d = gd.DIR_OF[kind]
    want = dict(gd.paths(c, d), geometry=-1 if rt else c.geometry(), grid_x=c.N, dir=d)
    if rt:
        want.update((c.expect or {}).get(d, {}))
    bad = {k: (v, f[k]) for k, v in want.items() if f[k] != v}
    assert not bad and f["lds_bytes"] > 0, "%s %s: (expected, reported) form differs at %s: %r" % (c.name, kind, bad, f)


def compare(c, kind, o, got, integer):
    """-> (max err / bracket over the tensors of the launch, the tensor it was seen at)"""
    ref, br = gd.reference(c, o, kind, integer, got=got)
    assert set(ref) <= set(got), (sorted(ref), sorted(got))
    worst, where = 0.0, "-"
    for k in ref:
        what = "%s %s %s (%s)" % (c.name, kind, k, "integer" if integer else "float")
        g = got[k].double()
        assert tuple(g.shape) == tuple(ref[k].shape), (what, g.shape, ref[k].shape)
        if integer and k not in gd.BRACKETED_ON_INTEGERS:
            bad = (g != ref[k]).nonzero()
            assert bad.numel() == 0, "%s: %d of %d elements differ from the exact result, first at %r: %r != %r" % (
                what, bad.shape[0], g.numel(), tuple(bad[0].tolist()), float(g[tuple(bad[0])]), float(ref[k][tuple(bad[0])]))
            continue
        r = gd.worst_ratio(g, ref[k], br[k])
        assert r <= 1.0, "%s: outside the bracket, max err / bracket = %.3f" % (what, r)
        if r > worst:
            worst, where = r, k
    for k in got:                       # a parameter-gradient sink of a branch the previous block does not have: untouched
        if k.startswith("sink_") and k not in ref:
            assert bool((got[k] == 0.25).all()), "%s %s: %s was written" % (c.name, kind, k)
    return worst, where


def run(c, kind, monkeypatch, rt):
    """integer and float data in one form -> (integer results, worst ratio, its tensor)"""
    if rt:
        monkeypatch.setenv("KG_GB_RT", "1")
    else:
        monkeypatch.delenv("KG_GB_RT", raising=False)
    oi = gd.operands(c, kind, 21, True)
    gi, f = launch(c, kind, oi, True)
    check_form(c, kind, rt, f)
    compare(c, kind, oi, gi, True)
    of = gd.operands(c, kind, gd.DATA_SEED, False)
    gf, f = launch(c, kind, of, False)                  # (the same ticket counter, not re-zeroed in between)
    check_form(c, kind, rt, f)
    r, where = compare(c, kind, of, gf, False)
    report(gd.DIR_OF[kind], "rt" if rt else "geo", "%s %s" % (c.name, kind), r, where)
    return gi


@pytest.mark.parametrize("name,kind", gd.launches(gd.TABLE_A))
def test_instantiation(name, kind, monkeypatch):
    """Table A: the launch in its GbGeo form and in the run-time form - the reported instantiation is the one the case is named
    after, exact on integer data, inside the bracket on float data, and the two forms bit-equal on integer data"""
    c = gd.CASES[name]
    a = run(c, kind, monkeypatch, False)
    b = run(c, kind, monkeypatch, True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "%s %s: %s differs between the compile-time and the run-time form" % (name, kind, k)


@pytest.mark.parametrize("name,kind", gd.launches(gd.TABLE_B))
def test_edge(name, kind, monkeypatch):
    """Table B, the logical edges in the run-time form"""
    run(gd.CASES[name], kind, monkeypatch, True)


@pytest.mark.parametrize("name", [c.name for c in gd.TABLE_B if c.reject])
def test_refused(name, monkeypatch):
    """the shapes one step beyond an edge: the launcher answers with its error code and launches nothing"""
    c = gd.CASES[name]
    monkeypatch.setenv("KG_GB_RT", "1")
    for what in c.reject:
        kind = "fwd" if what == "dims" else what
        with pytest.raises(RuntimeError, match="kg_genblock"):
            launch(c, kind, gd.operands(c, kind, 5, True), True)


@pytest.mark.parametrize("name,kind", [("g0-N4g2", "fwd"), ("g2-N5g1", "bwdprev"), ("res2-bn1", "pend")])
def test_same_ticket_counter_twice(name, kind, monkeypatch):
    """two launches on the same ticket counter without re-zeroing it: the same bits both times"""
    c = gd.CASES[name]
    o = gd.operands(c, kind, gd.DATA_SEED, False)
    a, _ = launch(c, kind, o, False)
    b, _ = launch(c, kind, o, False)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (name, kind, k)


def test_hook_is_off_by_default():
    assert nv.last_genblock_form is None
