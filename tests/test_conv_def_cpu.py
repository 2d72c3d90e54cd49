"""CPU: tests/conv_def.py can be trusted before a GPU is involved, and the launch tables of tests/test_conv_forms_gpu.py land on
the kernel forms they are named after.

  * the float64 definition lies within the bracket of oracle/prim_ref.conv and of a second fp32 evaluation in another
    summation order on every float case, and equals prim_ref bit for bit on integer data;
  * the definition with ONE column's tap read one frame later, ONE vmap entry changed, ONE weight pair swapped, bias1 dropped,
    `add` read without a_tstride, the mask side flipped at ONE element, or o_tstride ignored falls outside the bracket in at
    least one element, for every float case the mutation applies to - a kernel that is wrong by that much cannot pass;
  * every launch of the GPU tests is planned on the host (kg_conv_form_info / kg_conv_many_form: no GPU) onto the form it is
    named after, and Table A reaches every instantiation of conv_def.INSTANTIATIONS, no other;
  * the forms the default rules give the critic's conv launches at 64 samples are pinned.
(The two deep kg_conv_many shapes, Case.big, contract 1.5 and 3 G products per evaluation: they are planned here, their
definition - the same code - is evaluated on the device by the GPU tests only.)
"""
import ctypes

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from oracle import prim_ref as pr
from tests import conv_def as cd
from tests.util import ReloadingEnv

SEED = cd.DATA_SEED
FLOAT_CASES = [c for c in cd.TABLE_A + cd.TABLE_B if not c.big]
MANY_JOBS = {j.name: j for m in cd.MANY.values() for j in m[1] if not j.big}
FLOAT_ALL = {c.name: c for c in FLOAT_CASES}
FLOAT_ALL.update(MANY_JOBS)


@pytest.fixture
def monkeypatch(monkeypatch):
    env = ReloadingEnv(monkeypatch)
    yield env
    env.undo()


@pytest.fixture(scope="module")
def lib():
    return nv.load_library()


# ---- a KgConvArgs for the planner: geometry, strides, null-ness and alignment only -------------------------------------------------
PTR = 1 << 20              # (never dereferenced: kg_conv_form_info reads no operand)


def _strides(layout, N, C, T, V):
    """(sN, sC) as the binding derives them (_native._sn_sc)"""
    sn, sc = (T * V, N * T * V) if layout == "plane" else (C * T * V, T * V)
    return (sn if N > 1 else T * V), (sc if C > 1 else T * V)


def conv_args(c):
    a = nv._ConvArgs()
    a.N, a.M, a.T_out, a.V_out = c.N, c.M, c.T_out, c.V_out
    a.ngroups = len(c.groups)
    for i, g in enumerate(c.groups):
        cg = a.g[i]
        ch = g.Cin * (g.taps if g.tap_mode == cd.TAP_CHANBLOCK else 1)
        cg.x = PTR + 4 * g.x_off
        cg.x_sN, cg.x_sC = _strides(c.layout, c.N, ch, g.T_in, g.V_in)
        cg.Cin, cg.T_in, cg.V_in = g.Cin, g.T_in, g.V_in
        cg.vmap = PTR if g.vmap else None
        wv = c.weight_view(i)
        cg.w = PTR
        cg.w_sT, cg.w_sO, cg.w_sI, cg.w_sMB, cg.w_MB = wv.sT, wv.sO, wv.sI, wv.sMB, wv.MB
        cg.taps, cg.tap_mode, cg.t_stride, cg.transposed = g.taps, g.tap_mode, g.t_stride, int(g.transposed)
    t0, ots, T_total = c.out_spec()
    a.out = PTR
    a.o_sN, a.o_sC = _strides("plane" if c.out is None else c.layout, c.N, c.M, T_total, c.V_out)
    a.o_tstride = ots
    a.bias0 = PTR if c.bias0 else None
    a.bias1 = PTR if c.bias1 else None
    if c.add is not None:
        a.add = PTR
        a.a_sN, a.a_sC = _strides(c.layout, c.N, c.M, (c.T_out - 1) * c.add + 1, c.V_out)
        a.a_tstride = c.add
    else:
        a.a_tstride = 1
    a.act, a.slope = c.act, cd.SLOPE_FLOAT
    if c.mask:
        a.mask = PTR
        a.m_sN, a.m_sC = _strides(c.layout, c.N, c.M, c.T_out, c.V_out)
    if c.wpack:
        a.wpack = PTR
        a.wpack_bytes = nv.load_library().kg_conv_pack_bytes(ctypes.byref(a))
        assert a.wpack_bytes > 0, c.name
    # the binding hands a K-split launch its scratch and the stream's ticket counters (_native._workspace, lazy)
    if nv.load_library().kg_conv_workspace_bytes(ctypes.byref(a)) > 0:
        a.ws, a.ws_bytes = PTR, 1 << 40
        a.sync, a.sync_len = PTR, nv.SYNC_LEN
    return a


def plan(c, lib):
    return nv.conv_form_dict(conv_args(c))


def plan_many(jobs, lib):
    arr = (nv._ConvArgs * len(jobs))()
    for i, j in enumerate(jobs):
        arr[i] = conv_args(j)
    return nv.conv_many_form_dict(arr, len(jobs)), arr


def differs(expect, got):
    return {k: (v, got[k]) for k, v in expect.items() if got[k] != v}


# ---- planning -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cd.CASES))
def test_case_is_planned_onto_its_form(name, monkeypatch, lib):
    c = cd.CASES[name]
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    p = plan(c, lib)
    expect = c.expect or cd.DEFAULT_FORMS[name]
    assert not differs(expect, p), "%s: (expected, reported) form differs at %s: %r" % (name, differs(expect, p), p)
    # the coarse report agrees
    t, ns = ctypes.c_int32(), ctypes.c_int32()
    assert lib.kg_conv_plan_info(ctypes.byref(conv_args(c)), ctypes.byref(t), ctypes.byref(ns)) == 0
    assert (t.value, ns.value) == (p["tile"], p["nsplit"])
    assert (p["epilogue"] == 1) == (p["family"] == "direct" and p["nsplit"] > 1 and not p["INK"])
    # and the launch geometry follows from the instantiation
    if p["family"] == "direct":
        ncols = c.N * c.T_out * c.V_out
        ct, rt = -(-ncols // (32 * p["NW"] // p["KW"])), -(-c.M // p["BM"])
        assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (((ct + 7) // 8 * 8 * rt, 1) if p["xcd"] else (ct, rt)) + (p["nsplit"],)


@pytest.mark.parametrize("name", list(cd.MANY))
def test_many_call_is_planned_onto_its_form(name, monkeypatch, lib):
    _, jobs, env, expect = cd.MANY[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f, arr = plan_many(jobs, lib)
    assert not differs(expect, f), "%s: (expected, reported) form differs at %s: %r" % (name, differs(expect, f), f)
    t = ctypes.c_int32()
    assert lib.kg_conv_many_plan(arr, len(jobs), ctypes.byref(t)) == 0 and t.value == f["tile"]
    if f["tile"] >= 0:      # every job starts at a multiple of 8 workgroups, in order, and the grid holds them all
        assert all(b % 8 == 0 for b in f["wg_begin"]) and f["wg_begin"] == sorted(f["wg_begin"]) and f["wg_begin"][0] == 0
        assert f["total_wg"] >= f["wg_begin"][-1] + f["nwg"][-1]


def test_table_a_reaches_every_instantiation(monkeypatch, lib):
    """the union over Table A is the literal list - no instantiation without a case, no case on an unlisted one"""
    seen = {}
    for c in cd.TABLE_A:
        for k, v in c.env.items():
            monkeypatch.setenv(k, v)
        seen.setdefault(cd.instantiation(plan(c, lib)), []).append(c.name)
        monkeypatch.undo()
    for name, jobs, env, _ in cd.MANY_A:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        f, _ = plan_many(jobs, lib)
        assert f["tile"] >= 0, name
        seen.setdefault(cd.instantiation(f), []).append(name)
        monkeypatch.undo()
    missing = [i for i in cd.INSTANTIATIONS if i not in seen]
    extra = [i for i in seen if i not in cd.INSTANTIATIONS]
    assert not missing and not extra, (missing, extra)
    assert len(cd.INSTANTIATIONS) == 110 + 12 + 3 + 6 + 2


def test_hook_is_off_by_default():
    assert nv.last_conv_form is None and nv.last_conv_plan is None


# ---- the definition against prim_ref and another fp32 order -----------------------------------------------------------------------
def prim_ref_result(c, o, integer):
    groups = []
    for i, g in enumerate(c.groups):
        wv = o["wv"][i]
        groups.append(nv.Group(o["x"][i], o["w"][i][wv.off:], nv.WView(wv.sT, wv.sO, wv.sI, wv.sMB, wv.MB), g.Cin, g.taps, g.tap_mode,
                               g.t_stride, g.transposed, o["vmap"][i]))
    t0, ots, T_total = c.out_spec()
    dest = torch.full((c.N, c.M, T_total, c.V_out), cd.BASE)
    return pr.conv(groups, c.N, c.M, c.T_out, c.V_out, bias0=o.get("bias0"), bias1=o.get("bias1"), add=o.get("add"),
                   add_tstride=c.add or 1, act=c.act_for(integer), slope=c.slope(integer), mask=o.get("mask"), out=dest, out_t0=t0,
                   out_tstride=ots)


def other_order_fp32(c, o):
    """the same formula in fp32: groups, taps and channels backwards, the epilogue's additions in another order"""
    acc = torch.zeros(c.N, c.M, c.T_out, c.V_out)
    if o.get("add") is not None:
        acc = acc + o["add"][:, :, ::c.add][:, :, :c.T_out]
    for gi in reversed(range(len(c.groups))):
        g = c.groups[gi]
        W = cd.weights_f64(o["w"][gi], o["wv"][gi], g.taps, c.M, g.Cin).float()
        for d in reversed(range(g.taps)):
            xs, _ = cd.source_f64(o["x"][gi], g, d, c.T_out, c.V_out, o["vmap"][gi])
            acc = acc + torch.einsum("mc,nctv->nmtv", W[d].flip(1), xs.float().flip(1))
    for key in ("bias1", "bias0"):
        if o.get(key) is not None:
            acc = acc + o[key].view(1, -1, 1, 1)
    val = cd.act_f64(acc, c.act, torch.tensor(cd.SLOPE_FLOAT)) if c.act != cd.ACT_LRELU else torch.where(acc > 0, acc, acc * cd.SLOPE_FLOAT)
    if o.get("mask") is not None:
        val = val * torch.where(o["mask"] > 0, 1.0, cd.SLOPE_FLOAT)
    t0, ots, T_total = c.out_spec()
    out = torch.full((c.N, c.M, T_total, c.V_out), cd.BASE)
    out[:, :, t0:t0 + (c.T_out - 1) * ots + 1:ots] = val
    return out


@pytest.mark.parametrize("name", list(FLOAT_ALL))
def test_definition_against_prim_ref_and_another_order(name):
    c = FLOAT_ALL[name]
    o = c.operands(SEED, True)
    ref, _ = cd.reference(c, o, True)
    assert ref.abs().max() > 0 and torch.equal(prim_ref_result(c, o, True).double(), ref), "integer data: not the exact result"
    o = c.operands(SEED, False)
    ref, br = cd.reference(c._replace(expect={}), o, False)      # (the fp32 bracket with one slab: the narrowest any launch is held to)
    for what, got in (("prim_ref", prim_ref_result(c, o, False)), ("other order", other_order_fp32(c, o))):
        r = cd.worst_ratio(got, ref, br)
        assert r <= 1.0, "%s: the definition is %.3f brackets away from %s" % (name, r, what)


# ---- mutations: the bracket is tight enough to be a test ----------------------------------------------------------------------------
def mutations(c, o, ref):
    """the mutations that apply to the case, each aimed at a place where it changes something"""
    t0, ots, _ = c.out_spec()
    written = ref[:, :, t0:t0 + (c.T_out - 1) * ots + 1:ots]
    g0 = c.groups[0]
    muts = []
    if g0.T_in > 1 and not g0.transposed:       # a column whose last tap has a frame behind it
        to = 0
        vo = next(v for v in range(c.V_out) if o["vmap"][0] is None or int(o["vmap"][0][v]) >= 0)
        muts.append(("shift", c.N - 1, to, vo))
    if c.vmap_group() is not None and c.groups[c.vmap_group()].V_in > 1:
        muts.append(("vmap", 0))
    if g0.Cin > 1:
        muts.append(("wswap", c.M - 1, g0.Cin - 2))
    if c.bias1:
        muts.append(("nobias1",))
    if c.add is not None and c.add > 1 and c.T_out > 1:
        muts.append(("add_tstride",))
    if c.mask:
        idx = int(written.abs().reshape(-1).argmax())
        n, r = divmod(idx, c.M * c.T_out * c.V_out)
        m, r = divmod(r, c.T_out * c.V_out)
        muts.append(("maskflip", n, m) + divmod(r, c.V_out))
    if ots > 1 and c.T_out > 1:
        muts.append(("o_tstride",))
    return muts


@pytest.mark.parametrize("name", list(FLOAT_ALL))
def test_mutations_leave_the_bracket(name):
    """on the float data of the GPU tests, with the WIDEST bracket the case is compared under (its own form's)"""
    c = FLOAT_ALL[name]
    o = c.operands(SEED, False)
    nsplit = c.expect.get("nsplit", 1)
    ref, br = cd.reference(c, o, False, nsplit)
    muts = mutations(c, o, ref)
    assert muts, name
    for mu in muts:
        bad, _, _ = cd.conv_f64(c, o, c.slope(False), mutate=mu)
        r = cd.worst_ratio(bad, ref, br)
        assert r > 1.0, "%s: mutation %r stays inside the bracket (max err / bracket = %.3f)" % (name, mu, r)


def test_every_mutation_is_exercised():
    kinds = set()
    for c in FLOAT_ALL.values():
        o = c.operands(SEED, False)
        ref, _ = cd.reference(c, o, False)
        kinds |= {m[0] for m in mutations(c, o, ref)}
    assert kinds == {"shift", "vmap", "wswap", "nobias1", "add_tstride", "maskflip", "o_tstride"}


def test_parity_launches_are_the_transposed_stride_2_conv():
    """the two parity cases of Table B, on shared operands, are the definition of ONE transposed stride-2 temporal conv"""
    p0, p1 = cd.CASES["transposed stride 2 parity 0"], cd.CASES["transposed stride 2 parity 1"]
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (p0.N, 40, 5, 9), generator=gen).float()
    w = torch.randint(-3, 4, (3 * 40 * p0.M,), generator=gen).float()          # (taps, Cin, M): W(d, m, c) = w[d Cin M + c M + m]
    one = cd.WV(0, 1, p0.M, numel=40 * p0.M)
    tap = [w[d * 40 * p0.M:(d + 1) * 40 * p0.M] for d in range(3)]
    whole = cd.Case("whole", p0.N, p0.M, 10, 9, (cd.G(40, 5, 9, taps=3, t_stride=2, transposed=True, wkind="mf"),), {}, {})
    ref, _, _ = cd.conv_f64(whole, dict(x=[x], w=[w], wv=[whole.weight_view(0)], vmap=[None]), 0.25)
    r0, _, _ = cd.conv_f64(p0._replace(bias0=False), dict(x=[x], w=[tap[1]], wv=[one], vmap=[None]), 0.25)
    r1, _, _ = cd.conv_f64(p1._replace(bias0=False), dict(x=[x, x[:, :, 1:]], w=[tap[2], tap[0]], wv=[one, one], vmap=[None, None]), 0.25)
    both = torch.where(r0 != cd.BASE, r0, r1)
    assert ref.abs().max() > 0 and torch.equal(both, ref)


# ---- the default rules at the training step's launch shapes ------------------------------------------------------------------------
def spec_args(N, M, T_out, V_out, groups, add_tstride=None, bias0=False, bias1=False):
    """KgConvArgs of a launch on library-allocated plane tensors; groups: (ConvSpec, has vmap)"""
    a = nv._ConvArgs()
    a.N, a.M, a.T_out, a.V_out, a.ngroups = N, M, T_out, V_out, len(groups)
    for i, (sp, vmap) in enumerate(groups):
        cg = a.g[i]
        cg.x, cg.w, cg.vmap = PTR, PTR, (PTR if vmap else None)
        cg.x_sN, cg.x_sC = sp.T_in * sp.V_in, N * sp.T_in * sp.V_in
        cg.Cin, cg.T_in, cg.V_in = sp.Cin, sp.T_in, sp.V_in
        cg.w_sT, cg.w_sO, cg.w_sI, cg.w_sMB, cg.w_MB = sp.wv.sT, sp.wv.sO, sp.wv.sI, sp.wv.sMB, min(sp.wv.MB, 1 << 30)
        cg.taps, cg.tap_mode, cg.t_stride = sp.taps, sp.tap_mode, sp.t_stride
    a.out, a.o_sN, a.o_sC = PTR, T_out * V_out, N * T_out * V_out
    a.bias0, a.bias1 = (PTR if bias0 else None), (PTR if bias1 else None)
    a.a_tstride = 1
    if add_tstride is not None:
        a.add, a.a_sN, a.a_sC, a.a_tstride = PTR, T_out * add_tstride * V_out, N * T_out * add_tstride * V_out, add_tstride
    a.act, a.slope = nv.ACT_LRELU, 0.2
    if nv.load_library().kg_conv_workspace_bytes(ctypes.byref(a)) > 0:
        a.ws, a.ws_bytes, a.sync, a.sync_len = PTR, 1 << 40, PTR, nv.SYNC_LEN
    return a


def critic_forms(ds, n):
    """per critic block D0 .. D5 (disc_trunk.py): the gcn contraction of the unfused route (_gcn) and the tail (_tail: temporal
    conv + residual group or residual add, biases, LeakyReLU) -> (instantiation, nsplit, xcd) each, unforced"""
    from kinetic_gan_amd.discriminator import Discriminator
    from tests.util import CFG
    c = CFG[ds]
    D = Discriminator(c["channels"], c["n_classes"], c["t_size"], c["latent"], dataset=ds)
    meta = D._trunk_meta(c["t_size"], D.graph.num_node[0], torch.device("cpu"))
    out = []
    for g in meta.geoms:
        sg, st, sr = (g.spec_g1 if g.single else g.spec_g), g.spec_t, g.spec_r
        forms = []
        for a in (spec_args(n, sg.M, sg.T_out, sg.V_out, [(sg, False)]),
                  spec_args(n, st.M, st.T_out, st.V_out, [(st, False)] + ([(sr, sr.vmap is not None)] if g.res == "conv" else []),
                            add_tstride=st.t_stride if g.res == "identity" else None, bias0=True, bias1=g.res == "conv")):
            f = nv.conv_form_dict(a)
            forms.append(cd.instantiation(f) + (f["nsplit"], f["xcd"]))
        out.append(tuple(forms))
    return out


# per block D0 .. D5: (gcn launch, tail launch), each the instantiation (conv_def.instantiation) + (nsplit, xcd)
CRITIC_FORMS = {
    ('ntu', 64): [
        (('direct', 32, 4, 1, 1, 0, 0, 0, 1, 0), ('direct', 32, 4, 1, 1, 1, 1, 0, 1, 0)),
        (('direct', 32, 4, 1, 1, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 1, 2, 1, 0, 1, 0)),
        (('direct', 32, 4, 1, 1, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 1, 2, 1, 0, 1, 0)),
        (('direct', 32, 4, 1, 1, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 1, 2, 1, 1, 4, 0)),
        (('direct', 32, 4, 1, 4, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 4, 2, 1, 0, 1, 0)),
        (('direct', 32, 4, 1, 4, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 1, 1, 0, 0, 8, 0)),
    ],
    ('h36m', 64): [
        (('direct', 32, 2, 1, 1, 0, 0, 0, 1, 0), ('direct', 32, 2, 1, 1, 1, 1, 0, 1, 0)),
        (('direct', 32, 4, 1, 1, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 1, 2, 1, 0, 1, 0)),
        (('direct', 32, 4, 1, 1, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 4, 2, 1, 0, 1, 0)),
        (('direct', 32, 4, 1, 4, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 4, 2, 1, 0, 1, 0)),
        (('direct', 32, 4, 1, 4, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 1, 2, 1, 0, 8, 0)),
        (('direct', 32, 4, 1, 4, 1, 1, 0, 1, 0), ('direct', 32, 4, 1, 1, 1, 0, 0, 8, 0)),
    ],
}


@pytest.mark.parametrize("ds,n", [("ntu", 64), ("h36m", 64)])
def test_default_forms_of_the_critic_launches(ds, n, lib):
    """what the default rules give the training step's conv launches, unforced: a retuned rule - or a refactoring that moved
    a decision - shows here without a GPU (and must then update this table on purpose)"""
    assert critic_forms(ds, n) == CRITIC_FORMS[(ds, n)]
