"""CPU: tests/agg_def.py can be trusted before a GPU is involved, and the launch tables of tests/test_agg_forms_gpu.py land on the
kernel forms they are named after.

  * the float64 definitions equal oracle/prim_ref.py on integer data (where both are exact);
  * an fp32 evaluation in another summation order stays inside the bracket for the float cases;
  * the definition with ONE product left out, ONE frame read one frame later, or the residual hit test of ONE frame off by
    one falls outside the bracket in at least one element, for every float case - a kernel that is wrong by that much cannot
    pass the GPU tests;
  * every launch of the GPU tests is planned on the host (kg_agg_plan_info / kg_agg_outer_many_plan / kg_aggconv_plan_info:
    no GPU) onto the form and instantiation it is named after, and together the tables reach every instantiation;
  * the plans the default rules give the aggregation launches of the critic at the bench configurations are pinned.
"""
import ctypes

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import build
from oracle import prim_ref as pr
from tests import agg_def as ad
from tests.util import ReloadingEnv

FLOAT_AGG = [c for c in ad.AGG_CASES if c.is_float]
SEED = ad.DATA_SEED


# ---- the definitions against prim_ref ----------------------------------------------------------------------------------------
PRIM_CASES = ["frame expand K3 WP16", "frame reduce K3 WP28", "frame reduce K1 WP4", "stream expand K3 VM8", "mfma reduce SUB3 V5 485 frames",
              "mfma reduce V11 W11 KS17 RES1 MSK1", "outer mfma K3 TV2 TW2", "outer elementwise rep 2"]


@pytest.mark.parametrize("name", PRIM_CASES)
def test_definition_equals_prim_ref_on_integer_data(name):
    c = ad.AGG[name]
    o = c.operands(7, True)
    ref, _ = c.reference(o, True)
    if c.op == "expand":
        got = pr.agg_expand(o["x"], o["A"], c.rep)
    elif c.op == "reduce":
        got = pr.agg_reduce(o["y"], o["A"], c.rep, res=o.get("res"), res_tstride=c.res[0] if c.res else 1, res_inv=o.get("inv"),
                            mask=o.get("mask"), slope=ad.SLOPE_EXACT)
    else:
        got = pr.agg_outer(o["x"], o["y"], c.K, c.rep)
    assert ref.abs().max() > 0 and torch.equal(got.double(), ref)


@pytest.mark.parametrize("name", ["tile 321 XE3 XA1 ADD1", "tile 642 XE6 XA0 ADD1", "tile 642 tapmask hole", "tiny MT64 RG2 LB0"])
def test_aggconv_definition_equals_prim_ref_on_integer_data(name):
    c = ad.CONV[name]
    o = c.operands(7, True)
    ref, xa, _, _ = c.reference(o, True)
    got, gxa = pr.aggconv(o["x"], o["A"], o["nbr"], o["pcount"], o["wview"], nv.WView(*o["wv"]), c.M, add=o.get("add"),
                          add_tstride=c.add if c.add is not None else 1, want_xa=True)
    assert ref.abs().max() > 0 and torch.equal(got.double(), ref) and torch.equal(gxa.double(), xa)


def test_label_definition_equals_prim_ref_on_integer_data():
    c = ad.CONV["tiny MT32 RG1 LB1"]
    o = c.operands(7, True)
    ref, _, _, _ = c.reference(o, True)
    L, J, labels = c.label
    K, V, W = c.dims()
    ok = [n for n, lab in enumerate(labels) if 0 <= lab < L]
    bias = pr.label_bias_fwd(o["labels"][ok], o["emb"], o["wfull"].reshape(K * c.M, c.Cin + J, 1, 1), K, c.M, c.Cin + J, J, o["A"])
    got, _ = pr.aggconv(o["x"][ok], o["A"], o["nbr"], o["pcount"], o["wview"], nv.WView(*o["wv"]), c.M, add=bias, add_tstride=0)
    assert torch.equal(got.double(), ref[ok]) and bool(ref[[n for n in range(c.N) if n not in ok]].isnan().all())


# ---- another-order fp32 evaluation inside the bracket --------------------------------------------------------------------------
def emulate_fp32(c, o, slope=ad.SLOPE_FLOAT):
    """fp32 all the way in an order that is none of the kernels': the contraction index walked backwards"""
    if c.op == "expand":
        xr = o["x"].repeat_interleave(c.rep, 2)
        acc = torch.zeros(c.N, c.K, c.C, c.T * c.rep, c.W)
        for v in reversed(range(c.V)):
            acc = acc + xr[:, None, :, :, v, None] * o["A"][None, :, None, None, v, :]
        return acc.reshape(c.N, c.K * c.C, c.T * c.rep, c.W)
    if c.op == "reduce":
        y5 = o["y"].reshape(c.N, c.K, c.C, c.T, c.rep, c.V)
        acc = torch.zeros(c.N, c.C, c.T, c.W)
        for v in reversed(range(c.V)):
            part = torch.zeros_like(acc)
            for k in range(c.K):
                for q in range(c.rep):
                    part = part + y5[:, k, :, :, q, v, None] * o["A"][k, v]
            acc = acc + part
        if "res" in o:
            # (the definition of a zero aggregate is the scattered residual itself: copies, no arithmetic)
            acc = acc + ad.reduce_f64(torch.zeros_like(o["y"]), o["A"], c.rep, o["res"], c.res[0], o.get("inv")).float()
        if "mask" in o:
            acc = acc * torch.where(o["mask"] > 0, torch.ones(()), torch.tensor(slope))
        return acc
    xr = o["x"].repeat_interleave(c.rep, 2)
    y5 = o["y"].reshape(c.N, c.K, c.C, c.T * c.rep, c.W)
    acc = torch.zeros(c.K, c.V, c.W)
    for t in reversed(range(c.T * c.rep)):
        acc = acc + torch.einsum("ncv,nkcw->kvw", xr[:, :, t], y5[:, :, :, t])
    return acc


@pytest.mark.parametrize("c", FLOAT_AGG, ids=[c.name for c in FLOAT_AGG])
def test_another_order_stays_inside_the_bracket(c):
    assert c.n <= ad.N_FLOAT_MAX
    o = c.operands(SEED, False)
    ref, S = c.reference(o, False)
    r = ad.worst_ratio(emulate_fp32(c, o), ref, S, c.n, c.b)
    assert r <= 1.0, r
    o = c.operands(SEED + 1, True)
    ref, _ = c.reference(o, True)
    assert torch.equal(emulate_fp32(c, o, ad.SLOPE_EXACT).double(), ref)       # exact on integer data, as the kernels must be


@pytest.mark.parametrize("c", ad.CONV_CASES, ids=[c.name for c in ad.CONV_CASES])
def test_aggconv_another_order_stays_inside_the_bracket(c):
    o = c.operands(SEED, False)
    ref, xa, S, Sxa = c.reference(o, False)
    K, V, W = c.dims()
    # fp32: xa from the dense adjacency (zeros included) in torch's order, the channel contraction backwards
    xa32 = torch.einsum("nctv,kvw->nkctw", o["x"], o["A"])
    d = torch.arange(K).view(-1, 1, 1)
    m = torch.arange(c.M).view(1, -1, 1)
    ci = torch.arange(c.Cin).view(1, 1, -1)
    Wk = o["wview"][d * o["wv"].sT + m * o["wv"].sO + ci * o["wv"].sI]
    acc = torch.zeros(c.N, c.M, c.T, W)
    for k in reversed(range(K)):
        for cc in reversed(range(c.Cin)):
            acc = acc + Wk[k, :, cc].view(1, -1, 1, 1) * xa32[:, k, cc].unsqueeze(1)
    if "add" in o:
        acc = acc + (o["add"] if c.add == 0 else o["add"][:, :, ::c.add][:, :, :c.T])
    if c.label:
        L, J, labels = c.label
        bias = ad.label_bias_f64(o["A"].float(), o["wfull"], c.Cin + J, J, c.M, o["emb"], o["labels"]).float()
        acc = acc + bias
    assert ad.worst_ratio(acc, ref, S, c.n(o["pcount"]), c.b) <= 1.0
    assert ad.worst_ratio(xa32.reshape(xa.shape), xa, Sxa, max(o["pcount"]), ad.B_EXPAND) <= 1.0


# ---- mutation check --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FLOAT_AGG, ids=[c.name for c in FLOAT_AGG])
def test_one_wrong_term_falls_outside_the_bracket(c):
    """a condition on the INPUTS of the float cases (few enough products, these seeds), not a tolerance"""
    o = c.operands(SEED, False)
    ref, S = c.reference(o, False)
    muts = c.mutations(o, ad.MUTATION_SEED.get(c.name, SEED))
    assert len(muts) == (3 if c.res is not None else 2)
    for mut in muts:
        bad, _ = c.reference(o, False, mutate=mut)
        assert ad.worst_ratio(bad, ref, S, c.n, c.b) > 1.0, (c.name, mut)


@pytest.mark.parametrize("c", ad.CONV_CASES, ids=[c.name for c in ad.CONV_CASES])
def test_aggconv_one_wrong_term_falls_outside_the_bracket(c):
    o = c.operands(SEED, False)
    ref, _, S, _ = c.reference(o, False)
    for mut in c.mutations(o, ad.MUTATION_SEED.get(c.name, SEED)):
        bad = c.reference(o, False, mutate=mut)[0]
        assert ad.worst_ratio(bad, ref, S, c.n(o["pcount"]), c.b) > 1.0, (c.name, mut)


# ---- the plans of the GPU tests' launches (host code only) ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return nv.load_library()


def _strides(layout, N, C, T, V):
    """(sN, sC) of a (N, C, T, V) tensor stored channel-major or NCHW"""
    return (T * V, N * T * V) if layout == "plane" else (C * T * V, T * V)


def agg_args(c):
    """KgAggArgs of a case without tensors: what the plan looks at (outputs are channel-major planes, as the binding makes them)"""
    a = nv._AggArgs()
    a.N, a.C, a.K, a.V, a.W, a.T, a.rep = c.N, c.C, c.K, c.V, c.W, c.T, c.rep
    a.a = a.x = a.out = 0x1000
    if c.op == "expand":
        a.x_sN, a.x_sC = _strides(c.layout, c.N, c.C, c.T, c.V)
        a.o_sN, a.o_sC = _strides("plane", c.N, c.K * c.C, c.T * c.rep, c.W)
    elif c.op == "reduce":
        a.x_sN, a.x_sC = _strides(c.layout, c.N, c.K * c.C, c.T * c.rep, c.V)
        a.o_sN, a.o_sC = _strides("plane", c.N, c.C, c.T, c.W)
        if c.res is not None:
            s, drop = c.res
            a.res, a.r_T, a.r_V, a.r_tstride = 0x2000, -(-c.T // s), ad.res_inv(c.W, drop)[1], s
            a.r_inv = 0x3000 if drop else None
            a.r_sN, a.r_sC = _strides(c.layout, c.N, c.C, a.r_T, a.r_V)
        if c.mask:
            a.mask = 0x4000
            a.m_sN, a.m_sC = _strides(c.layout, c.N, c.C, c.T, c.W)
    else:
        a.y = a.ws = 0x5000
        a.x_sN, a.x_sC = _strides(c.layout, c.N, c.C, c.T, c.V)
        a.y_sN, a.y_sC = _strides(c.layout, c.N, c.K * c.C, c.T * c.rep, c.W)
    return a


OPS = {"expand": nv.AGG_OP_EXPAND, "reduce": nv.AGG_OP_REDUCE, "outer": nv.AGG_OP_OUTER}


def plan_agg(lib, c, env):
    try:
        for k, v in c.env.items():
            env.setenv(k, v)
        p = nv._AggPlanInfo()
        assert lib.kg_agg_plan_info(ctypes.byref(agg_args(c)), OPS[c.op], ctypes.byref(p)) == 0, lib.kg_last_error()
    finally:
        env.undo()
    return nv.plan_dict(p)


def conv_args(c):
    K, V, W = c.dims()
    a = nv._AggConvArgs()
    a.N, a.Cin, a.M, a.T, a.V, a.W, a.K = c.N, c.Cin, c.M, c.T, V, W, K
    a.x_sN, a.x_sC = _strides(c.layout, c.N, c.Cin, c.T, V)
    _, pcount = ad.nbr_table(c.pat())
    for i in range(3):
        a.pcount[i] = pcount[i] if i < K else 0
    ctot = c.Cin + c.cc + (c.label[1] if c.label else 0)
    a.w_sT, a.w_sO, a.w_sI = c.M * ctot, ctot, 1
    a.o_sN, a.o_sC = _strides("plane", c.N, c.M, c.T, W)
    a.add = 0x1000 if c.add is not None else None
    a.xa = 0x2000 if c.xa else None
    a.xa_sN, a.xa_sC = _strides("plane", c.N, K * c.Cin, c.T, W)
    return a


def plan_conv(lib, c, env):
    try:
        for k, v in c.env.items():
            env.setenv(k, v)
        p = nv._AggConvPlanInfo()
        assert lib.kg_aggconv_plan_info(ctypes.byref(conv_args(c)), c.label[1] if c.label else 0, ctypes.byref(p)) == 0, lib.kg_last_error()
    finally:
        env.undo()
    return nv.plan_dict(p)


def check_expect(c, p):
    bad = {k: (v, p[k]) for k, v in c.expect.items() if p[k] != v}
    assert not bad, "%s: (expected, planned) differ at %s" % (c.name, bad)


def test_form_numbers_are_the_headers():
    assert (nv.AGG_FORM_FRAME, nv.AGG_FORM_STREAM, nv.AGG_FORM_MFMA, nv.AGG_FORM_OUTER_ELEM, nv.AGG_FORM_OUTER_MFMA) == (
        ad.FRAME, ad.STREAM, ad.MFMA, ad.OUTER_ELEM, ad.OUTER_MFMA) and nv.AGG_FORM_NAMES == ad.FORM_NAMES and nv.AGGCONV_P == ad.PMAX


@pytest.mark.parametrize("c", ad.AGG_CASES, ids=[c.name for c in ad.AGG_CASES])
def test_agg_launches_are_planned_as_named(c, lib, monkeypatch):
    p = plan_agg(lib, c, ReloadingEnv(monkeypatch))
    check_expect(c, p)
    assert c.expect and ("ineligible" in c.name or ad.FORM_NAMES[p["form"]].replace("-", " ") in c.name)
    if p["form"] == ad.STREAM:                 # more than one workgroup per channel, the last one ragged
        rows = c.N * c.T * (c.rep if c.op == "expand" else 1)
        assert p["grid_x"] >= 2 and rows % p["FO"] != 0
    if p["form"] == ad.MFMA:                   # two or more tiles per channel with a ragged last tile; LDS as the kernel lays it out
        KI, KO = p["KI"], p["KO"]
        assert p["tiles_per_c"] >= 1 and p["ntiles"] == p["tiles_per_c"] * c.C and p["SUB"] * c.V <= 32
        assert p["lds_bytes"] == p["SUB"] * 128 * (KI * c.V + KO * c.W) * 4 <= 61440 and p["grid_x"] <= p["ntiles"]
        assert (c.N * c.T) % (128 * p["SUB"]) != 0
    if p["form"] == ad.OUTER_MFMA:
        assert p["F"] % (16 * p["P"]) == 0 and p["units"] == c.C * p["chunks"] and p["slabs"] == min(p["units"], 512) == p["grid_x"]
        assert p["lds_bytes"] <= 65536


def test_agg_cases_reach_every_instantiation(lib, monkeypatch):
    env = ReloadingEnv(monkeypatch)
    seen = {ad.instantiation(c.op, plan_agg(lib, c, env)) for c in ad.AGG_CASES}
    assert seen == ad.AGG_INSTANTIATIONS, (sorted(ad.AGG_INSTANTIATIONS - seen), sorted(seen - ad.AGG_INSTANTIATIONS))
    # and the properties section by section: every forced sub-tile count, a persistent loop with a ragged last round,
    # every P of the outer geometry, a short last chunk, fewer workgroups than units
    plans = {c.name: plan_agg(lib, c, env) for c in ad.AGG_CASES}
    mf = [p for p in plans.values() if p["form"] == ad.MFMA]
    assert {p["SUB"] for p in mf} == {1, 2, 3, 4, 6, 8}
    assert any(p["grid_x"] < p["ntiles"] and p["ntiles"] % p["grid_x"] for p in mf)
    om = [(ad.AGG[n], p) for n, p in plans.items() if p["form"] == ad.OUTER_MFMA]
    assert {p["P"] for _, p in om} == {16, 8, 3, 1}
    assert any(p["chunks"] > 1 and (c.N * c.T) % p["F"] for c, p in om)
    assert any(p["slabs"] < p["units"] for _, p in om) and any(p["slabs"] < p["units"] for p in plans.values() if p["form"] == ad.OUTER_ELEM)


def test_a_case_moved_off_its_form_fails(lib, monkeypatch):
    """the check above has teeth: the same case under another switch is reported as another form"""
    c = ad.AGG["mfma reduce SUB3 V5 485 frames"]
    p = plan_agg(lib, c._replace(env={"KG_AGG_MFMA": "0", "KG_AGG_STREAM": "0"}), ReloadingEnv(monkeypatch))
    with pytest.raises(AssertionError, match="differ at"):
        check_expect(c, p)


@pytest.mark.parametrize("c", ad.CONV_CASES, ids=[c.name for c in ad.CONV_CASES])
def test_aggconv_launches_are_planned_as_named(c, lib, monkeypatch):
    p = plan_conv(lib, c, ReloadingEnv(monkeypatch))
    check_expect(c, p)
    K, V, W = c.dims()
    if p["tiny"]:
        assert p["grid_x"] == c.N * -(-(c.T * W) // (256 // p["RG"])) and (c.T * W) % (256 // p["RG"]) != 0
        assert p["lds_bytes"] == 4 * (((K * V * W + 3) & ~3) + (K * c.M * c.label[1] + c.label[1] if c.label else 0))
    else:
        span = (127 // W + 2) * V
        assert p["spanp"] == (span + 3) // 4 * 4 <= 384 and (p["XE"] == 6) == (p["spanp"] > 192)
        assert p["tapmask"] == sum(1 << k for k in range(K) if ad.nbr_table(c.pat())[1][k] > 0)
        assert (p["grid_x"], p["grid_y"]) == (-(-(c.N * c.T * W) // 128), -(-c.M // p["BM"]))
        assert p["ADD"] == int(c.add is not None or c.M % p["BM"] != 0)


def test_aggconv_cases_reach_every_instantiation(lib, monkeypatch):
    env = ReloadingEnv(monkeypatch)
    plans = {c.name: plan_conv(lib, c, env) for c in ad.CONV_CASES}
    seen = {ad.conv_instantiation(p) for p in plans.values()}
    assert seen == ad.CONV_INSTANTIATIONS, (sorted(ad.CONV_INSTANTIATIONS - seen), sorted(seen - ad.CONV_INSTANTIATIONS))
    tiles = [(ad.CONV[n], p) for n, p in plans.items() if not p["tiny"]]
    assert {c.M for c, _ in tiles} >= {32, 33, 64, 70, 96, 128} and {c.Cin for c, _ in tiles} >= {3, 16, 20, 40}
    assert any(p["tapmask"] != 7 for _, p in tiles) and any(c.cc for c, _ in tiles)
    assert any(p["grid_y"] == 2 and c.M % p["BM"] for c, p in tiles) and any(p["grid_x"] > 1 for _, p in tiles)
    assert {c.dims()[2] for c in ad.CONV_CASES} >= {1, 7, 11, 25}


def many_args(m):
    return (nv._AggArgs * len(m.jobs))(*[agg_args(j) for j in m.jobs])


@pytest.mark.parametrize("name", list(ad.MANY))
def test_outer_many_launches_are_planned_as_named(name, lib, monkeypatch):
    m = ad.MANY[name]
    env = ReloadingEnv(monkeypatch)
    n = len(m.jobs)
    la, ns = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
    try:
        for k, v in m.env.items():
            env.setenv(k, v)
        assert lib.kg_agg_outer_many_plan(many_args(m), n, la, ns) == 0, lib.kg_last_error()
        singles = [plan_agg(lib, j._replace(env=m.env), ReloadingEnv(monkeypatch)) for j in m.jobs]
        for k, v in m.env.items():
            env.setenv(k, v)
    finally:
        env.undo()
    assert list(la) == m.launch
    for i, (p, s) in enumerate(zip(singles, ns)):
        assert (p["form"] == ad.OUTER_MFMA) == (la[i] >= 0) and 1 <= s <= p["slabs"]
    if name == "budget 6":
        assert singles[2]["units"] == 80 and ns[2] < 80 and ns[0] == 1 and singles[0]["units"] > 1 and sum(
            s for s, l in zip(ns, la) if l >= 0) <= 6 + n
    else:
        assert list(ns) == [p["slabs"] for p in singles]          # the default budget cuts nothing at these sizes


# ---- the default rules at the bench configurations --------------------------------------------------------------------------
# the critic's six blocks (discriminator.py): Cin, M, level, kept columns only, frames as a fraction of t_size
D_BLOCKS = [(3, 32, 0, True, 1), (32, 64, 1, False, 1), (64, 128, 1, True, 1), (128, 256, 2, False, 2), (256, 512, 2, True, 4), (512, 512, 3, False, 8)]
T_SIZE = {"ntu": 64, "h36m": 32}


def bench_plans(lib, ds, n):
    """per block: the fused forward launch (kg_aggconv with the aggregated planes, or kg_agg_expand where the fused kernel
    does not take the launch), the adjoint aggregation of the backward pass (kg_agg_reduce with A^T) and the adjacency
    gradient (kg_agg_outer) - unforced"""
    out = []
    for i, (cin, m, lvl, kept, tdiv) in enumerate(D_BLOCKS):
        pat = ad.graph_pattern(ds, lvl, kept)
        K, V, W = pat.shape
        T = T_SIZE[ds] // tdiv
        cin = cin if i else {"ntu": 3, "h36m": 2}[ds]
        _, pcount = ad.nbr_table(pat)
        if nv.aggconv_supported(V, W, pcount, n * T * W):
            c = ad.Conv("D%d" % i, (ds, lvl, kept), n, cin, m, T, xa=True)
            p = nv._AggConvPlanInfo()
            assert lib.kg_aggconv_plan_info(ctypes.byref(conv_args(c)), 0, ctypes.byref(p)) == 0, lib.kg_last_error()
            fwd = ad.conv_instantiation(nv.plan_dict(p))
        else:
            p = nv._AggPlanInfo()
            c = ad.Agg("D%d" % i, "expand", n, cin, T, V, W, K)
            assert lib.kg_agg_plan_info(ctypes.byref(agg_args(c)), OPS["expand"], ctypes.byref(p)) == 0, lib.kg_last_error()
            fwd = ad.instantiation("expand", nv.plan_dict(p))
        r, o = nv._AggPlanInfo(), nv._AggPlanInfo()
        adj = ad.Agg("D%d adjoint" % i, "reduce", n, cin, T, W, V, K)
        assert lib.kg_agg_plan_info(ctypes.byref(agg_args(adj)), OPS["reduce"], ctypes.byref(r)) == 0, lib.kg_last_error()
        da = ad.Agg("D%d dA" % i, "outer", n, cin, T, V, W, K)
        assert lib.kg_agg_plan_info(ctypes.byref(agg_args(da)), OPS["outer"], ctypes.byref(o)) == 0, lib.kg_last_error()
        r, o = nv.plan_dict(r), nv.plan_dict(o)
        out.append((fwd, ad.instantiation("reduce", r) + ((r["SUB"], r["grid_x"]) if r["form"] == ad.MFMA else ()),
                    ad.instantiation("outer", o) + (o["P"], o["F"], o["slabs"])))
    return out


# per block D0 .. D5: (forward launch, adjoint reduce + (SUB, grid) on the matrix cores, adjacency gradient + (P, F, slabs))
BENCH_PLANS = {('h36m', 64): [(('tiny', 32, 4, 0), ('frame', 'reduce', 3, 16), ('outer-mfma', 3, 1, 1, 1, 128, 32)),
                (('tile', 32, 1, 3, 1, 0), ('frame', 'reduce', 3, 8), ('outer-mfma', 3, 1, 1, 2, 256, 256)),
                (('frame', 'expand', 3, 4), ('stream', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 2, 288, 512)),
                (('frame', 'expand', 3, 4), ('frame', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 8, 896, 256)),
                (('frame', 'expand', 3, 4), ('stream', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 8, 512, 256)),
                (('frame', 'expand', 3, 4), ('frame', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 16, 256, 512))],
 ('h36m', 192): [(('tiny', 32, 4, 0), ('mfma', 3, 1, 17, 0, 0, 1, 96), ('outer-mfma', 3, 1, 1, 1, 128, 96)),
                 (('tile', 32, 1, 3, 1, 0), ('frame', 'reduce', 3, 8), ('outer-mfma', 3, 1, 1, 2, 256, 512)),
                 (('frame', 'expand', 3, 4), ('stream', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 2, 288, 512)),
                 (('frame', 'expand', 3, 4), ('frame', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 8, 896, 512)),
                 (('frame', 'expand', 3, 4), ('stream', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 8, 1024, 512)),
                 (('frame', 'expand', 3, 4), ('frame', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 16, 768, 512))],
 ('ntu', 64): [(('tiny', 32, 4, 0), ('mfma', 3, 1, 17, 0, 0, 1, 96), ('outer-mfma', 3, 2, 1, 1, 80, 156)),
               (('tile', 32, 1, 3, 1, 0), ('mfma', 3, 1, 17, 0, 0, 1, 512), ('outer-mfma', 3, 1, 1, 1, 160, 512)),
               (('tile', 32, 1, 6, 1, 0), ('mfma', 3, 1, 8, 0, 0, 2, 768), ('outer-mfma', 3, 1, 1, 1, 176, 512)),
               (('tile', 32, 1, 3, 1, 0), ('frame', 'reduce', 3, 8), ('outer-mfma', 3, 1, 1, 3, 384, 512)),
               (('frame', 'expand', 3, 4), ('stream', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 3, 384, 512)),
               (('frame', 'expand', 3, 4), ('frame', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 16, 512, 512))],
 ('ntu', 192): [(('tiny', 32, 1, 0), ('mfma', 3, 1, 17, 0, 0, 1, 288), ('outer-mfma', 3, 2, 1, 1, 80, 462)),
                (('tile', 64, 1, 3, 1, 0), ('mfma', 3, 1, 17, 0, 0, 2, 512), ('outer-mfma', 3, 1, 1, 1, 160, 512)),
                (('tile', 64, 2, 6, 1, 0), ('mfma', 3, 1, 8, 0, 0, 4, 768), ('outer-mfma', 3, 1, 1, 1, 176, 512)),
                (('tile', 64, 2, 3, 1, 0), ('frame', 'reduce', 3, 8), ('outer-mfma', 3, 1, 1, 3, 384, 512)),
                (('frame', 'expand', 3, 4), ('stream', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 3, 384, 512)),
                (('frame', 'expand', 3, 4), ('frame', 'reduce', 3, 4), ('outer-mfma', 3, 1, 1, 16, 1536, 512))]}


@pytest.mark.parametrize("ds,n", [("ntu", 64), ("ntu", 192), ("h36m", 64), ("h36m", 192)])
def test_default_plans_at_the_bench_configurations(ds, n, lib):
    """what the default rules give, unforced: a retuning shows here (and must then update this table on purpose)"""
    assert bench_plans(lib, ds, n) == BENCH_PLANS[(ds, n)]
