"""CPU: tests/genblock_def.py can be trusted before a GPU is involved, and the launch tables of
tests/test_genblock_forms_gpu.py land on the kernel forms they are named after.

  * the float64 definition against autograd through an independent float64 torch composition (conv2d / einsum /
    batch_norm): the forward values, the BatchNorm coefficients and running statistics, and every backward output;
  * teeth: the definition with the taps flipped, the frame repeat off by one, the partitions swapped, the residual bias
    dropped, the biased variance averaged into the running statistics, the pending tail's coefficient row of the wrong batch,
    or one zero-filled ragged-K term kept falls outside the bracket on the float data of a table case - a kernel that is wrong
    by that much cannot pass - while the definition rounded to fp32 lies inside it;
  * every launch of both tables is planned on the host (kg_genblock_form: no GPU) onto the instantiation and contraction
    paths it names, the refusals are refused, Table A reaches every entry of genblock_def.INSTANTIATIONS and no other, and
    the compile-time forms resolve the paths the layout chooses;
  * the eligibility answers of the library agree with oracle/prim_ref.py, in sign and value, on 2400 seeded dimension tuples.
"""
import ctypes
import os
import random
import re

import pytest
import torch
import torch.nn.functional as TF

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from oracle import prim_ref as pr
from tests import genblock_def as gd
from tests.util import ReloadingEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = gd.DATA_SEED
PTR = 1 << 20              # (never dereferenced)


@pytest.fixture
def monkeypatch(monkeypatch):
    env = ReloadingEnv(monkeypatch)
    yield env
    env.undo()


@pytest.fixture(scope="module")
def lib():
    return nv.load_library()


def dims_of(c):
    return nv.GenBlockDims(Cin=c.Cin, C=c.C, K=c.K, Kp=c.Kp, Tc=c.Tc, Vc=c.Vc, T=c.T, V=c.V, rep=c.rep, res_kind=c.res, bn_t=bool(c.bn_t),
                           act=c.act)


# ---- the definition against autograd -----------------------------------------------------------------------------------------
AUTOGRAD_CASES = [gd.Case("auto-conv", 4, 2, 6, 5, 3, 3, 3, 5, 2, 2, 1), gd.Case("auto-identity", 3, 1, 4, 4, 2, 2, 4, 4, 3, 1, 1, act=gd.ACT_TANH)]


def torch_act(v, act, slope):
    return TF.leaky_relu(v, slope) if act == gd.ACT_LRELU else torch.tanh(v) if act == gd.ACT_TANH else v


def compose(c, o, x):
    """the block's stages up to u and r with stock torch ops, float64, autograd on"""
    Wh = torch.cat([o["wg"].double()[:c.Mg], o["wr"].double()]) if c.res == 2 else o["wg"].double()[:c.Mg]
    yc = TF.conv2d(x, Wh.view(c.Mh, c.Cin, 1, 1))
    B = o["B"].double().requires_grad_()
    z = torch.zeros(c.N, c.C, c.Tc, c.V, dtype=torch.float64)
    for k in range(c.Kp):
        z = z + torch.matmul(yc[:, k * c.C:(k + 1) * c.C], B[k])
    z = z.repeat_interleave(c.rep, dim=2)
    r = None
    if c.res != 0:
        src = yc[:, c.Mg:] if c.res == 2 else x
        r = torch.matmul(src, o["U"].double()) if "U" in o else src
        if c.res == 2:
            r = r + o["br"].double().view(1, -1, 1, 1)
        r = r.repeat_interleave(c.rep, dim=2)
    u = TF.conv2d(z, o["wt"].double().view(c.C, c.C, 3, 1), o["bt"].double(), padding=(1, 0))
    return yc, z, r, u, B


def close64(a, b, what, tol=1e-11):
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), "%s: %g" % (what, err)


@pytest.mark.parametrize("c", AUTOGRAD_CASES, ids=lambda c: c.name)
def test_definition_against_autograd(c):
    o = gd.operands(c, "fwd", 11, False)
    x = o["x"].double().requires_grad_()
    yc, z, r, u, B = compose(c, o, x)
    ref, _, _ = gd.forward(c, o, "fwd", gd.SLOPE_FLOAT, c.act)
    for k, v in (("yc", yc), ("z", z), ("r", r), ("u", u)):
        if v is not None:
            close64(ref[k], v.detach(), k)
    # BatchNorm: torch's training-mode batch_norm per batch, running statistics updated in order
    h = c.N // c.groups
    for key, src in (("t", u), ("r", r)):
        if "bn_" + key not in o:
            continue
        L = o["bn_" + key]
        rm, rv = L["running_mean"].double().clone(), L["running_var"].double().clone()
        for g in range(c.groups):
            xs = src.detach()[g * h:(g + 1) * h]
            y = TF.batch_norm(xs, rm, rv, L["gamma"].double(), L["beta"].double(), True, L["momentum"], L["eps"])
            cf = ref["c" + key][g]
            close64(xs * cf[0].view(1, -1, 1, 1) + cf[1].view(1, -1, 1, 1), y, "bn %s batch %d" % (key, g))
            close64(cf[2], xs.mean((0, 2, 3)), "mean")
            close64(cf[3], torch.rsqrt(xs.var((0, 2, 3), unbiased=False) + L["eps"]), "rstd")
        close64(ref["rm_" + key], rm, "running_mean")
        close64(ref["rv_" + key], rv, "running_var")
    # backward chain: du / dr of the definition as cotangents of u / r
    ob = gd.operands(c, "bwd", 12, False)
    ob.update({k: o[k] for k in ("wg", "wr", "br", "wt", "bt", "B", "U") if k in o})
    bref, _, _ = gd.backward(c, ob, "bwd", gd.SLOPE_FLOAT)
    outs, cts = [u], [bref["du"]]
    if r is not None:
        outs.append(r)
        cts.append(bref["dr"])
    gx, gyc, gz, gB = torch.autograd.grad(outs, [x, yc, z, B], cts)
    close64(bref["gx"], gx, "gx")
    close64(bref["gyc"], gyc, "gyc")
    close64(bref["zf"], gz.reshape(c.N, c.C, c.Tc, c.rep, c.V).sum(3), "zf")
    # zf is the adjacency gradient's operand: d B_k[vc, w] = sum zf[c, (., w)] yc[k C + c, (., vc)]
    close64(torch.einsum("nctw,nkctv->kvw", bref["zf"], yc.detach()[:, :c.Mg].reshape(c.N, c.Kp, c.C, c.Tc, c.Vc)), gB, "dB from zf")


@pytest.mark.parametrize("act", [gd.ACT_LRELU, gd.ACT_TANH])
def test_tail_backward_against_autograd(act):
    """du / dr, the tail coefficients and the parameter gradients: out = act(BN_t(u) + BN_r(r) + nw noise) differentiated by
    autograd against prev_stats (the coefficients) followed by backward's stage 0 (their application)"""
    N, C, T, V = 3, 5, 4, 3
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)          # noqa: E731
    u, r = (rnd(N, C, T, V) * 1.5 + 0.3).requires_grad_(), rnd(N, C, T, V).requires_grad_()
    gam_t, bet_t, gam_r, bet_r, nw = [(rnd(C) + 2.0).requires_grad_() for _ in range(5)]
    noise, g = rnd(N, 1, T, V), rnd(N, C, T, V)
    eps = 1e-5
    out = torch_act(TF.batch_norm(u, None, None, gam_t, bet_t, True, 0.1, eps) + TF.batch_norm(r, None, None, gam_r, bet_r, True, 0.1, eps)
                    + nw.view(1, -1, 1, 1) * noise, act, 0.2)
    du, dr, dgt, dbt, dgr, dbr, dnw = torch.autograd.grad(out, [u, r, gam_t, bet_t, gam_r, bet_r, nw], g)
    # the tail as the "previous block" of a (Cin = C, Tc = T, Vc = V) case
    c = gd.Case("tail", N, 1, C, C, 1, T, V, V, 1, 1, 0, act=act)
    st = lambda x, gam: (gam.detach(), x.detach().mean((0, 2, 3)), torch.rsqrt(x.detach().var((0, 2, 3), unbiased=False) + eps))   # noqa: E731
    zero = {k: torch.zeros(C, dtype=torch.float64) for k in ("gamma_t", "beta_t", "gamma_r", "beta_r", "nw")}
    o = dict(prev=dict(x=out.detach(), act=act, u=u.detach(), r=r.detach(), noise=noise, bn_t=st(u, gam_t), bn_r=st(r, gam_r), sinks=zero))
    res = gd.prev_stats(c, o, g, 0.2, gd.Exact())
    for k, want in (("sink_gamma_t", dgt), ("sink_beta_t", dbt), ("sink_gamma_r", dgr), ("sink_beta_r", dbr), ("sink_nw", dnw)):
        close64(res[k][0], want, k, 1e-10)
    # ... and applied by backward's stage 0 (a conv-residual block with BatchNorm on both branches)
    c2 = gd.Case("apply", N, 1, C, C, 1, T, V, V, 1, 2, 1, act=act)
    o2 = gd.operands(c2, "bwd", 3, False)
    o2.update(g=g, out=out.detach(), u=u.detach(), r=r.detach(), coef=res["pcoef"][0])
    bref, _, _ = gd.backward(c2, o2, "bwd", 0.2)
    close64(bref["du"], du, "du", 1e-10)
    close64(bref["dr"], dr, "dr", 1e-10)


# ---- teeth -------------------------------------------------------------------------------------------------------------------
def as_kernel(ref):
    """the definition's chain rounded to fp32: what a correct kernel could return"""
    return {k: v.float() for k, v in ref.items()}


def worst(c, o, kind, got):
    ref, br = gd.reference(c, o, kind, False, got=got)
    return max(gd.worst_ratio(got[k], ref[k], br[k]) for k in ref)


TEETH = [  # mutation, table case, launch kind
    ("tapflip", "g1-N4g2", "fwd"), ("tapflip", "tcn-c16-nf70", "infer"),
    ("repeat", "g0-N4g2", "fwd"), ("repeat", "tcn-c16-nf70", "infer"),
    ("kswap", "g2-N4g2", "fwd"), ("kswap", "v32", "infer"),
    ("nobias", "g4-N4g2", "fwd"), ("nobias", "cols64-m12", "infer"),
    ("biased", "g0-N4g2", "fwd"), ("biased", "groups4-N4", "fwd"),
    ("grouprow", "g0-N4g2", "pend"), ("grouprow", "groups4-N8", "pend"),
    ("ragged", "at-mh20", "bwd"), ("ragged", "at-mh3", "bwdprev"), ("ragged", "g3-N5g1", "bwd"),
]


@pytest.mark.parametrize("mutation,name,kind", TEETH)
def test_teeth(mutation, name, kind):
    c = gd.CASES[name]
    assert kind in c.kinds
    o = gd.operands(c, kind, SEED, False)
    good, _ = gd.reference(c, o, kind, False)
    assert worst(c, o, kind, as_kernel(good)) <= 1.0, "the definition rounded to fp32 must lie inside its own bracket"
    bad, _ = gd.reference(c, o, kind, False, mutate=mutation)
    assert worst(c, o, kind, as_kernel(bad)) > 1.0, "%s on %s %s stays inside the bracket" % (mutation, name, kind)


@pytest.mark.parametrize("name,kind", gd.launches(gd.TABLE_A + gd.TABLE_B))
def test_data_is_exact_and_inside_its_bracket(name, kind):
    """every launch of both tables: the integer data is exact (the module asserts 16 S < 2^24 and every value is a multiple of 2^-4
    that fp32 holds), and on float data the definition rounded to fp32 lies inside the bracket built from it"""
    c = gd.CASES[name]
    o = gd.operands(c, kind, 21, True)
    ref, _ = gd.reference(c, o, kind, True)
    for k, v in ref.items():
        if k not in gd.BRACKETED_ON_INTEGERS and not k.startswith("sink"):
            assert bool((v.float().double() == v).all()) and bool((v * 16 == (v * 16).round()).all()), (name, kind, k)
    o = gd.operands(c, kind, SEED, False)
    ref, _ = gd.reference(c, o, kind, False)
    assert worst(c, o, kind, as_kernel(ref)) <= 1.0


# ---- planning ---------------------------------------------------------------------------------------------------------------
def plan(c, kind, lib=None):
    d = gd.DIR_OF[kind]
    return nv.genblock_form(dims_of(c), c.N, d, groups=c.groups if d == "fwd" else 1, prev=kind == "bwdprev")


def test_geometries_are_the_kernel_files():
    src = open(os.path.join(ROOT, "kinetic-gan_amd", "csrc", "kg_genblock.hip")).read()
    body = src[src.index("#define GB_GEOMETRIES(X)"):src.index("template <typename G>\nbool geo_matches")]
    geos = [tuple(int(v) for v in m.split(",")) for m in re.findall(r"X\(([^)]*\d)\)", body)]
    assert geos == gd.GEOMETRIES
    assert len(gd.INSTANTIATIONS) == 3 * (len(geos) + 1) and len(set(gd.INSTANTIATIONS)) == len(gd.INSTANTIATIONS)
    assert sorted(gd.INSTANTIATIONS) == sorted((d, g) for d in ("fwd", "bwd", "infer") for g in range(-1, len(geos)))


def test_table_a_reaches_every_instantiation(monkeypatch):
    reached = set()
    for rt in (False, True):
        if rt:
            monkeypatch.setenv("KG_GB_RT", "1")
        for c in gd.TABLE_A:
            gi = c.geometry()
            assert gi >= 0, c.name
            for kind in c.kinds:
                f = plan(c, kind)
                d = gd.DIR_OF[kind]
                want = dict(gd.paths(c, d), geometry=-1 if rt else gi, grid_x=c.N)
                assert {k: f[k] for k in want} == want and f["lds_bytes"] > 0, (c.name, kind, rt, f)
                reached.add((d, f["geometry"]))
    assert reached == set(gd.INSTANTIATIONS)


def test_compile_time_forms_resolve_the_layouts_paths(monkeypatch):
    """the path a GbGeo kernel resolves from its constants (reported for the compile-time forms) is the layout's (the
    run-time form's) for all six geometries and every direction"""
    for c in gd.TABLE_A:
        for kind in c.kinds:
            monkeypatch.delenv("KG_GB_RT", raising=False)
            ct = plan(c, kind)
            monkeypatch.setenv("KG_GB_RT", "1")
            rt = plan(c, kind)
            assert ct["geometry"] >= 0 and rt["geometry"] == -1
            assert all(ct[k] == rt[k] for k in ("mfma0", "mfma1", "mv0", "mv1", "lds_bytes", "grid_x")), (c.name, kind, ct, rt)


@pytest.mark.parametrize("name", [c.name for c in gd.TABLE_B])
def test_table_b_plans(name, monkeypatch, lib):
    c = gd.CASES[name]
    monkeypatch.setenv("KG_GB_RT", "1")
    for kind in c.kinds:
        d = gd.DIR_OF[kind]
        f = plan(c, kind)
        want = dict(gd.paths(c, d), geometry=-1, grid_x=c.N)
        want.update((c.expect or {}).get(d, {}))
        assert {k: f[k] for k in want} == want and f["lds_bytes"] > 0, (name, kind, f)
    for what in c.reject:
        if what == "dims":
            with pytest.raises(RuntimeError, match="exceed 32 vertices"):
                plan(c, "fwd")
        else:
            assert plan(c, what)["lds_bytes"] == -1, (name, what)
    if name.startswith("lds-") and name.endswith("under"):
        assert max(plan(c, k)["lds_bytes"] for k in c.kinds) > 140 * 1024
    assert c.kinds or c.reject


def test_launchers_refuse_what_the_form_query_refuses(lib):
    """the refused cases of Table B at the launchers themselves (they return before anything touches a device): the error
    code, with the message of the rule the case is named after"""
    messages = {"depth68-m20-refused": b"does not fit", "rows33-ragged-refused": b"does not fit", "tcn-c22-refused": b"does not fit",
                "merge-area-over": b"do not fit the merge area", "statrows-544-refused": b"does not fit", "v33-error": b"exceed 32 vertices",
                "prev-cols528-refused": b"Tc * Vc <= 512", "prev-cin528-refused": b"Cin <= 512", "lds-fwd-over": b"does not fit",
                "lds-bwd-over": b"does not fit"}
    assert sorted(messages) == sorted(c.name for c in gd.TABLE_B if c.reject)
    for name, msg in messages.items():
        c = gd.CASES[name]
        d = dims_of(c)
        for what in c.reject:
            if what in ("fwd", "dims"):
                a = nv._GenBlockArgs()
                a.N, a.groups = c.N, c.groups
                nv._gb_common(a, d, 0.2)
                a.wg, a.wr, a.wt = PTR, PTR, PTR
                assert lib.kg_genblock_lds_bytes(ctypes.byref(a)) < 0 or name == "merge-area-over"
                rc = lib.kg_genblock_fwd(ctypes.byref(a), None)
            elif what == "infer":
                a = nv._GenBlockInferArgs()
                a.N = c.N
                nv._gb_infer_dims(a, d, 0.2)
                a.wg, a.wr, a.wt = PTR, PTR, PTR
                rc = lib.kg_genblock_infer(ctypes.byref(a), None)
            else:
                a = nv._GenBlockBwdArgs()
                a.N = c.N
                nv._gb_common(a, d, 0.2)
                for fld in ("wg", "wr", "wt", "b", "u", "coef"):
                    setattr(a, fld, PTR)
                for fld in ("g", "out", "uo", "r", "du", "dr", "gyc", "zf", "gx") + (("px",) if what == "bwdprev" else ()):
                    getattr(a, fld).p = PTR
                rc = lib.kg_genblock_bwd(ctypes.byref(a), None)
            assert rc < 0 and msg in lib.kg_last_error(), (name, what, rc, lib.kg_last_error())


def test_refusals_sit_next_to_an_accepted_neighbour():
    """each refused case differs from an accepted one of the table in one dimension only (the edge is where the table says)"""
    pairs = [("depth60-m32", "depth68-m20-refused"), ("tcn-c21-edge", "tcn-c22-refused"), ("merge-area-2048", "merge-area-over"),
             ("statrows-512", "statrows-544-refused"), ("prev-cols512", "prev-cols528-refused"), ("prev-cin512", "prev-cin528-refused"),
             ("lds-fwd-under", "lds-fwd-over"), ("lds-bwd-under", "lds-bwd-over"), ("v32", "v33-error")]
    for a, b in pairs:
        assert gd.CASES[a].kinds and not gd.CASES[b].kinds and gd.CASES[b].reject


def test_form_query_validates_without_gpu(lib):
    from tests import abi_layout
    for cname in ("KgGenBlockFormQuery", "KgGenBlockForm"):          # the mirrors have the header's layout (tests/test_abi_cpu.py too)
        assert cname in abi_layout.header_structs()
        abi_layout.assert_mirror(cname)
    q, f = nv._GenBlockFormQuery(), nv._GenBlockForm()
    assert lib.kg_genblock_form(None, ctypes.byref(f)) < 0 and b"null query" in lib.kg_last_error()
    assert lib.kg_genblock_form(ctypes.byref(q), None) < 0 and b"null output" in lib.kg_last_error()
    assert lib.kg_genblock_form(ctypes.byref(q), ctypes.byref(f)) < 0 and b"bad dims" in lib.kg_last_error()
    q.dir = 7
    assert lib.kg_genblock_form(ctypes.byref(q), ctypes.byref(f)) < 0 and b"dir=7" in lib.kg_last_error()
    assert nv.last_genblock_form is None                   # the hook is off unless a test switches it on
    # unaligned weights: the matrix-core forward is refused, the VALU forward and every backward are not
    d = dims_of(gd.CASES["g0-N4g2"])
    assert nv.genblock_form(d, 4, "fwd", wt_aligned=False)["lds_bytes"] == -1
    assert nv.genblock_form(d, 4, "infer", wg_aligned=False)["lds_bytes"] == -1
    assert nv.genblock_form(d, 4, "bwd", wg_aligned=False, wt_aligned=False)["lds_bytes"] > 0
    assert nv.genblock_form(dims_of(gd.CASES["g5-N4g2"]), 4, "fwd", wg_aligned=False, wr_aligned=False, wt_aligned=False)["lds_bytes"] > 0


# ---- eligibility sweep ------------------------------------------------------------------------------------------------------
def test_eligibility_agrees_with_the_oracle(lib):
    rng = random.Random(20240917)
    pick = lambda *v: rng.choice(v)          # noqa: E731
    seen = {"fwd+": 0, "fwd-": 0, "bwd+": 0, "bwd-": 0, "infer+": 0, "infer-": 0, "rows": 0}
    for i in range(2400):
        K = pick(1, 2, 3)
        Kp = rng.randint(1, K)
        C = pick(1, 2, 3, 4, 5, 8, 11, 12, 16, 17, 20, 21, 22, 31, 32, 33, 48, 64, 128, 255, 256, 257, 272, 300, 512)
        res = pick(0, 1, 2)
        Cin = C if res == 1 else pick(1, 2, 3, 4, 8, 12, 16, 20, 32, 44, 48, 60, 64, 68, 128, 256, 512, 528)
        Tc, Vc, rep = pick(1, 1, 2, 3, 4, 8, 9, 16, 32, 33), pick(1, 1, 2, 5, 7, 11, 16, 25, 32), pick(1, 2, 3, 4)
        V = pick(Vc, Vc, 1, 5, 11, 25, 32)
        bn_t = pick(0, 1)
        if i % 8 == 0:          # the wide blocks on tiny grids, where only the statistics rows decide
            K = Kp = 1
            C, Cin, res = pick(128, 255, 256, 257, 272, 300, 512), pick(16, 32), pick(0, 2)
            Tc, Vc, V, rep = pick(1, 2), 1, 1, pick(1, 2)
        d = nv.GenBlockDims(Cin, C, K, Kp, Tc, Vc, Tc * rep, V, rep, res, bool(bn_t), 1)
        a = nv._GenBlockArgs()
        a.N, a.groups = 4, 1
        nv._gb_common(a, d, 0.2)
        a.wg, a.wr, a.wt = PTR, PTR, PTR
        b = nv._GenBlockBwdArgs()
        b.N = 4
        nv._gb_common(b, d, 0.2)
        e = nv._GenBlockInferArgs()
        e.N = 4
        nv._gb_infer_dims(e, d, 0.2)
        e.wg, e.wr, e.wt = PTR, PTR, PTR
        got = (lib.kg_genblock_lds_bytes(ctypes.byref(a)), lib.kg_genblock_bwd_lds_bytes(ctypes.byref(b)),
               lib.kg_genblock_infer_lds_bytes(ctypes.byref(e)))
        infer_ok = d.T > 1 and d.Tc * d.Vc >= 16
        want = (pr._gb_lds_bytes(d, False), pr._gb_lds_bytes(d, True), pr._gb_lds_bytes(d, False, stats=False) if infer_ok else -1)
        assert got == want, (d, got, want)
        assert [nv.genblock_form(d, 4, k)["lds_bytes"] for k in ("fwd", "bwd", "infer")] == list(got), d
        assert pr.genblock_supported(d, 4, None, None, None) == (got[0] >= 0)
        for k, g_ in zip(("fwd", "bwd", "infer"), got):
            seen[k + ("+" if g_ >= 0 else "-")] += 1
        seen["rows"] += got[0] == -1 and pr._gb_lds_bytes(d, False, stats=False) >= 0
    # both answers of every query occur, and so does the refusal for the statistics rows alone
    assert all(v >= (5 if k == "rows" else 20) for k, v in seen.items()), seen
