"""CPU: tests/wgrad_def.py can be trusted before a GPU is involved.

  * the float64 definition equals oracle/prim_ref.wgrad on integer data (where both are exact);
  * an fp32 evaluation in another summation order, and a three-term bf16-split evaluation with the six kept products, stay
    inside the bracket for every float case the GPU tests run;
  * the definition with ONE column's products left out, or ONE column read one time step later, falls outside the bracket in
    at least one element for every such case - a kernel that is wrong by that much cannot pass the GPU tests;
  * the launches of tests/test_wgrad_tiles_gpu.py are planned (kg_wgrad_many_plan: host code, no GPU) onto the tile
    variants and split classes they are named after.
"""
import ctypes

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import build
from oracle import prim_ref as pr
from tests import wgrad_def as wd
from tests.util import ReloadingEnv

FLOAT_IDS = [c.name for c in wd.FLOAT_CASES]


# ---- the definition against prim_ref ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wd.SMALL_CASES, ids=[c.name for c in wd.SMALL_CASES])
@pytest.mark.parametrize("npairs,accumulate", [(1, False), (3, True)])
def test_definition_equals_prim_ref_on_integer_data(case, npairs, accumulate):
    case = case._replace(Ns=tuple(case.Ns[0] + q for q in range(npairs)))
    pairs, base = wd.integer_case(7, case)
    wv, numel = case.view()
    vmap = None if case.vmap is None else torch.tensor(case.vmap, dtype=torch.int32)
    ref, _, _ = wd.reference(case, pairs, base if accumulate else None)
    out = base.clone() if accumulate else None
    got = pr.wgrad(pairs[0][0], pairs[0][1], case.Cin, case.taps, case.mode, case.stride, vmap, numel,
                   nv.WView(wv.sT, wv.sO, wv.sI), out=out, accumulate=accumulate, extra=pairs[1:])
    assert ref.abs().max() > 0 and torch.equal(got.double(), ref)


# ---- emulations inside the bracket --------------------------------------------------------------------------------------------
def _column_matrices(case, pairs):
    """per tap d and pair p: (G (M, cols), X (Cin, cols)) in fp32, columns in (n, to, vo) order"""
    out = []
    for d in range(case.taps):
        row = []
        for g, x in pairs:
            xs = wd._src(x, case.Cin, d, case.taps, case.mode, case.stride, case.vmap, case.T_out, case.V_out).float()
            row.append((g.permute(1, 0, 2, 3).reshape(case.M, -1).contiguous(), xs.permute(1, 0, 2, 3).reshape(case.Cin, -1).contiguous()))
        out.append(row)
    return out


def _scatter(case, vals, base):
    wv, numel = case.view()
    out = torch.zeros(numel) if base is None else base.clone()
    idx = wd._index(wv, case.taps, case.M, case.Cin)
    out[idx] = out[idx] + vals.reshape(-1) if base is not None else vals.reshape(-1)
    return out


def emulate_fp32(case, pairs, base, chunk=32, per_split=3):
    """fp32 all the way, in an order that is not torch's: 32-column chunks added up per split of three chunks, the splits
    added last to first, then the base"""
    vals = []
    for row in _column_matrices(case, pairs):
        slabs = []
        for G, X in row:
            chunks = [G[:, j:j + chunk] @ X[:, j:j + chunk].T for j in range(0, G.shape[1], chunk)]
            for s in range(0, len(chunks), per_split):
                acc = torch.zeros(case.M, case.Cin)
                for c in chunks[s:s + per_split]:
                    acc = acc + c
                slabs.append(acc)
        tot = torch.zeros(case.M, case.Cin)
        for s in reversed(slabs):
            tot = tot + s
        vals.append(tot)
    return _scatter(case, torch.stack(vals), base)


def _split3(t):
    h = t.bfloat16().float()
    m = (t - h).bfloat16().float()
    lo = (t - h - m).bfloat16().float()
    assert torch.equal(h + m + lo, t)          # (the three terms sum to x exactly)
    return h, m, lo


def emulate_split(case, pairs, base, chunk=16):
    """three bf16 terms per operand (torch's round-to-nearest bf16), the six kept products per 16-column group added small
    to large in fp32 - the arithmetic of wgrad_tile_bs in torch's summation order"""
    vals = []
    for row in _column_matrices(case, pairs):
        tot = torch.zeros(case.M, case.Cin)
        for G, X in row:
            gh, gm, gl = _split3(G)
            xh, xm, xl = _split3(X)
            for j in range(0, G.shape[1], chunk):
                s = slice(j, j + chunk)
                for a, b in ((gl, xh), (gh, xl), (gm, xm), (gm, xh), (gh, xm), (gh, xh)):
                    tot = tot + a[:, s] @ b[:, s].T
        vals.append(tot)
    return _scatter(case, torch.stack(vals), base)


@pytest.mark.parametrize("case", wd.FLOAT_CASES, ids=FLOAT_IDS)
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
def test_emulations_stay_inside_the_bracket(case, accumulate):
    assert case.K <= wd.K_FLOAT_MAX
    pairs, base = wd.operands(case, 11, integer=False)
    base = base if accumulate else None
    ref, S, K = wd.reference(case, pairs, base)
    r32 = wd.worst_ratio(emulate_fp32(case, pairs, base), ref, S, K)
    rbs = wd.worst_ratio(emulate_split(case, pairs, base), ref, S, K, split=True)
    print("%s: max err / bracket  fp32 order %.4f  bf16-split %.4f" % (case.name, r32, rbs))
    assert r32 <= 1.0 and rbs <= 1.0
    # and the emulations are exact on integer data, as the kernels must be
    pairs, base = wd.integer_case(12, case)
    base = base if accumulate else None
    ref, _, _ = wd.reference(case, pairs, base)
    assert torch.equal(emulate_fp32(case, pairs, base).double(), ref)
    assert torch.equal(emulate_split(case, pairs, base).double(), ref)


def test_dropped_terms_of_the_split_are_below_the_derived_bound():
    """the three dropped products of (gh + gm + gl)(xh + xm + xl): together below 3 * 2^-24 |g x|, each below 2^-24 (1 + 2^-8) |g x|"""
    gen = torch.Generator().manual_seed(5)
    g, x = torch.randn(1 << 16, generator=gen), torch.randn(1 << 16, generator=gen)
    (gh, gm, gl), (xh, xm, xl) = _split3(g), _split3(x)
    p = (g.double() * x.double()).abs()
    for a, b in ((gm, xl), (gl, xm), (gl, xl)):
        assert ((a.double() * b.double()).abs() <= 2.0 ** -24 * (1 + 2.0 ** -8) * p).all()
    kept = sum(a.double() * b.double() for a, b in ((gh, xh), (gh, xm), (gm, xh), (gm, xm), (gh, xl), (gl, xh)))
    assert ((kept - g.double() * x.double()).abs() <= 3 * 2.0 ** -24 * p).all()
    mags = sum((a.double() * b.double()).abs() for a, b in ((gh, xh), (gh, xm), (gm, xh), (gm, xm), (gh, xl), (gl, xh)))
    assert (mags <= (1 + 2.0 ** -6) * p).all()


# ---- mutation check -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wd.FLOAT_CASES, ids=FLOAT_IDS)
def test_one_wrong_column_falls_outside_the_bracket(case):
    """a condition on the INPUTS of the float cases (few enough columns), not a tolerance: with the wider of the two
    brackets, and with the accumulate base in place"""
    pairs, base = wd.operands(case, 11, integer=False)
    ref, S, K = wd.reference(case, pairs, base)
    col = wd.pick_column(case, 3)
    for kind in ("drop", "shift"):
        bad, _, _ = wd.reference(case, pairs, base, mutate=(kind,) + col)
        for split in (False, True):
            assert wd.worst_ratio(bad, ref, S, K, split=split) > 1.0, (case.name, kind, split)


# ---- the plan of the GPU tests' launches (host code only) ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return nv.load_library()


def geometry_args(case):
    """KgWgradArgs of a case without tensors (channel-major strides): what the plan looks at"""
    a = nv._WgradArgs()
    a.N, a.M, a.T_out, a.V_out = case.Ns[0], case.M, case.T_out, case.V_out
    a.Cin, a.T_in, a.V_in = case.Cin, case.T, case.V
    a.taps, a.tap_mode, a.t_stride = case.taps, case.mode, case.stride
    a.vmap = None if case.vmap is None else 0x1000
    lo, li = case.T_out * case.V_out, case.T * case.V
    a.g_sN, a.g_sC, a.x_sN, a.x_sC = lo, case.Ns[0] * lo, li, case.Ns[0] * li
    a.nextra = len(case.Ns) - 1
    for q, n in enumerate(case.Ns[1:]):
        e = a.extra[q]
        e.N, e.g_sN, e.g_sC, e.x_sN, e.x_sC = n, lo, n * lo, li, n * li
    return a


def plan_many(lib, cases):
    arr = (nv._WgradArgs * len(cases))(*[geometry_args(c) for c in cases])
    v, s = (ctypes.c_int32 * len(cases))(), (ctypes.c_int32 * len(cases))()
    assert lib.kg_wgrad_many_plan(arr, len(cases), v, s) == 0, lib.kg_last_error()
    return list(zip(v, s))


@pytest.mark.parametrize("name", list(wd.LAUNCHES))
def test_gpu_launches_are_planned_as_named(name, lib, monkeypatch):
    env = ReloadingEnv(monkeypatch)
    launch = wd.LAUNCHES[name]
    try:
        for k, v in launch.env.items():
            env.setenv(k, v)
        plan = plan_many(lib, launch.cases)
    finally:
        env.undo()
    launch.check(launch.cases, plan)


def test_small_cases_reach_all_four_small_variants(lib):
    seen = set()
    for cases in (wd.SMALL_CASES, [c.short() for c in wd.SMALL_CASES]):
        seen |= {v for v, _ in plan_many(lib, cases)}
        for c in cases:
            seen.add(plan_many(lib, [c])[0][0])
    assert seen == {nv.WGRAD_TILE_64x64, nv.WGRAD_TILE_64x32, nv.WGRAD_TILE_32x64, nv.WGRAD_TILE_32x32}
    v3264 = plan_many(lib, [wd.Case("3264", (5,), 70, 20, 9, 16, 3, wd.TAP_TIME, 1)])
    assert v3264[0][0] == nv.WGRAD_TILE_32x64


def test_single_layer_plan_is_the_64x64_tile(lib):
    for c in wd.SMALL_CASES + wd.BIG_DEFAULT:
        a = geometry_args(c)
        v, s = ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert lib.kg_wgrad_plan_info(ctypes.byref(a), ctypes.byref(v), ctypes.byref(s)) == 0
        assert v.value == nv.WGRAD_TILE_64x64 and 1 <= s.value <= nv.WGRAD_MAX_SPLITS + 2
        assert lib.kg_wgrad_workspace_bytes(ctypes.byref(a)) == 4 * s.value * c.taps * c.M * c.Cin
