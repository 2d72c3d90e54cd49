"""The C-ABI library builds for gfx950, loads without a GPU, and exports every symbol that
include/kgan_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build

import abi_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def header_functions():
    txt = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(kg_[a-z_0-9]+)\s*\(", txt)))


def test_header_symbols_exported(lib):
    names = header_functions()
    assert len(names) >= 15
    raw = ctypes.CDLL(_native.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in kgan_hip.h but not exported"
    assert sorted(_native.EXPORTS) == names       # the ctypes table binds exactly the header's API


def test_info_calls(lib):
    assert lib.kg_abi_version() == 9
    assert lib.kg_arch() == b"gfx950"


# every `#define KG_*` of the header that deliberately has no `_native` counterpart (KG_X <-> X); a name missing from both
# fails test_constants_match_header: a silently skipped name would hide a drift
DEFINES_WITHOUT_MIRROR = []


def test_struct_sizes_match_header():
    """ctypes mirrors must have the C layout: every ctypes.Structure of _native is a struct of the header (`_Foo` <-> `KgFoo`)
    and the other way round, with the header's size and the header's offset of every field (tests/abi_layout.py compiles one
    C program against the header)."""
    mirrors = abi_layout.mirrors()
    assert sorted(mirrors) == abi_layout.header_structs()
    assert len(mirrors) >= 44
    checked = 0
    for cname in sorted(mirrors):
        abi_layout.assert_mirror(cname)
        checked += len(abi_layout.header_layout(cname))
    assert checked >= 836       # sizeof of 44 structs + offsetof of their 792 fields


def test_constants_match_header():
    """every `#define KG_X` integer constant of the header equals `_native.X`; the ones without a counterpart are listed"""
    consts = abi_layout.header_constants()
    assert sorted(consts) == abi_layout.header_defines() and len(consts) >= 22
    assert consts["KG_ABI_VERSION"] == _native.ABI_VERSION
    missing = sorted(k for k in consts if not hasattr(_native, k[3:]))
    assert missing == sorted(DEFINES_WITHOUT_MIRROR)
    bad = {k: (v, getattr(_native, k[3:])) for k, v in consts.items() if hasattr(_native, k[3:]) and getattr(_native, k[3:]) != v}
    assert not bad, "(header, _native) differ at %s" % bad


def integration_md_stub(lib_path):
    """The fenced python block of INTEGRATION.md section B (the binding a reference maintainer would paste into
    models/init_gan/tgcn.py), executed as written against the in-tree library; returns its namespace."""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", txt, flags=re.S)
    stub = [b for b in blocks if "class KgAggArgs" in b]
    assert len(stub) == 1, "INTEGRATION.md must hold exactly one KgAggArgs stub"
    old = os.environ.get("KGAN_HIP_LIB")
    os.environ["KGAN_HIP_LIB"] = lib_path
    try:
        ns = {}
        exec(compile(stub[0], "INTEGRATION.md:stub", "exec"), ns)
    finally:
        if old is None:
            del os.environ["KGAN_HIP_LIB"]
        else:
            os.environ["KGAN_HIP_LIB"] = old
    return ns


def header_sizeof(name):
    return abi_layout.header_layout(name)["sizeof"]


def test_integration_md_stub(lib):
    """Round-5 VERDICT: the stub printed in INTEGRATION.md had gone stale (136-byte KgAggArgs against the header's 216).
    The stub a maintainer would paste is the stub this test runs: its struct must have the compiled header's size and
    field offsets, and its argtypes must bind (the GPU half, tests/test_kernels_gpu.py::test_integration_md_stub_values,
    calls graph_aggregate and compares with the oracle)."""
    ns = integration_md_stub(_native.LIB_PATH)
    S = ns["KgAggArgs"]
    assert ctypes.sizeof(S) == header_sizeof("KgAggArgs") == ctypes.sizeof(_native._AggArgs)
    mine = {n: getattr(_native._AggArgs, n).offset for n, _ in _native._AggArgs._fields_}
    theirs = {n: getattr(S, n).offset for n, _ in S._fields_}
    assert mine == theirs
    assert callable(ns["graph_aggregate"])


def test_invalid_args_are_rejected_without_gpu(lib):
    a = _native._ConvArgs()
    assert lib.kg_conv(ctypes.byref(a), None) < 0
    assert b"kg_conv" in lib.kg_last_error()
    w = _native._WgradArgs()
    assert lib.kg_wgrad_workspace_bytes(ctypes.byref(w)) < 0


def test_wgrad_many_plan_bounds_without_gpu(lib):
    """kg_wgrad_many_workspace_bytes plans a multi-layer weight-gradient call on the host (no launch): for the 16 conv
    weights of D at the critic step's sizes (bench.py: D_WGRAD_LAYERS, 192 samples) every layer gets at least one and at
    most 128 partial slabs, the wide early layers few (coarse workgroups), and a bad layer fails the whole call."""
    import bench
    n = len(bench.D_WGRAD_LAYERS)
    arr = (_native._WgradArgs * n)()
    slab = []
    for i, (M, Cin, taps, t_out, V, s) in enumerate(bench.D_WGRAD_LAYERS):
        a = arr[i]
        a.N, a.M, a.T_out, a.V_out, a.Cin, a.T_in, a.V_in = 128, M, t_out, V, Cin, t_out * s, V
        a.taps, a.tap_mode, a.t_stride = taps, _native.TAP_TIME, s
        a.g_sC, a.g_sN, a.x_sC, a.x_sN = 128 * t_out * V, t_out * V, 128 * t_out * s * V, t_out * s * V
        a.nextra = 1
        a.extra[0].N = 64
        a.extra[0].g_sC, a.extra[0].g_sN, a.extra[0].x_sC, a.extra[0].x_sN = 64 * t_out * V, t_out * V, 64 * t_out * s * V, t_out * s * V
        slab.append(4 * taps * M * Cin)
    total = lib.kg_wgrad_many_workspace_bytes(arr, n)
    assert sum(slab) <= total <= 128 * sum(slab), (total, sum(slab))
    # layer by layer: the same call with one layer plans that layer alone (>= 1 slab, <= 128 + one per extra pair)
    for i in range(n):
        one = lib.kg_wgrad_many_workspace_bytes(ctypes.byref(arr[i]), 1)
        assert slab[i] <= one <= 130 * slab[i], (i, one, slab[i])
    arr[3].taps = 2
    assert lib.kg_wgrad_many_workspace_bytes(arr, n) < 0 and b"taps" in lib.kg_last_error()


def test_wgrad_plan_reports_validate_without_gpu(lib):
    """kg_wgrad_many_plan / kg_wgrad_plan_info (additive, ABI v9): null or empty arguments are rejected by name, a bad layer
    fails the whole call with the launcher's own message, a good one is planned on the host - nothing is launched - and the
    plan agrees with the workspace the launcher asks for."""
    import bench
    v, s = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    arr = (_native._WgradArgs * 4)()
    assert lib.kg_wgrad_many_plan(None, 1, v, s) < 0 and b"kg_wgrad_many_plan: no jobs" in lib.kg_last_error()
    assert lib.kg_wgrad_many_plan(arr, 0, v, s) < 0 and b"kg_wgrad_many_plan: no jobs" in lib.kg_last_error()
    assert lib.kg_wgrad_many_plan(arr, 4, None, s) < 0 and b"kg_wgrad_many_plan: null output" in lib.kg_last_error()
    assert lib.kg_wgrad_many_plan(arr, 4, v, None) < 0 and b"kg_wgrad_many_plan: null output" in lib.kg_last_error()
    assert lib.kg_wgrad_many_plan(arr, 4, v, s) < 0 and b"kg_wgrad: bad dims" in lib.kg_last_error()       # empty structs
    one_v, one_s = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert lib.kg_wgrad_plan_info(None, ctypes.byref(one_v), ctypes.byref(one_s)) < 0 and b"kg_wgrad_plan_info: null" in lib.kg_last_error()
    assert lib.kg_wgrad_plan_info(ctypes.byref(arr[0]), None, ctypes.byref(one_s)) < 0 and b"kg_wgrad_plan_info: null" in lib.kg_last_error()
    assert lib.kg_wgrad_plan_info(ctypes.byref(arr[0]), ctypes.byref(one_v), None) < 0 and b"kg_wgrad_plan_info: null" in lib.kg_last_error()
    assert lib.kg_wgrad_plan_info(ctypes.byref(arr[0]), ctypes.byref(one_v), ctypes.byref(one_s)) < 0 and b"bad dims" in lib.kg_last_error()
    assert (one_v.value, one_s.value) == (-1, -1)
    for i, (M, Cin, taps, t_out, V, st) in enumerate(bench.D_WGRAD_LAYERS[:4]):
        a = arr[i]
        a.N, a.M, a.T_out, a.V_out, a.Cin, a.T_in, a.V_in = 128, M, t_out, V, Cin, t_out * st, V
        a.taps, a.tap_mode, a.t_stride = taps, _native.TAP_TIME, st
        a.g_sC, a.g_sN, a.x_sC, a.x_sN = 128 * t_out * V, t_out * V, 128 * t_out * st * V, t_out * st * V
    assert lib.kg_wgrad_many_plan(arr, 4, v, s) == 0
    tiles = (_native.WGRAD_TILE_128x128, _native.WGRAD_TILE_64x64, _native.WGRAD_TILE_64x32, _native.WGRAD_TILE_32x64,
             _native.WGRAD_TILE_32x32)
    assert tiles == (0, 1, 2, 3, 4) and set(_native.WGRAD_TILE_NAMES) == set(tiles)
    assert all(t in tiles for t in v) and all(1 <= n <= _native.WGRAD_MAX_SPLITS for n in s)
    # the launch never needs more workspace than the query promises (the query plans every layer at the finer, later-half cost)
    need = sum(4 * n * a.taps * a.M * a.Cin for n, a in zip(s, arr))
    assert 0 < need <= lib.kg_wgrad_many_workspace_bytes(arr, 4)
    for i in range(4):
        assert lib.kg_wgrad_plan_info(ctypes.byref(arr[i]), ctypes.byref(one_v), ctypes.byref(one_s)) == 0
        assert one_v.value == _native.WGRAD_TILE_64x64
        assert lib.kg_wgrad_workspace_bytes(ctypes.byref(arr[i])) == 4 * one_s.value * arr[i].taps * arr[i].M * arr[i].Cin
    arr[2].taps = 2
    assert lib.kg_wgrad_many_plan(arr, 4, v, s) < 0 and b"taps" in lib.kg_last_error()
    assert _native.last_wgrad_plan is None          # the hook is off unless a test switches it on


def test_agg_plan_reports_validate_without_gpu(lib):
    """kg_agg_plan_info / kg_agg_outer_many_plan / kg_aggconv_plan_info (additive, ABI v9): null arguments and a bad `op` are
    rejected by name, bad geometry fails with the launcher's own message and leaves the output untouched, good geometry is
    planned on the host - no operand pointer is needed, nothing is launched - and agrees with kg_agg_outer_slabs /
    kg_aggconv_supported."""
    p = _native._AggPlanInfo()
    p.form = -7
    a = _native._AggArgs()
    assert lib.kg_agg_plan_info(None, 0, ctypes.byref(p)) < 0 and b"kg_agg_plan_info: null" in lib.kg_last_error()
    assert lib.kg_agg_plan_info(ctypes.byref(a), 0, None) < 0 and b"kg_agg_plan_info: null" in lib.kg_last_error()
    assert lib.kg_agg_plan_info(ctypes.byref(a), 3, ctypes.byref(p)) < 0 and b"kg_agg_plan_info: op=3" in lib.kg_last_error()
    for op, who in ((_native.AGG_OP_EXPAND, b"kg_agg_expand: bad dims"), (_native.AGG_OP_REDUCE, b"kg_agg_reduce: bad dims"),
                    (_native.AGG_OP_OUTER, b"kg_agg_outer: bad dims")):
        assert lib.kg_agg_plan_info(ctypes.byref(a), op, ctypes.byref(p)) < 0 and who in lib.kg_last_error()
    assert p.form == -7
    a.N, a.C, a.K, a.V, a.W, a.T, a.rep = 64, 32, 3, 25, 11, 64, 1            # all pointers null: geometry only
    a.x_sN, a.x_sC, a.y_sN, a.y_sC, a.o_sN, a.o_sC = 64 * 25, 64 * 64 * 25, 64 * 11, 64 * 64 * 11, 64 * 11, 64 * 64 * 11
    assert lib.kg_agg_plan_info(ctypes.byref(a), _native.AGG_OP_EXPAND, ctypes.byref(p)) == 0
    assert p.form == _native.AGG_FORM_MFMA and (p.KI, p.KO, p.KS, p.RES, p.MSK) == (1, 3, 13, 0, 0) and p.ntiles == p.tiles_per_c * 32
    assert lib.kg_agg_plan_info(ctypes.byref(a), _native.AGG_OP_OUTER, ctypes.byref(p)) == 0
    assert p.form == _native.AGG_FORM_OUTER_MFMA and (p.K, p.TV, p.TW) == (3, 2, 1) and p.slabs == lib.kg_agg_outer_slabs(ctypes.byref(a)) == p.grid_x
    a.mask = 0x1000                                                           # (never read)
    assert lib.kg_agg_plan_info(ctypes.byref(a), _native.AGG_OP_EXPAND, ctypes.byref(p)) < 0 and b"kg_agg_reduce" in lib.kg_last_error()
    a.V, a.W, a.o_sN, a.o_sC = 11, 25, 64 * 25, 64 * 64 * 25
    a.x_sN, a.x_sC = 64 * 11, 64 * 64 * 11
    assert lib.kg_agg_plan_info(ctypes.byref(a), _native.AGG_OP_REDUCE, ctypes.byref(p)) == 0
    assert p.form == _native.AGG_FORM_MFMA and (p.KI, p.KO, p.KS, p.RES, p.MSK) == (3, 1, 17, 0, 1)
    a.rep = 2
    assert lib.kg_agg_plan_info(ctypes.byref(a), _native.AGG_OP_REDUCE, ctypes.byref(p)) < 0 and b"fold" in lib.kg_last_error()
    a.mask = None
    assert lib.kg_agg_plan_info(ctypes.byref(a), _native.AGG_OP_REDUCE, ctypes.byref(p)) == 0 and p.form != _native.AGG_FORM_MFMA
    # kg_agg_outer_many_plan
    arr = (_native._AggArgs * 3)()
    la, ns = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
    assert lib.kg_agg_outer_many_plan(None, 1, la, ns) < 0 and b"kg_agg_outer_many_plan: no jobs" in lib.kg_last_error()
    assert lib.kg_agg_outer_many_plan(arr, 0, la, ns) < 0 and b"kg_agg_outer_many_plan: no jobs" in lib.kg_last_error()
    assert lib.kg_agg_outer_many_plan(arr, 3, None, ns) < 0 and b"kg_agg_outer_many_plan: null output" in lib.kg_last_error()
    assert lib.kg_agg_outer_many_plan(arr, 3, la, None) < 0 and b"kg_agg_outer_many_plan: null output" in lib.kg_last_error()
    assert lib.kg_agg_outer_many_plan(arr, 3, la, ns) < 0 and b"kg_agg_outer_many: job 0 bad dims" in lib.kg_last_error()   # empty structs
    for i in range(3):
        j = arr[i]
        j.N, j.C, j.K, j.V, j.W, j.T, j.rep = 8, 4 + i, 3, 11, 5, 16, 2 if i == 1 else 1
        j.x_sN, j.x_sC, j.y_sN, j.y_sC = 16 * 11, 8 * 16 * 11, 16 * j.rep * 5, 8 * 16 * j.rep * 5
    assert lib.kg_agg_outer_many_plan(arr, 3, la, ns) == 0 and list(la) == [0, -1, 0]
    assert list(ns) == [lib.kg_agg_outer_slabs(ctypes.byref(arr[i])) for i in range(3)]
    arr[2].K = 2
    assert lib.kg_agg_outer_many_plan(arr, 3, la, ns) < 0 and b"job 2 K=2" in lib.kg_last_error()
    # kg_aggconv_plan_info
    q = _native._AggConvPlanInfo()
    q.tiny = -7
    c = _native._AggConvArgs()
    assert lib.kg_aggconv_plan_info(None, 0, ctypes.byref(q)) < 0 and b"kg_aggconv_plan_info: null" in lib.kg_last_error()
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 0, None) < 0 and b"kg_aggconv_plan_info: null" in lib.kg_last_error()
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), -1, ctypes.byref(q)) < 0 and b"label_J=-1" in lib.kg_last_error()
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 0, ctypes.byref(q)) < 0 and b"kg_aggconv: bad dims" in lib.kg_last_error()
    assert q.tiny == -7
    c.N, c.Cin, c.M, c.T, c.V, c.W, c.K = 192, 64, 128, 64, 11, 5, 3          # the critic's D2 launch at 192 samples
    c.x_sN, c.x_sC, c.w_sT, c.w_sO, c.w_sI, c.o_sN, c.o_sC = 64 * 11, 192 * 64 * 11, 128 * 64, 64, 1, 64 * 5, 192 * 64 * 5
    c.pcount[0], c.pcount[1], c.pcount[2] = 1, 4, 1
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 0, ctypes.byref(q)) == 0
    assert (q.tiny, q.BM, q.KS, q.XE, q.XA, q.ADD, q.tapmask) == (0, 64, 2, 6, 0, 0, 7) and q.spanp == (127 // 5 + 2) * 11 + 3 & ~3
    assert (q.grid_x, q.grid_y) == (192 * 64 * 5 // 128, 2)
    c.xa, c.add = 0x1000, 0x1000                                              # (never read)
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 0, ctypes.byref(q)) == 0 and (q.XA, q.ADD) == (1, 1)
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 20, ctypes.byref(q)) < 0 and b"takes the place of `add`" in lib.kg_last_error()
    c.add = None
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 20, ctypes.byref(q)) < 0 and b"tiny-channel geometry" in lib.kg_last_error()
    c.Cin, c.M = 3, 32
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 20, ctypes.byref(q)) == 0 and (q.tiny, q.MT, q.RG, q.LB) == (1, 32, 4, 1)     # 192 x 2 workgroups of 256 columns < 512: four threads per column
    assert q.lds_bytes == 4 * ((3 * 11 * 5 + 3 & ~3) + 3 * 32 * 20 + 20)
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 0, ctypes.byref(q)) == 0 and (q.tiny, q.LB) == (1, 0)
    c.V, c.W = 25, 1                                                          # 129 frames x 25 floats per staged row
    c.Cin = 8
    assert lib.kg_aggconv_plan_info(ctypes.byref(c), 0, ctypes.byref(q)) < 0 and b"source span" in lib.kg_last_error()
    assert _native.last_agg_plan is None and _native.last_aggconv_plan is None       # the hooks are off unless a test switches them on


def test_conv_form_reports_validate_without_gpu(lib):
    """kg_conv_form_info / kg_conv_many_form (additive, ABI v9): null arguments are rejected, the argument checks are those of
    the launch, nothing is launched and no operand is read (every pointer here is a made-up address)"""
    f, mf = _native._ConvFormInfo(), _native._ConvManyForm()
    a = _native._ConvArgs()
    assert lib.kg_conv_form_info(None, ctypes.byref(f)) < 0 and b"kg_conv: null args" in lib.kg_last_error()
    assert lib.kg_conv_form_info(ctypes.byref(a), ctypes.byref(f)) < 0 and b"kg_conv: bad dims" in lib.kg_last_error()
    a.N, a.M, a.T_out, a.V_out, a.ngroups = 2, 33, 9, 9, 1
    g = a.g[0]
    g.x, g.w, g.x_sN, g.x_sC, g.Cin, g.T_in, g.V_in = 0x1000, 0x1000, 81, 162, 64, 9, 9
    g.w_sT, g.w_sO, g.w_sI, g.w_MB, g.taps, g.t_stride = 33 * 64, 64, 1, 1 << 30, 3, 1
    assert lib.kg_conv_form_info(ctypes.byref(a), None) < 0 and b"kg_conv_form_info: null output" in lib.kg_last_error()
    assert lib.kg_conv_form_info(ctypes.byref(a), ctypes.byref(f)) == 0
    assert (f.family, f.tile, f.BM, f.NW, f.KW, f.KF, f.FAST, f.PLAIN, f.INK, f.nsplit, f.epilogue) == (
        _native.CONV_FAMILY_DIRECT, 2, 32, 4, 1, 1, 1, 0, 0, 1, 0) and (f.grid_x, f.grid_y, f.grid_z) == (2, 2, 1)
    g.taps = 2
    assert lib.kg_conv_form_info(ctypes.byref(a), ctypes.byref(f)) < 0 and b"taps=2" in lib.kg_last_error()
    g.taps = 3
    arr = (_native._ConvArgs * 2)(a, a)
    assert lib.kg_conv_many_form(None, 2, ctypes.byref(mf)) < 0 and b"kg_conv_many_form: bad arguments" in lib.kg_last_error()
    assert lib.kg_conv_many_form(arr, 0, ctypes.byref(mf)) < 0 and lib.kg_conv_many_form(arr, 2, None) < 0
    assert lib.kg_conv_many_form(arr, 2, ctypes.byref(mf)) == 0
    assert (mf.tile, mf.BM, mf.KF, mf.PLAIN, mf.njobs, mf.total_wg) == (2, 32, 1, 0, 2, 16) and list(mf.wg_begin)[:2] == [0, 8]
    assert lib.kg_conv_many_form(arr, 1, ctypes.byref(mf)) == 0 and mf.tile == -1          # one job: a plain kg_conv launch
    arr[1].g[0].Cin = 40
    assert lib.kg_conv_many_form(arr, 2, ctypes.byref(mf)) == 0 and mf.tile == -1          # partial K-slices: one launch per job
    arr[1].ngroups = 3
    assert lib.kg_conv_many_form(arr, 2, ctypes.byref(mf)) < 0 and b"ngroups=3" in lib.kg_last_error()
    assert _native.last_conv_form is None                                                  # the hook is off unless a test switches it on


def test_mapping_network_entry_points_validate_without_gpu(lib):
    """kg_linear_fwd / kg_linear_bwd / kg_embed_bwd (ABI v6): argument checking happens before any launch."""
    a = _native._LinearArgs()
    assert lib.kg_linear_fwd(ctypes.byref(a), None) < 0 and b"kg_linear_fwd" in lib.kg_last_error()
    a.N, a.Din, a.Dout, a.J = 4, 16, 16, 20
    assert lib.kg_linear_fwd(ctypes.byref(a), None) < 0 and b"J=20" in lib.kg_last_error()
    a.J = 4                                   # embedding columns without a table
    assert lib.kg_linear_bwd(ctypes.byref(a), None) < 0 and b"embedding" in lib.kg_last_error()
    a.J = 0
    a.x, a.x_ld = 16, 8                       # leading dimension shorter than the row
    assert lib.kg_linear_fwd(ctypes.byref(a), None) < 0 and b"x_ld" in lib.kg_last_error()
    a.x_ld, a.act = 16, 2                     # tanh is not an activation of this path
    assert lib.kg_linear_fwd(ctypes.byref(a), None) < 0 and b"act" in lib.kg_last_error()
    a.act = 1
    assert lib.kg_linear_fwd(ctypes.byref(a), None) < 0 and b"null w" in lib.kg_last_error()
    assert lib.kg_linear_bwd(ctypes.byref(a), None) < 0 and b"null g" in lib.kg_last_error()
    assert lib.kg_embed_bwd(ctypes.byref(a), None) < 0 and b"kg_embed_bwd" in lib.kg_last_error()


def test_round3_entry_points_validate_without_gpu(lib):
    """kg_conv_many / kg_conv_many_plan / kg_agg_reduce's epilogue fields: argument checking happens before any launch."""
    t = ctypes.c_int32(7)
    assert lib.kg_conv_many_plan(None, 0, ctypes.byref(t)) < 0 and b"kg_conv_many_plan" in lib.kg_last_error()
    arr = (_native._ConvArgs * 2)()
    assert lib.kg_conv_many(arr, 2, None) < 0 and b"kg_conv" in lib.kg_last_error()          # empty problems: bad dims
    a = _native._AggArgs()
    a.N, a.C, a.K, a.V, a.W, a.T, a.rep = 2, 4, 3, 5, 5, 8, 2
    a.a = a.x = a.out = 0x1000
    a.mask = 0x2000
    assert lib.kg_agg_reduce(ctypes.byref(a), None) < 0 and b"fold" in lib.kg_last_error()     # epilogue needs fold = 1
    a.rep, a.mask, a.res = 1, None, 0x3000                                                    # residual without its geometry
    assert lib.kg_agg_reduce(ctypes.byref(a), None) < 0 and b"residual geometry" in lib.kg_last_error()
    a.res = None
    a.mask = 0x2000
    assert lib.kg_agg_expand(ctypes.byref(a), None) < 0 and b"kg_agg_reduce" in lib.kg_last_error()   # epilogue is reduce-only


def test_no_cpu_fallback():
    import torch
    x = torch.zeros(1, 3, 4, 5)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.rowsum(x)


def test_host_code_under_asan(tmp_path):
    """SURVEY.md 5 (sanitizers): the library's host side - validation, plans, workspace sizing, job tables - built with
    -fsanitize=address (build.py --asan; device code unchanged, GPU ASAN is not available on this pool) and driven
    by tests/asan_host_check.c through every entry point that does not launch.  No GPU needed."""
    import glob
    import subprocess
    from kinetic_gan_amd import build as kbuild
    lib = kbuild.build_asan()
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    if not rt:
        pytest.skip("clang ASAN runtime not found")
    exe = os.path.join(tmp_path, "asan_host_check")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang", "-fsanitize=address", "-shared-libsan", "-g", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "asan_host_check.c"), lib, "-o", exe,
                           "-Wl,-rpath," + os.path.dirname(lib) + ":" + os.path.dirname(rt[-1]) + ":/opt/rocm/lib"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", LD_LIBRARY_PATH=os.path.dirname(rt[-1]) + ":/opt/rocm/lib")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "asan host check ok" in r.stdout and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr


def test_comm_entry_points_without_gpu(lib):
    """kg_comm_*: RCCL is bound lazily; the id call works on a CPU-only box, init fails cleanly without a device, destroy
    of NULL is a no-op, bad arguments are rejected."""
    import torch
    buf = ctypes.create_string_buffer(_native.COMM_ID_BYTES)
    rc = lib.kg_comm_unique_id(buf)
    if rc == 0:
        assert any(b != 0 for b in buf.raw)
    else:
        assert b"kg_comm_unique_id" in lib.kg_last_error()         # librccl not present on this box
    assert lib.kg_comm_destroy(None) == 0
    h = ctypes.c_void_p()
    assert lib.kg_comm_init(ctypes.byref(h), 1, 1, buf, 0) < 0 and b"rank" in lib.kg_last_error()
    assert lib.kg_allreduce_flat(None, None, 0, None) < 0
    if not torch.cuda.is_available():
        assert lib.kg_comm_init(ctypes.byref(h), 0, 1, buf, 0) != 0 and h.value is None
