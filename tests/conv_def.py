"""Float64 definition of the tap GEMM (kg_conv / kg_conv_many, include/kgan_hip.h), the bracket a correct kernel must land
in, and the data and the two case tables of tests/test_conv_def_cpu.py and tests/test_conv_forms_gpu.py.  Test code only:
torch ops that run on any device (nothing of oracle/prim_ref.py is called).

  out[m, j] = act( sum_g sum_d sum_c W_g(d, m, c) X_g[c (+ d Cin_g), src_g(j, d)] + bias0[m] + bias1[m]
                   + add[m, (n, to a_tstride, vo)] ) * (mask[m, j] > 0 ? 1 : slope)            (the last factor with `mask`)
  j = (n, to, vo);  src_g(j, d) = (n, ti, vi) with
    time taps       shift = d - (taps - 1) / 2;   channel blocks: shift = 0 and the channel is c + d Cin
    forward         ti = to t_stride + shift                      (a product with ti outside [0, T_in) is 0)
    transposed      ti = (to - shift) / t_stride                  (0 unless to - shift >= 0, divisible, ti < T_in)
    vi = vmap[vo]  (a product with vmap[vo] < 0 - a dropped vertex - is 0), or vo without a map
  W_g(d, m, c) = w[d w_sT + (m / w_MB) w_sMB + (m % w_MB) w_sO + c w_sI]
written to frame out_t0 + to o_tstride of `out`; every other frame of `out` keeps what it held (`base`).

Error bracket (derived, not measured).  u = 2^-24 (fp32 round to nearest).  Per element, n = the number of its non-zero
products (Cin_g for every (g, d) whose source exists; at most sum taps Cin), S = the same sum over |W| |X| plus
|bias0| + |bias1| + |add|.  A kernel's result r must satisfy

    |r - ref| <= (a n (1 + e) + b) u S + c u |ref|.

fp32 forms (kg_conv_kernel, kg_conv_many_kernel, kg_conv_tiny_kernel), a = 1, e = 0.  Every product enters a tree of additions
whose leaves are the element's n non-zero products - MFMA steps of two products each, or the tiny kernel's fma chain -
in some fixed order.  A product is rounded at most once when it is formed (not at all by a fused multiply-add) and once per
addition on its way to the root, at most n - 1 additions; additions of an exact zero (out-of-range loads, the zero an
accumulator starts from, a dead slice) round nothing.  So the sum is sum_i p_i (1 + t_i) with |t_i| <= (1 + u)^n - 1: the
classical bound, valid in ANY order - the wgrad_def.py argument.  b pays, a second time and separately, for what is added
outside that chain, counted from csrc/kg_conv.hip:
   3   K32x32: `v = 0 + red[0] + red[1] + red[2] + red[3]`, the four waves' partial tiles (conv_tile, KW > 1);
   nsplit - 1   the slabs, `s16 += v[k]` (finish_split) or `v += p[k per]` (kg_conv_splitk_epilogue), the first onto 0;
   2   the biases: `bias_r0 + bias_r1` then `acc + bias_lds` (store_tile), or `v += bias0; v += bias1` (epilogue, tiny);
   1   `v += add`;
   1   the second-order part of the bound above (n u <= 2^-10 for every n used here) and 1 spare:
b = nsplit + 7 (B_FP32), each term a rounding of a partial sum that is at most S in magnitude.
c pays for what multiplies the RESULT: 1 for the rounding of the value stored (the second-order remainder of the last
addition), 1 for LeakyReLU's `t * slope`, 1 for the mask factor: c = 1 + [act = LRELU] + [mask].  LeakyReLU (slope <= 1), tanh
and the mask factor (<= 1) are 1-Lipschitz, so the bracket of the pre-activation value carries through them unchanged.
tanh: the device's tanhf adds its own error.  The ROCm documentation on the build machine states no accuracy for it (no
mention of tanh next to "ulp" under the ROCm tree), so this file uses OpenCL's bound for tanh, 5 ulp <= 5 * 2^-23 |tanh| =
10 u |ref|: c = 11 for tanh launches.

bf16-split forms (kg_conv_bs_kernel, kg_conv_bsw_kernel), a = 6, e = 2^-6, b = nsplit + 10.  Each operand is split
x = h + m + l into three bf16 numbers and six of the nine products are kept - hh, hm, mh, mm, hl, lh; the three dropped are
below 3 * 2^-24 of |w x| together (3 more of b); the kept ones are exact in fp32 and are added in fp32, six per product: a
tree of 6 n leaves over magnitudes that sum to less than (1 + 2^-6) S.  The argument is written out in wgrad_def.py.

Exact cases.  Integer data: every operand an integer -3 .. 3, biases and `add` integers, act NONE or LRELU with slope 2^-2,
mask slope 2^-2.  Every product and every partial sum of any subset is an integer below 9 * 1536 + 9 < 2^24 and the slope
multiplies are exact, so every fp32 operation of every order is exact; every operand is a bf16 number (h = x, m = l = 0), so
the split forms are exact too.  On such data a kernel equals this definition bit for bit.  No tanh there.

Tables.  TABLE_A: one case (at least) per compiled instantiation a launch can reach, INSTANTIATIONS being the literal list
- 110 of kg_conv_kernel, 12 of kg_conv_many_kernel, 3 of kg_conv_bs_kernel, 6 of kg_conv_bsw_kernel, 2 of
kg_conv_tiny_kernel: 133, the count of the dispatch code.  TABLE_B: the logical edges.  A case names the KG_CONV_* switches
that force its form and the fields of kg_conv_form_info / kg_conv_many_form it expects.
"""
import math
from typing import NamedTuple, Optional, Tuple

import torch

TAP_TIME, TAP_CHANBLOCK = 0, 1
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
U = 2.0 ** -24
SLOPE_EXACT, SLOPE_FLOAT = 0.25, 0.2
TANH_ULP = 5                        # OpenCL's bound (module docstring)
DATA_SEED = 7
K_MAX = 1536                        # the most products of one element in any case (integer exactness, n u <= 2^-10)
BASE = -12345.0                     # what a caller's `out` holds before the launch


def b_of(nsplit, split_form):
    return nsplit + 7 + (3 if split_form else 0)


# ---- the definition -----------------------------------------------------------------------------------------------------------
class WV(NamedTuple):               # weight view: W(d, m, c) = buf[off + d sT + (m // MB) sMB + (m % MB) sO + c sI]
    sT: int
    sO: int
    sI: int
    sMB: int = 0
    MB: int = 1 << 30
    off: int = 0
    numel: int = 0                  # elements of the parent buffer


def weight_index(wv, taps, M, Cin, device="cpu"):
    d = torch.arange(taps, device=device).view(-1, 1, 1)
    m = torch.arange(M, device=device).view(1, -1, 1)
    c = torch.arange(Cin, device=device).view(1, 1, -1)
    mb = torch.div(m, wv.MB, rounding_mode="floor")
    return wv.off + d * wv.sT + mb * wv.sMB + (m - mb * wv.MB) * wv.sO + c * wv.sI


def weights_f64(wbuf, wv, taps, M, Cin):
    """(taps, M, Cin) float64"""
    return wbuf.double()[weight_index(wv, taps, M, Cin, wbuf.device)]


def source_index(g, d, T_out, V_out, T_in, vmap, device):
    """(ti (T_out,), vi (V_out,), ok (T_out, V_out)): where tap d of group g reads, clamped, and whether the product exists"""
    shift = d - (g.taps - 1) // 2 if g.tap_mode == TAP_TIME else 0
    to = torch.arange(T_out, device=device)
    if not g.transposed:
        ti = to * g.t_stride + shift
        ok_t = (ti >= 0) & (ti < T_in)
    else:
        num = to - shift
        ti = torch.div(num, g.t_stride, rounding_mode="floor")
        ok_t = (num >= 0) & (num - ti * g.t_stride == 0) & (ti < T_in)
    vi = torch.arange(V_out, device=device) if vmap is None else vmap.to(device).long()
    ok_v = vi >= 0
    return ti.clamp(0, T_in - 1), vi.clamp_min(0), ok_t.view(-1, 1) & ok_v.view(1, -1)


def source_f64(x, g, d, T_out, V_out, vmap, shifted=None):
    """(N, Cin, T_out, V_out) float64: X at the source of every column for tap d, 0 where there is none.
    shifted = (n, to, vo): that one column reads one frame later (a mutation, for the tests of the tests)."""
    T_in = x.shape[2]
    ch0 = d * g.Cin if g.tap_mode == TAP_CHANBLOCK else 0
    ti, vi, ok = source_index(g, d, T_out, V_out, T_in, vmap, x.device)
    xs = x[:, ch0:ch0 + g.Cin].double()[:, :, ti][:, :, :, vi] * ok.double()
    if shifted is not None:
        n, to, vo = shifted
        t1 = int(ti[to]) + 1
        xs[n, :, to, vo] = x[n, ch0:ch0 + g.Cin, t1, int(vi[vo])].double() if (t1 < T_in and bool(ok[to, vo])) else 0.0
    return xs, ok


def act_f64(v, act, slope):
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * slope)
    if act == ACT_TANH:
        return torch.tanh(v)
    return v


def conv_f64(c, o, slope, mutate=None):
    """The definition on the operands `o` (Case.operands) -> (ref, S, n): float64 tensors of the whole `out` tensor
    (N, M, T_total, V_out); frames the launch does not write hold BASE in ref and 0 in S and n.
    mutate (NOT the definition, for the mutation check): ("shift", n, to, vo) | ("vmap", vo) | ("wswap", m, cc) | ("nobias1",) |
    ("add_tstride",) | ("maskflip", n, m, to, vo) | ("o_tstride",)"""
    kind = mutate[0] if mutate else None
    dev = o["x"][0].device
    N, M, T_out, V_out = c.N, c.M, c.T_out, c.V_out
    pre = torch.zeros(N, M, T_out, V_out, dtype=torch.float64, device=dev)
    S = torch.zeros_like(pre)
    n = torch.zeros(T_out, V_out, dtype=torch.float64, device=dev)
    for gi, g in enumerate(c.groups):
        W = weights_f64(o["w"][gi], o["wv"][gi], g.taps, M, g.Cin)
        if kind == "wswap" and gi == 0:
            _, m, cc = mutate
            W = W.clone()
            W[:, m, [cc, cc + 1]] = W[:, m, [cc + 1, cc]]
        vmap = o["vmap"][gi]
        if kind == "vmap" and gi == c.vmap_group():
            vmap = vmap.clone()
            vo = mutate[1]
            vmap[vo] = (int(vmap[vo]) + 1) % g.V_in if int(vmap[vo]) >= 0 else 0
        for d in range(g.taps):
            xs, ok = source_f64(o["x"][gi], g, d, T_out, V_out, vmap, mutate[1:] if kind == "shift" and gi == 0 and d == g.taps - 1 else None)
            pre += torch.einsum("mc,nctv->nmtv", W[d], xs)
            S += torch.einsum("mc,nctv->nmtv", W[d].abs(), xs.abs())
            n += ok.double() * g.Cin
    for key in ("bias0", "bias1"):
        if o.get(key) is not None and not (kind == "nobias1" and key == "bias1"):
            pre += o[key].double().view(1, -1, 1, 1)
            S += o[key].double().abs().view(1, -1, 1, 1)
    if o.get("add") is not None:
        ats = 1 if kind == "add_tstride" else c.add
        a = o["add"].double()[:, :, ::ats][:, :, :T_out]
        pre += a
        S += a.abs()
    val = act_f64(pre, c.act, slope)
    if o.get("mask") is not None:
        side = o["mask"] > 0
        if kind == "maskflip":
            side = side.clone()
            side[mutate[1:]] = ~side[mutate[1:]]
        val = val * torch.where(side, 1.0, slope).double()
    t0, ots, T_total = c.out_spec()
    if kind == "o_tstride":
        ots = 1
    ref = torch.full((N, M, T_total, V_out), BASE, dtype=torch.float64, device=dev)
    Sf = torch.zeros_like(ref)
    nf = torch.zeros_like(ref)
    ref[:, :, t0:t0 + (T_out - 1) * ots + 1:ots] = val
    Sf[:, :, t0:t0 + (T_out - 1) * ots + 1:ots] = S
    nf[:, :, t0:t0 + (T_out - 1) * ots + 1:ots] = n.view(1, 1, T_out, V_out)
    return ref, Sf, nf


def bracket(ref, S, n, nsplit=1, split_form=False, act=ACT_NONE, mask=False):
    """per-element bound on |result - ref| (module docstring); 0 where the launch writes nothing (n = S = 0: exact BASE)"""
    a, e = (6.0, 2.0 ** -6) if split_form else (1.0, 0.0)
    cc = 1 + (act == ACT_LRELU) + bool(mask) + (2 * TANH_ULP if act == ACT_TANH else 0)
    written = (ref != BASE).double()
    return ((a * n * (1.0 + e) + b_of(nsplit, split_form)) * U * S + cc * U * ref.abs()) * written


def worst_ratio(out, ref, br):
    """max over the elements of |out - ref| / bracket (0 / 0 counts as 0): <= 1 means inside the bracket everywhere"""
    err = (out.detach().double().to(ref.device) - ref).abs()
    err = torch.where(err.isnan(), torch.full_like(err, float("inf")), err)
    r = torch.where(err == 0, torch.zeros_like(err), err / br.clamp_min(1e-300))
    return float(r.max())


# ---- cases --------------------------------------------------------------------------------------------------------------------
class G(NamedTuple):
    Cin: int
    T_in: int
    V_in: int
    taps: int = 1
    tap_mode: int = TAP_TIME
    t_stride: int = 1
    transposed: bool = False
    vmap: Optional[str] = None      # None | "keep" (forward: V_out of V_in vertices, some dropped) | "inv" (transposed: inverse map)
    wkind: str = "kf"               # "kf" (taps, M, Cin) | "mf" (taps, Cin, M) | "kfpad" / "mfpad": padded strides inside a parent
                                    # | "kfblk" / "mfblk": two row blocks (w_MB < M) at w_sMB
    x_off: int = 0                  # floats the feature tensor starts inside its buffer (1: no 16-byte alignment)


class Case(NamedTuple):
    name: str
    N: int
    M: int
    T_out: int
    V_out: int
    groups: Tuple[G, ...]
    env: dict
    expect: dict
    bias0: bool = False
    bias1: bool = False
    add: Optional[int] = None       # a_tstride of the residual operand, None: no `add`
    act: int = ACT_NONE
    mask: bool = False
    out: Optional[Tuple[int, int, int]] = None     # (out_t0, out_tstride, T_total): written into a caller's tensor
    layout: str = "plane"           # storage of x / add / mask / a caller's out: "plane" (channel-major) | "nchw"
    wpack: bool = False             # the launch runs on caller-packed weights
    big: bool = False               # the float64 definition is evaluated on the device (3 G products); not in the CPU checks

    def out_spec(self):
        return self.out if self.out is not None else (0, 1, self.T_out)

    def vmap_group(self):
        for i, g in enumerate(self.groups):
            if g.vmap:
                return i
        return None

    def nterms(self):
        return sum(g.taps * g.Cin for g in self.groups)

    def weight_view(self, gi):
        g, M = self.groups[gi], self.M
        t, C = g.taps, g.Cin
        k = g.wkind
        if k == "kf":
            return WV(M * C, C, 1, numel=t * M * C)
        if k == "mf":
            return WV(C * M, 1, M, numel=t * M * C)
        if k == "kfpad":
            sO = C + 3
            sT = M * sO + 5
            return WV(sT, sO, 1, off=7, numel=7 + t * sT)
        if k == "mfpad":
            sI = M + 3
            sT = C * sI + 5
            return WV(sT, 1, sI, off=7, numel=7 + t * sT)
        MB = (M + 1) // 2
        if k == "kfblk":
            sMB = t * MB * C + 11
            return WV(MB * C, C, 1, sMB, MB, 3, 3 + 2 * sMB)
        assert k == "mfblk", k
        sMB = t * MB * C + 11
        return WV(MB * C, 1, MB, sMB, MB, 3, 3 + 2 * sMB)

    def vmap_list(self, gi):
        g = self.groups[gi]
        if g.vmap is None:
            return None
        # deterministic, with repeats impossible for "keep" when V_in >= V_out; every 7th entry (from the 3rd) dropped
        vm = [(3 + 2 * vo) % g.V_in if g.vmap == "inv" else (vo * g.V_in) // self.V_out for vo in range(self.V_out)]
        return [-1 if vo % 7 == 2 else v for vo, v in enumerate(vm)]

    def operands(self, seed, integer):
        """dict of CPU tensors: x / w / wv / vmap per group, bias0, bias1, add, mask (those the case has)"""
        gen = torch.Generator().manual_seed(seed)

        def draw(*shape, scale=1.0):
            if integer:
                return torch.randint(-3, 4, shape, generator=gen).float()
            return torch.randn(*shape, generator=gen) * scale

        o = {"x": [], "w": [], "wv": [], "vmap": []}
        wscale = 1.0 / math.sqrt(self.nterms())
        for gi, g in enumerate(self.groups):
            ch = g.Cin * (g.taps if g.tap_mode == TAP_CHANBLOCK else 1)
            o["x"].append(draw(self.N, ch, g.T_in, g.V_in))
            wv = self.weight_view(gi)
            o["w"].append(draw(wv.numel, scale=wscale))
            o["wv"].append(wv)
            vm = self.vmap_list(gi)
            o["vmap"].append(None if vm is None else torch.tensor(vm, dtype=torch.int32))
        if self.bias0:
            o["bias0"] = draw(self.M)
        if self.bias1:
            o["bias1"] = draw(self.M)
        if self.add is not None:
            o["add"] = draw(self.N, self.M, (self.T_out - 1) * self.add + 1, self.V_out)
        if self.mask:
            o["mask"] = torch.randn(self.N, self.M, self.T_out, self.V_out, generator=gen)
        return o

    def slope(self, integer):
        return SLOPE_EXACT if integer else SLOPE_FLOAT

    def act_for(self, integer):
        return ACT_NONE if (integer and self.act == ACT_TANH) else self.act

    def is_split_form(self):
        return self.expect.get("family") in ("bs", "bsw")


def on_device(o, device):
    return {k: ([None if t is None else (t.to(device) if torch.is_tensor(t) else t) for t in v] if isinstance(v, list) else v.to(device))
            for k, v in o.items()}


def reference(c, o, integer, nsplit=1, device="cpu"):
    """(ref, bracket) of the case on the operands; `device`: where the definition is evaluated (Case.big)"""
    if integer and c.act == ACT_TANH:
        c = c._replace(act=ACT_NONE)
    od = on_device(o, device) if str(device) != "cpu" else o
    ref, S, n = conv_f64(c, od, c.slope(integer))
    return ref, bracket(ref, S, n, nsplit, c.is_split_form(), c.act, c.mask)


# ---- Table A: every reachable instantiation -----------------------------------------------------------------------------------
# (BM, NW, KW) by plan tile code
TILES = {0: (128, 4, 1), 1: (64, 4, 1), 2: (32, 4, 1), 3: (64, 2, 1), 4: (32, 2, 1), 9: (32, 4, 4)}


def _direct_cases():
    cases = []
    i = 0
    for tile, (BM, NW, KW) in TILES.items():
        for KF in (1, 0):
            for FAST, PLAIN in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
                for INK in ((0, 1) if BM <= 64 else (0,)):
                    i += 1
                    kind = ("kf", "kfpad", "kfblk")[i % 3] if KF else ("mf", "mfpad", "mfblk")[i % 3]
                    Cin = 40 if FAST == 0 else 64
                    groups = (G(Cin, 9, 9, taps=3, wkind=kind),)
                    if FAST == 2:        # a 1-tap residual group through a vertex map
                        groups += (G(32, 9, 12, vmap="keep", wkind="kf" if KF else "mf"),)
                    s_total = 3 * ((Cin + 31) // 32) + (1 if FAST == 2 else 0)
                    nsplit = (2 + i % 2) if INK else 1
                    per = -(-s_total // nsplit)
                    exp = dict(family="direct", tile=tile, BM=BM, NW=NW, KW=KW, KF=KF, FAST=FAST, PLAIN=PLAIN, INK=INK,
                               nsplit=-(-s_total // per), per=per, epilogue=0, xcd=0)
                    cases.append(Case(
                        "direct t%d %s FAST%d%s%s" % (tile, "KF" if KF else "MF", FAST, " PLAIN" if PLAIN else "", " INK" if INK else ""),
                        2, 2 * BM if PLAIN else BM + 1, 9, 9, groups,
                        {"KG_CONV_PLAN": "%d,%d" % (tile, nsplit)}, exp,
                        bias0=i % 2 == 0, bias1=i % 3 == 0, add=None if PLAIN else (1, 2)[i % 2], act=(ACT_LRELU, ACT_NONE, ACT_TANH)[i % 3],
                        mask=not PLAIN and i % 4 < 2, layout=("plane", "nchw")[i % 2],
                        out=(1, 2, 20) if i % 5 == 0 else None))
    return cases


def _epilogue_cases():
    """the separate split-K epilogue launch (kg_conv_splitk_epilogue): the 128-row tile, KG_CONV_INKERNEL=0, a split count above
    KG_CONV_INKERNEL_MAX"""
    out = []
    for name, tile, env, nsplit, kw in (
            ("epilogue t0 split 3", 0, {"KG_CONV_PLAN": "0,3"}, 3, dict(add=2, mask=True, act=ACT_LRELU, bias0=True)),
            ("epilogue t2 INKERNEL=0", 2, {"KG_CONV_PLAN": "2,2", "KG_CONV_INKERNEL": "0"}, 2, dict(add=1, bias1=True, act=ACT_TANH)),
            ("epilogue t9 INKERNEL_MAX=2", 9, {"KG_CONV_PLAN": "9,3", "KG_CONV_INKERNEL_MAX": "2"}, 3, dict(mask=True, bias0=True, bias1=True)),
            ("inkernel t4 INKERNEL_MAX=6", 4, {"KG_CONV_PLAN": "4,6", "KG_CONV_INKERNEL_MAX": "6"}, 6, dict(add=1, out=(0, 2, 18)))):
        BM, NW, KW = TILES[tile]
        ink = 1 if name.startswith("inkernel") else 0
        out.append(Case(name, 2, BM + 1, 9, 9, (G(64, 9, 9, taps=3),), env,
                        dict(family="direct", tile=tile, BM=BM, NW=NW, KW=KW, KF=1, FAST=1, PLAIN=0, INK=ink, nsplit=nsplit, per=6 // nsplit,
                             epilogue=1 - ink), **kw))
    return out


def _many_sets():
    """kg_conv_many: (name, jobs, env, expected KgConvManyForm fields).  The first job has the most work and decides the shared
    tile: shapes the default plan sends to the 32- / 64- / 128-row tile with nsplit = 1 (480 workgroups of 128 columns for the
    two deep ones); the PLAIN launches have whole row tiles and neither add nor mask."""
    sets = []
    shapes = {(32, 1): (2, 64, 64, 11, 32), (32, 0): (2, 33, 64, 11, 32),              # N, M, T, V, Cin
              (64, 1): (4, 64, 480, 32, 128), (64, 0): (2, 65, 480, 32, 128),
              (128, 1): (4, 256, 240, 32, 128), (128, 0): (4, 129, 240, 32, 128)}
    for BM in (32, 64, 128):
        for KF in (1, 0):
            for PLAIN in (1, 0):
                k = "kf" if KF else "mf"
                N, M, T, V, Cin = shapes[(BM, PLAIN)]
                name = "many%d %s%s" % (BM, k, " PLAIN" if PLAIN else "")
                first = Case(name + " job0", N, M, T, V, (G(Cin, T, V, taps=3, wkind=k),), {}, {}, bias0=True, act=ACT_LRELU,
                             add=None if PLAIN else 1, big=BM > 32)
                second = Case(name + " job1", 2, BM if PLAIN else 33, 9, 9, (G(32, 9, 9, wkind=k), G(32, 9, 12, vmap="keep", wkind=k)),
                              {}, {}, bias1=True, mask=not PLAIN, out=(1, 2, 19))
                sets.append((name, (first, second), {}, dict(tile={128: 0, 64: 1, 32: 2}[BM], BM=BM, KF=KF, PLAIN=PLAIN, njobs=2, xcd=[0, 0])))
    return sets


def _tiny_cases():
    e4 = dict(family="tiny", tile=11, MT=4, nsplit=1)
    e16 = dict(family="tiny", tile=11, MT=16, nsplit=1)
    return [
        Case("tiny M3 9 terms", 2, 3, 9, 11, (G(3, 9, 11, taps=3),), {}, e4, bias0=True, act=ACT_TANH),
        Case("tiny M3 two groups add mask", 2, 3, 9, 9, (G(2, 9, 9, taps=3, wkind="kfpad"), G(3, 9, 12, vmap="keep")), {}, e4,
             add=2, mask=True, bias1=True, act=ACT_LRELU, layout="nchw"),
        Case("tiny M3 transposed stride 2", 2, 3, 10, 9, (G(3, 5, 5, taps=3, t_stride=2, transposed=True, vmap="inv", wkind="mf"),), {}, e4,
             bias0=True, out=(0, 1, 12)),
        Case("tiny M12 12 terms", 2, 12, 9, 11, (G(4, 9, 11, taps=3, wkind="kfblk"),), {}, e16, bias0=True, bias1=True),
        Case("tiny M12 chanblock add mask", 2, 12, 9, 9, (G(3, 9, 9, taps=3, tap_mode=TAP_CHANBLOCK), G(3, 9, 12, vmap="keep")), {}, e16,
             add=1, mask=True, act=ACT_LRELU),
        Case("tiny M12 transposed stride 2", 2, 12, 9, 9, (G(4, 5, 5, taps=3, t_stride=2, transposed=True, vmap="inv", wkind="mfpad"),), {},
             e16, act=ACT_TANH, layout="nchw"),
    ]


BS_TILES = {0: (2, 1, 4, 64), 1: (1, 1, 4, 32), 2: (2, 2, 2, 128)}       # variant -> TM, RWV, CWV, rows


def _bs_cases():
    out = []
    for v, (TM, RWV, CWV, BM) in BS_TILES.items():
        env = {"KG_CONV_BS": "1", "KG_CONV_BS_TILE": str(v)}
        tile = dict(tile=40 + v, TM=TM, RWV=RWV, CWV=CWV, BM=BM, nsplit=1, pack=1, wpack=0)
        win_al = (G(64, 16, 5, taps=3),)                          # T_in V_in = 80: every row, sample and gap on 16 bytes
        win_un = (G(64, 15, 5, taps=3),)                          # 75: 4-byte window loads
        # column form: a strided temporal group and a residual group, both through a vertex map
        out.append(Case("bs%d columns" % v, 2, BM + 1, 9, 9, (G(64, 18, 12, taps=3, t_stride=2, vmap="keep"), G(32, 9, 12, vmap="keep")),
                        env, dict(tile, family="bs", win=[0, 0]), bias0=True, add=2, mask=True, act=ACT_LRELU))
        out.append(Case("bs%d window 4-byte" % v, 2, BM + 1, 15, 5, win_un, env, dict(tile, family="bs", win=[1, 0]), bias1=True, act=ACT_TANH,
                        layout="nchw"))
        out.append(Case("bs%d window 16-byte BS_ASM=0" % v, 2, BM + 1, 16, 5, win_al, dict(env, KG_CONV_BS_ASM="0"),
                        dict(tile, family="bs", win=[2, 0]), add=1, bias0=True))
        out.append(Case("bs%d window unaligned pointer" % v, 2, 2 * BM, 16, 5, (win_al[0]._replace(x_off=1),), env,
                        dict(tile, family="bs", win=[1, 0]), act=ACT_LRELU))
        out.append(Case("bsw%d" % v, 2, BM + 1, 16, 5, win_al + (G(32, 16, 5),), env, dict(tile, family="bsw", win=[2, 2], PLAIN=0),
                        add=1, mask=True, bias0=True, bias1=True, act=ACT_LRELU, out=(1, 1, 18)))
        out.append(Case("bsw%d PLAIN" % v, 2, 2 * BM, 16, 5, win_al, env, dict(tile, family="bsw", win=[2, 0], PLAIN=1), bias0=True,
                        act=ACT_TANH, layout="nchw"))
    # caller-packed weights select the form with no switch set: no pack launch
    out.append(Case("bsw packed weights", 2, 64, 16, 5, (G(64, 16, 5, taps=3),), {},
                    dict(family="bsw", tile=40, TM=2, RWV=1, CWV=4, pack=0, wpack=1, PLAIN=1, win=[2, 0]), bias0=True, wpack=True))
    out.append(Case("bs packed weights columns", 2, 33, 9, 9, (G(64, 9, 12, taps=3, vmap="keep"),), {},
                    dict(family="bs", tile=40, pack=0, wpack=1, win=[0, 0]), add=1, wpack=True))
    return out


TABLE_A = _direct_cases() + _epilogue_cases() + _tiny_cases() + _bs_cases()
MANY_A = _many_sets()


def instantiation(f):
    """the compiled kernel a reported form (dict) runs, as the tuple INSTANTIATIONS lists"""
    fam = f["family"]
    if fam == "direct":
        return ("direct", f["BM"], f["NW"], f["KF"], f["KW"], f["FAST"], f["PLAIN"], f["INK"])
    if fam == "many":
        return ("many", f["BM"], f["KF"], f["PLAIN"])
    if fam == "bs":
        return ("bs", f["TM"], f["RWV"], f["CWV"])
    if fam == "bsw":
        return ("bsw", f["TM"], f["RWV"], f["CWV"], f["PLAIN"])
    assert fam == "tiny", fam
    return ("tiny", f["MT"])


# ---- Table B: logical edges ---------------------------------------------------------------------------------------------------
T0_FAST0 = {"KG_CONV_PLAN": "2,1", "KG_CONV_FAST": "0"}            # one forced direct tile with FAST 0


def _both(name, *args, forced=True, **kw):
    """the case on the default plan and on the forced direct tile with FAST 0"""
    out = [Case(name, *args, {}, {}, **kw)]
    if forced:
        out.append(Case(name + " [t2 FAST0]", *args, T0_FAST0, dict(family="direct", tile=2, FAST=0, nsplit=1), **kw))
    return out


def _edge_cases():
    out = []
    out += _both("V_out 70 vmap forward", 2, 33, 5, 70, (G(33, 5, 80, vmap="keep"),), bias0=True, act=ACT_LRELU)
    out += _both("V_out 70 vmap transposed", 2, 33, 5, 70, (G(33, 5, 25, transposed=True, vmap="inv", wkind="mf"),), add=1)
    for ncols in (1, 31, 33):
        out += _both("ncols %d" % ncols, 1, 33, 1, ncols, (G(40, 1, ncols, taps=3),), bias0=True)
    for M in (1, 2, 3, 5, 33):
        out += _both("M %d add mask" % M, 2, M, 9, 9, (G(64, 9, 9, taps=3),), add=1, mask=True, act=ACT_LRELU, bias0=True)
    for Cin in (1, 33, 63):
        out += _both("Cin %d" % Cin, 2, 33, 9, 9, (G(Cin, 9, 9, taps=3, wkind="kfpad"),), bias1=True)
    out += _both("T_in odd stride 2", 2, 33, 5, 9, (G(40, 9, 9, taps=3, t_stride=2),), bias0=True)
    # a transposed stride-2 temporal conv as two parity launches (disc_trunk.py): even output frames take the middle tap, odd
    # ones the two outer taps, the first of them on the input one frame on; each writes its parity's frames of one tensor
    out += _both("transposed stride 2 parity 0", 2, 33, 5, 9, (G(40, 5, 9, wkind="mf"),), out=(0, 2, 10), bias0=True)
    out += _both("transposed stride 2 parity 1", 2, 33, 5, 9, (G(40, 5, 9, wkind="mf"), G(40, 4, 9, wkind="mf")), out=(1, 2, 10), bias0=True)
    out += _both("w_MB < M row blocks", 2, 40, 9, 9, (G(64, 9, 9, taps=3, wkind="kfblk"), G(32, 9, 9, wkind="kfblk")), bias0=True)
    # forced splits on a two-group launch with 3 + 1 taps: 7 slices in 64 + 32 channels -> a split (and, K32x32, a wave) starts
    # inside group 1 and in the middle of a chunk's taps; 7 slices in 3 / 5 / 2 splits do not divide
    for plan, ns, per in (("2,3", 3, 3), ("4,5", 4, 2), ("9,2", 2, 4), ("1,4", 4, 2)):
        t = int(plan.split(",")[0])
        BM, NW, KW = TILES[t]
        out.append(Case("forced split %s two groups" % plan, 2, 33, 9, 9, (G(64, 9, 9, taps=3), G(32, 9, 12, vmap="keep")),
                        {"KG_CONV_PLAN": plan}, dict(family="direct", tile=t, BM=BM, KW=KW, FAST=2, nsplit=ns, per=per, INK=1 if ns <= 4 else 0),
                        bias0=True, add=1, act=ACT_LRELU))
    out.append(Case("forced split 2,7 INKERNEL_MAX 8", 2, 33, 9, 9, (G(64, 9, 9, taps=3), G(32, 9, 12, vmap="keep")),
                    {"KG_CONV_PLAN": "2,7", "KG_CONV_INKERNEL_MAX": "8"},
                    dict(family="direct", tile=2, FAST=2, nsplit=7, per=1, INK=1), mask=True))
    out.append(Case("K32x32 workgroup split", 2, 64, 2, 2, (G(512, 2, 2),), {},
                    dict(family="direct", tile=9, KW=4, BM=32, nsplit=2, per=8, INK=1, FAST=1), bias0=True, act=ACT_LRELU))
    out.append(Case("XCD order 67 column tiles", 5, 64, 34, 50, (G(32, 34, 50, taps=3),), {"KG_CONV_XCD_MIN": "1"},
                    dict(family="direct", tile=2, xcd=1, grid_x=72 * 2, grid_y=1, nsplit=1), bias0=True, act=ACT_LRELU))
    for a in (ACT_NONE, ACT_LRELU, ACT_TANH):
        out += _both("act %d" % a, 2, 33, 9, 9, (G(40, 9, 9, taps=3),), act=a, bias0=True, bias1=True, forced=False)
    # the switches that take a launch OFF a form: the lean epilogue, the wave-level K-split tile, the tiny kernel
    out.append(Case("PLAIN_EPI=0 on a lean launch", 2, 64, 9, 9, (G(64, 9, 9, taps=3),), {"KG_CONV_PLAN": "2,1", "KG_CONV_PLAIN_EPI": "0"},
                    dict(family="direct", tile=2, FAST=1, PLAIN=0, nsplit=1), bias0=True, act=ACT_LRELU))
    out.append(Case("KW=0 on the K32x32 shape", 2, 64, 2, 2, (G(512, 2, 2),), {"KG_CONV_KW": "0"},
                    dict(family="direct", tile=2, KW=1, FAST=1, PLAIN=1, nsplit=8, INK=0, epilogue=1), bias0=True, act=ACT_LRELU))
    out.append(Case("TINY=0 on a tiny shape", 2, 3, 9, 11, (G(3, 9, 11, taps=3),), {"KG_CONV_TINY": "0"},
                    dict(family="direct", tile=4, FAST=0, nsplit=1), bias0=True, act=ACT_TANH))
    out += _both("bias1 without bias0", 2, 33, 9, 9, (G(64, 9, 9),), bias1=True)
    out += _both("a_tstride 2", 2, 33, 9, 9, (G(64, 9, 9),), add=2, layout="nchw")
    return out


TABLE_B = _edge_cases()
_xcd = next(c for c in TABLE_B if c.name.startswith("XCD order"))
MANY_B = [
    # three jobs, one of them the XCD shape (an XCD-grouped job next to plain ones in the shared launch)
    ("many three jobs one XCD",
     (Case("job0", 2, 32, 9, 9, (G(32, 9, 9, taps=3),), {}, {}, bias0=True),
      _xcd._replace(name="job1 xcd", env={}, expect={}),
      Case("job2", 2, 64, 9, 9, (G(64, 9, 9), G(32, 9, 12, vmap="keep")), {}, {}, bias1=True, out=(0, 2, 17))),
     {"KG_CONV_XCD_MIN": "1"}, dict(tile=2, BM=32, KF=1, PLAIN=1, njobs=3, xcd=[0, 1, 0], wg_begin=[0, 8, 152], nwg=[2, 134, 4], total_wg=160)),
    # a job with partial K-slices: one launch per job
    ("many falls back to single launches",
     (Case("job0", 2, 33, 9, 9, (G(40, 9, 9, taps=3),), {}, {}, bias0=True),
      Case("job1", 2, 32, 9, 9, (G(32, 9, 9),), {}, {}, add=1)),
     {}, dict(tile=-1, njobs=2)),
    ("many switched off", MANY_A[0][1], {"KG_CONV_MANY": "0"}, dict(tile=-1, njobs=2)),
]

# what the default plan gives the Table B cases that force nothing: asserted by the GPU tests from the form record, pinned on the
# host by tests/test_conv_def_cpu.py
DEFAULT_FORMS = {
    'V_out 70 vmap forward': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'V_out 70 vmap transposed': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 0, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'ncols 1': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'ncols 31': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'ncols 33': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'M 1 add mask': {'family': 'direct', 'tile': 4, 'nsplit': 1, 'KF': 1, 'FAST': 1, 'PLAIN': 0, 'INK': 0},
    'M 2 add mask': {'family': 'direct', 'tile': 4, 'nsplit': 1, 'KF': 1, 'FAST': 1, 'PLAIN': 0, 'INK': 0},
    'M 3 add mask': {'family': 'direct', 'tile': 4, 'nsplit': 1, 'KF': 1, 'FAST': 1, 'PLAIN': 0, 'INK': 0},
    'M 5 add mask': {'family': 'direct', 'tile': 4, 'nsplit': 1, 'KF': 1, 'FAST': 1, 'PLAIN': 0, 'INK': 0},
    'M 33 add mask': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 1, 'PLAIN': 0, 'INK': 0},
    'Cin 1': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'Cin 33': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'Cin 63': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'T_in odd stride 2': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'transposed stride 2 parity 0': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 0, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'transposed stride 2 parity 1': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 0, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'w_MB < M row blocks': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 2, 'PLAIN': 0, 'INK': 0},
    'act 0': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'act 1': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'act 2': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 0, 'PLAIN': 0, 'INK': 0},
    'bias1 without bias0': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 1, 'PLAIN': 0, 'INK': 0},
    'a_tstride 2': {'family': 'direct', 'tile': 2, 'nsplit': 1, 'KF': 1, 'FAST': 1, 'PLAIN': 0, 'INK': 0},
}

CASES = {c.name: c for c in TABLE_A + TABLE_B}
assert len(CASES) == len(TABLE_A) + len(TABLE_B), "case names must be unique"
MANY = {m[0]: m for m in MANY_A + MANY_B}
assert len(MANY) == len(MANY_A) + len(MANY_B)

# The compiled instantiations a launch can reach (the dispatch code of csrc/kg_conv.hip: launch<>(), launch_bs(), launch_tiny(),
# kg_conv_many()).  ("direct", BM, NW, KF, KW, FAST, PLAIN, INK) | ("many", BM, KF, PLAIN) | ("bs", TM, RWV, CWV) |
# ("bsw", TM, RWV, CWV, PLAIN) | ("tiny", MT)
INSTANTIATIONS = [
    ("direct", 128, 4, 1, 1, 0, 0, 0), ("direct", 128, 4, 1, 1, 1, 0, 0), ("direct", 128, 4, 1, 1, 1, 1, 0), ("direct", 128, 4, 1, 1, 2, 0, 0), ("direct", 128, 4, 1, 1, 2, 1, 0),
    ("direct", 128, 4, 0, 1, 0, 0, 0), ("direct", 128, 4, 0, 1, 1, 0, 0), ("direct", 128, 4, 0, 1, 1, 1, 0), ("direct", 128, 4, 0, 1, 2, 0, 0), ("direct", 128, 4, 0, 1, 2, 1, 0),
    ("direct", 64, 4, 1, 1, 0, 0, 0), ("direct", 64, 4, 1, 1, 0, 0, 1), ("direct", 64, 4, 1, 1, 1, 0, 0), ("direct", 64, 4, 1, 1, 1, 0, 1), ("direct", 64, 4, 1, 1, 1, 1, 0),
    ("direct", 64, 4, 1, 1, 1, 1, 1), ("direct", 64, 4, 1, 1, 2, 0, 0), ("direct", 64, 4, 1, 1, 2, 0, 1), ("direct", 64, 4, 1, 1, 2, 1, 0), ("direct", 64, 4, 1, 1, 2, 1, 1),
    ("direct", 64, 4, 0, 1, 0, 0, 0), ("direct", 64, 4, 0, 1, 0, 0, 1), ("direct", 64, 4, 0, 1, 1, 0, 0), ("direct", 64, 4, 0, 1, 1, 0, 1), ("direct", 64, 4, 0, 1, 1, 1, 0),
    ("direct", 64, 4, 0, 1, 1, 1, 1), ("direct", 64, 4, 0, 1, 2, 0, 0), ("direct", 64, 4, 0, 1, 2, 0, 1), ("direct", 64, 4, 0, 1, 2, 1, 0), ("direct", 64, 4, 0, 1, 2, 1, 1),
    ("direct", 32, 4, 1, 1, 0, 0, 0), ("direct", 32, 4, 1, 1, 0, 0, 1), ("direct", 32, 4, 1, 1, 1, 0, 0), ("direct", 32, 4, 1, 1, 1, 0, 1), ("direct", 32, 4, 1, 1, 1, 1, 0),
    ("direct", 32, 4, 1, 1, 1, 1, 1), ("direct", 32, 4, 1, 1, 2, 0, 0), ("direct", 32, 4, 1, 1, 2, 0, 1), ("direct", 32, 4, 1, 1, 2, 1, 0), ("direct", 32, 4, 1, 1, 2, 1, 1),
    ("direct", 32, 4, 0, 1, 0, 0, 0), ("direct", 32, 4, 0, 1, 0, 0, 1), ("direct", 32, 4, 0, 1, 1, 0, 0), ("direct", 32, 4, 0, 1, 1, 0, 1), ("direct", 32, 4, 0, 1, 1, 1, 0),
    ("direct", 32, 4, 0, 1, 1, 1, 1), ("direct", 32, 4, 0, 1, 2, 0, 0), ("direct", 32, 4, 0, 1, 2, 0, 1), ("direct", 32, 4, 0, 1, 2, 1, 0), ("direct", 32, 4, 0, 1, 2, 1, 1),
    ("direct", 64, 2, 1, 1, 0, 0, 0), ("direct", 64, 2, 1, 1, 0, 0, 1), ("direct", 64, 2, 1, 1, 1, 0, 0), ("direct", 64, 2, 1, 1, 1, 0, 1), ("direct", 64, 2, 1, 1, 1, 1, 0),
    ("direct", 64, 2, 1, 1, 1, 1, 1), ("direct", 64, 2, 1, 1, 2, 0, 0), ("direct", 64, 2, 1, 1, 2, 0, 1), ("direct", 64, 2, 1, 1, 2, 1, 0), ("direct", 64, 2, 1, 1, 2, 1, 1),
    ("direct", 64, 2, 0, 1, 0, 0, 0), ("direct", 64, 2, 0, 1, 0, 0, 1), ("direct", 64, 2, 0, 1, 1, 0, 0), ("direct", 64, 2, 0, 1, 1, 0, 1), ("direct", 64, 2, 0, 1, 1, 1, 0),
    ("direct", 64, 2, 0, 1, 1, 1, 1), ("direct", 64, 2, 0, 1, 2, 0, 0), ("direct", 64, 2, 0, 1, 2, 0, 1), ("direct", 64, 2, 0, 1, 2, 1, 0), ("direct", 64, 2, 0, 1, 2, 1, 1),
    ("direct", 32, 2, 1, 1, 0, 0, 0), ("direct", 32, 2, 1, 1, 0, 0, 1), ("direct", 32, 2, 1, 1, 1, 0, 0), ("direct", 32, 2, 1, 1, 1, 0, 1), ("direct", 32, 2, 1, 1, 1, 1, 0),
    ("direct", 32, 2, 1, 1, 1, 1, 1), ("direct", 32, 2, 1, 1, 2, 0, 0), ("direct", 32, 2, 1, 1, 2, 0, 1), ("direct", 32, 2, 1, 1, 2, 1, 0), ("direct", 32, 2, 1, 1, 2, 1, 1),
    ("direct", 32, 2, 0, 1, 0, 0, 0), ("direct", 32, 2, 0, 1, 0, 0, 1), ("direct", 32, 2, 0, 1, 1, 0, 0), ("direct", 32, 2, 0, 1, 1, 0, 1), ("direct", 32, 2, 0, 1, 1, 1, 0),
    ("direct", 32, 2, 0, 1, 1, 1, 1), ("direct", 32, 2, 0, 1, 2, 0, 0), ("direct", 32, 2, 0, 1, 2, 0, 1), ("direct", 32, 2, 0, 1, 2, 1, 0), ("direct", 32, 2, 0, 1, 2, 1, 1),
    ("direct", 32, 4, 1, 4, 0, 0, 0), ("direct", 32, 4, 1, 4, 0, 0, 1), ("direct", 32, 4, 1, 4, 1, 0, 0), ("direct", 32, 4, 1, 4, 1, 0, 1), ("direct", 32, 4, 1, 4, 1, 1, 0),
    ("direct", 32, 4, 1, 4, 1, 1, 1), ("direct", 32, 4, 1, 4, 2, 0, 0), ("direct", 32, 4, 1, 4, 2, 0, 1), ("direct", 32, 4, 1, 4, 2, 1, 0), ("direct", 32, 4, 1, 4, 2, 1, 1),
    ("direct", 32, 4, 0, 4, 0, 0, 0), ("direct", 32, 4, 0, 4, 0, 0, 1), ("direct", 32, 4, 0, 4, 1, 0, 0), ("direct", 32, 4, 0, 4, 1, 0, 1), ("direct", 32, 4, 0, 4, 1, 1, 0),
    ("direct", 32, 4, 0, 4, 1, 1, 1), ("direct", 32, 4, 0, 4, 2, 0, 0), ("direct", 32, 4, 0, 4, 2, 0, 1), ("direct", 32, 4, 0, 4, 2, 1, 0), ("direct", 32, 4, 0, 4, 2, 1, 1),
    ("many", 32, 1, 1), ("many", 32, 1, 0), ("many", 32, 0, 1), ("many", 32, 0, 0), ("many", 64, 1, 1), ("many", 64, 1, 0), ("many", 64, 0, 1), ("many", 64, 0, 0),
    ("many", 128, 1, 1), ("many", 128, 1, 0), ("many", 128, 0, 1), ("many", 128, 0, 0),
    ("bs", 2, 1, 4), ("bs", 1, 1, 4), ("bs", 2, 2, 2),
    ("bsw", 2, 1, 4, 0), ("bsw", 2, 1, 4, 1), ("bsw", 1, 1, 4, 0), ("bsw", 1, 1, 4, 1), ("bsw", 2, 2, 2, 0), ("bsw", 2, 2, 2, 1),
    ("tiny", 4), ("tiny", 16),
]
assert len(INSTANTIATIONS) == len(set(INSTANTIATIONS)) == 133
