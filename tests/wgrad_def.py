"""Float64 definition of the weight gradient of the tap GEMM (kg_wgrad / kg_wgrad_many, include/kgan_hip.h), the bracket a
correct kernel must land in, and the test data and case tables of tests/test_wgrad_def_cpu.py and
tests/test_wgrad_tiles_gpu.py.  Test code only: torch on the CPU, plain loops and einsums on doubles (nothing of
oracle/prim_ref.py is called).

  dW(d, m, c) = sum over the operand pairs p and their columns j = (n, to, vo) of  G_p[m, j] * X_p[c (+ d Cin), src(j, d)]
  src(j, d) = (n, ti, vi):  time taps     ti = to * t_stride + d - (taps - 1) / 2   (a product with ti outside [0, T_in) is 0)
                            channel blocks ti = to * t_stride, the channel is c + d Cin
              vi = vmap[vo] (a product with vmap[vo] < 0 - a dropped vertex - is 0), or vo without a map
written to  dw[d w_sT + m w_sO + c w_sI]  (+= with `accumulate`: `base` is what the destination held).

Error bracket (derived, not measured).  u = 2^-24 (fp32 round to nearest), S = the same sum over |G| |X|, K = the number of
contracted columns, all pairs together.  Per element a kernel's result r must satisfy

    |r - ref| <= (a K (1 + e) + b) u S + u |ref|.

fp32 tiles, a = 1, e = 0.  Every product enters a tree of additions whose leaves are the element's (at most K) non-zero
products: MFMA steps inside a chunk, the waves' accumulators through LDS, the partial slabs, all in some fixed order.  A
product is rounded at most once when it is formed (not at all by a fused multiply-add) and once per addition on its way to
the root; a tree with K leaves has at most K - 1 additions on any path, and additions of an exact zero (padding columns,
rows beyond M / Cin, the zero an accumulator starts from) round nothing.  So r_sum = sum_i p_i (1 + t_i) with
|t_i| <= (1 + u)^K - 1 <= K u / (1 - K u): the classical bound, valid in ANY order.  b = 40 pays, a second time and
separately, for what is added outside the MFMA chain - 3 additions of the four waves' accumulators, at most 35 on a path of
the slab reduction (130 slabs in four interleaved chains and a 4-way tree) - plus 1 for the second-order part of the bound
above (K u <= 2^-9 for every K used here) and 1 spare.  The final `base + sum` (or the store of the sum) is one more
rounding of the RESULT: u |ref| to first order; its second-order part is inside the spare of b.

bf16-split tiles, a = 6, e = 2^-6, b = 43.  Each operand is split x = h + m + l into three bf16 numbers (8 significant bits,
round to nearest: |x - h| <= 2^-8 |x|, so |m| <= 2^-8 (1 + 2^-8) |x|; |x - h - m| <= 2^-8 |x - h| <= 2^-16 |x| has at most 8
significant bits left, so l is exact and the three terms sum to x exactly).  Of the nine products of (gh + gm + gl)
(xh + xm + xl) six are kept - hh, hm, mh, mm, hl, lh - and three dropped: |gm xl|, |gl xm| <= 2^-24 (1 + 2^-8) |g x| each and
|gl xl| <= 2^-32 |g x|.  Each is below 2^-24 (1 + 2^-8) of the product (what the source comment states), all three together
below 3 * 2^-24 |g x|: 3 of b.  The kept products are exact in fp32 (16 significant bits) and are added in fp32, six per
column: a tree of 6 K leaves, (6 K) u times the sum of their magnitudes, which is at most
(1 + 2^-8)^2 (1 + 2 * 2^-8 + 3 * 2^-16) S < (1 + 2^-6) S: the factor (1 + e).  The other 40 of b as above.

Exact cases.  `integer_case` draws every operand from the integers -3 .. 3 and an integer `base`: every product and every
partial sum of any subset of products is an integer of magnitude <= 9 K + |base| < 2^24, so every fp32 operation of every
summation order is exact, and every operand is a bf16 number (h = x, m = l = 0), so the split form is exact too.  On such
data a kernel equals this definition bit for bit at any column count.
"""
from typing import NamedTuple, Optional, Tuple

import torch

TAP_TIME, TAP_CHANBLOCK = 0, 1
U = 2.0 ** -24
B_FP32, B_SPLIT = 40, 43
K_FLOAT_MAX = 512            # float cases stay at or below this many columns (the mutation check of test_wgrad_def_cpu.py)


class WV(NamedTuple):        # the fields of _native.WView this file reads
    sT: int
    sO: int
    sI: int


def _src(x, Cin, d, taps, tap_mode, t_stride, vmap, T_out, V_out, shifted=None):
    """(N, Cin, T_out, V_out) float64: X at the source of every column for tap d, 0 where there is none.
    shifted = (n, to, vo): that one column reads one time step later (a mutation for the tests of the tests)."""
    N, _, T_in, V_in = x.shape
    shift = d - (taps - 1) // 2 if tap_mode == TAP_TIME else 0
    ch0 = d * Cin if tap_mode == TAP_CHANBLOCK else 0
    vmap_l = list(range(V_out)) if vmap is None else [int(v) for v in vmap]
    assert len(vmap_l) == V_out and all(v < V_in for v in vmap_l)
    vo_ok = [vo for vo in range(V_out) if vmap_l[vo] >= 0]
    vi_ok = [vmap_l[vo] for vo in vo_ok]
    out = torch.zeros(N, Cin, T_out, V_out, dtype=torch.float64)
    for to in range(T_out):
        ti = to * t_stride + shift
        if 0 <= ti < T_in and vo_ok:
            out[:, :, to, vo_ok] = x[:, ch0:ch0 + Cin, ti, vi_ok].double()
    if shifted is not None:
        n, to, vo = shifted
        ti = to * t_stride + shift + 1
        out[n, :, to, vo] = x[n, ch0:ch0 + Cin, ti, vmap_l[vo]].double() if 0 <= ti < T_in and vmap_l[vo] >= 0 else 0.0
    return out


def _index(wv, taps, M, Cin):
    d = torch.arange(taps).view(-1, 1, 1)
    m = torch.arange(M).view(1, -1, 1)
    c = torch.arange(Cin).view(1, 1, -1)
    return (d * wv.sT + m * wv.sO + c * wv.sI).reshape(-1)


def _sum(pairs, Cin, taps, tap_mode, t_stride, vmap, absolute, mutate):
    vals = None
    for p, (g, x) in enumerate(pairs):
        g = g.double()
        x = x.double()
        shifted = None
        if mutate is not None and mutate[1] == p:
            kind, _, n, to, vo = mutate
            if kind == "drop":
                g = g.clone()
                g[n, :, to, vo] = 0.0
            else:
                assert kind == "shift"
                shifted = (n, to, vo)
        if absolute:
            g, x = g.abs(), x.abs()
        _, M, T_out, V_out = g.shape
        v = torch.stack([torch.einsum("nmtv,nctv->mc", g, _src(x, Cin, d, taps, tap_mode, t_stride, vmap, T_out, V_out, shifted))
                         for d in range(taps)])
        vals = v if vals is None else vals + v
    return vals                     # (taps, M, Cin) float64


def wgrad_f64(g, x, Cin, taps, tap_mode, t_stride, vmap, wv, numel, extra=(), base=None, mutate=None):
    """(numel,) float64: the gradient at the positions the weight view addresses, `base` (or 0) everywhere else; with `base`
    the call accumulates.  mutate = ("drop" | "shift", pair, n, to, vo): one column's products left out / read one time
    step later - NOT the definition, for the mutation check."""
    vals = _sum([(g, x)] + list(extra), Cin, taps, tap_mode, t_stride, vmap, False, mutate)
    idx = _index(wv, taps, g.shape[1], Cin)
    assert idx.unique().numel() == idx.numel() and int(idx.max()) < numel, "the weight view addresses an element twice"
    out = torch.zeros(numel, dtype=torch.float64) if base is None else base.double().clone()
    out[idx] = out[idx] + vals.reshape(-1)
    return out


def wgrad_abs_f64(g, x, Cin, taps, tap_mode, t_stride, vmap, wv, numel, extra=(), base=None):
    """S: the same sum over |G| |X| (0 at positions the view does not address; `base` does not enter)."""
    vals = _sum([(g, x)] + list(extra), Cin, taps, tap_mode, t_stride, vmap, True, None)
    out = torch.zeros(numel, dtype=torch.float64)
    out[_index(wv, taps, g.shape[1], Cin)] = vals.reshape(-1)
    return out


def bracket(ref, S, K, split=False):
    """per-element bound on |result - ref| (module docstring)"""
    a, e, b = (6.0, 2.0 ** -6, B_SPLIT) if split else (1.0, 0.0, B_FP32)
    return (a * K * (1.0 + e) + b) * U * S + U * ref.abs()


def worst_ratio(out, ref, S, K, split=False):
    """max over the elements of |out - ref| / bracket (0 / 0 counts as 0): <= 1 means inside the bracket everywhere"""
    err = (out.detach().double().cpu().reshape(-1) - ref).abs()
    br = bracket(ref, S, K, split)
    r = torch.where(err == 0, torch.zeros_like(err), err / br.clamp_min(1e-300))
    return float(r.max())


# ---- cases ----------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    Ns: Tuple[int, ...]          # batch size of every operand pair
    Cin: int
    M: int
    T: int                       # input frames; T_out = T // stride
    V: int                       # input vertices
    taps: int
    mode: int
    stride: int
    vmap: Optional[Tuple[int, ...]] = None      # V_out entries, -1 = dropped vertex

    @property
    def T_out(self):
        return self.T // self.stride

    @property
    def V_out(self):
        return self.V if self.vmap is None else len(self.vmap)

    @property
    def K(self):
        return sum(self.Ns) * self.T_out * self.V_out

    @property
    def x_channels(self):
        return self.Cin * (self.taps if self.mode == TAP_CHANBLOCK else 1)

    def view(self):
        """(weight view, elements) as the layers of the model address their weights"""
        if self.mode == TAP_CHANBLOCK:
            return WV(self.M * self.Cin, self.Cin, 1), self.taps * self.M * self.Cin
        if self.vmap is not None and self.taps == 1:
            return WV(0, self.Cin, 1), self.M * self.Cin
        return WV(1, self.Cin * self.taps, self.taps), self.M * self.Cin * self.taps

    def short(self):
        """the same layer with fewer frames / samples: at most K_FLOAT_MAX columns (float data)"""
        c = self
        while c.K > K_FLOAT_MAX and c.T % (2 * c.stride) == 0 and c.T // 2 >= c.stride:
            c = c._replace(T=c.T // 2)
        while c.K > K_FLOAT_MAX and max(c.Ns) > 1:
            c = c._replace(Ns=tuple(max(1, n // 2) for n in c.Ns))
        assert c.K <= K_FLOAT_MAX, c
        return c


# the twelve edge shapes of tests/test_kernels_gpu.py (WG_CASES: N, Cin, M, T, V, taps, mode, stride) and its vertex-gather shape
WG_SHAPES = [(2, 63, 32, 64, 11, 3, TAP_CHANBLOCK, 1), (2, 32, 64, 64, 11, 3, TAP_TIME, 1), (2, 64, 128, 64, 5, 3, TAP_TIME, 2),
             (4, 512, 512, 8, 1, 3, TAP_TIME, 2), (2, 572, 1536, 1, 1, 1, TAP_TIME, 1), (2, 3, 9, 64, 25, 1, TAP_TIME, 1),
             (3, 70, 65, 10, 7, 3, TAP_TIME, 2), (2, 256, 512, 16, 5, 1, TAP_TIME, 2), (2, 40, 70, 64, 25, 3, TAP_TIME, 1),
             (5, 33, 20, 9, 16, 3, TAP_TIME, 1), (3, 16, 16, 12, 2, 3, TAP_CHANBLOCK, 1), (1, 1, 1, 1, 1, 3, TAP_TIME, 1)]
GATHER = Case("gather", (2,), 30, 20, 8, 11, 1, TAP_TIME, 2, (2, 4, 6, 8, 10))
SMALL_CASES = [Case("wg%d" % i, (s[0],), *s[1:]) for i, s in enumerate(WG_SHAPES)] + [GATHER]

# the 128 x 128 tile at small column counts (KG_WGRAD_BIGCOLS=0 in the GPU tests)
BIG_CASES = [
    Case("full 256x128", (2,), 128, 256, 8, 5, 3, TAP_TIME, 1),
    Case("ragged 130x200, pairs", (2, 1), 200, 130, 6, 7, 3, TAP_TIME, 1),
    Case("ragged 129x255, 70 columns", (2,), 255, 129, 5, 7, 1, TAP_TIME, 1),
    Case("one column", (1,), 128, 128, 1, 1, 3, TAP_TIME, 1),
    Case("stride 2, time padding", (2,), 129, 130, 10, 3, 3, TAP_TIME, 2),
    Case("channel blocks", (2,), 130, 128, 4, 5, 3, TAP_CHANBLOCK, 1),
    Case("vertex map with dropped entries, stride 2", (3,), 128, 256, 8, 11, 1, TAP_TIME, 2, (2, 4, -1, 8, 10)),
    Case("ragged 200x136, 400 columns", (2,), 136, 200, 8, 25, 3, TAP_TIME, 1),          # more than 256 columns: two splits
]
# the default plan's 128 x 128 tile: exactly 4096 columns, alone and as three operand pairs
BIG_DEFAULT = [Case("default 4096", (8,), 128, 128, 32, 16, 3, TAP_TIME, 1),
               Case("default 4096, pairs", (3, 3, 2), 128, 128, 32, 16, 3, TAP_TIME, 1)]
# split classes (the GPU test asserts each from the reported plan)
CAP_CASE = Case("128 splits", (3,), 8, 8, 109, 100, 1, TAP_TIME, 1)             # 32700 columns: 256 chunks of the 32 x 32 tile
SHORT_LAST = Case("short last split", (1, 2), 40, 70, 50, 11, 3, TAP_TIME, 1)   # 550 + 1100 columns: 9 + 18 chunks of 64

FLOAT_CASES = [c.short() for c in SMALL_CASES] + BIG_CASES          # every case that runs on float data


def operands(case, seed, integer):
    """([(g, x)] per operand pair, base): seeded operands of `case` in NCHW, integers -3 .. 3 or standard normal"""
    gen = torch.Generator().manual_seed(seed)

    def draw(*shape):
        if integer:
            return torch.randint(-3, 4, shape, generator=gen).float()
        return torch.randn(*shape, generator=gen)
    pairs = [(draw(n, case.M, case.T_out, case.V_out), draw(n, case.x_channels, case.T, case.V)) for n in case.Ns]
    _, numel = case.view()
    return pairs, draw(numel)


def integer_case(seed, case):
    """operands with integer values in [-3, 3] and an integer base: 9 K + 3 < 2^24, every fp32 partial sum is exact"""
    assert 9 * case.K + 3 < 2 ** 24
    return operands(case, seed, True)


def reference(case, pairs, base=None, mutate=None):
    """(ref, S, K) of a case's operands"""
    wv, numel = case.view()
    args = (pairs[0][0], pairs[0][1], case.Cin, case.taps, case.mode, case.stride, case.vmap, wv, numel)
    ref = wgrad_f64(*args, extra=pairs[1:], base=base, mutate=mutate)
    S = wgrad_abs_f64(*args, extra=pairs[1:])
    return ref, S, case.K


def pick_column(case, seed):
    """(pair, n, to, vo) of one column chosen by seed among those with a source vertex"""
    gen = torch.Generator().manual_seed(1000 + seed)
    r = lambda n: int(torch.randint(0, n, (1,), generator=gen))
    p = r(len(case.Ns))
    vos = [vo for vo in range(case.V_out) if case.vmap is None or case.vmap[vo] >= 0]
    return p, r(case.Ns[p]), r(case.T_out), vos[r(len(vos))]


# ---- launches of the GPU tests and what the plan report must say about them ----------------------------------------------------
# tile variants (KG_WGRAD_TILE_* of include/kgan_hip.h) and the columns of one chunk of each (TILES[] of csrc/kg_wgrad.hip)
T128, T6464, T6432, T3264, T3232 = 0, 1, 2, 3, 4
CHUNK = {T128: 32, T6464: 64, T6432: 64, T3264: 64, T3232: 128}
MAX_SPLITS = 128
SMALL_VARIANTS = [T3264, T6432, T6464, T6464, T6464, T3232, T6464, T6464, T6464, T3264, T3232, T3232, T3232]   # of SMALL_CASES


def _cdiv(a, b):
    return -(-a // b)


def has_short_last_split(case, variant, splits):
    """the plan cuts every pair into ranges of `per` chunks: true when some pair's chunk count is no multiple of it"""
    chunks = [_cdiv(n * case.T_out * case.V_out, CHUNK[variant]) for n in case.Ns]
    pers = [p for p in range(1, sum(chunks) + 1) if sum(_cdiv(c, p) for c in chunks) == splits]
    return bool(pers) and all(any(c % p for c in chunks) for p in pers)


SPLIT_CLASSES = {
    "one": lambda cases, plan: all(s == 1 for _, s in plan),                      # the tile kernel writes dw itself
    "several": lambda cases, plan: all(s > 1 for _, s in plan),                   # the slab-only instantiation
    "mixed": lambda cases, plan: any(s == 1 for _, s in plan) and any(s > 1 for _, s in plan),
    "2 to 7": lambda cases, plan: any(2 <= s <= 7 for _, s in plan),
    "over 8 with remainder": lambda cases, plan: any(s > 8 and s % 8 for _, s in plan),     # both branches of the XCD order
    "cap": lambda cases, plan: any(s == MAX_SPLITS for _, s in plan),
    "short last split": lambda cases, plan: any(has_short_last_split(c, v, s) for c, (v, s) in zip(cases, plan)),
}


class Launch(NamedTuple):
    cases: list
    env: dict
    variants: Optional[list]         # per job, None = not pinned by this launch
    classes: Tuple[str, ...]         # keys of SPLIT_CLASSES that must hold

    def check(self, cases, plan):
        assert len(plan) == len(self.cases)
        if self.variants is not None:
            assert [v for v, _ in plan] == list(self.variants), plan
        for k in self.classes:
            assert SPLIT_CLASSES[k](cases, plan), (k, plan)
        assert all(1 <= s <= MAX_SPLITS + 2 for _, s in plan), plan


FORCE_BIG = {"KG_WGRAD_BIGCOLS": "0"}
LAUNCHES = {
    "default plan, 128x128, 4096 columns": Launch([BIG_DEFAULT[0]], {}, [T128], ("several",)),
    "default plan, 128x128, three pairs": Launch([BIG_DEFAULT[1]], {}, [T128], ("several",)),
    "forced 128x128, all shapes in one call": Launch(BIG_CASES, FORCE_BIG, [T128] * len(BIG_CASES), ("mixed",)),
    "small tiles, all shapes in one call": Launch(SMALL_CASES, {}, SMALL_VARIANTS, ("mixed", "2 to 7", "over 8 with remainder")),
    "small tiles, short float shapes in one call": Launch([c.short() for c in SMALL_CASES], {}, SMALL_VARIANTS, ("mixed", "2 to 7")),
    "one split": Launch([SMALL_CASES[6]], {}, [T6464], ("one",)),
    "every job several splits": Launch([SMALL_CASES[i] for i in (0, 1, 5, 8, 9)], {}, [T3264, T6432, T3232, T6464, T3264],
                                       ("several", "2 to 7", "over 8 with remainder")),
    "128 splits": Launch([CAP_CASE], {"KG_WGRAD_BUDGET": "100000"}, [T3232], ("cap",)),
    "128 splits next to a small job": Launch([SMALL_CASES[10], CAP_CASE], {"KG_WGRAD_BUDGET": "100000"}, [T3232, T3232], ("cap", "mixed")),
    "short last split": Launch([SHORT_LAST], {}, [T6464], ("short last split", "several")),
    "short last split, 128x128": Launch([BIG_DEFAULT[1]._replace(name="4320 columns, pairs", Ns=(3, 2, 4), T=30)], {}, [T128],
                                        ("short last split", "over 8 with remainder")),
}
for _i, _c in enumerate(BIG_CASES):
    LAUNCHES["forced 128x128: " + _c.name] = Launch([_c], FORCE_BIG, [T128], ("several",) if len(_c.Ns) > 1 or _c.K > 256 else ("one",))
for _i, _c in enumerate(SMALL_CASES):
    LAUNCHES["small tile %d: %s" % (SMALL_VARIANTS[_i], _c.name)] = Launch([_c], {}, [SMALL_VARIANTS[_i]], ())
    LAUNCHES["small tile %d: short %s" % (SMALL_VARIANTS[_i], _c.name)] = Launch([_c.short()], {}, [SMALL_VARIANTS[_i]], ())
