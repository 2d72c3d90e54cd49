"""Float64 definitions of the graph-aggregation kernels (kg_agg_expand / kg_agg_reduce / kg_agg_outer / kg_agg_outer_many /
kg_aggconv / kg_aggconv_label, include/kgan_hip.h), the bracket a correct kernel must land in, and the test data and launch
tables of tests/test_agg_def_cpu.py and tests/test_agg_forms_gpu.py.  Test code only: torch on the CPU, plain loops and
einsums on doubles (nothing of oracle/prim_ref.py is called).

  expand : out[n, k C + c, t', w] = sum_v x[n, c, t' // rep, v] A[k, v, w]                                  t' < T rep
  reduce : out[n, c, t, w] = ( sum_{q < fold} sum_k sum_v y[n, k C + c, t fold + q, v] A[k, v, w]
                               + [t % s == 0 and t / s < r_T and inv[w] >= 0] res[n, c, t / s, inv[w]] ) * (mask > 0 ? 1 : slope)
  outer  : dA[k, v, w] = sum_{n, c, t'} x[n, c, t' // rep, v] y[n, k C + c, t', w]
  aggconv: xa[n, k Cin + c, t, w] = sum over the listed neighbours v = nbr[k, w, p], p < pcount[k], v >= 0, of x[n, c, t, v] A[k, v, w]
           out[n, m, t, w] = sum_k sum_c W(k, m, c) xa[n, k Cin + c, t, w]  + add[n, m, t a_tstride, w]
  aggconv_label: `add` is the label bias  sum_k (sum_v A[k, v, w]) (sum_j Wc(k, m, j) E[label_n, j]);  a label outside
           [0, L) turns its sample into NaN.

Error bracket (derived, not measured).  u = 2^-24, S = the same sum over the magnitudes of its terms (the residual / `add`
term included, times the magnitude of the slope factor), n = the number of products of an element.  Per element

    |r - ref| <= (n + b) u S + u |ref|.

Every product enters a tree of additions whose leaves are the element's n products, in some fixed order (an FMA chain, MFMA
steps, partial sums of waves / k-groups / slabs); it is rounded at most once when it is formed and once per addition on its
way to the root, and a tree with n leaves has at most n - 1 additions on a path; additions of an exact zero (padding, rows
past the end, the zero an accumulator starts from) round nothing.  So the sum is sum_i p_i (1 + t_i), |t_i| <= n u / (1 - n u),
in ANY order.  b pays, a second time and separately, for the additions OUTSIDE the main chain as counted in the sources,
plus 1 for the second-order part of the bound (n u < 2^-9 for every float case) and 1 spare; u |ref| is the final rounding.

  expand, every form (csrc/kg_agg.hip): one chain, nothing outside it                                   b = 0 + 2 = 2
  reduce, every form: `+ res` (1) and the slope multiply (1) of agg_epi_apply / the mfma epilogue          b = 2 + 2 = 4
  outer, matrix-core form: the LDS sum over P <= 16 frame blocks x 4 waves in outer_mfma_body (64), the slab sum
      kg_slab_sum_256 - chains of ceil(512 / 4) slabs (128) and a 4-way tree (2); the element-wise form has the slab sum
      only.  Both take the larger count                                                                  b = 194 + 2 = 196
  aggconv, tile form (csrc/kg_aggconv.hip): n = the most neighbour products of an aggregated value (<= 4) + K Cin; the
      pair sum of the two k-groups of the KS = 2 form (1), `+ add` (1)                                   b = 2 + 2 = 4
  aggconv, tiny form: `+ add` (1); with the label bias n grows by J + V + K (the chains of P, S and their product;
      the (s0 + s1) + (s2 + s3) tree of P is inside J)                                                   b = 1 + 2 = 3 (4 is used)

Exact cases.  Integer operands in [-3, 3] (adjacency, weights, res, add, mask, embedding included) and slope = 0.25: the
definition computes S and asserts S < 2^24; every product, every partial sum of any subset of the terms and the product with
0.25 is then an fp32 number, every fp32 operation in every order is exact, and a kernel must equal the definition bit for bit.
"""
import itertools
from typing import NamedTuple, Optional, Tuple

import torch

U = 2.0 ** -24
B_EXPAND, B_REDUCE, B_OUTER, B_AGGCONV = 2, 4, 196, 4
SLOPE_EXACT, SLOPE_FLOAT = 0.25, 0.2
N_FLOAT_MAX = 2048           # float cases have at most this many products per element (the mutation check needs it)
PMAX = 4                     # width of the neighbour table
DATA_SEED = 11               # operands of the float cases in the mutation check
# seed of the mutated positions where the default (DATA_SEED) draws a product too small to leave the bracket
MUTATION_SEED = {"outer mfma P16": 12, "outer elementwise nchw": 12, "tile 642 XE3 XA1 ADD0": 12}


def draw(gen, integer, *shape):
    if integer:
        return torch.randint(-3, 4, shape, generator=gen).float()
    return torch.randn(*shape, generator=gen)


def bracket(ref, S, n, b):
    return (n + b) * U * S + U * ref.abs()


def worst_ratio(out, ref, S, n, b):
    """max over the elements of |out - ref| / bracket (0 / 0 counts as 0; NaN in ref must be NaN in out and is skipped)"""
    out = out.detach().double().cpu().reshape(-1)
    ref, S = ref.reshape(-1), S.reshape(-1)
    nan = ref.isnan()
    if nan.any():
        assert bool(out[nan].isnan().all()), "NaN expected where the definition has NaN"
        out, ref, S = out[~nan], ref[~nan], S[~nan]
    if ref.numel() == 0:
        return 0.0
    err = (out - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bracket(ref, S, n, b).clamp_min(1e-300))
    assert not bool(r.isnan().any()), "NaN in the result"
    return float(r.max())


def assert_exact(S):
    assert float(S.max()) < 2 ** 24, "integer case too long: S = %g" % float(S.max())


# ---- expand / reduce / outer ---------------------------------------------------------------------------------------------------
def _next_frame(t4, n, c, f):
    """frame f + 1 of channel c in the (n, t) order of a (N, C, T, V) tensor, zeros past the end (a mutation's source)"""
    N, _, T, V = t4.shape
    g = n * T + f + 1
    return t4[g // T, c, g % T] if g < N * T else torch.zeros(V, dtype=t4.dtype)


def expand_f64(x, A, rep, mutate=None, absolute=False):
    """(N, K C, T rep, W) float64.  mutate = ("drop", n, k, c, t', w, v): that product left out; ("shift", n, c, t'): that
    output frame reads the next input frame - NOT the definition (mutation check)."""
    x, A = x.double(), A.double()
    if absolute:
        x, A = x.abs(), A.abs()
    N, C, T, V = x.shape
    K, _, W = A.shape
    xr = x.repeat_interleave(rep, dim=2)
    out = torch.einsum("nctv,kvw->nkctw", xr, A).contiguous()
    if mutate is not None and mutate[0] == "drop":
        _, n, k, c, t, w, v = mutate
        out[n, k, c, t, w] -= xr[n, c, t, v] * A[k, v, w]
    elif mutate is not None:
        _, n, c, t = mutate
        out[n, :, c, t, :] = torch.einsum("v,kvw->kw", _next_frame(x, n, c, t // rep), A)
    return out.reshape(N, K * C, T * rep, W)


def res_inv(W, drop):
    """(inv, r_V): the vertex of `res` that w reads - every other vertex kept, or the identity (inv None)"""
    if not drop:
        return None, W
    keep = list(range(0, W, 2))
    inv = torch.full((W,), -1, dtype=torch.int32)
    inv[keep] = torch.arange(len(keep), dtype=torch.int32)
    return inv, len(keep)


def reduce_f64(y, A, fold=1, res=None, s=1, inv=None, mask=None, slope=SLOPE_FLOAT, mutate=None, absolute=False):
    """(N, C, T, W) float64.  mutate = ("drop", n, c, t, w, k, v, q) | ("shift", n, c, t) | ("res", n, t): the hit test of
    that output frame evaluated one frame later."""
    y, A = y.double(), A.double()
    if absolute:
        y, A = y.abs(), A.abs()
    N, KC, Tin, V = y.shape
    K, _, W = A.shape
    C, T = KC // K, Tin // fold
    y5 = y.reshape(N, K, C, Tin, V)
    agg = torch.einsum("nkctv,kvw->nctw", y5, A).reshape(N, C, T, fold, W).sum(3)
    if mutate is not None and mutate[0] == "drop":
        _, n, c, t, w, k, v, q = mutate
        agg[n, c, t, w] -= y5[n, k, c, t * fold + q, v] * A[k, v, w]
    elif mutate is not None and mutate[0] == "shift":
        _, n, c, t = mutate
        agg[n, c, t] = 0.0
        for q in range(fold):
            for k in range(K):
                agg[n, c, t] += _next_frame(y, n, k * C + c, t * fold + q) @ A[k]
    out = agg
    if res is not None:
        res = res.double().abs() if absolute else res.double()
        add = torch.zeros_like(agg)
        for n in range(N):
            for t in range(T):
                tt = t + 1 if mutate is not None and mutate[0] == "res" and mutate[1:] == (n, t) else t
                if tt % s == 0 and tt // s < res.shape[2]:
                    for w in range(W):
                        iv = w if inv is None else int(inv[w])
                        if iv >= 0:
                            add[n, :, t, w] = res[n, :, tt // s, iv]
        out = out + add
    if mask is not None:
        f = torch.where(mask > 0, torch.ones_like(out), torch.full_like(out, slope))
        out = out * f
    return out


def outer_f64(x, y, K, rep, mutate=None, absolute=False):
    """(K, V, W) float64.  mutate = ("drop", k, v, w, n, c, t') | ("shift", n, c, t')"""
    x, y = x.double(), y.double()
    if absolute:
        x, y = x.abs(), y.abs()
    N, C, T, V = x.shape
    W = y.shape[3]
    xr = x.repeat_interleave(rep, dim=2)
    y5 = y.reshape(N, K, C, T * rep, W)
    out = torch.einsum("nctv,nkctw->kvw", xr, y5).contiguous()
    if mutate is not None and mutate[0] == "drop":
        _, k, v, w, n, c, t = mutate
        out[k, v, w] -= xr[n, c, t, v] * y5[n, k, c, t, w]
    elif mutate is not None:
        _, n, c, t = mutate
        d = _next_frame(x, n, c, t // rep) - xr[n, c, t]
        out += torch.einsum("v,kw->kvw", d, y5[n, :, c, t, :])
    return out


# ---- aggconv ---------------------------------------------------------------------------------------------------------------------
class WV(NamedTuple):        # the fields of _native.WView this file reads
    sT: int
    sO: int
    sI: int


def nbr_table(pattern):
    """(nbr (K, W, 4) int32, pcount [3]) of a boolean (K, V, W) pattern"""
    K, V, W = pattern.shape
    tab = torch.full((K, W, PMAX), -1, dtype=torch.int32)
    pcount = [0, 0, 0]
    for k in range(K):
        for w in range(W):
            vs = torch.nonzero(pattern[k, :, w]).flatten().tolist()
            assert len(vs) <= PMAX
            pcount[k] = max(pcount[k], len(vs))
            tab[k, w, :len(vs)] = torch.tensor(vs, dtype=torch.int32)
    return tab, pcount


def aggconv_f64(x, A, nbr, pcount, wflat, wv, M, add=None, add_tstride=1, mutate=None, absolute=False):
    """(out (N, M, T, W), xa (N, K Cin, T, W)) float64, through the neighbour table as the kernels go.
    mutate = ("drop", n, m, t, w, k, c, p): the product W(k, m, c) A[k, v_p, w] x[n, c, t, v_p] left out of `out`;
    ("shift", n, t, w): that column of `out` reads frame t + 1 (zeros past the sample's end)."""
    x, A, wflat = x.double(), A.double(), wflat.double()
    if absolute:
        x, A, wflat = x.abs(), A.abs(), wflat.abs()
    N, Cin, T, V = x.shape
    K, _, W = A.shape
    listed = torch.zeros(K, V, W, dtype=torch.bool)
    xa = torch.zeros(N, K, Cin, T, W, dtype=torch.float64)
    for k in range(K):
        for w in range(W):
            for p in range(pcount[k]):
                v = int(nbr[k, w, p])
                if v >= 0:
                    listed[k, v, w] = True
                    xa[:, k, :, :, w] += x[:, :, :, v] * A[k, v, w]
    assert not bool(((A != 0) & ~listed).any()), "the neighbour table misses non-zeros of the adjacency"
    d = torch.arange(K).view(-1, 1, 1)
    m = torch.arange(M).view(1, -1, 1)
    c = torch.arange(Cin).view(1, 1, -1)
    Wk = wflat[d * wv.sT + m * wv.sO + c * wv.sI]            # (K, M, Cin)
    out = torch.einsum("kmc,nkctw->nmtw", Wk, xa).contiguous()
    if mutate is not None and mutate[0] == "drop":
        _, n, mm, t, w, k, cc, p = mutate
        v = int(nbr[k, w, p])
        assert v >= 0 and p < pcount[k]
        out[n, mm, t, w] -= Wk[k, mm, cc] * A[k, v, w] * x[n, cc, t, v]
    elif mutate is not None:
        _, n, t, w = mutate
        col = torch.zeros(K, Cin, dtype=torch.float64)
        if t + 1 < T:
            for k in range(K):
                for p in range(pcount[k]):
                    v = int(nbr[k, w, p])
                    if v >= 0:
                        col[k] += x[n, :, t + 1, v] * A[k, v, w]
        out[n, :, t, w] = torch.einsum("kmc,kc->m", Wk, col)
    if add is not None:
        add = add.double().abs() if absolute else add.double()
        out = out + (add[:, :, :1] if add_tstride == 0 else add[:, :, ::add_tstride][:, :, :T])
    return out, xa.reshape(N, K * Cin, T, W)


def label_bias_f64(A, wg, cin, J, M, emb, labels, absolute=False):
    """(N, M, 1, W) float64: sum_k (sum_v A[k, v, w]) (sum_j Wc(k, m, j) E[label, j]); NaN for a label outside [0, L).
    wg: the whole gcn weight (K M, cin): its first J columns multiply the label channels."""
    A, wg, emb = A.double(), wg.double().reshape(-1, cin), emb.double()
    if absolute:
        A, wg, emb = A.abs(), wg.abs(), emb.abs()
    K, _, W = A.shape
    Wc = wg[:, :J].reshape(K, M, J)
    Ssum = A.sum(1)                                           # (K, W)
    out = torch.full((labels.numel(), M, 1, W), float("nan"), dtype=torch.float64)
    for n, lab in enumerate(labels.tolist()):
        if 0 <= lab < emb.shape[0]:
            P = Wc @ emb[lab]                                 # (K, M)
            out[n, :, 0, :] = torch.einsum("kw,km->mw", Ssum, P)
    return out


# ---- cases of expand / reduce / outer ----------------------------------------------------------------------------------------
FRAME, STREAM, MFMA, OUTER_ELEM, OUTER_MFMA = 0, 1, 2, 3, 4       # KG_AGG_FORM_* of include/kgan_hip.h
FORM_NAMES = {FRAME: "frame", STREAM: "stream", MFMA: "mfma", OUTER_ELEM: "outer-elementwise", OUTER_MFMA: "outer-mfma"}
ENV_FRAME = {"KG_AGG_MFMA": "0", "KG_AGG_STREAM": "0"}
ENV_STREAM = {"KG_AGG_MFMA": "0", "KG_AGG_STREAM": "1"}
ENV_MFMA = {"KG_AGG_MFMA": "1"}


class Agg(NamedTuple):
    name: str
    op: str                      # "expand" | "reduce" | "outer"
    N: int
    C: int
    T: int                       # frames of x (expand / outer) / of out (reduce)
    V: int
    W: int
    K: int
    rep: int = 1                 # expand / outer: rep, reduce: fold
    layout: str = "plane"        # channel-major planes or "nchw"
    a_tr: bool = False           # the adjacency handed over as the transposed view of a (K, W, V) tensor
    res: Optional[Tuple[int, bool]] = None      # reduce: (r_tstride, with r_inv)
    mask: bool = False
    env: dict = {}
    expect: dict = {}            # fields of the plan report that must hold
    exact_only: bool = False

    @property
    def n(self):
        return {"expand": self.V, "reduce": self.K * self.V * self.rep, "outer": self.C * self.N * self.T * self.rep}[self.op]

    @property
    def b(self):
        return {"expand": B_EXPAND, "reduce": B_REDUCE, "outer": B_OUTER}[self.op]

    @property
    def is_float(self):
        return not self.exact_only

    def operands(self, seed, integer):
        """dict of CPU tensors in NCHW"""
        g = torch.Generator().manual_seed(seed)
        N, C, T, V, W, K, rep = self.N, self.C, self.T, self.V, self.W, self.K, self.rep
        o = {}
        if self.op != "outer":
            o["A"] = draw(g, integer, K, V, W)
        if self.op == "expand":
            o["x"] = draw(g, integer, N, C, T, V)
        elif self.op == "reduce":
            o["y"] = draw(g, integer, N, K * C, T * rep, V)
            if self.res is not None:
                s, drop = self.res
                o["inv"], rv = res_inv(W, drop)
                o["res"] = draw(g, integer, N, C, -(-T // s), rv)
            if self.mask:
                o["mask"] = draw(g, integer, N, C, T, W)
        else:
            o["x"] = draw(g, integer, N, C, T, V)
            o["y"] = draw(g, integer, N, K * C, T * rep, W)
        return o

    def reference(self, o, integer, mutate=None):
        """(ref, S) float64"""
        slope = SLOPE_EXACT if integer else SLOPE_FLOAT
        if self.op == "expand":
            ref, S = expand_f64(o["x"], o["A"], self.rep, mutate), expand_f64(o["x"], o["A"], self.rep, absolute=True)
        elif self.op == "reduce":
            kw = dict(fold=self.rep, res=o.get("res"), s=self.res[0] if self.res else 1, inv=o.get("inv"), mask=o.get("mask"), slope=slope)
            ref, S = reduce_f64(o["y"], o["A"], mutate=mutate, **kw), reduce_f64(o["y"], o["A"], absolute=True, **kw)
        else:
            ref, S = outer_f64(o["x"], o["y"], self.K, self.rep, mutate), outer_f64(o["x"], o["y"], self.K, self.rep, absolute=True)
        if integer:
            assert_exact(S)
        return ref, S

    def mutations(self, o, seed):
        """the mutations of the mutation check, seeded positions"""
        g = torch.Generator().manual_seed(2000 + seed)
        r = lambda n: int(torch.randint(0, n, (1,), generator=g))
        N, C, T, V, W, K, rep = self.N, self.C, self.T, self.V, self.W, self.K, self.rep
        if self.op == "expand":
            out = [("drop", r(N), r(K), r(C), r(T * rep), r(W), r(V)), ("shift", r(N), r(C), r(T * rep))]
        elif self.op == "reduce":
            out = [("drop", r(N), r(C), r(T), r(W), r(K), r(V), r(rep)), ("shift", r(N), r(C), r(T))]
            if self.res is not None:
                out.append(("res", r(N), r(-(-T // self.res[0])) * self.res[0]))
        else:
            out = [("drop", r(K), r(V), r(W), r(N), r(C), r(T * rep)), ("shift", r(N), r(C), r(T * rep))]
        return out


def stream_fo(W, mult, per_frame, lds_floats):
    """frames per workgroup of the stream kernels at these sizes: the cases below are cut to FO + a few frames; the plan
    test asserts that the report's FO is this number (a retuning fails there)"""
    fo = min(8 * (256 // W), lds_floats // per_frame) // mult * mult
    return max(fo, mult)


def _frame_cases():
    # N, T, rep: N T rep = 1, 255, 257, and fold / rep 2 at 42 frames
    geo = [(1, 1, 1), (5, 17, 3), (257, 1, 1), (3, 7, 2), (1, 257, 1)]
    out = []
    for i, (op, K, (W, wp)) in enumerate(itertools.product(("expand", "reduce"), (1, 3), ((3, 4), (7, 8), (11, 16), (25, 28)))):
        N, T, rep = geo[i % len(geo)]
        V = (5, 1, 11, 25, 7)[(i // 2) % 5]
        epi = op == "reduce" and rep == 1 and i % 2 == 0
        out.append(Agg("frame %s K%d WP%d" % (op, K, wp), op, N, 2 + i % 2, T, V, W, K, rep, ("nchw", "plane")[i % 2], a_tr=i % 3 == 0,
                       res=(1 + i % 3, i % 4 == 0) if epi else None, mask=epi, env=ENV_FRAME, expect=dict(form=FRAME, K=K, WP=wp)))
    return out


def _stream_cases():
    out = []
    for i, (op, K, (V, vm)) in enumerate(itertools.product(("expand", "reduce"), (1, 3), ((3, 4), (5, 8), (11, 16), (25, 25)))):
        W = (5, 11, 25, 9)[i % 4]
        rep = 1 + i % 3 if op == "expand" else (1, 2)[i % 2]
        if op == "expand":
            fo = stream_fo(W, 4 * rep, V, 8192 * rep - 2 * V * rep)
            T = fo // rep + 1                        # FO + rep output frames: two workgroups, the last one ragged
        else:
            fo = stream_fo(W, 4, K * rep * V, 12288)
            T = fo + 3
        epi = op == "reduce" and rep == 1
        # the frames of one channel times V: no multiple of 4 where the sizes allow it
        out.append(Agg("stream %s K%d VM%d" % (op, K, vm), op, 1, 2, T, V, W, K, rep, a_tr=i % 2 == 1,
                       res=(1 + i % 3, i % 4 == 1) if epi else None, mask=epi, env=ENV_STREAM,
                       expect=dict(form=STREAM, K=K, VM=vm, FO=fo, grid_x=2, grid_y=2)))
    return out


def _mfma_cases():
    out = []
    ks_red = {1: 8, 5: 8, 6: 17, 11: 17, 12: 38, 13: 38, 25: 38}
    ks_exp = {1: 3, 5: 3, 6: 3, 11: 6, 12: 6, 13: 13, 25: 13}
    Ws = (1, 5, 11, 25)
    for i, V in enumerate(ks_red):
        W = Ws[i % 4]
        out.append(Agg("mfma expand V%d W%d KS%d" % (V, W, ks_exp[V]), "expand", 2, 3, 75, V, W, 3, a_tr=i % 2 == 0, env=ENV_MFMA,
                       expect=dict(form=MFMA, KI=1, KO=3, KS=ks_exp[V], RES=0, MSK=0, SUB=1, tiles_per_c=2, ntiles=6, grid_x=6)))
        for j, (r, m) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            Wr = Ws[(i + j) % 4]
            out.append(Agg("mfma reduce V%d W%d KS%d RES%d MSK%d" % (V, Wr, ks_red[V], r, m), "reduce", 3, 2, 50, V, Wr, 3,
                           a_tr=(i + j) % 2 == 1, res=(1 + (i + j) % 3, j == 1) if r else None, mask=bool(m), env=ENV_MFMA,
                           expect=dict(form=MFMA, KI=3, KO=1, KS=ks_red[V], RES=r, MSK=m, SUB=1, tiles_per_c=2, ntiles=4, grid_x=4)))
    sub = lambda s: dict(ENV_MFMA, KG_AGG_MFMA_SUB=str(s))
    full = (2, True)
    out += [
        # forced sub-tiles: SUB V <= 32 and SUB * 512 (KI V + KO W) <= 61440 bytes
        Agg("mfma reduce SUB8 V1", "reduce", 1, 2, 1100, 1, 5, 3, res=full, mask=True, env=sub(8),
            expect=dict(form=MFMA, KS=8, SUB=8, tiles_per_c=2, ntiles=4, lds_bytes=8 * 512 * 8)),
        Agg("mfma reduce SUB6 V5", "reduce", 2, 2, 400, 5, 5, 3, res=(3, False), mask=True, env=sub(6),
            expect=dict(form=MFMA, KS=8, SUB=6, tiles_per_c=2, ntiles=4, lds_bytes=61440)),
        Agg("mfma expand SUB6 V5", "expand", 2, 2, 400, 5, 5, 3, env=sub(6), expect=dict(form=MFMA, KS=3, SUB=6, tiles_per_c=2, lds_bytes=61440)),
        Agg("mfma reduce SUB4 V6", "reduce", 1, 3, 600, 6, 11, 3, mask=True, env=sub(4), expect=dict(form=MFMA, KS=17, SUB=4, tiles_per_c=2)),
        Agg("mfma expand SUB4 V5", "expand", 3, 2, 200, 5, 1, 3, env=sub(4), expect=dict(form=MFMA, KS=3, SUB=4, tiles_per_c=2)),
        # two tiles per channel, the last one ragged: 485 frames in tiles of 3 x 128
        Agg("mfma reduce SUB3 V5 485 frames", "reduce", 5, 2, 97, 5, 11, 3, res=(1, True), mask=True, env=sub(3),
            expect=dict(form=MFMA, KS=8, SUB=3, tiles_per_c=2, ntiles=4)),
        Agg("mfma expand SUB3 V5 485 frames", "expand", 5, 2, 97, 5, 11, 3, env=sub(3), expect=dict(form=MFMA, KS=3, SUB=3, tiles_per_c=2)),
        Agg("mfma reduce SUB2 V13", "reduce", 2, 2, 150, 13, 5, 3, res=(2, False), env=sub(2), expect=dict(form=MFMA, KS=38, SUB=2, tiles_per_c=2)),
        Agg("mfma expand SUB2 V12", "expand", 2, 2, 150, 12, 5, 3, env=sub(2), expect=dict(form=MFMA, KS=6, SUB=2, tiles_per_c=2)),
        Agg("mfma reduce SUB1 V25", "reduce", 2, 2, 100, 25, 25, 3, res=(3, True), mask=True, env=sub(1), expect=dict(form=MFMA, KS=38, SUB=1, tiles_per_c=2)),
        # a value the host must reject (8 x 5 > 32): its own choice, one sub-tile at this size
        Agg("mfma reduce SUB8 rejected V5", "reduce", 2, 2, 100, 5, 5, 3, mask=True, env=sub(8), expect=dict(form=MFMA, KS=8, SUB=1, tiles_per_c=2)),
        # the persistent loop: 7 tiles on 3 workgroups, a ragged last round
        Agg("mfma reduce GRID3 7 tiles", "reduce", 1, 7, 100, 11, 11, 3, res=(2, True), mask=True, env=dict(ENV_MFMA, KG_AGG_MFMA_GRID="3"),
            expect=dict(form=MFMA, KS=17, ntiles=7, grid_x=3)),
        Agg("mfma expand GRID3 7 tiles", "expand", 1, 7, 100, 11, 11, 3, env=dict(ENV_MFMA, KG_AGG_MFMA_GRID="3"),
            expect=dict(form=MFMA, KS=6, ntiles=7, grid_x=3)),
        # the mask's 128-bit path needs m_sC = N T W to be a multiple of 4: one case with, one without (the GPU test asserts it)
        Agg("mfma reduce mask rows aligned", "reduce", 2, 3, 66, 5, 6, 3, mask=True, env=ENV_MFMA, expect=dict(form=MFMA, MSK=1, RES=0)),
        Agg("mfma reduce mask rows unaligned", "reduce", 3, 3, 47, 5, 5, 3, mask=True, env=ENV_MFMA, expect=dict(form=MFMA, MSK=1, RES=0)),
        Agg("mfma reduce N1", "reduce", 1, 3, 131, 11, 5, 3, res=(2, True), mask=True, env=ENV_MFMA, expect=dict(form=MFMA, KS=17, RES=1, MSK=1)),
        Agg("mfma expand N1", "expand", 1, 3, 131, 11, 5, 3, env=ENV_MFMA, expect=dict(form=MFMA, KS=6)),
        # not eligible under KG_AGG_MFMA=1: the report says frame
        Agg("mfma ineligible: fold 2", "reduce", 2, 2, 40, 5, 5, 3, rep=2, env=dict(ENV_MFMA, KG_AGG_STREAM="0"), expect=dict(form=FRAME, WP=8)),
        Agg("mfma ineligible: nchw", "expand", 2, 2, 40, 5, 5, 3, layout="nchw", env=dict(ENV_MFMA, KG_AGG_STREAM="0"), expect=dict(form=FRAME, WP=8)),
        Agg("mfma ineligible: K 1", "reduce", 2, 2, 40, 5, 5, 1, env=dict(ENV_MFMA, KG_AGG_STREAM="0"), expect=dict(form=FRAME, WP=8)),
    ]
    return out


def _outer_cases():
    om = lambda K, tv, tw, **kw: dict(form=OUTER_MFMA, K=K, TV=tv, TW=tw, **kw)
    el = {"KG_AGG_OUTER_MFMA": "0"}
    out = []
    # all eight bodies; V, W <= 16 / > 16 choose TV, TW
    for i, (K, (V, tv), (W, tw)) in enumerate(itertools.product((1, 3), ((11, 1), (25, 2)), ((5, 1), (17, 2)))):
        out.append(Agg("outer mfma K%d TV%d TW%d" % (K, tv, tw), "outer", 2 + i % 2, 3, 23 + i, V, W, K, expect=om(K, tv, tw, P=1)))
    out += [
        Agg("outer mfma P16", "outer", 3, 2, 90, 1, 1, 3, expect=om(3, 1, 1, P=16)),
        Agg("outer mfma P8", "outer", 2, 3, 77, 2, 1, 1, expect=om(1, 1, 1, P=8)),
        Agg("outer mfma P3", "outer", 2, 3, 50, 5, 4, 3, expect=om(3, 1, 1, P=3)),
        Agg("outer mfma P1 N1", "outer", 1, 4, 100, 11, 16, 1, expect=om(1, 1, 1, P=1)),
        # 150 frames in units of 64: three chunks, the last one 22 frames
        Agg("outer mfma short last chunk", "outer", 2, 4, 75, 25, 25, 3, expect=om(3, 2, 2, P=1, F=64, chunks=3, units=12, slabs=12)),
        # more units than workgroups: every workgroup walks its strided list (exact only: 180000 products per element)
        Agg("outer mfma 600 units on 512 workgroups", "outer", 3, 600, 100, 1, 1, 1, exact_only=True,
            expect=om(1, 1, 1, P=16, chunks=1, units=600, slabs=512)),
        Agg("outer elementwise rep 2", "outer", 2, 3, 21, 5, 11, 3, rep=2, expect=dict(form=OUTER_ELEM, K=3)),
        Agg("outer elementwise nchw", "outer", 3, 2, 45, 11, 5, 1, layout="nchw", expect=dict(form=OUTER_ELEM, K=1)),
        Agg("outer elementwise forced", "outer", 2, 3, 40, 25, 25, 3, env=el, expect=dict(form=OUTER_ELEM, K=3)),
        Agg("outer elementwise forced K1 one frame", "outer", 1, 2, 1, 3, 25, 1, env=el, expect=dict(form=OUTER_ELEM, K=1, slabs=2)),
        Agg("outer elementwise 600 units on 512 workgroups", "outer", 1, 600, 33, 2, 3, 1, env=el, exact_only=True,
            expect=dict(form=OUTER_ELEM, K=1, units=1200, slabs=512)),
    ]
    return out


AGG_CASES = _frame_cases() + _stream_cases() + _mfma_cases() + _outer_cases()
AGG = {c.name: c for c in AGG_CASES}
assert len(AGG) == len(AGG_CASES)

# every instantiation the cases above must reach, taken together (test_agg_def_cpu.py asserts it from the plan reports)
AGG_INSTANTIATIONS = (
    {("frame", op, K, wp) for op in ("expand", "reduce") for K in (1, 3) for wp in (4, 8, 16, 28)}
    | {("stream", op, K, vm) for op in ("expand", "reduce") for K in (1, 3) for vm in (4, 8, 16, 25)}
    | {("mfma", 1, 3, ks, 0, 0) for ks in (3, 6, 13)}
    | {("mfma", 3, 1, ks, r, m) for ks in (8, 17, 38) for r in (0, 1) for m in (0, 1)}
    | {("outer-mfma", K, tv, tw) for K in (1, 3) for tv in (1, 2) for tw in (1, 2)}
    | {("outer-elementwise", K) for K in (1, 3)})


def instantiation(op, p):
    """the key of AGG_INSTANTIATIONS a plan report (dict) names"""
    f = p["form"]
    if f == FRAME:
        return ("frame", op, p["K"], p["WP"])
    if f == STREAM:
        return ("stream", op, p["K"], p["VM"])
    if f == MFMA:
        return ("mfma", p["KI"], p["KO"], p["KS"], p["RES"], p["MSK"])
    if f == OUTER_MFMA:
        return ("outer-mfma", p["K"], p["TV"], p["TW"])
    return ("outer-elementwise", p["K"])


# ---- kg_agg_outer_many -----------------------------------------------------------------------------------------------------------
def _many_job(i, shared):
    """job i of a call: small, its own shape; `shared`: the matrix-core form (else rep = 2: launched on its own)"""
    V, W = ((5, 11), (11, 5), (25, 25), (1, 3), (16, 17), (7, 7))[i % 6]
    return Agg("job %d" % i, "outer", 2, 2 + i % 3, 9 + i, V, W, (3, 1)[i % 2], rep=1 if shared else 2)


class Many(NamedTuple):
    jobs: list
    env: dict
    launch: list                 # per job: index of the shared launch, -1 = on its own
    slabs: Optional[list] = None


def _launch_indices(shared):
    """the walk of kg_agg_outer_many written down from its description in the header: a shared launch closes after 8
    jobs and wherever 16 jobs' slab sums are flushed"""
    out, idx, n = [], 0, 0
    for i, s in enumerate(shared):
        if s:
            out.append(idx)
            n += 1
            if n == 8:
                idx, n = idx + 1, 0
        else:
            out.append(-1)
        if (i + 1) % 16 == 0 and n:
            idx, n = idx + 1, 0
    return out


def _many(shared, env=None, slabs=None, big=None):
    jobs = [_many_job(i, s) for i, s in enumerate(shared)]
    if big is not None:
        jobs[big] = jobs[big]._replace(C=40, T=64, rep=1, V=25, W=25, K=3)       # 128 frames in units of 64: 80 units
    return Many(jobs, env or {}, _launch_indices(shared), slabs)


MANY = {
    "1 job": _many([1]),
    "8 jobs": _many([1] * 8),
    "9 jobs": _many([1] * 9),
    "17 jobs": _many([1] * 17),
    # one-by-one jobs at 2, 7, 8 and 15, 16: the shared launches close at the 8th shared job and at the 16-job flush
    "17 jobs interleaved": _many([1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0]),
    "19 jobs, one-by-one first": _many([0] + [1] * 18),
    # a budget of 6 workgroups: the 80-unit job gets fewer slabs than units, the small ones round to one slab
    "budget 6": _many([1, 1, 1, 0, 1], env={"KG_AGG_OUTER_BUDGET": "6"}, big=2),
}
assert MANY["17 jobs"].launch == [0] * 8 + [1] * 8 + [2]
assert MANY["17 jobs interleaved"].launch == [0, 0, -1, 0, 0, 0, 0, -1, -1, 0, 0, 1, 1, 1, 1, -1, -1]


# ---- cases of kg_aggconv ---------------------------------------------------------------------------------------------------------
def graph_pattern(ds, lvl, kept):
    """the boolean (3, V, W) pattern of a real level (kinetic_gan_amd.graph.build_graph), all columns or the kept ones"""
    import numpy as np
    from kinetic_gan_amd.graph import build_graph
    g = build_graph(ds)
    A = torch.tensor(np.asarray(g.As[lvl]), dtype=torch.float32)
    if kept:
        A = A[:, :, torch.as_tensor(np.asarray(g.map[lvl + 1][:, 1]))]
    return A != 0


def synthetic_pattern(K, V, W, pc, seed):
    """a pattern with at most pc[k] non-zeros per column of partition k; column 0 of every partition has no neighbour
    (where there is another column)"""
    g = torch.Generator().manual_seed(seed)
    pat = torch.zeros(K, V, W, dtype=torch.bool)
    for k in range(K):
        for w in range(1 if W > 1 else 0, W):
            cnt = min(pc[k], V)
            if cnt:
                pat[k, torch.randperm(V, generator=g)[:cnt], w] = True
    return pat


class Conv(NamedTuple):
    name: str
    pattern: tuple               # ("ntu" | "h36m", level, kept) or ("syn", K, V, W, pcount, seed)
    N: int
    Cin: int
    M: int
    T: int
    add: Optional[int] = None    # None, or add_tstride 0 / 1
    xa: bool = False
    cc: int = 0                  # channels in front of the weight view inside its parent
    layout: str = "plane"
    label: Optional[Tuple[int, int, Tuple[int, ...]]] = None     # (L, J, labels): kg_aggconv_label
    env: dict = {}
    expect: dict = {}

    def pat(self):
        return graph_pattern(*self.pattern) if self.pattern[0] != "syn" else synthetic_pattern(*self.pattern[1:])

    def dims(self):
        K, V, W = self.pat().shape
        return K, V, W

    @property
    def b(self):
        return B_AGGCONV

    def n(self, pcount):
        K = self.dims()[0]
        n = max(pcount) + K * self.Cin
        if self.label is not None:
            n += self.label[1] + self.dims()[1] + K
        return n

    def operands(self, seed, integer):
        g = torch.Generator().manual_seed(seed)
        pat = self.pat()
        K, V, W = pat.shape
        nbr, pcount = nbr_table(pat)
        o = dict(nbr=nbr, pcount=pcount)
        o["A"] = draw(g, integer, K, V, W) * pat
        o["x"] = draw(g, integer, self.N, self.Cin, self.T, V)
        J = self.label[1] if self.label else 0
        ctot = self.Cin + self.cc + J
        wfull = draw(g, integer, K * self.M, ctot)
        if not integer:
            wfull = wfull / (K * self.Cin) ** 0.5
        o["wfull"] = wfull
        o["wview"] = wfull.reshape(-1)[self.cc + J:]
        o["wv"] = WV(self.M * ctot, ctot, 1)
        if self.add is not None:
            o["add"] = draw(g, integer, self.N, self.M, 1 if self.add == 0 else self.T, W)
        if self.label:
            L, J, labels = self.label
            assert len(labels) == self.N and self.cc == 0
            o["emb"] = draw(g, integer, L, J)
            o["labels"] = torch.tensor(labels, dtype=torch.int64)
        return o

    def reference(self, o, integer, mutate=None):
        """(out, xa, S of out, S of xa)"""
        kw = dict(add=o.get("add"), add_tstride=self.add if self.add is not None else 1)
        ref, xa = aggconv_f64(o["x"], o["A"], o["nbr"], o["pcount"], o["wview"], o["wv"], self.M, mutate=mutate, **kw)
        S, Sxa = aggconv_f64(o["x"], o["A"], o["nbr"], o["pcount"], o["wview"], o["wv"], self.M, absolute=True, **kw)
        if self.label:
            L, J, _ = self.label
            ref = ref + label_bias_f64(o["A"], o["wfull"], self.Cin + J, J, self.M, o["emb"], o["labels"])
            S = S + label_bias_f64(o["A"], o["wfull"], self.Cin + J, J, self.M, o["emb"], o["labels"], absolute=True).nan_to_num(0.0)
        if integer:
            assert_exact(S)
        return ref, xa, S, Sxa

    def mutations(self, o, seed):
        g = torch.Generator().manual_seed(3000 + seed)
        r = lambda n: int(torch.randint(0, n, (1,), generator=g))
        K, V, W = self.dims()
        ok_n = [n for n in range(self.N) if not self.label or 0 <= self.label[2][n] < self.label[0]]
        n = ok_n[r(len(ok_n))]
        ent = [(k, w, p) for k in range(K) for w in range(W) for p in range(o["pcount"][k]) if int(o["nbr"][k, w, p]) >= 0]
        k, w, p = ent[r(len(ent))]
        return [("drop", n, r(self.M), r(self.T), w, k, r(self.Cin), p), ("shift", n, r(self.T - 1) if self.T > 1 else 0, w)]


NTU_NARROW, NTU_WIDE = ("ntu", 0, False), ("ntu", 0, True)          # V = 25: W = 25 (span 175), W = 11 kept (span 325)


def _tile_cases():
    out = []
    # span = (127 // W + 2) V floats per staged row: narrow <= 192 < wide <= 384
    narrow = [NTU_NARROW, ("ntu", 1, False), ("h36m", 0, False), ("syn", 3, 7, 25, (1, 4, 1), 1), ("syn", 3, 1, 1, (1, 1, 0), 2),
              ("syn", 3, 5, 11, (1, 4, 0), 3), ("ntu", 2, False), ("h36m", 1, False)]
    wide = [NTU_WIDE, ("syn", 3, 20, 9, (1, 4, 1), 4), ("syn", 3, 16, 7, (0, 3, 1), 5), ("syn", 3, 2, 1, (1, 2, 0), 6)]
    Ms = {32: (32, 33, 64, 70, 96, 128), 64: (64, 70, 128, 33, 32, 96)}
    Cins = (3, 16, 20, 40)
    i = 0
    for plan, xe, xa, add in itertools.product((321, 322, 641, 642), (3, 6), (0, 1), (0, 1)):
        bm, ks = plan // 10, plan % 10
        pat = (narrow if xe == 3 else wide)[i % (8 if xe == 3 else 4)]
        # ADD = 0 needs whole row tiles and no `add`: M a multiple of BM; ADD = 1: an `add` operand (a_tstride 0 / 1), or
        # none and a ragged last row tile
        j = i // 2
        if not add:
            M, with_add = (bm, 2 * bm)[j % 2], None
        else:
            M = Ms[bm][j % 6]
            with_add = None if (M % bm and j % 4 == 3) else j % 2
        N, T = ((3, 7), (2, 5), (1, 13), (4, 3))[j % 4]              # e.g. 3 x 7 x 11 = 231 columns: ragged against 128
        out.append(Conv("tile %d XE%d XA%d ADD%d" % (plan, xe, xa, add), pat, N, Cins[(i + j // 4) % 4], M, T, add=with_add, xa=bool(xa),
                        cc=(0, 5)[j % 2], layout=("plane", "nchw")[(j // 2) % 2], env={"KG_AGGCONV_PLAN": str(plan)},
                        expect=dict(tiny=0, BM=bm, KS=ks, XE=xe, XA=xa, ADD=add)))
        i += 1
    out += [
        # a tiny-geometry launch (Cin 3, M 32) forced onto the tile kernel
        Conv("tile 321 tiny geometry", NTU_NARROW, 2, 3, 32, 5, add=0, xa=True, env={"KG_AGGCONV_PLAN": "321"},
             expect=dict(tiny=0, BM=32, KS=1, XE=3, XA=1, ADD=1)),
        # partitions without a non-zero: tapmask has a hole
        Conv("tile 642 tapmask hole", ("syn", 3, 5, 11, (1, 0, 1), 7), 3, 16, 128, 7, xa=True, env={"KG_AGGCONV_PLAN": "642"},
             expect=dict(tiny=0, BM=64, KS=2, tapmask=5, ADD=0)),
        # an invalid plan value: neither 64 rows nor two k-groups
        Conv("tile invalid plan 999", NTU_WIDE, 3, 20, 70, 7, add=1, env={"KG_AGGCONV_PLAN": "999"},
             expect=dict(tiny=0, BM=32, KS=1, XE=6, ADD=1)),
        # the unforced rule at test sizes
        Conv("tile default plan", ("ntu", 1, False), 2, 40, 33, 8, expect=dict(tiny=0, BM=32, KS=1, XE=3, XA=0, ADD=1)),
    ]
    return out


def _tiny_cases():
    out = []
    pats = [NTU_NARROW, ("h36m", 0, True), ("syn", 3, 9, 25, (1, 4, 1), 8), ("syn", 2, 25, 7, (1, 3, 0), 9), NTU_WIDE, ("syn", 1, 5, 32, (1, 0, 0), 10)]
    for i, (mt, rg, lb) in enumerate(itertools.product((32, 64), (1, 2, 4), (0, 1))):
        pat = pats[i % 6]
        M = {32: (32, 20, 1), 64: (64, 33, 50)}[mt][i % 3]
        N, T = ((3, 13), (2, 27), (4, 5))[i % 3]                     # T W: ragged against 256 / RG
        label = (6, (20, 7, 64)[i % 3], tuple((1, 5, -1, 6, 0)[q % 5] for q in range(N))) if lb else None
        out.append(Conv("tiny MT%d RG%d LB%d" % (mt, rg, lb), pat, N, (3, 2, 4, 1)[i % 4], M, T, add=None if lb else (None, 0, 1)[i % 3],
                        xa=i % 2 == 0, cc=0 if lb else (0, 5)[i % 2], layout=("plane", "nchw")[i % 2], label=label,
                        env={"KG_AGGCONV_TINY_RG": str(rg)}, expect=dict(tiny=1, MT=mt, RG=rg, LB=lb)))
    return out


CONV_CASES = _tile_cases() + _tiny_cases()
CONV = {c.name: c for c in CONV_CASES}
assert len(CONV) == len(CONV_CASES)
CONV_INSTANTIATIONS = ({("tile", bm, ks, xe, xa, add) for bm in (32, 64) for ks in (1, 2) for xe in (3, 6) for xa in (0, 1) for add in (0, 1)}
                       | {("tiny", mt, rg, lb) for mt in (32, 64) for rg in (1, 2, 4) for lb in (0, 1)})


def conv_instantiation(p):
    if p["tiny"]:
        return ("tiny", p["MT"], p["RG"], p["LB"])
    return ("tile", p["BM"], p["KS"], p["XE"], p["XA"], p["ADD"])
