// kg_nn_gram: the results of kg_nn / kg_nn_sets, bit for bit, with the Q x N x D work on the fp32 matrix cores (see
// include/kgan_hip.h).  The Gram value |b|^2 - 2 q.b cancels for near-copies, so it only FILTERS: every row keeps
// `cand` > k candidates by key, their distances come from the direct-difference chain of kg_nn, and a per-row certificate
// proves that no base point outside the candidates can enter or tie with the row's list.  Rows without the proof go through
// the exact search of kg_nn (kg_nn_search.h, its row-list form).  Six launches, no atomics, no host synchronisation.
//
// kg_nn_gram_search_kernel: the grid, the LDS lists and the rank merge of kg_nn_search_kernel; the tile of squared distances
// is replaced by a tile of keys.  A wave owns a 32 x 32 block of the tile's q.b: v_mfma_f32_32x32x2f32 on operands staged
// in LDS as dist_stage lays them out (s[k][p]: lane l reads dimension 2 q + (l >> 5) of point l & 31 of its block - consecutive
// banks), by dist_stage itself or, where every address allows, by 16-byte loads that fly under the MFMAs of the chunk before.
// The accumulator restarts every GR_BLOCK = 256 dimensions and the blocks are added in order: the shape of a pair's chain is
// fixed by D alone, so its key depends on the two points alone - not on the tile, the chunk or the plan - and the worst-case
// rounding error of q.b is (256 + D / 256 + c) u instead of (D + c) u.  With a 32-tile one wave computes, four stage.
// kg_nn_gram_rescore_kernel: a wave per row, a lane per candidate: 64 dimensions of the row and of its candidates go through
// LDS (coalesced 256-byte reads of each candidate), then lane c runs the fmaf chain of kg_nn over them in ascending order.
// The row's norm is summed on the way.  Rank by (d2, j) through shuffles, the first k are written, the certificate is
// evaluated in fp64 by lane 0 and the row's flag written.
// kg_nn_gram_compact_kernel: a workgroup per (set, class) scans the flags in row order (ballots, four wave totals in LDS) and
// writes the list of open rows, its length and stats.
// kg_nn_norms_kernel: a workgroup per (class, part p): a wave per point j = p mod 64.
#include "kg_nn_search.h"

namespace {

constexpr int GR_BLOCK = 256;           // dimensions after which the pre-filter's accumulator restarts
constexpr int RS_W = 4;                 // rows (waves) of a re-score workgroup
constexpr int NP = KG_NN_NORM_PARTS;
static_assert(GR_BLOCK % DT_KC == 0 && NP == 64, "blocks are whole staged chunks; a lane per part");

struct GramDev {
    NnDev n;                            // the caller's k; d2 / idx the outputs
    int cand;
    const float* ckey;  const int* cidx;    // (nsets, classes, Q, cand): the merged candidates, ascending (key, j)
    const float* parts;                 // (classes, NP)
    int* flag;                          // (nsets, classes, Q): 1 = the row is not certified
    int* list;  int* count;             // (nsets, classes, Q) / (nsets, classes): the open rows
    int* stats;
    double tau, en, ecoef, eabs;        // the certificate's constants (kg_nn_gram sets them)
};

// The 16-byte staging path of the pre-filter (VEC: the inner run, every stride and every pointer are multiples of 4 floats):
// a thread owns 4 consecutive dimensions (k = 4 (tid & 7) ..) of the points tid >> 3, + 32, ..: global -> registers (gram_fetch,
// in flight under the MFMAs of the chunk before) -> LDS (gram_put: the affine, s[k][p] as dist_stage leaves it).  Which path
// stages an element does not show in any bit: both put the same fp32 value, or zero outside the set / dimension, in place.
template <int TI>
struct GramRegs {
    float4 v[TI / 32];
};

template <int TI>
__device__ __forceinline__ void gram_fetch(GramRegs<TI>& r, const float* base, long sp, long so, const FastDiv& inner, int p0, int n,
                                           int k0, int D) {
    const int d = k0 + 4 * (threadIdx.x & 7), pl = threadIdx.x >> 3;
    unsigned o = 0, e = 0;
    if (d < D) inner.divmod((unsigned)d, o, e);
    const float* col = base + ((long)o * so + e);
#pragma unroll
    for (int m = 0; m < TI / 32; ++m) {
        const int pi = p0 + pl + 32 * m;
        r.v[m] = (d < D && pi < n) ? *reinterpret_cast<const float4*>(col + (long)pi * sp) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

template <int TI, class Load>
__device__ __forceinline__ void gram_put(float (*s)[TI + DT_PAD], const GramRegs<TI>& r, int p0, int n, int k0, int D, const Load& load) {
    const int kq = 4 * (threadIdx.x & 7), pl = threadIdx.x >> 3;
    const bool din = k0 + kq < D;
#pragma unroll
    for (int m = 0; m < TI / 32; ++m) {
        const int p = pl + 32 * m;
        const bool in = din && p0 + p < n;
        s[kq + 0][p] = in ? load(r.v[m].x) : 0.f;
        s[kq + 1][p] = in ? load(r.v[m].y) : 0.f;
        s[kq + 2][p] = in ? load(r.v[m].z) : 0.f;
        s[kq + 3][p] = in ? load(r.v[m].w) : 0.f;
    }
}

template <int TI, bool VEC>
__global__ __launch_bounds__(DT_NT) void kg_nn_gram_search_kernel(NnDev a) {
    constexpr int CW = NnLists<TI>::CW;
    __shared__ __attribute__((aligned(16))) float stage[2][DT_KC][TI + DT_PAD];
    __shared__ float cand[TI][CW];
    __shared__ int cidx[TI][KG_NN_MAX_K];
    static_assert(2 * TI * KG_NN_MAX_K <= 2 * DT_KC * (TI + DT_PAD), "best / bidx do not fit the staging buffers");
    float (*si)[TI + DT_PAD] = stage[0];
    float (*sj)[TI + DT_PAD] = stage[1];
    float (*best)[KG_NN_MAX_K] = reinterpret_cast<float (*)[KG_NN_MAX_K]>(&stage[0][0][0]);
    float (*bidx)[KG_NN_MAX_K] = best + TI;

    const NnPlace w = nn_place(a);
    const int i0 = (int)w.rt * TI, k = a.k, Q = a.q.n;      // (k: the number of candidates kept)
    const long cb = (long)w.ch * a.chunk;
    const int ce = (int)min(cb + a.chunk, (long)a.b.n);
    const float* qb = w.qp + (long)w.cls * a.q.sc;
    const float* bb = a.b.p + (long)w.cls * a.b.sc;
    const float* bn = a.bn + (long)w.cls * a.b.n;
    const int tid = threadIdx.x, wave = tid >> 6, l31 = tid & 31, kh = (tid >> 5) & 1;
    const int rb = (wave >> 1) * 32, cb32 = (wave & 1) * 32;    // the wave's block of the tile
    const bool active = rb < TI && cb32 < TI;

    nn_lists_clear<TI>(cand, cidx);

    for (long jl = cb; jl < ce; jl += TI) {
        const int j0 = (int)jl;
        kg_f32x16 tot, acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) { tot[r] = 0.f; acc[r] = 0.f; }
        GramRegs<TI> ra, rb_;
        if (VEC) {
            gram_fetch<TI>(ra, qb, a.q.sp, a.q.so, a.inner, i0, Q, 0, a.D);
            gram_fetch<TI>(rb_, bb, a.b.sp, a.b.so, a.inner, j0, ce, 0, a.D);
        }
        for (int k0 = 0; k0 < a.D; k0 += DT_KC) {
            const int kn = min(DT_KC, a.D - k0);            // (dimensions past D are staged as zeros: fma(0, 0, acc) = acc)
            if (VEC) {
                gram_put<TI>(si, ra, i0, Q, k0, a.D, a.qa);
                gram_put<TI>(sj, rb_, j0, ce, k0, a.D, a.ba);
            } else {
                dist_stage<TI>(si, qb, a.q.sp, a.q.so, a.inner, i0, Q, k0, kn, a.qa);
                dist_stage<TI>(sj, bb, a.b.sp, a.b.so, a.inner, j0, ce, k0, kn, a.ba);
            }
            __syncthreads();
            if (VEC && k0 + DT_KC < a.D) {                  // the next chunk's loads fly under this chunk's MFMAs
                gram_fetch<TI>(ra, qb, a.q.sp, a.q.so, a.inner, i0, Q, k0 + DT_KC, a.D);
                gram_fetch<TI>(rb_, bb, a.b.sp, a.b.so, a.inner, j0, ce, k0 + DT_KC, a.D);
            }
            if (active) {
#pragma unroll
                for (int q = 0; q < DT_KC / 2; ++q)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(si[2 * q + kh][rb + l31], sj[2 * q + kh][cb32 + l31], acc, 0, 0, 0);
            }
            if (((k0 + DT_KC) & (GR_BLOCK - 1)) == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { tot[r] += acc[r]; acc[r] = 0.f; }
            }
            __syncthreads();
        }
        if (active) {
            // C/D layout: column = l31, row of register r = (r & 3) + 8 (r >> 2) + 4 kh
            const int col = cb32 + l31, j = j0 + col;
            const float nb = j < ce ? bn[j] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb + (r & 3) + 8 * (r >> 2) + 4 * kh, i = i0 + row;
                const float g = tot[r] + acc[r];
                cand[row][k + col] = (i >= Q || j >= ce || (a.exclude_self && i == j)) ? INFINITY : fmaf(-2.f, g, nb);
            }
        }
        __syncthreads();
        nn_lists_merge<TI>(cand, cidx, best, bidx, k, j0);
    }
    __syncthreads();
    nn_lists_store<TI>(a, cand, cidx, w.sc, w.ch, i0, Q, NnRows{nullptr});
}

__global__ __launch_bounds__(RS_W * 64) void kg_nn_gram_rescore_kernel(GramDev g) {
    __shared__ float bt[RS_W][KG_NN_MAX_K][65];     // 64 dimensions of every candidate (row stride 65: a lane per row, no conflicts)
    __shared__ float qs[RS_W][64];
    const NnDev& a = g.n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Q = a.q.n, N = a.b.n, D = a.D, cand = g.cand, k = a.k;
    const long rows = (long)a.nsets * a.classes * Q;
    long row = (long)blockIdx.x * RS_W + wave;
    const bool in = row < rows;
    if (!in) row = rows - 1;                        // (a wave past the end walks the last row along - the barriers - and writes nothing)
    const int sc = (int)(row / Q), i = (int)(row % Q), set = sc / a.classes, cls = sc % a.classes;
    const float* qp = a.q.p;
#pragma unroll
    for (int s = 1; s < KG_NN_MAX_SETS; ++s)
        if (set == s) qp = a.qs[s - 1];
    const float* qrow = qp + (long)cls * a.q.sc + (long)i * a.q.sp;
    const float* bb = a.b.p + (long)cls * a.b.sc;

    int cj = INT_MAX;
    if (lane < cand) cj = g.cidx[row * cand + lane];
    const bool mine = cj >= 0 && cj < N;            // (an unfilled entry is INT_MAX; nothing outside the base is ever read)
    float acc = 0.f, nq = 0.f;
    for (int d0 = 0; d0 < D; d0 += 64) {
        const int d = d0 + lane;
        const bool din = d < D;
        unsigned o = 0, e = 0;
        if (din) a.inner.divmod((unsigned)d, o, e);
        const float qv = din ? a.qa(qrow[(long)o * a.q.so + e]) : 0.f;
        nq = fmaf(qv, qv, nq);
        qs[wave][lane] = qv;
        const long boff = (long)o * a.b.so + e;
        for (int c = 0; c < cand; ++c) {
            const int j = __shfl(cj, c, 64);
            bt[wave][c][lane] = (din && j >= 0 && j < N) ? a.ba(bb[(long)j * a.b.sp + boff]) : 0.f;
        }
        __syncthreads();
        if (mine) {
            const int n = min(64, D - d0);
            const float* bc = bt[wave][lane];
            for (int x = 0; x < n; ++x) {
                const float df = qs[wave][x] - bc[x];
                acc = fmaf(df, df, acc);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nq += __shfl_xor(nq, off, 64);
    float bmax = g.parts[(long)cls * NP + lane];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, off, 64));

    const float dc = mine ? acc : INFINITY;
    const int jc = mine ? cj : INT_MAX;
    int rank = 0;
#pragma unroll 4
    for (int b = 0; b < KG_NN_MAX_K; ++b) {
        const float db = __shfl(dc, b, 64);
        const int jb = __shfl(jc, b, 64);
        rank += (db < dc || (db == dc && jb < jc)) ? 1 : 0;
    }
    if (in && mine && rank < k) {
        a.d2[row * k + rank] = dc;
        a.idx[row * k + rank] = jc;
    }
    const unsigned long long kth = __ballot(mine && rank == k - 1);
    const float t = kth ? __shfl(dc, __ffsll((long long)kth) - 1, 64) : INFINITY;
    if (lane == 0 && in) {
        const int admissible = N - ((a.exclude_self && i < N) ? 1 : 0);
        bool cert = admissible <= cand;             // every admissible base point is a candidate
        if (!cert) {
            // a lower bound of the chain distance of every pair whose key is at least the cand-th smallest
            const double key = (double)g.ckey[row * cand + cand - 1];
            const double m = (double)fmaxf(nq, bmax);
            const double low = (1.0 - g.tau) * (key + (double)nq * (1.0 - g.en) - g.ecoef * m) - g.eabs;
            cert = low > (double)t;                 // (strict: no tie reaches across; false for NaN)
        }
        g.flag[row] = cert ? 0 : 1;
    }
}

__global__ __launch_bounds__(256) void kg_nn_gram_compact_kernel(GramDev g) {
    __shared__ int wsum[4];
    const int sc = blockIdx.x, Q = g.n.q.n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int* flag = g.flag + (long)sc * Q;
    int* list = g.list + (long)sc * Q;
    int base = 0;
    for (int r0 = 0; r0 < Q; r0 += 256) {
        const int i = r0 + tid;
        const bool f = i < Q && flag[i] != 0;
        const unsigned long long b = __ballot(f);
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int off = base;
        for (int v = 0; v < wave; ++v) off += wsum[v];
        if (f) list[off + __popcll(b & ((1ull << lane) - 1ull))] = i;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) {
        g.count[sc] = base;
        g.stats[sc * 2 + 0] = Q - base;
        g.stats[sc * 2 + 1] = base;
    }
}

constexpr int NORM_W = 16;              // waves of a norms workgroup: a point each

__global__ __launch_bounds__(NORM_W * 64) void kg_nn_norms_kernel(DistSet x, NnAffine f, FastDiv inner, int D, float* norms,
                                                                  float* parts) {
    __shared__ float wmax[NORM_W];
    const int cls = blockIdx.x / NP, p = blockIdx.x % NP, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* xb = x.p + (long)cls * x.sc;
    float most = 0.f;
    for (long j = p + (long)NP * wave; j < x.n; j += (long)NP * NORM_W) {
        const float* pt = xb + j * x.sp;
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) {
            unsigned o, e;
            inner.divmod((unsigned)d, o, e);
            const float v = f(pt[(long)o * x.so + e]);
            acc = fmaf(v, v, acc);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) norms[(long)cls * x.n + j] = acc;
        most = fmaxf(most, acc);
    }
    if (lane == 0) wmax[wave] = most;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < NORM_W; ++v) most = fmaxf(most, wmax[v]);
        parts[(long)cls * NP + p] = most;
    }
}

KgNnSetsArgs gram_as_sets(const KgNnGramArgs* a) {
    KgNnSetsArgs s = {};
    for (int g = 0; g < KG_NN_MAX_SETS; ++g) s.query[g] = a->query[g];
    s.q_sc = a->q_sc;  s.q_sp = a->q_sp;  s.q_so = a->q_so;  s.nsets = a->nsets;
    s.base = a->base;  s.b_sc = a->b_sc;  s.b_sp = a->b_sp;  s.b_so = a->b_so;
    s.Q = a->Q;  s.N = a->N;  s.d_outer = a->d_outer;  s.d_inner = a->d_inner;  s.classes = a->classes;  s.k = a->k;
    s.q_affine = a->q_affine;  s.b_affine = a->b_affine;
    s.q_scale = a->q_scale;  s.q_shift = a->q_shift;  s.b_scale = a->b_scale;  s.b_shift = a->b_shift;
    s.tile = a->tile;  s.split = a->split;
    s.idx = a->idx;  s.d2 = a->d2;  s.ws = a->ws;  s.ws_bytes = a->ws_bytes;
    return s;
}

int gram_cand(const KgNnGramArgs* a) {
    if (a->cand) return a->cand;
    const int want = a->k + 8 > 2 * a->k ? a->k + 8 : 2 * a->k;
    return want < KG_NN_MAX_K ? want : KG_NN_MAX_K;
}

int gram_validate(const KgNnGramArgs* a, const KgNnSetsArgs* s, const char* who) {
    KG_REQUIRE(a->nsets >= 1 && a->nsets <= KG_NN_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, a->nsets, KG_NN_MAX_SETS);
    KG_REQUIRE(!a->exclude_self || a->nsets == 1, "%s: exclude_self=%d needs nsets=%d to be 1", who, a->exclude_self, a->nsets);
    if (int rc = nn_validate(s, a->exclude_self, true, who)) return rc;
    KG_REQUIRE(a->k < KG_NN_MAX_K, "%s: k=%d leaves no cand in (k, %d]", who, a->k, KG_NN_MAX_K);
    KG_REQUIRE(a->cand == 0 || (a->cand > a->k && a->cand <= KG_NN_MAX_K), "%s: cand=%d is neither 0 (automatic) nor in (k=%d, %d]",
               who, a->cand, a->k, KG_NN_MAX_K);
    return 0;
}

int64_t gram_ws_bytes(const KgNnGramArgs* a, const NnPlan& p) {
    const int64_t cand = gram_cand(a);
    return (int64_t)a->nsets * a->classes * ((int64_t)a->Q * (8 * cand * (p.split + 1) + 8) + 4);
}

}  // namespace

extern "C" int kg_nn_norms(const KgNnGramArgs* a, float* norms, float* parts, void* stream) {
    const char* who = "kg_nn_norms";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->N >= 1, "%s: N=%d < 1", who, a->N);
    KG_REQUIRE(a->N <= KG_NN_MAX_POINTS, "%s: N=%d above the cap of %d points per class", who, a->N, KG_NN_MAX_POINTS);
    KG_REQUIRE(a->classes >= 1 && a->classes <= (1 << 16), "%s: classes=%d outside [1, 65536]", who, a->classes);
    KG_REQUIRE(a->d_outer >= 1, "%s: d_outer=%d < 1", who, a->d_outer);
    KG_REQUIRE(a->d_inner >= 1, "%s: d_inner=%d < 1", who, a->d_inner);
    KG_REQUIRE((long)a->d_outer * a->d_inner <= 0x7fffffffL, "%s: d_outer=%d x d_inner=%d does not fit 31 bits", who, a->d_outer,
               a->d_inner);
    KG_REQUIRE(a->base != nullptr, "%s: null pointer base", who);
    KG_REQUIRE(norms != nullptr, "%s: null pointer norms", who);
    KG_REQUIRE(parts != nullptr, "%s: null pointer parts", who);
    DistSet x;
    x.p = a->base;  x.sc = a->b_sc;  x.sp = a->b_sp;  x.so = a->b_so;  x.n = a->N;
    NnAffine f;
    f.on = a->b_affine ? 1 : 0;  f.scale = a->b_scale;  f.shift = a->b_shift;
    hipLaunchKernelGGL(kg_nn_norms_kernel, dim3((unsigned)a->classes * NP), dim3(NORM_W * 64), 0, (hipStream_t)stream, x, f,
                       FastDiv::make((unsigned)a->d_inner), a->d_outer * a->d_inner, norms, parts);
    return kg_launch_status(who);
}

extern "C" int64_t kg_nn_gram_workspace_bytes(const KgNnGramArgs* a) {
    const char* who = "kg_nn_gram_workspace_bytes";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    const KgNnSetsArgs s = gram_as_sets(a);
    if (int rc = gram_validate(a, &s, who)) return rc;
    return gram_ws_bytes(a, nn_plan(&s));
}

extern "C" int kg_nn_gram(const KgNnGramArgs* a, void* stream) {
    const char* who = "kg_nn_gram";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    const KgNnSetsArgs s = gram_as_sets(a);
    if (int rc = gram_validate(a, &s, who)) return rc;
    for (int g = 0; g < a->nsets; ++g) KG_REQUIRE(a->query[g] != nullptr, "%s: null pointer query[%d]", who, g);
    KG_REQUIRE(a->base != nullptr, "%s: null pointer base", who);
    KG_REQUIRE(a->b_norms != nullptr, "%s: null pointer b_norms", who);
    KG_REQUIRE(a->b_norm_parts != nullptr, "%s: null pointer b_norm_parts", who);
    KG_REQUIRE(a->idx != nullptr, "%s: null pointer idx", who);
    KG_REQUIRE(a->d2 != nullptr, "%s: null pointer d2", who);
    KG_REQUIRE(a->stats != nullptr, "%s: null pointer stats", who);
    KG_REQUIRE(a->ws != nullptr, "%s: null pointer ws", who);
    const NnPlan p = nn_plan(&s);
    const int64_t need = gram_ws_bytes(a, p);
    KG_REQUIRE(a->ws_bytes >= need, "%s: ws_bytes=%lld < %lld (%s_workspace_bytes)", who, (long long)a->ws_bytes, (long long)need,
               who);
    const int cand = gram_cand(a);
    const long S = (long)a->nsets * a->classes, rows = S * a->Q;
    hipStream_t st = (hipStream_t)stream;

    // the workspace: chunk lists (keys, then distances of the fallback), merged candidates, flags, row lists, their lengths
    float* pd = (float*)a->ws;
    int* pj = (int*)(pd + rows * p.split * cand);
    float* ckey = (float*)(pj + rows * p.split * cand);
    int* cidx = (int*)(ckey + rows * cand);
    int* flag = cidx + rows * cand;
    int* list = flag + rows;
    int* count = list + rows;

    NnDev e = nn_dev(&s, a->exclude_self, p);       // the exact search over the open rows
    e.pd = pd;  e.pj = pj;  e.rows = list;  e.nrows = count;
    NnDev f = e;                                    // the pre-filter: cand (key, j) per row into ckey / cidx
    f.k = cand;  f.d2 = ckey;  f.idx = cidx;  f.rows = nullptr;  f.nrows = nullptr;  f.bn = a->b_norms;
    GramDev g = {};
    g.n = e;  g.cand = cand;  g.ckey = ckey;  g.cidx = cidx;  g.parts = a->b_norm_parts;
    g.flag = flag;  g.list = list;  g.count = count;  g.stats = a->stats;
    // the constants of the certificate (include/kgan_hip.h prints the formula)
    const double u = 1.0 / 16777216.0, D = (double)e.D;
    const double eg = 1.01 * ((D < GR_BLOCK ? D : (double)GR_BLOCK) + (double)kg_cdiv(e.D, GR_BLOCK) + 4.0) * u;
    g.tau = (D + 4.0) * u;
    g.en = 1.01 * ((double)kg_cdiv(e.D, 64) + 8.0) * u;
    g.ecoef = (g.en + 2.0 * eg + 4.0 * u) * (1.0 + 2.0 * g.en);
    g.eabs = (D + 16.0) * 7.52316384526264e-37;     // 2^-120

    // 16-byte staging loads where every address they would form is a multiple of 16 bytes
    bool vec = a->d_inner % 4 == 0 && ((uintptr_t)a->base & 15) == 0;
    for (const int64_t st4 : {a->q_sc, a->q_sp, a->q_so, a->b_sc, a->b_sp, a->b_so}) vec = vec && st4 % 4 == 0;
    for (int q = 0; q < a->nsets; ++q) vec = vec && ((uintptr_t)a->query[q] & 15) == 0;
    const dim3 grid((unsigned)p.grid_search), block(DT_NT);
    if (p.ti == 32 && vec) hipLaunchKernelGGL((kg_nn_gram_search_kernel<32, true>), grid, block, 0, st, f);
    else if (p.ti == 32) hipLaunchKernelGGL((kg_nn_gram_search_kernel<32, false>), grid, block, 0, st, f);
    else if (vec) hipLaunchKernelGGL((kg_nn_gram_search_kernel<64, true>), grid, block, 0, st, f);
    else hipLaunchKernelGGL((kg_nn_gram_search_kernel<64, false>), grid, block, 0, st, f);
    if (int rc = kg_launch_status("kg_nn_gram_search")) return rc;
    hipLaunchKernelGGL(kg_nn_merge_kernel<false>, dim3((unsigned)p.grid_merge), dim3(NN_MW * 64), 0, st, f);
    if (int rc = kg_launch_status("kg_nn_gram_merge")) return rc;
    hipLaunchKernelGGL(kg_nn_gram_rescore_kernel, dim3((unsigned)((rows + RS_W - 1) / RS_W)), dim3(RS_W * 64), 0, st, g);
    if (int rc = kg_launch_status("kg_nn_gram_rescore")) return rc;
    hipLaunchKernelGGL(kg_nn_gram_compact_kernel, dim3((unsigned)S), dim3(256), 0, st, g);
    if (int rc = kg_launch_status("kg_nn_gram_compact")) return rc;
    return nn_launch<true>(e, p, "kg_nn_gram_fallback_search", "kg_nn_gram_fallback_merge", st);
}
