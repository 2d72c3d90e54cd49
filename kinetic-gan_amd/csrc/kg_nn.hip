// Exact k-nearest-neighbour search between two point sets of many classes in two launches (see include/kgan_hip.h,
// DESIGN.md 22).  Per class: Q query and N base points of dimension D; for every query the k base points with the smallest
// (d2, j) - squared distance, then base index - and their distances.
//
// kg_nn_search_kernel: one workgroup = TI queries of one class x one chunk of base points.  It walks the column tiles of its
// chunk; the squared distances of a TI x TI tile are the shared tile body of kg_prdc (kg_dist_tile.h: direct differences,
// one fmaf chain per pair in dimension order, so a pair's bits depend on the two points alone), the load going through the
// optional affine of its side ((x * scale) + shift as two separately rounded operations; staged zeros stay zero).  After
// each tile the k best (value, index) of every row are merged with the tile's TI new ones in LDS by the rank merge of
// kg_prdc_radii_kernel: the best so far come from lower columns and are sorted, the tile's candidates lie in column order,
// so "ties broken by position" IS the order (d2, j).  Only the best carry a stored index: tile candidate c is column
// j0 + c.  Pair i == j is left out by index when asked.  The chunk's list goes to the workspace; entries a short chunk
// cannot fill are (inf, INT_MAX).
// kg_nn_merge_kernel: one wave per (class, query); every one of the row's split * k candidates finds its rank under
// (d2, j, position) among all of them and the ones ranked below k are written at their rank.
// The order is total and no bit of a pair depends on the plan: every (tile, split) gives the same idx and d2.  No atomics,
// no tickets, no Q x N matrix, no scratch, no dynamically indexed private array.
// kg_nn_sets: up to KG_NN_MAX_SETS query sets with shared strides against ONE base in the same two launches -
// the workgroup index of the search is (set, class, row tile, chunk), a merge row is (set, class, query).  A set only chooses
// the query pointer and the output row, so every set's bits are those of kg_nn on it; kg_nn IS the one-set case: one
// kernel body, one plan, one launcher (nn_run).
// kg_nn_scores_kernel: from the nearest neighbour of every query of every set to the two memorisation tallies - authentic
// (d2 >= the neighbour's own leave-one-out distance) and agreeing (the neighbour carries the query's label) - one workgroup
// per set, integer LDS tallies, one owner per output word.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "kg_common.h"
#include "kg_dist_tile.h"

namespace {

constexpr int NN_MW = 4;                // waves (= rows) of a merge workgroup
constexpr long NN_MAX_GRID = 1L << 24;  // workgroups of a launch (exclusive): grid x 256 threads stays below 2^32

// (x * scale) + shift in two separately rounded operations - the arithmetic of kg_step_inputs (kg_input.hip: the compiler
// contracts the pair into one FMA by default, so contraction is off for this block); off: the value as stored
struct NnAffine {
    int on;
    float scale, shift;
    __device__ __forceinline__ float operator()(float x) const {
#pragma clang fp contract(off)
        const float p = x * scale;
        const float y = p + shift;
        return on ? y : x;
    }
};

struct NnDev {
    DistSet q, b;               // q.n = Q, b.n = N; q.p = the query set 0
    const float* qs[KG_NN_MAX_SETS - 1];    // the query sets 1 .. nsets - 1 (strides shared)
    int nsets;
    NnAffine qa, ba;
    FastDiv inner;              // dimension d = o * d_inner + e
    int D, classes, k, exclude_self;
    int nrt, split, chunk;      // row tiles per class; column chunks, base points of a chunk
    float* pd;  int* pj;        // ws: (nsets, classes, Q, split, k) distances, then as many indices
    float* d2;  int* idx;       // (nsets, classes, Q, k)
};

template <int TI, int MI>
__global__ __launch_bounds__(DT_NT) void kg_nn_search_kernel(NnDev a) {
    static_assert(TI == 16 * MI, "tile / micro-tile mismatch");
    constexpr int CW = KG_NN_MAX_K + TI + 1;        // candidates of a row: [0, k) the best so far, [k, k + TI) the tile
    constexpr int TPR = DT_NT / TI;                 // threads that rank the candidates of one row
    __shared__ __attribute__((aligned(16))) float stage[2][DT_KC][TI + DT_PAD];
    __shared__ float cand[TI][CW];
    __shared__ int cidx[TI][KG_NN_MAX_K];           // indices of cand[.][0, k)
    // the merge's destination lies over the staging buffers, which are dead between two tiles (the index as float bits)
    static_assert(2 * TI * KG_NN_MAX_K <= 2 * DT_KC * (TI + DT_PAD), "best / bidx do not fit the staging buffers");
    float (*si)[TI + DT_PAD] = stage[0];
    float (*sj)[TI + DT_PAD] = stage[1];
    float (*best)[KG_NN_MAX_K] = reinterpret_cast<float (*)[KG_NN_MAX_K]>(&stage[0][0][0]);
    float (*bidx)[KG_NN_MAX_K] = best + TI;

    const unsigned per = (unsigned)a.nrt * (unsigned)a.split;
    const unsigned sc = blockIdx.x / per, t = blockIdx.x % per;     // (set, class), then (row tile, chunk)
    const unsigned set = sc / (unsigned)a.classes, cls = sc % (unsigned)a.classes;
    const unsigned rt = t / (unsigned)a.split, ch = t % (unsigned)a.split;
    const int i0 = (int)rt * TI, k = a.k, Q = a.q.n;
    const long cb = (long)ch * a.chunk;             // the chunk: base points [cb, ce), empty when cb >= N
    const int ce = (int)min(cb + a.chunk, (long)a.b.n);
    DistSet B = a.b;
    B.n = ce;                                       // nothing beyond the chunk is read
    const float* qp = a.q.p;
#pragma unroll
    for (int g = 1; g < KG_NN_MAX_SETS; ++g)
        if (set == (unsigned)g) qp = a.qs[g - 1];
    const float* qb = qp + (long)cls * a.q.sc;
    const float* bb = a.b.p + (long)cls * a.b.sc;
    const int tid = threadIdx.x, ri = tid >> 4, rj = tid & 15;

    for (int e = tid; e < TI * KG_NN_MAX_K; e += DT_NT) {
        cand[e / KG_NN_MAX_K][e % KG_NN_MAX_K] = INFINITY;
        cidx[e / KG_NN_MAX_K][e % KG_NN_MAX_K] = INT_MAX;
    }

    const bool live = i0 + (tid >> 6) * 4 * MI < Q;
    for (long jl = cb; jl < ce; jl += TI) {
        const int j0 = (int)jl;
        float acc[MI][MI];
        dist_tile<TI, MI>(acc, si, sj, a.D, a.inner, a.q, qb, i0, B, bb, j0, live, a.qa, a.ba);
#pragma unroll
        for (int r = 0; r < MI; ++r)
#pragma unroll
            for (int s = 0; s < MI; ++s) {
                const int i = i0 + ri * MI + r, j = j0 + rj * MI + s;
                cand[ri * MI + r][k + rj * MI + s] = (i >= Q || j >= ce || (a.exclude_self && i == j)) ? INFINITY : acc[r][s];
            }
        __syncthreads();
        {
            const int row = tid / TPR, sub = tid % TPR, nc = k + TI;
            const float kth = cand[row][k - 1];
            for (int c = sub; c < nc; c += TPR) {
                const float v = cand[row][c];
                if (c >= k && !(v < kth)) continue;     // k entries in front of it are <= v: its rank is >= k
                int rank = 0;
                for (int b = 0; b < nc; ++b) {
                    const float w = cand[row][b];
                    rank += (w < v || (w == v && b < c)) ? 1 : 0;
                }
                if (rank < k) {
                    best[row][rank] = v;
                    bidx[row][rank] = __int_as_float(c < k ? cidx[row][c] : j0 + (c - k));
                }
            }
        }
        __syncthreads();
        {
            const int row = tid / TPR, sub = tid % TPR;
            for (int c = sub; c < k; c += TPR) {
                cand[row][c] = best[row][c];
                cidx[row][c] = __float_as_int(bidx[row][c]);
            }
        }
        __syncthreads();
    }
    __syncthreads();            // (an empty chunk: the initial list)
    {
        const int row = tid / TPR, sub = tid % TPR, i = i0 + row;
        if (i < Q) {
            const long o = (((long)sc * Q + i) * a.split + ch) * k;
            for (int c = sub; c < k; c += TPR) {
                a.pd[o + c] = cand[row][c];
                a.pj[o + c] = cidx[row][c];
            }
        }
    }
}

__global__ __launch_bounds__(NN_MW * 64) void kg_nn_merge_kernel(NnDev a) {
    __shared__ float sv[NN_MW][KG_NN_MAX_SPLIT * KG_NN_MAX_K];
    __shared__ int sx[NN_MW][KG_NN_MAX_SPLIT * KG_NN_MAX_K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long rows = (long)a.nsets * a.classes * a.q.n, row = (long)blockIdx.x * NN_MW + wave;
    const int nc = a.split * a.k, k = a.k;
    const bool in = row < rows;
    if (in) {
        for (int c = lane; c < nc; c += 64) {
            sv[wave][c] = a.pd[row * nc + c];
            sx[wave][c] = a.pj[row * nc + c];
        }
    }
    __syncthreads();
    if (!in) return;
    for (int c = lane; c < nc; c += 64) {
        const float v = sv[wave][c];
        const int j = sx[wave][c];
        int rank = 0;
        for (int b = 0; b < nc; ++b) {
            const float w = sv[wave][b];
            const int jb = sx[wave][b];
            rank += (w < v || (w == v && (jb < j || (jb == j && b < c)))) ? 1 : 0;
        }
        if (rank < k) {
            a.d2[row * k + rank] = v;
            a.idx[row * k + rank] = j;
        }
    }
}

// ---- kg_nn_scores: one workgroup per set ---------------------------------------------------------------------------------
constexpr int NS_NT = 256;                  // threads of the scores workgroup
constexpr int NS_MAXC = KG_NN_SCORES_MAX_CLASSES;

// set s = blockIdx.x.  The tallies are integers in LDS (integer addition does not depend on the order), the totals a shuffle
// tree and NS_NT / 64 words; every output word has one owner and is written on every call.  An index outside [0, N) is
// outside the definition: the query is SKIPPED (nothing is read for it, it counts nowhere); a query label outside
// [0, n_classes) counts in the totals and in no class.
__global__ __launch_bounds__(NS_NT) void kg_nn_scores_kernel(const KgNnScoresArgs a) {
    __shared__ int cls_s[NS_MAXC][2];
    __shared__ int tot_s[NS_NT / 64][2];
    const int tid = threadIdx.x, s = blockIdx.x, K = a.n_classes, Q = a.Q;
    for (int c = tid; c < K; c += NS_NT) { cls_s[c][0] = 0; cls_s[c][1] = 0; }
    __syncthreads();
    const int32_t* idx = a.idx + (long)s * Q * a.ld;
    const float* d2 = a.d2 + (long)s * Q * a.ld;
    int na = 0, ng = 0;
    for (int j = tid; j < Q; j += NS_NT) {
        const int i = idx[(long)j * a.ld];
        if (i < 0 || i >= a.N) continue;
        const int y = a.query_labels[j];
        const int au = d2[(long)j * a.ld] >= a.base_loo[i] ? 1 : 0;
        const int ag = a.base_labels[i] == y ? 1 : 0;
        na += au;
        ng += ag;
        if (a.counts_per_class && y >= 0 && y < K) {
            if (au) atomicAdd(&cls_s[y][0], 1);
            if (ag) atomicAdd(&cls_s[y][1], 1);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        na += __shfl_xor(na, off, 64);
        ng += __shfl_xor(ng, off, 64);
    }
    if ((tid & 63) == 0) { tot_s[tid >> 6][0] = na; tot_s[tid >> 6][1] = ng; }
    __syncthreads();
    if (a.counts_per_class)
        for (int c = tid; c < K; c += NS_NT) {
            a.counts_per_class[((long)s * K + c) * 2 + 0] = cls_s[c][0];
            a.counts_per_class[((long)s * K + c) * 2 + 1] = cls_s[c][1];
        }
    if (tid >= 2) return;
    long total = 0;
    for (int w = 0; w < NS_NT / 64; ++w) total += tot_s[w][tid];
    const double share = (double)total / (double)Q;
    a.counts[s * 2 + tid] = total;
    a.scores64[s * 2 + tid] = share;
    a.scores[s * 2 + tid] = (float)share;
}

struct NnPlan {
    int ti, split, chunk;
    long grid_search, grid_merge;
};

// The rule of prdc_edge (kg_prdc.hip) - the 64-tile once it alone gives every CU two workgroups (512 of them) - with the
// workgroups this launch can have: row tiles x column chunks.  The chunks then make up what the row tiles lack of 512,
// each a whole number of column tiles and at most KG_NN_MAX_SPLIT of them: 6000 x 40000 points run as 94 row tiles of 64
// x 7 chunks of 104 column tiles, 70 x 40000 as 3 row tiles of 32 x 32 chunks of 40.  A forced split cuts N into that
// many equal chunks of ceil(N / split) points, whatever the tile (tests: ragged and empty chunks at small shapes).
// The sets of kg_nn_sets count as row tiles: two sets of 6000 x 40000 run as 188 row tiles of 64 x 4 chunks of 208 column tiles.
int nn_edge(long groups64) { return groups64 >= 512 ? 64 : 32; }

NnPlan nn_plan(const KgNnSetsArgs* a) {
    NnPlan p;
    const long c64 = kg_cdiv(a->N, 64), sets = (long)a->nsets * a->classes;
    p.ti = a->tile ? a->tile : nn_edge(sets * kg_cdiv(a->Q, 64) * (c64 < KG_NN_MAX_SPLIT ? c64 : KG_NN_MAX_SPLIT));
    const long rows = sets * kg_cdiv(a->Q, p.ti);
    if (a->split) {
        p.split = a->split;
        p.chunk = kg_cdiv(a->N, a->split);
    } else {
        const long nt = kg_cdiv(a->N, p.ti);
        long want = (512 + rows - 1) / rows;
        if (want > nt) want = nt;
        if (want > KG_NN_MAX_SPLIT) want = KG_NN_MAX_SPLIT;
        long tiles = nt / want;                             // column tiles of a chunk: rounded down, so at least `want` chunks
        if ((nt + tiles - 1) / tiles > KG_NN_MAX_SPLIT) tiles = (nt + KG_NN_MAX_SPLIT - 1) / KG_NN_MAX_SPLIT;
        p.chunk = (int)(tiles * p.ti);                      // (<= N + 63)
        p.split = kg_cdiv(a->N, p.chunk);
    }
    p.grid_search = rows * p.split;
    p.grid_merge = (sets * a->Q + NN_MW - 1) / NN_MW;
    return p;
}

// the one-set call as the general one (its own fields: exclude_self, which a group of sets does not have)
KgNnSetsArgs nn_one_set(const KgNnArgs* a) {
    KgNnSetsArgs s = {};
    s.query[0] = a->query;  s.q_sc = a->q_sc;  s.q_sp = a->q_sp;  s.q_so = a->q_so;  s.nsets = 1;
    s.base = a->base;  s.b_sc = a->b_sc;  s.b_sp = a->b_sp;  s.b_so = a->b_so;
    s.Q = a->Q;  s.N = a->N;  s.d_outer = a->d_outer;  s.d_inner = a->d_inner;  s.classes = a->classes;  s.k = a->k;
    s.q_affine = a->q_affine;  s.b_affine = a->b_affine;
    s.q_scale = a->q_scale;  s.q_shift = a->q_shift;  s.b_scale = a->b_scale;  s.b_shift = a->b_shift;
    s.tile = a->tile;  s.split = a->split;
    s.idx = a->idx;  s.d2 = a->d2;  s.ws = a->ws;  s.ws_bytes = a->ws_bytes;
    return s;
}

// sets: the caller is kg_nn_sets (nsets is a field of its own and named); else kg_nn, whose exclude_self is passed beside
int nn_validate(const KgNnSetsArgs* a, int exclude_self, bool sets, const char* who) {
    if (sets)
        KG_REQUIRE(a->nsets >= 1 && a->nsets <= KG_NN_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, a->nsets, KG_NN_MAX_SETS);
    KG_REQUIRE(a->Q >= 1, "%s: Q=%d < 1", who, a->Q);
    KG_REQUIRE(a->N >= 1, "%s: N=%d < 1", who, a->N);
    KG_REQUIRE(a->classes >= 1, "%s: classes=%d < 1", who, a->classes);
    KG_REQUIRE(a->d_outer >= 1, "%s: d_outer=%d < 1", who, a->d_outer);
    KG_REQUIRE(a->d_inner >= 1, "%s: d_inner=%d < 1", who, a->d_inner);
    KG_REQUIRE((long)a->d_outer * a->d_inner <= 0x7fffffffL, "%s: d_outer=%d x d_inner=%d does not fit 31 bits", who, a->d_outer,
               a->d_inner);
    KG_REQUIRE(a->Q <= KG_NN_MAX_POINTS, "%s: Q=%d above the cap of %d points per class", who, a->Q, KG_NN_MAX_POINTS);
    KG_REQUIRE(a->N <= KG_NN_MAX_POINTS, "%s: N=%d above the cap of %d points per class", who, a->N, KG_NN_MAX_POINTS);
    KG_REQUIRE(a->k >= 1 && a->k <= KG_NN_MAX_K, "%s: k=%d outside [1, %d]", who, a->k, KG_NN_MAX_K);
    const int self = exclude_self ? 1 : 0;
    if (sets) KG_REQUIRE(a->k <= a->N, "%s: k=%d > N=%d neighbours", who, a->k, a->N);
    else KG_REQUIRE(a->k <= a->N - self, "%s: k=%d > N=%d - %d neighbours (exclude_self=%d)", who, a->k, a->N, self, exclude_self);
    KG_REQUIRE(a->tile == 0 || a->tile == 32 || a->tile == 64, "%s: tile=%d is none of 0 (automatic), 32, 64", who, a->tile);
    KG_REQUIRE(a->split >= 0 && a->split <= KG_NN_MAX_SPLIT && a->split <= a->N,
               "%s: split=%d outside [0 (automatic), min(%d, N=%d)]", who, a->split, KG_NN_MAX_SPLIT, a->N);
    const NnPlan p = nn_plan(a);
    // gridDim.x * blockDim.x has to stay below 2^32 for the runtime to take the launch: below 2^24 workgroups of 256 threads
    const long most = p.grid_search > p.grid_merge ? p.grid_search : p.grid_merge;
    if (sets)
        KG_REQUIRE(most < NN_MAX_GRID, "%s: nsets=%d x classes=%d x Q=%d x split=%d make %ld workgroups, one launch takes fewer than %ld",
                   who, a->nsets, a->classes, a->Q, p.split, most, NN_MAX_GRID);
    else
        KG_REQUIRE(most < NN_MAX_GRID, "%s: classes=%d x Q=%d x split=%d make %ld workgroups, one launch takes fewer than %ld", who,
                   a->classes, a->Q, p.split, most, NN_MAX_GRID);
    return 0;
}

int64_t nn_ws_bytes(const KgNnSetsArgs* a, const NnPlan& p) {
    return (int64_t)a->nsets * a->classes * a->Q * p.split * a->k * 8;
}

template <int TI, int MI>
void nn_launch_search(const NnDev& d, long grid, hipStream_t s) {
    hipLaunchKernelGGL((kg_nn_search_kernel<TI, MI>), dim3((unsigned)grid), dim3(DT_NT), 0, s, d);
}

// the one launcher: search, then merge, of nsets sets (validated by the caller)
int nn_run(const KgNnSetsArgs* a, int exclude_self, bool sets, const char* who, void* stream) {
    if (sets) {
        for (int g = 0; g < a->nsets; ++g) KG_REQUIRE(a->query[g] != nullptr, "%s: null pointer query[%d]", who, g);
    } else {
        KG_REQUIRE(a->query[0] != nullptr, "%s: null pointer query", who);
    }
    KG_REQUIRE(a->base != nullptr, "%s: null pointer base", who);
    KG_REQUIRE(a->idx != nullptr, "%s: null pointer idx", who);
    KG_REQUIRE(a->d2 != nullptr, "%s: null pointer d2", who);
    KG_REQUIRE(a->ws != nullptr, "%s: null pointer ws", who);
    const NnPlan p = nn_plan(a);
    const int64_t need = nn_ws_bytes(a, p);
    KG_REQUIRE(a->ws_bytes >= need, "%s: ws_bytes=%lld < %lld (%s_workspace_bytes)", who, (long long)a->ws_bytes, (long long)need,
               who);

    NnDev d = {};
    d.q.p = a->query[0];  d.q.sc = a->q_sc;  d.q.sp = a->q_sp;  d.q.so = a->q_so;  d.q.n = a->Q;
    for (int g = 1; g < a->nsets; ++g) d.qs[g - 1] = a->query[g];
    d.nsets = a->nsets;
    d.b.p = a->base;  d.b.sc = a->b_sc;  d.b.sp = a->b_sp;  d.b.so = a->b_so;  d.b.n = a->N;
    d.qa.on = a->q_affine ? 1 : 0;  d.qa.scale = a->q_scale;  d.qa.shift = a->q_shift;
    d.ba.on = a->b_affine ? 1 : 0;  d.ba.scale = a->b_scale;  d.ba.shift = a->b_shift;
    d.inner = FastDiv::make((unsigned)a->d_inner);
    d.D = a->d_outer * a->d_inner;  d.classes = a->classes;  d.k = a->k;  d.exclude_self = exclude_self ? 1 : 0;
    d.nrt = kg_cdiv(a->Q, p.ti);  d.split = p.split;  d.chunk = p.chunk;
    d.pd = (float*)a->ws;
    d.pj = (int*)(d.pd + (long)a->nsets * a->classes * a->Q * p.split * a->k);
    d.d2 = a->d2;  d.idx = a->idx;
    hipStream_t s = (hipStream_t)stream;

    if (p.ti == 32) nn_launch_search<32, 2>(d, p.grid_search, s);
    else nn_launch_search<64, 4>(d, p.grid_search, s);
    if (int rc = kg_launch_status(sets ? "kg_nn_sets_search" : "kg_nn_search")) return rc;
    hipLaunchKernelGGL(kg_nn_merge_kernel, dim3((unsigned)p.grid_merge), dim3(NN_MW * 64), 0, s, d);
    return kg_launch_status(sets ? "kg_nn_sets_merge" : "kg_nn_merge");
}

}  // namespace

extern "C" int64_t kg_nn_workspace_bytes(const KgNnArgs* a) {
    KG_REQUIRE(a != nullptr, "kg_nn_workspace_bytes: null args");
    const KgNnSetsArgs s = nn_one_set(a);
    if (int rc = nn_validate(&s, a->exclude_self, false, "kg_nn_workspace_bytes")) return rc;
    return nn_ws_bytes(&s, nn_plan(&s));
}

extern "C" int kg_nn(const KgNnArgs* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_nn: null args");
    const KgNnSetsArgs s = nn_one_set(a);
    if (int rc = nn_validate(&s, a->exclude_self, false, "kg_nn")) return rc;
    return nn_run(&s, a->exclude_self, false, "kg_nn", stream);
}

extern "C" int64_t kg_nn_sets_workspace_bytes(const KgNnSetsArgs* a) {
    KG_REQUIRE(a != nullptr, "kg_nn_sets_workspace_bytes: null args");
    if (int rc = nn_validate(a, 0, true, "kg_nn_sets_workspace_bytes")) return rc;
    return nn_ws_bytes(a, nn_plan(a));
}

extern "C" int kg_nn_sets(const KgNnSetsArgs* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_nn_sets: null args");
    if (int rc = nn_validate(a, 0, true, "kg_nn_sets")) return rc;
    return nn_run(a, 0, true, "kg_nn_sets", stream);
}

extern "C" int kg_nn_scores(const KgNnScoresArgs* a, void* stream) {
    const char* who = "kg_nn_scores";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->nsets >= 1 && a->nsets <= KG_NN_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, a->nsets, KG_NN_MAX_SETS);
    KG_REQUIRE(a->Q >= 1, "%s: Q=%d < 1", who, a->Q);
    KG_REQUIRE(a->N >= 1, "%s: N=%d < 1", who, a->N);
    KG_REQUIRE(a->Q <= KG_NN_MAX_POINTS, "%s: Q=%d above the cap of %d points", who, a->Q, KG_NN_MAX_POINTS);
    KG_REQUIRE(a->N <= KG_NN_MAX_POINTS, "%s: N=%d above the cap of %d points", who, a->N, KG_NN_MAX_POINTS);
    KG_REQUIRE(a->n_classes >= 1 && a->n_classes <= NS_MAXC, "%s: n_classes=%d outside [1, %d]", who, a->n_classes, NS_MAXC);
    KG_REQUIRE(a->ld >= 1, "%s: ld=%lld < 1", who, (long long)a->ld);
    KG_REQUIRE(a->idx != nullptr, "%s: null pointer idx", who);
    KG_REQUIRE(a->d2 != nullptr, "%s: null pointer d2", who);
    KG_REQUIRE(a->query_labels != nullptr, "%s: null pointer query_labels", who);
    KG_REQUIRE(a->base_labels != nullptr, "%s: null pointer base_labels", who);
    KG_REQUIRE(a->base_loo != nullptr, "%s: null pointer base_loo", who);
    KG_REQUIRE(a->counts != nullptr, "%s: null pointer counts", who);
    KG_REQUIRE(a->scores64 != nullptr, "%s: null pointer scores64", who);
    KG_REQUIRE(a->scores != nullptr, "%s: null pointer scores", who);
    hipLaunchKernelGGL(kg_nn_scores_kernel, dim3(a->nsets), dim3(NS_NT), 0, (hipStream_t)stream, *a);
    return kg_launch_status(who);
}
