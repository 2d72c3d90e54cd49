// The search and merge kernels of kg_nn / kg_nn_sets (kg_nn.hip) with their plan, validation and launcher, shared with the
// matrix-core pre-filter kg_nn_gram (kg_nn_gram.hip).  See kg_nn.hip for the description of the kernels.
// IND: the rows of a (set, class) are not 0 .. Q - 1 but the entries of a list (NnDev::rows, its length NnDev::nrows) - the
// fallback of kg_nn_gram, which searches only the rows its certificate left open.  kg_nn and kg_nn_sets are the identity
// case (IND = false: no list is read, the code is the one they always ran).
#pragma once
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
    const int* rows;            // IND: (nsets, classes, Q) the listed rows of every (set, class), in front
    const int* nrows;           // IND: (nsets, classes) how many
    const float* bn;            // kg_nn_gram's pre-filter: (classes, N) squared norms of the base points
};

// the row list of a (set, class): position -> row (identity without a list)
struct NnRows {
    const int* list;
    __device__ __forceinline__ int operator()(int p) const { return list ? list[p] : p; }
};

template <int TI>
struct NnLists {
    static constexpr int CW = KG_NN_MAX_K + TI + 1;        // candidates of a row: [0, k) the best so far, [k, k + TI) the tile
    static constexpr int TPR = DT_NT / TI;                 // threads that rank the candidates of one row
};

// all k best so far (inf, INT_MAX)
template <int TI>
__device__ __forceinline__ void nn_lists_clear(float (*cand)[NnLists<TI>::CW], int (*cidx)[KG_NN_MAX_K]) {
    for (int e = threadIdx.x; e < TI * KG_NN_MAX_K; e += DT_NT) {
        cand[e / KG_NN_MAX_K][e % KG_NN_MAX_K] = INFINITY;
        cidx[e / KG_NN_MAX_K][e % KG_NN_MAX_K] = INT_MAX;
    }
}

// After a tile's TI new values of every row stand in cand[.][k, k + TI) (and a __syncthreads): merge them with the k best so
// far by rank under (value, position) - the best come from lower columns and are sorted, the tile's lie in column order, so
// this IS the order (value, j).  best / bidx: the destination, over the (dead) staging buffers.  Ends synchronised.
template <int TI>
__device__ __forceinline__ void nn_lists_merge(float (*cand)[NnLists<TI>::CW], int (*cidx)[KG_NN_MAX_K], float (*best)[KG_NN_MAX_K],
                                               float (*bidx)[KG_NN_MAX_K], int k, int j0) {
    constexpr int TPR = NnLists<TI>::TPR;
    const int tid = threadIdx.x;
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

// the chunk's list of the tile's rows to the workspace: position p of the tile is row rows(i0 + p) of the (set, class) sc
template <int TI>
__device__ __forceinline__ void nn_lists_store(const NnDev& a, float (*cand)[NnLists<TI>::CW], int (*cidx)[KG_NN_MAX_K], unsigned sc,
                                               unsigned ch, int i0, int nq, const NnRows& rows) {
    constexpr int TPR = NnLists<TI>::TPR;
    const int row = threadIdx.x / TPR, sub = threadIdx.x % TPR, i = i0 + row, k = a.k;
    if (i < nq) {
        const long o = (((long)sc * a.q.n + rows(i)) * a.split + ch) * k;
        for (int c = sub; c < k; c += TPR) {
            a.pd[o + c] = cand[row][c];
            a.pj[o + c] = cidx[row][c];
        }
    }
}

// the workgroup's place in the grid: (set, class), row tile, chunk; the query pointer of its set
struct NnPlace {
    unsigned sc, set, cls, rt, ch;
    const float* qp;
};
__device__ __forceinline__ NnPlace nn_place(const NnDev& a) {
    NnPlace w;
    const unsigned per = (unsigned)a.nrt * (unsigned)a.split;
    const unsigned t = blockIdx.x % per;
    w.sc = blockIdx.x / per;                                        // (set, class), then (row tile, chunk)
    w.set = w.sc / (unsigned)a.classes;  w.cls = w.sc % (unsigned)a.classes;
    w.rt = t / (unsigned)a.split;  w.ch = t % (unsigned)a.split;
    w.qp = a.q.p;
#pragma unroll
    for (int g = 1; g < KG_NN_MAX_SETS; ++g)
        if (w.set == (unsigned)g) w.qp = a.qs[g - 1];
    return w;
}

template <int TI, int MI, bool IND>
__global__ __launch_bounds__(DT_NT) void kg_nn_search_kernel(NnDev a) {
    static_assert(TI == 16 * MI, "tile / micro-tile mismatch");
    constexpr int CW = NnLists<TI>::CW;
    __shared__ __attribute__((aligned(16))) float stage[2][DT_KC][TI + DT_PAD];
    __shared__ float cand[TI][CW];
    __shared__ int cidx[TI][KG_NN_MAX_K];           // indices of cand[.][0, k)
    // the merge's destination lies over the staging buffers, which are dead between two tiles (the index as float bits)
    static_assert(2 * TI * KG_NN_MAX_K <= 2 * DT_KC * (TI + DT_PAD), "best / bidx do not fit the staging buffers");
    float (*si)[TI + DT_PAD] = stage[0];
    float (*sj)[TI + DT_PAD] = stage[1];
    float (*best)[KG_NN_MAX_K] = reinterpret_cast<float (*)[KG_NN_MAX_K]>(&stage[0][0][0]);
    float (*bidx)[KG_NN_MAX_K] = best + TI;

    const NnPlace w = nn_place(a);
    const unsigned sc = w.sc, cls = w.cls, ch = w.ch;
    const int i0 = (int)w.rt * TI, k = a.k;
    NnRows rows = {nullptr};
    int Q = a.q.n;
    if (IND) {                                      // (uniform: a tile past the end of the list leaves at once)
        Q = a.nrows[sc];
        if (i0 >= Q) return;
        rows.list = a.rows + (long)sc * a.q.n;
    }
    const long cb = (long)ch * a.chunk;             // the chunk: base points [cb, ce), empty when cb >= N
    const int ce = (int)min(cb + a.chunk, (long)a.b.n);
    DistSet B = a.b;
    B.n = ce;                                       // nothing beyond the chunk is read
    DistSet X = a.q;
    X.n = Q;
    const float* qb = w.qp + (long)cls * a.q.sc;
    const float* bb = a.b.p + (long)cls * a.b.sc;
    const int tid = threadIdx.x, ri = tid >> 4, rj = tid & 15;

    nn_lists_clear<TI>(cand, cidx);

    int self[MI];                                   // the row a pair i == j names (exclude_self)
#pragma unroll
    for (int r = 0; r < MI; ++r) {
        const int i = i0 + ri * MI + r;
        self[r] = IND ? (i < Q ? rows(i) : -1) : i;
    }

    const bool live = i0 + (tid >> 6) * 4 * MI < Q;
    for (long jl = cb; jl < ce; jl += TI) {
        const int j0 = (int)jl;
        float acc[MI][MI];
        if (IND) dist_tile<TI, MI>(acc, si, sj, a.D, a.inner, X, qb, i0, B, bb, j0, live, a.qa, a.ba, rows);
        else dist_tile<TI, MI>(acc, si, sj, a.D, a.inner, X, qb, i0, B, bb, j0, live, a.qa, a.ba);
#pragma unroll
        for (int r = 0; r < MI; ++r)
#pragma unroll
            for (int s = 0; s < MI; ++s) {
                const int i = i0 + ri * MI + r, j = j0 + rj * MI + s;
                cand[ri * MI + r][k + rj * MI + s] = (i >= Q || j >= ce || (a.exclude_self && self[r] == j)) ? INFINITY : acc[r][s];
            }
        __syncthreads();
        nn_lists_merge<TI>(cand, cidx, best, bidx, k, j0);
    }
    __syncthreads();            // (an empty chunk: the initial list)
    nn_lists_store<TI>(a, cand, cidx, sc, ch, i0, Q, rows);
}

template <bool IND>
__global__ __launch_bounds__(NN_MW * 64) void kg_nn_merge_kernel(NnDev a) {
    __shared__ float sv[NN_MW][KG_NN_MAX_SPLIT * KG_NN_MAX_K];
    __shared__ int sx[NN_MW][KG_NN_MAX_SPLIT * KG_NN_MAX_K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long rows = (long)a.nsets * a.classes * a.q.n;
    long row = (long)blockIdx.x * NN_MW + wave;
    const int nc = a.split * a.k, k = a.k;
    bool in = row < rows;
    if (IND && in) {                                // position `row` of the lists -> the row it names
        const long sc = row / a.q.n, p = row % a.q.n;
        in = p < a.nrows[sc];
        if (in) row = sc * a.q.n + a.rows[row];
    }
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
inline int nn_edge(long groups64) { return groups64 >= 512 ? 64 : 32; }

inline NnPlan nn_plan(const KgNnSetsArgs* a) {
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

// sets: the caller has nsets as a field of its own, and it is named (kg_nn_sets, kg_nn_gram); else kg_nn.  exclude_self is
// passed beside (kg_nn_sets has none)
inline int nn_validate(const KgNnSetsArgs* a, int exclude_self, bool sets, const char* who) {
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
    if (sets && !self) KG_REQUIRE(a->k <= a->N, "%s: k=%d > N=%d neighbours", who, a->k, a->N);
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

inline int64_t nn_ws_bytes(const KgNnSetsArgs* a, const NnPlan& p) {
    return (int64_t)a->nsets * a->classes * a->Q * p.split * a->k * 8;
}

// the launch's view of the arguments (the workspace pointers pd / pj and the lists are the caller's to set)
inline NnDev nn_dev(const KgNnSetsArgs* a, int exclude_self, const NnPlan& p) {
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
    d.d2 = a->d2;  d.idx = a->idx;
    return d;
}

// search, then merge: the two launches of the exact search (IND: over the listed rows only)
template <bool IND>
int nn_launch(const NnDev& d, const NnPlan& p, const char* search, const char* merge, hipStream_t s) {
    if (p.ti == 32) hipLaunchKernelGGL((kg_nn_search_kernel<32, 2, IND>), dim3((unsigned)p.grid_search), dim3(DT_NT), 0, s, d);
    else hipLaunchKernelGGL((kg_nn_search_kernel<64, 4, IND>), dim3((unsigned)p.grid_search), dim3(DT_NT), 0, s, d);
    if (int rc = kg_launch_status(search)) return rc;
    hipLaunchKernelGGL(kg_nn_merge_kernel<IND>, dim3((unsigned)p.grid_merge), dim3(NN_MW * 64), 0, s, d);
    return kg_launch_status(merge);
}

}  // namespace
