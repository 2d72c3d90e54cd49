// Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) of many classes in
// three launches (see include/kgan_hip.h).  Per class: n real and m fake points of dimension D.
//
// kg_prdc_radii_kernel: one workgroup = TI rows of one (class, set in {real, fake}).  It walks every column tile of the same
// set; the squared distances of a TI x TI tile are accumulated as kg_mmd does it (PR_KC dimensions of the row and the
// column points staged in LDS, MI x MI pairs per thread, direct differences on the VALU, one fmaf chain per pair in
// dimension order - no |a|^2 + |b|^2 - 2ab, and the same bits under every tile plan).  After each tile the k smallest
// distances seen so far of every row are merged with the tile's TI new ones IN LDS: every candidate finds its rank among
// the row's k + TI candidates (ties broken by position, so the ranks are a permutation) and the ones ranked below k are
// stored at their rank.  rho = entry k - 1 after the last tile.  The self pair is left out by INDEX.  The same launch clears
// the flag / hit words of its rows, which the cross launch accumulates into.
// kg_prdc_cross_kernel: one workgroup = one TI x TI tile of the (real i, fake j) space of a class.  From the distances in
// registers: P = [d <= rho_R(i)], Q = [d <= rho_F(j)]; row ORs of Q (bit 0: recall) and P (bit 1: coverage) and column
// counts of P (precision / density) are reduced through lane shuffles and LDS and leave the tile as one integer atomic per
// row and column that has something to add.  Integer OR / add: the result does not depend on the order.
// kg_prdc_finish_kernel: one workgroup; per class the four counts, the four quotients (evaluated in double, rounded once)
// and the class means (fp64 sum in class order, rounded once); copies hits / flags to the caller's arrays.
// No n x n or n x m matrix is written; no scratch; no dynamically indexed private array.
//
// Several fake sets against one real set (kg_prdc_sets) are the SAME three kernels: a fake set g is one more
// leading index - its base pointer from a table of KG_PRDC_MAX_SETS, its radii / hit / flag words at (g * classes + c) - and
// the real radii are an input, so the radii launch has row-tile workgroups for fake rows only (they also clear the flag
// words of their (set, class), which the real rows clear in kg_prdc).  kg_prdc is the case of one set with the real rows in
// the radii launch; kg_prdc_radii is the radii launch of one set alone.  The tile body is shared: no bit depends on the
// grouping.
#include <float.h>
#include <math.h>

#include "kg_common.h"
#include "kg_dist_tile.h"

namespace {

constexpr int PR_NT = DT_NT;    // threads of a tile workgroup, dimensions staged per chunk and row padding: the shared
constexpr int PR_KC = DT_KC;    // tile's (kg_dist_tile.h)
constexpr int PR_PAD = DT_PAD;
constexpr int PR_FIN = 1024;    // threads of the finishing workgroup
constexpr long PR_MAX_GRID = 1L << 24;  // workgroups of a tile launch (exclusive): grid x PR_NT threads stays below 2^32

using PrdcSet = DistSet;

struct PrdcDev {
    PrdcSet set[2];             // 0 = real, 1 = fake (its p: fake set 0)
    const float* fp[KG_PRDC_MAX_SETS];  // base pointers of the fake sets (strides and m shared: set[1])
    FastDiv inner;              // dimension d = o * d_inner + e
    int D, classes, k, nsets;
    float* rho[2];              // (classes, n), (nsets, classes, m): ws, or the caller's real radii (an input of kg_prdc_sets)
    float* rho_out[2];          // the caller's radii arrays or null
    int* flags;                 // ws: (nsets, classes, n)  bit 0 = exists j Q_ij, bit 1 = exists j P_ij; null: kg_prdc_radii
    int* hits;                  // ws: (nsets, classes, m)  sum_i P_ij; null: kg_prdc_radii
    int nrt[2];                 // radii launch: row tiles of the real set (0: it takes no part) and of EACH fake set
    int nti, ntj;               // cross launch: tiles along i and j
};

struct PrdcFin {
    const int* flags;  const int* hits;
    int32_t* hits_out;  uint8_t* flags_out;
    int32_t* counts;  float* values;  float* mean;
    int n, m, classes, k, nsets;
};

// the tile body (kg_dist_tile.h) on two sets of this launch, the values as stored
template <int TI, int MI>
__device__ __forceinline__ void prdc_tile(float (&acc)[MI][MI], float (*si)[TI + PR_PAD], float (*sj)[TI + PR_PAD],
                                          const PrdcDev& a, const PrdcSet& X, const float* xb, int i0, const PrdcSet& Y,
                                          const float* yb, int j0, bool live) {
    dist_tile<TI, MI>(acc, si, sj, a.D, a.inner, X, xb, i0, Y, yb, j0, live, DistIdentity(), DistIdentity());
}

template <int TI, int MI>
__global__ __launch_bounds__(PR_NT) void kg_prdc_radii_kernel(PrdcDev a) {
    static_assert(TI == 16 * MI, "tile / micro-tile mismatch");
    constexpr int CW = KG_PRDC_MAX_K + TI + 1;      // candidates of a row: [0, k) the best so far, [k, k + TI) the tile
    constexpr int TPR = PR_NT / TI;                 // threads that rank the candidates of one row
    __shared__ __attribute__((aligned(16))) float si[PR_KC][TI + PR_PAD];
    __shared__ __attribute__((aligned(16))) float sj[PR_KC][TI + PR_PAD];
    __shared__ float cand[TI][CW];
    __shared__ float best[TI][KG_PRDC_MAX_K];

    // per class: the row tiles of the real set (if it takes part), then those of fake set 0, 1, ..
    const unsigned per = (unsigned)a.nrt[0] + (unsigned)a.nsets * (unsigned)a.nrt[1];
    const unsigned cls = blockIdx.x / per, t = blockIdx.x % per;
    const int set = t >= (unsigned)a.nrt[0] ? 1 : 0;
    const unsigned u = t - (set ? (unsigned)a.nrt[0] : 0u);
    const unsigned g = set ? u / (unsigned)a.nrt[1] : 0u;          // the fake set
    const unsigned rt = set ? u % (unsigned)a.nrt[1] : u;          // its row tile
    const int i0 = (int)rt * TI;
    PrdcSet X = a.set[set];
    if (set) X.p = a.fp[g];
    const int n = X.n, k = a.k;
    const float* xb = X.p + (long)cls * X.sc;
    const long row0 = ((long)g * a.classes + cls) * n;             // of this (set, class) in rho / hits (real: g = 0)
    const int tid = threadIdx.x, ri = tid >> 4, rj = tid & 15;

    // the words the cross launch accumulates into: real rows own the flags, fake rows the hit counts; without real rows
    // in the launch the workgroups of a fake (set, class) share out its flag words
    {
        int* own = set ? a.hits : a.flags;
        if (own != nullptr && tid < TI && i0 + tid < n) own[row0 + i0 + tid] = 0;
        if (set && a.nrt[0] == 0 && a.flags != nullptr) {
            const int nr = a.set[0].n;
            int* fl = a.flags + ((long)g * a.classes + cls) * nr;
            for (int i = (int)rt * PR_NT + tid; i < nr; i += a.nrt[1] * PR_NT) fl[i] = 0;
        }
    }
    for (int e = tid; e < TI * KG_PRDC_MAX_K; e += PR_NT) cand[e / KG_PRDC_MAX_K][e % KG_PRDC_MAX_K] = INFINITY;

    const bool live = i0 + (tid >> 6) * 4 * MI < n;
    const int ntj = (n + TI - 1) / TI;
    for (int jt = 0; jt < ntj; ++jt) {
        const int j0 = jt * TI;
        float acc[MI][MI];
        prdc_tile<TI, MI>(acc, si, sj, a, X, xb, i0, X, xb, j0, live);
#pragma unroll
        for (int r = 0; r < MI; ++r)
#pragma unroll
            for (int s = 0; s < MI; ++s) {
                const int i = i0 + ri * MI + r, j = j0 + rj * MI + s;
                cand[ri * MI + r][k + rj * MI + s] = (i >= n || j >= n || i == j) ? INFINITY : acc[r][s];
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
                if (rank < k) best[row][rank] = v;
            }
        }
        __syncthreads();
        {
            const int row = tid / TPR, sub = tid % TPR;
            for (int c = sub; c < k; c += TPR) cand[row][c] = best[row][c];
        }
        __syncthreads();
    }
    if (tid < TI && i0 + tid < n) {
        const float rho = cand[tid][k - 1];
        a.rho[set][row0 + i0 + tid] = rho;
        if (a.rho_out[set] != nullptr) a.rho_out[set][row0 + i0 + tid] = rho;
    }
}

template <int TI, int MI>
__global__ __launch_bounds__(PR_NT) void kg_prdc_cross_kernel(PrdcDev a) {
    static_assert(TI == 16 * MI, "tile / micro-tile mismatch");
    __shared__ __attribute__((aligned(16))) float si[PR_KC][TI + PR_PAD];
    __shared__ __attribute__((aligned(16))) float sj[PR_KC][TI + PR_PAD];
    __shared__ int srow[TI];
    __shared__ int scol[PR_NT / 64][TI];

    const unsigned ntiles = (unsigned)a.nti * (unsigned)a.ntj;
    const unsigned gc = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;      // gc = set * classes + class
    const unsigned g = gc / (unsigned)a.classes, cls = gc % (unsigned)a.classes;
    const int i0 = (int)(tile / (unsigned)a.ntj) * TI, j0 = (int)(tile % (unsigned)a.ntj) * TI;
    const PrdcSet R = a.set[0];
    PrdcSet F = a.set[1];
    F.p = a.fp[g];
    const int n = R.n, m = F.n;
    const int tid = threadIdx.x, ri = tid >> 4, rj = tid & 15, wave = tid >> 6;
    const bool live = i0 + wave * 4 * MI < n;

    float acc[MI][MI];
    prdc_tile<TI, MI>(acc, si, sj, a, R, R.p + (long)cls * R.sc, i0, F, F.p + (long)cls * F.sc, j0, live);

    float rr[MI], rf[MI];
#pragma unroll
    for (int r = 0; r < MI; ++r) {
        const int i = i0 + ri * MI + r, j = j0 + rj * MI + r;
        rr[r] = i < n ? a.rho[0][(long)cls * n + i] : 0.f;
        rf[r] = j < m ? a.rho[1][(long)gc * m + j] : 0.f;
    }
    int rowbits[MI], colcnt[MI];
#pragma unroll
    for (int r = 0; r < MI; ++r) rowbits[r] = colcnt[r] = 0;
#pragma unroll
    for (int r = 0; r < MI; ++r)
#pragma unroll
        for (int s = 0; s < MI; ++s) {
            const bool valid = i0 + ri * MI + r < n && j0 + rj * MI + s < m;
            const int P = (valid && acc[r][s] <= rr[r]) ? 1 : 0;
            const int Q = (valid && acc[r][s] <= rf[s]) ? 1 : 0;
            rowbits[r] |= Q | (P << 1);
            colcnt[s] += P;
        }
    // a row lives in the 16 lanes that share ri; a column in the lanes rj, rj + 16, rj + 32, rj + 48 of each wave
#pragma unroll
    for (int r = 0; r < MI; ++r) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) rowbits[r] |= __shfl_xor(rowbits[r], off, 64);
        colcnt[r] += __shfl_xor(colcnt[r], 16, 64);
        colcnt[r] += __shfl_xor(colcnt[r], 32, 64);
        if (rj == 0) srow[ri * MI + r] = rowbits[r];
        if ((tid & 63) < 16) scol[wave][rj * MI + r] = colcnt[r];
    }
    __syncthreads();
    if (tid < TI) {
        const int i = i0 + tid, v = srow[tid];
        if (i < n && v != 0) atomicOr(&a.flags[(long)gc * n + i], v);
    } else if (tid < 2 * TI) {
        const int c = tid - TI, j = j0 + c;
        const int v = (scol[0][c] + scol[1][c]) + (scol[2][c] + scol[3][c]);
        if (j < m && v != 0) atomicAdd(&a.hits[(long)gc * m + j], v);
    }
}

__device__ __forceinline__ int prdc_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(PR_FIN) void kg_prdc_finish_kernel(PrdcFin a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = PR_FIN / 64;
    for (int c = wave; c < a.nsets * a.classes; c += NW) {       // c = set * classes + class
        int cP = 0, cR = 0, cD = 0, cC = 0;
        for (int j = lane; j < a.m; j += 64) {
            const int h = a.hits[(long)c * a.m + j];
            cP += h > 0 ? 1 : 0;
            cD += h;
            if (a.hits_out != nullptr) a.hits_out[(long)c * a.m + j] = h;
        }
        for (int i = lane; i < a.n; i += 64) {
            const int f = a.flags[(long)c * a.n + i];
            cR += f & 1;
            cC += (f >> 1) & 1;
            if (a.flags_out != nullptr) a.flags_out[(long)c * a.n + i] = (uint8_t)f;
        }
        cP = prdc_wave_sum(cP);  cR = prdc_wave_sum(cR);  cD = prdc_wave_sum(cD);  cC = prdc_wave_sum(cC);
        if (lane == 0) {
            a.counts[c * 4 + 0] = cP;  a.counts[c * 4 + 1] = cR;  a.counts[c * 4 + 2] = cD;  a.counts[c * 4 + 3] = cC;
            a.values[c * 4 + 0] = (float)((double)cP / (double)a.m);
            a.values[c * 4 + 1] = (float)((double)cR / (double)a.n);
            a.values[c * 4 + 2] = (float)((double)cD / ((double)a.k * (double)a.m));
            a.values[c * 4 + 3] = (float)((double)cC / (double)a.n);
        }
    }
    if (a.mean == nullptr) return;
    __syncthreads();
    if (tid < 4 * a.nsets) {
        const int g = tid >> 2, q = tid & 3;
        double s = 0.0;
        for (int c = 0; c < a.classes; ++c) s += (double)a.values[((long)g * a.classes + c) * 4 + q];
        a.mean[tid] = (float)(s / a.classes);
    }
}

struct PrdcPlan {
    int ti_radii, ti_cross;     // tile edges: 32 (2 x 2 pairs per thread) or 64 (4 x 4)
    long grid_radii, grid_cross;
};

// The 64-tile has the better ratio of LDS reads to arithmetic (8 floats read for 16 pairs against 4 for 4); the 32-tile
// makes four times as many workgroups.  A launch takes the 64-tile once that alone gives every CU two workgroups
// (512 of them).  The two launches choose separately: the cross launch has one workgroup per TILE, so with one class it
// moves to 64-tiles from about 1500 x 1500 points (and 6 classes of 600 x 600 do); the radii launch has one per ROW tile
// only, so it stays on 32-tiles until classes * (n + m) reaches about 32768 points - one class of 4096 + 4096 gives 128
// row tiles of 64 and runs its radii on 32-tiles.  The protocol's 60 x (100 + 100) runs both launches on 32-tiles.
int prdc_edge(long groups64) { return groups64 >= 512 ? 64 : 32; }

// gc: (set, class) pairs; n_radii: the real rows of the radii launch (n: kg_prdc, 0: kg_prdc_sets, whose real radii are given)
PrdcPlan prdc_plan(long gc, int n_radii, int n, int m) {
    PrdcPlan p;
    p.ti_radii = prdc_edge(gc * ((long)kg_cdiv(n_radii, 64) + kg_cdiv(m, 64)));
    p.grid_radii = gc * ((long)kg_cdiv(n_radii, p.ti_radii) + kg_cdiv(m, p.ti_radii));
    p.ti_cross = prdc_edge(gc * kg_cdiv(n, 64) * kg_cdiv(m, 64));
    p.grid_cross = gc * kg_cdiv(n, p.ti_cross) * kg_cdiv(m, p.ti_cross);
    return p;
}
PrdcPlan prdc_plan(const KgPrdcArgs* a) { return prdc_plan(a->classes, a->n, a->n, a->m); }

// The shape requirements of every entry point, in the order their callers are told about them.  m null: one set alone
// (kg_prdc_radii).
int prdc_check_shape(const char* who, int n, const int32_t* m, int classes, int d_outer, int d_inner, int k) {
    KG_REQUIRE(n >= 1, "%s: n=%d < 1", who, n);
    KG_REQUIRE(m == nullptr || *m >= 1, "%s: m=%d < 1", who, m ? *m : 0);
    KG_REQUIRE(classes >= 1, "%s: classes=%d < 1", who, classes);
    KG_REQUIRE(d_outer >= 1, "%s: d_outer=%d < 1", who, d_outer);
    KG_REQUIRE(d_inner >= 1, "%s: d_inner=%d < 1", who, d_inner);
    KG_REQUIRE((long)d_outer * d_inner <= 0x7fffffffL, "%s: d_outer=%d x d_inner=%d does not fit 31 bits", who, d_outer, d_inner);
    KG_REQUIRE(k >= 1 && k <= KG_PRDC_MAX_K, "%s: k=%d outside [1, %d]", who, k, KG_PRDC_MAX_K);
    KG_REQUIRE(n <= KG_PRDC_MAX_POINTS, "%s: n=%d above the cap of %d points per class", who, n, KG_PRDC_MAX_POINTS);
    if (m == nullptr) {
        KG_REQUIRE(k <= n - 1, "%s: k=%d > n=%d - 1 neighbours", who, k, n);
        return 0;
    }
    KG_REQUIRE(*m <= KG_PRDC_MAX_POINTS, "%s: m=%d above the cap of %d points per class", who, *m, KG_PRDC_MAX_POINTS);
    KG_REQUIRE(k <= (n < *m ? n : *m) - 1, "%s: k=%d > min(n=%d, m=%d) - 1 neighbours", who, k, n, *m);
    return 0;
}

int prdc_validate(const KgPrdcArgs* a, const char* who) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    if (int rc = prdc_check_shape(who, a->n, &a->m, a->classes, a->d_outer, a->d_inner, a->k)) return rc;
    const PrdcPlan p = prdc_plan(a);
    // gridDim.x * blockDim.x has to stay below 2^32 for the runtime to take the launch: below 2^24 workgroups of 256 threads
    KG_REQUIRE(p.grid_radii < PR_MAX_GRID && p.grid_cross < PR_MAX_GRID,
               "%s: classes=%d x tiles of n=%d x m=%d make %ld workgroups, one launch takes fewer than %ld", who, a->classes, a->n,
               a->m, p.grid_cross > p.grid_radii ? p.grid_cross : p.grid_radii, PR_MAX_GRID);
    return 0;
}

int64_t prdc_ws_bytes(const KgPrdcArgs* a) { return (int64_t)a->classes * ((int64_t)a->n + a->m) * 8; }

template <int TI, int MI>
void prdc_launch_radii(const PrdcDev& d, long grid, hipStream_t s) {
    hipLaunchKernelGGL((kg_prdc_radii_kernel<TI, MI>), dim3((unsigned)grid), dim3(PR_NT), 0, s, d);
}
template <int TI, int MI>
void prdc_launch_cross(const PrdcDev& d, long grid, hipStream_t s) {
    hipLaunchKernelGGL((kg_prdc_cross_kernel<TI, MI>), dim3((unsigned)grid), dim3(PR_NT), 0, s, d);
}

// the finish launch on the flag / hit words of d; `what`: the entry point's name for the launch in the messages
int prdc_finish(const PrdcDev& d, int32_t* hits_out, uint8_t* flags_out, int32_t* counts, float* values, float* mean,
                hipStream_t s, const char* what) {
    PrdcFin fin;
    fin.flags = d.flags;  fin.hits = d.hits;
    fin.hits_out = hits_out;  fin.flags_out = flags_out;
    fin.counts = counts;  fin.values = values;  fin.mean = mean;
    fin.n = d.set[0].n;  fin.m = d.set[1].n;  fin.classes = d.classes;  fin.k = d.k;  fin.nsets = d.nsets;
    hipLaunchKernelGGL(kg_prdc_finish_kernel, dim3(1), dim3(PR_FIN), 0, s, fin);
    return kg_launch_status(what);
}

}  // namespace

extern "C" int64_t kg_prdc_workspace_bytes(const KgPrdcArgs* a) {
    if (int rc = prdc_validate(a, "kg_prdc_workspace_bytes")) return rc;
    return prdc_ws_bytes(a);
}

extern "C" int kg_prdc(const KgPrdcArgs* a, void* stream) {
    if (int rc = prdc_validate(a, "kg_prdc")) return rc;
    KG_REQUIRE(a->real != nullptr, "kg_prdc: null pointer real");
    KG_REQUIRE(a->fake != nullptr, "kg_prdc: null pointer fake");
    KG_REQUIRE(a->counts != nullptr, "kg_prdc: null pointer counts");
    KG_REQUIRE(a->values != nullptr, "kg_prdc: null pointer values");
    KG_REQUIRE(a->ws != nullptr, "kg_prdc: null pointer ws");
    const int64_t need = prdc_ws_bytes(a);
    KG_REQUIRE(a->ws_bytes >= need, "kg_prdc: ws_bytes=%lld < %lld (kg_prdc_workspace_bytes)", (long long)a->ws_bytes,
               (long long)need);
    const PrdcPlan p = prdc_plan(a);
    const long cn = (long)a->classes * a->n, cm = (long)a->classes * a->m;

    PrdcDev d = {};
    d.nsets = 1;  d.fp[0] = a->fake;
    d.set[0].p = a->real;  d.set[0].sc = a->r_sc;  d.set[0].sp = a->r_sp;  d.set[0].so = a->r_so;  d.set[0].n = a->n;
    d.set[1].p = a->fake;  d.set[1].sc = a->f_sc;  d.set[1].sp = a->f_sp;  d.set[1].so = a->f_so;  d.set[1].n = a->m;
    d.inner = FastDiv::make((unsigned)a->d_inner);
    d.D = a->d_outer * a->d_inner;  d.classes = a->classes;  d.k = a->k;
    float* wf = (float*)a->ws;
    d.rho[0] = wf;  d.rho[1] = wf + cn;
    d.flags = (int*)(wf + cn + cm);  d.hits = d.flags + cn;
    d.rho_out[0] = a->radii_real;  d.rho_out[1] = a->radii_fake;
    d.nrt[0] = kg_cdiv(a->n, p.ti_radii);  d.nrt[1] = kg_cdiv(a->m, p.ti_radii);
    d.nti = kg_cdiv(a->n, p.ti_cross);  d.ntj = kg_cdiv(a->m, p.ti_cross);
    hipStream_t s = (hipStream_t)stream;

    if (p.ti_radii == 32) prdc_launch_radii<32, 2>(d, p.grid_radii, s);
    else prdc_launch_radii<64, 4>(d, p.grid_radii, s);
    if (int rc = kg_launch_status("kg_prdc_radii")) return rc;
    if (p.ti_cross == 32) prdc_launch_cross<32, 2>(d, p.grid_cross, s);
    else prdc_launch_cross<64, 4>(d, p.grid_cross, s);
    if (int rc = kg_launch_status("kg_prdc_cross")) return rc;

    return prdc_finish(d, a->fake_hits, a->real_flags, a->counts, a->values, a->mean, s, "kg_prdc_finish");
}

// ---- one set's radii alone; several fake sets against one real set with given radii ------------------------

namespace {

// The rule of prdc_plan with the workgroups these launches really have: row tiles of the nsets fake sets (radii), tiles of
// nsets x classes x (n x m) (cross).
PrdcPlan prdc_sets_plan(const KgPrdcSetsArgs* a) { return prdc_plan((long)a->nsets * a->classes, 0, a->n, a->m); }

int prdc_sets_validate(const KgPrdcSetsArgs* a, const char* who) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->nsets >= 1 && a->nsets <= KG_PRDC_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, a->nsets, KG_PRDC_MAX_SETS);
    if (int rc = prdc_check_shape(who, a->n, &a->m, a->classes, a->d_outer, a->d_inner, a->k)) return rc;
    const PrdcPlan p = prdc_sets_plan(a);
    KG_REQUIRE(p.grid_radii < PR_MAX_GRID && p.grid_cross < PR_MAX_GRID,
               "%s: nsets=%d x classes=%d x tiles of n=%d x m=%d make %ld workgroups, one launch takes fewer than %ld", who, a->nsets,
               a->classes, a->n, a->m, p.grid_cross > p.grid_radii ? p.grid_cross : p.grid_radii, PR_MAX_GRID);
    return 0;
}

int64_t prdc_sets_ws_bytes(const KgPrdcSetsArgs* a) {
    return 4 * (int64_t)a->nsets * a->classes * (2 * (int64_t)a->m + a->n);
}

}  // namespace

extern "C" int kg_prdc_radii(const KgPrdcRadiiArgs* a, void* stream) {
    const char* who = "kg_prdc_radii";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    if (int rc = prdc_check_shape(who, a->n, nullptr, a->classes, a->d_outer, a->d_inner, a->k)) return rc;
    const int ti = prdc_edge((long)a->classes * kg_cdiv(a->n, 64));
    const long grid = (long)a->classes * kg_cdiv(a->n, ti);
    KG_REQUIRE(grid < PR_MAX_GRID, "%s: classes=%d x row tiles of n=%d make %ld workgroups, one launch takes fewer than %ld", who,
               a->classes, a->n, grid, PR_MAX_GRID);
    KG_REQUIRE(a->x != nullptr, "%s: null pointer x", who);
    KG_REQUIRE(a->radii != nullptr, "%s: null pointer radii", who);

    PrdcDev d = {};             // the set takes the real side's place; no fake rows, no flag / hit words
    d.set[0].p = a->x;  d.set[0].sc = a->sc;  d.set[0].sp = a->sp;  d.set[0].so = a->so;  d.set[0].n = a->n;
    d.inner = FastDiv::make((unsigned)a->d_inner);
    d.D = a->d_outer * a->d_inner;  d.classes = a->classes;  d.k = a->k;  d.nsets = 1;
    d.rho[0] = a->radii;
    d.nrt[0] = kg_cdiv(a->n, ti);  d.nrt[1] = 0;
    if (ti == 32) prdc_launch_radii<32, 2>(d, grid, (hipStream_t)stream);
    else prdc_launch_radii<64, 4>(d, grid, (hipStream_t)stream);
    return kg_launch_status("kg_prdc_radii");
}

extern "C" int64_t kg_prdc_sets_workspace_bytes(const KgPrdcSetsArgs* a) {
    if (int rc = prdc_sets_validate(a, "kg_prdc_sets_workspace_bytes")) return rc;
    return prdc_sets_ws_bytes(a);
}

extern "C" int kg_prdc_sets(const KgPrdcSetsArgs* a, void* stream) {
    if (int rc = prdc_sets_validate(a, "kg_prdc_sets")) return rc;
    KG_REQUIRE(a->real != nullptr, "kg_prdc_sets: null pointer real");
    for (int g = 0; g < a->nsets; ++g) KG_REQUIRE(a->fake[g] != nullptr, "kg_prdc_sets: null pointer fake[%d]", g);
    KG_REQUIRE(a->radii_real != nullptr, "kg_prdc_sets: null pointer radii_real");
    KG_REQUIRE(a->counts != nullptr, "kg_prdc_sets: null pointer counts");
    KG_REQUIRE(a->values != nullptr, "kg_prdc_sets: null pointer values");
    KG_REQUIRE(a->ws != nullptr, "kg_prdc_sets: null pointer ws");
    const int64_t need = prdc_sets_ws_bytes(a);
    KG_REQUIRE(a->ws_bytes >= need, "kg_prdc_sets: ws_bytes=%lld < %lld (kg_prdc_sets_workspace_bytes)", (long long)a->ws_bytes,
               (long long)need);
    const PrdcPlan p = prdc_sets_plan(a);
    const long gcm = (long)a->nsets * a->classes * a->m;

    PrdcDev d = {};
    d.set[0].p = a->real;  d.set[0].sc = a->r_sc;  d.set[0].sp = a->r_sp;  d.set[0].so = a->r_so;  d.set[0].n = a->n;
    d.set[1].p = a->fake[0];  d.set[1].sc = a->f_sc;  d.set[1].sp = a->f_sp;  d.set[1].so = a->f_so;  d.set[1].n = a->m;
    d.nsets = a->nsets;
    for (int g = 0; g < a->nsets; ++g) d.fp[g] = a->fake[g];
    d.inner = FastDiv::make((unsigned)a->d_inner);
    d.D = a->d_outer * a->d_inner;  d.classes = a->classes;  d.k = a->k;
    float* wf = (float*)a->ws;  // fake radii (nsets, classes, m) | hit words (nsets, classes, m) | flag words (nsets, classes, n)
    d.rho[0] = const_cast<float*>(a->radii_real);   // read only: no real row takes part in the radii launch
    d.rho[1] = wf;
    d.hits = (int*)(wf + gcm);  d.flags = d.hits + gcm;
    d.rho_out[0] = nullptr;  d.rho_out[1] = a->radii_fake;
    d.nrt[0] = 0;  d.nrt[1] = kg_cdiv(a->m, p.ti_radii);
    d.nti = kg_cdiv(a->n, p.ti_cross);  d.ntj = kg_cdiv(a->m, p.ti_cross);
    hipStream_t s = (hipStream_t)stream;

    if (p.ti_radii == 32) prdc_launch_radii<32, 2>(d, p.grid_radii, s);
    else prdc_launch_radii<64, 4>(d, p.grid_radii, s);
    if (int rc = kg_launch_status("kg_prdc_sets_radii")) return rc;
    if (p.ti_cross == 32) prdc_launch_cross<32, 2>(d, p.grid_cross, s);
    else prdc_launch_cross<64, 4>(d, p.grid_cross, s);
    if (int rc = kg_launch_status("kg_prdc_sets_cross")) return rc;

    return prdc_finish(d, a->fake_hits, a->real_flags, a->counts, a->values, a->mean, s, "kg_prdc_sets_finish");
}
