// MMD evaluation (evaluation/mmd-actions.py:79-115): kernel two-sample statistics of many point-set groups and many
// bandwidths in one launch + one single-workgroup finishing launch (see include/kgan_hip.h).
//
// kg_mmd_tile_kernel: one workgroup = one TI x TI tile of the (i, j) pair space of one group.  The dimension is walked in
// chunks of KC staged in LDS (four slabs: X rows, Y rows, X columns, Y columns, read through arbitrary strides); every
// thread keeps the three squared distances |x_i - x_j|^2, |y_i - y_j|^2, |x_i - y_j|^2 of its MI x MI pairs in registers
// (direct differences on the VALU: no |a|^2 + |b|^2 - 2ab cancellation).  The epilogue evaluates every bandwidth from
// those registers - exp(-d / bw) as exp2(-d * (log2(e) / bw)), one multiply and one v_exp_f32 - and reduces the fp32
// pair sum of the tile in a fixed order into ws[(g * nbw + b) * ntiles + tile].  No Gram matrix is written.
// Two regimes share the kernel: tiny groups (the reference protocol, m = 16 / 25: a single 16 x 16 or 32 x 32 tile covers
// the group, so one workgroup per group) and large sample sets (m in the thousands: 32 x 32 or 64 x 64 tiles).
// kg_mmd_finish_kernel: one workgroup of 1024 threads combines the tile partials in fp64 (fixed order), divides by
// m (m - 1), averages sqrt(MMD^2) over the groups of a class, takes the reference's per-class maximum and the class mean.
// Deterministic: no atomics; every sum has an order fixed by the shape alone.
#include <float.h>
#include <math.h>

#include "kg_common.h"

namespace {

constexpr int MMD_NT = 256;     // threads of a tile workgroup
constexpr int MMD_KC = 16;      // dimensions staged per chunk
constexpr int MMD_FIN = 1024;   // threads of the finishing workgroup

struct MmdDev {
    const float* x;  long x_sp, x_sd, x_sg, x_sc;
    const float* y;  long y_sp, y_sd, y_sg, y_sc;
    int m, dim, groups, nbw, nti, ntiles;
    float c[KG_MMD_MAX_BW];     // log2(e) / bw
    float* ws;
};

struct MmdFin {
    const float* ws;
    float *mmd2, *mmd, *result, *mean;
    int G, groups, classes, nbw, ntiles;
    double pairs;               // m (m - 1)
};

// stage KC dimensions of TI points (rows p0.. of base) into s[k][p]; zeros outside the group / dimension
template <int TI>
__device__ __forceinline__ void mmd_stage(float (*s)[TI], const float* base, long sp, long sd, int p0, int m, int k0, int kn) {
    const bool kfast = sd < sp;         // walk the smaller stride across neighbouring lanes
    for (int e = threadIdx.x; e < MMD_KC * TI; e += MMD_NT) {
        int k, p;
        if (kfast) { k = e % MMD_KC; p = e / MMD_KC; } else { p = e % TI; k = e / TI; }
        const int pi = p0 + p;
        s[k][p] = (k < kn && pi < m) ? base[(long)pi * sp + (long)(k0 + k) * sd] : 0.f;
    }
}

template <int TI, int MI>
__global__ __launch_bounds__(MMD_NT) void kg_mmd_tile_kernel(MmdDev a) {
    constexpr int NT = TI / MI;
    static_assert(NT * NT == MMD_NT, "tile / micro-tile mismatch");
    __shared__ float sxi[MMD_KC][TI], syi[MMD_KC][TI], sxj[MMD_KC][TI], syj[MMD_KC][TI];
    __shared__ float red[MMD_NT / 64][KG_MMD_MAX_BW];

    const unsigned blk = blockIdx.x;
    const unsigned tile = blk % (unsigned)a.ntiles, g = blk / (unsigned)a.ntiles;
    const int i0 = (int)(tile / (unsigned)a.nti) * TI, j0 = (int)(tile % (unsigned)a.nti) * TI;
    const long cls = g / (unsigned)a.groups, f = g % (unsigned)a.groups;
    const float* xb = a.x + cls * a.x_sc + f * a.x_sg;
    const float* yb = a.y + cls * a.y_sc + f * a.y_sg;
    const int ri = threadIdx.x / NT, rj = threadIdx.x % NT;

    float dxx[MI][MI], dyy[MI][MI], dxy[MI][MI];
#pragma unroll
    for (int r = 0; r < MI; ++r)
#pragma unroll
        for (int s = 0; s < MI; ++s) dxx[r][s] = dyy[r][s] = dxy[r][s] = 0.f;

    auto step = [&](int k) {
        float xi[MI], yi[MI], xj[MI], yj[MI];
#pragma unroll
        for (int r = 0; r < MI; ++r) {
            xi[r] = sxi[k][ri * MI + r];
            yi[r] = syi[k][ri * MI + r];
            xj[r] = sxj[k][rj * MI + r];
            yj[r] = syj[k][rj * MI + r];
        }
#pragma unroll
        for (int r = 0; r < MI; ++r)
#pragma unroll
            for (int s = 0; s < MI; ++s) {
                float d = xi[r] - xj[s];
                dxx[r][s] = fmaf(d, d, dxx[r][s]);
                d = yi[r] - yj[s];
                dyy[r][s] = fmaf(d, d, dyy[r][s]);
                d = xi[r] - yj[s];
                dxy[r][s] = fmaf(d, d, dxy[r][s]);
            }
    };

    for (int k0 = 0; k0 < a.dim; k0 += MMD_KC) {
        const int kn = min(MMD_KC, a.dim - k0);
        mmd_stage<TI>(sxi, xb, a.x_sp, a.x_sd, i0, a.m, k0, kn);
        mmd_stage<TI>(syi, yb, a.y_sp, a.y_sd, i0, a.m, k0, kn);
        mmd_stage<TI>(sxj, xb, a.x_sp, a.x_sd, j0, a.m, k0, kn);
        mmd_stage<TI>(syj, yb, a.y_sp, a.y_sd, j0, a.m, k0, kn);
        __syncthreads();
        if (kn == MMD_KC) {
#pragma unroll
            for (int k = 0; k < MMD_KC; ++k) step(k);
        } else {
            for (int k = 0; k < kn; ++k) step(k);
        }
        __syncthreads();
    }

    // pairs outside the group and the diagonal get distance +inf: exp2(-inf) = 0 for all three kernel values, h = 0
    float dmin = FLT_MAX;
#pragma unroll
    for (int r = 0; r < MI; ++r)
#pragma unroll
        for (int s = 0; s < MI; ++s) {
            const int i = i0 + ri * MI + r, j = j0 + rj * MI + s;
            if (i >= a.m || j >= a.m || i == j) dxx[r][s] = dyy[r][s] = dxy[r][s] = INFINITY;
            dmin = fminf(dmin, fminf(dxx[r][s], fminf(dyy[r][s], dxy[r][s])));
        }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int b = 0; b < KG_MMD_MAX_BW; ++b) {
        if (b < a.nbw) {
            const float cb = a.c[b];
            float acc = 0.f;
            // a bandwidth under which every kernel value of the wave underflows (2^-160 is 0 in fp32, denormals included)
            // contributes exactly 0: skipped by a wave-uniform test, the sum is the same bits either way
            if (!__all(dmin * cb > 160.f)) {
#pragma unroll
                for (int r = 0; r < MI; ++r)
#pragma unroll
                    for (int s = 0; s < MI; ++s) {
                        const float kxx = exp2f(-dxx[r][s] * cb), kyy = exp2f(-dyy[r][s] * cb), kxy = exp2f(-dxy[r][s] * cb);
                        acc += (kxx + kyy) - 2.f * kxy;
                    }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
            if (lane == 0) red[wave][b] = acc;
        }
    }
    __syncthreads();
    if (threadIdx.x < a.nbw) {
        const int b = threadIdx.x;
        a.ws[((long)g * a.nbw + b) * a.ntiles + tile] = (red[0][b] + red[1][b]) + (red[2][b] + red[3][b]);
    }
}

__device__ __forceinline__ double mmd_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(MMD_FIN) void kg_mmd_finish_kernel(MmdFin a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = MMD_FIN / 64;
    // 1. MMD^2 per (group, bandwidth): the tile partials of the item, summed in fp64
    const long items = (long)a.G * a.nbw;
    if (a.ntiles >= 32) {
        for (long it = wave; it < items; it += NW) {
            double s = 0.0;
            for (int t = lane; t < a.ntiles; t += 64) s += (double)a.ws[it * a.ntiles + t];
            s = mmd_wave_sum(s);
            if (lane == 0) a.mmd2[it] = (float)(s / a.pairs);
        }
    } else {
        for (long it = tid; it < items; it += MMD_FIN) {
            double s = 0.0;
            for (int t = 0; t < a.ntiles; ++t) s += (double)a.ws[it * a.ntiles + t];
            a.mmd2[it] = (float)(s / a.pairs);
        }
    }
    __syncthreads();
    // 2. per (class, bandwidth): the mean over the class's groups of sqrt(MMD^2) (NaN for a negative MMD^2, as torch)
    const int citems = a.classes * a.nbw;
    if (a.groups >= 64) {
        for (int it = wave; it < citems; it += NW) {
            const int c = it / a.nbw, b = it % a.nbw;
            double s = 0.0;
            for (int f = lane; f < a.groups; f += 64) s += sqrt((double)a.mmd2[((long)c * a.groups + f) * a.nbw + b]);
            s = mmd_wave_sum(s);
            if (lane == 0) a.mmd[it] = (float)(s / a.groups);
        }
    } else {
        for (int it = tid; it < citems; it += MMD_FIN) {
            const int c = it / a.nbw, b = it % a.nbw;
            double s = 0.0;
            for (int f = 0; f < a.groups; ++f) s += sqrt((double)a.mmd2[((long)c * a.groups + f) * a.nbw + b]);
            a.mmd[it] = (float)(s / a.groups);
        }
    }
    __syncthreads();
    // 3. per class: r = 0, replaced on a strict '>' in bandwidth order (mmd-actions.py:107-110: NaN never wins)
    for (int c = tid; c < a.classes; c += MMD_FIN) {
        float r = 0.f;
        for (int b = 0; b < a.nbw; ++b) {
            const float v = a.mmd[c * a.nbw + b];
            if (v > r) r = v;
        }
        a.result[c] = r;
    }
    if (a.mean == nullptr) return;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int c = 0; c < a.classes; ++c) s += (double)a.result[c];
        *a.mean = (float)(s / a.classes);
    }
}

struct MmdPlan {
    int ti;         // tile edge: 16, 32 or 64
    int nti;        // tiles along i (= along j)
    long ntiles;
};

// tile edge: the smallest of 16 / 32 that covers a tiny group; for large groups the 64 x 64 tile (4 x 4 pairs per thread)
// once the launch has enough workgroups to fill the chip twice, else 32 x 32
MmdPlan mmd_plan(const KgMmdArgs* a) {
    MmdPlan p;
    const long G = (long)a->groups * a->classes;
    if (a->m <= 16) p.ti = 16;
    else if (a->m <= 32) p.ti = 32;
    else {
        const long n64 = (long)kg_cdiv(a->m, 64);
        p.ti = G * n64 * n64 >= 512 ? 64 : 32;
    }
    p.nti = kg_cdiv(a->m, p.ti);
    p.ntiles = (long)p.nti * p.nti;
    return p;
}

int mmd_validate(const KgMmdArgs* a, const char* who) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->m == a->n, "%s: m=%d != n=%d (both sets need the same number of points)", who, a->m, a->n);
    KG_REQUIRE(a->m >= 1, "%s: m=%d < 1", who, a->m);
    KG_REQUIRE(a->dim >= 1, "%s: dim=%d < 1", who, a->dim);
    KG_REQUIRE(a->groups >= 1 && a->classes >= 1, "%s: groups=%d / classes=%d < 1", who, a->groups, a->classes);
    KG_REQUIRE(a->nbw >= 1 && a->nbw <= KG_MMD_MAX_BW, "%s: nbw=%d outside [1, %d]", who, a->nbw, KG_MMD_MAX_BW);
    for (int b = 0; b < a->nbw; ++b)
        KG_REQUIRE(a->bw[b] > 0.0 && isfinite(a->bw[b]), "%s: bw[%d]=%g is not a positive bandwidth", who, b, a->bw[b]);
    const MmdPlan p = mmd_plan(a);
    KG_REQUIRE((long)a->groups * a->classes * a->nbw * p.ntiles <= 0x7fffffffL, "%s: groups x classes x nbw x tiles too large",
               who);
    return 0;
}

}  // namespace

extern "C" int64_t kg_mmd_workspace_bytes(const KgMmdArgs* a) {
    if (int rc = mmd_validate(a, "kg_mmd_workspace_bytes")) return rc;
    return (int64_t)a->groups * a->classes * a->nbw * mmd_plan(a).ntiles * 4;
}

extern "C" int kg_mmd(const KgMmdArgs* a, void* stream) {
    if (int rc = mmd_validate(a, "kg_mmd")) return rc;
    KG_REQUIRE(a->x != nullptr, "kg_mmd: null pointer x");
    KG_REQUIRE(a->y != nullptr, "kg_mmd: null pointer y");
    KG_REQUIRE(a->mmd2 != nullptr, "kg_mmd: null pointer mmd2");
    KG_REQUIRE(a->mmd != nullptr, "kg_mmd: null pointer mmd");
    KG_REQUIRE(a->result != nullptr, "kg_mmd: null pointer result");
    KG_REQUIRE(a->ws != nullptr, "kg_mmd: null pointer ws");
    const MmdPlan p = mmd_plan(a);
    const long G = (long)a->groups * a->classes;
    const int64_t need = G * a->nbw * p.ntiles * 4;
    KG_REQUIRE(a->ws_bytes >= need, "kg_mmd: ws_bytes=%lld < %lld (kg_mmd_workspace_bytes)", (long long)a->ws_bytes,
               (long long)need);

    MmdDev d;
    d.x = a->x;  d.x_sp = a->x_sp;  d.x_sd = a->x_sd;  d.x_sg = a->x_sg;  d.x_sc = a->x_sc;
    d.y = a->y;  d.y_sp = a->y_sp;  d.y_sd = a->y_sd;  d.y_sg = a->y_sg;  d.y_sc = a->y_sc;
    d.m = a->m;  d.dim = a->dim;  d.groups = a->groups;  d.nbw = a->nbw;  d.nti = p.nti;  d.ntiles = (int)p.ntiles;
    for (int b = 0; b < KG_MMD_MAX_BW; ++b) d.c[b] = b < a->nbw ? (float)(M_LOG2E / a->bw[b]) : 0.f;
    d.ws = (float*)a->ws;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(G * p.ntiles));
    if (p.ti == 16) hipLaunchKernelGGL((kg_mmd_tile_kernel<16, 1>), grid, dim3(MMD_NT), 0, s, d);
    else if (p.ti == 32) hipLaunchKernelGGL((kg_mmd_tile_kernel<32, 2>), grid, dim3(MMD_NT), 0, s, d);
    else hipLaunchKernelGGL((kg_mmd_tile_kernel<64, 4>), grid, dim3(MMD_NT), 0, s, d);
    if (int rc = kg_launch_status("kg_mmd_tile")) return rc;

    MmdFin fin;
    fin.ws = (const float*)a->ws;
    fin.mmd2 = a->mmd2;  fin.mmd = a->mmd;  fin.result = a->result;  fin.mean = a->mean;
    fin.G = (int)G;  fin.groups = a->groups;  fin.classes = a->classes;  fin.nbw = a->nbw;  fin.ntiles = (int)p.ntiles;
    fin.pairs = (double)a->m * (double)(a->m - 1);
    hipLaunchKernelGGL(kg_mmd_finish_kernel, dim3(1), dim3(MMD_FIN), 0, s, fin);
    return kg_launch_status("kg_mmd_finish");
}
