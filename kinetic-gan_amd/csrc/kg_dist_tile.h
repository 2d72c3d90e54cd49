// The squared-distance tile shared by kg_prdc.hip and kg_nn.hip: DT_KC dimensions of TI row points and
// TI column points staged in LDS, MI x MI pairs per thread of a 16 x 16 thread grid, direct differences on the VALU, one
// fmaf chain per pair in dimension order - no |a|^2 + |b|^2 - 2ab.  The bits of a pair depend on the two points alone:
// not on the tile edge, not on where the tile starts, not on which kernel asks.
// A point set is read through class / point / outer strides with a contiguous inner run (DistSet); the load goes through a
// transform hook (DistIdentity: the value as stored), which is applied to elements of the set only - the staged zeros outside
// the set or the dimension stay zero.
#pragma once
#include "kg_common.h"

namespace {

constexpr int DT_NT = 256;      // threads of a tile workgroup: 16 x 16 micro-tiles
constexpr int DT_KC = 32;       // dimensions staged per chunk
constexpr int DT_PAD = 4;       // floats of padding per staged row: rows stay 16-byte aligned, row stride = 4 banks mod 32

struct DistSet {
    const float* p;
    long sc, sp, so;
    int n;
};

struct DistIdentity {
    __device__ __forceinline__ float operator()(float x) const { return x; }
};

// which point of the set stands at position p of a tile's side: p itself, or an entry of a caller's list (kg_nn_search.h)
struct DistRowsIdentity {
    __device__ __forceinline__ int operator()(int p) const { return p; }
};

// Stage DT_KC dimensions of TI points (points rows(p0 ..) of base) into s[k][p]; zeros outside the set / dimension (n bounds
// the POSITIONS p0 ..: rows is only asked for positions below it).
// Lane bits of the element index e: [0,3) -> k low, [3,5) -> p low, [5,7) -> k high, [7,..) -> p high: a wave reads 64
// contiguous bytes of each of 4 points, and the 32 lanes of a half wave write 32 different LDS banks
// (bank = 4 k + p mod 32 with the padded row).
template <int TI, class Load, class Rows = DistRowsIdentity>
__device__ __forceinline__ void dist_stage(float (*s)[TI + DT_PAD], const float* base, long sp, long so, const FastDiv& inner,
                                           int p0, int n, int k0, int kn, const Load& load, const Rows& rows = Rows()) {
    static_assert(DT_NT == 256, "the k bits of the element index must lie below the loop stride");
    // e advances by DT_NT = 2^8 and k is made of bits [0,3) and [5,7) of e: a thread stages ONE dimension of several points
    const int k = (threadIdx.x & 7) | ((threadIdx.x >> 2) & 24);
    const bool kin = k < kn;
    unsigned o = 0, r = 0;
    if (kin) inner.divmod((unsigned)(k0 + k), o, r);
    const float* col = base + ((long)o * so + r);
    for (int e = threadIdx.x; e < DT_KC * TI; e += DT_NT) {
        const int p = ((e >> 3) & 3) | ((e >> 5) & ~3);
        const int pi = p0 + p;
        s[k][p] = (kin && pi < n) ? load(col[(long)rows(pi) * sp]) : 0.f;
    }
}

// acc[r][s] += (x_{i0 + ri MI + r}[d] - y_{j0 + rj MI + s}[d])^2 over all D dimensions, d ascending; X.n / Y.n bound the
// points that are read (a caller that owns a column chunk passes the chunk's end); xrows: the row side's list, if it has one
template <int TI, int MI, class LoadX, class LoadY, class RowsX = DistRowsIdentity>
__device__ __forceinline__ void dist_tile(float (&acc)[MI][MI], float (*si)[TI + DT_PAD], float (*sj)[TI + DT_PAD], int D,
                                          const FastDiv& inner, const DistSet& X, const float* xb, int i0, const DistSet& Y,
                                          const float* yb, int j0, bool live, const LoadX& lx, const LoadY& ly,
                                          const RowsX& xrows = RowsX()) {
    const int ri = threadIdx.x >> 4, rj = threadIdx.x & 15;
#pragma unroll
    for (int r = 0; r < MI; ++r)
#pragma unroll
        for (int s = 0; s < MI; ++s) acc[r][s] = 0.f;

    auto step = [&](int k) {
        float xi[MI], yj[MI];
#pragma unroll
        for (int r = 0; r < MI; ++r) {
            xi[r] = si[k][ri * MI + r];
            yj[r] = sj[k][rj * MI + r];
        }
#pragma unroll
        for (int r = 0; r < MI; ++r)
#pragma unroll
            for (int s = 0; s < MI; ++s) {
                const float d = xi[r] - yj[s];
                acc[r][s] = fmaf(d, d, acc[r][s]);
            }
    };

    for (int k0 = 0; k0 < D; k0 += DT_KC) {
        const int kn = min(DT_KC, D - k0);
        dist_stage<TI>(si, xb, X.sp, X.so, inner, i0, X.n, k0, kn, lx, xrows);
        dist_stage<TI>(sj, yb, Y.sp, Y.so, inner, j0, Y.n, k0, kn, ly);
        __syncthreads();
        if (live) {     // (wave-uniform: a wave whose rows all lie outside the set only helps staging)
            if (kn == DT_KC) {
#pragma unroll
                for (int k = 0; k < DT_KC; ++k) step(k);
            } else {
                for (int k = 0; k < kn; ++k) step(k);
            }
        }
        __syncthreads();
    }
}

}  // namespace
