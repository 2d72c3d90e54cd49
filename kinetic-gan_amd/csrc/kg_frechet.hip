// Frechet distance between the point sets of many classes in fp64 (see include/kgan_hip.h).  Per class: a real
// and a fake set of P_r / P_f points of dimension d = d_outer * d_inner <= 96 - the frames of n / m samples (pose) or the
// differences of consecutive frames (motion), read in place through strides.  Four launches:
//
// kg_frechet_moments_kernel: one workgroup = one chunk of the points of one (class, set).  The points are staged 32 at a
//   time in LDS as doubles, CENTRED on the set's first point (the provisional shift: what is left of the one-pass
//   cancellation is |mu - x_0|^2 against the variance, both of the order of the data's range), and every thread keeps a
//   6 x 6 (d <= 48: 3 x 3) tile of sum (x - x_0)(x - x_0)^T in registers: one v_fma_f64 chain per entry in point order.
//   The chunk's sum and second-moment matrix go to the workspace; nothing is accumulated across workgroups.
// kg_frechet_merge_kernel: one thread per entry of S: the chunks' partials summed in chunk order (the chunking depends on
//   the shape alone: the same bits on every call), S = (M2 - s s^T / P) / (P - 1), mu = x_0 + s / P.
// kg_frechet_solve_kernel: one workgroup of 1024 threads per class.  S_r and its eigenvector matrix live in LDS as doubles
//   (row stride m + 1, m = d rounded up to even: 2 x 96 x 97 x 8 = 148,992 bytes at d = 96).  Cyclic Jacobi with the
//   round-robin parallel ordering: every step computes m / 2 disjoint rotations (phase 1) and applies them as independent
//   2 x 2 blocks J_k^T B J_l, upper blocks computed and mirrored so the matrix stays symmetric bit for bit (phase 2): two
//   barriers per step.  Then G = V sqrt(max(l, 0)), W = S_f G (S_f from the workspace) into the place of S_r,
//   H = sym(G^T W) through registers into the same place, the eigenvalues of H by the same iteration without vectors,
//   T = sum sqrt(max(e, 0)), and the four terms and FD of the class.
// kg_frechet_mean_kernel: the class mean (fp64 sum in class order).
// No atomics, no ticket, no scratch, no dynamically indexed private array; every launch on the caller's stream.
//
// The Evaluator's split: the real set of a run never changes, so kg_frechet_real runs the moments and merge
// launch on the real set alone (the chunking kg_frechet gives it) and kg_frechet_real_solve_kernel, and keeps mu_r, tr S_r,
// G and the sweeps; kg_frechet_sets runs the moments and merge launch on up to KG_FRECHET_MAX_SETS fake sets (the chunking
// kg_frechet gives a fake set), kg_frechet_sets_solve_kernel - one workgroup per (set, class), G read from the cache into the
// place where kg_frechet_solve_kernel forms it - and kg_frechet_sets_finish_kernel.  The solve is written once, as two
// device functions: fr_real_half (S_r -> V, sqrt(l)) and fr_fake_half (G, S_f -> the terms).  kg_frechet_solve_kernel calls
// both, the real kernel the first, the sets kernel the second: shared code, not mirrored code.  The moments and merge kernels
// walk a list of sets; every sum keeps its order, so each output is, bit for bit, that of kg_frechet(real, fake[g]).
#include <math.h>

#include "kg_common.h"

namespace {

constexpr int FR_MAXD = KG_FRECHET_MAX_DIM;
constexpr int FR_NT = 256;          // threads of a moments / merge workgroup: 16 x 16 register tiles
constexpr int FR_KB = 32;           // points staged per batch
constexpr int FR_MINCHUNK = 64;     // points of the smallest chunk
constexpr int FR_TARGET = 1024;     // workgroups the moments launch aims at (4 of them fit a CU)
constexpr int FR_SOLVE_NT = 1024;   // threads of the solving workgroup
constexpr int FR_MAXSWEEPS = 40;
constexpr long FR_MAX_POINTS = 1L << 24;
constexpr long FR_MAX_GRID = 1L << 24;  // workgroups of one launch (exclusive): grid x 256 threads stays below 2^32
constexpr int FR_MAXPAIRS = FR_MAXD / 2;
constexpr int FR_MAXSETS = KG_FRECHET_MAX_SETS;     // sets of one moments / merge launch (kg_frechet: real, fake)
static_assert(FR_MAXSETS >= 2, "kg_frechet's launches hold the real and the fake set");
constexpr int FR_HREG = FR_MAXD * FR_MAXD / FR_SOLVE_NT;    // entries of H a thread carries through the barrier
static_assert(FR_MAXD % 16 == 0 && FR_MAXD % 2 == 0 && FR_HREG * FR_SOLVE_NT == FR_MAXD * FR_MAXD, "tile plan");

struct FrSet {
    const float* p;
    long sc, ss, sf, so;        // class, sample, frame, outer strides (elements); the inner run is contiguous
    int P;                      // points per class
    int cs, nch;                // points per chunk (a multiple of FR_KB), chunks
    int ch0;                    // chunks of the sets in front of this one
};

struct FrDev {
    FrSet set[FR_MAXSETS];      // kg_frechet: 0 = real, 1 = fake; kg_frechet_real: the real set; kg_frechet_sets: the fake sets
    int nset, per;              // sets in use, chunks of all of them (of one class)
    FastDiv inner, fr;          // j = o * d_inner + e;  point p = sample * fr + frame
    int d, diff, classes;
    double* part;               // ws: (classes, per, d + d*d)
    double* mu;                 // ws: (classes, nset, d)
    double* cov;                // ws: (classes, nset, d, d)
    double* mu_out[FR_MAXSETS]; // the caller's arrays or null
    double* cov_out[FR_MAXSETS];
    double* values;  double* terms;  int32_t* sweeps;
};

// coordinate j of point (sample i, frame f) of a class, formed in fp64 (the motion difference is exact there)
__device__ __forceinline__ double fr_coord(const float* base, const FrSet& X, int diff, long i, long f, unsigned o, unsigned e) {
    const float* q = base + (i * X.ss + f * X.sf + (long)o * X.so + e);
    return diff ? (double)q[X.sf] - (double)q[0] : (double)q[0];
}

template <int NR>
__global__ __launch_bounds__(FR_NT) void kg_frechet_moments_kernel(FrDev a) {
    constexpr int W = NR * 16;                      // columns a workgroup covers (d <= W)
    __shared__ double pts[FR_KB][W];
    __shared__ double shift[W];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const unsigned per = (unsigned)a.per;
    const unsigned cls = blockIdx.x / per, t = blockIdx.x % per;
    int set = 0;
    while (set + 1 < a.nset && t >= (unsigned)a.set[set + 1].ch0) ++set;
    const FrSet X = a.set[set];
    const int chunk = (int)t - X.ch0;
    const float* base = X.p + (long)cls * X.sc;
    const int d = a.d;

    for (int e = tid; e < FR_KB * W; e += FR_NT) pts[e / W][e % W] = 0.0;      // columns >= d stay zero
    if (tid < W) {
        double s = 0.0;
        if (tid < d) {
            unsigned o, r;
            a.inner.divmod((unsigned)tid, o, r);
            s = fr_coord(base, X, a.diff, 0, 0, o, r);
        }
        shift[tid] = s;
    }
    __syncthreads();

    double acc[NR][NR];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int s = 0; s < NR; ++s) acc[r][s] = 0.0;
    double sum = 0.0;

    const int pbeg = chunk * X.cs, pend = min(X.P, pbeg + X.cs);
    for (int p0 = pbeg; p0 < pend; p0 += FR_KB) {
        // element e = (o, k, inner): a wave reads runs of d_inner floats of consecutive frames
        for (int e = tid; e < FR_KB * d; e += FR_NT) {
            unsigned q, v;
            a.inner.divmod((unsigned)e, q, v);
            const int k = (int)(q & (FR_KB - 1));
            const unsigned o = q / FR_KB;
            const int j = (int)(o * a.inner.d + v);
            const int p = p0 + k;
            double x = 0.0;
            if (p < pend) {
                unsigned i, f;
                a.fr.divmod((unsigned)p, i, f);
                x = fr_coord(base, X, a.diff, i, f, o, v) - shift[j];
            }
            pts[k][j] = x;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < FR_KB; ++k) {
            double xi[NR], yj[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                xi[r] = pts[k][r * 16 + ti];
                yj[r] = pts[k][r * 16 + tj];
            }
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int s = 0; s < NR; ++s) acc[r][s] = fma(xi[r], yj[s], acc[r][s]);
        }
        if (tid < W) {
            for (int k = 0; k < FR_KB; ++k) sum += pts[k][tid];
        }
        __syncthreads();
    }

    double* part = a.part + ((long)cls * per + t) * ((long)d + (long)d * d);
    if (tid < d) part[tid] = sum;
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int s = 0; s < NR; ++s) {
            const int ra = r * 16 + ti, cb = s * 16 + tj;
            if (ra < d && cb < d) part[d + ra * d + cb] = acc[r][s];
        }
}

__global__ __launch_bounds__(FR_NT) void kg_frechet_merge_kernel(FrDev a) {
    const int d = a.d, dd = d * d;
    const unsigned nb = (unsigned)((dd + FR_NT - 1) / FR_NT);
    const unsigned cs = blockIdx.x / nb, tile = blockIdx.x % nb;        // cs = class * nset + set
    const unsigned cls = cs / (unsigned)a.nset;
    const int set = (int)(cs % (unsigned)a.nset);
    const int entry = (int)tile * FR_NT + (int)threadIdx.x;
    if (entry >= dd) return;
    const int ra = entry / d, cb = entry % d;
    const FrSet X = a.set[set];
    const long per = a.per, stride = (long)d + dd;
    const double* part = a.part + ((long)cls * per + X.ch0) * stride;
    double m2 = 0.0, sa = 0.0, sb = 0.0;
    for (int c = 0; c < X.nch; ++c) {
        const double* q = part + (long)c * stride;
        m2 += q[d + entry];
        sa += q[ra];
        sb += q[cb];
    }
    const double P = (double)X.P;
    const double cov = (m2 - (sa * sb) / P) / (P - 1.0);
    a.cov[(long)cs * dd + entry] = cov;
    if (a.cov_out[set] != nullptr) a.cov_out[set][(long)cls * dd + entry] = cov;
    if (cb == 0) {
        unsigned o, r;
        a.inner.divmod((unsigned)ra, o, r);
        const double mu = fr_coord(X.p + (long)cls * X.sc, X, a.diff, 0, 0, o, r) + sa / P;
        a.mu[(long)cs * d + ra] = mu;
        if (a.mu_out[set] != nullptr) a.mu_out[set][(long)cls * d + ra] = mu;
    }
}

struct FrSmall {
    double c[FR_MAXPAIRS], s[FR_MAXPAIRS], t[FR_MAXPAIRS];
    int p[FR_MAXPAIRS], q[FR_MAXPAIRS], rot[FR_MAXPAIRS];
    double root[FR_MAXD];       // sqrt(max(l, 0)) of S_r
    double red[FR_SOLVE_NT / 64];
    double thresh;
    int any;
};

// Cyclic Jacobi, round-robin ordering, on the symmetric m x m matrix A (m even, row stride ld) in LDS; V (or null)
// accumulates the rotations.  Returns the sweeps run (the last one applied no rotation unless the cap was met).
__device__ int fr_jacobi(double* A, double* V, int m, int ld, int d, FrSmall& sm) {
    const int tid = threadIdx.x, np = m >> 1;
    {   // |a_pq| <= 2^-52 ||A||_F / d is left alone; the norm is taken once
        double s = 0.0;
        for (int e = tid; e < m * m; e += FR_SOLVE_NT) {
            const double v = A[(e / m) * ld + (e % m)];
            s = fma(v, v, s);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if ((tid & 63) == 0) sm.red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            for (int w = 0; w < FR_SOLVE_NT / 64; ++w) tot += sm.red[w];
            sm.thresh = 0x1p-52 * sqrt(tot) / (double)d;
        }
        __syncthreads();
    }
    const double thresh = sm.thresh;
    int sweeps = 0;
    for (int sweep = 0; sweep < FR_MAXSWEEPS; ++sweep) {
        if (tid == 0) sm.any = 0;
        __syncthreads();
        for (int r = 0; r < m - 1; ++r) {
            // phase 1: the rotations of this step's m / 2 disjoint pairs (circle method: m - 1 stays, the others turn)
            if (tid < np) {
                int p, q;
                if (tid == 0) {
                    p = r;  q = m - 1;
                } else {
                    p = (r + tid) % (m - 1);
                    q = (r - tid + (m - 1)) % (m - 1);
                }
                if (p > q) { const int x = p; p = q; q = x; }
                const double apq = A[p * ld + q];
                double c = 1.0, s = 0.0, t = 0.0;
                const int rot = fabs(apq) > thresh ? 1 : 0;
                if (rot) {
                    const double theta = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
                    t = 1.0 / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
                    if (theta < 0.0) t = -t;
                    c = 1.0 / sqrt(fma(t, t, 1.0));
                    s = t * c;
                    sm.any = 1;
                }
                sm.p[tid] = p;  sm.q[tid] = q;  sm.rot[tid] = rot;
                sm.c[tid] = c;  sm.s[tid] = s;  sm.t[tid] = t;
            }
            __syncthreads();
            // phase 2: A <- J^T A J as independent 2 x 2 blocks (k <= l computed, mirrored), V <- V J
            for (int item = tid; item < np * np; item += FR_SOLVE_NT) {
                const int k = item / np, l = item % np;
                if (k > l || !(sm.rot[k] | sm.rot[l])) continue;
                const int pk = sm.p[k], qk = sm.q[k];
                if (k == l) {
                    const double apq = A[pk * ld + qk], t = sm.t[k];
                    A[pk * ld + pk] -= t * apq;
                    A[qk * ld + qk] += t * apq;
                    A[pk * ld + qk] = 0.0;
                    A[qk * ld + pk] = 0.0;
                    continue;
                }
                const int pl = sm.p[l], ql = sm.q[l];
                const double ck = sm.c[k], sk = sm.s[k], cl = sm.c[l], sl = sm.s[l];
                const double b00 = A[pk * ld + pl], b01 = A[pk * ld + ql], b10 = A[qk * ld + pl], b11 = A[qk * ld + ql];
                const double r00 = ck * b00 - sk * b10, r01 = ck * b01 - sk * b11;      // rows: J_k^T B
                const double r10 = sk * b00 + ck * b10, r11 = sk * b01 + ck * b11;
                const double n00 = cl * r00 - sl * r01, n01 = sl * r00 + cl * r01;      // columns: (.) J_l
                const double n10 = cl * r10 - sl * r11, n11 = sl * r10 + cl * r11;
                A[pk * ld + pl] = n00;  A[pl * ld + pk] = n00;
                A[pk * ld + ql] = n01;  A[ql * ld + pk] = n01;
                A[qk * ld + pl] = n10;  A[pl * ld + qk] = n10;
                A[qk * ld + ql] = n11;  A[ql * ld + qk] = n11;
            }
            if (V != nullptr) {
                for (int item = tid; item < m * np; item += FR_SOLVE_NT) {
                    const int i = item / np, l = item % np;
                    if (!sm.rot[l]) continue;
                    const int pl = sm.p[l], ql = sm.q[l];
                    const double cl = sm.c[l], sl = sm.s[l];
                    const double vp = V[i * ld + pl], vq = V[i * ld + ql];
                    V[i * ld + pl] = cl * vp - sl * vq;
                    V[i * ld + ql] = sl * vp + cl * vq;
                }
            }
            __syncthreads();
        }
        sweeps = sweep + 1;
        const int any = sm.any;
        __syncthreads();
        if (!any) break;
    }
    return sweeps;
}

// The solve of one class in two halves, each written ONCE: kg_frechet_solve_kernel runs both, kg_frechet_real_solve_kernel
// the real half, kg_frechet_sets_solve_kernel the fake half on the G of the cache.  A, V: the two m x m matrices (m = d
// rounded up to even, row stride ld = m + 1) in dynamic LDS.

// Real half: S_r = V diag(l) V^T.  Leaves V and sm.root[] = sqrt(max(l, 0)) behind a barrier and returns the sweeps;
// G = V sqrt(l) is the caller's one loop over V[..] * sm.root[..] - in place, or on the way to global memory.
__device__ __forceinline__ int fr_real_half(const double* __restrict__ Sr, double* A, double* V, int m, int ld, int d, FrSmall& sm) {
    const int tid = threadIdx.x;
    for (int e = tid; e < m * m; e += FR_SOLVE_NT) {
        const int i = e / m, j = e % m;
        A[i * ld + j] = (i < d && j < d) ? Sr[i * d + j] : 0.0;      // (odd d: one idle index, never rotated)
        V[i * ld + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    const int sweeps_r = fr_jacobi(A, V, m, ld, d, sm);

    if (tid < m) sm.root[tid] = sqrt(fmax(A[tid * ld + tid], 0.0));
    __syncthreads();
    return sweeps_r;
}

// Fake half: V holds G (behind a barrier).  W = S_f G into A, H = sym(G^T W) through registers into A, the eigenvalues of
// H, T, and thread 0 stores the four terms and FD at index o and the sweeps of H at sweeps[slot].  tr S_r is summed from
// Sr's diagonal, or - Sr null - read from *trr_given.
__device__ __forceinline__ void fr_fake_half(double* A, double* V, int m, int ld, int d, FrSmall& sm,
                                             const double* __restrict__ mr, const double* __restrict__ mf,
                                             const double* __restrict__ Sf, const double* __restrict__ Sr,
                                             const double* __restrict__ trr_given, double* __restrict__ terms,
                                             double* __restrict__ values, int32_t* __restrict__ sweeps, long o, long slot) {
    const int tid = threadIdx.x;
    for (int e = tid; e < m * m; e += FR_SOLVE_NT) {           // W = S_f G, in the place of S_r
        const int i = e / m, j = e % m;
        double w = 0.0;
        if (i < d) {
            for (int b = 0; b < d; ++b) w = fma(Sf[i * d + b], V[b * ld + j], w);
        }
        A[i * ld + j] = w;
    }
    __syncthreads();
    double h[FR_HREG];                                          // H = sym(G^T W), upper entries, through registers
#pragma unroll
    for (int u = 0; u < FR_HREG; ++u) {
        const int e = tid + u * FR_SOLVE_NT;
        const int i = e / m, j = e % m;
        double x = 0.0, y = 0.0;
        if (e < m * m && i <= j) {
            for (int b = 0; b < m; ++b) {
                x = fma(V[b * ld + i], A[b * ld + j], x);
                y = fma(V[b * ld + j], A[b * ld + i], y);
            }
        }
        h[u] = 0.5 * (x + y);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < FR_HREG; ++u) {
        const int e = tid + u * FR_SOLVE_NT;
        const int i = e / m, j = e % m;
        if (e < m * m && i <= j) {
            A[i * ld + j] = h[u];
            A[j * ld + i] = h[u];
        }
    }
    __syncthreads();
    const int sweeps_h = fr_jacobi(A, nullptr, m, ld, d, sm);

    if (tid == 0) {
        double dmu2 = 0.0, trr = 0.0, trf = 0.0, T = 0.0;
        for (int i = 0; i < d; ++i) {
            const double df = mr[i] - mf[i];
            dmu2 += df * df;
            if (Sr != nullptr) trr += Sr[i * d + i];
            trf += Sf[i * d + i];
        }
        if (Sr == nullptr) trr = *trr_given;
        for (int i = 0; i < m; ++i) T += sqrt(fmax(A[i * ld + i], 0.0));
        terms[o * 4 + 0] = dmu2;
        terms[o * 4 + 1] = trr;
        terms[o * 4 + 2] = trf;
        terms[o * 4 + 3] = T;
        values[o] = ((dmu2 + trr) + trf) - 2.0 * T;
        sweeps[slot] = sweeps_h;
    }
}

__global__ __launch_bounds__(FR_SOLVE_NT) void kg_frechet_solve_kernel(FrDev a) {
    extern __shared__ __attribute__((aligned(16))) double fr_lds[];
    __shared__ FrSmall sm;
    const int tid = threadIdx.x, d = a.d, dd = d * d;
    const int m = d + (d & 1), ld = m + 1;
    double* A = fr_lds;
    double* V = fr_lds + m * ld;
    const unsigned cls = blockIdx.x;
    const double* Sr = a.cov + (long)(cls * 2) * dd;
    const double* mr = a.mu + (long)(cls * 2) * d;

    const int sweeps_r = fr_real_half(Sr, A, V, m, ld, d, sm);
    for (int e = tid; e < m * m; e += FR_SOLVE_NT) V[(e / m) * ld + (e % m)] *= sm.root[e % m];      // G = V sqrt(l)
    __syncthreads();
    if (tid == 0) a.sweeps[cls * 2 + 0] = sweeps_r;
    fr_fake_half(A, V, m, ld, d, sm, mr, mr + d, Sr + dd, Sr, nullptr, a.terms, a.values, a.sweeps, cls, cls * 2 + 1);
}

__global__ void kg_frechet_mean_kernel(const double* values, double* mean, int classes) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int c = 0; c < classes; ++c) s += values[c];
    *mean = s / (double)classes;
}

// ---- the real side alone, and several fake sets against its cache -----------------------------------------

struct FrRealDev {
    const double* cov;          // ws: (classes, d, d), the merge launch's S_r
    int d;
    double* G;                  // (classes, m, m)
    double* tr;                 // (classes)
    int32_t* sweeps;            // (classes)
};

// The real half alone: G = V sqrt(max(l, 0)) - the words kg_frechet_solve_kernel holds in LDS when it enters the fake half -,
// tr S_r in that kernel's order, the sweeps.
__global__ __launch_bounds__(FR_SOLVE_NT) void kg_frechet_real_solve_kernel(FrRealDev a) {
    extern __shared__ __attribute__((aligned(16))) double fr_lds[];
    __shared__ FrSmall sm;
    const int tid = threadIdx.x, d = a.d, dd = d * d;
    const int m = d + (d & 1), ld = m + 1;
    double* A = fr_lds;
    double* V = fr_lds + m * ld;
    const unsigned cls = blockIdx.x;
    const double* Sr = a.cov + (long)cls * dd;

    const int sweeps_r = fr_real_half(Sr, A, V, m, ld, d, sm);
    double* G = a.G + (long)cls * m * m;
    for (int e = tid; e < m * m; e += FR_SOLVE_NT) G[e] = V[(e / m) * ld + (e % m)] * sm.root[e % m];
    if (tid == 0) {
        double trr = 0.0;
        for (int i = 0; i < d; ++i) trr += Sr[i * d + i];
        a.tr[cls] = trr;
        a.sweeps[cls] = sweeps_r;
    }
}

struct FrSetsDev {
    const double* mu;           // ws: (classes, nsets, d)
    const double* cov;          // ws: (classes, nsets, d, d)
    const double* mu_real;      // the cache: (classes, d), (classes), (classes, m, m)
    const double* tr_real;
    const double* G;
    int d, nsets, classes;
    double* values;  double* terms;  int32_t* sweeps;       // (nsets, classes), (nsets, classes, 4), (nsets, classes)
};

// The fake half alone for one (set, class): G from the cache into the place where kg_frechet_solve_kernel forms it.
__global__ __launch_bounds__(FR_SOLVE_NT) void kg_frechet_sets_solve_kernel(FrSetsDev a) {
    extern __shared__ __attribute__((aligned(16))) double fr_lds[];
    __shared__ FrSmall sm;
    const int tid = threadIdx.x, d = a.d, dd = d * d;
    const int m = d + (d & 1), ld = m + 1;
    double* A = fr_lds;
    double* V = fr_lds + m * ld;
    const unsigned g = blockIdx.x / (unsigned)a.classes, cls = blockIdx.x % (unsigned)a.classes;
    const long fs = (long)cls * a.nsets + g, o = (long)g * a.classes + cls;     // in the workspace; in the outputs
    const double* G = a.G + (long)cls * m * m;

    for (int e = tid; e < m * m; e += FR_SOLVE_NT) V[(e / m) * ld + (e % m)] = G[e];
    __syncthreads();
    fr_fake_half(A, V, m, ld, d, sm, a.mu_real + (long)cls * d, a.mu + fs * d, a.cov + fs * dd, nullptr, a.tr_real + cls,
                 a.terms, a.values, a.sweeps, o, o);
}

// per set: the class mean as kg_frechet_mean_kernel forms it, and its fp32 rounding (the word kg_eval_record2 reads)
__global__ void kg_frechet_sets_finish_kernel(const double* values, double* mean, float* mean32, int classes, int nsets) {
    const int g = (int)threadIdx.x;
    if (blockIdx.x != 0 || g >= nsets) return;
    double s = 0.0;
    for (int c = 0; c < classes; ++c) s += values[(long)g * classes + c];
    const double mu = s / (double)classes;
    mean[g] = mu;
    mean32[g] = (float)mu;
}

struct FrPlan {
    long P[2];
    int cs[2], nch[2];
    long grid_moments, grid_merge;
    int64_t part_doubles, ws_bytes;
    int d, m, lds_solve;
};

// The chunking is a function of the shape alone: about FR_TARGET workgroups in all, chunks of at least FR_MINCHUNK points,
// a multiple of the FR_KB points staged at a time.
void frechet_plan(const KgFrechetArgs* a, FrPlan& p) {
    const long fr = (long)a->frames - (a->diff ? 1 : 0);
    p.P[0] = (long)a->n * fr;
    p.P[1] = (long)a->m * fr;
    p.d = a->d_outer * a->d_inner;
    p.m = p.d + (p.d & 1);
    const long per_set = FR_TARGET / (2L * a->classes) > 1 ? FR_TARGET / (2L * a->classes) : 1;
    for (int s = 0; s < 2; ++s) {
        long cs = (p.P[s] + per_set - 1) / per_set;
        if (cs < FR_MINCHUNK) cs = FR_MINCHUNK;
        cs = (cs + FR_KB - 1) / FR_KB * FR_KB;
        p.cs[s] = (int)cs;
        p.nch[s] = (int)((p.P[s] + cs - 1) / cs);
    }
    const long dd = (long)p.d * p.d;
    p.grid_moments = (long)a->classes * (p.nch[0] + p.nch[1]);
    p.grid_merge = (long)a->classes * 2 * ((dd + FR_NT - 1) / FR_NT);
    p.part_doubles = (int64_t)p.grid_moments * (p.d + dd);
    p.ws_bytes = 8 * (p.part_doubles + (int64_t)a->classes * 2 * (p.d + dd));
    p.lds_solve = 2 * p.m * (p.m + 1) * 8;
}

// sides: 1 = the real set, 2 = the fake set(s), 3 = both (kg_frechet); nset: sets of the moments / merge launches.  A call
// for one side alone is handed the other side's count equal to its own, so only its own field is ever named.
int frechet_validate(const KgFrechetArgs* a, const char* who, FrPlan& p, int sides = 3, int nset = 2) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->classes >= 1, "%s: classes=%d < 1", who, a->classes);
    KG_REQUIRE(!(sides & 1) || a->n >= 1, "%s: n=%d < 1", who, a->n);
    KG_REQUIRE(!(sides & 2) || a->m >= 1, "%s: m=%d < 1", who, a->m);
    KG_REQUIRE(a->d_outer >= 1, "%s: d_outer=%d < 1", who, a->d_outer);
    KG_REQUIRE(a->d_inner >= 1, "%s: d_inner=%d < 1", who, a->d_inner);
    KG_REQUIRE(a->diff == 0 || a->diff == 1, "%s: diff=%d is neither 0 (pose) nor 1 (motion)", who, a->diff);
    KG_REQUIRE((long)a->d_outer * a->d_inner <= KG_FRECHET_MAX_DIM, "%s: d = d_outer=%d x d_inner=%d above KG_FRECHET_MAX_DIM = %d",
               who, a->d_outer, a->d_inner, KG_FRECHET_MAX_DIM);
    KG_REQUIRE(a->frames >= 1 + a->diff, "%s: frames=%d < %d%s", who, a->frames, 1 + a->diff,
               a->diff ? " (a motion point needs two frames)" : "");
    const long fr = (long)a->frames - a->diff;
    KG_REQUIRE(!(sides & 1) || (long)a->n * fr >= 2, "%s: n=%d gives P=%ld < 2 real points", who, a->n, (long)a->n * fr);
    KG_REQUIRE(!(sides & 2) || (long)a->m * fr >= 2, "%s: m=%d gives P=%ld < 2 fake points", who, a->m, (long)a->m * fr);
    KG_REQUIRE(!(sides & 1) || (long)a->n * fr <= FR_MAX_POINTS, "%s: n=%d x frames=%d gives P=%ld real points, above 2^24", who,
               a->n, a->frames, (long)a->n * fr);
    KG_REQUIRE(!(sides & 2) || (long)a->m * fr <= FR_MAX_POINTS, "%s: m=%d x frames=%d gives P=%ld fake points, above 2^24", who,
               a->m, a->frames, (long)a->m * fr);
    frechet_plan(a, p);
    if (sides != 3) {           // nset sets of ONE side, each with the chunking kg_frechet gives that side
        const int s = sides == 1 ? 0 : 1;
        const long dd = (long)p.d * p.d;
        p.grid_moments = (long)a->classes * nset * p.nch[s];
        p.grid_merge = (long)a->classes * nset * ((dd + FR_NT - 1) / FR_NT);
        p.part_doubles = (int64_t)p.grid_moments * (p.d + dd);
        p.ws_bytes = 8 * (p.part_doubles + (int64_t)a->classes * nset * (p.d + dd));
    }
    const long grid = p.grid_moments > p.grid_merge ? p.grid_moments : p.grid_merge;
    KG_REQUIRE(grid < FR_MAX_GRID, "%s: classes=%d make %ld workgroups, one launch takes fewer than %ld", who, a->classes, grid,
               FR_MAX_GRID);
    return 0;
}

// set `side` (0 = real, 1 = fake) of the plan read through the caller's strides; ch0: the chunks in front of it
FrSet frechet_set(const float* x, long sc, long ss, long sf, long so, const FrPlan& p, int side, int ch0) {
    FrSet X;
    X.p = x;  X.sc = sc;  X.ss = ss;  X.sf = sf;  X.so = so;
    X.P = (int)p.P[side];  X.cs = p.cs[side];  X.nch = p.nch[side];  X.ch0 = ch0;
    return X;
}

// what every launcher fills alike: the index arithmetic, the shape, and the workspace laid out for nset sets
void frechet_fill(FrDev& d, const FrPlan& p, int nset, int d_inner, int frames, int diff, int classes, void* ws) {
    d.nset = nset;
    d.inner = FastDiv::make((unsigned)d_inner);
    d.fr = FastDiv::make((unsigned)(frames - diff));
    d.d = p.d;  d.diff = diff;  d.classes = classes;
    d.part = (double*)ws;
    d.mu = d.part + p.part_doubles;
    d.cov = d.mu + (long)classes * nset * p.d;
}

// the moments and the merge launch; the status strings are the entry point's own
int frechet_moments_merge(const FrDev& d, const FrPlan& p, hipStream_t s, const char* moments, const char* merge) {
    if (p.d <= 48) hipLaunchKernelGGL(kg_frechet_moments_kernel<3>, dim3((unsigned)p.grid_moments), dim3(FR_NT), 0, s, d);
    else hipLaunchKernelGGL(kg_frechet_moments_kernel<6>, dim3((unsigned)p.grid_moments), dim3(FR_NT), 0, s, d);
    if (int rc = kg_launch_status(moments)) return rc;
    hipLaunchKernelGGL(kg_frechet_merge_kernel, dim3((unsigned)p.grid_merge), dim3(FR_NT), 0, s, d);
    return kg_launch_status(merge);
}

// a solve kernel takes the LDS of d = FR_MAXD: asked for once per device, before the kernel's first launch there
#define FR_SOLVE_LDS(kern_)                                                                               \
    do {                                                                                                  \
        static unsigned long long mask_ = 0;                                                              \
        if (kg_first_on_device(mask_)) KG_SET_DYN_LDS(kern_, 2 * FR_MAXD * (FR_MAXD + 1) * 8);            \
    } while (0)

}  // namespace

extern "C" int64_t kg_frechet_workspace_bytes(const KgFrechetArgs* a) {
    FrPlan p;
    if (int rc = frechet_validate(a, "kg_frechet_workspace_bytes", p)) return rc;
    return p.ws_bytes;
}

extern "C" int kg_frechet(const KgFrechetArgs* a, void* stream) {
    FrPlan p;
    if (int rc = frechet_validate(a, "kg_frechet", p)) return rc;
    KG_REQUIRE(a->real != nullptr, "kg_frechet: null pointer real");
    KG_REQUIRE(a->fake != nullptr, "kg_frechet: null pointer fake");
    KG_REQUIRE(a->values != nullptr, "kg_frechet: null pointer values");
    KG_REQUIRE(a->terms != nullptr, "kg_frechet: null pointer terms");
    KG_REQUIRE(a->sweeps != nullptr, "kg_frechet: null pointer sweeps");
    KG_REQUIRE(a->ws != nullptr, "kg_frechet: null pointer ws");
    KG_REQUIRE(((uintptr_t)a->ws & 7) == 0, "kg_frechet: ws is not 8-byte aligned");
    KG_REQUIRE(a->ws_bytes >= p.ws_bytes, "kg_frechet: ws_bytes=%lld < %lld (kg_frechet_workspace_bytes)", (long long)a->ws_bytes,
               (long long)p.ws_bytes);

    FrDev d = {};
    frechet_fill(d, p, 2, a->d_inner, a->frames, a->diff, a->classes, a->ws);
    d.set[0] = frechet_set(a->real, a->r_sc, a->r_ss, a->r_sf, a->r_so, p, 0, 0);
    d.set[1] = frechet_set(a->fake, a->f_sc, a->f_ss, a->f_sf, a->f_so, p, 1, p.nch[0]);
    d.per = p.nch[0] + p.nch[1];
    d.mu_out[0] = a->mu_real;  d.mu_out[1] = a->mu_fake;
    d.cov_out[0] = a->cov_real;  d.cov_out[1] = a->cov_fake;
    d.values = a->values;  d.terms = a->terms;  d.sweeps = a->sweeps;
    hipStream_t s = (hipStream_t)stream;

    FR_SOLVE_LDS(kg_frechet_solve_kernel);
    if (int rc = frechet_moments_merge(d, p, s, "kg_frechet_moments", "kg_frechet_merge")) return rc;
    hipLaunchKernelGGL(kg_frechet_solve_kernel, dim3((unsigned)a->classes), dim3(FR_SOLVE_NT), (size_t)p.lds_solve, s, d);
    if (int rc = kg_launch_status("kg_frechet_solve")) return rc;
    if (a->mean != nullptr) {
        hipLaunchKernelGGL(kg_frechet_mean_kernel, dim3(1), dim3(64), 0, s, (const double*)a->values, a->mean, a->classes);
        return kg_launch_status("kg_frechet_mean");
    }
    return 0;
}

// ---- the real side once, several fake sets per call --------------------------------------------------------

namespace {

// kg_frechet's shape checks and chunking for ONE side: the other side's count is a copy, so it never decides anything
KgFrechetArgs frechet_side_shape(int count, int frames, int diff, int d_outer, int d_inner, int classes) {
    KgFrechetArgs f = {};
    f.n = count;  f.m = count;  f.frames = frames;  f.diff = diff;
    f.d_outer = d_outer;  f.d_inner = d_inner;  f.classes = classes;
    return f;
}

int frechet_real_validate(const KgFrechetRealArgs* a, const char* who, FrPlan& p) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    const KgFrechetArgs f = frechet_side_shape(a->n, a->frames, a->diff, a->d_outer, a->d_inner, a->classes);
    return frechet_validate(&f, who, p, 1, 1);
}

int frechet_sets_validate(const KgFrechetSetsArgs* a, const char* who, FrPlan& p) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->nsets >= 1 && a->nsets <= KG_FRECHET_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, a->nsets, KG_FRECHET_MAX_SETS);
    const KgFrechetArgs f = frechet_side_shape(a->m, a->frames, a->diff, a->d_outer, a->d_inner, a->classes);
    if (int rc = frechet_validate(&f, who, p, 2, a->nsets)) return rc;
    KG_REQUIRE((long)a->nsets * a->classes < FR_MAX_GRID, "%s: nsets=%d x classes=%d make %ld workgroups, one launch takes fewer than %ld",
               who, a->nsets, a->classes, (long)a->nsets * a->classes, FR_MAX_GRID);
    return 0;
}

}  // namespace

extern "C" int64_t kg_frechet_real_workspace_bytes(const KgFrechetRealArgs* a) {
    FrPlan p;
    if (int rc = frechet_real_validate(a, "kg_frechet_real_workspace_bytes", p)) return rc;
    return p.ws_bytes;
}

extern "C" int kg_frechet_real(const KgFrechetRealArgs* a, void* stream) {
    FrPlan p;
    if (int rc = frechet_real_validate(a, "kg_frechet_real", p)) return rc;
    KG_REQUIRE(a->real != nullptr, "kg_frechet_real: null pointer real");
    KG_REQUIRE(a->mu_real != nullptr, "kg_frechet_real: null pointer mu_real");
    KG_REQUIRE(a->tr_real != nullptr, "kg_frechet_real: null pointer tr_real");
    KG_REQUIRE(a->G != nullptr, "kg_frechet_real: null pointer G");
    KG_REQUIRE(a->sweeps_real != nullptr, "kg_frechet_real: null pointer sweeps_real");
    KG_REQUIRE(a->ws != nullptr, "kg_frechet_real: null pointer ws");
    KG_REQUIRE(((uintptr_t)a->ws & 7) == 0, "kg_frechet_real: ws is not 8-byte aligned");
    KG_REQUIRE(a->ws_bytes >= p.ws_bytes, "kg_frechet_real: ws_bytes=%lld < %lld (kg_frechet_real_workspace_bytes)",
               (long long)a->ws_bytes, (long long)p.ws_bytes);

    FrDev d = {};
    frechet_fill(d, p, 1, a->d_inner, a->frames, a->diff, a->classes, a->ws);
    d.set[0] = frechet_set(a->real, a->r_sc, a->r_ss, a->r_sf, a->r_so, p, 0, 0);
    d.per = p.nch[0];
    d.mu_out[0] = a->mu_real;
    FrRealDev r = {};
    r.cov = d.cov;  r.d = p.d;  r.G = a->G;  r.tr = a->tr_real;  r.sweeps = a->sweeps_real;
    hipStream_t s = (hipStream_t)stream;

    FR_SOLVE_LDS(kg_frechet_real_solve_kernel);
    if (int rc = frechet_moments_merge(d, p, s, "kg_frechet_real moments", "kg_frechet_real merge")) return rc;
    hipLaunchKernelGGL(kg_frechet_real_solve_kernel, dim3((unsigned)a->classes), dim3(FR_SOLVE_NT), (size_t)p.lds_solve, s, r);
    return kg_launch_status("kg_frechet_real solve");
}

extern "C" int64_t kg_frechet_sets_workspace_bytes(const KgFrechetSetsArgs* a) {
    FrPlan p;
    if (int rc = frechet_sets_validate(a, "kg_frechet_sets_workspace_bytes", p)) return rc;
    return p.ws_bytes;
}

extern "C" int kg_frechet_sets(const KgFrechetSetsArgs* a, void* stream) {
    FrPlan p;
    if (int rc = frechet_sets_validate(a, "kg_frechet_sets", p)) return rc;
    for (int g = 0; g < a->nsets; ++g) KG_REQUIRE(a->fake[g] != nullptr, "kg_frechet_sets: null pointer fake[%d]", g);
    KG_REQUIRE(a->mu_real != nullptr, "kg_frechet_sets: null pointer mu_real");
    KG_REQUIRE(a->tr_real != nullptr, "kg_frechet_sets: null pointer tr_real");
    KG_REQUIRE(a->G != nullptr, "kg_frechet_sets: null pointer G");
    KG_REQUIRE(a->values != nullptr, "kg_frechet_sets: null pointer values");
    KG_REQUIRE(a->terms != nullptr, "kg_frechet_sets: null pointer terms");
    KG_REQUIRE(a->sweeps != nullptr, "kg_frechet_sets: null pointer sweeps");
    KG_REQUIRE(a->mean != nullptr, "kg_frechet_sets: null pointer mean");
    KG_REQUIRE(a->mean32 != nullptr, "kg_frechet_sets: null pointer mean32");
    KG_REQUIRE(a->ws != nullptr, "kg_frechet_sets: null pointer ws");
    KG_REQUIRE(((uintptr_t)a->ws & 7) == 0, "kg_frechet_sets: ws is not 8-byte aligned");
    KG_REQUIRE(a->ws_bytes >= p.ws_bytes, "kg_frechet_sets: ws_bytes=%lld < %lld (kg_frechet_sets_workspace_bytes)",
               (long long)a->ws_bytes, (long long)p.ws_bytes);

    FrDev d = {};
    frechet_fill(d, p, a->nsets, a->d_inner, a->frames, a->diff, a->classes, a->ws);
    for (int g = 0; g < a->nsets; ++g) d.set[g] = frechet_set(a->fake[g], a->f_sc, a->f_ss, a->f_sf, a->f_so, p, 1, g * p.nch[1]);
    d.per = a->nsets * p.nch[1];
    FrSetsDev v = {};
    v.mu = d.mu;  v.cov = d.cov;  v.mu_real = a->mu_real;  v.tr_real = a->tr_real;  v.G = a->G;
    v.d = p.d;  v.nsets = a->nsets;  v.classes = a->classes;
    v.values = a->values;  v.terms = a->terms;  v.sweeps = a->sweeps;
    hipStream_t s = (hipStream_t)stream;

    FR_SOLVE_LDS(kg_frechet_sets_solve_kernel);
    if (int rc = frechet_moments_merge(d, p, s, "kg_frechet_sets moments", "kg_frechet_sets merge")) return rc;
    hipLaunchKernelGGL(kg_frechet_sets_solve_kernel, dim3((unsigned)(a->nsets * a->classes)), dim3(FR_SOLVE_NT), (size_t)p.lds_solve, s, v);
    if (int rc = kg_launch_status("kg_frechet_sets solve")) return rc;
    hipLaunchKernelGGL(kg_frechet_sets_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)a->values, a->mean, a->mean32,
                       a->classes, a->nsets);
    return kg_launch_status("kg_frechet_sets finish");
}
