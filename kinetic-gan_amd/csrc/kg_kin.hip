// Kinematic plausibility of skeleton sequences (see include/kgan_hip.h): six dimensionless descriptors per
// sample - bone-length constancy, left / right symmetry, speed, acceleration, jerk, stillness - and, per class and
// descriptor, the Wasserstein-1 distance between the real and the generated samples' values.
//
// kg_kin_desc_kernel: one workgroup = one sample.  The sample goes through the strides into LDS once (fp32, [c][f][v]); every
// later read is an LDS read.  Bones: thread (b = tid mod 32, q = tid div 32) adds the lengths of bone b at the frames q,
// q + 8, .. in frame order, the 8 partials of a bone are added as ((0+1)+(2+3))+((4+5)+(6+7)); the second pass about mu_b has
// the same shape.  Joints: element e = f V + v of the [f][v] plane IS the LDS offset, so D1 .. D3 need no division; a thread
// adds its elements e = tid, tid + 256, .. in order, then a shuffle tree and the four waves in order.  Every sum's shape
// depends on (T, V, B) alone.  fp64 throughout; one rounding to fp32 at the store.
// The tables (bones, mirror) travel in the kernel arguments and are moved into LDS with constant indices only (a lane-indexed
// read of an argument array would put the whole struct into scratch).
// degenerate: thread 0 stores the sample's flag (kg_handoff.h), the last workgroup to arrive counts every class's flags - a
// wave per class, integer adds.
// kg_kin_desc_sets: the same kernel body over nsets sets with shared strides - workgroup (g, class, sample), the set slowest;
// the set's two pointers are picked with constant indices (the rule of the tables above), everything behind them is the
// one-set code, so every set has the bits of its own kg_kin_desc call.  ONE ticket over the whole grid; the last arriver
// counts the flags of every (set, class).  kg_kin_desc is the one-set case: one body (a template, whose one-set instantiation
// has the set coordinate compiled away), one validation, one launcher.
//
// kg_kin_w1_kernel: one workgroup = one (set, class, descriptor) column.  ONE LDS array of P 8-byte words, P the power of two
// >= n + m, serves in turn as: the real values as doubles (tree -> mean_real, set 0 only), the fake values (tree ->
// mean_fake), the n + m sort keys, and the terms (written over the keys: a thread owns a contiguous run of positions and has
// read its right neighbour's first key before anyone writes).  key = (image << 1) | side, image = the order-preserving
// unsigned image of the fp32 bits (-0.0 below +0.0: their gap is 0), padding = all ones.  The tree runs over P words: the words
// behind the n + m - 1 terms are +0.0, and x + +0.0 == x for the non-negative terms, so the wider tree has the bits of the
// definition's.
// kg_kin_finish_kernel: a workgroup per (side, class) counts the samples with a non-finite descriptor; workgroup 0 also adds
// the classes' w1 in class order.
// No atomics on global memory but the ticket of kg_kin_desc; no scratch; no dynamically indexed private array.
#include <math.h>

#include "kg_common.h"
#include "kg_handoff.h"

namespace {

constexpr int KD_NT = 256;                      // threads of a descriptor workgroup
constexpr int KD_FL = 8;                        // frame lanes per bone
constexpr int KD_MAXB = KG_KIN_MAX_BONES, KD_MAXM = KG_KIN_MAX_MIRROR;
static_assert(KD_MAXB * KD_FL == KD_NT && 2 * KD_MAXB + 2 * KD_MAXM <= KD_NT, "kg_kin_desc: thread mapping");

// the fixed part of the LDS, in front of the staged sample (doubles first: 8-byte aligned at offset 0)
struct KdFixed {
    double part[KD_FL][KD_MAXB];
    double mu[KD_MAXB];
    double cv[KD_MAXB];
    double red[KD_NT / 64][4];
    double s, bone_cv, asym, pad_;
    int tab[2 * KD_MAXB + 2 * KD_MAXM];         // bones, then mirror
    int last, pad2_[3];
};
static_assert(sizeof(KdFixed) % 16 == 0, "kg_kin_desc: the staged sample starts 16-byte aligned");

struct KinDescDev {
    const float* x[KG_KIN_MAX_SETS];  long sc, ss, sf, so;
    int n, T, C, V, classes, B, M, nsets;
    double still_eps;
    float* desc[KG_KIN_MAX_SETS];  int* degenerate;  float* flags;  int* counter;
    FastDiv divTV, divV;
    int bones[2 * KD_MAXB];
    int mirror[2 * KD_MAXM];
};

__device__ __forceinline__ double kd_len(const float* xs, int C, int TV, int pu, int pv) {
    const double d0 = (double)xs[pu] - (double)xs[pv];
    const double d1 = (double)xs[TV + pu] - (double)xs[TV + pv];
    double q = d0 * d0 + d1 * d1;
    if (C == 3) {
        const double d2 = (double)xs[2 * TV + pu] - (double)xs[2 * TV + pv];
        q += d2 * d2;
    }
    return sqrt(q);
}

__device__ __forceinline__ double kd_norm(double d0, double d1, double d2) { return sqrt(d0 * d0 + d1 * d1 + d2 * d2); }

// SETS = false: the one-set instantiation - g is the constant 0, so the set coordinate, its division and the pointer choice
// compile away and kg_kin_desc (and a kg_kin_desc_sets call with one set) runs the code it ran before the sets existed
template <bool SETS>
__global__ __launch_bounds__(KD_NT) void kg_kin_desc_kernel(const KinDescDev a) {
    extern __shared__ __attribute__((aligned(16))) char kd_smem[];
    KdFixed& F = *(KdFixed*)kd_smem;
    float* xs = (float*)(kd_smem + sizeof(KdFixed));
    const int tid = threadIdx.x;
    const int T = a.T, C = a.C, V = a.V, B = a.B, M = a.M, TV = T * V;
    // workgroup = (set g, class, sample), the set slowest; row = the sample's row in its set's (classes, n) outputs
    const int per_set = a.classes * a.n, g = SETS ? (int)blockIdx.x / per_set : 0, row = (int)blockIdx.x - g * per_set;
    const int cls = row / a.n, smp = row - cls * a.n;
    // (the set's two pointers are picked with constant indices, each where it is used: picked up here, all eight are live
    // across the table moves and cost the eighth wave per SIMD)
    static_assert(KG_KIN_MAX_SETS == 4, "kg_kin_desc: the set's pointers are picked with constant indices");

    // tables -> LDS (constant indices into the arguments)
    {
        int v = 0;
#pragma unroll
        for (int i = 0; i < 2 * KD_MAXB; ++i) v = tid == i ? a.bones[i] : v;
#pragma unroll
        for (int i = 0; i < 2 * KD_MAXM; ++i) v = tid == 2 * KD_MAXB + i ? a.mirror[i] : v;
        if (tid < 2 * KD_MAXB + 2 * KD_MAXM) F.tab[tid] = v;
    }
    // the sample -> LDS, [c][f][v]
    {
        const float* xg = g == 0 ? a.x[0] : g == 1 ? a.x[1] : g == 2 ? a.x[2] : a.x[3];
        const float* src = xg + (long)cls * a.sc + (long)smp * a.ss;
        const int tot = C * TV;
        for (int e = tid; e < tot; e += KD_NT) {
            unsigned c, r, f, v;
            a.divTV.divmod((unsigned)e, c, r);
            a.divV.divmod(r, f, v);
            xs[e] = src[(long)f * a.sf + (long)c * a.so + v];
        }
    }
    __syncthreads();

    // bones, pass 1: sums of lengths
    const int b = tid & (KD_MAXB - 1), q = tid / KD_MAXB;
    const int ju = b < B ? F.tab[2 * b] : 0, jv = b < B ? F.tab[2 * b + 1] : 0;
    {
        double acc = 0.0;
        if (b < B)
            for (int f = q; f < T; f += KD_FL) acc += kd_len(xs, C, TV, f * V + ju, f * V + jv);
        F.part[q][b] = acc;
    }
    __syncthreads();
    if (tid < KD_MAXB) {
        const double sum = ((F.part[0][tid] + F.part[1][tid]) + (F.part[2][tid] + F.part[3][tid])) +
                           ((F.part[4][tid] + F.part[5][tid]) + (F.part[6][tid] + F.part[7][tid]));
        F.mu[tid] = sum / (double)T;
        F.cv[tid] = sum;                        // (the bone's sum, until pass 2 puts sd / mu here)
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < B; ++i) tot += F.cv[i];
        F.s = tot / ((double)B * (double)T);
    }
    // pass 2: squared deviations from mu_b
    const double mu_b = F.mu[b];
    __syncthreads();
    {
        double acc = 0.0;
        if (b < B)
            for (int f = q; f < T; f += KD_FL) {
                const double d = kd_len(xs, C, TV, f * V + ju, f * V + jv) - mu_b;
                acc += d * d;
            }
        F.part[q][b] = acc;
    }
    __syncthreads();
    if (tid < KD_MAXB) {
        const double ssq = ((F.part[0][tid] + F.part[1][tid]) + (F.part[2][tid] + F.part[3][tid])) +
                           ((F.part[4][tid] + F.part[5][tid]) + (F.part[6][tid] + F.part[7][tid]));
        const double sd = sqrt(ssq / (double)T), mu = F.mu[tid];
        F.cv[tid] = mu != 0.0 ? sd / mu : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < B; ++i) tot += F.cv[i];
        F.bone_cv = tot / (double)B;
        double as = 0.0;
        for (int p = 0; p < M; ++p) {
            const double ma = F.mu[F.tab[2 * KD_MAXB + 2 * p]], mb = F.mu[F.tab[2 * KD_MAXB + 2 * p + 1]];
            const double den = 0.5 * (ma + mb);
            as += den != 0.0 ? fabs(ma - mb) / den : 0.0;
        }
        F.asym = M > 0 ? as / (double)M : 0.0;
    }

    // joints: |D1|, |D2|, |D3| of element e = f V + v, f < T - 1 (F.s is visible: two barriers since it was written)
    const double s = F.s, thr = a.still_eps * s;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int still = 0;
    const int n1 = (T - 1) * V, n2 = (T - 2) * V, n3 = (T - 3) * V;
    for (int e = tid; e < n1; e += KD_NT) {
        double d[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < C) {
                const float* p = xs + c * TV + e;
                const double x0 = (double)p[0], x1 = (double)p[V];
                d[0][c] = x1 - x0;
                if (e < n2) {
                    const double x2 = (double)p[2 * V];
                    d[1][c] = (x2 - 2.0 * x1) + x0;
                    if (e < n3) {
                        const double x3 = (double)p[3 * V];
                        d[2][c] = ((x3 - 3.0 * x2) + 3.0 * x1) - x0;
                    }
                }
            }
        }
        const double v1 = kd_norm(d[0][0], d[0][1], d[0][2]);
        s1 += v1;
        still += v1 < thr ? 1 : 0;
        if (e < n2) s2 += kd_norm(d[1][0], d[1][1], d[1][2]);
        if (e < n3) s3 += kd_norm(d[2][0], d[2][1], d[2][2]);
    }
    double cnt = (double)still;                 // (an integer below 2^24: exact in every order)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off, 64);
        s2 += __shfl_xor(s2, off, 64);
        s3 += __shfl_xor(s3, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
    }
    if ((tid & 63) == 0) {
        F.red[tid >> 6][0] = s1;
        F.red[tid >> 6][1] = s2;
        F.red[tid >> 6][2] = s3;
        F.red[tid >> 6][3] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        double r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (F.red[0][k] + F.red[1][k]) + (F.red[2][k] + F.red[3][k]);
        const bool degen = s == 0.0;
        float* dg = g == 0 ? a.desc[0] : g == 1 ? a.desc[1] : g == 2 ? a.desc[2] : a.desc[3];
        float* o = dg + (long)row * KG_KIN_DESC;
        o[0] = degen ? 0.f : (float)F.bone_cv;
        o[1] = degen ? 0.f : (float)F.asym;
        o[2] = degen ? 0.f : (float)(r[0] / (double)n1 / s);
        o[3] = degen ? 0.f : (float)(r[1] / (double)n2 / s);
        o[4] = degen ? 0.f : (float)(r[2] / (double)n3 / s);
        o[5] = degen ? 0.f : (float)(r[3] / (double)n1);
        kg_pub_store(a.flags + blockIdx.x, degen ? 1.f : 0.f);
        F.last = kg_ticket_draw(a.counter, (int)gridDim.x) ? 1 : 0;
    }
    __syncthreads();
    if (!F.last) return;
    // the last workgroup to arrive: a wave per (set, class) counts the flags (integers: any order gives the same count);
    // flags and degenerate are (nsets, classes, ..): c walks the sets' classes in one go
    const int lane = tid & 63;
    for (int c = tid >> 6; c < (SETS ? a.nsets : 1) * a.classes; c += KD_NT / 64) {
        int k = 0;
        for (int i = lane; i < a.n; i += 64) k += kg_pub_load(a.flags + (long)c * a.n + i) != 0.f ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) k += __shfl_xor(k, off, 64);
        if (lane == 0) a.degenerate[c] = k;
    }
}

// ---- scores -------------------------------------------------------------------------------------------------------------------
constexpr unsigned long long KW_PAD = ~0ull;

__device__ __forceinline__ unsigned long long kw_key(float v, int side) {
    const unsigned u = __float_as_uint(v);
    const unsigned img = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)img << 1) | (unsigned long long)side;
}
__device__ __forceinline__ double kw_value(unsigned long long key) {
    const unsigned img = (unsigned)(key >> 1);
    const unsigned u = (img & 0x80000000u) ? (img ^ 0x80000000u) : ~img;
    return (double)__uint_as_float(u);
}
__device__ __forceinline__ bool kw_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// buf[0] = the pairwise tree over the P words of buf (P a power of two); all threads call it, a barrier precedes every read
template <int NT>
__device__ __forceinline__ double kw_tree(double* buf, int P, int tid) {
    for (int h = P >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        for (int i = tid; i < h; i += NT) buf[i] += buf[i + h];
    }
    __syncthreads();
    const double r = buf[0];
    __syncthreads();                            // (the caller refills buf)
    return r;
}

// the mean of column j of cnt rows (tree over the next power of two Pc <= P)
template <int NT>
__device__ __forceinline__ double kw_mean(double* buf, const float* col, int cnt, int Pc, int tid) {
    for (int i = tid; i < Pc; i += NT) buf[i] = i < cnt ? (double)col[(long)i * KG_KIN_DESC] : 0.0;
    return kw_tree<NT>(buf, Pc, tid) / (double)cnt;
}

template <int NT>
__global__ __launch_bounds__(NT) void kg_kin_w1_kernel(const KgKinScoresArgs a, int P, int Pr, int Pf) {
    extern __shared__ __attribute__((aligned(16))) char kw_smem[];
    unsigned long long* keys = (unsigned long long*)kw_smem;
    double* buf = (double*)kw_smem;
    int* cnts = (int*)(kw_smem + (size_t)P * 8);
    int* bad = cnts + NT;
    const int tid = threadIdx.x, n = a.n, m = a.m, N = n + m;
    const int blk = (int)blockIdx.x, j = blk % KG_KIN_DESC, gc = blk / KG_KIN_DESC, c = gc % a.classes, g = gc / a.classes;
    const float* fk = g == 0 ? a.fake[0] : g == 1 ? a.fake[1] : g == 2 ? a.fake[2] : a.fake[3];
    const float* rcol = a.real + (long)c * n * KG_KIN_DESC + j;
    const float* fcol = fk + (long)c * m * KG_KIN_DESC + j;

    if (g == 0) {
        const double mr = kw_mean<NT>(buf, rcol, n, Pr, tid);
        if (tid == 0) a.mean_real[c * KG_KIN_DESC + j] = mr;
    }
    {
        const double mf = kw_mean<NT>(buf, fcol, m, Pf, tid);
        if (tid == 0) a.mean_fake[(long)gc * KG_KIN_DESC + j] = mf;
    }
    // keys
    if (tid == 0) *bad = 0;
    __syncthreads();
    {
        bool nf = false;
        for (int i = tid; i < P; i += NT) {
            unsigned long long k = KW_PAD;
            if (i < N) {
                const float v = i < n ? rcol[(long)i * KG_KIN_DESC] : fcol[(long)(i - n) * KG_KIN_DESC];
                nf |= !kw_finite(v);
                k = kw_key(v, i < n ? 0 : 1);
            }
            keys[i] = k;
        }
        if (nf) *bad = 1;
    }
    __syncthreads();
    if (*bad) {                                 // (uniform)
        if (tid == 0) a.w1[(long)gc * KG_KIN_DESC + j] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    // bitonic sort, ascending
    for (int k = 2; k <= P; k <<= 1)
        for (int st = k >> 1; st > 0; st >>= 1) {
            for (int t = tid; t < (P >> 1); t += NT) {
                const int i = 2 * t - (t & (st - 1)), l = i + st;
                const unsigned long long x = keys[i], y = keys[l];
                if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
            }
            __syncthreads();
        }
    // prefix count of the real keys: thread t owns the positions [t per, t per + per)
    const int per = P >= NT ? P / NT : 1, i0 = tid * per;
    int mine = 0;
    unsigned long long nxt = KW_PAD;
    if (i0 < P) {
        for (int i = i0; i < i0 + per; ++i) mine += (keys[i] != KW_PAD && (keys[i] & 1ull) == 0) ? 1 : 0;
        if (i0 + per < P) nxt = keys[i0 + per];
    }
    cnts[tid] = mine;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const int v = tid >= off ? cnts[tid - off] : 0;
        __syncthreads();
        cnts[tid] += v;
        __syncthreads();
    }
    // the terms, written over the keys (every thread holds its right neighbour's first key)
    if (i0 < P) {
        long long cr = cnts[tid] - mine;
        unsigned long long cur = keys[i0];
        for (int i = i0; i < i0 + per; ++i) {
            const unsigned long long next = i + 1 < i0 + per ? keys[i + 1] : nxt;
            double term = 0.0;
            if (i < N - 1) {
                cr += (cur & 1ull) == 0 ? 1 : 0;
                const long long cf = (long long)(i + 1) - cr;
                const long long w = cr * (long long)m - cf * (long long)n;
                term = (double)(w < 0 ? -w : w) * (kw_value(next) - kw_value(cur));
            }
            buf[i] = term;
            cur = next;
        }
    }
    const double tot = kw_tree<NT>(buf, P, tid);
    if (tid == 0) a.w1[(long)gc * KG_KIN_DESC + j] = tot / (double)((long long)n * (long long)m);
}

constexpr int KF_NT = 256;

__global__ __launch_bounds__(KF_NT) void kg_kin_finish_kernel(const KgKinScoresArgs a) {
    __shared__ int tot_s[KF_NT / 64];
    const int tid = threadIdx.x, blk = (int)blockIdx.x, r = blk / a.classes, c = blk - r * a.classes;
    const float* src = r == 0 ? a.real : r == 1 ? a.fake[0] : r == 2 ? a.fake[1] : r == 3 ? a.fake[2] : a.fake[3];
    const int cnt = r == 0 ? a.n : a.m;
    src += (long)c * cnt * KG_KIN_DESC;
    int k = 0;
    for (int i = tid; i < cnt; i += KF_NT) {
        bool nf = false;
#pragma unroll
        for (int q = 0; q < KG_KIN_DESC; ++q) nf |= !kw_finite(src[(long)i * KG_KIN_DESC + q]);
        k += nf ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) k += __shfl_xor(k, off, 64);
    if ((tid & 63) == 0) tot_s[tid >> 6] = k;
    __syncthreads();
    if (tid == 0) a.nonfinite[blk] = (tot_s[0] + tot_s[1]) + (tot_s[2] + tot_s[3]);
    if (blk == 0 && tid < a.nsets * KG_KIN_DESC) {
        const int g = tid / KG_KIN_DESC, j = tid - g * KG_KIN_DESC;
        double sum = 0.0;
        for (int cc = 0; cc < a.classes; ++cc) sum += a.w1[((long)g * a.classes + cc) * KG_KIN_DESC + j];
        const double mean = sum / (double)a.classes;
        a.w1_mean[tid] = mean;
        a.scores[tid] = (float)mean;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int next_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// everything but the device pointers: the shape, the strides, the two host tables, still_eps.  A = KgKinDescArgs (nsets = 1)
// or KgKinDescSetsArgs, which share every field name read here
template <class A>
int kin_desc_validate(const A* a, int nsets, const char* who) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(nsets >= 1 && nsets <= KG_KIN_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, nsets, KG_KIN_MAX_SETS);
    KG_REQUIRE(a->classes >= 1, "%s: classes=%d < 1", who, a->classes);
    KG_REQUIRE(a->n >= 1, "%s: n=%d < 1", who, a->n);
    KG_REQUIRE((long)a->classes * a->n < (1L << 24), "%s: classes * n = %ld samples, at most 2^24 - 1", who, (long)a->classes * a->n);
    KG_REQUIRE((long)nsets * a->classes * a->n < (1L << 24), "%s: nsets * classes * n = %ld workgroups, at most 2^24 - 1", who,
               (long)nsets * a->classes * a->n);
    KG_REQUIRE(a->C == 2 || a->C == 3, "%s: C=%d is not 2 or 3", who, a->C);
    KG_REQUIRE(a->V >= 1 && a->V <= KG_KIN_MAX_JOINTS, "%s: V=%d outside [1, %d]", who, a->V, KG_KIN_MAX_JOINTS);
    KG_REQUIRE(a->B >= 1 && a->B <= KG_KIN_MAX_BONES, "%s: B=%d outside [1, %d]", who, a->B, KG_KIN_MAX_BONES);
    KG_REQUIRE(a->M >= 0 && a->M <= KG_KIN_MAX_MIRROR, "%s: M=%d outside [0, %d]", who, a->M, KG_KIN_MAX_MIRROR);
    KG_REQUIRE(a->T >= KG_KIN_MIN_FRAMES, "%s: T=%d < %d frames (jerk needs four)", who, a->T, KG_KIN_MIN_FRAMES);
    KG_REQUIRE((long)a->C * a->T * a->V <= KG_KIN_MAX_ELEMS, "%s: C*T*V = %ld above %d (the sample is staged in LDS)", who,
               (long)a->C * a->T * a->V, KG_KIN_MAX_ELEMS);
    KG_REQUIRE(a->sc >= 0 && a->ss >= 0 && a->sf >= 0 && a->so >= 0, "%s: negative stride (sc, ss, sf, so)", who);
    KG_REQUIRE(isfinite(a->still_eps) && a->still_eps >= 0.0, "%s: still_eps=%g is not a finite number >= 0", who, a->still_eps);
    KG_REQUIRE(a->bones != nullptr, "%s: null pointer bones", who);
    KG_REQUIRE(a->M == 0 || a->mirror != nullptr, "%s: null pointer mirror with M=%d", who, a->M);
    for (int b = 0; b < 2 * a->B; ++b)
        KG_REQUIRE(a->bones[b] >= 0 && a->bones[b] < a->V, "%s: bones[%d][%d]=%d outside [0, V=%d)", who, b / 2, b % 2, a->bones[b], a->V);
    for (int p = 0; p < 2 * a->M; ++p)
        KG_REQUIRE(a->mirror[p] >= 0 && a->mirror[p] < a->B, "%s: mirror[%d][%d]=%d outside [0, B=%d)", who, p / 2, p % 2, a->mirror[p],
                   a->B);
    return 0;
}

template <class A>
int64_t kin_desc_lds(const A* a) { return (int64_t)sizeof(KdFixed) + 4 * (int64_t)a->C * a->T * a->V; }

int kin_scores_validate(const KgKinScoresArgs* a, const char* who) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->nsets >= 1 && a->nsets <= KG_KIN_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, a->nsets, KG_KIN_MAX_SETS);
    KG_REQUIRE(a->classes >= 1 && a->classes <= (1 << 20), "%s: classes=%d outside [1, 2^20]", who, a->classes);
    KG_REQUIRE(a->n >= 1, "%s: n=%d < 1", who, a->n);
    KG_REQUIRE(a->m >= 1, "%s: m=%d < 1", who, a->m);
    KG_REQUIRE((long)a->n + a->m <= KG_KIN_MAX_POINTS, "%s: n + m = %ld above the cap of %d points", who, (long)a->n + a->m,
               KG_KIN_MAX_POINTS);
    return 0;
}

struct KwPlan { int P, Pr, Pf, nt; int64_t lds; };
KwPlan kin_scores_plan(const KgKinScoresArgs* a) {
    KwPlan p;
    p.P = next_pow2(a->n + a->m);
    p.Pr = next_pow2(a->n);
    p.Pf = next_pow2(a->m);
    p.nt = p.P <= 2048 ? 256 : 1024;
    p.lds = 8 * (int64_t)p.P + 4 * (int64_t)p.nt + 16;
    return p;
}
constexpr int KW_MAX_LDS_256 = 8 * 2048 + 4 * 256 + 16, KW_MAX_LDS_1024 = 8 * KG_KIN_MAX_POINTS + 4 * 1024 + 16;
constexpr int KD_MAX_LDS = (int)sizeof(KdFixed) + 4 * KG_KIN_MAX_ELEMS;
static_assert(KW_MAX_LDS_1024 <= 160 * 1024 && KD_MAX_LDS <= 160 * 1024, "kg_kin: one workgroup's LDS");

}  // namespace

extern "C" int64_t kg_kin_desc_workspace_bytes(const KgKinDescArgs* a) {
    if (int rc = kin_desc_validate(a, 1, "kg_kin_desc_workspace_bytes")) return rc;
    return 4 * (int64_t)a->classes * a->n;
}

extern "C" int64_t kg_kin_desc_lds_bytes(const KgKinDescArgs* a) {
    if (int rc = kin_desc_validate(a, 1, "kg_kin_desc_lds_bytes")) return rc;
    return kin_desc_lds(a);
}

extern "C" int64_t kg_kin_desc_sets_workspace_bytes(const KgKinDescSetsArgs* a) {
    if (int rc = kin_desc_validate(a, a != nullptr ? a->nsets : 1, "kg_kin_desc_sets_workspace_bytes")) return rc;
    return 4 * (int64_t)a->nsets * a->classes * a->n;
}

extern "C" int64_t kg_kin_desc_sets_lds_bytes(const KgKinDescSetsArgs* a) {
    if (int rc = kin_desc_validate(a, a != nullptr ? a->nsets : 1, "kg_kin_desc_sets_lds_bytes")) return rc;
    return kin_desc_lds(a);
}

namespace {

unsigned long long kd_attr_mask = 0;     // (one for both instantiations of the launcher: they launch the same kernel)

// Both descriptor entry points behind their validation: the pointer checks, the kernel's arguments and the ONE launch of
// nsets * classes * n workgroups; x / desc: the nsets pointers of the call
template <class A>
int kin_desc_launch(const char* who, const A* a, int nsets, bool indexed, const float* const* x, float* const* desc, void* stream) {
    for (int g = 0; g < nsets; ++g) {       // (the messages name the field of the caller's struct: x or x[g])
        char at[16] = "";
        if (indexed) snprintf(at, sizeof(at), "[%d]", g);
        KG_REQUIRE(x[g] != nullptr, "%s: null pointer x%s", who, at);
        KG_REQUIRE(desc[g] != nullptr, "%s: null pointer desc%s", who, at);
    }
    KG_REQUIRE(a->degenerate != nullptr, "%s: null pointer degenerate", who);
    KG_REQUIRE(a->ws != nullptr, "%s: null pointer ws", who);
    KG_REQUIRE(a->counters != nullptr, "%s: null pointer counters", who);
    KG_REQUIRE(a->counters_len >= 1, "%s: counters_len=%d < 1", who, a->counters_len);
    const int64_t need = 4 * (int64_t)nsets * a->classes * a->n;
    KG_REQUIRE(a->ws_bytes >= need, "%s: ws_bytes=%lld < %lld (%s_workspace_bytes)", who, (long long)a->ws_bytes, (long long)need, who);
    KinDescDev d = {};
    for (int g = 0; g < nsets; ++g) {
        d.x[g] = x[g];
        d.desc[g] = desc[g];
    }
    d.sc = a->sc;  d.ss = a->ss;  d.sf = a->sf;  d.so = a->so;
    d.n = a->n;  d.T = a->T;  d.C = a->C;  d.V = a->V;  d.classes = a->classes;  d.B = a->B;  d.M = a->M;  d.nsets = nsets;
    d.still_eps = a->still_eps;
    d.degenerate = a->degenerate;  d.flags = a->ws;  d.counter = a->counters;
    d.divTV = FastDiv::make((unsigned)(a->T * a->V));
    d.divV = FastDiv::make((unsigned)a->V);
    for (int b = 0; b < 2 * a->B; ++b) d.bones[b] = a->bones[b];
    for (int p = 0; p < 2 * a->M; ++p) d.mirror[p] = a->mirror[p];
    if (kg_first_on_device(kd_attr_mask)) {
        KG_SET_DYN_LDS(kg_kin_desc_kernel<false>, KD_MAX_LDS);
        KG_SET_DYN_LDS(kg_kin_desc_kernel<true>, KD_MAX_LDS);
    }
    const dim3 grid(nsets * a->classes * a->n);
    if (nsets == 1)
        hipLaunchKernelGGL(kg_kin_desc_kernel<false>, grid, dim3(KD_NT), (size_t)kin_desc_lds(a), (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL(kg_kin_desc_kernel<true>, grid, dim3(KD_NT), (size_t)kin_desc_lds(a), (hipStream_t)stream, d);
    return kg_launch_status(who);
}

}  // namespace

extern "C" int kg_kin_desc(const KgKinDescArgs* a, void* stream) {
    const char* who = "kg_kin_desc";
    if (int rc = kin_desc_validate(a, 1, who)) return rc;
    const float* x[1] = {a->x};
    float* desc[1] = {a->desc};
    return kin_desc_launch(who, a, 1, /*indexed=*/false, x, desc, stream);
}

extern "C" int kg_kin_desc_sets(const KgKinDescSetsArgs* a, void* stream) {
    const char* who = "kg_kin_desc_sets";
    if (int rc = kin_desc_validate(a, a != nullptr ? a->nsets : 1, who)) return rc;
    return kin_desc_launch(who, a, a->nsets, /*indexed=*/true, a->x, a->desc, stream);
}

extern "C" int64_t kg_kin_scores_lds_bytes(const KgKinScoresArgs* a) {
    if (int rc = kin_scores_validate(a, "kg_kin_scores_lds_bytes")) return rc;
    return kin_scores_plan(a).lds;
}

extern "C" int kg_kin_scores(const KgKinScoresArgs* a, void* stream) {
    const char* who = "kg_kin_scores";
    if (int rc = kin_scores_validate(a, who)) return rc;
    KG_REQUIRE(a->real != nullptr, "%s: null pointer real", who);
    for (int g = 0; g < a->nsets; ++g) KG_REQUIRE(a->fake[g] != nullptr, "%s: null pointer fake[%d]", who, g);
    KG_REQUIRE(a->mean_real != nullptr, "%s: null pointer mean_real", who);
    KG_REQUIRE(a->mean_fake != nullptr, "%s: null pointer mean_fake", who);
    KG_REQUIRE(a->w1 != nullptr, "%s: null pointer w1", who);
    KG_REQUIRE(a->w1_mean != nullptr, "%s: null pointer w1_mean", who);
    KG_REQUIRE(a->scores != nullptr, "%s: null pointer scores", who);
    KG_REQUIRE(a->nonfinite != nullptr, "%s: null pointer nonfinite", who);
    const KwPlan p = kin_scores_plan(a);
    static unsigned long long attr_mask = 0;
    if (kg_first_on_device(attr_mask)) {
        KG_SET_DYN_LDS(kg_kin_w1_kernel<256>, KW_MAX_LDS_256);
        KG_SET_DYN_LDS(kg_kin_w1_kernel<1024>, KW_MAX_LDS_1024);
    }
    const dim3 grid(a->nsets * a->classes * KG_KIN_DESC);
    if (p.nt == 256)
        hipLaunchKernelGGL(kg_kin_w1_kernel<256>, grid, dim3(256), (size_t)p.lds, (hipStream_t)stream, *a, p.P, p.Pr, p.Pf);
    else
        hipLaunchKernelGGL(kg_kin_w1_kernel<1024>, grid, dim3(1024), (size_t)p.lds, (hipStream_t)stream, *a, p.P, p.Pr, p.Pf);
    if (int rc = kg_launch_status("kg_kin_scores (w1)")) return rc;
    hipLaunchKernelGGL(kg_kin_finish_kernel, dim3((a->nsets + 1) * a->classes), dim3(KF_NT), 0, (hipStream_t)stream, *a);
    return kg_launch_status(who);
}
