// The action classifier's head (classifier.Classifier; include/kgan_hip.h "action classifier head"):
//
//   kg_cls_head_fwd     global average pool -> fc1 + LeakyReLU -> fcn -> log-sum-exp, per-sample loss, argmax; one workgroup
//                       per KG_CLS_TILE samples, then ONE workgroup for the batch mean of the loss and the correct count
//   kg_cls_head_bwd     softmax cross-entropy, fcn^T, LeakyReLU', fc1^T and the trunk's top gradient, same tiles
//   kg_cls_head_wgrad   the four parameter gradients: one thread per output element, summed over the samples in index order
//   kg_cls_scores       accuracy, per-class counts, diversity and multimodality of up to KG_CLS_MAX_SETS sets:
//                       a wave per (set, pair) for the fp64 feature distances, then ONE workgroup per set for the tallies
//                       (integer adds in LDS) and the two means (one thread, index order)
//
// Latency bound (fc1.weight, 128 KB at the default sizes, is the largest operand).  Deterministic: every output element has
// one owner, workgroups exchange nothing inside a launch - no tickets, no atomics, no polled words.
#include "kg_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int NT = 256, NW = NT / 64, TILE = KG_CLS_TILE;
constexpr int MAXC = KG_CLS_MAX_C, MAXF = KG_FRECHET_MAX_DIM, MAXL = KG_CLS_MAX_CLASSES;
static_assert(TILE == NW, "one wave per sample of the tile in the softmax steps");

// (every lane gets the total)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the largest non-NaN value of x[0..L) in every lane (-inf when there is none)
__device__ __forceinline__ float wave_row_max(const float* x, int L, int lane) {
    float m = -INFINITY;
    for (int l = lane; l < L; l += 64) {
        const float v = x[l];
        if (v > m) m = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(m, off, 64);
        if (o > m) m = o;
    }
    return m;
}

// acc[s] = sum_k w[k] * x[s * ld + k] over the lanes of a wave (k = lane, lane + 64, ...; x in LDS); every lane gets the totals
__device__ __forceinline__ void wave_dot_tile(const float* w, const float* x, int K, int ld, int lane, float (&acc)[TILE]) {
#pragma unroll
    for (int s = 0; s < TILE; ++s) acc[s] = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float wv = w[k];
#pragma unroll
        for (int s = 0; s < TILE; ++s) acc[s] = fmaf(wv, x[s * ld + k], acc[s]);
    }
#pragma unroll
    for (int s = 0; s < TILE; ++s) acc[s] = wave_sum(acc[s]);
}

// acc[lane] without a run-time index into the register array
__device__ __forceinline__ float pick(const float (&acc)[TILE], int lane) {
    float v = 0.f;
#pragma unroll
    for (int s = 0; s < TILE; ++s)
        if (lane == s) v = acc[s];
    return v;
}

__global__ __launch_bounds__(NT) void kg_cls_head_fwd_kernel(const KgClsHeadArgs a) {
    __shared__ float pooled_s[TILE * MAXC];
    __shared__ float feat_s[TILE * MAXF];
    __shared__ float logit_s[TILE * MAXL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, F = a.F, L = a.L, P = a.T * a.V;
    const int n0 = blockIdx.x * TILE;
    const int ns = min(TILE, a.N - n0);          // samples of this tile (the last one may be ragged)

    // 1. pooled[s][c]: (t, v) in index order, then one division; rows of absent samples are zero
    for (int e = tid; e < TILE * C; e += NT) {
        const int c = e / TILE, s = e - c * TILE;
        float m = 0.f;
        if (s < ns) {
            const float* p = a.h + (long)(n0 + s) * a.h_sN + (long)c * a.h_sC;
            float acc = 0.f;
            for (int r = 0; r < P; ++r) acc += p[r];
            m = acc / (float)P;
            a.pooled[(long)(n0 + s) * C + c] = m;
        }
        pooled_s[s * C + c] = m;
    }
    __syncthreads();

    // 2. fc1 + LeakyReLU: a wave per output row (its weight row is read once, coalesced, for all samples of the tile)
    for (int f = wave; f < F; f += NW) {
        float acc[TILE];
        wave_dot_tile(a.w1 + (long)f * C, pooled_s, C, C, lane, acc);
        if (lane < TILE) {
            float v = pick(acc, lane) + a.b1[f];
            v = v > 0.f ? v : v * a.slope;
            feat_s[lane * F + f] = v;
            if (lane < ns) a.feat[(long)(n0 + lane) * F + f] = v;
        }
    }
    __syncthreads();

    // 3. fcn
    for (int l = wave; l < L; l += NW) {
        float acc[TILE];
        wave_dot_tile(a.w2 + (long)l * F, feat_s, F, F, lane, acc);
        if (lane < TILE) {
            const float v = pick(acc, lane) + a.b2[l];
            logit_s[lane * L + l] = v;
            if (lane < ns) a.logits[(long)(n0 + lane) * L + l] = v;
        }
    }
    __syncthreads();

    // 4. a wave per sample: argmax (lowest index of the largest logit; NaN never wins), log-sum-exp, loss
    if (wave < ns) {
        const int n = n0 + wave;
        const float* x = logit_s + wave * L;
        float bv = -INFINITY;
        int bi = INT_MAX;
        for (int l = lane; l < L; l += 64) {
            const float v = x[l];
            if (v > bv || (v == bv && l < bi)) { bv = v; bi = l; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        // the sequential rule starts at class 0: a NaN there is never replaced (and nothing but NaN leaves bi unset)
        const float x0 = x[0];
        if (x0 != x0 || bi == INT_MAX) bi = 0;
        if (a.labels != nullptr) {
            float se = 0.f;
            for (int l = lane; l < L; l += 64) se += expf(x[l] - bv);
            se = wave_sum(se);
            if (lane == 0) {
                const long y = a.labels[n];
                const bool ok = y >= 0 && y < (long)L;
                a.loss_per_sample[n] = ok ? (bv + logf(se)) - x[ok ? y : 0] : NAN;
            }
        }
        if (lane == 0) a.pred[n] = bi;
    }
}

// loss = (1/N) sum_n loss_per_sample[n] in fp64, sample-index order, rounded once; correct = #{pred == label}
__global__ __launch_bounds__(NT) void kg_cls_head_finish_kernel(const KgClsHeadArgs a) {
    __shared__ int cnt_s[NW];
    const int tid = threadIdx.x;
    int cnt = 0;
    for (int n = tid; n < a.N; n += NT) {
        const long y = a.labels[n];
        cnt += (y >= 0 && y < (long)a.L && (long)a.pred[n] == y) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((tid & 63) == 0) cnt_s[tid >> 6] = cnt;
    __syncthreads();
    if (tid != 0) return;
    int total = 0;
    for (int w = 0; w < NW; ++w) total += cnt_s[w];
    a.correct[0] = total;
    double s = 0.0;
    for (int n = 0; n < a.N; ++n) s += (double)a.loss_per_sample[n];
    a.loss[0] = (float)(s / (double)a.N);
}

__global__ __launch_bounds__(NT) void kg_cls_head_bwd_kernel(const KgClsHeadArgs a) {
    __shared__ float dl_s[TILE * MAXL];
    __shared__ float df_s[TILE * MAXF];
    __shared__ float dp_s[TILE * MAXC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, F = a.F, L = a.L, P = a.T * a.V;
    const int n0 = blockIdx.x * TILE;
    const int ns = min(TILE, a.N - n0);
    float* ws_dl = (float*)a.ws;
    float* ws_df = ws_dl + (long)a.N * L;

    // 1. dlogits: a wave per sample (rows of absent samples are zero)
    if (wave < ns) {
        const int n = n0 + wave;
        const float* x = a.logits + (long)n * L;
        const float g = a.gtop[0];
        const float m = wave_row_max(x, L, lane);
        float se = 0.f;
        for (int l = lane; l < L; l += 64) se += expf(x[l] - m);
        se = wave_sum(se);
        const long y = a.labels[n];
        const bool ok = y >= 0 && y < (long)L;
        for (int l = lane; l < L; l += 64) {
            const float p = expf(x[l] - m) / se;
            const float d = ok ? ((p - ((long)l == y ? 1.f : 0.f)) * g) / (float)a.N : NAN;
            dl_s[wave * L + l] = d;
            ws_dl[(long)n * L + l] = d;
        }
    } else {
        for (int l = lane; l < L; l += 64) dl_s[wave * L + l] = 0.f;
    }
    __syncthreads();

    // 2. dfeat: a thread per feature, fcn.weight read down its columns (coalesced across the threads)
    for (int f = tid; f < F; f += NT) {
        float acc[TILE];
#pragma unroll
        for (int s = 0; s < TILE; ++s) acc[s] = 0.f;
        for (int l = 0; l < L; ++l) {
            const float w = a.w2[(long)l * F + f];
#pragma unroll
            for (int s = 0; s < TILE; ++s) acc[s] = fmaf(w, dl_s[s * L + l], acc[s]);
        }
#pragma unroll
        for (int s = 0; s < TILE; ++s) {
            float d = 0.f;
            if (s < ns) {
                d = acc[s] * (a.feat[(long)(n0 + s) * F + f] > 0.f ? 1.f : a.slope);
                ws_df[(long)(n0 + s) * F + f] = d;
            }
            df_s[s * F + f] = d;
        }
    }
    __syncthreads();

    // 3. dpooled: a thread per channel, fc1.weight read down its columns
    for (int c = tid; c < C; c += NT) {
        float acc[TILE];
#pragma unroll
        for (int s = 0; s < TILE; ++s) acc[s] = 0.f;
        for (int f = 0; f < F; ++f) {
            const float w = a.w1[(long)f * C + c];
#pragma unroll
            for (int s = 0; s < TILE; ++s) acc[s] = fmaf(w, df_s[s * F + f], acc[s]);
        }
#pragma unroll
        for (int s = 0; s < TILE; ++s) dp_s[s * C + c] = acc[s];
    }
    __syncthreads();

    // 4. the trunk's top gradient of the tile's samples
    const float fp = (float)P;
    const int per_c = ns * P;
    for (int e = tid; e < C * per_c; e += NT) {
        const int c = e / per_c, rem = e - c * per_c;
        const int s = rem / P, r = rem - s * P;
        float v = dp_s[s * C + c] / fp;
        const long n = n0 + s;
        if (a.masked) v *= a.h[n * a.h_sN + (long)c * a.h_sC + r] > 0.f ? 1.f : a.slope;
        a.g[n * a.g_sN + (long)c * a.g_sC + r] = v;
    }
}

// one thread per output element: [dw1 (F C) | db1 (F) | dw2 (L F) | db2 (L)], the samples in index order
__global__ __launch_bounds__(NT) void kg_cls_head_wgrad_kernel(const KgClsHeadArgs a) {
    const int C = a.C, F = a.F, L = a.L, N = a.N;
    const float* dl = (const float*)a.ws;
    const float* df = dl + (long)N * L;
    const long n1 = (long)F * C, n2 = n1 + F, n3 = n2 + (long)L * F, n4 = n3 + L;
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    float s = 0.f;
    float* out;
    if (i < n1) {
        const int f = (int)(i / C), c = (int)(i - (long)f * C);
        for (int n = 0; n < N; ++n) s = fmaf(df[(long)n * F + f], a.pooled[(long)n * C + c], s);
        out = a.dw1 + i;
    } else if (i < n2) {
        const int f = (int)(i - n1);
        for (int n = 0; n < N; ++n) s += df[(long)n * F + f];
        out = a.db1 + f;
    } else if (i < n3) {
        const long j = i - n2;
        const int l = (int)(j / F), f = (int)(j - (long)l * F);
        for (int n = 0; n < N; ++n) s = fmaf(dl[(long)n * L + l], a.feat[(long)n * F + f], s);
        out = a.dw2 + j;
    } else {
        const int l = (int)(i - n3);
        for (int n = 0; n < N; ++n) s += dl[(long)n * L + l];
        out = a.db2 + l;
    }
    *out = (a.accumulate ? *out : 0.f) + s;
}

// dist[s, p] of the pair p (the diversity table, then the multimodality table): one wave, the lanes strided over the features
__global__ __launch_bounds__(NT) void kg_cls_dist_kernel(const KgClsScoresArgs a) {
    const int lane = threadIdx.x & 63;
    const int npairs = a.Sd + a.K * a.Sl;
    const long wp = (long)blockIdx.x * NW + (threadIdx.x >> 6);       // (wave-uniform)
    if (wp >= (long)a.nsets * npairs) return;
    const int s = (int)(wp / npairs), p = (int)(wp - (long)s * npairs);
    const int32_t* pr = p < a.Sd ? a.div_pairs + 2 * (long)p : a.mm_pairs + 2 * (long)(p - a.Sd);
    const int i = pr[0], j = pr[1];
    double d = NAN;
    if (i >= 0 && i < a.N && j >= 0 && j < a.N) {
        const float* fs = a.feat[0];
#pragma unroll
        for (int q = 1; q < KG_CLS_MAX_SETS; ++q)
            if (s == q) fs = a.feat[q];
        const float* x = fs + (long)i * a.feat_ld;
        const float* y = fs + (long)j * a.feat_ld;
        double acc = 0.0;
        for (int f = lane; f < a.F; f += 64) {
            const double t = (double)x[f] - (double)y[f];
            acc = fma(t, t, acc);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        d = sqrt(acc);
    }
    if (lane == 0) a.dist[wp] = d;
}

// set s = blockIdx.x: the integer tallies (LDS counters: integer addition does not depend on the order), then thread 0 adds
// the set's distances in index order - staged through LDS a tile at a time - and divides once per mean
__global__ __launch_bounds__(NT) void kg_cls_scores_finish_kernel(const KgClsScoresArgs a) {
    constexpr int DT = 1024;
    __shared__ int cor_s[MAXL];
    __shared__ int cnt_s[MAXL];
    __shared__ int tot_s[NW];
    __shared__ double tile_s[DT];
    const int tid = threadIdx.x, s = blockIdx.x, K = a.K, N = a.N;
    const int32_t* pred = a.pred[0];
#pragma unroll
    for (int q = 1; q < KG_CLS_MAX_SETS; ++q)
        if (s == q) pred = a.pred[q];
    for (int c = tid; c < K; c += NT) { cor_s[c] = 0; cnt_s[c] = 0; }
    __syncthreads();
    int cnt = 0;
    for (int n = tid; n < N; n += NT) {
        const long y = a.labels[n];
        if (y >= 0 && y < (long)K) {
            atomicAdd(&cnt_s[y], 1);
            if ((long)pred[n] == y) { atomicAdd(&cor_s[y], 1); ++cnt; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((tid & 63) == 0) tot_s[tid >> 6] = cnt;
    __syncthreads();
    for (int c = tid; c < K; c += NT) {
        a.correct_per_class[(long)s * K + c] = cor_s[c];
        if (s == 0) a.count_per_class[c] = cnt_s[c];
    }
    const int npairs = a.Sd + K * a.Sl;
    const double* dist = a.dist + (long)s * npairs;
    double sd = 0.0, sm = 0.0;
    for (int p0 = 0; p0 < npairs; p0 += DT) {
        const int np = min(DT, npairs - p0);
        __syncthreads();
        for (int p = tid; p < np; p += NT) tile_s[p] = dist[p0 + p];
        __syncthreads();
        if (tid == 0) {
            const int nd = max(0, min(np, a.Sd - p0));       // the tile's diversity pairs come first
#pragma unroll 8
            for (int p = 0; p < nd; ++p) sd += tile_s[p];
#pragma unroll 8
            for (int p = nd; p < np; ++p) sm += tile_s[p];
        }
    }
    if (tid != 0) return;
    int total = 0;
    for (int w = 0; w < NW; ++w) total += tot_s[w];
    a.correct[s] = total;
    const double sc[3] = {(double)total / (double)N, sd / (double)a.Sd, sm / (double)(K * a.Sl)};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        a.scores64[s * 3 + q] = sc[q];
        a.scores[s * 3 + q] = (float)sc[q];
    }
}

int validate_cls(const KgClsHeadArgs* a, const char* who) {
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->N >= 1, "%s: N=%d < 1", who, a->N);
    KG_REQUIRE(a->T >= 1 && a->V >= 1, "%s: T=%d / V=%d < 1", who, a->T, a->V);
    KG_REQUIRE(a->C >= 1 && a->C <= MAXC, "%s: C=%d outside [1, %d]", who, a->C, MAXC);
    KG_REQUIRE(a->F >= 1 && a->F <= MAXF, "%s: F=%d outside [1, %d]", who, a->F, MAXF);
    KG_REQUIRE(a->L >= 1 && a->L <= MAXL, "%s: L=%d outside [1, %d]", who, a->L, MAXL);
    KG_REQUIRE((long)a->N * a->C * a->T * a->V < (1L << 31) && (long)a->N * a->L < (1L << 31), "%s: too large", who);
    return 0;
}

int64_t cls_ws_bytes(const KgClsHeadArgs* a) { return 4 * (int64_t)a->N * ((int64_t)a->L + a->F); }

}  // namespace

extern "C" int64_t kg_cls_head_workspace_bytes(const KgClsHeadArgs* a) {
    if (int rc = validate_cls(a, "kg_cls_head_workspace_bytes")) return rc;
    return cls_ws_bytes(a);
}

extern "C" int kg_cls_head_fwd(const KgClsHeadArgs* a, void* stream) {
    if (int rc = validate_cls(a, "kg_cls_head_fwd")) return rc;
    KG_REQUIRE(a->h && a->w1 && a->b1 && a->w2 && a->b2, "kg_cls_head_fwd: null operand");
    KG_REQUIRE(a->pooled && a->feat && a->logits && a->pred, "kg_cls_head_fwd: null output");
    KG_REQUIRE(!a->labels || (a->loss_per_sample && a->loss && a->correct), "kg_cls_head_fwd: labels without loss outputs");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kg_cls_head_fwd_kernel, dim3(kg_cdiv(a->N, TILE)), dim3(NT), 0, s, *a);
    if (int rc = kg_launch_status("kg_cls_head_fwd")) return rc;
    if (!a->labels) return 0;
    hipLaunchKernelGGL(kg_cls_head_finish_kernel, dim3(1), dim3(NT), 0, s, *a);
    return kg_launch_status("kg_cls_head_fwd (finish)");
}

extern "C" int kg_cls_head_bwd(const KgClsHeadArgs* a, void* stream) {
    if (int rc = validate_cls(a, "kg_cls_head_bwd")) return rc;
    KG_REQUIRE(a->w1 && a->w2 && a->labels && a->feat && a->logits && a->gtop && (!a->masked || a->h),
               "kg_cls_head_bwd: null operand");
    KG_REQUIRE(a->g, "kg_cls_head_bwd: null output");
    KG_REQUIRE(a->ws && a->ws_bytes >= cls_ws_bytes(a), "kg_cls_head_bwd: ws_bytes=%lld < %lld (kg_cls_head_workspace_bytes)",
               (long long)(a->ws ? a->ws_bytes : 0), (long long)cls_ws_bytes(a));
    hipLaunchKernelGGL(kg_cls_head_bwd_kernel, dim3(kg_cdiv(a->N, TILE)), dim3(NT), 0, (hipStream_t)stream, *a);
    return kg_launch_status("kg_cls_head_bwd");
}

extern "C" int kg_cls_head_wgrad(const KgClsHeadArgs* a, void* stream) {
    if (int rc = validate_cls(a, "kg_cls_head_wgrad")) return rc;
    KG_REQUIRE(a->pooled && a->feat, "kg_cls_head_wgrad: null operand");
    KG_REQUIRE(a->dw1 && a->db1 && a->dw2 && a->db2, "kg_cls_head_wgrad: null output");
    KG_REQUIRE(a->ws && a->ws_bytes >= cls_ws_bytes(a), "kg_cls_head_wgrad: ws_bytes=%lld < %lld (kg_cls_head_workspace_bytes)",
               (long long)(a->ws ? a->ws_bytes : 0), (long long)cls_ws_bytes(a));
    const long total = (long)a->F * a->C + a->F + (long)a->L * a->F + a->L;
    hipLaunchKernelGGL(kg_cls_head_wgrad_kernel, dim3(kg_cdiv(total, NT)), dim3(NT), 0, (hipStream_t)stream, *a);
    return kg_launch_status("kg_cls_head_wgrad");
}

extern "C" int kg_cls_scores(const KgClsScoresArgs* a, void* stream) {
    const char* who = "kg_cls_scores";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->nsets >= 1 && a->nsets <= KG_CLS_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, a->nsets, KG_CLS_MAX_SETS);
    KG_REQUIRE(a->N >= 1, "%s: N=%d < 1", who, a->N);
    KG_REQUIRE(a->F >= 1 && a->F <= MAXF, "%s: F=%d outside [1, %d]", who, a->F, MAXF);
    KG_REQUIRE(a->K >= 1 && a->K <= MAXL, "%s: K=%d outside [1, %d]", who, a->K, MAXL);
    KG_REQUIRE(a->Sd >= 1 && a->Sl >= 1, "%s: Sd=%d / Sl=%d < 1", who, a->Sd, a->Sl);
    KG_REQUIRE(a->feat_ld >= a->F, "%s: feat_ld=%lld < F=%d", who, (long long)a->feat_ld, a->F);
    const long npairs = (long)a->Sd + (long)a->K * a->Sl;
    KG_REQUIRE((long)a->K * a->Sl < (1L << 31) && (long)a->nsets * npairs < (1L << 31), "%s: too many pairs", who);
    for (int s = 0; s < a->nsets; ++s) KG_REQUIRE(a->feat[s] && a->pred[s], "%s: null operand (set %d)", who, s);
    KG_REQUIRE(a->labels && a->div_pairs && a->mm_pairs, "%s: null operand", who);
    KG_REQUIRE(a->dist && a->scores64 && a->scores && a->correct && a->correct_per_class && a->count_per_class,
               "%s: null output", who);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kg_cls_dist_kernel, dim3(kg_cdiv((long)a->nsets * npairs, NW)), dim3(NT), 0, st, *a);
    if (int rc = kg_launch_status("kg_cls_scores (dist)")) return rc;
    hipLaunchKernelGGL(kg_cls_scores_finish_kernel, dim3(a->nsets), dim3(NT), 0, st, *a);
    return kg_launch_status("kg_cls_scores");
}
