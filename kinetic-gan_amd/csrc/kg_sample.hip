// Small launches of the inference-only generation path (include/kgan_hip.h; sample.Sampler):
//   kg_bn_eval_coef : eval-mode BatchNorm coefficients of all layers of the generator in one launch
//   kg_trunc_lerp   : the truncation trick - column means of the truncation draws, then the pull towards them, in place
// Both read everything through pointers when they run, so a captured graph that holds them follows in-place updates of
// the parameters and running statistics (kg_adam_step, kg_bn_fwd_many, training replays) without a rebuild.
#include "kg_common.h"

namespace {

struct BnEvalJobs {
    KgBnEvalJob j[KG_BN_EVAL_MAX_JOBS];
};

// grid (ceil(max C / 256), njobs): thread = channel
__global__ __launch_bounds__(256) void kg_bn_eval_coef_kernel(const BnEvalJobs jobs) {
    const KgBnEvalJob& j = jobs.j[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= j.C) return;
    const float mean = j.running_mean[c];
    const float rstd = 1.f / sqrtf(j.running_var[c] + j.eps);
    const float scale = (j.gamma ? j.gamma[c] : 1.f) * rstd;
    const float shift = (j.beta ? j.beta[c] : 0.f) - mean * scale;
    j.coef[0 * j.C + c] = scale;
    j.coef[1 * j.C + c] = shift;
    j.coef[2 * j.C + c] = mean;
    j.coef[3 * j.C + c] = rstd;
}

// A workgroup owns TL_COLS consecutive columns.  Thread (sub, col) adds rows sub, sub + TL_SUBS, ... of its column in
// order (a wave reads one 256-byte run per row: coalesced), the TL_SUBS partial sums of a column are added in order by
// its sub-0 thread, and every thread then walks the rows of x the same way.  Nothing depends on the grid.
constexpr int TL_COLS = 64, TL_SUBS = 16, TL_NT = TL_COLS * TL_SUBS;

__global__ __launch_bounds__(TL_NT) void kg_trunc_lerp_kernel(float* x, long x_ld, int N, int D, const float* t, long t_ld, int M,
                                                              float truncation) {
    __shared__ float part[TL_SUBS][TL_COLS];
    __shared__ float mean[TL_COLS];
    const int col = threadIdx.x & (TL_COLS - 1), sub = threadIdx.x / TL_COLS;
    const int d = blockIdx.x * TL_COLS + col;
    const bool live = d < D;
    float s = 0.f;
    if (live) {
#pragma unroll 8
        for (int i = sub; i < M; i += TL_SUBS) s += t[(long)i * t_ld + d];
    }
    part[sub][col] = s;
    __syncthreads();
    if (sub == 0) {
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < TL_SUBS; ++k) tot += part[k][col];
        mean[col] = tot / (float)M;
    }
    __syncthreads();
    if (!live) return;
    const float m = mean[col];
#pragma unroll 4
    for (int n = sub; n < N; n += TL_SUBS) {
        float* p = x + (long)n * x_ld + d;
        *p = m + truncation * (*p - m);
    }
}

}  // namespace

extern "C" int kg_bn_eval_coef(const KgBnEvalJob* jobs, int32_t njobs, void* stream) {
    KG_REQUIRE(jobs != nullptr, "kg_bn_eval_coef: null jobs");
    KG_REQUIRE(njobs >= 1 && njobs <= KG_BN_EVAL_MAX_JOBS, "kg_bn_eval_coef: njobs=%d outside [1, %d]", njobs, KG_BN_EVAL_MAX_JOBS);
    BnEvalJobs b = {};
    int maxc = 0;
    for (int i = 0; i < njobs; ++i) {
        const KgBnEvalJob& j = jobs[i];
        KG_REQUIRE(j.C >= 1, "kg_bn_eval_coef: job %d: C=%d < 1", i, j.C);
        KG_REQUIRE(j.running_mean != nullptr && j.running_var != nullptr, "kg_bn_eval_coef: job %d: null running statistics", i);
        KG_REQUIRE(j.coef != nullptr, "kg_bn_eval_coef: job %d: null coef", i);
        KG_REQUIRE(j.eps >= 0.f, "kg_bn_eval_coef: job %d: eps=%g < 0", i, (double)j.eps);
        b.j[i] = j;
        maxc = j.C > maxc ? j.C : maxc;
    }
    hipLaunchKernelGGL(kg_bn_eval_coef_kernel, dim3(kg_cdiv(maxc, 256), njobs), dim3(256), 0, (hipStream_t)stream, b);
    return kg_launch_status("kg_bn_eval_coef");
}

extern "C" int kg_trunc_lerp(float* x, int64_t x_ld, int32_t N, int32_t D, const float* t, int64_t t_ld, int32_t M, float truncation,
                             void* stream) {
    KG_REQUIRE(x != nullptr && t != nullptr, "kg_trunc_lerp: null x / t");
    KG_REQUIRE(N >= 1 && D >= 1 && M >= 1, "kg_trunc_lerp: N=%d D=%d M=%d", N, D, M);
    KG_REQUIRE(x_ld >= D && t_ld >= D, "kg_trunc_lerp: x_ld=%lld / t_ld=%lld shorter than D=%d", (long long)x_ld, (long long)t_ld, D);
    hipLaunchKernelGGL(kg_trunc_lerp_kernel, dim3(kg_cdiv(D, TL_COLS)), dim3(TL_NT), 0, (hipStream_t)stream, x, (long)x_ld, N, D, t,
                       (long)t_ld, M, truncation);
    return kg_launch_status("kg_trunc_lerp");
}
