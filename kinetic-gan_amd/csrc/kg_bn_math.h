// The BatchNorm finish arithmetic of the statistics kernels (kg_misc.hip, kg_gen.hip, kg_genblock.hip), written once: the
// kernels differ in how they reduce, not in what the finishing lane computes.  Expression order is part of the contract -
// the results of the single-launch, many-job and fused-block forms are compared bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// forward: coef rows (scale, shift, mean, rstd) of channel c from the mean and the BIASED variance; returns rstd
// (gamma / beta: the values, 1 / 0 for a layer without affine parameters)
__device__ __forceinline__ float kg_bn_fwd_coef(float* coef, int C, int c, float mean, float var, float gamma, float beta, float eps) {
    const float rstd = 1.f / sqrtf(var + eps);
    const float scale = gamma * rstd;
    const float shift = beta - mean * scale;
    coef[0 * C + c] = scale;
    coef[1 * C + c] = shift;
    coef[2 * C + c] = mean;
    coef[3 * C + c] = rstd;
    return rstd;
}

// running statistics take one batch of n elements (biased variance in, unbiased variance averaged); n: long or float
template <typename N>
__device__ __forceinline__ void kg_bn_running_update(float& running_mean, float& running_var, float momentum, float mean, float var, N n) {
    const float unb = var * ((float)n / (float)(n > 1 ? n - 1 : 1));
    running_mean = (1.f - momentum) * running_mean + momentum * mean;
    running_var = (1.f - momentum) * running_var + momentum * unb;
}

// Chan et al.: (n_tot, mean, M2) takes a chunk of nb elements with mean mk and centred sum of squares qk
__device__ __forceinline__ void kg_chan_merge(float& n_tot, float& mean, float& M2, float nb, float mk, float qk) {
    const float n_new = n_tot + nb;
    const float delta = mk - mean;
    mean += delta * (nb / n_new);
    M2 += qk + delta * delta * (n_tot * nb / n_new);
    n_tot = n_new;
}

// backward: dx = a g + b x + c from s_g = sum g and s_x = sum g (x - mean); coef rows (a, b, c, sum g xhat, sum g)
__device__ __forceinline__ void kg_bn_bwd_coef(float* coef, int C, int c, float s_g, float s_x, float mean, float rstd, float gamma, bool training, float n) {
    const float q = s_x * rstd;                                  // sum g * xhat
    const float ga = gamma * rstd;
    float b = 0.f, cc = 0.f;
    if (training) {
        b = -ga * rstd * q / n;
        cc = -ga * s_g / n - b * mean;
    }
    coef[0 * C + c] = ga;
    coef[1 * C + c] = b;
    coef[2 * C + c] = cc;
    coef[3 * C + c] = q;
    coef[4 * C + c] = s_g;
}

// The tail of a generator block, out = act(BN_t(u) + BN_r(r) + w_noise * noise), backward, ONE BatchNorm branch: from the
// channel's sums s_g = sum gp and s_x = sum gp (x - mean) the coefficients of d/dx = a gp + b x + c (a branch without BatchNorm
// keeps the caller's (1, 0, 0)), the parameter gradients ADDED into the buffers that are given.  Called inside the caller's
// `if (branch has a BatchNorm)`, with the kernel's argument fields as operands: kg_genblock_bwd has no scalar register to
// spare, and every form that took both branches, the noise add and the six coefficient stores in one call moved its scalar
// allocation and cost its G3 / G4 launches 0.3-0.5 us (profiles/lastarriver_refactor_resources.log).
__device__ __forceinline__ void kg_tail_bwd_branch(float& a, float& b, float& cc, int c, float s_g, float s_x, float inv_n, const float* rstd_p,
                                                   const float* mean_p, const float* gamma, float* dgamma, float* dbeta) {
    const float rstd = rstd_p[c], q = s_x * rstd, mean = mean_p[c];
    a = (gamma ? gamma[c] : 1.f) * rstd;
    b = -a * rstd * q * inv_n;
    cc = -a * s_g * inv_n - b * mean;
    if (dgamma) dgamma[c] += q;
    if (dbeta) dbeta[c] += s_g;
}
