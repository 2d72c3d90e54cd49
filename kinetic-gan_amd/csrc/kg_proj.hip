// Projection into W (see include/kgan_hip.h): the tail of one iteration of project.Projector behind the
// generator's forward and backward pass, as two launches.
//
// kg_proj_loss_kernel: one workgroup = one sample.  The frames go through the strides into LDS in chunks of KP_F frames with one
// halo frame in front and one behind (x and y' as fp32 [c][frame][v], the weights as [frame][v]; a halo frame outside [0, T)
// is staged as zeros with weight 0, which switches its terms off), so LDS puts no cap on T.  Pass 1 walks the chunks and adds,
// per thread and in fp64, the three weighted sums and their three weight sums: bones as items (frame, bone) = tid, tid + 256,
// .., joints as plane positions (frame, v) = tid, tid + 256, .. with the channels innermost; then a shuffle tree and the four
// waves as (0 + 1) + (2 + 3).  Thread 0 forms the four loss words and the three gradient coefficients.  Pass 2 walks the
// chunks again (with one chunk the staged data of pass 1 is still there) and stores gx: the position term, the two velocity
// neighbours and, bone by bone in table order, the bones that end at the joint.  Every sum's shape depends on (C, T, V, B)
// alone.  A weight that is not > 0 selects its term away.
// The bone table travels in the kernel arguments and is moved into LDS with constant indices only (a lane-indexed read of an
// argument array would put the whole struct into scratch).
//
// kg_proj_step_kernel: one workgroup = one sample.  The prior's sum: a thread adds its elements d = tid, tid + 256, .. in order,
// shuffle tree, four waves in order; the same pass looks for a non-finite gradient word (__syncthreads_or).  The objective, the
// best-so-far record and the schedule are uniform over the workgroup; the Adam update is element-wise.  fp64 inside.
// No atomics; no scratch; no dynamically indexed private array.
#include <math.h>

#include "kg_common.h"

namespace {

constexpr int KP_NT = 256;                      // threads of a workgroup (both kernels)
constexpr int KP_F = KG_PROJ_CHUNK_FRAMES;
constexpr int KP_MAXC = KG_PROJ_MAX_CHANNELS, KP_MAXV = KG_PROJ_MAX_JOINTS, KP_MAXB = KG_KIN_MAX_BONES;
constexpr int KP_PLANE = (KP_F + 2) * KP_MAXV;  // floats of one staged plane: the chunk and its two halo frames
constexpr int KP_SUMS = 6;                      // pos, vel, bone, then their weight sums
static_assert(2 * KP_MAXB <= KP_NT, "kg_proj_loss: one thread per table entry");
static_assert(8 * KP_F * KP_MAXB + 8 * (KP_NT / 64) * KP_SUMS + 4 * (2 * KP_MAXC + 1) * KP_PLANE + 4 * 2 * KP_MAXB + 64 <= 64 * 1024,
              "kg_proj_loss: static LDS of a workgroup");

struct ProjLossDev {
    const float* x;  long x_sn, x_sc, x_st;
    const float* y;  long y_sn, y_sc, y_st;
    const float* m;  long sm;
    float scale, shift;
    int n, C, T, V, B;
    double lp, lv, lb;
    float* loss;  float* gx;
    FastDiv divV, divB;
    int bones[2 * KP_MAXB];
};

__device__ __forceinline__ bool kp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// Separately rounded operations (__fmul_rn and its kin are plain operators in HIP's headers, and hipcc contracts a product and
// a sum into one FMA by default): contraction is switched off inside these helpers.
// y' = fp32(fp32(y * scale) + shift): what two stock launches compute
__device__ __forceinline__ float kp_target(float y, float scale, float shift) {
#pragma clang fp contract(off)
    const float p = y * scale;
    return p + shift;
}
// (a x + b y) + c z, every product and sum rounded once
__device__ __forceinline__ double kp_weighted3(double a, double x, double b, double y, double c, double z) {
#pragma clang fp contract(off)
    const double p = a * x, q = b * y, r = c * z;
    const double s = p + q;
    return s + r;
}
// x + a y, product and sum rounded once
__device__ __forceinline__ double kp_axpy(double x, double a, double y) {
#pragma clang fp contract(off)
    const double p = a * y;
    return x + p;
}
__device__ __forceinline__ float kp_diff(float x, float y) {
#pragma clang fp contract(off)
    return x - y;
}

__global__ __launch_bounds__(KP_NT) void kg_proj_loss_kernel(const ProjLossDev a) {
    __shared__ double bd[KP_F * KP_MAXB];       // mb (s_x - s_y) of the chunk's (frame, bone); 0 where mb is off
    __shared__ double red[KP_NT / 64][KP_SUMS];
    __shared__ double coef[4];
    __shared__ float xs[2][KP_MAXC][KP_PLANE];  // [0]: x, [1]: y'
    __shared__ float ms[KP_PLANE];
    __shared__ int tab[2 * KP_MAXB];
    const int tid = threadIdx.x;
    const int T = a.T, C = a.C, V = a.V, B = a.B;
    const long smp = (long)blockIdx.x;
    const float* xp = a.x + smp * a.x_sn;
    const float* yp = a.y + smp * a.y_sn;
    const float* mp = a.m != nullptr ? a.m + smp * a.sm : nullptr;
    const int nchunks = (T + KP_F - 1) / KP_F;

    // table -> LDS (constant indices into the arguments)
    {
        int v = 0;
#pragma unroll
        for (int i = 0; i < 2 * KP_MAXB; ++i) v = tid == i ? a.bones[i] : v;
        if (tid < 2 * KP_MAXB) tab[tid] = v;
    }

    // frames t0 - 1 .. t0 + Fc of x, y' and m -> LDS rows 0 .. Fc + 1; the barrier in front protects the previous chunk's readers
    auto stage = [&](int t0, int Fc) {
        __syncthreads();
        const int cnt = (Fc + 2) * V;
        for (int q = tid; q < cnt; q += KP_NT) {
            unsigned j, v;
            a.divV.divmod((unsigned)q, j, v);
            const int t = t0 - 1 + (int)j;
            const bool in = t >= 0 && t < T;
            ms[q] = in ? (mp != nullptr ? mp[(long)t * V + v] : 1.f) : 0.f;
#pragma unroll
            for (int c = 0; c < KP_MAXC; ++c) {
                if (c < C) {
                    float xv = 0.f, yv = 0.f;
                    if (in) {
                        xv = xp[(long)t * a.x_st + (long)c * a.x_sc + v];
                        yv = kp_target(yp[(long)t * a.y_st + (long)c * a.y_sc + v], a.scale, a.shift);
                    }
                    xs[0][c][q] = xv;
                    xs[1][c][q] = yv;
                }
            }
        }
        __syncthreads();
    };

    // bd of the chunk; the weighted sum of squares and the weight sum go to sB / wB
    auto bones_of_chunk = [&](int Fc, double& sB, double& wB) {
        const int items = Fc * B;
        for (int i = tid; i < items; i += KP_NT) {
            unsigned f, b;
            a.divB.divmod((unsigned)i, f, b);
            const int qa = ((int)f + 1) * V + tab[2 * b], qc = ((int)f + 1) * V + tab[2 * b + 1];
            const float ma = ms[qa], mc = ms[qc];
            double w = 0.0;
            if (ma > 0.f && mc > 0.f) {
                const double mb = (double)ma * (double)mc;
                double sx = 0.0, sy = 0.0;
#pragma unroll
                for (int c = 0; c < KP_MAXC; ++c) {
                    if (c < C) {
                        const double ex = (double)xs[0][c][qa] - (double)xs[0][c][qc];
                        const double ey = (double)xs[1][c][qa] - (double)xs[1][c][qc];
                        sx += ex * ex;
                        sy += ey * ey;
                    }
                }
                const double df = sx - sy;
                w = mb * df;
                sB += w * df;
                wB += mb;
            }
            bd[i] = w;
        }
    };

    // ---- pass 1: the sums ----
    double sP = 0.0, sV = 0.0, sB = 0.0, wP = 0.0, wV = 0.0, wB = 0.0;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int t0 = ch * KP_F, Fc = min(KP_F, T - t0);
        stage(t0, Fc);
        bones_of_chunk(Fc, sB, wB);
        const int cnt = Fc * V;
        for (int p = tid; p < cnt; p += KP_NT) {
            const int q = p + V;
            const float m1 = ms[q], m2 = ms[q + V];
            const bool on1 = m1 > 0.f, on2 = on1 && m2 > 0.f;
            const double mv = on2 ? (double)m1 * (double)m2 : 0.0;
            if (on1) wP += (double)m1;
            if (on2) wV += mv;
#pragma unroll
            for (int c = 0; c < KP_MAXC; ++c) {
                if (c < C && on1) {
                    const double d0 = (double)kp_diff(xs[0][c][q], xs[1][c][q]);
                    sP += (double)m1 * d0 * d0;
                    if (on2) {
                        const double e = (double)kp_diff(xs[0][c][q + V], xs[1][c][q + V]) - d0;
                        sV += mv * e * e;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sP += __shfl_xor(sP, off, 64);
        sV += __shfl_xor(sV, off, 64);
        sB += __shfl_xor(sB, off, 64);
        wP += __shfl_xor(wP, off, 64);
        wV += __shfl_xor(wV, off, 64);
        wB += __shfl_xor(wB, off, 64);
    }
    if ((tid & 63) == 0) {
        double* r = red[tid >> 6];
        r[0] = sP;  r[1] = sV;  r[2] = sB;  r[3] = wP;  r[4] = wV;  r[5] = wB;
    }
    __syncthreads();
    if (tid == 0) {
        double r[KP_SUMS];
#pragma unroll
        for (int k = 0; k < KP_SUMS; ++k) r[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        const double Wp = (double)C * r[3], Wv = (double)C * r[4], Wb = r[5];
        const bool onp = a.lp > 0.0 && Wp > 0.0, onv = a.lv > 0.0 && Wv > 0.0, onb = a.lb > 0.0 && Wb > 0.0;
        const double Lp = onp ? r[0] / Wp : 0.0, Lv = onv ? r[1] / Wv : 0.0, Lb = onb ? r[2] / Wb : 0.0;
        const double L = kp_weighted3(a.lp, Lp, a.lv, Lv, a.lb, Lb);
        float* o = a.loss + smp * 4;
        o[0] = (float)L;
        o[1] = (float)Lp;
        o[2] = (float)Lv;
        o[3] = (float)Lb;
        coef[0] = onp ? 2.0 * a.lp / Wp : 0.0;
        coef[1] = onv ? 2.0 * a.lv / Wv : 0.0;
        coef[2] = onb ? 4.0 * a.lb / Wb : 0.0;
    }
    __syncthreads();
    const double cp = coef[0], cv = coef[1], cb = coef[2];

    // ---- pass 2: the gradient ----
    float* gp = a.gx + smp * ((long)C * T * V);
    const long TV = (long)T * V;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int t0 = ch * KP_F, Fc = min(KP_F, T - t0);
        if (nchunks > 1) {
            double s_ = 0.0, w_ = 0.0;
            stage(t0, Fc);
            bones_of_chunk(Fc, s_, w_);
            __syncthreads();
        }
        const int cnt = Fc * V;
        for (int p = tid; p < cnt; p += KP_NT) {
            const int q = p + V;
            unsigned f, v;
            a.divV.divmod((unsigned)p, f, v);
            const float m0 = ms[q - V], m1 = ms[q], m2 = ms[q + V];
            const bool on1 = m1 > 0.f, onA = on1 && m0 > 0.f, onB = on1 && m2 > 0.f;
            double g[KP_MAXC] = {0.0, 0.0, 0.0};
            if (on1) {
#pragma unroll
                for (int c = 0; c < KP_MAXC; ++c) {
                    if (c < C) {
                        const double d1 = (double)kp_diff(xs[0][c][q], xs[1][c][q]);
                        double acc = 0.0;
                        if (cp != 0.0) acc = cp * ((double)m1 * d1);
                        if (cv != 0.0) {
                            if (onA) acc += cv * (((double)m0 * (double)m1) * (d1 - (double)kp_diff(xs[0][c][q - V], xs[1][c][q - V])));
                            if (onB) acc -= cv * (((double)m1 * (double)m2) * ((double)kp_diff(xs[0][c][q + V], xs[1][c][q + V]) - d1));
                        }
                        g[c] = acc;
                    }
                }
                if (cb != 0.0) {
                    const int row = ((int)f + 1) * V;
                    for (int b = 0; b < B; ++b) {
                        const int ja = tab[2 * b], jc = tab[2 * b + 1];
                        if ((ja == (int)v) != (jc == (int)v)) {
                            const double w = (ja == (int)v ? cb : -cb) * bd[(int)f * B + b];
#pragma unroll
                            for (int c = 0; c < KP_MAXC; ++c)
                                if (c < C) g[c] += w * ((double)xs[0][c][row + ja] - (double)xs[0][c][row + jc]);
                        }
                    }
                }
            }
            const long at = (long)(t0 + (int)f) * V + v;
#pragma unroll
            for (int c = 0; c < KP_MAXC; ++c)
                if (c < C) gp[c * TV + at] = (float)g[c];
        }
    }
}

__global__ __launch_bounds__(KP_NT) void kg_proj_step_kernel(const KgProjStepArgs a) {
    __shared__ double red[KP_NT / 64];
    const int tid = threadIdx.x, D = a.D, i = (int)blockIdx.x;
    const long base = (long)i * D;
    const int s = *a.step;
    const long lab = (long)a.labels[i];
    const bool lab_ok = lab >= 0 && lab < (long)a.K;
    const float* wm = a.wmean + (lab_ok ? lab : 0) * (long)D;
    const float best = a.best_obj[i];
    const float L32 = a.loss[4 * (long)i];
    const bool prior_on = a.lambda_w > 0.0;

    double acc = 0.0;
    int bad = 0;
    for (int d = tid; d < D; d += KP_NT) {
        bad |= kp_finite(a.gw[base + d]) ? 0 : 1;
        if (prior_on) {
            const double e = (double)a.w[base + d] - (double)wm[d];
            acc += e * e;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    const int any_bad = __syncthreads_or(bad);  // (a barrier: red is visible, and every thread has read best_obj[i])
    const double prior = prior_on ? ((red[0] + red[1]) + (red[2] + red[3])) / (double)D : 0.0;
    const float obj = prior_on ? (float)kp_axpy((double)L32, a.lambda_w, prior) : L32;
    const bool ok = lab_ok && kp_finite(obj) && any_bad == 0;
    if (tid == 0 && a.hist != nullptr && s >= 1 && s <= a.S) a.hist[(long)(s - 1) * a.n + i] = obj;
    if (!ok) {                                  // (uniform) frozen: nothing but the count moves
        if (tid == 0) a.nonfinite[i] += 1;
        return;
    }
    const bool better = obj < best;
    if (better && tid == 0) {
        a.best_obj[i] = obj;
#pragma unroll
        for (int k = 0; k < 4; ++k) a.best_loss[4 * (long)i + k] = a.loss[4 * (long)i + k];
    }
    // the schedule
    const double sd = (double)s;
    double lr = a.lr;
    if (a.ramp_up > 0) lr = lr * fmin(1.0, sd / (double)a.ramp_up);
    if (a.ramp_down > 0 && s > a.S - a.ramp_down)
        lr = lr * (0.5 * (1.0 + cos(M_PI * ((sd - (double)(a.S - a.ramp_down)) / (double)a.ramp_down))));
    const double sc = (double)(s < 1 ? 1 : s);
    const double c1 = 1.0 - pow(a.b1, sc), c2 = 1.0 - pow(a.b2, sc);
    const double pg = prior_on ? 2.0 * a.lambda_w / (double)D : 0.0;
    for (int d = tid; d < D; d += KP_NT) {
        const float w0 = a.w[base + d];
        if (better) a.best_w[base + d] = w0;
        double g = (double)a.gw[base + d];
        if (prior_on) g += pg * ((double)w0 - (double)wm[d]);
        const double m1 = a.b1 * (double)a.am[base + d] + (1.0 - a.b1) * g;
        const double v1 = a.b2 * (double)a.av[base + d] + (1.0 - a.b2) * (g * g);
        const double up = (m1 / c1) / (sqrt(v1 / c2) + a.eps);
        a.am[base + d] = (float)m1;
        a.av[base + d] = (float)v1;
        a.w[base + d] = (float)((double)w0 - lr * up);
    }
}

bool kp_num(double v) { return isfinite(v) && v >= 0.0; }

}  // namespace

extern "C" int kg_proj_loss(const KgProjLossArgs* a, void* stream) {
    const char* who = "kg_proj_loss";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->x != nullptr, "%s: null pointer x", who);
    KG_REQUIRE(a->y != nullptr, "%s: null pointer y", who);
    KG_REQUIRE(a->loss != nullptr, "%s: null pointer loss", who);
    KG_REQUIRE(a->gx != nullptr, "%s: null pointer gx", who);
    KG_REQUIRE(a->n >= 1, "%s: n=%d < 1", who, a->n);
    KG_REQUIRE(a->C >= 1 && a->C <= KG_PROJ_MAX_CHANNELS, "%s: C=%d outside [1, %d]", who, a->C, KG_PROJ_MAX_CHANNELS);
    KG_REQUIRE(a->T >= 1, "%s: T=%d < 1", who, a->T);
    KG_REQUIRE(a->V >= 1 && a->V <= KG_PROJ_MAX_JOINTS, "%s: V=%d outside [1, %d]", who, a->V, KG_PROJ_MAX_JOINTS);
    KG_REQUIRE((long)a->T * a->V < (1L << 31), "%s: T * V = %ld, at most 2^31 - 1", who, (long)a->T * a->V);
    KG_REQUIRE(a->B >= 0 && a->B <= KG_KIN_MAX_BONES, "%s: B=%d outside [0, %d]", who, a->B, KG_KIN_MAX_BONES);
    KG_REQUIRE(a->B == 0 || a->bones != nullptr, "%s: null pointer bones with B=%d", who, a->B);
    for (int b = 0; b < 2 * a->B; ++b)
        KG_REQUIRE(a->bones[b] >= 0 && a->bones[b] < a->V, "%s: bones[%d][%d]=%d outside [0, V=%d)", who, b / 2, b % 2, a->bones[b], a->V);
    KG_REQUIRE(a->x_sn >= 0 && a->x_sc >= 0 && a->x_st >= 0, "%s: negative stride of x (x_sn, x_sc, x_st)", who);
    KG_REQUIRE(a->y_sn >= 0 && a->y_sc >= 0 && a->y_st >= 0, "%s: negative stride of y (y_sn, y_sc, y_st)", who);
    KG_REQUIRE(a->sm >= 0, "%s: negative stride sm=%lld", who, (long long)a->sm);
    KG_REQUIRE(kp_num(a->lambda_pos), "%s: lambda_pos=%g is not a finite number >= 0", who, a->lambda_pos);
    KG_REQUIRE(kp_num(a->lambda_vel), "%s: lambda_vel=%g is not a finite number >= 0", who, a->lambda_vel);
    KG_REQUIRE(kp_num(a->lambda_bone), "%s: lambda_bone=%g is not a finite number >= 0", who, a->lambda_bone);
    KG_REQUIRE(isfinite(a->scale) && isfinite(a->shift), "%s: scale=%g / shift=%g is not finite", who, (double)a->scale, (double)a->shift);
    ProjLossDev d = {};
    d.x = a->x;  d.x_sn = a->x_sn;  d.x_sc = a->x_sc;  d.x_st = a->x_st;
    d.y = a->y;  d.y_sn = a->y_sn;  d.y_sc = a->y_sc;  d.y_st = a->y_st;
    d.m = a->m;  d.sm = a->sm;  d.scale = a->scale;  d.shift = a->shift;
    d.n = a->n;  d.C = a->C;  d.T = a->T;  d.V = a->V;  d.B = a->B;
    d.lp = a->lambda_pos;  d.lv = a->lambda_vel;  d.lb = a->lambda_bone;
    d.loss = a->loss;  d.gx = a->gx;
    d.divV = FastDiv::make((unsigned)a->V);
    d.divB = FastDiv::make((unsigned)(a->B > 0 ? a->B : 1));
    for (int b = 0; b < 2 * a->B; ++b) d.bones[b] = a->bones[b];
    hipLaunchKernelGGL(kg_proj_loss_kernel, dim3(a->n), dim3(KP_NT), 0, (hipStream_t)stream, d);
    return kg_launch_status(who);
}

extern "C" int kg_proj_step(const KgProjStepArgs* a, void* stream) {
    const char* who = "kg_proj_step";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->w != nullptr, "%s: null pointer w", who);
    KG_REQUIRE(a->am != nullptr, "%s: null pointer am", who);
    KG_REQUIRE(a->av != nullptr, "%s: null pointer av", who);
    KG_REQUIRE(a->gw != nullptr, "%s: null pointer gw", who);
    KG_REQUIRE(a->wmean != nullptr, "%s: null pointer wmean", who);
    KG_REQUIRE(a->labels != nullptr, "%s: null pointer labels", who);
    KG_REQUIRE(a->loss != nullptr, "%s: null pointer loss", who);
    KG_REQUIRE(a->step != nullptr, "%s: null pointer step", who);
    KG_REQUIRE(a->best_obj != nullptr, "%s: null pointer best_obj", who);
    KG_REQUIRE(a->best_loss != nullptr, "%s: null pointer best_loss", who);
    KG_REQUIRE(a->best_w != nullptr, "%s: null pointer best_w", who);
    KG_REQUIRE(a->nonfinite != nullptr, "%s: null pointer nonfinite", who);
    KG_REQUIRE(a->n >= 1, "%s: n=%d < 1", who, a->n);
    KG_REQUIRE(a->D >= 1, "%s: D=%d < 1", who, a->D);
    KG_REQUIRE(a->K >= 1, "%s: K=%d < 1", who, a->K);
    KG_REQUIRE(a->S >= 1, "%s: S=%d < 1", who, a->S);
    KG_REQUIRE(a->ramp_up >= 0 && a->ramp_up <= a->S, "%s: ramp_up=%d outside [0, S=%d]", who, a->ramp_up, a->S);
    KG_REQUIRE(a->ramp_down >= 0 && a->ramp_down <= a->S, "%s: ramp_down=%d outside [0, S=%d]", who, a->ramp_down, a->S);
    KG_REQUIRE(kp_num(a->lambda_w), "%s: lambda_w=%g is not a finite number >= 0", who, a->lambda_w);
    KG_REQUIRE(kp_num(a->lr), "%s: lr=%g is not a finite number >= 0", who, a->lr);
    KG_REQUIRE(a->b1 >= 0.0 && a->b1 < 1.0, "%s: b1=%g outside [0, 1)", who, a->b1);
    KG_REQUIRE(a->b2 >= 0.0 && a->b2 < 1.0, "%s: b2=%g outside [0, 1)", who, a->b2);
    KG_REQUIRE(kp_num(a->eps), "%s: eps=%g is not a finite number >= 0", who, a->eps);
    hipLaunchKernelGGL(kg_proj_step_kernel, dim3(a->n), dim3(KP_NT), 0, (hipStream_t)stream, *a);
    return kg_launch_status(who);
}
