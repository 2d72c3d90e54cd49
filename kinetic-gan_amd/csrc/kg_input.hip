// Inputs of one training iteration in ONE launch (see include/kgan_hip.h): the batch gathered from the
// device-resident dataset through the epoch's permutation (normalised as x * scale, then + shift: two separately rounded
// operations, what DeviceBatches does with two stock launches), its labels, and every random input - latents, the
// penalty's interpolation weights, the injected noise of both generator syntheses - from Philox4x32-10, all driven by an
// iteration counter in device memory that the launch's last workgroup advances.  A hipGraph that starts with this launch
// replays a training run with no host work between iterations.
//
// Thread-to-element map.  Every thread owns one 16-byte piece (four consecutive fp32 values) of one output: a wave writes
// 1 KiB per store instruction, the widest access there is.  The launch is a list of workgroup ranges, one per output -
// [gather | z | alpha | noise of the critic step's synthesis | noise of the generator step's] - so a workgroup never
// mixes tasks.  Gather: a sample of the resident array is one contiguous, 16-byte aligned row (C*T*V floats: 19200 bytes
// for NTU), read as float4 straight into the float4 store (row-granular gather: every 1-KiB wave access lies inside one
// row except at row ends); any other stride / alignment takes the element-wise form of the same arithmetic.  Random
// streams: a thread evaluates ONE Philox counter - the four words are the stream's elements 4q .. 4q+3 - so the value of
// an element depends on (seed, rank, step, stream, index) and on nothing the launch shape decides.
//
// The counter: every workgroup reads *step first (the value is an input of all its work), draws a ticket when it is done;
// the workgroup that draws the last ticket stores step + 1 and puts the ticket counter back to zero.  No workgroup reads
// anything another one writes in the launch, so no fence is needed beyond the atomics' own ordering on one address.
//
// kg_sample_inputs (sample.Sampler) is the same scheme for a generation round: z, the noise planes of one
// synthesis and the truncation draws as three flat normal streams with counter word 1 = KG_STREAM_SAMPLE + stream.
#include <math.h>

#include "kg_common.h"
#include "kg_handoff.h"

namespace {

constexpr int SI_NT = 256;

struct StepDev {
    long long* step;
    int* ticket;
    unsigned k0, k1;            // Philox key: the seed's low and high word
    unsigned rank4;             // 4 * rank (added to the stream id in counter word 1)
    int rank, world, B;
    // gather
    const float* data;  long d_sN, d_sC, d_sT, d_sV;
    long n_rows;
    const long long* label_src;
    const long long* perm;  long perm_stride;
    long bpe;
    float scale, shift;
    float* real;  long long* labels;
    int C, T, V;
    int row_vec;                // 1: rows are contiguous and 16-byte aligned on both sides (float4 path)
    long row_len;               // C*T*V
    // random outputs
    float* z;  long z_len;
    float* alpha;
    float* noise;  int n_planes;  long pre[KG_STEP_MAX_PLANES + 1];       // prefix sums of plane_len
    // workgroup ranges: [0, b_gather) gather, [.., b_z) z, [.., b_alpha) alpha, [.., b_nd) noise_d, [.., b_ng) noise_g
    unsigned b_gather, b_z, b_alpha, b_nd, b_ng;
};

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;  c1 = lo1;  c2 = n2;  c3 = lo0;
        k0 += 0x9E3779B9u;  k1 += 0xBB67AE85u;
    }
    out[0] = c0;  out[1] = c1;  out[2] = c2;  out[3] = c3;
}

// x * scale, then + shift: two separately rounded operations (what two stock launches compute).  __fmul_rn / __fadd_rn
// are plain operators in HIP's headers and hipcc contracts them into one FMA by default, so contraction is switched off
// for this block.
__device__ __forceinline__ float normalise(float x, float scale, float shift) {
#pragma clang fp contract(off)
    const float p = x * scale;
    return p + shift;
}

__device__ __forceinline__ float uniform24(unsigned w) { return (float)(w >> 8) * 0x1p-24f; }

// Box-Muller on (1 - u0): the log argument lies in (2^-24, 1]
__device__ __forceinline__ void box_muller(unsigned w0, unsigned w1, float& a, float& b) {
    const float rad = sqrtf(__fmul_rn(-2.f, logf(1.f - uniform24(w0))));
    float sn, cs;
    sincosf(__fmul_rn(6.2831855f, uniform24(w1)), &sn, &cs);
    a = __fmul_rn(rad, cs);
    b = __fmul_rn(rad, sn);
}

// elements 4q .. 4q+3 of a stream of `len` elements -> dst[4q ..] (dst = where element 0 of the stream's run starts)
__device__ __forceinline__ void store4(float* dst, long e0, long len, const float (&v)[4]) {
    if (e0 + 4 <= len && (((unsigned long long)(dst + e0)) & 15ull) == 0) {
        *reinterpret_cast<float4*>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < len) dst[e0 + i] = v[i];
    }
}

__global__ __launch_bounds__(SI_NT) void kg_step_inputs_kernel(StepDev a) {
    const long long s = kg_pub_load(a.step);
    const unsigned blk = blockIdx.x;
    const unsigned s_lo = (unsigned)((unsigned long long)s), s_hi = (unsigned)((unsigned long long)s >> 32);

    if (blk < a.b_gather) {
        const long epoch = (long)(s / a.bpe), b = (long)(s - epoch * a.bpe);
        const long long* perm = a.perm + (epoch & 1) * a.perm_stride + (b * a.world + a.rank) * (long)a.B;
        const long q = (long)blk * SI_NT + threadIdx.x;           // 4-element piece of the (B, row_len) output
        if (a.row_vec) {
            const long per_row = a.row_len >> 2;
            if (q < (long)a.B * per_row) {
                const long j = q / per_row, p = q - j * per_row;
                long r = (long)perm[j];
                r = r < 0 ? 0 : (r >= a.n_rows ? a.n_rows - 1 : r);
                const float4 x = *reinterpret_cast<const float4*>(a.data + r * a.d_sN + 4 * p);
                float4 y;
                y.x = normalise(x.x, a.scale, a.shift);
                y.y = normalise(x.y, a.scale, a.shift);
                y.z = normalise(x.z, a.scale, a.shift);
                y.w = normalise(x.w, a.scale, a.shift);
                *reinterpret_cast<float4*>(a.real + j * a.row_len + 4 * p) = y;
                if (p == 0) a.labels[j] = a.label_src[r];
            }
        } else {
            const long total = (long)a.B * a.row_len;
            const long tv = (long)a.T * a.V;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long e = 4 * q + i;
                if (e >= total) break;
                const long j = e / a.row_len, o = e - j * a.row_len;
                const long c = o / tv, rem = o - c * tv, t = rem / a.V, v = rem - t * a.V;
                long r = (long)perm[j];
                r = r < 0 ? 0 : (r >= a.n_rows ? a.n_rows - 1 : r);
                const float x = a.data[r * a.d_sN + c * a.d_sC + t * a.d_sT + v * a.d_sV];
                a.real[e] = normalise(x, a.scale, a.shift);
                if (o == 0) a.labels[j] = a.label_src[r];
            }
        }
    } else if (blk < a.b_alpha) {
        // z (normals) or alpha (uniforms): one flat run each
        const bool is_z = blk < a.b_z;
        const long q = (long)(blk - (is_z ? a.b_gather : a.b_z)) * SI_NT + threadIdx.x;
        const long len = is_z ? a.z_len : (long)a.B;
        if (4 * q < len) {
            unsigned w[4];
            philox4x32_10((unsigned)q, (is_z ? KG_STREAM_Z : KG_STREAM_ALPHA) + a.rank4, s_lo, s_hi, a.k0, a.k1, w);
            float v[4];
            if (is_z) {
                box_muller(w[0], w[1], v[0], v[1]);
                box_muller(w[2], w[3], v[2], v[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = uniform24(w[i]);
            }
            store4(is_z ? a.z : a.alpha, 4 * q, len, v);
        }
    } else {
        // injected noise: stream element e of a synthesis lies in plane i (pre[i] <= e < pre[i+1]); the plane's two halves
        // (critic step's synthesis, generator step's) are adjacent in memory: noise + 2 pre[i] (+ plane_len[i])
        const bool is_d = blk < a.b_nd;
        const long q = (long)(blk - (is_d ? a.b_alpha : a.b_nd)) * SI_NT + threadIdx.x;
        const long total = a.pre[a.n_planes];
        const long e0 = 4 * q;
        if (e0 < total) {
            unsigned w[4];
            philox4x32_10((unsigned)q, (is_d ? KG_STREAM_NOISE_D : KG_STREAM_NOISE_G) + a.rank4, s_lo, s_hi, a.k0, a.k1, w);
            float v[4];
            box_muller(w[0], w[1], v[0], v[1]);
            box_muller(w[2], w[3], v[2], v[3]);
            int i = 0;
#pragma unroll
            for (int k = 1; k < KG_STEP_MAX_PLANES; ++k)
                if (k < a.n_planes && e0 >= a.pre[k]) i = k;
            const long lo = a.pre[i], hi = a.pre[i + 1];
            float* const dst = a.noise + 2 * lo + (is_d ? 0 : hi - lo) - lo;     // element e of this plane at dst[e]
            if (e0 + 4 <= hi && (((unsigned long long)(dst + e0)) & 15ull) == 0) {
                *reinterpret_cast<float4*>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                // a piece that crosses into the next plane(s), the stream's end, or an unaligned plane: element by element
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long e = e0 + k;
                    if (e >= total) break;
                    while (e >= a.pre[i + 1]) ++i;
                    const long l2 = a.pre[i], h2 = a.pre[i + 1];
                    a.noise[2 * l2 + (is_d ? 0 : h2 - l2) + (e - l2)] = v[k];
                }
            }
        }
    }

    // last arriver advances the counter (every workgroup has read it before it draws its ticket)
    __syncthreads();
    if (threadIdx.x == 0 && kg_ticket_draw(a.ticket, (int)gridDim.x)) kg_pub_store(a.step, s + 1);
}

__global__ __launch_bounds__(64) void kg_loss_append_kernel(float* ring, long ring_len, const long long* step, const float* d_loss,
                                                            const float* g_loss) {
    if (threadIdx.x != 0) return;
    const long long s = *step - 1;
    if (s < 0) return;
    const long k = (long)(s % ring_len), kp = (long)((s + ring_len - 1) % ring_len);
    ring[2 * k] = *d_loss;
    ring[2 * k + 1] = g_loss != nullptr ? *g_loss : (s == 0 ? __builtin_nanf("") : ring[2 * kp + 1]);
}

// ---- kg_sample_inputs: the random inputs of one Sampler replay (sample.py) - three flat normal streams -----------------
struct SampleDev {
    long long* step;
    int* ticket;
    unsigned k0, k1;
    float* dst[3];              // z, noise, t (NULL: skipped, no workgroups)
    long len[3];
    unsigned b[3];              // workgroup ranges: stream k owns [b[k-1], b[k])
};

__global__ __launch_bounds__(SI_NT) void kg_sample_inputs_kernel(SampleDev a) {
    const long long s = kg_pub_load(a.step);
    const unsigned blk = blockIdx.x;
    const unsigned s_lo = (unsigned)((unsigned long long)s), s_hi = (unsigned)((unsigned long long)s >> 32);
    const int k = blk < a.b[0] ? 0 : (blk < a.b[1] ? 1 : 2);
    const long q = (long)(blk - (k == 0 ? 0u : a.b[k - 1])) * SI_NT + threadIdx.x;
    const long len = a.len[k];
    if (4 * q < len) {
        unsigned w[4];
        philox4x32_10((unsigned)q, KG_STREAM_SAMPLE + (unsigned)k, s_lo, s_hi, a.k0, a.k1, w);
        float v[4];
        box_muller(w[0], w[1], v[0], v[1]);
        box_muller(w[2], w[3], v[2], v[3]);
        store4(a.dst[k], 4 * q, len, v);
    }
    // last arriver advances the counter (every workgroup has read it before it draws its ticket): nobody waits
    __syncthreads();
    if (threadIdx.x == 0 && kg_ticket_draw(a.ticket, (int)gridDim.x)) kg_pub_store(a.step, s + 1);
}

}  // namespace

extern "C" int kg_sample_inputs(const KgSampleInputsArgs* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_sample_inputs: null args");
    KG_REQUIRE(a->step != nullptr && a->ticket != nullptr, "kg_sample_inputs: null step / ticket");
    SampleDev d = {};
    d.step = (long long*)a->step;  d.ticket = a->ticket;
    d.k0 = (unsigned)(a->seed & 0xffffffffull);  d.k1 = (unsigned)(a->seed >> 32);
    if (a->z != nullptr) {
        KG_REQUIRE(a->B >= 1 && a->latent >= 1, "kg_sample_inputs: z with B=%d latent=%d", a->B, a->latent);
        d.dst[0] = a->z;  d.len[0] = (long)a->B * a->latent;
    }
    if (a->noise != nullptr) {
        KG_REQUIRE(a->noise_len >= 1, "kg_sample_inputs: noise_len=%lld < 1", (long long)a->noise_len);
        d.dst[1] = a->noise;  d.len[1] = (long)a->noise_len;
    }
    if (a->t != nullptr) {
        KG_REQUIRE(a->t_rows >= 1 && a->t_cols >= 1, "kg_sample_inputs: t with t_rows=%d t_cols=%d", a->t_rows, a->t_cols);
        d.dst[2] = a->t;  d.len[2] = (long)a->t_rows * a->t_cols;
    }
    long total = 0;
    for (int k = 0; k < 3; ++k) {
        KG_REQUIRE(d.len[k] <= 0x7fffffffL * 4L, "kg_sample_inputs: stream %d too long", k);
        total += kg_cdiv((d.len[k] + 3) / 4, SI_NT);
        KG_REQUIRE(total <= 0x7fffffffL, "kg_sample_inputs: grid too large");
        d.b[k] = (unsigned)total;
    }
    KG_REQUIRE(total >= 1, "kg_sample_inputs: nothing to write (no z, noise or t)");
    hipLaunchKernelGGL(kg_sample_inputs_kernel, dim3((unsigned)total), dim3(SI_NT), 0, (hipStream_t)stream, d);
    return kg_launch_status("kg_sample_inputs");
}

extern "C" int kg_step_inputs(const KgStepInputsArgs* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_step_inputs: null args");
    KG_REQUIRE(a->step != nullptr && a->ticket != nullptr, "kg_step_inputs: null step / ticket");
    KG_REQUIRE(a->B >= 1, "kg_step_inputs: B=%d < 1", a->B);
    KG_REQUIRE(a->world >= 1 && a->rank >= 0 && a->rank < a->world, "kg_step_inputs: rank=%d outside world=%d", a->rank, a->world);
    KG_REQUIRE(a->rank < (1 << 28), "kg_step_inputs: rank=%d too large", a->rank);
    StepDev d = {};
    d.step = (long long*)a->step;  d.ticket = a->ticket;
    d.k0 = (unsigned)(a->seed & 0xffffffffull);  d.k1 = (unsigned)(a->seed >> 32);
    d.rank4 = 4u * (unsigned)a->rank;
    d.rank = a->rank;  d.world = a->world;  d.B = a->B;
    long n_gather = 0;
    if (a->data != nullptr) {
        KG_REQUIRE(a->C >= 1 && a->T >= 1 && a->V >= 1, "kg_step_inputs: sample shape C=%d T=%d V=%d", a->C, a->T, a->V);
        KG_REQUIRE(a->n_rows >= 1, "kg_step_inputs: n_rows=%lld < 1", (long long)a->n_rows);
        KG_REQUIRE(a->label_src != nullptr && a->perm != nullptr && a->real != nullptr && a->labels != nullptr,
                   "kg_step_inputs: the gather needs label_src, perm, real and labels");
        KG_REQUIRE(a->batches_per_epoch >= 1, "kg_step_inputs: batches_per_epoch=%lld < 1", (long long)a->batches_per_epoch);
        KG_REQUIRE(a->d_sN >= 0 && a->d_sC >= 0 && a->d_sT >= 0 && a->d_sV >= 0, "kg_step_inputs: negative data stride");
        KG_REQUIRE(a->perm_stride >= a->batches_per_epoch * a->world * (int64_t)a->B,
                   "kg_step_inputs: perm_stride=%lld < batches_per_epoch * world * B", (long long)a->perm_stride);
        d.data = a->data;  d.d_sN = a->d_sN;  d.d_sC = a->d_sC;  d.d_sT = a->d_sT;  d.d_sV = a->d_sV;
        d.n_rows = a->n_rows;  d.label_src = (const long long*)a->label_src;
        d.perm = (const long long*)a->perm;  d.perm_stride = a->perm_stride;  d.bpe = a->batches_per_epoch;
        d.scale = a->scale;  d.shift = a->shift;
        d.real = a->real;  d.labels = (long long*)a->labels;
        d.C = a->C;  d.T = a->T;  d.V = a->V;
        d.row_len = (long)a->C * a->T * a->V;
        KG_REQUIRE((long)a->B * d.row_len <= 0x7fffffffL * 4L, "kg_step_inputs: batch too large");
        d.row_vec = a->d_sV == 1 && a->d_sT == a->V && a->d_sC == (long)a->T * a->V && d.row_len % 4 == 0 && a->d_sN % 4 == 0 &&
                    ((unsigned long long)a->data & 15ull) == 0 && ((unsigned long long)a->real & 15ull) == 0;
        n_gather = ((long)a->B * d.row_len + 3) / 4;
    }
    if (a->z != nullptr) {
        KG_REQUIRE(a->latent >= 1, "kg_step_inputs: latent=%d < 1", a->latent);
        d.z = a->z;  d.z_len = (long)a->B * a->latent;
    }
    d.alpha = a->alpha;
    if (a->noise != nullptr) {
        KG_REQUIRE(a->n_planes >= 1 && a->n_planes <= KG_STEP_MAX_PLANES, "kg_step_inputs: n_planes=%d outside [1, %d]", a->n_planes,
                   KG_STEP_MAX_PLANES);
        d.noise = a->noise;  d.n_planes = a->n_planes;
        for (int i = 0; i < a->n_planes; ++i) {
            KG_REQUIRE(a->plane_len[i] >= 1, "kg_step_inputs: plane_len[%d]=%lld < 1", i, (long long)a->plane_len[i]);
            d.pre[i + 1] = d.pre[i] + a->plane_len[i];
        }
        for (int i = a->n_planes; i < KG_STEP_MAX_PLANES; ++i) d.pre[i + 1] = d.pre[a->n_planes];
    }
    const long n_noise = d.noise != nullptr ? (d.pre[d.n_planes] + 3) / 4 : 0;
    KG_REQUIRE(d.z_len <= 0x7fffffffL * 4L && n_noise <= 0x7fffffffL, "kg_step_inputs: random streams too long");
    const long g_gather = kg_cdiv(n_gather, SI_NT), g_z = kg_cdiv((d.z_len + 3) / 4, SI_NT),
               g_alpha = d.alpha != nullptr ? kg_cdiv(((long)a->B + 3) / 4, SI_NT) : 0, g_noise = kg_cdiv(n_noise, SI_NT);
    const long total = g_gather + g_z + g_alpha + 2 * g_noise;
    KG_REQUIRE(total >= 1, "kg_step_inputs: nothing to write (no data, z, alpha or noise)");
    KG_REQUIRE(total <= 0x7fffffffL, "kg_step_inputs: grid too large");
    d.b_gather = (unsigned)g_gather;
    d.b_z = d.b_gather + (unsigned)g_z;
    d.b_alpha = d.b_z + (unsigned)g_alpha;
    d.b_nd = d.b_alpha + (unsigned)g_noise;
    d.b_ng = d.b_nd + (unsigned)g_noise;
    hipLaunchKernelGGL(kg_step_inputs_kernel, dim3((unsigned)total), dim3(SI_NT), 0, (hipStream_t)stream, d);
    return kg_launch_status("kg_step_inputs");
}

extern "C" int kg_loss_append(float* ring, int64_t ring_len, const int64_t* step, const float* d_loss, const float* g_loss,
                              void* stream) {
    KG_REQUIRE(ring != nullptr && step != nullptr && d_loss != nullptr, "kg_loss_append: null ring / step / d_loss");
    KG_REQUIRE(ring_len >= 1, "kg_loss_append: ring_len=%lld < 1", (long long)ring_len);
    hipLaunchKernelGGL(kg_loss_append_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ring, (long)ring_len,
                       (const long long*)step, d_loss, g_loss);
    return kg_launch_status("kg_loss_append");
}
