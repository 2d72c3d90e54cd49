/*
 * kgan_hip.h - C ABI of libkgan_hip.so: the MI355X (gfx950) st_gcn hot path of Kinetic-GAN.
 *
 * The reference has no FFI layer: its hot path is reached through Python
 * nn.Modules that call stock ATen ops.  Each entry point below names the reference op(s) it
 * replaces (file:line relative to the reference repo).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - every tensor is fp32 and lives in device memory owned by the caller (borrowed from torch);
 *    the library never allocates, frees or synchronises; scratch is passed in by the caller,
 *    sized by the matching *_workspace_bytes() query;
 *  - a "plane tensor" is a logical (N, C, T, V) array whose (t, v) plane is contiguous:
 *    element (n,c,t,v) sits at  p + n*sN + c*sC + t*V + v   (strides in elements).  Both the
 *    reference's NCHW layout (sN = C*T*V, sC = T*V) and the channel-major layout this library
 *    prefers between blocks (sN = T*V, sC = N*T*V) are plane tensors;
 *  - `stream` is a hipStream_t passed as void* (the caller passes
 *    torch.cuda.current_stream().cuda_stream); kernels are only enqueued on it;
 *  - return value: 0 = ok, negative = invalid argument / unsupported shape (see
 *    kg_last_error()), positive = hipError_t from the launch;
 *  - re-entrant and thread-safe: no global mutable state except the thread-local error string.
 */
#ifndef KGAN_HIP_H
#define KGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KG_ABI_VERSION 9

enum { KG_ACT_NONE = 0, KG_ACT_LRELU = 1, KG_ACT_TANH = 2 };
enum { KG_TAP_TIME = 0,   /* tap d reads the input at time  t*stride + d - (taps-1)/2            */
       KG_TAP_CHANBLOCK = 1 /* tap d reads input channels [d*Cin, (d+1)*Cin) at the same time  */ };

/* ---- library info -------------------------------------------------------------------------- */
int         kg_abi_version(void);
const char* kg_arch(void);              /* "gfx950" */
const char* kg_last_error(void);        /* thread-local, valid until the next failing call    */
/* The KG_* test / tuning switches (environment variables) are read once when the library is loaded;
 * a test that flips one inside a running process calls this to have them read again.  Not for production use.  */
void        kg_reload_env(void);

/* ---- channel contraction ("tap GEMM") on the fp32 matrix cores ---------------------------------
 * One launch computes, for every output column j = (n, t, v):
 *
 *   out[m, j] = act( sum_g sum_d sum_c  W_g(d, m, c) * X_g[c (+ d*Cin_g if CHANBLOCK), src_g(j, d)]
 *                    + bias0[m] + bias1[m] + add[m, (n, t*add_tstride, v)] )  *  lrelu'(mask[m, j])
 *
 * (the last factor only when `mask` is given: slope where mask <= 0, else 1 - the LeakyReLU derivative expressed
 *  on the activation OUTPUT `mask`, which folds "g * act'(out)" of the consumer into the producing launch)
 *
 * forward  : src = (n, t*stride + shift_d, vmap ? vmap[v] : v)        (zero outside [0,T_in))
 * transposed: src = (n, (t - shift_d)/stride, vmap[v])  if divisible, in range and vmap[v] >= 0
 *             (the adjoint of `forward` w.r.t. its input; vmap is then the inverse vertex map)
 * W_g(d, m, c) = w + d*w_sT + (m / w_MB)*w_sMB + (m % w_MB)*w_sO + c*w_sI
 *
 * Replaces: the 1x1 conv of ConvTemporalGraphical (tgcn.py:48-55,61), the (3x1) temporal conv
 * (discriminator.py:99-105, generator.py:134-140), the 1x1 residual conv (discriminator.py:115-120,
 * generator.py:154-159), "+ res" (discriminator.py:130, generator.py:176), the vertex gather
 * `tensor[:,:,:,keep]` (discriminator.py:139-142), the nearest T/2 resize
 * (discriminator.py:134: only even frames are computed), LeakyReLU / tanh
 * (discriminator.py:136, generator.py:182), and - in transposed mode - their backward-data passes.
 */
typedef struct KgConvGroup {
    const float* x;  int64_t x_sN, x_sC;
    int32_t Cin, T_in, V_in;
    int32_t x_lead;                 /* floats in front of x that belong to the same allocation (>= 0).  Not read by
                                       any kernel: no load path reads in front of a row (0 is fine); kept for the ABI */
    const int32_t* vmap;            /* device ptr, V_out entries, or NULL                         */
    const float* w;  int64_t w_sT, w_sO, w_sI, w_sMB;  int32_t w_MB;
    int32_t taps, tap_mode, t_stride, transposed;
} KgConvGroup;

typedef struct KgConvArgs {
    int32_t N, M, T_out, V_out;
    float* out;  int64_t o_sN, o_sC;
    int32_t ngroups;
    KgConvGroup g[2];
    const float* bias0;  const float* bias1;
    const float* add;  int64_t a_sN, a_sC;  int32_t a_tstride;
    int32_t act;  float slope;
    float* ws;  int64_t ws_bytes;    /* scratch for K-split partial sums (kg_conv_workspace_bytes)  */
    const float* mask;  int64_t m_sN, m_sC;   /* optional (N, M, T_out, V_out) plane tensor, see above      */
    int32_t* sync;  int32_t sync_len;         /* optional: sync_len zeroed ticket counters.  A K-split launch with at most
                                                 sync_len output tiles then completes them itself - the last workgroup of
                                                 a tile to arrive sums the partial slabs in split order and runs the
                                                 epilogue - instead of a second launch; a tile's counter
                                                 is zero again from the moment its last ticket is drawn.
                                                 NULL: the separate epilogue launch.  Launches that share the counters
                                                 must not overlap.                                                     */
    int32_t o_tstride;                        /* 0 / 1: output frames follow each other; s > 1: output frame `to` is
                                                 written at frame to * s of `out` (a transposed stride-2 temporal conv
                                                 runs as two launches, one per output-frame parity, each with only
                                                 the taps that reach it)                                            */
    const void* wpack;  int64_t wpack_bytes;  /* optional (ABI v8): the groups' weights as kg_conv_pack wrote them.  A launch
                                                 the bf16-split form can run (kg_conv_pack_bytes > 0) then runs its tile
                                                 kernel on them - no weight-pack launch, no workspace; any other launch
                                                 ignores the field.  The caller re-packs when the weights change.    */
} KgConvArgs;

int64_t kg_conv_workspace_bytes(const KgConvArgs* a);   /* 0 when the launch needs no scratch (K-split partial slabs; the
                                                           packed weights of the opt-in bf16-split form, KG_CONV_BS=1:
                                                           then `ws` must be 16-byte aligned)                          */
/* which kernel configuration kg_conv would pick (tests / tuning): tile 0..4 = direct kernel with
 * BMxBN = 128x128, 64x128, 32x128, 64x64, 32x64; 9 = 32x32 with the waves splitting K; 11 = tiny-channel streaming
 * kernel; 20.. = tile of the persistent LDS-ring form (KG_CONV_RING); 40..42 = tile of the bf16-split form (KG_CONV_BS) */
int     kg_conv_plan_info(const KgConvArgs* a, int32_t* tile, int32_t* nsplit);
/* several independent problems (own operands, geometry and epilogue each) in ONE launch where the launcher's plans allow it
 * - full K-slices, no K-split, the same weight orientation - and one launch each otherwise; results are those of
 * kg_conv(job i) for every i.  The jobs must not write what another job of the call reads.                          */
#define KG_CONV_MANY_MAX 4
int     kg_conv_many(const KgConvArgs* jobs, int32_t njobs, void* stream);
/* tests / tuning: *tile = the plan tile (0 / 1 / 2) of the shared launch, or -1 when kg_conv_many would launch one by one */
int     kg_conv_many_plan(const KgConvArgs* jobs, int32_t njobs, int32_t* tile);
int     kg_conv(const KgConvArgs* a, void* stream);
/* The weights of a launch in the bf16-split form's layout: every fp32 weight as three bf16 terms,
 * [step = (group, 32-channel slice, tap)][term][8-channel octet][row padded to 128] x 16 bytes.  The layout depends on the
 * groups' weights, Cin, taps and M only - a buffer packed once serves launches of any batch size until the weights change.
 * kg_conv_pack_bytes: bytes to allocate (16-byte aligned), 0 when the bf16-split form cannot run the launch, -1 on bad
 * arguments.  Replaces nothing in the reference (a layout transform of discriminator.py:99-105,115-120's weights).       */
int64_t kg_conv_pack_bytes(const KgConvArgs* a);
int     kg_conv_pack(const KgConvArgs* a, void* wpack, int64_t wpack_bytes, void* stream);
/* tests / tuning (additive, ABI v9): the kernel family, the template instantiation and the launch geometry kg_conv /
 * kg_conv_many take for these arguments under the current KG_CONV_* switches - from the same host functions as the launch
 * itself.  Only dimensions, strides, the null-ness of add / mask / sync / vmap / wpack and the 16-byte alignment of x / wpack
 * are read: no pointer is dereferenced, nothing is launched.  Fields that do not belong to the reported family are 0.    */
#define KG_CONV_FAMILY_DIRECT 0      /* kg_conv_kernel<BM, NW, KF, KW, FAST, PLAIN, INK>                               */
#define KG_CONV_FAMILY_TINY 1        /* kg_conv_tiny_kernel<MT>                                                        */
#define KG_CONV_FAMILY_BS 2          /* kg_conv_bs_kernel<TM, RWV, CWV>: bf16-split, column (or 4-byte window) staging */
#define KG_CONV_FAMILY_BSW 3         /* kg_conv_bsw_kernel<TM, RWV, CWV, PLAIN>: bf16-split, every group a 16-byte window */
#define KG_CONV_FAMILY_MANY 4        /* kg_conv_many_kernel<BM, KF, PLAIN> (KgConvManyForm)                            */
#define KG_CONV_FAMILY_RING 5        /* the LDS-ring form (not in the default build): only `tile` is reported          */
typedef struct KgConvFormInfo {
    int32_t family, tile;                    /* tile: the code of kg_conv_plan_info                                   */
    int32_t BM, NW, KW, KF, FAST, PLAIN, INK;/* direct: the instantiation (KW 4 = K32x32); bs / bsw: BM (rows), PLAIN (bsw) */
    int32_t TM, RWV, CWV;                    /* bs / bsw: the tile variant                                            */
    int32_t MT;                              /* tiny: 4 / 16 rows                                                     */
    int32_t nsplit, per;                     /* workgroups along K, K-slices per split                                */
    int32_t epilogue;                        /* 1: the kg_conv_splitk_epilogue launch follows (K-split, not INK)      */
    int32_t pack, wpack;                     /* bs / bsw: the weight-pack launch precedes; the caller's wpack is used  */
    int32_t win[2];                          /* bs / bsw: group staged as a window (0 no, 1 4-byte, 2 16-byte loads)   */
    int32_t xcd;                             /* 1: XCD-aware 1-D tile order (column tiles padded to a multiple of 8)   */
    int32_t grid_x, grid_y, grid_z;
} KgConvFormInfo;
int     kg_conv_form_info(const KgConvArgs* a, KgConvFormInfo* info);
typedef struct KgConvManyForm {
    int32_t tile;                            /* the shared launch's plan tile (0 / 1 / 2), or -1: one kg_conv per job  */
    int32_t BM, KF, PLAIN;                   /* kg_conv_many_kernel<BM, KF, PLAIN> (every job: NW 4, KW 1, FAST 2)     */
    int32_t njobs, total_wg;                 /* grid of the shared launch                                             */
    int32_t xcd[4], wg_begin[4], nwg[4];     /* per job: tile order, first workgroup, workgroups that do work          */
} KgConvManyForm;
int     kg_conv_many_form(const KgConvArgs* jobs, int32_t njobs, KgConvManyForm* form);

/* ---- weight gradient of the tap GEMM -----------------------------------------------------------
 *   dW(d, m, c) = sum_j  G[m, j] * X[c (+ d*Cin if CHANBLOCK), src(j, d)]      (src as `forward`)
 * written to  dw + d*w_sT + m*w_sO + c*w_sI.  Split over column ranges into `splits` partial
 * slabs in `ws` (deterministic two-pass reduction, no atomics).
 * Replaces aten::convolution_backward's weight part for the three convs above.                 */
/* an additional (g, x) operand pair of the same layer geometry whose product is added into the same dW: the same
 * weight receives several gradient contributions in one WGAN-GP backward pass (the real+fake batch, the penalty's
 * forward graph and its double-backward graph); one launch over the concatenated column ranges replaces three. */
typedef struct KgWgradPair {
    int32_t N;
    const float* g;  int64_t g_sN, g_sC;
    const float* x;  int64_t x_sN, x_sC;
} KgWgradPair;

typedef struct KgWgradArgs {
    int32_t N, M, T_out, V_out;
    const float* g;  int64_t g_sN, g_sC;
    const float* x;  int64_t x_sN, x_sC;
    int32_t Cin, T_in, V_in;
    const int32_t* vmap;
    int32_t taps, tap_mode, t_stride;
    float* dw;  int64_t w_sT, w_sO, w_sI;
    float* ws;  int64_t ws_bytes;
    int32_t accumulate;             /* 0: dw = result; 1: dw += result (gradient accumulation in place, e.g. into
                                       the flat gradient bucket the all-reduce and the optimizer work on)        */
    int32_t nextra;                 /* 0..2 additional operand pairs                                               */
    KgWgradPair extra[2];
    int32_t defer_reduce;           /* 1: only write the partial slabs; the caller reduces them later with
                                       kg_wgrad_reduce_many (ws must stay alive until then)                        */
} KgWgradArgs;

int64_t kg_wgrad_workspace_bytes(const KgWgradArgs* a);   /* = splits * taps * M * Cin * 4                        */
int     kg_wgrad(const KgWgradArgs* a, void* stream);
/* tile variants of the weight-gradient kernels (output rows x input channels per workgroup), as the plan reports name them */
#define KG_WGRAD_TILE_128x128 0
#define KG_WGRAD_TILE_64x64   1
#define KG_WGRAD_TILE_64x32   2
#define KG_WGRAD_TILE_32x64   3
#define KG_WGRAD_TILE_32x32   4
/* tests / tuning (additive, ABI v9): the tile variant and the number of partial slabs kg_wgrad takes for `a` (the variant is
 * always KG_WGRAD_TILE_64x64 today).  Geometry only: the pointers of `a` are not looked at.  Launches nothing.        */
int     kg_wgrad_plan_info(const KgWgradArgs* a, int32_t* variant, int32_t* splits);

/* The slab reductions of several deferred kg_wgrad launches in ONE launch (a backward pass produces the weight
 * gradients of all layers back to back; 17-19 reductions of a few microseconds each become one).              */
typedef struct KgWgradReduceJob {
    const float* ws;  float* dw;
    int64_t w_sT, w_sO, w_sI;
    int32_t taps, M, Cin, splits, accumulate;
} KgWgradReduceJob;
#define KG_WGRAD_REDUCE_MAX_JOBS 24
typedef struct KgWgradReduceJobs {
    int32_t njobs;
    KgWgradReduceJob job[KG_WGRAD_REDUCE_MAX_JOBS];
} KgWgradReduceJobs;
int     kg_wgrad_reduce_many(const KgWgradReduceJobs* jobs, void* stream);

/* The weight gradients of SEVERAL layers (jobs[0..njobs), each a complete KgWgradArgs with its operand pairs, dw,
 * strides and accumulate flag; jobs[i].ws / ws_bytes / defer_reduce are ignored) in shared launches: the column
 * ranges of all layers are split against ONE workgroup budget and the slab reductions follow in the same call.
 * No two jobs may write the same dw.  Replaces one kg_wgrad + one reduction per layer of a backward pass
 * (aten::convolution_backward's weight halves of all of discriminator.py:99-120 / generator.py:134-159).        */
int64_t kg_wgrad_many_workspace_bytes(const KgWgradArgs* jobs, int32_t njobs);
int     kg_wgrad_many(const KgWgradArgs* jobs, int32_t njobs, float* ws, int64_t ws_bytes, void* stream);
/* tests / tuning (additive, ABI v9): variant[i] / splits[i] = the tile variant (KG_WGRAD_TILE_*) and the number of partial
 * slabs job i of kg_wgrad_many(jobs, njobs, ...) takes (1 = the tile kernel writes dw itself) - the same walk over the jobs
 * as the launch (cost target, coarser first half, KG_WGRAD_* switches).  Geometry only; launches nothing.               */
int     kg_wgrad_many_plan(const KgWgradArgs* jobs, int32_t njobs, int32_t* variant, int32_t* splits);

/* ---- spatial graph aggregation -------------------------------------------------------------------
 * A is (K, V, W) row-major fp32 in device memory (the effective adjacency A[lvl]*importance,
 * optionally restricted to kept columns, or the up-sampling matrix with K = 1); it is staged in
 * LDS once per workgroup.
 *
 *  expand : out[k*C + c, (n, t', w)] = sum_v x[c, (n, t'/rep, v)] * A[k, v, w]       T' = T*rep
 *  reduce : out[c, (n, t, w)] = sum_{q<fold} sum_k sum_v y[k*C + c, (n, t*fold+q, v)] * A[k, v, w]
 *  outer  : dA[k, v, w] = sum_{c, n, t'} x[c, (n, t'/rep, v)] * y[k*C + c, (n, t', w)]
 *
 * Replaces torch.einsum('nkctv,kvw->nctw') (tgcn.py:66) in both operand orders, its two
 * gradients, upsample_s + the nearest T up-sampling of the generator (generator.py:172,185-200;
 * K = 1, A = U) and their adjoints.                                                             */
typedef struct KgAggArgs {
    int32_t N, C, K, V, W;          /* C = channels of the un-expanded side                       */
    int32_t T;                      /* frames of the (t,V) side: x for expand/outer, out for reduce */
    int32_t rep;                    /* expand/outer: rep; reduce: fold                             */
    const float* a;                 /* (K, V, W)                                                   */
    const float* x;  int64_t x_sN, x_sC;   /* expand/outer: x (C ch, V) ; reduce: y (K*C ch, V)    */
    const float* y;  int64_t y_sN, y_sC;   /* outer only: y (K*C ch, W)                            */
    float* out;  int64_t o_sN, o_sC;       /* expand: (K*C ch, W); reduce: (C ch, W); outer: dA    */
    float* ws;  int64_t ws_bytes;          /* outer only                                           */
    int32_t a_transposed;                  /* expand / reduce: `a` is stored (K, W, V): A[k][v][w] = a[(k*W + w)*V + v]
                                              (the adjoint passes use A^T without materialising it)              */
    int32_t defer_sum;                     /* outer: 1 = only the partial slabs are written to ws; the caller finishes
                                              several launches at once with kg_agg_outer_sum_many                 */
    /* reduce only (fold = 1), optional epilogue - the backward pass of a discriminator block (ABI v5):
     *   out[n,c,t,w] = ( aggregate + [t % r_tstride == 0 and r_inv[w] >= 0] res[n,c,t/r_tstride,r_inv[w]] ) * lrelu'(mask[n,c,t,w])
     * res: (N, C, r_T, r_V) plane tensor, the residual branch's input gradient at the frames / vertices the branch reads
     * (discriminator.py:115-120,134,139-142); r_inv (W): vertex of res that w reads or -1, NULL = identity;
     * mask: (N, C, T, W) activation output of the previous block (slope where <= 0).  Either may be NULL.          */
    const float* res;  int64_t r_sN, r_sC;  int32_t r_T, r_V, r_tstride;  const int32_t* r_inv;
    const float* mask;  int64_t m_sN, m_sC;  float slope;
} KgAggArgs;

int     kg_agg_expand(const KgAggArgs* a, void* stream);
int     kg_agg_reduce(const KgAggArgs* a, void* stream);
int64_t kg_agg_outer_workspace_bytes(const KgAggArgs* a);
int     kg_agg_outer(const KgAggArgs* a, void* stream);
/* the slab reductions of several deferred kg_agg_outer launches (one per block of a backward pass) in ONE launch */
int     kg_agg_outer_slabs(const KgAggArgs* a);          /* partial slabs kg_agg_outer writes for these arguments */
typedef struct KgOuterSumJob { const float* ws; float* out; int32_t nout, slabs; } KgOuterSumJob;
#define KG_OUTER_SUM_MAX_JOBS 16
typedef struct KgOuterSumJobs { int32_t njobs; KgOuterSumJob job[KG_OUTER_SUM_MAX_JOBS]; } KgOuterSumJobs;
int     kg_agg_outer_sum_many(const KgOuterSumJobs* jobs, void* stream);
/* several kg_agg_outer problems (every job with its own ws / ws_bytes / out; defer_sum ignored) in one launch for the
 * matrix-core form plus one launch for all slab sums: the adjacency gradients of a whole backward pass            */
int     kg_agg_outer_many(const KgAggArgs* jobs, int32_t njobs, void* stream);
/* tests / tuning (additive, ABI v9): the kernel form, the template instantiation and the launch geometry kg_agg_expand /
 * kg_agg_reduce / kg_agg_outer take for these arguments under the current KG_AGG_* switches - from the same host
 * planning functions as the launch itself.  Only dimensions, strides and the null-ness of res / mask are read: no pointer is
 * dereferenced, nothing is launched.  Fields that do not belong to the reported form are 0.                          */
#define KG_AGG_OP_EXPAND 0
#define KG_AGG_OP_REDUCE 1
#define KG_AGG_OP_OUTER 2
#define KG_AGG_FORM_FRAME 0          /* one thread per frame: kg_agg_{expand,reduce}_kernel<K, WP>                     */
#define KG_AGG_FORM_STREAM 1         /* kg_agg_{expand,reduce}_stream_kernel<K, VM>                                    */
#define KG_AGG_FORM_MFMA 2           /* kg_agg_mfma_kernel<KI, KO, KS, RES, MSK>                                       */
#define KG_AGG_FORM_OUTER_ELEM 3     /* kg_agg_outer_kernel<K>                                                         */
#define KG_AGG_FORM_OUTER_MFMA 4     /* kg_agg_outer_mfma_kernel<K, TV, TW>                                            */
typedef struct KgAggPlanInfo {
    int32_t form, K;
    int32_t WP;                              /* frame form: W padded to 4 / 8 / 16 / 28                                */
    int32_t VM, FO;                          /* stream form: V padded to 4 / 8 / 16 / 25, output frames per workgroup  */
    int32_t KI, KO, KS, RES, MSK;            /* mfma form: the instantiation ...                                       */
    int32_t SUB, tiles_per_c, ntiles;        /* ... sub-tiles per tile, tiles per channel, tiles of the launch         */
    int32_t TV, TW;                          /* outer mfma form: 16-wide tiles over V / W                              */
    int32_t P, F, chunks, units, slabs;      /* outer: frame blocks per MFMA tile (mfma form), frames per unit, units per
                                                channel, units of the launch, partial slabs (= workgroups)             */
    int32_t grid_x, grid_y, lds_bytes;       /* every form; lds_bytes = dynamic LDS of the launch                      */
} KgAggPlanInfo;
int     kg_agg_plan_info(const KgAggArgs* a, int32_t op, KgAggPlanInfo* info);
/* launch[i] = index of the shared kg_agg_outer_many launch job i rides in, or -1 when it is launched on its own;
 * slabs[i] = partial slabs (workgroups) the launch's budget (KG_AGG_OUTER_BUDGET) gives it.  The walk of kg_agg_outer_many. */
int     kg_agg_outer_many_plan(const KgAggArgs* jobs, int32_t njobs, int32_t* launch, int32_t* slabs);

/* ---- fused aggregation + gcn contraction of a discriminator block ("disc block forward", first half) -----------
 *   out[m, (n,t,w)] = sum_k sum_c W(k,m,c) * ( sum_v x[c, (n,t,v)] * A[k,v,w] )  + add[m, (n, t*a_tstride, w)]
 * = ConvTemporalGraphical (tgcn.py:58-68) in aggregate-first order restricted to the vertices the block keeps
 * (discriminator.py:125-142): sum_k (W_k x) A_k == sum_k W_k (x A_k).  The K*Cin aggregated planes are formed in
 * LDS / registers as the B operand of the MFMA and never written to HBM - unless `xa` is given, then they are also
 * stored (the gcn weight gradient needs them).  The adjacency's fixed sparsity pattern comes as a neighbour table:
 * nbr[(k*W + w)*4 + p] = p-th source vertex v with A[k,v,w] != 0, or -1; pcount[k] = most entries of any column of
 * A_k (supported: <= 1 / 4 / 1, what graph_ntu.py / graph_h36m.py produce at every level); the VALUES are read
 * from `a` (the live A[lvl] * edge_importance, (K,V,W), or stored (K,W,V) with a_transposed).
 * kg_aggconv_supported: 1 if this launch geometry can take the fused kernel (else use kg_agg_expand + kg_conv).  */
typedef struct KgAggConvArgs {
    int32_t N, Cin, M, T, V, W, K;
    const float* x;  int64_t x_sN, x_sC;           /* (N, Cin, T, V) plane tensor                              */
    const float* a;  int32_t a_transposed;
    const int32_t* nbr;  int32_t pcount[3];
    const float* w;  int64_t w_sT, w_sO, w_sI;     /* W(k, m, c) = w + k*w_sT + m*w_sO + c*w_sI                */
    float* out;  int64_t o_sN, o_sC;               /* (N, M, T, W)                                             */
    const float* add;  int64_t a_sN, a_sC;  int32_t a_tstride;   /* optional; a_tstride 0 = one frame for all t */
    float* xa;  int64_t xa_sN, xa_sC;              /* optional (N, K*Cin, T, W)                                */
} KgAggConvArgs;

int kg_aggconv_supported(const KgAggConvArgs* a);
int kg_aggconv(const KgAggConvArgs* a, void* stream);
/* tests / tuning (additive, ABI v9): the form kg_aggconv (label_J = 0) or kg_aggconv_label (label_J = J of its label bias, > 0)
 * takes for these arguments under the current KG_AGGCONV_* switches, from the launchers' own planning function; no pointer
 * is dereferenced (null-ness of add / xa is read), nothing is launched.
 * tiny = 1: kg_aggconv_tiny_kernel<MT, RG, LB>;  tiny = 0: kg_aggconv_kernel<BM, XE, KS, XA, ADD, 1, 4, 1>, tapmask / spanp
 * as the kernel receives them.  Fields of the other form are 0.                                                       */
typedef struct KgAggConvPlanInfo {
    int32_t tiny;
    int32_t MT, RG, LB;
    int32_t BM, KS, XE, XA, ADD, tapmask, spanp;
    int32_t grid_x, grid_y, lds_bytes;
} KgAggConvPlanInfo;
int kg_aggconv_plan_info(const KgAggConvArgs* a, int32_t label_J, KgAggConvPlanInfo* info);

/* ---- generator st_gcn block on the coarse grid ("fused G-block", generator.py:168-182) -------------------------------
 * The block's 1x1 convs commute with upsample_s (x U, generator.py:185-200) and the nearest frame repeat
 * (generator.py:172), so ONE kg_conv launch computes y = [W_gcn; W_res] x on the block's INPUT grid (N, *, Tc, Vc) and
 *
 *  kg_gen_expand:  z[c,(n,t',w)]  = sum_k sum_vc y[k*C + c,(n,t'/rep,vc)] * B_k[vc,w],        B_k = U A_k   (Vc x V)
 *                  r[cr,(n,t',w)] = sum_vc rs[cr,(n,t'/rep,vc)] * U[vc,w] + rbias[cr]          T' = Tc*rep
 *                  = upsample_s + F.interpolate + tgcn.py:66's einsum of the gcn branch, and upsample_s + interpolate
 *                  (+ bias) of the residual branch (rs = the residual conv's rows of y, or the block input itself for an
 *                  identity residual); the up-sampled input and the fine-grid conv output never exist
 *  kg_gen_fold:    the adjoint:  y_out[k*C + c,(n,tc,vc)] = sum_{q<rep} sum_w z[c,(n,tc*rep+q,w)] * B_k[vc,w]
 *                                rs_out[cr,(n,tc,vc)]     = sum_{q<rep} sum_w r[cr,(n,tc*rep+q,w)] * U[vc,w]
 *                                zf[c,(n,tc,w)]           = sum_{q<rep} z[c,(n,tc*rep+q,w)]          (optional)
 *                  (z, r hold the gradients w.r.t. z and r here; zf feeds the adjacency gradient:
 *                   d B_k[vc,w] = sum zf[c,(.,w)] * y[k*C + c,(.,vc)] = kg_agg_outer(zf, y) transposed)
 *  kg_gen_adj_finish: out[k,v,w] (+)= a[k,v,w] * sum_vc u[vc,v] * dbt[k,w,vc]     for k < Kd, 0 beyond
 *                  = d edge_importance from the (Kd, V, Vc) outer products of all blocks in ONE launch
 *                  (generator.py:92-93: A[lvl] * importance; d A_k = U^T d B_k).
 * a: (K, V, V); u: (Vc, V) or NULL (no spatial up-sampling: Vc == V).  Either branch may be absent (z / r NULL).
 * Tensors are limited to 2^31 elements per launch (32-bit item indices).                                             */
typedef struct KgGenArgs {
    int32_t N, C, K, Cr, Tc, Vc, V, rep;
    const float* a;  const float* u;
    const float* b;                                          /* optional: the product U A_k (K, Vc, V) precomputed by
                                                                kg_gen_adj_prepare; NULL: formed from a and u in LDS   */
    const float* y;  float* y_out;  int64_t y_sN, y_sC;      /* (N, K*C, Tc, Vc): expand reads y, fold writes y_out */
    float* z;  int64_t z_sN, z_sC;                           /* (N, C, Tc*rep, V): expand writes, fold reads          */
    float* zf;  int64_t zf_sN, zf_sC;                        /* fold only, optional: (N, C, Tc, V)                     */
    const float* rs;  float* rs_out;  int64_t rs_sN, rs_sC;  /* (N, Cr, Tc, Vc)                                        */
    const float* rbias;                                      /* expand: (Cr) or NULL                                   */
    float* r;  int64_t r_sN, r_sC;                           /* (N, Cr, Tc*rep, V)                                     */
} KgGenArgs;

int kg_gen_expand(const KgGenArgs* a, void* stream);
int kg_gen_fold(const KgGenArgs* a, void* stream);

typedef struct KgGenAdjJob {
    const float* dbt;               /* (Kd, V, Vc) */
    const float* u;                 /* (Vc, V) or NULL */
    const float* a;                 /* (K, V, V) fixed adjacency A[lvl] or NULL (= 1) */
    float* out;                     /* (K, V, V) */
    int32_t K, Kd, V, Vc, accumulate;
} KgGenAdjJob;
#define KG_GEN_ADJ_MAX_JOBS 8
int kg_gen_adj_finish(const KgGenAdjJob* jobs, int32_t njobs, void* stream);

/* kg_gen_adj_prepare: aeff[k,v,w] = a[k,v,w] * imp[k,v,w] (generator.py:92-93: A[lvl] * importance; imp NULL = 1) and
 * b[k,vc,w] = sum_v u[vc,v] * aeff[k,v,w] (u NULL: b = aeff) for all blocks of a forward pass in ONE launch.       */
typedef struct KgGenPrepJob {
    const float* a;  const float* imp;  const float* u;
    float* aeff;  float* b;
    int32_t K, V, Vc;
} KgGenPrepJob;
int kg_gen_adj_prepare(const KgGenPrepJob* jobs, int32_t njobs, void* stream);

/* Backward of a generator block's tail  out = act( BN_t(u) + BN_r(r) + w_noise * noise )  (generator.py:142,160,176,179-182):
 *   kg_gen_tail_stats : with gp = g * act'(out) formed on the fly, the per-channel sums  sum gp, sum gp (u - mean_t),
 *                       sum gp (r - mean_r), sum gp * noise  ->  coef (6, C) = [a_t, b_t, c_t, a_r, b_r, c_r] with
 *                       d loss / d u = a_t gp + b_t u + c_t (BatchNorm2d backward in training mode; a branch without
 *                       BatchNorm: (1, 0, 0)), and d gamma / d beta of both layers and d w_noise ADDED into the given
 *                       (C) buffers (NULL: skipped) - e.g. their slices of the flat gradient bucket
 *   kg_gen_tail_apply : du (and dr) from g, out, u, r and coef in one pass
 * u == NULL: no BatchNorm on the tcn branch; mean_r == NULL: none on the residual branch (r may still be given: an
 * identity residual, dr = gp).  `counters`: >= C zeroed int32, left zeroed (each is zero
 * again from the moment its last ticket is drawn).                                                     */
typedef struct KgGenTailArgs {
    int32_t N, C, T, V;  int32_t act;  float slope;
    const float* g;  int64_t g_sN, g_sC;
    const float* out;  int64_t o_sN, o_sC;
    const float* u;  int64_t u_sN, u_sC;  const float* mean_t;  const float* rstd_t;  const float* gamma_t;
    const float* r;  int64_t r_sN, r_sC;  const float* mean_r;  const float* rstd_r;  const float* gamma_r;
    const float* noise;                     /* (N, 1, T, V) contiguous or NULL                                 */
    float* coef;                            /* (6, C)                                                          */
    float* dgamma_t;  float* dbeta_t;  float* dgamma_r;  float* dbeta_r;  float* dnw;
    float* ws;  int64_t ws_bytes;  int32_t* counters;  int32_t counters_len;
    float* du;  int64_t du_sN, du_sC;
    float* dr;  int64_t dr_sN, dr_sC;       /* NULL: no residual branch                                        */
} KgGenTailArgs;
int64_t kg_gen_tail_workspace_bytes(const KgGenTailArgs* a);
int     kg_gen_tail_stats(const KgGenTailArgs* a, void* stream);
int     kg_gen_tail_apply(const KgGenTailArgs* a, void* stream);

/* ---- fused generator block (ABI v9): generator.st_gcn.forward (generator.py:168-182) and its backward as ONE launch each --
 * The launch-per-stage form above (kg_conv on the input grid -> kg_gen_expand -> kg_conv (tcn) -> kg_bn_fwd_many ->
 * kg_affine_act) is 5-7 launches per block for a few MFLOP: pure latency.  For the blocks whose per-sample working set
 * fits LDS (the generator's last four: <= 128 input channels) ONE workgroup carries ONE sample through the whole block:
 *
 *   fwd:  x    = finished input, or the PREVIOUS block's pending tail  pact(pu*s_t + b_t + pr*s_r + b_r + pnw*pnoise)
 *                (its BatchNorm coefficients became known at the previous launch's end; x is written to `xout`)
 *         yc   = [W_gcn[:Kp*C]; W_res] x                         on the input grid (Tc, Vc)          -> `yc`
 *         z, r = sum_k yc_k (U A_k) / yc_res U + b_res (or x U: identity residual), frames repeated  -> `z`, `r`
 *         u    = W_tcn (*) z + b_tcn                             3 temporal taps, zero padding       -> `u`
 *         per-sample (mean, centred sum of squares) of u and r per channel -> the last workgroup to arrive merges them in
 *         sample order (Chan et al.) into coef_t / coef_r (groups, 4, C) = [scale, shift, mean, rstd] and updates the
 *         running statistics batch by batch, exactly as kg_bn_fwd_many; a block without any BatchNorm finishes itself:
 *         out = act(u + r + nw * noise)                                                               -> `out`
 *   bwd:  du, dr from g, out, u, r and the tail coefficients `coef` (6, C) (kg_gen_tail_stats, or the previous fused
 *         backward launch);  gz = W_tcn^T (*) du;  gyc = fold(gz (U A_k)^T), fold(dr U^T);  zf = gz summed over repeated
 *         frames;  gx = [W_gcn; W_res]^T gyc (+ identity branch);  then the tail statistics of the block BEFORE this one
 *         (sums of gp = gx * pact'(x) against pu, pr, pnoise -> `pcoef` (6, Cin), parameter gradients ADDED into the given
 *         buffers), merged by the last workgroup to arrive.
 * Every tensor the deferred parameter-gradient launches read (x, yc, z, u, r / du, dr, gyc, zf) is written exactly as
 * the staged form writes it.  kg_genblock_lds_bytes: dynamic LDS the launch needs, or -1 when the block does not fit
 * (then the staged entry points apply).  `counters`: >= 1 zeroed int32, left zeroed (forward: zero again from the
 * moment the launch's last ticket is drawn; backward: when its last workgroup has finished - DESIGN.md 5.6).          */
typedef struct KgPlane { float* p;  int64_t sN, sC; } KgPlane;             /* (N, C, T, V) plane tensor, NULL p = absent */
typedef struct KgGenBnLayer {                                             /* one training-mode BatchNorm2d of the block */
    const float* gamma;  const float* beta;  float* running_mean;  float* running_var;  int64_t* num_batches_tracked;
    float momentum, eps;
    float* coef;                                                          /* out: (groups, 4, C)                        */
} KgGenBnLayer;
typedef struct KgGenBlockArgs {
    int32_t N, groups;                      /* N samples = `groups` batches stacked along N (BatchNorm statistics per batch) */
    int32_t Cin, C, K, Kp;                  /* channels in / out; partitions of the gcn weight / of them that act (1 at V = 1) */
    int32_t Tc, Vc, T, V, rep;              /* input grid, output grid, T = Tc * rep                                     */
    int32_t res_kind;                       /* 0 none, 1 identity (Cin == C), 2 conv + BatchNorm                          */
    int32_t bn_t;                           /* BatchNorm behind the temporal conv                                        */
    int32_t act;  float slope;
    KgPlane x;                              /* finished input (N, Cin, Tc, Vc), or absent: the pending tail below       */
    KgPlane pu, pr;  const float* pcoef_t;  const float* pcoef_r;  const float* pnoise;  const float* pnw;  int32_t pact;
    KgPlane xout;
    const float* wg;  const float* wr;  const float* br;  const float* wt;  const float* bt;
    const float* b;                         /* (Kp, Vc, V) = U (A * importance), kg_gen_adj_prepare                     */
    const float* u;                         /* (Vc, V) up-sampling matrix or NULL (Vc == V)                             */
    KgPlane yc, z, r, uo;                   /* tape: (N, Kp*C [+ C], Tc, Vc), (N, C, T, V) x 3; r absent for res_kind 0  */
    KgGenBnLayer bt_, br_;                  /* used when bn_t / res_kind == 2                                           */
    const float* noise;  const float* nw;  KgPlane out;       /* self-finishing blocks (no BatchNorm at all)            */
    float* ws;  int64_t ws_bytes;  int32_t* counters;  int32_t counters_len;
} KgGenBlockArgs;
typedef struct KgGenBlockBwdArgs {
    int32_t N;                              /* samples of the differentiated batch                                      */
    int32_t Cin, C, K, Kp, Tc, Vc, T, V, rep, res_kind, bn_t, act;  float slope;
    KgPlane g, out, uo, r;                  /* d loss / d out, and the block's taped out / u / r                        */
    const float* coef;                      /* (6, C) tail coefficients of THIS block                                   */
    const float* wg;  const float* wr;  const float* wt;  const float* b;  const float* u;
    KgPlane du, dr, gyc, zf, gx;            /* out.  dr absent: no residual branch, or du == dr (no BatchNorm at all);
                                               gyc (N, Kp*C [+ C], Tc, Vc); zf (N, C, Tc, V); gx (N, Cin, Tc, Vc)       */
    /* tail statistics of the PREVIOUS block (absent px: skipped)                                                        */
    KgPlane px, pu, pr;  const float* pnoise;  int32_t pact;
    const float* pmean_t;  const float* prstd_t;  const float* pgamma_t;
    const float* pmean_r;  const float* prstd_r;  const float* pgamma_r;
    float* pcoef;  float* dgamma_t;  float* dbeta_t;  float* dgamma_r;  float* dbeta_r;  float* dnw;
    float* ws;  int64_t ws_bytes;  int32_t* counters;  int32_t counters_len;
} KgGenBlockBwdArgs;
int64_t kg_genblock_lds_bytes(const KgGenBlockArgs* a);
int64_t kg_genblock_workspace_bytes(const KgGenBlockArgs* a);
int     kg_genblock_fwd(const KgGenBlockArgs* a, void* stream);
int64_t kg_genblock_bwd_lds_bytes(const KgGenBlockBwdArgs* a);
int64_t kg_genblock_bwd_workspace_bytes(const KgGenBlockBwdArgs* a);
int     kg_genblock_bwd(const KgGenBlockBwdArgs* a, void* stream);
/* tests / tuning (additive, ABI v9): the kernel instantiation, the path of the two channel contractions and the launch
 * geometry kg_genblock_fwd / _bwd / _infer take for a block under the current KG_GB_RT switch - from the same host functions
 * as the launchers.  Only dimensions and flags are read: nothing is dereferenced, nothing is launched.
 *   geometry   index into the compile-time geometries (GB_GEOMETRIES of csrc/kg_genblock.hip), -1: the run-time form
 *   mfma0/1    1: the head contraction (yc forward, gx backward) / the tcn contraction runs on the matrix cores - for a
 *              compile-time geometry the path the kernel itself resolves from its constants
 *   mv0/1      the row bucket (4 / 16 / 32) of the VALU path, 0 on the matrix-core path
 *   lds_bytes  dynamic LDS of the launch, -1 where the launcher (or its eligibility query) refuses the block
 *   grid_x     workgroups (one per sample)                                                                            */
#define KG_GB_DIR_FWD 0
#define KG_GB_DIR_BWD 1
#define KG_GB_DIR_INFER 2
typedef struct KgGenBlockFormQuery {
    int32_t N, groups;                      /* groups: forward only (1 elsewhere)                                        */
    int32_t Cin, C, K, Kp, Tc, Vc, T, V, rep, res_kind, bn_t;
    int32_t dir;                            /* KG_GB_DIR_*                                                               */
    int32_t prev;                           /* backward: the previous block's tail statistics ride along (px given)      */
    int32_t wg_aligned, wr_aligned, wt_aligned;     /* 16-byte alignment of the weight pointers (forward, inference)     */
} KgGenBlockFormQuery;
typedef struct KgGenBlockForm {
    int32_t geometry, mfma0, mfma1, mv0, mv1, lds_bytes, grid_x;
} KgGenBlockForm;
int     kg_genblock_form(const KgGenBlockFormQuery* q, KgGenBlockForm* form);

/* ---- per-channel reductions over (n, t, v) ---------------------------------------------------------
 *   out[0*C + c] = sum x ;  out[1*C + c] = sum x*(y - shift[c])   (y == NULL: sum (x - shift[c])^2)
 * shift (C floats, may be NULL = 0) makes the second moment a centred one: BatchNorm2d batch
 * statistics are taken in two passes (mean, then sum (x-mean)^2) to avoid the E[x^2]-mean^2
 * cancellation.  Used for conv bias gradients and BatchNorm2d (generator.py:142,160).            */
typedef struct KgRowsumArgs {
    int32_t N, C, T, V;
    const float* x;  int64_t x_sN, x_sC;
    const float* y;  int64_t y_sN, y_sC;
    const float* shift;
    int32_t want_second;            /* 0: out (1, C) = sum x; 1: out (2, C) = [sum x, sum x*(y-shift)] ((x-shift)^2 without y);
                                       2: out (1, C) = the second sum alone (NoiseInjection.weight gradient)    */
    float* out;                     /* (2, C) or (1, C)                                            */
    float* ws;  int64_t ws_bytes;
    int32_t accumulate;             /* 0: out = sums; 1: out += sums                               */
    float* out2;                    /* optional second destination of the same sums (two biases that share one
                                       gradient: tcn + residual conv of a D block), same accumulate rule        */
} KgRowsumArgs;

int64_t kg_rowsum_workspace_bytes(const KgRowsumArgs* a);
int     kg_rowsum(const KgRowsumArgs* a, void* stream);
/* several reductions (jobs[i].ws / ws_bytes are ignored; no two jobs may share a destination) in one launch + one
 * finishing launch: the bias gradients of all convs of a backward pass                                          */
int64_t kg_rowsum_many_workspace_bytes(const KgRowsumArgs* jobs, int32_t njobs);
int     kg_rowsum_many(const KgRowsumArgs* jobs, int32_t njobs, float* ws, int64_t ws_bytes, void* stream);

/* ---- pointwise epilogues ---------------------------------------------------------------------------
 * kg_act_bwd : out = g * act'(ref)  where ref is the activation OUTPUT
 *              (LeakyReLU: ref > 0 ? 1 : slope; tanh: 1 - ref^2)      discriminator.py:136, generator.py:182
 * kg_affine_act: out = act( x*sx[c] + bx[c] + r*sr[c] + br[c] + nw[c]*noise[n,t,v] )
 *              the generator block tail: BatchNorm2d normalise/affine of the tcn branch and of the
 *              residual branch, "+ res", NoiseInjection and the activation in one pass
 *              (generator.py:142,160,176,179-182).  r / noise / any scale vector may be NULL.     */
typedef struct KgEltArgs {
    int32_t N, C, T, V;
    const float* x;  int64_t x_sN, x_sC;
    const float* r;  int64_t r_sN, r_sC;
    const float* noise;                 /* (N, 1, T, V) contiguous                                 */
    const float* sx; const float* bx; const float* sr; const float* br; const float* nw;
    float* out;  int64_t o_sN, o_sC;
    int32_t act;  float slope;
    int32_t groups;                     /* kg_affine_act: > 1 = that many batches stacked along N, each with its own  */
    int64_t coef_gs;                    /* sx/bx/sr/br: batch q reads them at + q * coef_gs floats (nw is shared)      */
} KgEltArgs;

int kg_act_bwd(const KgEltArgs* a, void* stream);      /* x = g, r = ref                           */
int kg_affine_act(const KgEltArgs* a, void* stream);

/* ---- BatchNorm2d statistics + coefficients in one launch (generator.py:142,160: tcn.1 / residual.1) -------
 * One workgroup per channel, two passes over the channel (mean, then sum (x-mean)^2: no E[x^2]-mean^2
 * cancellation).  kg_bn_fwd writes coef (4, C) = [scale, shift, mean, rstd] with
 *     rstd = 1/sqrt(var_biased + eps), scale = gamma*rstd, shift = beta - mean*scale
 * so that BN(x) = x*scale + shift is applied by kg_affine_act, and in training mode updates
 * running_mean / running_var (unbiased variance, momentum) and increments num_batches_tracked exactly as
 * torch.nn.BatchNorm2d does.  training = 0: no reduction, mean/var are the running statistics.
 * kg_bn_bwd: from g (= dL/d(BN output)) and the BN input x it writes coef (5, C) = [a, b, c, dgamma, dbeta]:
 *     dgamma = sum g*(x-mean)*rstd, dbeta = sum g,
 *     training: dL/dx = a*g + b*x + c with a = gamma*rstd, b = -a*rstd*dgamma/n, c = -a*dbeta/n - b*mean
 *     eval    : dL/dx = a*g            with a = gamma*rstd (b = c = 0)
 * (applied by kg_affine_act: out = g*a + c + x*b).  Replaces ~17 / ~11 per-channel-vector launches.   */
typedef struct KgBnArgs {
    int32_t N, C, T, V;
    const float* x;  int64_t x_sN, x_sC;
    const float* g;  int64_t g_sN, g_sC;       /* bwd only                                             */
    const float* gamma; const float* beta;     /* (C) or NULL (= 1 / 0)                                */
    float* running_mean; float* running_var;   /* (C) or NULL; updated by fwd in training mode         */
    int64_t* num_batches_tracked;              /* or NULL; += 1 by fwd in training mode                */
    const float* mean; const float* rstd;      /* bwd only: the statistics kg_bn_fwd used              */
    float momentum, eps;                       /* fwd: momentum < 0 = torch's momentum=None (cumulative moving
                                                  average: factor 1 / num_batches_tracked incl. this batch, formed
                                                  on the device from the live counter)                            */
    int32_t training;
    float* coef;                               /* fwd (4, C); bwd (5, C)                               */
} KgBnArgs;

int kg_bn_fwd(const KgBnArgs* a, void* stream);
int kg_bn_bwd(const KgBnArgs* a, void* stream);

/* Training-mode statistics of up to 4 BatchNorm layers in ONE launch, each over `groups` independent batches stacked
 * along N (a.N = samples PER batch; batch q = samples [q N, (q+1) N) of a.x): a.coef is (groups, 4, C), the running
 * statistics take the batches' updates in order, num_batches_tracked += groups - the same results as `groups`
 * kg_bn_fwd calls per layer (generator.py:142,160 on the two syntheses of a WGAN-GP iteration, kinetic-gan.py:143,167).
 * `counters`: >= sum of C zeroed int32, left zeroed (a channel's counter is zero again from the moment its last ticket
 * is drawn).                                                                                          */
typedef struct KgBnJob {
    KgBnArgs a;
    int32_t groups;
} KgBnJob;

/* the backward sums of up to 4 layers (kg_bn_bwd arguments each, coef (5, C)) in one launch; chunked partial sums,
 * the last workgroup of a channel finishes (`counters` as above)                                                    */
int64_t kg_bn_bwd_many_workspace_bytes(const KgBnArgs* jobs, int32_t njobs);
int     kg_bn_bwd_many(const KgBnArgs* jobs, int32_t njobs, float* ws, int64_t ws_bytes, int32_t* counters,
                       int32_t counters_len, void* stream);
int64_t kg_bn_fwd_many_workspace_bytes(const KgBnJob* jobs, int32_t njobs);
int     kg_bn_fwd_many(const KgBnJob* jobs, int32_t njobs, float* ws, int64_t ws_bytes, int32_t* counters,
                       int32_t counters_len, void* stream);

/* ---- WGAN-GP gradient penalty (kinetic-gan.py:112-113) --------------------------------------------------------
 *   kg_gp_fwd: nrm[n] = |g_n|_2 over (c, t, v);  gp[0] = mean_n (nrm[n] - 1)^2
 *   kg_gp_bwd: out = g * (2/N) * (1 - 1/nrm[n]) * gout[0]      (0 where nrm[n] == 0; gout: upstream gradient, device)
 * Replaces gradients.view(N,-1).norm(2, dim=1), (norm - 1)**2, .mean() and their autograd backward (~25 launches). */
typedef struct KgGpArgs {
    int32_t N, C, T, V;
    const float* g;  int64_t g_sN, g_sC;
    float* nrm;                         /* (N)  written by fwd, read by bwd                            */
    float* gp;                          /* (1)  fwd                                                    */
    const float* gout;                  /* (1)  bwd                                                    */
    float* out;  int64_t o_sN, o_sC;    /* bwd: (N, C, T, V) plane tensor                              */
} KgGpArgs;

int kg_gp_fwd(const KgGpArgs* a, void* stream);
int kg_gp_bwd(const KgGpArgs* a, void* stream);

/* ---- flat-buffer Adam (kinetic-gan.py:77-78: Adam(lr, betas=(b1,b2)), eps 1e-8, no weight decay) --
 * p, g, m, v are flat fp32 buffers of n elements; *step (device memory, so that a captured
 * hipGraph replays with the live value) is the 1-based step count.
 * grad_scale multiplies g first (1/world_size after the RCCL sum).                               */
int kg_adam_step(float* p, const float* g, float* m, float* v, int64_t n,
                 float lr, float b1, float b2, float eps, const int32_t* step, float grad_scale,
                 void* stream);
/* The same step with the loop's zero_grad() folded in (ABI v9; kinetic-gan.py:137,157): with zero_grad != 0 every gradient
 * element is set to 0 once it has been consumed - the next backward pass accumulates into a clean bucket without a fill
 * launch.  (*step stays the caller's 1-based count: advancing it inside the launch needed a ticket per workgroup, ~900
 * same-address atomics = 15 us, against 2 us for the `step += 1` launch.)                                              */
int kg_adam_step_fused(float* p, float* g, float* m, float* v, int64_t n,
                       float lr, float b1, float b2, float eps, const int32_t* step, float grad_scale,
                       int32_t zero_grad, void* stream);
/* The same step with an exponential moving average of the parameters riding on the launch (still ABI v9): e is a fifth flat
 * buffer of n elements; the thread that has computed p_new also writes  e <- e + (1 - beta_s) (p_new - e)  with
 * beta_s = ema_decay when ema_warmup == 0, else min(ema_decay, (1 + s) / (ema_warmup + s)), s = *step read from device
 * memory (a replayed graph follows the ramp).  p, g, m, v come out bit for bit as from kg_adam_step_fused (zero_grad != 0)
 * or kg_adam_step (zero_grad == 0).  128-bit accesses when all FIVE buffers are 16-byte aligned.  0 <= ema_decay < 1,
 * ema_warmup >= 0.                                                                                                      */
int kg_adam_step_ema(float* p, float* g, float* m, float* v, float* e, int64_t n,
                     float lr, float b1, float b2, float eps, const int32_t* step, float grad_scale,
                     int32_t zero_grad, float ema_decay, float ema_warmup, void* stream);

/* ---- container-level fusions around the discriminator's blocks ---------------------------------------
 * kg_head_fwd   : v[n] = b + sum_c w[c] * mean_{t,v} h[n,c,t,v]           global average pool + Linear(latent, 1)
 *                                                                         (discriminator.py:68-72)
 * kg_head_bwd   : g[n,c,t,v] = gv[n] * w[c] / (T V) * (masked ? lrelu'(h[n,c,t,v]) : 1)
 *                 the backward pass's top gradient for d loss / d v = gv, with the last block's LeakyReLU derivative
 *                 (expressed on its output h, discriminator.py:136) already applied when `masked`
 * kg_head_wgrad : dw[c] (+)= sum_n gv[n] * mean_{t,v} h[n,c,t,v],  db (+)= sum_n gv[n]
 *                 (h = the last block's output for the Linear's first-order gradient, or the double backward's
 *                  cotangent of the top gradient: the WGAN-GP penalty differentiates gv * w / (T V) w.r.t. w)        */
typedef struct KgHeadArgs {
    int32_t N, C, T, V;
    const float* h;  int64_t h_sN, h_sC;
    const float* w;  const float* b;        /* (C), (1) or NULL                                                */
    float* v;                               /* fwd: (N)                                                        */
    const float* gv;                        /* bwd / wgrad: (N)                                                */
    float* g;  int64_t g_sN, g_sC;          /* bwd: (N, C, T, V) plane tensor                                  */
    float slope;  int32_t masked;
    float* dw;  float* db;  int32_t accumulate;   /* wgrad: (C), (1) or NULL                                   */
} KgHeadArgs;
int kg_head_fwd(const KgHeadArgs* a, void* stream);
int kg_head_bwd(const KgHeadArgs* a, void* stream);
int kg_head_wgrad(const KgHeadArgs* a, void* stream);

/* The label channels of discriminator block 0 (discriminator.py:57-60: the class embedding, broadcast over (t, v) and
 * concatenated in FRONT of x) are constant over (t, v): through the gcn (tgcn.py:61-66) they contribute a per-sample
 * bias   zl[n,c,w] = sum_k S[k,w] * sum_j Wc(k,c,j) E[label_n, j],   S[k,w] = sum_v ak[k,v,w]
 * with Wc(k,c,j) = w + k*w_sK + c*w_sC + j the first J input columns of the gcn weight and ak (K, V, W) the block's
 * masked kept-column adjacency - the (N, J, T, V) label planes are never built.
 * kg_label_bias_bwd (first order; gz (N, C, T, W) = gradient of the gcn output): demb[l,j] (+)= ..., dw (same addressing
 * as w) (+)= ..., dak[k,v,w] (+)= dS[k,w] for every v; NULL outputs are skipped.  Both directions work per CLASS first
 * (the bias depends on a sample only through its class) and keep those records in `ws`
 * (kg_label_bias_workspace_bytes); deterministic (a class's samples are visited in index order).                     */
typedef struct KgLabelBiasArgs {
    int32_t N, L, J, K, C, V, W, T;
    const int64_t* labels;                  /* (N) class of every sample                                       */
    const float* emb;                       /* (L, J) label_emb.weight                                         */
    const float* w;  int64_t w_sK, w_sC;
    const float* ak;                        /* (K, V, W)                                                       */
    float* zl;                              /* fwd: (N, C, W) contiguous                                       */
    const float* gz;  int64_t gz_sN, gz_sC; /* bwd: (N, C, T, W) plane tensor                                  */
    float* demb;  float* dw;  int32_t accumulate;
    float* dak;  int32_t dak_accumulate;
    float* ws;  int64_t ws_bytes;
} KgLabelBiasArgs;
int     kg_label_bias_fwd(const KgLabelBiasArgs* a, void* stream);
int64_t kg_label_bias_workspace_bytes(const KgLabelBiasArgs* a);
int     kg_label_bias_bwd(const KgLabelBiasArgs* a, void* stream);
/* kg_aggconv_label: block 0's gcn with its label bias in ONE launch - the output of
 *     kg_label_bias_fwd(lb) -> zl;  kg_aggconv(a with add = zl, a_sN = C*W, a_sC = W, a_tstride = 0)
 * without the zl tensor, the workspace or the class-table launch (discriminator.py:57-60, tgcn.py:58-68): every
 * workgroup forms the bias of its sample's class from lb->emb, the label columns lb->w and the column sums of a->a
 * (lb->ak, lb->zl and lb->ws are not read).  Tiny-channel geometry only (K <= 3, Cin <= 4, M <= 64, W <= 32, K*V*W <= 4096;
 * K*M*J <= 12288, J <= 512); a->add must be NULL; lb->{N, K, C, V, W} must equal a->{N, K, M, V, W}.  A label outside
 * [0, L) turns that sample's output into NaN.  The aggregated planes are written when a->xa is given.               */
int     kg_aggconv_label(const KgAggConvArgs* a, const KgLabelBiasArgs* lb, void* stream);

/* kg_mix3: out (3N, C, T, V) = [real | fake | alpha[n] real + (1 - alpha[n]) fake] - the three batches the critic step
 * runs D on (kinetic-gan.py:97-99,146-148) as one tensor.                                                            */
typedef struct KgMixArgs {
    int32_t N, C, T, V;
    const float* real;  int64_t r_sN, r_sC;
    const float* fake;  int64_t f_sN, f_sC;
    const float* alpha;                     /* (N)                                                             */
    float* out;  int64_t o_sN, o_sC;        /* (3N, C, T, V)                                                   */
} KgMixArgs;
int kg_mix3(const KgMixArgs* a, void* stream);

/* kg_masked_adj_fwd: ak[i] = a[s] * imp[s], s = sel ? sel[i] : i, i < n   (discriminator.py:63-64 / generator.py:92-93:
 * A[lvl] * edge_importance of ALL blocks, flattened and concatenated, restricted to the kept columns through `sel`)
 * kg_masked_adj_bwd: dimp[s] (+)= g[i] * a[s]   (sel injective: every element has one writer)                        */
typedef struct KgMaskedAdjArgs {
    int32_t n;
    const float* a;  const float* imp;  const int64_t* sel;
    float* ak;
    const float* g;  float* dimp;  int32_t accumulate;
} KgMaskedAdjArgs;
int kg_masked_adj_fwd(const KgMaskedAdjArgs* a, void* stream);
int kg_masked_adj_bwd(const KgMaskedAdjArgs* a, void* stream);

/* ---- label embedding + mapping network of the generator (generator.py:22-37 Mapping_Net, :80-85) -----------------------
 * nn.Linear(D, D) + LeakyReLU(0.2), mlp_dim times, on the (N, D) latents of a step; D = latent + n_classes.
 *   kg_linear_fwd : y[n,o] = act( sum_i xin[n,i] w[o,i] + bias[o] )
 *                   xin[n, :] = [ emb[labels[n], 0:J) | x[n, 0:Din-J) ]: the nn.Embedding lookup and torch.cat of
 *                   generator.py:80-82 folded into the FIRST layer's operand load (J = 0: xin = x); a label outside [0, L)
 *                   makes its sample NaN (nn.Embedding raises)
 *   kg_linear_bwd : with g' = g * act'(y) (the LeakyReLU derivative expressed on the layer's output y):
 *                   gx[n, i] = sum_o g'[n,o] w[o,i]  for i < gx_cols (the first layer needs the J embedding columns only,
 *                   0 = no input gradient);  dw[o,i] (+)= sum_n g'[n,o] xin[n,i];  db[o] (+)= sum_n g'[n,o]   (NULL = skip);
 *                   one launch
 *   kg_embed_bwd  : demb[l, j] (+)= sum_{n: labels[n] = l} gx[n, j], j < J  (aten::embedding_dense_backward; samples in
 *                   index order)
 * w: (Dout, Din) contiguous (nn.Linear.weight); x, y, g, gx: row-major with leading dimensions *_ld (floats).
 * Replaces per layer: aten::addmm + leaky_relu forward; leaky_relu_backward + mm (input) + mm (weight) + sum (bias) + the
 * accumulation adds backward; plus embedding, cat and embedding_dense_backward once.                                   */
typedef struct KgLinearArgs {
    int32_t N, Din, Dout;
    int32_t L, J;                           /* embedding table rows / columns folded into xin (J = 0: none)              */
    const float* x;  int64_t x_ld;          /* (N, Din - J)                                                              */
    const float* emb;                       /* (L, J) label_emb.weight or NULL                                           */
    const int64_t* labels;                  /* (N) or NULL                                                               */
    const float* w;  const float* bias;     /* (Dout, Din), (Dout) or NULL                                               */
    float* y;  int64_t y_ld;                /* fwd: output (N, Dout); bwd: the forward output (read)                     */
    int32_t act;  float slope;              /* KG_ACT_NONE or KG_ACT_LRELU                                               */
    const float* g;  int64_t g_ld;          /* bwd: (N, Dout) gradient of y                                              */
    float* gx;  int64_t gx_ld;  int32_t gx_cols;   /* bwd: (N, gx_cols) or NULL / 0; kg_embed_bwd: its input             */
    float* dw;  float* db;                  /* bwd: (Dout, Din), (Dout) or NULL                                          */
    float* demb;                            /* kg_embed_bwd: (L, J)                                                      */
    int32_t accumulate;                     /* 0: dw / db / demb = result, 1: += (flat gradient bucket)                  */
} KgLinearArgs;
int kg_linear_fwd(const KgLinearArgs* a, void* stream);
int kg_linear_bwd(const KgLinearArgs* a, void* stream);
int kg_embed_bwd(const KgLinearArgs* a, void* stream);

/* ---- data-parallel gradient exchange over RCCL / xGMI -------------------------------------------------
 * One process per GPU; every rank holds full replicas and, per optimiser step (kinetic-gan.py:155,174), the ranks' flat
 * fp32 gradient buckets are summed in place by ONE all-reduce; kg_adam_step's grad_scale = 1 / world averages them.
 * The reference has no distributed code: this is what a data-parallel launcher of its loop binds instead of
 * torch.distributed.  RCCL is dlopen'ed on first use (no link-time dependency).
 *   kg_comm_unique_id : rank 0 fills `id` (KG_COMM_ID_BYTES bytes) and ships it to the other ranks by any side channel
 *   kg_comm_init      : collective over all ranks; binds the communicator to HIP device `device`; *comm = opaque handle
 *   kg_allreduce_flat : buf[0..n) <- sum over ranks, in place, enqueued on `stream` (capturable into a hipGraph)
 *   kg_comm_destroy   : releases the communicator (NULL is a no-op)                                                    */
#define KG_COMM_ID_BYTES 128
int kg_comm_unique_id(void* id);
int kg_comm_init(void** comm, int32_t rank, int32_t world, const void* id, int32_t device);
int kg_comm_world(const void* comm);
int kg_allreduce_flat(void* comm, float* buf, int64_t n, void* stream);
int kg_comm_destroy(void* comm);

/* ---- measured peaks ("use measured peaks as denominators"; ABI v7) ----------------------------------------
 * Two probe launches bench.py times next to every roofline leg, so that the clock the chip really holds in launches of
 * that length is on the benchmark line and not in prose (the reference has no counterpart):
 *   kg_peak_mfma_f32 : every wave of a full grid (four workgroups of four waves per CU) issues `iters` x 16 independent
 *                      v_mfma_f32_32x32x2_f32 on N(0,1)-like operands; *flops (host, optional) = the flops of the launch.
 *                      `sink` (>= 64 floats, device) receives a value that keeps the loop alive.
 *   kg_peak_copy     : dst[i] = src[i], i < n, 16 bytes per lane, grid-stride (the "float4 copy" of the hardware guide);
 *                      n multiple of 4, both pointers 16-byte aligned; moves 8 n bytes.                                    */
int kg_peak_mfma_f32(float* sink, int32_t iters, double* flops, void* stream);
int kg_peak_copy(const float* src, float* dst, int64_t n, void* stream);

/* ---- MMD evaluation (evaluation/mmd-actions.py:79-115; additive, ABI v9) -------------------------------------------
 * For every group g of every class c: X_g, Y_g are m points of dimension `dim`, read through strides (elements):
 *   X_g[i][d] = x + c*x_sc + f*x_sg + i*x_sp + d*x_sd      (f < groups: the group's index inside its class)
 * and likewise Y_g.  For every bandwidth bw[b] (k(a, b') = exp(-|a - b'|^2 / bw)):
 *   mmd2[(c*groups + f)*nbw + b] = sum_{i != j} [k(x_i, x_j) + k(y_i, y_j) - 2 k(x_i, y_j)] / (m (m - 1))
 *   mmd[c*nbw + b]               = (1/groups) sum_f sqrt(mmd2)    (NaN from a negative MMD^2 or m = 1, as torch's pow(0.5))
 *   result[c]                    = r, r = 0 replaced by mmd[c, b] whenever mmd[c, b] > r (b ascending; NaN never wins)
 *   mean (optional)              = (1/classes) sum_c result[c]
 * The reference protocol reads the feeder's (N, C, T, V) tensor directly: point = v (x_sp = 1), dimension = c
 * (x_sd = T*V), group = frame t (x_sg = V), class = one sample (x_sc = sample stride) in `avg` mode, and point = v,
 * dimension = (c, t) (x_sd = V, dim = C*T, groups = 1) in `joint` mode.  One launch computes the pair sums of every
 * (group, bandwidth) (tiles of the pair space, fp32 partial sums per tile, no Gram matrix is written) and one
 * single-workgroup launch finishes: tile partials combined in fp64 in a fixed order - two calls on the same input give
 * the same bits.  ws: kg_mmd_workspace_bytes(a) bytes of scratch.  m != n, m < 1, dim < 1, nbw outside [1, 16], a
 * bandwidth <= 0, a null pointer or a small workspace are rejected (< 0, kg_last_error() names the field).            */
#define KG_MMD_MAX_BW 16
typedef struct KgMmdArgs {
    const float* x;  int64_t x_sp, x_sd, x_sg, x_sc;   /* point, dimension, group and class strides (elements)    */
    const float* y;  int64_t y_sp, y_sd, y_sg, y_sc;
    int32_t m, n, dim;              /* points of X and Y (must be equal), dimension                                  */
    int32_t groups, classes;        /* groups per class (frames in avg mode, 1 in joint), classes                  */
    int32_t nbw;                    /* bandwidths used, 1..KG_MMD_MAX_BW                                           */
    double bw[KG_MMD_MAX_BW];
    float* mmd2;                    /* (classes*groups, nbw)                                                       */
    float* mmd;                     /* (classes, nbw)                                                              */
    float* result;                  /* (classes)                                                                   */
    float* mean;                    /* (1) or NULL                                                                 */
    void* ws;  int64_t ws_bytes;
} KgMmdArgs;
int64_t kg_mmd_workspace_bytes(const KgMmdArgs* a);   /* < 0 for invalid shapes                                    */
int     kg_mmd(const KgMmdArgs* a, void* stream);

/* ---- precision / recall / density / coverage (additive, ABI v9; DESIGN.md 16, csrc/kg_prdc.hip) -----------------------
 * For every class c: R = n real points, F = m fake points of dimension D = d_outer*d_inner, read through strides (elements):
 *   r_i[(o, e)] = real + c*r_sc + i*r_sp + o*r_so + e      (o < d_outer, e < d_inner: the inner run is contiguous)
 * and likewise f_j.  With d2(a, b) = sum_d (a_d - b_d)^2 (direct differences in fp32, d ascending: the same bits per call):
 *   rho_R(i) = the k-th smallest of { d2(r_i, r_l) : l != i }     (left out by INDEX: a duplicate is a neighbour at 0)
 *   rho_F(j) = the k-th smallest of { d2(f_j, f_l) : l != j }
 *   P_ij = [d2(r_i, f_j) <= rho_R(i)],  Q_ij = [d2(r_i, f_j) <= rho_F(j)]        (ties are inside)
 *   counts[c] = (cP, cR, cD, cC) = (#{j : exists i P_ij}, #{i : exists j Q_ij}, sum_ij P_ij, #{i : exists j P_ij})
 *   values[c] = (precision, recall, density, coverage) = (cP / m, cR / n, cD / (k m), cC / n)   (in double, rounded once)
 *   mean (optional) = the mean over classes of values (fp64 sum in class order, rounded once)
 * A sample (C, T, V) cropped in T is d_outer = C, d_inner = t*V, r_so = the channel stride; a contiguous one d_outer = 1.
 * Three launches: radii (which also clears the words the next launch accumulates into: ws may hold anything), cross
 * (integer atomics: order-independent, so two calls give the same bits), finish (one workgroup).  No n x n or n x m matrix
 * is written: ws is kg_prdc_workspace_bytes(a) = 8 classes (n + m) bytes (radii and flag / hit words; no tile partials).
 * Every pointer is read when the launches run; nothing is synchronised; capturable on one stream.
 * Rejected (< 0, kg_last_error() names the field): null real / fake / counts / values / ws; n, m, classes, d_outer or
 * d_inner < 1; k < 1, k > KG_PRDC_MAX_K or k > min(n, m) - 1; n or m above KG_PRDC_MAX_POINTS; classes x tiles of 2^24
 * workgroups or more in one launch (first met at 64 classes of 32768 x 32768 points); ws_bytes too small.                */
#define KG_PRDC_MAX_K 32
#define KG_PRDC_MAX_POINTS 32768    /* per class and set: n*m stays below 2^31 (cD is an int32)                           */
typedef struct KgPrdcArgs {
    const float* real;  int64_t r_sc, r_sp, r_so;   /* class, point, outer-dimension strides (elements)                   */
    const float* fake;  int64_t f_sc, f_sp, f_so;
    int32_t n, m;                   /* real / fake points per class (n != m allowed)                                   */
    int32_t d_outer, d_inner;       /* D = d_outer*d_inner; element (o, e) at + o*so + e                                */
    int32_t classes, k;
    float* radii_real;              /* (classes, n) squared radii, or NULL (kept in ws only)                           */
    float* radii_fake;              /* (classes, m) or NULL                                                            */
    int32_t* fake_hits;             /* (classes, m): sum_i P_ij (precision flag = hits > 0), or NULL                   */
    uint8_t* real_flags;            /* (classes, n): bit 0 = exists j Q_ij (recall), bit 1 = exists j P_ij (coverage), or NULL */
    int32_t* counts;                /* (classes, 4): cP, cR, cD, cC                                                    */
    float* values;                  /* (classes, 4): precision, recall, density, coverage                              */
    float* mean;                    /* (4) or NULL                                                                     */
    void* ws;  int64_t ws_bytes;
} KgPrdcArgs;
int64_t kg_prdc_workspace_bytes(const KgPrdcArgs* a);   /* < 0 for invalid shapes                                    */
int     kg_prdc(const KgPrdcArgs* a, void* stream);

/* ---- several fake sets against ONE real set whose radii are given (additive, ABI v9; DESIGN.md 17, csrc/kg_prdc.hip) --------
 * The Evaluator's case: the real set is fixed for a whole run and every named generator is scored against it.
 * kg_prdc_radii: rho(i) of ONE point set alone, as defined above (k-th smallest d2 to the other points of its class, left
 * out by index), read through the strides of kg_prdc (x + c*sc + i*sp + o*so + e), written to radii (classes, n).  ONE
 * launch of the radii kernel restricted to that set; no workspace.  Rejected: null x / radii; n, classes, d_outer or
 * d_inner < 1; k < 1, k > KG_PRDC_MAX_K or k > n - 1; n above KG_PRDC_MAX_POINTS; 2^24 workgroups or more.
 * kg_prdc_sets: nsets (1..KG_PRDC_MAX_SETS) fake sets fake[g] with shared strides and m, one real set, and the real set's
 * radii as an INPUT (radii_real (classes, n), read when the launches run).  For every set g every output - counts[g],
 * values[g], mean[g], radii_fake[g], fake_hits[g], real_flags[g] - equals, bit for bit, the same output of
 * kg_prdc(real, fake[g]) given radii_real as kg_prdc computes it: every pair is the same fmaf chain over d ascending, the
 * counts are integers, and neither the tile plan nor the grouping into sets shows in any bit.
 * Three launches whatever nsets is: radii of all fake sets (row-tile workgroups for fake rows only; it clears the words
 * the next launch accumulates into, so ws may hold anything), cross counts of every (set, class, tile) (vector integer
 * atomics), finish (a wave per (set, class), then the class means).  No n x n or n x m matrix is written.
 * ws = kg_prdc_sets_workspace_bytes(a) = 4 nsets classes (2 m + n) bytes: the fake radii (nsets, classes, m) fp32, the hit
 * words (nsets, classes, m) int32, the per-set flag words (nsets, classes, n) int32.
 * Every pointer is read when the launches run; nothing is synchronised; capturable on one stream.
 * Rejected (< 0, kg_last_error() names the field): null real / fake[g] / radii_real / counts / values / ws; nsets outside
 * [1, KG_PRDC_MAX_SETS]; n, m, classes, d_outer or d_inner < 1; k < 1, k > KG_PRDC_MAX_K or k > min(n, m) - 1; n or m above
 * KG_PRDC_MAX_POINTS; nsets x classes x tiles of 2^24 workgroups or more in one launch; ws_bytes too small.                */
#define KG_PRDC_MAX_SETS 4
typedef struct KgPrdcRadiiArgs {
    const float* x;  int64_t sc, sp, so;            /* class, point, outer-dimension strides (elements)                  */
    int32_t n, d_outer, d_inner, classes, k;
    float* radii;                   /* (classes, n) squared radii                                                      */
} KgPrdcRadiiArgs;
typedef struct KgPrdcSetsArgs {
    const float* real;  int64_t r_sc, r_sp, r_so;
    const float* fake[KG_PRDC_MAX_SETS];  int64_t f_sc, f_sp, f_so;   /* fake[0 .. nsets): strides and m are shared        */
    int32_t nsets;
    int32_t n, m;
    int32_t d_outer, d_inner;
    int32_t classes, k;
    const float* radii_real;        /* (classes, n): INPUT (kg_prdc_radii of the real set, or radii_real of kg_prdc)   */
    float* radii_fake;              /* (nsets, classes, m) or NULL                                                     */
    int32_t* fake_hits;             /* (nsets, classes, m) or NULL                                                     */
    uint8_t* real_flags;            /* (nsets, classes, n) or NULL                                                     */
    int32_t* counts;                /* (nsets, classes, 4)                                                             */
    float* values;                  /* (nsets, classes, 4)                                                             */
    float* mean;                    /* (nsets, 4) or NULL                                                              */
    void* ws;  int64_t ws_bytes;
} KgPrdcSetsArgs;
int     kg_prdc_radii(const KgPrdcRadiiArgs* a, void* stream);
int64_t kg_prdc_sets_workspace_bytes(const KgPrdcSetsArgs* a);   /* < 0 for invalid shapes                           */
int     kg_prdc_sets(const KgPrdcSetsArgs* a, void* stream);

/* ---- exact k nearest neighbours between two point sets (additive, ABI v9; DESIGN.md 22, csrc/kg_nn.hip) -------------------
 * For every class c: Q query points and N base points of dimension D = d_outer*d_inner, read through strides (elements) as
 * kg_prdc reads its sets:
 *   q_i[(o, e)] = f_q(query + c*q_sc + i*q_sp + o*q_so + e)     (o < d_outer, e < d_inner: the inner run is contiguous)
 * and likewise b_j with f_b.  f is the identity, or with q_affine / b_affine != 0 the affine (x * scale) + shift in two
 * separately rounded fp32 operations (no FMA: the arithmetic of kg_step_inputs) - an unnormalised array searched in place
 * gives the bits of the normalised one.  With d2(a, b) = sum_d (a_d - b_d)^2 (direct differences in fp32, one fmaf per
 * dimension, d ascending: the chain of kg_prdc, never |a|^2 + |b|^2 - 2ab, so near-copies do not cancel):
 *   (d2[c, i, r], idx[c, i, r]), r < k = the k smallest of { (d2(q_i, b_j), j) : j < N, j != i if exclude_self } in the
 *   total order (d2, j) ascending: ties go to the lower base index, a duplicate is a neighbour at distance 0.
 * exclude_self leaves pair i == j out by INDEX (one set searched against itself: query and base name the same points).
 * Two launches: search (a workgroup = one class x a row tile of `tile` queries x one of `split` chunks of base points; the
 * k best (d2, j) of every row are kept in LDS and written to ws), merge (a wave per query ranks its split * k candidates).
 * No atomics, no tickets, no Q x N matrix.  tile (0 automatic, 32, 64) and split (0 automatic, else that many chunks of
 * ceil(N / split) points, at most KG_NN_MAX_SPLIT and N) only choose the plan: every plan gives the same bits.
 * ws is kg_nn_workspace_bytes(a) = classes * Q * split * k * 8 bytes (split: the plan's) and may hold anything.
 * Every pointer is read when the launches run; nothing is synchronised; capturable on one stream.
 * Rejected (< 0, kg_last_error() names the field): null query / base / idx / d2 / ws; Q, N, classes, d_outer or d_inner < 1;
 * Q or N above KG_NN_MAX_POINTS; k < 1, k > KG_NN_MAX_K or k > N - (exclude_self ? 1 : 0); tile not 0 / 32 / 64; split
 * outside [0, min(KG_NN_MAX_SPLIT, N)]; 2^24 workgroups or more in one launch; ws_bytes too small.                         */
#define KG_NN_MAX_K 32
#define KG_NN_MAX_POINTS 16777216   /* per class and side (2^24); no count is formed, so there is no n*m bound as in PRDC    */
#define KG_NN_MAX_SPLIT 32
typedef struct KgNnArgs {
    const float* query;  int64_t q_sc, q_sp, q_so;  /* class, point, outer-dimension strides (elements)                   */
    const float* base;   int64_t b_sc, b_sp, b_so;
    int32_t Q, N;                   /* query / base points per class                                                   */
    int32_t d_outer, d_inner;       /* D = d_outer*d_inner; element (o, e) at + o*so + e                                */
    int32_t classes, k;
    int32_t exclude_self;           /* != 0: pair i == j is left out by index                                          */
    int32_t q_affine, b_affine;     /* != 0: that side is read as (x * scale) + shift                                  */
    float q_scale, q_shift, b_scale, b_shift;
    int32_t tile, split;            /* 0 = automatic, or a forced plan (tests)                                         */
    int32_t* idx;                   /* (classes, Q, k): base index inside the class                                    */
    float* d2;                      /* (classes, Q, k): squared distances, non-decreasing along k                      */
    void* ws;  int64_t ws_bytes;
} KgNnArgs;
int64_t kg_nn_workspace_bytes(const KgNnArgs* a);   /* < 0 for invalid shapes                                          */
int     kg_nn(const KgNnArgs* a, void* stream);

/* ---- several query sets against ONE base; memorisation score words (additive, ABI v9; DESIGN.md 23, csrc/kg_nn.hip) --------
 * The Evaluator's case: the training set is the base for a whole run and every named generator's round is a query set.
 * kg_nn_sets: nsets (1..KG_NN_MAX_SETS) query sets query[g] with shared strides, Q and affine against one base.  For every
 * set g, idx[g] and d2[g] equal, bit for bit, what kg_nn(query[g], base) writes on the same data, under every (tile, split)
 * plan of either call: a set only chooses the query pointer and the output rows - neither the plan nor the grouping into
 * sets shows in any bit.  There is no exclude_self: a group of sets searched against one base has no "self".
 * Two launches whatever nsets is - the kernels of kg_nn, of which kg_nn is the one-set case: a search workgroup is one
 * (set, class, row tile, chunk), a merge wave one (set, class, query).  The automatic plan counts the sets as row tiles: the
 * tile is 64 once nsets * classes * ceil(Q / 64) * min(32, ceil(N / 64)) >= 512, and the chunks make up what
 * nsets * classes * row tiles lack of 512 workgroups - fewer, longer chunks than one set gets.
 * ws = kg_nn_sets_workspace_bytes(a) = nsets * classes * Q * split * k * 8 bytes (split: the plan's) and may hold anything.
 * Every pointer is read when the launches run; nothing is synchronised; capturable on one stream.
 * Rejected (< 0, kg_last_error() names the field): nsets outside [1, KG_NN_MAX_SETS]; null query[g] (g < nsets) / base /
 * idx / d2 / ws; every rule of kg_nn but the exclude_self ones (k > N); nsets * classes * row tiles * split or
 * ceil(nsets * classes * Q / 4) of 2^24 workgroups or more; ws_bytes too small.
 *
 * kg_nn_scores: from the nearest neighbour (idx, d2) of every query of nsets sets to the memorisation tallies of
 * metrics.memorisation.  idx / d2 are (nsets, Q) with the element stride ld (set g, query j at g*Q*ld + j*ld: column 0 of a
 * (nsets, 1, Q, k) result of kg_nn_sets is ld = k, read in place).  Per set g and query j, with i = idx[g][j]:
 *   authentic_j = d2[g][j] >= base_loo[i]          (>=: equality is authentic; base_loo (N): the leave-one-out nearest
 *                                                   squared distance of every base point - d2 of kg_nn(base, base,
 *                                                   k = 1, exclude_self))
 *   agree_j     = base_labels[i] == query_labels[j]
 *   counts (nsets, 2) int64 = #authentic, #agreeing;   counts_per_class (nsets, n_classes, 2) int32 (or NULL) the same by
 *   the QUERY's label;   scores64 (nsets, 2) = counts / Q evaluated in fp64;   scores (nsets, 2) = its one fp32 rounding.
 * ONE launch, one workgroup per set: integer tallies in LDS, no atomics on global memory, one owner per output word, every
 * word written on every call - the same bits on every call.  Nothing is synchronised; capturable.
 * Outside the definition, and never out of bounds: a query whose idx is outside [0, N) is SKIPPED (nothing is read for it,
 * it counts nowhere); a query label outside [0, n_classes) counts in `counts` and in no class.
 * Rejected (< 0, kg_last_error() names the field): null idx / d2 / query_labels / base_labels / base_loo / counts /
 * scores64 / scores; Q, N, n_classes or ld < 1; nsets outside [1, KG_NN_MAX_SETS]; Q or N above KG_NN_MAX_POINTS; n_classes
 * above KG_NN_SCORES_MAX_CLASSES (the LDS tallies: 2 words per class).                                                   */
#define KG_NN_MAX_SETS 4
#define KG_NN_SCORES_MAX_CLASSES 1024
typedef struct KgNnSetsArgs {
    const float* query[KG_NN_MAX_SETS];  int64_t q_sc, q_sp, q_so;    /* query[0 .. nsets): strides, Q and affine are shared */
    int32_t nsets;
    const float* base;   int64_t b_sc, b_sp, b_so;
    int32_t Q, N;
    int32_t d_outer, d_inner;
    int32_t classes, k;
    int32_t q_affine, b_affine;
    float q_scale, q_shift, b_scale, b_shift;
    int32_t tile, split;            /* 0 = automatic, or a forced plan (tests)                                         */
    int32_t* idx;                   /* (nsets, classes, Q, k)                                                          */
    float* d2;                      /* (nsets, classes, Q, k)                                                          */
    void* ws;  int64_t ws_bytes;
} KgNnSetsArgs;
typedef struct KgNnScoresArgs {
    int32_t nsets, Q, N, n_classes;
    int64_t ld;                     /* elements between two queries of idx / d2                                        */
    const int32_t* idx;  const float* d2;           /* (nsets, Q) x ld                                                   */
    const int32_t* query_labels;    /* (Q), shared by the sets                                                         */
    const int32_t* base_labels;     /* (N)                                                                             */
    const float* base_loo;          /* (N)                                                                             */
    int64_t* counts;                /* out: (nsets, 2)                                                                 */
    int32_t* counts_per_class;      /* out: (nsets, n_classes, 2) or NULL                                              */
    double* scores64;  float* scores;               /* out: (nsets, 2), (nsets, 2)                                       */
} KgNnScoresArgs;
int64_t kg_nn_sets_workspace_bytes(const KgNnSetsArgs* a);   /* < 0 for invalid shapes                                 */
int     kg_nn_sets(const KgNnSetsArgs* a, void* stream);
int     kg_nn_scores(const KgNnScoresArgs* a, void* stream);

/* ---- matrix-core pre-filter with exact re-score for kg_nn (additive, ABI v9; DESIGN.md 24, csrc/kg_nn_gram.hip) ---------------
 * kg_nn_gram: the arguments of kg_nn_sets (plus exclude_self, which needs nsets == 1).  For every set g, idx[g] and d2[g]
 * equal, bit for bit, what kg_nn(query[g], base) writes on the same data: the k smallest under (d2, j), d2 the fp32
 * direct-difference fmaf chain in ascending dimension, the affine two roundings, exclude_self by index - for EVERY input of
 * that definition, data on which the Gram form |q|^2 + |b|^2 - 2 q.b loses all its digits included.  The Gram value is only a
 * filter:
 *   1 search   a workgroup = (set, class, row tile, chunk) as in kg_nn.  The tile of q.b comes from the fp32 matrix cores
 *              (v_mfma_f32_32x32x2f32 on LDS-staged operands; the accumulator restarts every 256 dimensions and the blocks
 *              are summed in order, so a pair's value depends on the two points alone).  key(i, j) = fma(-2, q_i.b_j, nb_j)
 *              with nb_j = b_norms[c, j]; each row keeps its `cand` smallest (key, j).
 *   2 merge    the merge of kg_nn with k = cand: the row's cand smallest (key, j) over all chunks.
 *   3 re-score every candidate's d2 from the chain of kg_nn (a wave per row, a lane per candidate); the candidates ordered by
 *              (d2, j), the first k are written.  With t the k-th of them and a the cand-th smallest key the row is
 *              CERTIFIED when   (1 - tau) * (a + nq * (1 - e_n) - E) - E_abs  >  t   (evaluated in fp64; nq the row's fp32
 *              squared norm, E = (e_n + 2 e_g + 4 u) * max(nq, max_j nb_j) * (1 + 2 e_n), u = 2^-24, tau = (D + 4) u,
 *              e_n = 1.01 (ceil(D / 64) + 8) u, e_g = 1.01 (min(D, 256) + ceil(D / 256) + 4) u, E_abs = (D + 16) 2^-120:
 *              DESIGN.md 24 derives it): no base point outside the candidates can enter the list or tie with it.  A row all
 *              of whose admissible base points are candidates (N - excluded <= cand) is certified as well.
 *   4 compact  the rows that are not certified, per (set, class) in row order, by a scan; stats.
 *   5, 6       the search and merge of kg_nn over the listed rows only (a grid sized for all rows, workgroups past the end
 *              of a list leave at once); their results overwrite those rows.
 * Six launches whatever the data; no host synchronisation, no atomics on global memory, capturable on one stream, the same
 * bits on every call; ws may hold anything.  stats (nsets, classes, 2) int32 is always written: certified rows, fallback
 * rows - the same under every (tile, split) plan (they depend on cand).
 * cand: 0 = automatic, min(32, max(k + 8, 2 k)); else k < cand <= KG_NN_MAX_K (tests).  k = KG_NN_MAX_K has no cand.
 * b_norms (classes, N) and b_norm_parts (classes, KG_NN_NORM_PARTS) are kg_nn_norms of the base, computed once for a base that
 * does not change.  ws = kg_nn_gram_workspace_bytes(a) = nsets * classes * (Q * (8 * cand * (split + 1) + 8) + 4) bytes.
 * Rejected (< 0, kg_last_error() names the field; all before any GPU call): every rule of kg_nn_sets; exclude_self with
 * nsets != 1 (and then k > N - 1); cand outside {0} u (k, KG_NN_MAX_K]; k = KG_NN_MAX_K; null b_norms / b_norm_parts / stats.
 *
 * kg_nn_norms: ONE launch - the fp32 squared norm of every BASE point of `a` (base, b_s*, N, d_outer, d_inner, classes, the
 * b_affine: no other field is read) into norms (classes, N), and the largest of them in KG_NN_NORM_PARTS parts per class into
 * parts (classes, KG_NN_NORM_PARTS): parts[c, p] = max over the points j = p mod KG_NN_NORM_PARTS (0 where there is none); the
 * class's largest norm is the largest of its parts (a workgroup owns one part: no atomics, no second launch).  A norm is one
 * fmaf chain per lane over the dimensions lane, lane + 64, .. and a butterfly sum of the 64 lanes.                         */
#define KG_NN_NORM_PARTS 64
typedef struct KgNnGramArgs {
    const float* query[KG_NN_MAX_SETS];  int64_t q_sc, q_sp, q_so;    /* query[0 .. nsets): strides, Q and affine are shared */
    int32_t nsets;
    const float* base;   int64_t b_sc, b_sp, b_so;
    int32_t Q, N;
    int32_t d_outer, d_inner;
    int32_t classes, k;
    int32_t exclude_self;           /* != 0: pair i == j is left out by index (nsets == 1)                               */
    int32_t q_affine, b_affine;
    float q_scale, q_shift, b_scale, b_shift;
    int32_t cand;                   /* 0 = automatic, or a forced number of candidates per row (tests)                   */
    int32_t tile, split;            /* 0 = automatic, or a forced plan (tests)                                           */
    const float* b_norms;           /* (classes, N): kg_nn_norms of the base                                            */
    const float* b_norm_parts;      /* (classes, KG_NN_NORM_PARTS)                                                      */
    int32_t* idx;                   /* (nsets, classes, Q, k)                                                           */
    float* d2;                      /* (nsets, classes, Q, k)                                                           */
    int32_t* stats;                 /* (nsets, classes, 2): certified rows, fallback rows                               */
    void* ws;  int64_t ws_bytes;
} KgNnGramArgs;
int     kg_nn_norms(const KgNnGramArgs* a, float* norms, float* parts, void* stream);
int64_t kg_nn_gram_workspace_bytes(const KgNnGramArgs* a);   /* < 0 for invalid shapes                                 */
int     kg_nn_gram(const KgNnGramArgs* a, void* stream);

/* ---- Frechet distance of pose / motion / caller features in fp64 (additive, ABI v9; DESIGN.md 18, csrc/kg_frechet.hip) -----
 * For every class c: a real set of n and a fake set of m samples of `frames` frames, a frame being d = d_outer*d_inner <= 96
 * floats read through strides (elements):
 *   x_(i, f)[(o, e)] = real + c*r_sc + i*r_ss + f*r_sf + o*r_so + e      (o < d_outer, e < d_inner: the inner run is contiguous)
 * and likewise the fake set.  The points of a set:
 *   diff = 0 (pose):    x_(i, f),                 f < frames       P = n frames
 *   diff = 1 (motion):  x_(i, f + 1) - x_(i, f),  f < frames - 1   P = n (frames - 1)     (the difference formed in fp64: exact)
 * An (N, d) feature matrix is frames = 1, d_outer = 1, d_inner = d.  With X in {real R, fake F}, everything in fp64:
 *   mu_X = the mean of the points,  S_X = their unbiased covariance (divided by P - 1)
 *   S_R = V diag(l) V^T,  l clamped at 0,  G = V diag(sqrt l)             (it is always the REAL covariance that is decomposed)
 *   H = sym(G^T S_F G),  e = the eigenvalues of H,  T = sum_i sqrt(max(e_i, 0))          (= tr sqrt(S_R S_F))
 *   terms[c] = (|mu_R - mu_F|^2, tr S_R, tr S_F, T),   values[c] = FD = ((terms0 + terms1) + terms2) - 2 T
 *   mean (optional) = the mean over classes of values (fp64 sum in class order)
 *   sweeps[c] = the Jacobi sweeps of the two eigen-problems (S_R, H), the last, rotation-free one included; at most 40
 * Four launches (three without mean): moments of chunks of points (centred on the set's first point, fp64 FMA chains in point
 * order), merge (chunks summed in chunk order: the chunking depends on the shape alone, so two calls give the same bits),
 * solve (one workgroup per class, both eigen-problems in LDS by cyclic Jacobi in the round-robin ordering, which depends on d
 * alone), mean.  No atomics, no ticket.  ws = kg_frechet_workspace_bytes(a) bytes, 8-byte aligned: chunk partials, then mu
 * (classes, 2, d) and S (classes, 2, d, d); its contents on entry do not matter.
 * Every pointer is read when the launches run; nothing is synchronised; capturable on one stream.
 * Rejected (< 0, kg_last_error() names the field) before any GPU call: null real / fake / values / terms / sweeps / ws;
 * classes, n, m, d_outer or d_inner < 1; diff not 0 or 1; d above KG_FRECHET_MAX_DIM; frames < 1 + diff; P < 2 or P > 2^24 in
 * either set; classes that need 2^24 workgroups or more in one launch; ws misaligned or ws_bytes too small.                */
#define KG_FRECHET_MAX_DIM 96
typedef struct KgFrechetArgs {
    const float* real;  int64_t r_sc, r_ss, r_sf, r_so;   /* class, sample, frame, outer-dimension strides (elements)    */
    const float* fake;  int64_t f_sc, f_ss, f_sf, f_so;
    int32_t n, m;                   /* real / fake samples per class (n != m allowed)                                  */
    int32_t frames;                 /* frames per sample                                                               */
    int32_t diff;                   /* 0: a point is a frame, 1: the difference of two consecutive frames              */
    int32_t d_outer, d_inner;       /* d = d_outer*d_inner; element (o, e) at + o*so + e                                */
    int32_t classes;
    double* values;                 /* (classes): FD                                                                   */
    double* terms;                  /* (classes, 4): |dmu|^2, tr S_R, tr S_F, T                                        */
    double* mean;                   /* (1) or NULL                                                                     */
    int32_t* sweeps;                /* (classes, 2)                                                                    */
    double* mu_real;                /* (classes, d) or NULL                                                            */
    double* mu_fake;                /* (classes, d) or NULL                                                            */
    double* cov_real;               /* (classes, d, d) or NULL                                                         */
    double* cov_fake;               /* (classes, d, d) or NULL                                                         */
    void* ws;  int64_t ws_bytes;
} KgFrechetArgs;
int64_t kg_frechet_workspace_bytes(const KgFrechetArgs* a);   /* < 0 for invalid shapes                              */
int     kg_frechet(const KgFrechetArgs* a, void* stream);

/* ---- several fake sets against ONE real set whose Frechet side is cached (additive, ABI v9; DESIGN.md 19, csrc/kg_frechet.hip)
 * The Evaluator's case: the real set is fixed for a whole run and every named generator is scored against it.  Strides, diff,
 * d_outer / d_inner, the fp64 arithmetic and the shape rules are those of kg_frechet; e = d + (d & 1) below.
 * kg_frechet_real: the real side of ONE (data, diff) pair: mu_real (classes, d), tr_real (classes) = tr S_R, G (classes, e, e)
 * = V diag(sqrt(max(l, 0))) of S_R row-major (the padding row and column of an odd d are zero), sweeps_real (classes).  Three
 * launches: moments of the real set alone - chunked exactly as kg_frechet chunks the real set of a call with the same n,
 * frames, diff and classes (that chunking depends on P_r and classes alone) -, merge, one workgroup per class running the
 * Jacobi iteration with vectors: the device function kg_frechet's solve runs first.  The four arrays hold the bits kg_frechet
 * forms internally.
 * ws = kg_frechet_real_workspace_bytes(a) = 8 classes (nch_r + 1) (d + d*d) bytes, nch_r the real set's chunks.
 * kg_frechet_sets: nsets (1..KG_FRECHET_MAX_SETS) fake sets fake[g] with shared strides and m against that cache, which is an
 * INPUT read when the launches run; the real data is never touched.  Four launches whatever nsets is: moments of all fake
 * sets (chunked as kg_frechet chunks a fake set of m samples), merge, one workgroup per (set, class) - W = S_F G, H = sym(G^T
 * W), the Jacobi iteration without vectors, T, the terms and the FD: the device function kg_frechet's solve runs second, not a
 * copy of it -, finish (per set the class mean in fp64 and its fp32 rounding mean32, the word kg_eval_record2 reads).
 * For every set g, values[g], terms[g] and
 * sweeps[g] equal, bit for bit, values, terms and sweeps[:, 1] of kg_frechet(real, fake[g]) on the same data, mean[g] its
 * mean, and sweeps_real its sweeps[:, 0]; the grouping into sets shows in no bit.
 * ws = kg_frechet_sets_workspace_bytes(a) = 8 nsets classes (nch_f + 1) (d + d*d) bytes, nch_f the chunks of one fake set.
 * No atomics, no ticket, no scratch; the workspace contents on entry do not matter; every output word is written; nothing is
 * synchronised; capturable on one stream.
 * Rejected (< 0, kg_last_error() names the field) before any GPU call: what kg_frechet rejects for the side in question; nsets
 * outside [1, KG_FRECHET_MAX_SETS]; a null fake[g] with g < nsets; a null cache or output pointer; ws null, misaligned or
 * ws_bytes too small.                                                                                                        */
#define KG_FRECHET_MAX_SETS 4
typedef struct KgFrechetRealArgs {
    const float* real;  int64_t r_sc, r_ss, r_sf, r_so;   /* class, sample, frame, outer-dimension strides (elements)    */
    int32_t n;                      /* real samples per class                                                          */
    int32_t frames, diff;
    int32_t d_outer, d_inner;
    int32_t classes;
    double* mu_real;                /* (classes, d)                                                                    */
    double* tr_real;                /* (classes)                                                                       */
    double* G;                      /* (classes, e, e)                                                                 */
    int32_t* sweeps_real;           /* (classes)                                                                       */
    void* ws;  int64_t ws_bytes;
} KgFrechetRealArgs;
typedef struct KgFrechetSetsArgs {
    const float* fake[KG_FRECHET_MAX_SETS];  int64_t f_sc, f_ss, f_sf, f_so;   /* fake[0 .. nsets): strides and m are shared */
    int32_t nsets;
    int32_t m;                      /* fake samples per class                                                          */
    int32_t frames, diff;
    int32_t d_outer, d_inner;
    int32_t classes;
    const double* mu_real;          /* INPUT: the cache of kg_frechet_real for the same frames, diff, d and classes    */
    const double* tr_real;
    const double* G;
    double* values;                 /* (nsets, classes): FD                                                            */
    double* terms;                  /* (nsets, classes, 4)                                                             */
    int32_t* sweeps;                /* (nsets, classes): the sweeps of H                                               */
    double* mean;                   /* (nsets)                                                                         */
    float* mean32;                  /* (nsets): (float)mean                                                            */
    void* ws;  int64_t ws_bytes;
} KgFrechetSetsArgs;
int64_t kg_frechet_real_workspace_bytes(const KgFrechetRealArgs* a);   /* < 0 for invalid shapes                     */
int     kg_frechet_real(const KgFrechetRealArgs* a, void* stream);
int64_t kg_frechet_sets_workspace_bytes(const KgFrechetSetsArgs* a);   /* < 0 for invalid shapes                     */
int     kg_frechet_sets(const KgFrechetSetsArgs* a, void* stream);

/* ---- inputs of one training iteration (additive, ABI v9; DESIGN.md 11, csrc/kg_input.hip) ---------------------------
 * kg_step_inputs writes, in ONE launch, every input of iteration s = *step and then stores s + 1 (last workgroup).
 * Batch: b = s mod batches_per_epoch, e = s div batches_per_epoch, row r_j = perm[(e & 1)*perm_stride + (b*world +
 * rank)*B + j] (clamped into [0, n_rows)); real[j][c][t][v] = (data[r_j*d_sN + c*d_sC + t*d_sT + v*d_sV] * scale) +
 * shift as two separately rounded fp32 operations; labels[j] = label_src[r_j].  data == NULL: no gather.
 * Random: Philox4x32-10, key = seed (low, high word), counter = (q, stream + 4*rank, s low, s high), the four output
 * words are elements 4q .. 4q+3 of the stream; uniform u = (word >> 8) * 2^-24; normals by Box-Muller on word pairs:
 * sqrt(-2 log(1 - u0)) * (cos, sin)(2 pi u1).  z (B, latent) and alpha (B) are flat; noise plane i of the critic
 * step's synthesis lies at noise + 2*P_i, of the generator step's at noise + 2*P_i + plane_len[i] (P_i = sum of the
 * plane_len before i); a noise stream's element index counts through the synthesis' planes in order.
 * kg_loss_append: ring[2k], ring[2k+1] = *d_loss, *g_loss, k = (*step - 1) mod ring_len; g_loss == NULL repeats the
 * previous slot's g_loss (NaN for iteration 0).                                                                       */
#define KG_STEP_MAX_PLANES 8
#define KG_STREAM_Z 0
#define KG_STREAM_ALPHA 1
#define KG_STREAM_NOISE_D 2
#define KG_STREAM_NOISE_G 3
typedef struct KgStepInputsArgs {
    int64_t* step;                  /* device: iteration counter                                                     */
    int32_t* ticket;                /* device: one zeroed int32, left at zero (from the last ticket's draw on)       */
    uint64_t seed;
    int32_t rank, world;
    int32_t B;
    int32_t C, T, V;                /* sample shape of `real`                                                        */
    const float* data;  int64_t d_sN, d_sC, d_sT, d_sV;    /* element strides                                       */
    int64_t n_rows;
    const int64_t* label_src;       /* (n_rows)                                                                      */
    const int64_t* perm;  int64_t perm_stride;             /* (2, perm_stride)                                       */
    int64_t batches_per_epoch;
    float scale, shift;
    float* real;                    /* (B, C, T, V) contiguous                                                       */
    int64_t* labels;                /* (B)                                                                           */
    float* z;  int32_t latent;      /* (B, latent) or NULL                                                           */
    float* alpha;                   /* (B) or NULL                                                                   */
    float* noise;  int32_t n_planes;  int64_t plane_len[KG_STEP_MAX_PLANES];   /* 2 * sum(plane_len) floats or NULL  */
} KgStepInputsArgs;
int kg_step_inputs(const KgStepInputsArgs* a, void* stream);
int kg_loss_append(float* ring, int64_t ring_len, const int64_t* step, const float* d_loss, const float* g_loss,
                   void* stream);

/* ---- inference-only generation path (additive, ABI v9; DESIGN.md 12, sample.Sampler) --------------------------------
 * kg_bn_eval_coef: the eval-mode coefficients of up to KG_BN_EVAL_MAX_JOBS BatchNorm layers in ONE launch.  Per layer
 *     coef (4, C) = [scale, shift, mean, rstd],  rstd = 1/sqrtf(running_var + eps), scale = gamma*rstd,
 *     shift = beta - running_mean*scale, mean = running_mean          (gamma / beta NULL = 1 / 0)
 * - the layout kg_bn_fwd writes and kg_affine_act / kg_genblock_infer read.  The running statistics are read through
 * their pointers when the launch RUNS: inside a captured graph the coefficients follow every in-place update of them.  */
#define KG_BN_EVAL_MAX_JOBS 8
typedef struct KgBnEvalJob {
    int32_t C;
    const float* gamma;  const float* beta;  const float* running_mean;  const float* running_var;
    float eps;
    float* coef;                    /* out: (4, C)                                                                   */
} KgBnEvalJob;
int kg_bn_eval_coef(const KgBnEvalJob* jobs, int32_t njobs, void* stream);

/* kg_genblock_infer: one generator block (generator.py:168-182) in eval mode as ONE launch, one sample per workgroup:
 *     yc = [W_gcn[:Kp*C]; W_res] x;  z, r = sum_k yc_k (U A_k) / yc_res U + b_res (or x U);  u = W_tcn (*) z + b_tcn;
 *     out = act(u*s_t + b_t + r*s_r + b_r + nw*noise)
 * with (s_t, b_t) = rows 0, 1 of coef_t (4, C) and (s_r, b_r) of coef_r (kg_bn_eval_coef; NULL = 1 / 0).  The BatchNorm
 * coefficients are inputs, so the launch takes no statistics, writes no tape and has no communication between
 * workgroups.  Geometry rules as kg_genblock_fwd; kg_genblock_infer_lds_bytes = -1 where the block does not fit: the
 * LDS / contraction-shape rule of kg_genblock_lds_bytes, and T > 1 with at least 16 input-grid columns Tc*Vc (the
 * weight-bound front blocks stay on the staged launches).                                                              */
typedef struct KgGenBlockInferArgs {
    int32_t N;
    int32_t Cin, C, K, Kp, Tc, Vc, T, V, rep, res_kind, act;  float slope;
    KgPlane x;                              /* (N, Cin, Tc, Vc)                                                          */
    const float* wg;  const float* wr;  const float* br;  const float* wt;  const float* bt;
    const float* b;                         /* (Kp, Vc, V) = U (A * importance), kg_gen_adj_prepare                     */
    const float* u;                         /* (Vc, V) up-sampling matrix or NULL (Vc == V)                             */
    const float* coef_t;  const float* coef_r;      /* (4, C) or NULL                                                   */
    const float* noise;  const float* nw;   /* (N, 1, T, V) contiguous, (C); both or neither                            */
    KgPlane out;                            /* (N, C, T, V)                                                              */
} KgGenBlockInferArgs;
int64_t kg_genblock_infer_lds_bytes(const KgGenBlockInferArgs* a);
int     kg_genblock_infer(const KgGenBlockInferArgs* a, void* stream);

/* kg_sample_inputs: the random inputs of replay s = *step of a Sampler in ONE launch, then *step = s + 1 (last workgroup
 * to finish, as kg_step_inputs).  Philox4x32-10 / Box-Muller exactly as kg_step_inputs with counter
 * (q, KG_STREAM_SAMPLE + stream, s low, s high): streams 0 = z (B, latent; skipped when z == NULL), 1 = noise (noise_len
 * values: the noise planes of ONE synthesis, flat, in plane order; skipped when NULL), 2 = t (t_rows, t_cols: the
 * truncation draws; skipped when NULL).  Word 1 of the training streams is stream + 4*rank: 0x100 .. 0x102 is reached
 * there only by rank 64 of a data-parallel run, so a sampler and a trainer of up to 64 ranks that share a seed never
 * draw the same numbers.                                                                                              */
#define KG_STREAM_SAMPLE 0x100
typedef struct KgSampleInputsArgs {
    int64_t* step;                  /* device: replay counter                                                        */
    int32_t* ticket;                /* device: one zeroed int32, left at zero (from the last ticket's draw on)       */
    uint64_t seed;
    int32_t B, latent;
    float* z;                       /* (B, latent) or NULL                                                           */
    float* noise;  int64_t noise_len;
    float* t;  int32_t t_rows, t_cols;
} KgSampleInputsArgs;
int kg_sample_inputs(const KgSampleInputsArgs* a, void* stream);

/* kg_trunc_lerp: the truncation trick (generate.py:14-21 on Z, generator.py:97-108 on W) in ONE launch:
 *     m[d] = (1/M) sum_i t[i*t_ld + d]  (fixed summation order: two calls give the same bits),
 *     x[n*x_ld + d] = m[d] + truncation * (x[n*x_ld + d] - m[d])   in place, n < N, d < D.
 * A workgroup owns a slab of columns: it reduces them, then applies them; no step across workgroups.                  */
int kg_trunc_lerp(float* x, int64_t x_ld, int32_t N, int32_t D, const float* t, int64_t t_ld, int32_t M, float truncation,
                  void* stream);

/* ---- scoring the generator during training (additive, ABI v9; DESIGN.md 15, evaluate.Evaluator) ----------------------
 * kg_eval_record: the bookkeeping of ONE evaluation, one small workgroup (as kg_loss_append).  With s = *scores[select],
 * n = *count, it = iter ? *iter : -1:
 *     improved = (s < *best_val)            strict: a NaN never wins, an equal score keeps the earlier snapshot
 *     ring_val[(n mod ring_len)*nscores + i] = *scores[i];   ring_iter[(n mod ring_len)*2 + {0, 1}] = it, improved
 *     *flag = improved;   improved: *best_val = s, *best_iter = it;   *count = n + 1
 * The host initialises *best_val = +inf, *best_iter = -1, *count = 0.  The iteration is int64 throughout (fp32 holds
 * integers up to 2^24 only).  Everything is read through its pointer when the launch RUNS: a captured launch follows the
 * training replays in between.  Call sites: evaluate.Evaluator._round, behind the kg_mmd launches of an evaluation.      */
#define KG_EVAL_MAX_SCORES 8
typedef struct KgEvalRecordArgs {
    const float* scores[KG_EVAL_MAX_SCORES];   /* device: one fp32 each                                               */
    int32_t nscores, select;
    const int64_t* iter;            /* device: the loop's iteration counter, or NULL (recorded as -1)                  */
    int64_t* count;                 /* device: evaluations so far, advanced by the launch                              */
    float* ring_val;                /* (ring_len, nscores)                                                             */
    int64_t* ring_iter;             /* (ring_len, 2): [iteration, improved]                                            */
    int64_t ring_len;
    float* best_val;                /* (1)                                                                             */
    int64_t* best_iter;             /* (1)                                                                             */
    int32_t* flag;                  /* (1): the decision kg_copy_if reads                                              */
} KgEvalRecordArgs;
int kg_eval_record(const KgEvalRecordArgs* a, void* stream);

/* kg_eval_record2: kg_eval_record with room for KG_EVAL2_MAX_SCORES scores and a sense:
 *     improved = maximise ? (s > *best_val) : (s < *best_val)      strict either way: a NaN never wins, an equal score
 *                                                                  keeps the earlier snapshot
 * The host initialises *best_val = -inf when maximising, +inf otherwise.  Everything else is the definition above (ring
 * rows, [iteration, improved] in int64, *flag, *count, one thread of one small workgroup); with maximise = 0 and nscores <=
 * KG_EVAL_MAX_SCORES it leaves the same bits as kg_eval_record (one kernel template, one launcher).  Call site:
 * evaluate.Evaluator._round when precision / recall / density / coverage are recorded (live + ema x 6 scores = 12 > 8). */
#define KG_EVAL2_MAX_SCORES 32
typedef struct KgEvalRecord2Args {
    const float* scores[KG_EVAL2_MAX_SCORES];  /* device: one fp32 each                                               */
    int32_t nscores, select;
    const int64_t* iter;
    int64_t* count;
    float* ring_val;                /* (ring_len, nscores)                                                             */
    int64_t* ring_iter;             /* (ring_len, 2): [iteration, improved]                                            */
    int64_t ring_len;
    float* best_val;
    int64_t* best_iter;
    int32_t* flag;
    int32_t maximise;               /* 0: smaller is better, else larger is better                                     */
} KgEvalRecord2Args;
int kg_eval_record2(const KgEvalRecord2Args* a, void* stream);

/* kg_eval_record3: kg_eval_record2 with room for KG_EVAL3_MAX_SCORES scores - the third instantiation of the
 * same kernel template behind the same launcher; the definition, the sense and the host's initial values are those of
 * kg_eval_record2, and with nscores <= KG_EVAL2_MAX_SCORES it leaves the same bits.  Rejected (< 0) before any GPU call:
 * nscores outside [1, KG_EVAL3_MAX_SCORES], select outside [0, nscores), ring_len < 1, a null pointer (iter may be NULL).
 * Call site: evaluate.Evaluator._round when the kinematic columns are recorded (live + ema with everything on = 40 > 32).  */
#define KG_EVAL3_MAX_SCORES 64
typedef struct KgEvalRecord3Args {
    const float* scores[KG_EVAL3_MAX_SCORES];  /* device: one fp32 each                                               */
    int32_t nscores, select;
    const int64_t* iter;
    int64_t* count;
    float* ring_val;                /* (ring_len, nscores)                                                             */
    int64_t* ring_iter;             /* (ring_len, 2): [iteration, improved]                                            */
    int64_t ring_len;
    float* best_val;
    int64_t* best_iter;
    int32_t* flag;
    int32_t maximise;               /* 0: smaller is better, else larger is better                                     */
} KgEvalRecord3Args;
int kg_eval_record3(const KgEvalRecord3Args* a, void* stream);

/* kg_copy_if: when *flag != 0 every job's run of `nwords` 4-byte words is copied src -> dst bit for bit; when *flag == 0
 * the launch writes nothing at all.  A job whose src and dst are both 16-byte aligned moves 128 bits per access with a
 * scalar tail, any other job word by word.  No ticket, no atomic, no LDS, no scratch: the grid only reads the decision a
 * PREVIOUS launch wrote.  Up to KG_COPY_IF_MAX_JOBS jobs per launch; src / dst 4-byte aligned; a job whose src and dst
 * overlap is rejected.  Call site: evaluate.Evaluator._round (the snapshot of the best-scoring weights: the flat
 * parameter buffer plus every module buffer, an int64 batch counter as two words per element).                        */
#define KG_COPY_IF_MAX_JOBS 32
typedef struct KgCopyJob { const void* src;  void* dst;  int64_t nwords; } KgCopyJob;
int kg_copy_if(const int32_t* flag, const KgCopyJob* jobs, int32_t njobs, void* stream);

/* ---- action classifier head (additive, ABI v9; DESIGN.md 20, csrc/kg_cls.hip) ------------------------------------------
 * The head of classifier.Classifier on the last st_gcn block's output h (N, C, T, V), P = T V, read in place through
 * (h_sN, h_sC) - the trunk's channel-major planes and an NCHW tensor alike:
 *   pooled[n, c] = (sum_{t,v} h[n, c, t, v]) / P                          (t, v) in index order
 *   feat[n, f]   = lrelu_slope(b1[f] + sum_c w1[f, c] pooled[n, c])       w1 (F, C), F <= KG_FRECHET_MAX_DIM
 *   logits[n, l] = b2[l] + sum_f w2[l, f] feat[n, f]                      w2 (L, F)
 *   pred[n]      = lowest class index holding the largest logit: start at class 0, replace on a strict '>' (NaN never wins)
 *   loss_per_sample[n] = (m + log sum_l exp(logits[n, l] - m)) - logits[n, y_n],  m = max_l logits[n, l]
 *                        NaN when y_n is outside [0, L): such a sample is never counted correct and reads nothing
 *   loss = (1/N) sum_n loss_per_sample[n]        correct = #{n : 0 <= y_n < L and pred[n] == y_n}
 * kg_cls_head_fwd: a workgroup owns KG_CLS_TILE samples (w1 is read once per tile) and writes pooled, feat, logits, pred
 *   and - with labels - loss_per_sample; then ONE workgroup finishes loss (fp64, sample-index order, rounded once) and
 *   correct.  No exchange between the workgroups of a launch: no tickets, no atomics - two calls give the same bits.
 *   labels == NULL: features, logits and predictions only (loss_per_sample, loss, correct are not touched).
 * kg_cls_head_bwd: from the scalar top gradient *gtop (device memory), the forward's feat / logits and the labels:
 *   dlogits[n, l] = ((softmax(logits[n])[l] - [l == y_n]) * gtop) / N     (NaN for a label outside [0, L))
 *   dfeat[n, f]   = (sum_l w2[l, f] dlogits[n, l]) * lrelu'(feat[n, f])   lrelu'(o) = o > 0 ? 1 : slope
 *   dpooled[n, c] = sum_f w1[f, c] dfeat[n, f]
 *   g[n, c, t, v] = dpooled[n, c] / P * (masked ? lrelu'(h[n, c, t, v]) : 1)      (the contract of kg_head_bwd)
 *   dlogits (N, L) and dfeat (N, F) go to the workspace, in this order.
 * kg_cls_head_wgrad: from the workspace kg_cls_head_bwd filled, pooled and feat:
 *   dw2[l, f] (+)= sum_n dlogits[n, l] feat[n, f]      db2[l] (+)= sum_n dlogits[n, l]
 *   dw1[f, c] (+)= sum_n dfeat[n, f] pooled[n, c]      db1[f] (+)= sum_n dfeat[n, f]
 *   every output element is summed over n in index order by one thread; `accumulate` as in kg_head_wgrad.
 * ws: kg_cls_head_workspace_bytes(a) = 4 N (L + F) bytes.  A null operand, N, T, V < 1, C outside [1, KG_CLS_MAX_C],
 * F outside [1, KG_FRECHET_MAX_DIM], L outside [1, KG_CLS_MAX_CLASSES] or a small workspace are rejected on the host
 * (< 0, kg_last_error() names the entry point) before anything is launched.                                          */
#define KG_CLS_TILE 4
#define KG_CLS_MAX_C 1024
#define KG_CLS_MAX_CLASSES 1024
typedef struct KgClsHeadArgs {
    int32_t N, C, T, V, F, L;
    const float* h;  int64_t h_sN, h_sC;        /* (N, C, T, V) plane tensor; bwd: read only when `masked`            */
    const float* w1;  const float* b1;          /* fc1: (F, C), (F)                                                    */
    const float* w2;  const float* b2;          /* fcn: (L, F), (L)                                                    */
    const int64_t* labels;                      /* (N) or NULL (fwd only)                                              */
    float slope;  int32_t masked;
    float* pooled;                              /* (N, C)   fwd: out; wgrad: in                                        */
    float* feat;                                /* (N, F)   fwd: out; bwd, wgrad: in                                   */
    float* logits;                              /* (N, L)   fwd: out; bwd: in                                          */
    float* loss_per_sample;                     /* (N)      fwd with labels                                            */
    int32_t* pred;                              /* (N)      fwd                                                        */
    float* loss;  int32_t* correct;             /* (1), (1) fwd with labels                                            */
    const float* gtop;                          /* bwd: (1) d(objective) / d loss, on the device                       */
    float* g;  int64_t g_sN, g_sC;              /* bwd: (N, C, T, V) plane tensor                                      */
    float* dw1;  float* db1;  float* dw2;  float* db2;  int32_t accumulate;      /* wgrad                             */
    void* ws;  int64_t ws_bytes;
} KgClsHeadArgs;
int64_t kg_cls_head_workspace_bytes(const KgClsHeadArgs* a);   /* < 0 for invalid shapes                              */
int     kg_cls_head_fwd(const KgClsHeadArgs* a, void* stream);
int     kg_cls_head_bwd(const KgClsHeadArgs* a, void* stream);
int     kg_cls_head_wgrad(const KgClsHeadArgs* a, void* stream);

/* ---- classifier scores of up to four sets (additive, ABI v9; DESIGN.md 21, csrc/kg_cls.hip) ----------------------------
 * From the features feat[s] (N, F; fp32, shared row stride feat_ld >= F) and predictions pred[s] (N) of nsets sets that
 * share the labels (N) and two tables of row-index pairs - div_pairs (Sd, 2) and mm_pairs (K*Sl, 2), class-major:
 *   dist[s, p]             = sqrt(sum_f ((double)feat[s][i_p, f] - (double)feat[s][j_p, f])^2)
 *                            p over the Sd diversity pairs, then the K*Sl multimodality pairs; an index outside [0, N)
 *                            gives NaN and nothing is read for the pair
 *   diversity[s]           = (sum_{p < Sd} dist[s, p]) / Sd                     fp64, index order, one division
 *   multimodality[s]       = (sum over the K*Sl pairs, index order) / (K*Sl)
 *   correct_per_class[s,c] = #{n : labels[n] == c and pred[s][n] == c}          a label outside [0, K) counts nowhere
 *   count_per_class[c]     = #{n : labels[n] == c}
 *   correct[s]             = sum_c correct_per_class[s, c];   accuracy[s] = (double)correct[s] / N
 *   scores64 (nsets, 3)    = [accuracy, diversity, multimodality];   scores = its fp32 rounding, once
 * Two launches: a wave per (set, pair) writes dist (lane-strided fp64 squares, a shuffle tree, one sqrt); then ONE workgroup
 * per set tallies the integers in LDS (integer adds only) and ONE thread adds the two means in index order.  No tickets,
 * no polled words, no atomics on global memory; every output element has one owner (count_per_class: the workgroup of set
 * 0) and is written on every call - two calls give the same bits.  No scratch beyond dist.  A null operand, nsets outside
 * [1, KG_CLS_MAX_SETS], N < 1, F outside [1, KG_FRECHET_MAX_DIM], K outside [1, KG_CLS_MAX_CLASSES], Sd < 1, Sl < 1 or
 * feat_ld < F are rejected on the host (< 0, kg_last_error() names the entry point) before anything is launched.        */
#define KG_CLS_MAX_SETS 4
typedef struct KgClsScoresArgs {
    int32_t nsets, N, F, K, Sd, Sl;
    int64_t feat_ld;
    const float* feat[KG_CLS_MAX_SETS];         /* (N, F) rows feat_ld floats apart                                    */
    const int32_t* pred[KG_CLS_MAX_SETS];       /* (N)                                                                 */
    const int64_t* labels;                      /* (N)                                                                 */
    const int32_t* div_pairs;                   /* (Sd, 2)                                                             */
    const int32_t* mm_pairs;                    /* (K*Sl, 2), class-major                                              */
    double* dist;                               /* out: (nsets, Sd + K*Sl)                                             */
    double* scores64;  float* scores;           /* out: (nsets, 3), (nsets, 3)                                         */
    int32_t* correct;                           /* out: (nsets)                                                        */
    int32_t* correct_per_class;                 /* out: (nsets, K)                                                     */
    int32_t* count_per_class;                   /* out: (K)                                                            */
} KgClsScoresArgs;
int     kg_cls_scores(const KgClsScoresArgs* a, void* stream);

/* ---- kinematic plausibility: bones, smoothness, W1 (additive, ABI v9; DESIGN.md 25, csrc/kg_kin.hip) ---------------------
 * A sample is x[c, f, v], c < C (2 or 3), f < T, v < V, fp32, read in place:
 *   x[c, f, v] of sample i of class k = x + k*sc + i*ss + f*sf + c*so + v            (the joint axis is contiguous)
 * With bones (B, 2) joint pairs (u_b, v_b) and mirror (M, 2) pairs of bone indices, everything in fp64 from the fp32 inputs,
 * |.| the Euclidean norm over c:
 *   L[b, f] = |x[:, f, u_b] - x[:, f, v_b]|     mu_b = mean_f L[b, f]     sd_b = sqrt(mean_f (L[b, f] - mu_b)^2)  (two passes)
 *   s = mean_{b, f} L[b, f]                     the sample's own length unit: every descriptor is dimensionless
 *   D1 = x[f+1] - x[f],   D2 = (x[f+2] - 2 x[f+1]) + x[f],   D3 = ((x[f+3] - 3 x[f+2]) + 3 x[f+1]) - x[f]      per joint
 * The KG_KIN_DESC = 6 descriptors of a sample:
 *   0 bone_cv    mean over bones of sd_b / mu_b (a bone with mu_b == 0 contributes 0)
 *   1 asymmetry  mean over mirror pairs (a, b) of abs(mu_a - mu_b) / (0.5 (mu_a + mu_b)) (a zero denominator contributes 0;
 *                M == 0: the descriptor is 0)
 *   2 speed      mean_{v, f < T-1} |D1| / s
 *   3 accel      mean_{v, f < T-2} |D2| / s
 *   4 jerk       mean_{v, f < T-3} |D3| / s
 *   5 still      the share of (v, f < T-1) with |D1| < still_eps * s
 * s == 0 (every bone collapsed): six zeros, and the sample counts in degenerate[class].  Non-finite inputs propagate.  The
 * six fp64 values are rounded ONCE to fp32: desc (classes, n, 6).
 * kg_kin_desc: ONE launch, a workgroup per sample.  The sample is staged into LDS through the strides (4 C T V bytes: it is
 * read from memory once), then bone sums, the second pass about mu_b, and the joint differences, all in fp64; every sum has
 * a fixed shape (a thread's items in index order, a shuffle tree, the waves in order), so two calls give the same bits.  No
 * atomics on data.  degenerate: every workgroup hands its flag over (csrc/kg_handoff.h), the last one to arrive counts the
 * flags of every class (integers).  ws = kg_kin_desc_workspace_bytes(a) = 4 classes n bytes, contents on entry do not matter;
 * counters: >= 1 zeroed int32, left zeroed.  bones / mirror are HOST pointers: validated and copied into the launch's
 * arguments.  kg_kin_desc_lds_bytes(a) = the LDS of a workgroup (4 C T V + a fixed part), < 0 for a shape it rejects.
 * Rejected (< 0, kg_last_error() names the field) before any GPU call: null x / desc / degenerate / bones / ws / counters (a
 * null mirror with M > 0); classes or n < 1; classes * n >= 2^24; C not 2 or 3; V outside [1, KG_KIN_MAX_JOINTS]; B outside
 * [1, KG_KIN_MAX_BONES]; M outside [0, KG_KIN_MAX_MIRROR]; T < KG_KIN_MIN_FRAMES; C*T*V > KG_KIN_MAX_ELEMS; a negative stride;
 * a bone endpoint outside [0, V); a mirror index outside [0, B); a non-finite or negative still_eps; ws_bytes too small;
 * counters_len < 1.
 *
 * kg_kin_scores: nsets (1..KG_KIN_MAX_SETS) fake descriptor matrices fake[g] (classes, m, 6) against ONE real matrix
 * (classes, n, 6), contiguous fp32; every score is a function of the stored fp32 values alone:
 *   tree(t) = pad t with +0.0 to the next power of two P, then t[i] += t[i + h] for h = P/2, P/4, .., 1;  t[0]
 *   mean_real (classes, 6), mean_fake (nsets, classes, 6) fp64 = tree(the column's values in sample order) / count
 *   w1 (nsets, classes, 6) fp64, the Wasserstein-1 distance of the two empirical distributions of a descriptor: sort the
 *     n + m values ascending to z; cr_i / cf_i = the real / fake values among the first i + 1;
 *     term_i = (double)abs(cr_i * m - cf_i * n) * ((double)z_{i+1} - (double)z_i), i < n + m - 1 (64-bit integers);
 *     w1 = tree(term) / (double)(n * m).  Ties have a gap of 0, so their order shows in no bit.  Any non-finite value among
 *     the n + m: NaN.
 *   w1_mean (nsets, 6) fp64 = (sum over classes in class order) / classes;   scores (nsets, 6) = its one fp32 rounding
 *   nonfinite (nsets + 1, classes) int32 = the samples with a non-finite descriptor, the real side in row 0
 * TWO launches whatever nsets is: a workgroup per (set, class, descriptor) - the means by trees in LDS (the real side's by the
 * workgroups of set 0 only), then the n + m values as 64-bit keys in LDS (the order-preserving integer image of the fp32 value,
 * a side bit, padding keys above everything), a bitonic sort, a prefix count, the terms written over the keys, the tree -; then
 * one small launch for w1_mean, scores and nonfinite.  No atomics on global memory, no workspace, no host synchronisation;
 * every output word has one owner and is written on every call; capturable on one stream.
 * kg_kin_scores_lds_bytes(a) = the LDS of a workgroup of launch 1 (8 bytes per key of the padded power of two, at most
 * 8 KG_KIN_MAX_POINTS = 128 KiB), < 0 for a shape it rejects.
 * Rejected (< 0, kg_last_error() names the field) before any GPU call: a null real / output pointer; classes, n or m < 1;
 * n + m > KG_KIN_MAX_POINTS; nsets outside [1, KG_KIN_MAX_SETS]; a null fake[g] with g < nsets; classes above 2^20.            */
#define KG_KIN_DESC 6
#define KG_KIN_MAX_JOINTS 32
#define KG_KIN_MAX_BONES 32
#define KG_KIN_MAX_MIRROR 16
#define KG_KIN_MIN_FRAMES 4
#define KG_KIN_MAX_ELEMS 32768
#define KG_KIN_MAX_SETS 4
#define KG_KIN_MAX_POINTS 16384
typedef struct KgKinDescArgs {
    const float* x;  int64_t sc, ss, sf, so;    /* class, sample, frame, channel strides (elements)                     */
    int32_t n;                                  /* samples per class                                                   */
    int32_t T, C, V;
    int32_t classes;
    int32_t B, M;
    const int32_t* bones;                       /* HOST: (B, 2) joints                                                 */
    const int32_t* mirror;                      /* HOST: (M, 2) bone indices; may be NULL when M == 0                  */
    double still_eps;
    float* desc;                                /* out: (classes, n, 6)                                                */
    int32_t* degenerate;                        /* out: (classes)                                                      */
    float* ws;  int64_t ws_bytes;  int32_t* counters;  int32_t counters_len;
} KgKinDescArgs;
typedef struct KgKinScoresArgs {
    const float* real;                          /* (classes, n, 6)                                                     */
    const float* fake[KG_KIN_MAX_SETS];         /* fake[0 .. nsets): (classes, m, 6)                                   */
    int32_t nsets, n, m, classes;
    double* mean_real;                          /* out: (classes, 6)                                                   */
    double* mean_fake;                          /* out: (nsets, classes, 6)                                            */
    double* w1;                                 /* out: (nsets, classes, 6)                                            */
    double* w1_mean;                            /* out: (nsets, 6)                                                     */
    float* scores;                              /* out: (nsets, 6) = (float)w1_mean                                    */
    int32_t* nonfinite;                         /* out: (nsets + 1, classes)                                           */
} KgKinScoresArgs;
int64_t kg_kin_desc_workspace_bytes(const KgKinDescArgs* a);   /* < 0 for invalid arguments                            */
int64_t kg_kin_desc_lds_bytes(const KgKinDescArgs* a);         /* < 0 for invalid arguments                            */
int     kg_kin_desc(const KgKinDescArgs* a, void* stream);
int64_t kg_kin_scores_lds_bytes(const KgKinScoresArgs* a);     /* < 0 for invalid arguments                            */
int     kg_kin_scores(const KgKinScoresArgs* a, void* stream);

/* kg_kin_desc_sets: the descriptors of nsets (1..KG_KIN_MAX_SETS) sets x[g] in ONE launch.  The sets share
 * the strides, n, T, C, V, classes, the two tables and still_eps; every set has outputs of its own.  The grid is
 * nsets * classes * n workgroups, (set, class, sample) with the set as the slowest coordinate; a workgroup picks its set's two
 * pointers and from there on runs the code of kg_kin_desc - one kernel body (a template: with one set the set coordinate is
 * compiled away), one validation, one launcher; kg_kin_desc is the one-set case.  Per set g, bit for bit:
 *     desc[g] (classes, n, 6) and degenerate[g*classes .. (g+1)*classes) = what kg_kin_desc(x[g]) writes
 * (every sum keeps its shape, which depends on (T, V, B) alone).  ONE ticket over the whole grid (csrc/kg_handoff.h): the
 * last workgroup to arrive counts the flags of every (set, class) with integer adds; no other atomics.
 * ws = kg_kin_desc_sets_workspace_bytes(a) = 4 nsets classes n bytes, contents on entry do not matter; counters: >= 1 zeroed
 * int32, left zeroed.  kg_kin_desc_sets_lds_bytes(a) = kg_kin_desc_lds_bytes of the shared shape.  No host synchronisation;
 * capturable; launches that share ws or counters must not overlap.
 * Rejected (< 0, kg_last_error() names the field) before any GPU call: every rule of kg_kin_desc; nsets outside
 * [1, KG_KIN_MAX_SETS]; a null x[g] or desc[g] with g < nsets; nsets * classes * n >= 2^24.
 * Call site: evaluate.Evaluator._kinematics_scores (the rounds of up to four generators through their shared strides).      */
typedef struct KgKinDescSetsArgs {
    const float* x[KG_KIN_MAX_SETS];            /* x[0 .. nsets)                                                        */
    int64_t sc, ss, sf, so;                     /* class, sample, frame, channel strides (elements), shared            */
    int32_t nsets;
    int32_t n;                                  /* samples per class                                                   */
    int32_t T, C, V;
    int32_t classes;
    int32_t B, M;
    const int32_t* bones;                       /* HOST: (B, 2) joints                                                 */
    const int32_t* mirror;                      /* HOST: (M, 2) bone indices; may be NULL when M == 0                  */
    double still_eps;
    float* desc[KG_KIN_MAX_SETS];               /* out: desc[0 .. nsets), each (classes, n, 6)                         */
    int32_t* degenerate;                        /* out: (nsets, classes)                                               */
    float* ws;  int64_t ws_bytes;  int32_t* counters;  int32_t counters_len;
} KgKinDescSetsArgs;
int64_t kg_kin_desc_sets_workspace_bytes(const KgKinDescSetsArgs* a);   /* < 0 for invalid arguments                   */
int64_t kg_kin_desc_sets_lds_bytes(const KgKinDescSetsArgs* a);         /* < 0 for invalid arguments                   */
int     kg_kin_desc_sets(const KgKinDescSetsArgs* a, void* stream);

/* ---- projection into W: per-sample objective and per-sample optimiser step (additive, ABI v9; DESIGN.md 29, csrc/kg_proj.hip)
 * The tail of one iteration of project.Projector behind the generator's forward and backward pass: two launches.
 *
 * kg_proj_loss: ONE launch, a workgroup per sample.  x (n, C, T, V) generated, y the target, both through sample / channel /
 * frame strides (elements) of their own with the joints contiguous; y is read as  y' = fp32(fp32(y * scale) + shift)  (two
 * separately rounded fp32 operations: what two stock launches compute), so a row of a resident dataset or a crop in T is read
 * in place.  m: weights >= 0, (T, V) per sample at sample stride sm (sm = 0: one mask for all samples); NULL: all ones.
 * bones: HOST (B, 2) joints, 0 <= B <= KG_KIN_MAX_BONES, copied into the launch.  With
 *     d = fp32(x - y')                                               one fp32 subtraction
 *     Wp = C sum_{t,v} m[t,v]                                        L_pos  = sum_{c,t,v} m d^2 / Wp
 *     mv[t,v] = m[t,v] m[t+1,v],  Wv = C sum_{t<T-1,v} mv            L_vel  = sum mv (d[c,t+1,v] - d[c,t,v])^2 / Wv
 *     mb[t,b] = m[t,a_b] m[t,c_b], Wb = sum mb,
 *     s_x = sum_c (x[c,t,a_b] - x[c,t,c_b])^2, s_y likewise on y'    L_bone = sum mb (s_x - s_y)^2 / Wb
 *     L = (lambda_pos L_pos + lambda_vel L_vel) + lambda_bone L_bone
 * everything after d in fp64 (the bone differences are exact there), every output word rounded once:
 *     loss (n, 4) = [L, L_pos, L_vel, L_bone],   gx (n, C, T, V) contiguous = dL_i / dx_i  (d counts as x - y').
 * A term whose lambda is 0 or whose W is 0 (T < 2 for the velocity term, B == 0 for the bone term) is off: its loss word is 0
 * and it adds nothing to L or gx.  An entry whose weight is not > 0 is selected away, never multiplied: a NaN in a masked-out
 * target entry changes no output bit.  The frames are staged in LDS in chunks of KG_PROJ_CHUNK_FRAMES with one halo frame on
 * each side, so T has no cap.  Each thread adds its terms in frame order, then a shuffle tree and the four waves in order: the
 * shape of every sum depends on (C, T, V, B) alone.  No atomics, no host synchronisation, capturable; two calls, same bits.
 * Rejected (< 0, kg_last_error() names the field) before any GPU call: null x / y / loss / gx (null bones with B > 0); n, C, T
 * or V < 1; C > KG_PROJ_MAX_CHANNELS; V > KG_PROJ_MAX_JOINTS; B outside [0, KG_KIN_MAX_BONES]; a bone joint outside [0, V); a
 * negative stride; a lambda that is negative or not finite; scale or shift not finite.
 *
 * kg_proj_step: ONE launch, a workgroup per sample i.  w, am, av (n, D) fp32 the latents and their Adam moments, gw (n, D)
 * the gradient of L_i, wmean (K, D), labels (n) int64, loss (n, 4) of kg_proj_loss, *step the 1-based number of THIS step in
 * device memory (as kg_adam_step: the launch does not advance it).  With s = *step, fp64 inside, every output rounded once:
 *     prior_i = mean_d (w - wmean[label_i])^2,   obj_i = fp32(L_i + lambda_w prior_i)      (lambda_w == 0: obj_i = L_i)
 *     hist[(s - 1) n + i] = obj_i                                   (hist (S, n) may be NULL; 1 <= s <= S, else no write)
 *     frozen_i = obj_i not finite, or a gw[i, :] not finite, or label_i outside [0, K):
 *                w, am, av, best_* of the sample keep their bits and nonfinite[i] += 1
 *     else: if obj_i < best_obj[i]: best_obj[i] = obj_i, best_loss[i, :] = loss[i, :], best_w[i, :] = w[i, :] (before the update)
 *           g = gw + 2 lambda_w (w - wmean[label_i]) / D
 *           lr_s = lr min(1, s / ramp_up) (s > S - ramp_down ? (1 + cos(pi (s - (S - ramp_down)) / ramp_down)) / 2 : 1)
 *                  (ramp_up / ramp_down == 0: that factor is 1)
 *           am = b1 am + (1 - b1) g,  av = b2 av + (1 - b2) g^2,  w -= lr_s (am / (1 - b1^s)) / (sqrt(av / (1 - b2^s)) + eps)
 * No atomics, no host synchronisation, capturable.
 * Rejected (< 0, kg_last_error() names the field) before any GPU call: null w / am / av / gw / wmean / labels / loss / step /
 * best_obj / best_loss / best_w / nonfinite; n, D or K < 1; lambda_w negative or not finite; lr negative or not finite; b1 or b2
 * outside [0, 1); eps negative or not finite; S < 1; ramp_up or ramp_down outside [0, S].
 * Call site: project.Projector._iteration.                                                                                   */
#define KG_PROJ_MAX_CHANNELS 3
#define KG_PROJ_MAX_JOINTS 32
#define KG_PROJ_CHUNK_FRAMES 32
typedef struct KgProjLossArgs {
    const float* x;  int64_t x_sn, x_sc, x_st;  /* generated: sample, channel, frame strides (elements)                        */
    const float* y;  int64_t y_sn, y_sc, y_st;  /* target, read as y * scale + shift                                           */
    float scale, shift;
    const float* m;  int64_t sm;                /* weights (T, V) per sample, sample stride sm (0: shared); NULL: all ones      */
    int32_t n, C, T, V, B;
    const int32_t* bones;                       /* HOST: (B, 2) joints; may be NULL when B == 0                                */
    double lambda_pos, lambda_vel, lambda_bone;
    float* loss;                                /* out: (n, 4)                                                                 */
    float* gx;                                  /* out: (n, C, T, V) contiguous                                                */
} KgProjLossArgs;
typedef struct KgProjStepArgs {
    float* w;  float* am;  float* av;           /* in / out: (n, D)                                                            */
    const float* gw;                            /* (n, D)                                                                      */
    const float* wmean;                         /* (K, D)                                                                      */
    const int64_t* labels;                      /* (n)                                                                         */
    const float* loss;                          /* (n, 4)                                                                      */
    const int32_t* step;                        /* device: the 1-based number of this step                                     */
    float* best_obj;  float* best_loss;  float* best_w;     /* in / out: (n), (n, 4), (n, D)                                   */
    float* hist;                                /* out: (S, n); may be NULL                                                    */
    int32_t* nonfinite;                         /* in / out: (n)                                                               */
    int32_t n, D, K, S, ramp_up, ramp_down;
    double lambda_w, lr, b1, b2, eps;
} KgProjStepArgs;
int     kg_proj_loss(const KgProjLossArgs* a, void* stream);
int     kg_proj_step(const KgProjStepArgs* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KGAN_HIP_H */
