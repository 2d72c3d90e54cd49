// Scoring the generator during training (include/kgan_hip.h; evaluate.Evaluator):
//   kg_eval_record : ONE thread compares the deciding score of an evaluation with the best so far, appends the evaluation
//                    to the device record and leaves the decision in `flag`
//   kg_eval_record2: the same kernel template and the same launcher (eval_record_launch) with room for KG_EVAL2_MAX_SCORES
//                    scores and a sense (larger or smaller is better)
//   kg_eval_record3: the third instantiation, room for KG_EVAL3_MAX_SCORES scores (the kinematic columns)
//   kg_copy_if     : a grid that only READS that decision and, when it is set, copies a table of word runs - the snapshot
//                    of the best-scoring weights, taken by the device with no host synchronisation
// Two launches on purpose: one writer of the decision, then readers of it, with a launch boundary in between - there is no
// ordering between workgroups to get wrong (no ticket, no atomic).  Both read everything through pointers when they run,
// so a captured evaluation follows the training replays in between.
#include "kg_common.h"

namespace {

template <int MAXS>
struct EvalRecDev {
    const float* scores[MAXS];
    int nscores, select, maximise;
    const long long* iter;
    long long* count;
    float* ring_val;
    long long* ring_iter;
    long ring_len;
    float* best_val;
    long long* best_iter;
    int* flag;
};

template <int MAXS>
__global__ __launch_bounds__(64) void kg_eval_record_kernel(const EvalRecDev<MAXS> a) {
    if (threadIdx.x != 0) return;
    const long long n = *a.count;
    const long long it = a.iter != nullptr ? *a.iter : -1ll;
    if (n < 0) return;                              // (a counter the host never initialised: no slot to write)
    const long k = (long)(n % a.ring_len);
    float s = 0.f;
    for (int i = 0; i < a.nscores; ++i) {
        const float v = *a.scores[i];
        a.ring_val[k * a.nscores + i] = v;
        if (i == a.select) s = v;
    }
    const float b = *a.best_val;                    // strict: a NaN never wins, an equal score keeps the earlier snapshot
    const bool improved = a.maximise ? s > b : s < b;
    a.ring_iter[2 * k] = it;
    a.ring_iter[2 * k + 1] = improved ? 1ll : 0ll;
    *a.flag = improved ? 1 : 0;
    if (improved) {
        *a.best_val = s;
        *a.best_iter = it;
    }
    *a.count = n + 1;
}

struct CopyJobs {
    const int* flag;
    KgCopyJob j[KG_COPY_IF_MAX_JOBS];
};

constexpr int CP_NT = 256;
constexpr int CP_MAX_BLOCKS = 512;      // per job: 2 workgroups per CU; longer runs take a grid-stride loop

// grid (blocks of the longest job, njobs); a workgroup beyond its job's length has nothing to do
__global__ __launch_bounds__(CP_NT) void kg_copy_if_kernel(const CopyJobs a) {
    if (*a.flag == 0) return;
    const KgCopyJob& j = a.j[blockIdx.y];
    const unsigned* src = (const unsigned*)j.src;
    unsigned* dst = (unsigned*)j.dst;
    const long n = (long)j.nwords;
    const long stride = (long)gridDim.x * CP_NT;
    const long first = (long)blockIdx.x * CP_NT + threadIdx.x;
    if ((((unsigned long long)j.src | (unsigned long long)j.dst) & 15ull) == 0) {
        const long n4 = n >> 2;
        const uint4* s4 = (const uint4*)src;
        uint4* d4 = (uint4*)dst;
        for (long i = first; i < n4; i += stride) d4[i] = s4[i];
        const long t = (n4 << 2) + first;           // the scalar tail: at most 3 words, threads 0..2 of workgroup 0
        if (first < 4 && t < n) dst[t] = src[t];
    } else {
        for (long i = first; i < n; i += stride) dst[i] = src[i];
    }
}

}  // namespace

namespace {

// Both record entry points: the checks, the kernel's arguments and the launch of kg_eval_record_kernel<MAXS>; `who` is the
// entry point's name in the messages
template <int MAXS>
int eval_record_launch(const char* who, const float* const* scores, int nscores, int select, int maximise, const int64_t* iter,
                       int64_t* count, float* ring_val, int64_t* ring_iter, int64_t ring_len, float* best_val, int64_t* best_iter,
                       int32_t* flag, void* stream) {
    KG_REQUIRE(nscores >= 1 && nscores <= MAXS, "%s: nscores=%d outside [1, %d]", who, nscores, MAXS);
    KG_REQUIRE(select >= 0 && select < nscores, "%s: select=%d outside [0, nscores=%d)", who, select, nscores);
    KG_REQUIRE(ring_len >= 1, "%s: ring_len=%lld < 1", who, (long long)ring_len);
    EvalRecDev<MAXS> d = {};
    for (int i = 0; i < nscores; ++i) {
        KG_REQUIRE(scores[i] != nullptr, "%s: null score %d", who, i);
        d.scores[i] = scores[i];
    }
    KG_REQUIRE(count != nullptr && ring_val != nullptr && ring_iter != nullptr, "%s: null count / ring_val / ring_iter", who);
    KG_REQUIRE(best_val != nullptr && best_iter != nullptr && flag != nullptr, "%s: null best_val / best_iter / flag", who);
    d.nscores = nscores;
    d.select = select;
    d.maximise = maximise;
    d.iter = (const long long*)iter;
    d.count = (long long*)count;
    d.ring_val = ring_val;
    d.ring_iter = (long long*)ring_iter;
    d.ring_len = (long)ring_len;
    d.best_val = best_val;
    d.best_iter = (long long*)best_iter;
    d.flag = flag;
    hipLaunchKernelGGL(kg_eval_record_kernel<MAXS>, dim3(1), dim3(64), 0, (hipStream_t)stream, d);
    return kg_launch_status(who);
}

}  // namespace

extern "C" int kg_eval_record(const KgEvalRecordArgs* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_eval_record: null arguments");
    return eval_record_launch<KG_EVAL_MAX_SCORES>("kg_eval_record", a->scores, a->nscores, a->select, /*maximise=*/0, a->iter,
                                                  a->count, a->ring_val, a->ring_iter, a->ring_len, a->best_val, a->best_iter,
                                                  a->flag, stream);
}

extern "C" int kg_eval_record2(const KgEvalRecord2Args* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_eval_record2: null arguments");
    return eval_record_launch<KG_EVAL2_MAX_SCORES>("kg_eval_record2", a->scores, a->nscores, a->select, a->maximise != 0 ? 1 : 0,
                                                   a->iter, a->count, a->ring_val, a->ring_iter, a->ring_len, a->best_val,
                                                   a->best_iter, a->flag, stream);
}

extern "C" int kg_eval_record3(const KgEvalRecord3Args* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_eval_record3: null arguments");
    return eval_record_launch<KG_EVAL3_MAX_SCORES>("kg_eval_record3", a->scores, a->nscores, a->select, a->maximise != 0 ? 1 : 0,
                                                   a->iter, a->count, a->ring_val, a->ring_iter, a->ring_len, a->best_val,
                                                   a->best_iter, a->flag, stream);
}

extern "C" int kg_copy_if(const int32_t* flag, const KgCopyJob* jobs, int32_t njobs, void* stream) {
    KG_REQUIRE(flag != nullptr && jobs != nullptr, "kg_copy_if: null flag / jobs");
    KG_REQUIRE(njobs >= 1 && njobs <= KG_COPY_IF_MAX_JOBS, "kg_copy_if: njobs=%d outside [1, %d]", njobs, KG_COPY_IF_MAX_JOBS);
    CopyJobs c = {};
    c.flag = flag;
    long most = 0;
    for (int i = 0; i < njobs; ++i) {
        const KgCopyJob& j = jobs[i];
        KG_REQUIRE(j.src != nullptr && j.dst != nullptr, "kg_copy_if: job %d: null src / dst", i);
        KG_REQUIRE(j.nwords >= 1 && j.nwords < (1ll << 40), "kg_copy_if: job %d: nwords=%lld", i, (long long)j.nwords);
        const uintptr_t s = (uintptr_t)j.src, d = (uintptr_t)j.dst, bytes = (uintptr_t)j.nwords * 4;
        KG_REQUIRE(((s | d) & 3) == 0, "kg_copy_if: job %d: src / dst not 4-byte aligned", i);
        KG_REQUIRE(s + bytes <= d || d + bytes <= s, "kg_copy_if: job %d: src and dst overlap", i);
        c.j[i] = j;
        // blocks of the job: 128-bit form = 4 words per thread (an unaligned job only needs more trips of its loop)
        const long units = (j.nwords + 3) / 4;
        most = units > most ? units : most;
    }
    long gx = (most + CP_NT - 1) / CP_NT;
    gx = gx < 1 ? 1 : (gx > CP_MAX_BLOCKS ? CP_MAX_BLOCKS : gx);
    hipLaunchKernelGGL(kg_copy_if_kernel, dim3((unsigned)gx, (unsigned)njobs), dim3(CP_NT), 0, (hipStream_t)stream, c);
    return kg_launch_status("kg_copy_if");
}
