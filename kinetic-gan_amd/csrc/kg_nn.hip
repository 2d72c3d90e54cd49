// Exact k-nearest-neighbour search between two point sets of many classes in two launches (see include/kgan_hip.h,
// DESIGN.md 22).  Per class: Q query and N base points of dimension D; for every query the k base points with the smallest
// (d2, j) - squared distance, then base index - and their distances.
//
// kg_nn_search_kernel: one workgroup = TI queries of one class x one chunk of base points.  It walks the column tiles of its
// chunk; the squared distances of a TI x TI tile are the shared tile body of kg_prdc (kg_dist_tile.h: direct differences,
// one fmaf chain per pair in dimension order, so a pair's bits depend on the two points alone), the load going through the
// optional affine of its side ((x * scale) + shift as two separately rounded operations; staged zeros stay zero).  After
// each tile the k best (value, index) of every row are merged with the tile's TI new ones in LDS by the rank merge of
// kg_prdc_radii_kernel: the best so far come from lower columns and are sorted, the tile's candidates lie in column order,
// so "ties broken by position" IS the order (d2, j).  Only the best carry a stored index: tile candidate c is column
// j0 + c.  Pair i == j is left out by index when asked.  The chunk's list goes to the workspace; entries a short chunk
// cannot fill are (inf, INT_MAX).
// kg_nn_merge_kernel: one wave per (class, query); every one of the row's split * k candidates finds its rank under
// (d2, j, position) among all of them and the ones ranked below k are written at their rank.
// The order is total and no bit of a pair depends on the plan: every (tile, split) gives the same idx and d2.  No atomics,
// no tickets, no Q x N matrix, no scratch, no dynamically indexed private array.
// kg_nn_sets: up to KG_NN_MAX_SETS query sets with shared strides against ONE base in the same two launches -
// the workgroup index of the search is (set, class, row tile, chunk), a merge row is (set, class, query).  A set only chooses
// the query pointer and the output row, so every set's bits are those of kg_nn on it; kg_nn IS the one-set case: one
// kernel body, one plan, one launcher (nn_run).
// kg_nn_scores_kernel: from the nearest neighbour of every query of every set to the two memorisation tallies - authentic
// (d2 >= the neighbour's own leave-one-out distance) and agreeing (the neighbour carries the query's label) - one workgroup
// per set, integer LDS tallies, one owner per output word.
// The search and merge kernels, their plan, validation and launcher live in kg_nn_search.h: kg_nn_gram.hip runs
// the same bodies over a list of rows; kg_nn and kg_nn_sets are their identity case.
#include "kg_nn_search.h"

namespace {

// ---- kg_nn_scores: one workgroup per set ---------------------------------------------------------------------------------
constexpr int NS_NT = 256;                  // threads of the scores workgroup
constexpr int NS_MAXC = KG_NN_SCORES_MAX_CLASSES;

// set s = blockIdx.x.  The tallies are integers in LDS (integer addition does not depend on the order), the totals a shuffle
// tree and NS_NT / 64 words; every output word has one owner and is written on every call.  An index outside [0, N) is
// outside the definition: the query is SKIPPED (nothing is read for it, it counts nowhere); a query label outside
// [0, n_classes) counts in the totals and in no class.
__global__ __launch_bounds__(NS_NT) void kg_nn_scores_kernel(const KgNnScoresArgs a) {
    __shared__ int cls_s[NS_MAXC][2];
    __shared__ int tot_s[NS_NT / 64][2];
    const int tid = threadIdx.x, s = blockIdx.x, K = a.n_classes, Q = a.Q;
    for (int c = tid; c < K; c += NS_NT) { cls_s[c][0] = 0; cls_s[c][1] = 0; }
    __syncthreads();
    const int32_t* idx = a.idx + (long)s * Q * a.ld;
    const float* d2 = a.d2 + (long)s * Q * a.ld;
    int na = 0, ng = 0;
    for (int j = tid; j < Q; j += NS_NT) {
        const int i = idx[(long)j * a.ld];
        if (i < 0 || i >= a.N) continue;
        const int y = a.query_labels[j];
        const int au = d2[(long)j * a.ld] >= a.base_loo[i] ? 1 : 0;
        const int ag = a.base_labels[i] == y ? 1 : 0;
        na += au;
        ng += ag;
        if (a.counts_per_class && y >= 0 && y < K) {
            if (au) atomicAdd(&cls_s[y][0], 1);
            if (ag) atomicAdd(&cls_s[y][1], 1);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        na += __shfl_xor(na, off, 64);
        ng += __shfl_xor(ng, off, 64);
    }
    if ((tid & 63) == 0) { tot_s[tid >> 6][0] = na; tot_s[tid >> 6][1] = ng; }
    __syncthreads();
    if (a.counts_per_class)
        for (int c = tid; c < K; c += NS_NT) {
            a.counts_per_class[((long)s * K + c) * 2 + 0] = cls_s[c][0];
            a.counts_per_class[((long)s * K + c) * 2 + 1] = cls_s[c][1];
        }
    if (tid >= 2) return;
    long total = 0;
    for (int w = 0; w < NS_NT / 64; ++w) total += tot_s[w][tid];
    const double share = (double)total / (double)Q;
    a.counts[s * 2 + tid] = total;
    a.scores64[s * 2 + tid] = share;
    a.scores[s * 2 + tid] = (float)share;
}

// the one-set call as the general one (its own fields: exclude_self, which a group of sets does not have)
KgNnSetsArgs nn_one_set(const KgNnArgs* a) {
    KgNnSetsArgs s = {};
    s.query[0] = a->query;  s.q_sc = a->q_sc;  s.q_sp = a->q_sp;  s.q_so = a->q_so;  s.nsets = 1;
    s.base = a->base;  s.b_sc = a->b_sc;  s.b_sp = a->b_sp;  s.b_so = a->b_so;
    s.Q = a->Q;  s.N = a->N;  s.d_outer = a->d_outer;  s.d_inner = a->d_inner;  s.classes = a->classes;  s.k = a->k;
    s.q_affine = a->q_affine;  s.b_affine = a->b_affine;
    s.q_scale = a->q_scale;  s.q_shift = a->q_shift;  s.b_scale = a->b_scale;  s.b_shift = a->b_shift;
    s.tile = a->tile;  s.split = a->split;
    s.idx = a->idx;  s.d2 = a->d2;  s.ws = a->ws;  s.ws_bytes = a->ws_bytes;
    return s;
}

// the one launcher: search, then merge, of nsets sets (validated by the caller)
int nn_run(const KgNnSetsArgs* a, int exclude_self, bool sets, const char* who, void* stream) {
    if (sets) {
        for (int g = 0; g < a->nsets; ++g) KG_REQUIRE(a->query[g] != nullptr, "%s: null pointer query[%d]", who, g);
    } else {
        KG_REQUIRE(a->query[0] != nullptr, "%s: null pointer query", who);
    }
    KG_REQUIRE(a->base != nullptr, "%s: null pointer base", who);
    KG_REQUIRE(a->idx != nullptr, "%s: null pointer idx", who);
    KG_REQUIRE(a->d2 != nullptr, "%s: null pointer d2", who);
    KG_REQUIRE(a->ws != nullptr, "%s: null pointer ws", who);
    const NnPlan p = nn_plan(a);
    const int64_t need = nn_ws_bytes(a, p);
    KG_REQUIRE(a->ws_bytes >= need, "%s: ws_bytes=%lld < %lld (%s_workspace_bytes)", who, (long long)a->ws_bytes, (long long)need,
               who);
    NnDev d = nn_dev(a, exclude_self, p);
    d.pd = (float*)a->ws;
    d.pj = (int*)(d.pd + (long)a->nsets * a->classes * a->Q * p.split * a->k);
    return nn_launch<false>(d, p, sets ? "kg_nn_sets_search" : "kg_nn_search", sets ? "kg_nn_sets_merge" : "kg_nn_merge",
                            (hipStream_t)stream);
}

}  // namespace

extern "C" int64_t kg_nn_workspace_bytes(const KgNnArgs* a) {
    KG_REQUIRE(a != nullptr, "kg_nn_workspace_bytes: null args");
    const KgNnSetsArgs s = nn_one_set(a);
    if (int rc = nn_validate(&s, a->exclude_self, false, "kg_nn_workspace_bytes")) return rc;
    return nn_ws_bytes(&s, nn_plan(&s));
}

extern "C" int kg_nn(const KgNnArgs* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_nn: null args");
    const KgNnSetsArgs s = nn_one_set(a);
    if (int rc = nn_validate(&s, a->exclude_self, false, "kg_nn")) return rc;
    return nn_run(&s, a->exclude_self, false, "kg_nn", stream);
}

extern "C" int64_t kg_nn_sets_workspace_bytes(const KgNnSetsArgs* a) {
    KG_REQUIRE(a != nullptr, "kg_nn_sets_workspace_bytes: null args");
    if (int rc = nn_validate(a, 0, true, "kg_nn_sets_workspace_bytes")) return rc;
    return nn_ws_bytes(a, nn_plan(a));
}

extern "C" int kg_nn_sets(const KgNnSetsArgs* a, void* stream) {
    KG_REQUIRE(a != nullptr, "kg_nn_sets: null args");
    if (int rc = nn_validate(a, 0, true, "kg_nn_sets")) return rc;
    return nn_run(a, 0, true, "kg_nn_sets", stream);
}

extern "C" int kg_nn_scores(const KgNnScoresArgs* a, void* stream) {
    const char* who = "kg_nn_scores";
    KG_REQUIRE(a != nullptr, "%s: null args", who);
    KG_REQUIRE(a->nsets >= 1 && a->nsets <= KG_NN_MAX_SETS, "%s: nsets=%d outside [1, %d]", who, a->nsets, KG_NN_MAX_SETS);
    KG_REQUIRE(a->Q >= 1, "%s: Q=%d < 1", who, a->Q);
    KG_REQUIRE(a->N >= 1, "%s: N=%d < 1", who, a->N);
    KG_REQUIRE(a->Q <= KG_NN_MAX_POINTS, "%s: Q=%d above the cap of %d points", who, a->Q, KG_NN_MAX_POINTS);
    KG_REQUIRE(a->N <= KG_NN_MAX_POINTS, "%s: N=%d above the cap of %d points", who, a->N, KG_NN_MAX_POINTS);
    KG_REQUIRE(a->n_classes >= 1 && a->n_classes <= NS_MAXC, "%s: n_classes=%d outside [1, %d]", who, a->n_classes, NS_MAXC);
    KG_REQUIRE(a->ld >= 1, "%s: ld=%lld < 1", who, (long long)a->ld);
    KG_REQUIRE(a->idx != nullptr, "%s: null pointer idx", who);
    KG_REQUIRE(a->d2 != nullptr, "%s: null pointer d2", who);
    KG_REQUIRE(a->query_labels != nullptr, "%s: null pointer query_labels", who);
    KG_REQUIRE(a->base_labels != nullptr, "%s: null pointer base_labels", who);
    KG_REQUIRE(a->base_loo != nullptr, "%s: null pointer base_loo", who);
    KG_REQUIRE(a->counts != nullptr, "%s: null pointer counts", who);
    KG_REQUIRE(a->scores64 != nullptr, "%s: null pointer scores64", who);
    KG_REQUIRE(a->scores != nullptr, "%s: null pointer scores", who);
    hipLaunchKernelGGL(kg_nn_scores_kernel, dim3(a->nsets), dim3(NS_NT), 0, (hipStream_t)stream, *a);
    return kg_launch_status(who);
}
