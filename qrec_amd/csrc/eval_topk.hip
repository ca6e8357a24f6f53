// Full-rank evaluation, the entry points: score every item for a batch of users, mask the user's rated items to 0, keep the N
// largest (base/recommender.py:143-150, util/qmath.py:134-146), then count hits and DCG (util/measure.py).  The argument checks
// and the choice of route live here; the work is in eval_block.hip (every dtype and shape: score block -> mask -> the reference's
// heap) and eval_fused.hip (fp32 from 16,384 items: threshold -> filter -> select, bit-identical to the block route).
#include "common.h"

using namespace qrec;

namespace {

// Measure.hits (util/measure.py:15-21) and the DCG sum of Measure.NDCG (util/measure.py:70-82) for the lists a
// previous qrec_score_topk left on the device: one lane per user walks its first n_cut recommendations in rank
// order, looks each id up in the user's sorted test items and adds the caller's discount[pos] (the host passes
// Python's own 1/math.log(pos+2) doubles) in that order -- the same sequential fp64 sum the reference runs.
__global__ __launch_bounds__(256) void rank_hits_kernel(const int32_t *__restrict__ ids, int n_users, int row_stride, int n_cut,
                                                        const int32_t *__restrict__ user_ids, const int64_t *__restrict__ test_indptr,
                                                        const int32_t *__restrict__ test_items, const double *__restrict__ discount,
                                                        int32_t *__restrict__ hits_out, double *__restrict__ dcg_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_users) return;
    const int u = user_ids[b];
    const int64_t lo0 = test_indptr[u], hi0 = test_indptr[u + 1];
    int hits = 0;
    double dcg = 0.0;
    for (int pos = 0; pos < n_cut; pos++) {
        const int item = ids[(int64_t)b * row_stride + pos];
        if (item < 0) break;                       // -1 padding: fewer than N items exist
        if (sorted_find(test_items + lo0, hi0 - lo0, item) >= 0) { hits++; dcg += discount[pos]; }
    }
    hits_out[b] = hits;
    dcg_out[b] = dcg;
}

}  // namespace

extern "C" {

int qrec_score_topk_scratch_bytes(int dtype, int32_t n_items, int32_t n_batch_users, int32_t ld, int32_t K, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_items >= 0 && n_batch_users >= 0, "qrec_score_topk_scratch_bytes: bad arguments");
    QREC_REQUIRE(dtype == QREC_F32 || dtype == QREC_F64, "qrec_score_topk_scratch_bytes: bad dtype %d", dtype);
    // fused route: bf16 copies, candidate lists, and a block-route scratch for the flagged users' rounds.  Block route: the
    // transposed score block, then the sliced top-N's candidates (scores + ids), flags, flagged list, counter
    *bytes = fused_ok(dtype, ld, n_items, K) && n_batch_users > 0 ? fused_path_bytes(n_items, n_batch_users, ld)
                                                                  : block_path_bytes(dtype, n_items, n_batch_users);
    return QREC_OK;
}

int qrec_score_topk(const void *d_U, const void *d_V, int dtype, int32_t d, int32_t ld, int32_t n_items,
                    const int32_t *d_user_ids, int32_t n_batch_users, const int64_t *d_rated_indptr,
                    const int32_t *d_rated_items, int32_t K, void *d_scratch, int32_t *d_ids_out,
                    void *d_scores_out, void *stream) {
    QREC_REQUIRE(d_U && d_V && d_user_ids && d_scratch && d_ids_out && d_scores_out, "qrec_score_topk: null argument");
    QREC_REQUIRE(dtype == QREC_F32 || dtype == QREC_F64, "qrec_score_topk: bad dtype %d", dtype);
    QREC_REQUIRE(d >= 1 && ld >= d && n_items >= 1 && n_batch_users >= 0, "qrec_score_topk: bad sizes");
    QREC_REQUIRE(ld % (dtype == QREC_F64 ? 16 : 32) == 0,
                 "qrec_score_topk: the row stride must be a multiple of 32 floats / 16 doubles, pad columns zero (got ld=%d)", ld);
    QREC_REQUIRE(K >= 1 && K <= 100, "qrec_score_topk: N must be in 1..100 (base/recommender.py:132-134)");
    QREC_REQUIRE((d_rated_indptr == nullptr) == (d_rated_items == nullptr), "qrec_score_topk: rated CSR incomplete");
    if (n_batch_users == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    if (fused_ok(dtype, ld, n_items, K))
        return run_fused_topk_f32((const float *)d_U, (const float *)d_V, ld, n_items, d_user_ids, n_batch_users, d_rated_indptr,
                                  d_rated_items, K, d_scratch, d_ids_out, (float *)d_scores_out, st);
    return run_score_topk(dtype, d_U, d_V, ld, n_items, d_user_ids, n_batch_users, d_rated_indptr, d_rated_items, K, d_scratch,
                          d_ids_out, d_scores_out, st);
}

int qrec_score_topk_sigmoid_bias_scratch_bytes(int32_t n_items, int32_t n_batch_users, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_items >= 0 && n_batch_users >= 0, "qrec_score_topk_sigmoid_bias_scratch_bytes: bad arguments");
    *bytes = block_path_bytes(QREC_F32, n_items, n_batch_users);
    return QREC_OK;
}

int qrec_score_topk_sigmoid_bias(const float *d_U, const float *d_V, const float *d_item_bias, int32_t d, int32_t ld, int32_t n_items,
                                 const int32_t *d_user_ids, int32_t n_batch_users, const int64_t *d_rated_indptr,
                                 const int32_t *d_rated_items, int32_t K, void *d_scratch, int32_t *d_ids_out, float *d_scores_out,
                                 void *stream) {
    QREC_REQUIRE(d_U && d_V && d_item_bias && d_user_ids && d_scratch && d_ids_out && d_scores_out, "qrec_score_topk_sigmoid_bias: null argument");
    QREC_REQUIRE(d >= 1 && ld >= d && n_items >= 1 && n_batch_users >= 0, "qrec_score_topk_sigmoid_bias: bad sizes");
    QREC_REQUIRE(ld % 32 == 0, "qrec_score_topk_sigmoid_bias: the row stride must be a multiple of 32 floats, pad columns zero (got ld=%d)", ld);
    QREC_REQUIRE(K >= 1 && K <= 100, "qrec_score_topk_sigmoid_bias: N must be in 1..100 (base/recommender.py:132-134)");
    QREC_REQUIRE((d_rated_indptr == nullptr) == (d_rated_items == nullptr), "qrec_score_topk_sigmoid_bias: rated CSR incomplete");
    if (n_batch_users == 0) return QREC_OK;
    return run_score_topk(QREC_F32, d_U, d_V, ld, n_items, d_user_ids, n_batch_users, d_rated_indptr, d_rated_items, K, d_scratch,
                          d_ids_out, d_scores_out, as_stream(stream), d_item_bias);
}

int qrec_score_topk_sparse_row_sigmoid_bias_scratch_bytes(int32_t n_items, int32_t n_batch_users, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_items >= 0 && n_batch_users >= 0, "qrec_score_topk_sparse_row_sigmoid_bias_scratch_bytes: bad arguments");
    *bytes = block_path_bytes(QREC_F32, n_items, n_batch_users);
    return QREC_OK;
}

int qrec_score_topk_sparse_row_sigmoid_bias(const float *d_W, const float *d_item_bias, int32_t ld, int32_t n_items,
                                            const int32_t *d_user_ids, int32_t n_batch_users, const int64_t *d_rated_indptr,
                                            const int32_t *d_rated_items, const float *d_rated_vals, int32_t K, void *d_scratch,
                                            int32_t *d_ids_out, float *d_scores_out, void *stream) {
    QREC_REQUIRE(d_W && d_item_bias && d_user_ids && d_rated_indptr && d_rated_items && d_rated_vals && d_scratch && d_ids_out && d_scores_out,
                 "qrec_score_topk_sparse_row_sigmoid_bias: null argument");
    QREC_REQUIRE(n_items >= 1 && ld >= n_items && n_batch_users >= 0, "qrec_score_topk_sparse_row_sigmoid_bias: bad sizes");
    QREC_REQUIRE(ld % 32 == 0, "qrec_score_topk_sparse_row_sigmoid_bias: the row stride must be a multiple of 32 floats (got ld=%d)", ld);
    QREC_REQUIRE(K >= 1 && K <= 100, "qrec_score_topk_sparse_row_sigmoid_bias: N must be in 1..100 (base/recommender.py:132-134)");
    if (n_items > QREC_CFGAN_MAX_ITEMS) {
        ::qrec::set_error("qrec_score_topk_sparse_row_sigmoid_bias: %d items above the supported %d", n_items, QREC_CFGAN_MAX_ITEMS);
        return QREC_ERR_UNSUPPORTED;
    }
    if (n_batch_users == 0) return QREC_OK;
    const qrec::SparseRows rows{d_W, ld, d_rated_indptr, d_rated_items, d_rated_vals};
    return run_score_topk(QREC_F32, nullptr, nullptr, 32, n_items, d_user_ids, n_batch_users, d_rated_indptr, d_rated_items, K, d_scratch,
                          d_ids_out, d_scores_out, as_stream(stream), d_item_bias, &rows);
}

int qrec_rank_hits(const int32_t *d_ids, int32_t n_batch_users, int32_t row_stride, int32_t n_cut,
                   const int32_t *d_user_ids, const int64_t *d_test_indptr, const int32_t *d_test_items,
                   const double *d_discount, int32_t *d_hits_out, double *d_dcg_out, void *stream) {
    QREC_REQUIRE(d_ids && d_user_ids && d_test_indptr && d_discount && d_hits_out && d_dcg_out, "qrec_rank_hits: null argument");
    QREC_REQUIRE(n_batch_users >= 0 && n_cut >= 1 && row_stride >= n_cut, "qrec_rank_hits: bad sizes");
    if (n_batch_users == 0) return QREC_OK;
    hipLaunchKernelGGL(rank_hits_kernel, dim3((unsigned)((n_batch_users + 255) / 256)), dim3(256), 0, as_stream(stream), d_ids,
                       n_batch_users, row_stride, n_cut, d_user_ids, d_test_indptr, d_test_items, d_discount, d_hits_out,
                       d_dcg_out);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // extern "C"
