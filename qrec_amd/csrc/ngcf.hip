// NGCF's dense propagation layers (model/ranking/NGCF.py:27-42) and their backward pass.
//
//   side = A E (qrec_spmm_csr)
//   pre  = (side + E) W1 + (E * side) W2                       layer_fwd_*<SumProductOps>   (f32 MFMA, mfma_layer.h)
//   act  = leaky_relu(pre, 0.2); nxt = dropout(act, keep); z = l2_normalize(nxt)
//                                                              activate_rows_kernel
//   backward:
//   dnxt = dE_next + normalize_bwd(dz);  dpre = dnxt * gate     dpre_rows_kernel
//   dA1 = dpre W1^T, dA2 = dpre W2^T;  dside = dA1 + dA2*E;  dE = dA1 + dA2*side
//                                                              layer_bwd_*<SumProductOps>   (f32 MFMA)
//   dW1 = (side+E)^T dpre, dW2 = (E*side)^T dpre               layer_wgrad_*<SumProductOps> + wgrad_sum_kernel (MFMA)
//   dE += A^T dside (qrec_spmm_csr with addend)
//
// Tables are [rows][ld] fp32 with ld in {32, 64, 128}; the d x d weights are stored zero-padded as
// [ld][ld].  The N x d x d products are the only GEMM-shaped work (2 N d^2 FLOP each, K = d small):
// one wavefront per 32 rows holds its A fragments in registers and sweeps the output column tiles.
#include "mfma_layer.h"

using namespace qrec;

namespace {

// One group of LPR lanes per row (float4 per lane).  In place on `pre_gate`: reads pre, writes the
// backward gate = (mask/keep) * (pre > 0 ? 1 : 0.2).  Writes nxt, z = l2_normalize(nxt) into the wide
// output table at column offset `out_off` (row stride out_ld), and 1/|nxt|.
template <int LPR>
__global__ __launch_bounds__(256) void activate_rows_kernel(float *__restrict__ pre_gate, int64_t n_rows, int d, float keep,
                                                            const float *__restrict__ mask, uint64_t seed, uint64_t stream_id,
                                                            float *__restrict__ nxt, float *__restrict__ out, int out_ld,
                                                            int out_off, float *__restrict__ inv_norm,
                                                            const int32_t *__restrict__ row_ids, const int32_t *__restrict__ n_ids,
                                                            int64_t philox_row0) {
    constexpr int GPW = kWave / LPR;
    const int lane = threadIdx.x & 63, g = lane / LPR, r = lane % LPR;
    const int64_t gid = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GPW + g;
    const int64_t n_groups = (int64_t)gridDim.x * 4 * GPW;
    const int64_t n_todo = row_ids ? *n_ids : n_rows;
    for (int64_t v = gid; v < n_todo; v += n_groups) {
        const int64_t row = row_ids ? (int64_t)row_ids[v] : v;
        const int64_t off = row * (4 * LPR) + 4 * r;
        const f32x4 p = *reinterpret_cast<const f32x4 *>(pre_gate + off);
        f32x4 fac = {1.f, 1.f, 1.f, 1.f};
        if (keep < 1.f) {
            f32x4 u;
            if (mask) {
                u = *reinterpret_cast<const f32x4 *>(mask + off);       // injected 0/1 keep decisions
                fac = u / keep;
            } else {
                const int64_t grow = row + philox_row0;      // the table row this block row stands for (row-partitioned tables)
                uint32_t c[4] = {(uint32_t)grow, (uint32_t)(grow >> 32) ^ ((uint32_t)r << 8), (uint32_t)stream_id, (uint32_t)(stream_id >> 32)};
                philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
                // tf.nn.dropout: keep iff uniform >= 1 - keep_prob
                fac.x = (uniform24(c[0]) >= 1.f - keep) ? 1.f / keep : 0.f;
                fac.y = (uniform24(c[1]) >= 1.f - keep) ? 1.f / keep : 0.f;
                fac.z = (uniform24(c[2]) >= 1.f - keep) ? 1.f / keep : 0.f;
                fac.w = (uniform24(c[3]) >= 1.f - keep) ? 1.f / keep : 0.f;
            }
        }
        auto lrelu = [](float x) { return fmaxf(0.2f * x, x); };
        f32x4 y = {lrelu(p.x) * fac.x, lrelu(p.y) * fac.y, lrelu(p.z) * fac.z, lrelu(p.w) * fac.w};
        f32x4 gate = {fac.x * (p.x > 0.f ? 1.f : 0.2f), fac.y * (p.y > 0.f ? 1.f : 0.2f),
                      fac.z * (p.z > 0.f ? 1.f : 0.2f), fac.w * (p.w > 0.f ? 1.f : 0.2f)};
        if (4 * r + 0 >= d) { y.x = 0.f; gate.x = 0.f; }
        if (4 * r + 1 >= d) { y.y = 0.f; gate.y = 0.f; }
        if (4 * r + 2 >= d) { y.z = 0.f; gate.z = 0.f; }
        if (4 * r + 3 >= d) { y.w = 0.f; gate.w = 0.f; }
        float ss = y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w;
        ss = row_allreduce_sum<LPR>(ss);
        const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
        *reinterpret_cast<f32x4 *>(pre_gate + off) = gate;
        *reinterpret_cast<f32x4 *>(nxt + off) = y;
        float *o = out + row * out_ld + out_off + 4 * r;      // out_off is not 16-byte aligned in general
        if (4 * r + 0 < d) o[0] = y.x * inv;
        if (4 * r + 1 < d) o[1] = y.y * inv;
        if (4 * r + 2 < d) o[2] = y.z * inv;
        if (4 * r + 3 < d) o[3] = y.w * inv;
        if (r == 0) inv_norm[row] = inv;
    }
}

// dpre = (dE_next + (dz - z (z.dz)) * inv) * gate        (dz, z: wide tables at column offset `off`)
template <int LPR>
__global__ __launch_bounds__(256) void dpre_rows_kernel(const float *__restrict__ dE_next, const float *__restrict__ dAll,
                                                        const float *__restrict__ All, int wide_ld, int col_off,
                                                        const float *__restrict__ inv_norm, const float *__restrict__ gate,
                                                        int64_t n_rows, int d, float *__restrict__ dpre,
                                                        const int32_t *__restrict__ row_ids, const int32_t *__restrict__ n_ids,
                                                        const uint32_t *__restrict__ wide_row_mask) {
    constexpr int GPW = kWave / LPR;
    const int lane = threadIdx.x & 63, g = lane / LPR, r = lane % LPR;
    const int64_t gid = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GPW + g;
    const int64_t n_groups = (int64_t)gridDim.x * 4 * GPW;
    const int64_t n_todo = row_ids ? *n_ids : n_rows;
    for (int64_t v = gid; v < n_todo; v += n_groups) {
        const int64_t row = row_ids ? (int64_t)row_ids[v] : v;
        const int64_t off = row * (4 * LPR) + 4 * r;
        const float *dzp = dAll + row * wide_ld + col_off + 4 * r, *zp = All + row * wide_ld + col_off + 4 * r;
        f32x4 dz = {0.f, 0.f, 0.f, 0.f}, z = dz;
        // wide_row_mask: the wide gradient is only defined (and only non-zero) at the marked rows; elsewhere dz = 0
        const bool has = !wide_row_mask || ((wide_row_mask[row >> 5] >> (row & 31)) & 1u);
        if (has) {
            if (4 * r + 0 < d) { dz.x = dzp[0]; z.x = zp[0]; }
            if (4 * r + 1 < d) { dz.y = dzp[1]; z.y = zp[1]; }
            if (4 * r + 2 < d) { dz.z = dzp[2]; z.z = zp[2]; }
            if (4 * r + 3 < d) { dz.w = dzp[3]; z.w = zp[3]; }
        }
        float dot = z.x * dz.x + z.y * dz.y + z.z * dz.z + z.w * dz.w;
        dot = row_allreduce_sum<LPR>(dot);
        f32x4 dn = (dz - z * dot) * inv_norm[row];
        if (dE_next) dn = dn + *reinterpret_cast<const f32x4 *>(dE_next + off);
        const f32x4 gt = *reinterpret_cast<const f32x4 *>(gate + off);
        *reinterpret_cast<f32x4 *>(dpre + off) = dn * gt;
    }
}

// dst[row][c] (=|+=) src[row][off + c], c < d     (the ego block of the wide table, in and out).  row_ids (may be null):
// only the listed rows are touched
__global__ __launch_bounds__(256) void add_cols_kernel(float *__restrict__ dst, int dst_ld, const float *__restrict__ src,
                                                       int src_ld, int off, int64_t n_rows, int d, int assign,
                                                       const int32_t *__restrict__ row_ids, const int32_t *__restrict__ n_ids) {
    const int64_t total = (row_ids ? (int64_t)*n_ids : n_rows) * d;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = row_ids ? (int64_t)row_ids[k / d] : k / d; const int c = (int)(k % d);
        const float v = src[row * src_ld + off + c];
        if (assign) dst[row * dst_ld + c] = v; else dst[row * dst_ld + c] += v;
    }
}

// X[row][0 .. ld) = 0 for the listed rows: one float4 per thread
__global__ __launch_bounds__(256) void zero_rows_kernel(float *__restrict__ X, int ld, const int32_t *__restrict__ row_ids,
                                                        const int32_t *__restrict__ n_ids) {
    const int per_row = ld / 4;
    const int64_t total = (int64_t)*n_ids * per_row;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x)
        *reinterpret_cast<f32x4 *>(X + (int64_t)row_ids[k / per_row] * ld + 4 * (k % per_row)) = zero;
}

// rows[0 .. count) = the set bits of a row bitmap, ascending.  One block: thread t owns a contiguous run of mask words,
// counts its bits, the block scans the counts, every thread writes its rows.
__global__ __launch_bounds__(1024) void compact_rows_kernel(const uint32_t *__restrict__ mask, int64_t n_rows,
                                                            int32_t *__restrict__ rows, int32_t *__restrict__ count, int capacity) {
    __shared__ int s_wave[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_words = (n_rows + 31) / 32;
    const int64_t per = (n_words + 1023) / 1024, w0 = per * threadIdx.x, w1 = w0 + per < n_words ? w0 + per : n_words;
    auto word = [&](int64_t w) {
        uint32_t m = mask[w];
        if (w == n_words - 1 && (n_rows & 31)) m &= (1u << (n_rows & 31)) - 1u;      // bits past the last row do not count
        return m;
    };
    int mine = 0;
    for (int64_t w = w0; w < w1; w++) mine += __popc(word(w));
    int incl = mine;                                     // inclusive scan inside the wavefront, then over the 16 wavefronts
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, kWave); if (lane >= off) incl += v; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { const int v = s_wave[k]; if (k < wave) base += v; total += v; }
    int pos = base + incl - mine;
    for (int64_t w = w0; w < w1; w++) {
        uint32_t m = word(w);
        while (m) {
            const int b = __ffs(m) - 1; m &= m - 1;
            if (pos < capacity) rows[pos] = (int32_t)(w * 32 + b);
            pos++;
        }
    }
    if (threadIdx.x == 0) *count = total < capacity ? total : capacity;
}

// The whole "which rows does this batch touch" step in one launch, for tables whose bitmap fits the LDS: clear the
// bitmap, mark u / n_users + i / n_users + j, publish the bitmap, emit the ascending row list.  (As three launches --
// memset, qrec_mark_batch_rows, compaction -- it is three launch latencies, ~14 us, for a few KB of work.)
__global__ __launch_bounds__(1024) void mark_compact_kernel(const int32_t *__restrict__ u, const int32_t *__restrict__ i,
                                                            const int32_t *__restrict__ j, int B, int n_users, int64_t n_rows,
                                                            uint32_t *__restrict__ mask_out, int32_t *__restrict__ rows,
                                                            int32_t *__restrict__ count, int capacity,
                                                            double *__restrict__ zero8, int n_zero8) {
    extern __shared__ uint32_t s_mask[];               // n_words words, then 16 wave sums
    if ((int)threadIdx.x < n_zero8) zero8[threadIdx.x] = 0.0;      // the step's scalar accumulators (loss terms): no memset launch for 8 bytes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_words = (n_rows + 31) / 32;
    int *s_wave = reinterpret_cast<int *>(s_mask + n_words);
    for (int64_t w = threadIdx.x; w < n_words; w += 1024) s_mask[w] = 0u;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 1024) {
        const int ru = u[b], ri = n_users + i[b], rj = n_users + j[b];
        atomicOr(&s_mask[ru >> 5], 1u << (ru & 31));
        atomicOr(&s_mask[ri >> 5], 1u << (ri & 31));
        atomicOr(&s_mask[rj >> 5], 1u << (rj & 31));
    }
    __syncthreads();
    for (int64_t w = threadIdx.x; w < n_words; w += 1024) mask_out[w] = s_mask[w];
    const int64_t per = (n_words + 1023) / 1024, w0 = per * threadIdx.x, w1 = w0 + per < n_words ? w0 + per : n_words;
    int mine = 0;
    for (int64_t w = w0; w < w1; w++) mine += __popc(s_mask[w]);
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, kWave); if (lane >= off) incl += v; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { const int v = s_wave[k]; if (k < wave) base += v; total += v; }
    int pos = base + incl - mine;
    for (int64_t w = w0; w < w1; w++) {
        uint32_t m = s_mask[w];
        while (m) {
            const int b = __ffs(m) - 1; m &= m - 1;
            if (rows && pos < capacity) rows[pos] = (int32_t)(w * 32 + b);
            pos++;
        }
    }
    if (count && threadIdx.x == 0) *count = total < capacity ? total : capacity;
}
constexpr int64_t kLdsMaskRows = 1 << 20;              // 128 KB of bitmap

// tf.unique of every batch of an epoch's id stream in one launch (SimGCL.py:61-64 on a device-drawn batch stream): block b
// marks ids[b * batch ...] in an LDS bitmap over [0, id_range) and emits the distinct ids, ascending and shifted by
// out_offset, to rows[b * batch ...]; counts[b] = how many.  (tf.unique keeps first-appearance order; the InfoNCE sums
// that consume the list do not depend on the order beyond fp32 rounding.)
__global__ __launch_bounds__(1024) void unique_per_batch_kernel(const int32_t *__restrict__ ids, int64_t n, int batch, int id_range,
                                                                int out_offset, int32_t *__restrict__ rows, int32_t *__restrict__ counts) {
    extern __shared__ uint32_t s_mask[];               // n_words words, then 16 wave sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_words = (id_range + 31) / 32;
    int *s_wave = reinterpret_cast<int *>(s_mask + n_words);
    const int64_t b0 = (int64_t)blockIdx.x * batch;
    const int B = (int)(n - b0 < batch ? n - b0 : batch);
    for (int w = threadIdx.x; w < n_words; w += 1024) s_mask[w] = 0u;
    __syncthreads();
    for (int k = threadIdx.x; k < B; k += 1024) { const int v = ids[b0 + k]; atomicOr(&s_mask[v >> 5], 1u << (v & 31)); }
    __syncthreads();
    const int per = (n_words + 1023) / 1024, w0 = per * (int)threadIdx.x, w1 = w0 + per < n_words ? w0 + per : n_words;
    int mine = 0;
    for (int w = w0; w < w1; w++) mine += __popc(s_mask[w]);
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, kWave); if (lane >= off) incl += v; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { const int v = s_wave[k]; if (k < wave) base += v; total += v; }
    int pos = base + incl - mine;
    for (int w = w0; w < w1; w++) {
        uint32_t m = s_mask[w];
        while (m) {
            const int b = __ffs(m) - 1; m &= m - 1;
            rows[b0 + pos++] = w * 32 + b + out_offset;
        }
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

}  // namespace

extern "C" {

int qrec_ngcf_dense_fwd(const float *d_E, const float *d_side, const float *d_W1, const float *d_W2, int64_t n_rows,
                        int32_t ld, float *d_pre, const int32_t *d_row_ids, const int32_t *d_n_row_ids, int32_t max_row_ids,
                        void *stream) {
    QREC_REQUIRE(d_E && d_side && d_W1 && d_W2 && d_pre && n_rows >= 0, "qrec_ngcf_dense_fwd: bad argument");
    QREC_REQUIRE(!d_row_ids || (d_n_row_ids && max_row_ids >= 0 && ld <= 64), "qrec_ngcf_dense_fwd: a row subset needs its count, a bound, and ld <= 64");
    const int64_t work_rows = d_row_ids ? max_row_ids : n_rows;
    if (work_rows == 0) return QREC_OK;
    QREC_REQUIRE(ld == 32 || ld == 64 || ld == 128, "qrec_ngcf_dense_fwd: row stride must be 32, 64 or 128 floats (got %d)", ld);
    const float *no_residual = nullptr;
    return launch_layer_fwd<SumProductOps>(as_stream(stream), ld, work_rows, d_E, d_side, d_W1, d_W2, no_residual, n_rows, 0, d_pre,
                                           d_row_ids, d_n_row_ids);
}

int qrec_ngcf_activate(float *d_pre_gate, int64_t n_rows, int32_t d, int32_t ld, float keep, const float *d_mask,
                       uint64_t seed, uint64_t stream_id, float *d_next, float *d_wide, int32_t wide_ld,
                       int32_t col_off, float *d_inv_norm, const int32_t *d_row_ids, const int32_t *d_n_row_ids,
                       int32_t max_row_ids, int64_t philox_row0, void *stream) {
    QREC_REQUIRE(d_pre_gate && d_next && d_wide && d_inv_norm && n_rows >= 0 && d >= 1 && ld >= d && keep > 0.f && keep <= 1.f,
                 "qrec_ngcf_activate: bad argument");
    QREC_REQUIRE(col_off >= 0 && col_off + d <= wide_ld, "qrec_ngcf_activate: column block outside the wide table");
    QREC_REQUIRE(!d_row_ids || (d_n_row_ids && max_row_ids >= 0), "qrec_ngcf_activate: a row subset needs its count and a bound");
    const int64_t work_rows = d_row_ids ? max_row_ids : n_rows;
    if (work_rows == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    int64_t blocks;
#define QREC_ACT(LPR)                                                                                              \
    blocks = (work_rows + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)); if (blocks > 2048) blocks = 2048;                  \
    hipLaunchKernelGGL((activate_rows_kernel<LPR>), dim3((unsigned)blocks), dim3(256), 0, st, d_pre_gate, n_rows, d, keep, \
                       d_mask, seed, stream_id, d_next, d_wide, wide_ld, col_off, d_inv_norm, d_row_ids, d_n_row_ids, philox_row0)
    switch (ld) {
        case 32: QREC_ACT(8); break;
        case 64: QREC_ACT(16); break;
        case 128: QREC_ACT(32); break;
        default: set_error("qrec_ngcf_activate: row stride must be 32, 64 or 128 floats (got %d)", ld); return QREC_ERR_INVALID;
    }
#undef QREC_ACT
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_ngcf_layer_bwd(const float *d_dE_next, const float *d_dWide, const float *d_wide, int32_t wide_ld,
                        int32_t col_off, const float *d_inv_norm, const float *d_gate, const float *d_E,
                        const float *d_side, const float *d_W1, const float *d_W2, int64_t n_rows, int32_t d,
                        int32_t ld, float *d_dpre, float *d_dside, float *d_dE, float *d_partial, float *d_gW1,
                        float *d_gW2, const int32_t *d_row_ids, const int32_t *d_n_row_ids, int32_t max_row_ids,
                        const uint32_t *d_wide_row_mask, void *stream) {
    QREC_REQUIRE(d_dWide && d_wide && d_inv_norm && d_gate && d_E && d_side && d_W1 && d_W2 && d_dpre && d_dside && d_dE &&
                     d_partial && d_gW1 && d_gW2 && n_rows > 0, "qrec_ngcf_layer_bwd: bad argument");
    QREC_REQUIRE(!d_row_ids || (d_n_row_ids && max_row_ids > 0 && ld <= 64), "qrec_ngcf_layer_bwd: a row subset needs its count, a bound > 0, and ld <= 64");
    const int64_t work_rows = d_row_ids ? max_row_ids : n_rows;
    hipStream_t st = as_stream(stream);
    int64_t blocks;
#define QREC_DP(LPR)                                                                                              \
    blocks = (work_rows + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)); if (blocks > 2048) blocks = 2048;                 \
    hipLaunchKernelGGL((dpre_rows_kernel<LPR>), dim3((unsigned)blocks), dim3(256), 0, st, d_dE_next, d_dWide, d_wide, \
                       wide_ld, col_off, d_inv_norm, d_gate, n_rows, d, d_dpre, d_row_ids, d_n_row_ids, d_wide_row_mask)
    switch (ld) {
        case 32: QREC_DP(8); break;
        case 64: QREC_DP(16); break;
        case 128: QREC_DP(32); break;
        default: set_error("qrec_ngcf_layer_bwd: row stride must be 32, 64 or 128 floats (got %d)", ld); return QREC_ERR_INVALID;
    }
#undef QREC_DP
    QREC_LAUNCH_CHECK();
    // X[0] = E, X[1] = side: the kernels write dX[0] = dE, dX[1] = dside
    const int rc = launch_layer_bwd<SumProductOps>(st, ld, work_rows, d_dpre, d_W1, d_W2, d_E, d_side, n_rows, 0, d_dE, d_dside, d_row_ids,
                                                   d_n_row_ids);
    if (rc != QREC_OK) return rc;
    return launch_layer_wgrad<SumProductOps>(st, ld, work_rows, d_E, d_side, d_dpre, n_rows, d_partial, d_row_ids, d_n_row_ids, d_gW1, d_gW2);
}

int qrec_ngcf_wgrad_partial_bytes(int64_t n_rows, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_rows >= 0 && ld > 0, "qrec_ngcf_wgrad_partial_bytes: bad argument");
    *bytes = wgrad_slabs(n_rows, ld) * 2 * (int64_t)ld * ld * 4;
    return QREC_OK;
}

int qrec_compact_marked_rows(const uint32_t *d_row_mask, int64_t n_rows, int32_t *d_rows, int32_t *d_count, int32_t capacity,
                             void *stream) {
    QREC_REQUIRE(d_row_mask && d_rows && d_count && n_rows >= 0 && n_rows < (1ll << 31) && capacity >= 0, "qrec_compact_marked_rows: bad argument");
    hipLaunchKernelGGL(compact_rows_kernel, dim3(1), dim3(1024), 0, as_stream(stream), d_row_mask, n_rows, d_rows, d_count, capacity);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_mark_compact_batch_rows(const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int32_t B, int32_t n_users,
                                 int64_t n_rows, uint32_t *d_row_mask, int32_t *d_rows, int32_t *d_count, int32_t capacity,
                                 double *d_zero8, int32_t n_zero8, void *stream) {
    QREC_REQUIRE(d_row_mask && B >= 0 && n_users >= 0 && n_rows >= n_users && n_rows < (1ll << 31) && capacity >= 0 &&
                 (!d_rows == !d_count) && n_zero8 >= 0 && n_zero8 <= 64 && (n_zero8 == 0 || d_zero8),
                 "qrec_mark_compact_batch_rows: bad argument");
    QREC_REQUIRE(B == 0 || (d_u && d_i && d_j), "qrec_mark_compact_batch_rows: null index array");
    hipStream_t st = as_stream(stream);
    const int64_t n_words = (n_rows + 31) / 32;
    if (n_rows <= kLdsMaskRows) {
        const size_t lds = (size_t)n_words * 4 + 64;
        QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(&mark_compact_kernel), lds));
        hipLaunchKernelGGL(mark_compact_kernel, dim3(1), dim3(1024), lds, st, d_u, d_i, d_j, B, n_users, n_rows, d_row_mask, d_rows,
                           d_count, capacity, d_zero8, n_zero8);
        QREC_LAUNCH_CHECK();
        return QREC_OK;
    }
    if (n_zero8) QREC_HIP_CHECK(hipMemsetAsync(d_zero8, 0, (size_t)n_zero8 * 8, st));
    QREC_HIP_CHECK(hipMemsetAsync(d_row_mask, 0, (size_t)n_words * 4, st));
    int rc = qrec_mark_batch_rows(d_u, d_i, d_j, B, n_users, d_row_mask, stream);
    if (rc != QREC_OK || !d_rows) return rc;
    return qrec_compact_marked_rows(d_row_mask, n_rows, d_rows, d_count, capacity, stream);
}

int qrec_unique_per_batch(const int32_t *d_ids, int64_t n, int32_t batch, int32_t id_range, int32_t out_offset, int32_t *d_rows,
                          int32_t *d_counts, void *stream) {
    QREC_REQUIRE(n >= 0 && batch >= 1 && id_range >= 1 && id_range <= kLdsMaskRows, "qrec_unique_per_batch: bad sizes (id_range <= 2^20)");
    QREC_REQUIRE(n == 0 || (d_ids && d_rows && d_counts), "qrec_unique_per_batch: null argument");
    if (n == 0) return QREC_OK;
    const size_t lds = (size_t)((id_range + 31) / 32) * 4 + 64;
    QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(&unique_per_batch_kernel), lds));
    hipLaunchKernelGGL(unique_per_batch_kernel, dim3((unsigned)((n + batch - 1) / batch)), dim3(1024), lds, as_stream(stream), d_ids, n, batch,
                       id_range, out_offset, d_rows, d_counts);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_copy_cols(float *d_dst, int32_t dst_ld, const float *d_src, int32_t src_ld, int32_t src_col_off, int64_t n_rows,
                   int32_t d, int32_t accumulate, const int32_t *d_row_ids, const int32_t *d_n_row_ids, int32_t max_row_ids,
                   void *stream) {
    QREC_REQUIRE(d_dst && d_src && n_rows >= 0 && d >= 1 && d <= dst_ld && src_col_off >= 0 && src_col_off + d <= src_ld,
                 "qrec_copy_cols: bad argument");
    QREC_REQUIRE(!d_row_ids || (d_n_row_ids && max_row_ids >= 0), "qrec_copy_cols: a row subset needs its count and a bound");
    const int64_t work_rows = d_row_ids ? max_row_ids : n_rows;
    if (work_rows == 0) return QREC_OK;
    int64_t blocks = (work_rows * d + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(add_cols_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), d_dst, dst_ld, d_src, src_ld,
                       src_col_off, n_rows, d, accumulate ? 0 : 1, d_row_ids, d_n_row_ids);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_zero_rows(float *d_X, int32_t ld, const int32_t *d_row_ids, const int32_t *d_n_row_ids, int32_t max_row_ids, void *stream) {
    QREC_REQUIRE(d_X && d_row_ids && d_n_row_ids && ld > 0 && ld % 4 == 0 && max_row_ids >= 0, "qrec_zero_rows: bad argument");
    if (max_row_ids == 0) return QREC_OK;
    int64_t blocks = ((int64_t)max_row_ids * (ld / 4) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), d_X, ld, d_row_ids, d_n_row_ids);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // extern "C"
