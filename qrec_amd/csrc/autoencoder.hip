// CDAE (model/ranking/CDAE.py): the denoising auto-encoder over a whole user row, evaluated where the reference's dense
// batch x n_items arithmetic is non-zero only -- a sparse gather-sum encoder, a SAMPLED decoder (one dot product per live
// loss position), their transposed weight-gradient passes over the item-major views of the same lists, and the loss.
// fp32 throughout, fp64 for the loss sums.  No batch x n_items array exists, no float atomic is used: every sum below has
// one fixed order (list order inside a batch row, then batch-row order), so two launches give the same bits.
//
// Shapes: tables [rows][ld], ld a multiple of 32 up to QREC_CDAE_MAX_LD, columns [nh, ld) zero.  The decoder weight is
// item-major ([n_items][ld]), so both weight tables are read and written one row per item.
// These kernels are gather- and latency-bound (a few thousand rows of <= 1 KB per step), not MFMA work: what matters is
// that every row read is one coalesced wave access and that enough independent rows are in flight.
#include "common.h"

namespace {

using namespace qrec;

constexpr int kSplit = QREC_CDAE_SPLIT;          // workgroups per batch row in the decoder
constexpr int kRegBlocks = QREC_CDAE_REG_BLOCKS;

// workspace layout (qrec_cdae_workspace_bytes): doubles first, then the decoder's partial dh rows
struct Ws {
    double *loss_part;   // [B * kSplit]  sum of the loss terms of one decoder workgroup
    double *vsq;         // [B]           sum of squares of V[u_b]
    double *reg_part;    // [kRegBlocks]  partial sums of squares of the four weight variables
    float *dh_part;      // [B * kSplit][ld]
};
__host__ __device__ inline Ws ws_layout(Carver &c, int B, int ld) {
    return {c.take<double>((size_t)B * kSplit), c.take<double>((size_t)B), c.take<double>(kRegBlocks), c.take<float>((size_t)B * kSplit * ld)};
}

// ---- encoder: one workgroup per batch row, one thread per hidden column ------------------------------------------------
__global__ __launch_bounds__(256) void encode_kernel(const float *__restrict__ Wenc, const float *__restrict__ benc,
                                                     const float *__restrict__ V, int n_items, int n_users, int nh, int ld,
                                                     const int32_t *__restrict__ users, const int32_t *__restrict__ in_ptr,
                                                     const int32_t *__restrict__ in_item, const float *__restrict__ in_val,
                                                     float *__restrict__ h) {
    const int b = blockIdx.x, c = threadIdx.x;
    const int beg = in_ptr[b], end = in_ptr[b + 1];
    float z = 0.0f;
    int e = beg;
    for (; e + 4 <= end; e += 4) {        // four independent row reads in flight, added in list order
        int it[4]; float x[4], w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { it[q] = in_item[e + q]; x[q] = in_val[e + q]; }
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = (unsigned)it[q] < (unsigned)n_items ? Wenc[(size_t)it[q] * ld + c] : 0.0f;
#pragma unroll
        for (int q = 0; q < 4; q++) z += x[q] * w[q];
    }
    for (; e < end; e++) {
        const int it = in_item[e];
        if ((unsigned)it < (unsigned)n_items) z += in_val[e] * Wenc[(size_t)it * ld + c];
    }
    const int u = users[b];
    const float v = (unsigned)u < (unsigned)n_users ? V[(size_t)u * ld + c] : 0.0f;
    h[(size_t)b * ld + c] = c < nh ? sigmoidf(z + benc[c] + v) : 0.0f;       // padding columns stay zero
}

// ---- sampled decoder + loss + upstream gradient ------------------------------------------------------------------------
// kSplit workgroups per batch row, each a contiguous share of the row's live slots; inside a workgroup the four wavefronts
// take the share's slots round-robin, 64 lanes across the hidden columns (NK = ceil(ld / 64) columns per lane).  The item's
// decoder row is read once: for the dot product, then, still in registers, for the row's contribution to dh.
template <int NK>
__global__ __launch_bounds__(256) void decode_kernel(const float *__restrict__ Wdec, const float *__restrict__ bdec, int n_items,
                                                     int ld, const float *__restrict__ h, const int32_t *__restrict__ lv_ptr,
                                                     const int32_t *__restrict__ lv_item, const int32_t *__restrict__ lv_label,
                                                     float scale, float *__restrict__ g_out, float *__restrict__ dh_part,
                                                     double *__restrict__ loss_part) {
    __shared__ float acc_lds[4][QREC_CDAE_MAX_LD];
    __shared__ double loss_lds[4];
    const int b = blockIdx.x / kSplit, part = blockIdx.x % kSplit;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int beg = lv_ptr[b], cnt = lv_ptr[b + 1] - beg;
    const int per = (cnt + kSplit - 1) / kSplit;
    const int lo = beg + (part * per < cnt ? part * per : cnt), hi = beg + ((part + 1) * per < cnt ? (part + 1) * per : cnt);
    float hr[NK], acc[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int c = lane + 64 * k;
        hr[k] = c < ld ? h[(size_t)b * ld + c] : 0.0f;
        acc[k] = 0.0f;
    }
    double loss = 0.0;
    for (int s = lo + wave; s < hi; s += 4) {
        const int it = lv_item[s];
        const bool ok = (unsigned)it < (unsigned)n_items;
        float w[NK], p = 0.0f;
#pragma unroll
        for (int k = 0; k < NK; k++) {
            const int c = lane + 64 * k;
            w[k] = ok && c < ld ? Wdec[(size_t)it * ld + c] : 0.0f;
            p += hr[k] * w[k];
        }
        const float logit = wave_sum_dpp(p) + (ok ? bdec[it] : 0.0f);
        const float y = sigmoidf(logit);
        const bool pass = y >= 1e-6f;                      // tf.maximum(1e-6, y): the gradient reaches y only here
        const float yc = pass ? y : 1e-6f;
        float g, term;
        if (lv_label[s]) { term = -logf(yc); g = pass ? -(1.0f - y) : 0.0f; }
        else             { term = -logf(1.0f - yc); g = pass ? y : 0.0f; }
        if (!ok) { g = 0.0f; term = 0.0f; }
        g *= scale;
        loss += (double)term;
        if (lane == 0) g_out[s] = g;
#pragma unroll
        for (int k = 0; k < NK; k++) acc[k] += g * w[k];
    }
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int c = lane + 64 * k;
        if (c < ld) acc_lds[wave][c] = acc[k];
    }
    if (lane == 0) loss_lds[wave] = loss;
    __syncthreads();
    for (int c = threadIdx.x; c < ld; c += 256)
        dh_part[(size_t)blockIdx.x * ld + c] = ((acc_lds[0][c] + acc_lds[1][c]) + acc_lds[2][c]) + acc_lds[3][c];
    if (threadIdx.x == 0) loss_part[blockIdx.x] = ((loss_lds[0] + loss_lds[1]) + loss_lds[2]) + loss_lds[3];
}

// ---- hidden backward: dh_b = the kSplit partial rows in order, dz_b = dh_b h_b (1 - h_b) -------------------------------
__global__ __launch_bounds__(256) void hidden_bwd_kernel(const float *__restrict__ h, const float *__restrict__ dh_part, int ld,
                                                         float *__restrict__ dz) {
    const int b = blockIdx.x, c = threadIdx.x;
    float dh = 0.0f;
#pragma unroll
    for (int p = 0; p < kSplit; p++) dh += dh_part[((size_t)b * kSplit + p) * ld + c];
    const float hv = h[(size_t)b * ld + c];
    dz[(size_t)b * ld + c] = dh * hv * (1.0f - hv);
}

// g_V[u] = sum over the batch rows b with u_b = u, ascending b, of (dz_b + reg V[u]) -- one term PER OCCURRENCE, as the
// reference's l2_loss of the gathered rows counts a user drawn twice two times.  The first occurrence of a user does the sum.
__global__ __launch_bounds__(256) void user_grad_kernel(const float *__restrict__ dz, const float *__restrict__ V, int n_users, int nh,
                                                        int ld, const int32_t *__restrict__ users, int B, float reg,
                                                        float *__restrict__ gV, double *__restrict__ vsq) {
    __shared__ double red[256];
    const int b = blockIdx.x, c = threadIdx.x;
    const int u = users[b];
    const bool ok = (unsigned)u < (unsigned)n_users;
    const float v = ok ? V[(size_t)u * ld + c] : 0.0f;
    const double sq = block_sum_fixed(c < nh ? (double)v * (double)v : 0.0, red);
    if (c == 0) vsq[b] = sq;
    if (!ok) return;
    for (int k = 0; k < b; k++)
        if (users[k] == u) return;
    float acc = 0.0f;
    for (int k = b; k < B; k++)
        if (users[k] == u) acc += dz[(size_t)k * ld + c] + reg * v;
    gV[(size_t)u * ld + c] = acc;
}

// g_benc = sum over b of dz_b, ascending b
__global__ __launch_bounds__(256) void bias_grad_kernel(const float *__restrict__ dz, int ld, int B, float *__restrict__ gbenc) {
    const int c = threadIdx.x;
    float acc = 0.0f;
    for (int b = 0; b < B; b++) acc += dz[(size_t)b * ld + c];
    gbenc[c] = acc;
}

// ---- weight gradients by item over the item-major views; one workgroup per item, one thread per column ----------------
// Every item's rows are written, so the rows of items absent from a view come out exactly zero without a fill.
__global__ __launch_bounds__(256) void weight_grad_kernel(const float *__restrict__ h, const float *__restrict__ dz,
                                                          const float *__restrict__ g, int ld, int B, int64_t n_live, int n_item_blocks,
                                                          const int32_t *__restrict__ lv_cptr, const int32_t *__restrict__ lv_crow,
                                                          const int32_t *__restrict__ lv_cslot, const int32_t *__restrict__ in_cptr,
                                                          const int32_t *__restrict__ in_crow, const float *__restrict__ in_cval,
                                                          float *__restrict__ gWdec, float *__restrict__ gbdec, float *__restrict__ gWenc) {
    const int c = threadIdx.x;
    for (int it = blockIdx.x; it < n_item_blocks; it += gridDim.x) {
        float acc = 0.0f, gsum = 0.0f;
        for (int e = lv_cptr[it], end = lv_cptr[it + 1]; e < end; e++) {
            const int b = lv_crow[e], s = lv_cslot[e];
            if ((unsigned)b >= (unsigned)B || (uint64_t)(int64_t)s >= (uint64_t)n_live) continue;
            const float gs = g[s];
            acc += gs * h[(size_t)b * ld + c];
            gsum += gs;
        }
        gWdec[(size_t)it * ld + c] = acc;
        if (c == 0) gbdec[it] = gsum;
        acc = 0.0f;
        for (int e = in_cptr[it], end = in_cptr[it + 1]; e < end; e++) {
            const int b = in_crow[e];
            if ((unsigned)b >= (unsigned)B) continue;
            acc += in_cval[e] * dz[(size_t)b * ld + c];
        }
        gWenc[(size_t)it * ld + c] = acc;
    }
}

// ---- the loss the reference prints: reduce_mean of the dense block + regU * (l2_loss of the four weights + of V[u_b]) --
__global__ __launch_bounds__(256) void reg_part_kernel(const float *__restrict__ theta, int64_t n, double *__restrict__ reg_part) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)kRegBlocks * 256) {
        const double x = theta[k];
        s += x * x;
    }
    s = block_sum_fixed(s, red);
    if (threadIdx.x == 0) reg_part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void loss_kernel(const double *__restrict__ loss_part, int n_parts, const double *__restrict__ vsq, int B,
                                                   const double *__restrict__ reg_part, double scale, double reg, double *__restrict__ out) {
    __shared__ double red[256];
    double a = 0.0, r = 0.0;
    for (int k = threadIdx.x; k < n_parts; k += 256) a += loss_part[k];
    for (int k = threadIdx.x; k < B; k += 256) r += vsq[k];
    r += reg_part[threadIdx.x];                      // kRegBlocks == the workgroup's size
    a = block_sum_fixed(a, red);
    r = block_sum_fixed(r, red);
    if (threadIdx.x == 0) out[0] = a * scale + reg * 0.5 * r;
}
static_assert(kRegBlocks == 256, "loss_kernel reads one regulariser partial per thread");

// ---- S = sigmoid(S + bias[item]) over the transposed score block of the evaluation (eval_block.hip) ---------------------
__global__ __launch_bounds__(256) void sigmoid_bias_kernel(float *__restrict__ S_T, const float *__restrict__ bias, int n_items, int b_pad) {
    const int64_t n = (int64_t)n_items * b_pad;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256)
        S_T[k] = sigmoidf(S_T[k] + bias[k / b_pad]);
}

// ---- throughput mode: the batch drawn and its lists built on the device -------------------------------------------------
// Same distribution as the reference's loop (np.random.binomial mask, choice(userList), 5 |rated| rejection draws of
// choice(itemList), negatives a set), not its streams: every draw is Philox4x32-10 of (seed, step, position), so the lists
// depend on nothing else.  Per batch row two bitmaps over the items (rated, sampled) make the negatives a set and give the
// ascending order for free; the keep decision is evaluated only at the set bits.
constexpr uint32_t kTagUser = 0x75736572u, kTagNeg = 0x6e656761u, kTagKeep = 0x6b656570u;
constexpr uint32_t kMaxDrawBlocks = 4096;          // a row whose user rated every item draws no negative (the reference would not return)

// draw workspace (qrec_cdae_draw_workspace_bytes): four [B][W] word arrays, W = ceil(n_items / 32)
struct DrawWs {
    uint32_t *pos;      // rated bits; after keep_kernel the kept inputs (rated and kept)
    uint32_t *neg;      // sampled bits; after keep_kernel the live positions ((rated or sampled) and kept)
    int32_t *in_pre;    // kept inputs of the row in the words before this one
    int32_t *lv_pre;    // live positions of the row in the words before this one
};
__host__ __device__ inline DrawWs draw_layout(Carver &c, int B, int W) {
    const size_t n = (size_t)B * W;       // neg right behind pos: one memset clears both
    return {c.take<uint32_t>(n), c.take<uint32_t>(n), c.take<int32_t>(n), c.take<int32_t>(n)};
}

// index of item in the ascending row, or -1
__device__ inline int find_sorted(const int32_t *row, int len, int item) { return sorted_find(row, len, item); }

// one workgroup per batch row: the user, the bits of its rated items, the bits of its per_rated * |rated| negatives.
// The bitmaps are zero on entry; integer OR makes the result independent of the order the draws land in.
__global__ __launch_bounds__(256) void draw_row_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ rated, int n_users,
                                                       int n_items, int W, int per_rated, uint32_t seed_lo, uint32_t seed_hi,
                                                       uint32_t step_lo, uint32_t step_hi, int ushift, int ishift,
                                                       int32_t *__restrict__ users, uint32_t *__restrict__ pos, uint32_t *__restrict__ neg) {
    __shared__ int s_user;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int u = 0;
        for (uint32_t block = 0, done = 0; !done && block < kMaxDrawBlocks; block++) {
            uint32_t c[4] = {(uint32_t)b, 0u, block, step_lo};
            philox4x32_10(c, seed_lo ^ kTagUser, seed_hi ^ step_hi);
            for (int w = 0; w < 4 && !done; w++) {
                const uint32_t r = c[w] >> ushift;
                if (r < (uint32_t)n_users) { u = (int)r; done = 1; }
            }
        }
        s_user = u;
        users[b] = u;
    }
    __syncthreads();
    const int u = s_user;
    const int64_t beg = indptr[u];
    const int len = (int)(indptr[u + 1] - beg);
    const int32_t *row = rated + beg;
    uint32_t *prow = pos + (size_t)b * W, *nrow = neg + (size_t)b * W;
    for (int e = threadIdx.x; e < len; e += 256) {
        const int it = row[e];
        if ((unsigned)it < (unsigned)n_items) atomicOr(&prow[it >> 5], 1u << (it & 31));
    }
    if (len >= n_items) return;
    const int64_t n_draws = (int64_t)per_rated * len;
    for (int64_t t = threadIdx.x; t < n_draws; t += 256) {
        for (uint32_t block = 0, done = 0; !done && block < kMaxDrawBlocks; block++) {
            uint32_t c[4] = {(uint32_t)t, (uint32_t)b, block, step_lo};
            philox4x32_10(c, seed_lo ^ kTagNeg, seed_hi ^ step_hi);
            for (int w = 0; w < 4 && !done; w++) {
                const uint32_t r = c[w] >> ishift;
                if (r >= (uint32_t)n_items || find_sorted(row, len, (int)r) >= 0) continue;
                atomicOr(&nrow[r >> 5], 1u << (r & 31));
                done = 1;
            }
        }
    }
}

// keep decision of (step, row, item): one Philox block per position, evaluated only where the row has a rated or sampled bit
__device__ inline bool keep_position(uint32_t item, uint32_t b, uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi,
                                     double keep_prob) {
    uint32_t c[4] = {item, b, step_lo, step_hi};
    philox4x32_10(c, seed_lo ^ kTagKeep, seed_hi);
    return (double)c[0] * (1.0 / 4294967296.0) < keep_prob;
}

// one workgroup per batch row, each thread a contiguous share of the row's words: apply the keep decisions, then the
// row's running counts per word and its totals (raw counts into in_ptr[b] / lv_ptr[b]; scan_kernel turns them into pointers)
__global__ __launch_bounds__(256) void keep_kernel(int n_items, int W, double keep_prob, uint32_t seed_lo, uint32_t seed_hi,
                                                   uint32_t step_lo, uint32_t step_hi, uint32_t *__restrict__ pos,
                                                   uint32_t *__restrict__ neg, int32_t *__restrict__ in_pre, int32_t *__restrict__ lv_pre,
                                                   int32_t *__restrict__ in_cnt, int32_t *__restrict__ lv_cnt, int32_t *__restrict__ cand_cnt) {
    __shared__ int s_in[256], s_lv[256], s_cand[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int per = (W + 255) / 256;
    const int lo = t * per < W ? t * per : W, hi = (t + 1) * per < W ? (t + 1) * per : W;
    uint32_t *prow = pos + (size_t)b * W, *nrow = neg + (size_t)b * W;
    int n_in = 0, n_lv = 0, n_cand = 0;
    for (int w = lo; w < hi; w++) {
        const uint32_t p = prow[w], cand = p | nrow[w];
        uint32_t keep = 0;
        for (uint32_t rest = cand; rest; rest &= rest - 1) {
            const int bit = __ffs(rest) - 1;
            if (keep_position((uint32_t)(w * 32 + bit), (uint32_t)b, seed_lo, seed_hi, step_lo, step_hi, keep_prob)) keep |= 1u << bit;
        }
        prow[w] = p & keep; nrow[w] = cand & keep;
        n_in += __popc(p & keep); n_lv += __popc(cand & keep); n_cand += __popc(cand);
    }
    s_in[t] = n_in; s_lv[t] = n_lv; s_cand[t] = n_cand;
    __syncthreads();
    int a_in = 0, a_lv = 0;
    for (int k = 0; k < t; k++) { a_in += s_in[k]; a_lv += s_lv[k]; }
    for (int w = lo; w < hi; w++) {          // this thread's own words, written above
        in_pre[(size_t)b * W + w] = a_in; lv_pre[(size_t)b * W + w] = a_lv;
        a_in += __popc(prow[w]); a_lv += __popc(nrow[w]);
    }
    if (t == 255) {
        int c = 0;
        for (int k = 0; k < 256; k++) c += s_cand[k];
        in_cnt[b] = a_in; lv_cnt[b] = a_lv;
        if (cand_cnt) cand_cnt[b] = c;
    }
    (void)n_items;
}

// per item the number of batch rows that keep it as input / hold it live (raw counts; scan_kernel makes the pointers)
__global__ __launch_bounds__(256) void item_count_kernel(int n_items, int W, int B, const uint32_t *__restrict__ in_bits,
                                                         const uint32_t *__restrict__ lv_bits, int32_t *__restrict__ in_cnt,
                                                         int32_t *__restrict__ lv_cnt) {
    const int it = blockIdx.x * 256 + threadIdx.x;
    if (it >= n_items) return;
    const int w = it >> 5, bit = it & 31;
    int n_in = 0, n_lv = 0;
    for (int b = 0; b < B; b++) {
        n_in += (in_bits[(size_t)b * W + w] >> bit) & 1u;
        n_lv += (lv_bits[(size_t)b * W + w] >> bit) & 1u;
    }
    in_cnt[it] = n_in; lv_cnt[it] = n_lv;
}

// counts a[0, n) -> exclusive pointers a[0, n], in place, each clamped to cap; one workgroup per array
struct ScanJob { int32_t *a; int n; int64_t cap; };
struct ScanJobs { ScanJob j[4]; };
__global__ __launch_bounds__(1024) void scan_kernel(ScanJobs jobs) {
    __shared__ int64_t s_sum[1024];
    const ScanJob job = jobs.j[blockIdx.x];
    const int t = threadIdx.x;
    const int per = (job.n + 1 + 1023) / 1024;
    const int lo = t * per < job.n + 1 ? t * per : job.n + 1, hi = (t + 1) * per < job.n + 1 ? (t + 1) * per : job.n + 1;
    int64_t s = 0;
    for (int k = lo; k < hi; k++) s += k < job.n ? job.a[k] : 0;
    s_sum[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int k = 0; k < 1024; k++) { const int64_t v = s_sum[k]; s_sum[k] = run; run += v; }
    }
    __syncthreads();
    int64_t run = s_sum[t];
    for (int k = lo; k < hi; k++) {
        const int64_t v = k < job.n ? job.a[k] : 0;
        job.a[k] = (int32_t)(run < job.cap ? run : job.cap);
        run += v;
    }
}

// row-major lists: one workgroup per batch row, a thread per word, items ascending by construction
__global__ __launch_bounds__(256) void fill_rows_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ rated,
                                                        const float *__restrict__ rated_vals, int W, const int32_t *__restrict__ users,
                                                        const uint32_t *__restrict__ in_bits, const uint32_t *__restrict__ lv_bits,
                                                        const int32_t *__restrict__ in_pre, const int32_t *__restrict__ lv_pre,
                                                        const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ lv_ptr,
                                                        int64_t cap_in, int64_t cap_live, int32_t *__restrict__ in_item,
                                                        float *__restrict__ in_val, int32_t *__restrict__ lv_item, int32_t *__restrict__ lv_label) {
    const int b = blockIdx.x;
    const int u = users[b];
    const int64_t beg = indptr[u];
    const int len = (int)(indptr[u + 1] - beg);
    for (int w = threadIdx.x; w < W; w += 256) {
        const uint32_t in = in_bits[(size_t)b * W + w], lv = lv_bits[(size_t)b * W + w];
        int64_t s = (int64_t)lv_ptr[b] + lv_pre[(size_t)b * W + w];
        for (uint32_t rest = lv; rest; rest &= rest - 1, s++) {
            const int bit = __ffs(rest) - 1;
            if (s < cap_live) { lv_item[s] = w * 32 + bit; lv_label[s] = (int32_t)((in >> bit) & 1u); }
        }
        s = (int64_t)in_ptr[b] + in_pre[(size_t)b * W + w];
        for (uint32_t rest = in; rest; rest &= rest - 1, s++) {
            const int it = w * 32 + __ffs(rest) - 1;
            const int e = find_sorted(rated + beg, len, it);
            if (s < cap_in) { in_item[s] = it; in_val[s] = e >= 0 ? rated_vals[beg + e] : 0.0f; }
        }
    }
}

// item-major views: a thread per item walks the batch rows in ascending order; a live entry carries its CSR slot
__global__ __launch_bounds__(256) void fill_items_kernel(int n_items, int W, int B, const uint32_t *__restrict__ in_bits,
                                                         const uint32_t *__restrict__ lv_bits, const int32_t *__restrict__ in_pre,
                                                         const int32_t *__restrict__ lv_pre, const int32_t *__restrict__ in_ptr,
                                                         const int32_t *__restrict__ lv_ptr, const int32_t *__restrict__ in_cptr,
                                                         const int32_t *__restrict__ lv_cptr, const float *__restrict__ in_val,
                                                         int64_t cap_in, int64_t cap_live, int32_t *__restrict__ in_crow,
                                                         float *__restrict__ in_cval, int32_t *__restrict__ lv_crow, int32_t *__restrict__ lv_cslot) {
    const int it = blockIdx.x * 256 + threadIdx.x;
    if (it >= n_items) return;
    const int w = it >> 5, bit = it & 31;
    const uint32_t below = (1u << bit) - 1u;
    int64_t e_in = in_cptr[it], e_lv = lv_cptr[it];
    for (int b = 0; b < B; b++) {
        const size_t k = (size_t)b * W + w;
        const uint32_t in = in_bits[k], lv = lv_bits[k];
        if ((lv >> bit) & 1u) {
            const int64_t slot = (int64_t)lv_ptr[b] + lv_pre[k] + __popc(lv & below);
            if (e_lv < cap_live && slot < cap_live) { lv_crow[e_lv] = b; lv_cslot[e_lv] = (int32_t)slot; }
            e_lv++;
        }
        if ((in >> bit) & 1u) {
            const int64_t slot = (int64_t)in_ptr[b] + in_pre[k] + __popc(in & below);
            if (e_in < cap_in && slot < cap_in) { in_crow[e_in] = b; in_cval[e_in] = in_val[slot]; }
            e_in++;
        }
    }
}

bool ld_ok(int nh, int ld) { return nh >= 1 && ld >= nh && ld % 32 == 0; }

}  // namespace

namespace qrec {
// the element-wise pass of qrec_score_topk_sigmoid_bias; S_T is the block route's [n_items][b_pad] score block
int score_block_sigmoid_bias(float *S_T, const float *bias, int n_items, int b_pad, hipStream_t st) {
    int64_t blocks = ((int64_t)n_items * b_pad + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sigmoid_bias_kernel, dim3((unsigned)blocks), dim3(256), 0, st, S_T, bias, n_items, b_pad);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}
}  // namespace qrec

extern "C" {

#define QREC_CDAE_WIDTH(name)                                                                                              \
    do {                                                                                                                   \
        QREC_REQUIRE(ld_ok(nh, ld), name ": bad width (nh=%d, ld=%d; ld must be a multiple of 32 and >= nh)", nh, ld);     \
        if (ld > QREC_CDAE_MAX_LD) {                                                                                       \
            ::qrec::set_error(name ": hidden width %d (row stride %d) above the supported %d", nh, ld, QREC_CDAE_MAX_LD);  \
            return QREC_ERR_UNSUPPORTED;                                                                                   \
        }                                                                                                                  \
    } while (0)

int qrec_cdae_workspace_bytes(int32_t B, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && B >= 0 && ld >= 1, "qrec_cdae_workspace_bytes: bad arguments");
    *bytes = layout_bytes(ws_layout, B, ld);
    return QREC_OK;
}

int qrec_cdae_encode(const float *d_Wenc, const float *d_benc, const float *d_V, int32_t n_items, int32_t n_users, int32_t nh,
                     int32_t ld, const int32_t *d_users, int32_t B, const int32_t *d_in_ptr, const int32_t *d_in_item,
                     const float *d_in_val, float *d_h, void *stream) {
    QREC_CDAE_WIDTH("qrec_cdae_encode");
    QREC_REQUIRE(B >= 0 && n_items >= 1 && n_users >= 1, "qrec_cdae_encode: bad sizes");
    if (B == 0) return QREC_OK;
    QREC_REQUIRE(d_Wenc && d_benc && d_V && d_users && d_in_ptr && d_h, "qrec_cdae_encode: null argument");
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)B), dim3((unsigned)ld), 0, as_stream(stream), d_Wenc, d_benc, d_V, n_items, n_users,
                       nh, ld, d_users, d_in_ptr, d_in_item, d_in_val, d_h);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_cdae_decode(const float *d_Wdec, const float *d_bdec, int32_t n_items, int32_t nh, int32_t ld, const float *d_h, int32_t B,
                     const int32_t *d_lv_ptr, const int32_t *d_lv_item, const int32_t *d_lv_label, float *d_g, void *d_ws,
                     void *stream) {
    QREC_CDAE_WIDTH("qrec_cdae_decode");
    QREC_REQUIRE(B >= 0 && n_items >= 1, "qrec_cdae_decode: bad sizes");
    if (B == 0) return QREC_OK;
    QREC_REQUIRE(d_Wdec && d_bdec && d_h && d_lv_ptr && d_ws, "qrec_cdae_decode: null argument");
    const Ws w = carve(d_ws, ws_layout, B, ld);
    const float scale = (float)(1.0 / ((double)B * (double)n_items));
    const dim3 grid((unsigned)B * kSplit);
#define QREC_CDAE_DECODE(NK)                                                                                                       \
    hipLaunchKernelGGL(decode_kernel<NK>, grid, dim3(256), 0, as_stream(stream), d_Wdec, d_bdec, n_items, ld, d_h, d_lv_ptr, d_lv_item, \
                       d_lv_label, scale, d_g, w.dh_part, w.loss_part)
    if (ld <= 64) QREC_CDAE_DECODE(1);
    else if (ld <= 128) QREC_CDAE_DECODE(2);
    else if (ld <= 192) QREC_CDAE_DECODE(3);
    else QREC_CDAE_DECODE(4);
#undef QREC_CDAE_DECODE
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_cdae_hidden_bwd(const float *d_h, const float *d_V, int32_t n_users, int32_t nh, int32_t ld, const int32_t *d_users, int32_t B,
                         float reg, void *d_ws, float *d_dz, float *d_gbenc, float *d_gV, void *stream) {
    QREC_CDAE_WIDTH("qrec_cdae_hidden_bwd");
    QREC_REQUIRE(B >= 0 && n_users >= 1 && d_gbenc && d_gV, "qrec_cdae_hidden_bwd: bad arguments");
    hipStream_t st = as_stream(stream);
    QREC_HIP_CHECK(hipMemsetAsync(d_gV, 0, sizeof(float) * (size_t)n_users * ld, st));
    QREC_HIP_CHECK(hipMemsetAsync(d_gbenc, 0, sizeof(float) * (size_t)ld, st));
    if (B == 0) return QREC_OK;
    QREC_REQUIRE(d_h && d_V && d_users && d_ws && d_dz, "qrec_cdae_hidden_bwd: null argument");
    const Ws w = carve(d_ws, ws_layout, B, ld);
    hipLaunchKernelGGL(hidden_bwd_kernel, dim3((unsigned)B), dim3((unsigned)ld), 0, st, d_h, w.dh_part, ld, d_dz);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(user_grad_kernel, dim3((unsigned)B), dim3((unsigned)ld), 0, st, d_dz, d_V, n_users, nh, ld, d_users, B, reg, d_gV,
                       w.vsq);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(bias_grad_kernel, dim3(1), dim3((unsigned)ld), 0, st, d_dz, ld, B, d_gbenc);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_cdae_weight_grads(const float *d_h, const float *d_dz, const float *d_g, int32_t n_items, int32_t nh, int32_t ld, int32_t B,
                           int64_t n_live, const int32_t *d_lv_cptr, const int32_t *d_lv_crow, const int32_t *d_lv_cslot,
                           const int32_t *d_in_cptr, const int32_t *d_in_crow, const float *d_in_cval, float *d_gWdec, float *d_gbdec,
                           float *d_gWenc, void *stream) {
    QREC_CDAE_WIDTH("qrec_cdae_weight_grads");
    QREC_REQUIRE(B >= 0 && n_items >= 1 && n_live >= 0, "qrec_cdae_weight_grads: bad sizes");
    QREC_REQUIRE(d_lv_cptr && d_in_cptr && d_gWdec && d_gbdec && d_gWenc && (B == 0 || (d_h && d_dz)),
                 "qrec_cdae_weight_grads: null argument");
    const int blocks = n_items < 65536 ? n_items : 65536;
    hipLaunchKernelGGL(weight_grad_kernel, dim3((unsigned)blocks), dim3((unsigned)ld), 0, as_stream(stream), d_h, d_dz, d_g, ld, B, n_live,
                       n_items, d_lv_cptr, d_lv_crow, d_lv_cslot, d_in_cptr, d_in_crow, d_in_cval, d_gWdec, d_gbdec, d_gWenc);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_cdae_loss(const float *d_theta, int64_t n_theta, float reg, int32_t B, int32_t n_items, int32_t ld, void *d_ws, double *d_loss,
                   void *stream) {
    QREC_REQUIRE(d_theta && n_theta >= 0 && B >= 1 && n_items >= 1 && ld >= 1 && d_ws && d_loss, "qrec_cdae_loss: bad arguments");
    const Ws w = carve(d_ws, ws_layout, B, ld);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(reg_part_kernel, dim3(kRegBlocks), dim3(256), 0, st, d_theta, n_theta, w.reg_part);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(256), 0, st, w.loss_part, B * kSplit, w.vsq, B, w.reg_part,
                       1.0 / ((double)B * (double)n_items), (double)reg, d_loss);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_cdae_draw_workspace_bytes(int32_t B, int32_t n_items, int64_t *bytes) {
    QREC_REQUIRE(bytes && B >= 0 && n_items >= 1, "qrec_cdae_draw_workspace_bytes: bad arguments");
    *bytes = layout_bytes(draw_layout, B, (n_items + 31) / 32);
    return QREC_OK;
}

int qrec_cdae_draw_batch(const int64_t *d_rated_indptr, const int32_t *d_rated_items, const float *d_rated_vals, int32_t n_users,
                         int32_t n_items, int32_t B, int32_t per_rated, float keep_prob, uint64_t seed, uint64_t step, int64_t cap_in,
                         int64_t cap_live, void *d_ws, int32_t *d_users, int32_t *d_in_ptr, int32_t *d_in_item, float *d_in_val,
                         int32_t *d_in_cptr, int32_t *d_in_crow, float *d_in_cval, int32_t *d_lv_ptr, int32_t *d_lv_item,
                         int32_t *d_lv_label, int32_t *d_lv_cptr, int32_t *d_lv_crow, int32_t *d_lv_cslot, int32_t *d_cand_count,
                         void *stream) {
    QREC_REQUIRE(n_users >= 1 && n_items >= 1 && B >= 1 && per_rated >= 0 && cap_in >= 1 && cap_live >= 1 && cap_in <= INT32_MAX &&
                     cap_live <= INT32_MAX && keep_prob >= 0.0f && keep_prob <= 1.0f,
                 "qrec_cdae_draw_batch: bad sizes");
    QREC_REQUIRE(d_rated_indptr && d_rated_items && d_rated_vals && d_ws && d_users && d_in_ptr && d_in_item && d_in_val && d_in_cptr &&
                     d_in_crow && d_in_cval && d_lv_ptr && d_lv_item && d_lv_label && d_lv_cptr && d_lv_crow && d_lv_cslot,
                 "qrec_cdae_draw_batch: null argument");
    const int W = (n_items + 31) / 32;
    const DrawWs w = carve(d_ws, draw_layout, B, W);
    hipStream_t st = as_stream(stream);
    const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32), step_lo = (uint32_t)step, step_hi = (uint32_t)(step >> 32);
    QREC_HIP_CHECK(hipMemsetAsync(w.pos, 0, sizeof(uint32_t) * 2 * (size_t)B * W, st));
    hipLaunchKernelGGL(draw_row_kernel, dim3((unsigned)B), dim3(256), 0, st, d_rated_indptr, d_rated_items, n_users, n_items, W, per_rated,
                       seed_lo, seed_hi, step_lo, step_hi, __builtin_clz((uint32_t)n_users), __builtin_clz((uint32_t)n_items), d_users,
                       w.pos, w.neg);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(keep_kernel, dim3((unsigned)B), dim3(256), 0, st, n_items, W, (double)keep_prob, seed_lo, seed_hi, step_lo, step_hi,
                       w.pos, w.neg, w.in_pre, w.lv_pre, d_in_ptr, d_lv_ptr, d_cand_count);
    QREC_LAUNCH_CHECK();
    const unsigned item_blocks = (unsigned)((n_items + 255) / 256);
    hipLaunchKernelGGL(item_count_kernel, dim3(item_blocks), dim3(256), 0, st, n_items, W, B, w.pos, w.neg, d_in_cptr, d_lv_cptr);
    QREC_LAUNCH_CHECK();
    ScanJobs jobs = {{{d_in_ptr, B, cap_in}, {d_lv_ptr, B, cap_live}, {d_in_cptr, n_items, cap_in}, {d_lv_cptr, n_items, cap_live}}};
    hipLaunchKernelGGL(scan_kernel, dim3(4), dim3(1024), 0, st, jobs);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(fill_rows_kernel, dim3((unsigned)B), dim3(256), 0, st, d_rated_indptr, d_rated_items, d_rated_vals, W, d_users, w.pos,
                       w.neg, w.in_pre, w.lv_pre, d_in_ptr, d_lv_ptr, cap_in, cap_live, d_in_item, d_in_val, d_lv_item, d_lv_label);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(fill_items_kernel, dim3(item_blocks), dim3(256), 0, st, n_items, W, B, w.pos, w.neg, w.in_pre, w.lv_pre, d_in_ptr,
                       d_lv_ptr, d_in_cptr, d_lv_cptr, d_in_val, cap_in, cap_live, d_in_crow, d_in_cval, d_lv_crow, d_lv_cslot);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

#undef QREC_CDAE_WIDTH

}  // extern "C"
