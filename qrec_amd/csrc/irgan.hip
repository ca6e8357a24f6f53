// IRGAN (model/ranking/IRGAN.py): a categorical distribution over the whole item table per user -- tempered softmax, its CDF,
// many draws from it -- and the policy-gradient step whose gradient is dense over the item table, followed by TF's dense Adam.
// Both towers score P[u] . Q[i] + b[i]; here an item table carries its bias in column d of the row ([Q | b], d + 1 <= ld), and
// the user's row is read as [P[u] | 1], so one dot product gives the logit and one row update moves weights and bias alike.
// fp32 throughout, fp64 for the CDF and the loss sums.  No float atomic: every sum has one fixed order, two launches give the
// same bits.  Plain launches on the caller's stream, nothing is read back.
//
// The chain of a generator step (B = 1) and of get_data (B = a block of users):
//   logits_kernel     z = ([P[u] | 1] . Qb[j]) / T for a tile of 256 items per workgroup, with the tile's max and sum of exps
//   rowstat_kernel    the row's max and  S = sum_j exp(z_j - max)  from the tiles' pairs, in tile order
//   weights_kernel    w_j (negatives: exp(z - max), 0 at positives; mixture: pn), p_j = softmax, and per chunk of 64 items the
//                     fp64 sum of w in index order
//   scan_kernel       inclusive fp64 prefix sums of the chunk sums, in index order
//   draw_kernel       inverse CDF, searchsorted(.., 'right'): binary search over the chunk sums, then the walk inside the chunk in
//                     the order the chunk's sum was formed -- so the walk always ends on an item of non-zero weight
//   reward_kernel     2 (sigmoid([P_d[u] | 1] . Qb_d[i]) - 1/2) p_i / pn_i per sample
//   gen_prep / sort / gen_walk / gen_sums   c_j, n_j (sample order inside an item: stable radix sort + walk), R and the loss
//   gen_item_kernel   g_j, Adam on Qb_g[j] without an [n_items][ld] gradient, per-workgroup partial rows of sum_j g_j Qb_g[j]
//   gen_user_kernel   the partial rows added in workgroup order -> row u of the user table's gradient buffer
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.h"

namespace {

using namespace qrec;

constexpr int kChunk = QREC_IRGAN_CHUNK;        // items per CDF chunk = one wavefront
constexpr int kTile = 256;                      // items per logits workgroup
constexpr int kItemsPerWave = 16;               // gen_item_kernel: items a wavefront walks, 64 per workgroup
constexpr uint32_t kTagDraw = 0x69726764u;

// the uniform of (seed, step, row, k) in [0, 1): 53 bits, formed as numpy's random_sample forms its doubles
__device__ inline double draw_uniform(uint64_t seed, uint64_t step, uint32_t row, uint32_t k) {
    uint32_t c[4] = {(uint32_t)step, (uint32_t)(step >> 32), row, k};
    philox4x32_10(c, (uint32_t)seed ^ kTagDraw, (uint32_t)(seed >> 32));
    return ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) / 9007199254740992.0;
}

// row b of the draws: the last b with ptr[b] <= s
__device__ inline int row_of(const int64_t *__restrict__ ptr, int B, int64_t s) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline bool in_sorted(const int32_t *__restrict__ row, int64_t len, int item) { return sorted_find(row, len, item) >= 0; }

// the user's row as [P[u] | 1 | 0 ...] on the lanes of a wavefront, NK columns per lane; a user outside the table reads as zeros
template <int NK>
__device__ inline void load_user_row(const float *__restrict__ P, int n_users, int d, int ld, int u, int lane, float (&pu)[NK]) {
    const bool ok = (unsigned)u < (unsigned)n_users;
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int c = lane + 64 * k;
        pu[k] = !ok ? 0.0f : c < d ? P[(size_t)u * ld + c] : c == d ? 1.0f : 0.0f;
    }
}
template <int NK>
__device__ inline void load_row(const float *__restrict__ Q, int ld, int j, bool ok, int lane, float (&q)[NK]) {
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int c = lane + 64 * k;
        q[k] = ok && c < ld ? Q[(size_t)j * ld + c] : 0.0f;
    }
}

// ---- logits of one row against a tile of items ------------------------------------------------------------------------------
template <int NK>
__global__ __launch_bounds__(256) void logits_kernel(const float *__restrict__ P, const float *__restrict__ Q, int n_users, int n_items,
                                                     int d, int ld, const int32_t *__restrict__ users, float temperature,
                                                     float *__restrict__ z, float *__restrict__ tile_max, double *__restrict__ tile_sum) {
    __shared__ float mx[4];
    __shared__ double sm[4];
    const int b = blockIdx.y, tile = blockIdx.x, n_tiles = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float pu[NK];
    load_user_row<NK>(P, n_users, d, ld, users[b], lane, pu);
    const int base = tile * kTile + wave * 64;
    float mine = 0.0f;
#pragma unroll 4
    for (int i = 0; i < 64; i++) {
        const int j = base + i;
        float q[NK], s = 0.0f;
        load_row<NK>(Q, ld, j, j < n_items, lane, q);
#pragma unroll
        for (int k = 0; k < NK; k++) s += pu[k] * q[k];
        s = wave_sum_dpp(s);
        if (lane == i) mine = s;
    }
    const int j = base + lane;
    const bool live = j < n_items;
    const float zt = mine / temperature;                     // the reference divides the float32 logits by the temperature
    if (live) z[(size_t)b * n_items + j] = zt;
    float m = live ? zt : -INFINITY;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, kWave));
    if (lane == 0) mx[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3]));      // the tile's first wavefront always holds a live item
    const double e = wave_sum_dpp(live ? (double)expf(zt - m) : 0.0);
    if (lane == 0) sm[wave] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_max[(size_t)b * n_tiles + tile] = m;
        tile_sum[(size_t)b * n_tiles + tile] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    }
}

__global__ __launch_bounds__(256) void rowstat_kernel(const float *__restrict__ tile_max, const double *__restrict__ tile_sum, int n_tiles,
                                                      float *__restrict__ row_max, double *__restrict__ row_sum) {
    __shared__ double lds[256];
    __shared__ float mx[256];
    const int b = blockIdx.x, t = threadIdx.x;
    float m = -INFINITY;
    for (int k = t; k < n_tiles; k += 256) m = fmaxf(m, tile_max[(size_t)b * n_tiles + k]);
    mx[t] = m;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) mx[t] = fmaxf(mx[t], mx[t + s]);
        __syncthreads();
    }
    m = mx[0];
    double acc = 0.0;
    for (int k = t; k < n_tiles; k += 256) acc += tile_sum[(size_t)b * n_tiles + k] * (double)expf(tile_max[(size_t)b * n_tiles + k] - m);
    acc = block_sum_fixed(acc, lds);
    if (t == 0) { row_max[b] = m; row_sum[b] = acc; }
}

// ---- weights: one wavefront per chunk of 64 items ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void weights_kernel(const float *__restrict__ z, int n_items, int n_users, const int32_t *__restrict__ users,
                                                      const int64_t *__restrict__ pos_indptr, const int32_t *__restrict__ pos_items, int mode,
                                                      float keep, float mix, const float *__restrict__ row_max,
                                                      const double *__restrict__ row_sum, float *__restrict__ w_out, float *__restrict__ p_out,
                                                      int n_chunks, double *__restrict__ chunk_sum) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_chunks) return;
    const int u = users[b];
    const bool uok = (unsigned)u < (unsigned)n_users;
    const int64_t pbeg = uok ? pos_indptr[u] : 0, plen = uok ? pos_indptr[u + 1] - pbeg : 0;
    const int j = c * kChunk + lane;
    const bool live = j < n_items;
    const float e = live ? expf(z[(size_t)b * n_items + j] - row_max[b]) : 0.0f;
    const bool pos = live && plen > 0 && in_sorted(pos_items + pbeg, plen, j);
    float w;
    if (mode == QREC_IRGAN_NEGATIVES) {
        w = pos ? 0.0f : e;
        if (live && p_out) p_out[(size_t)b * n_items + j] = e;
    } else {
        const float p = e / (float)row_sum[b];
        w = keep * p;
        if (pos) w += mix / (float)plen;
        if (!live) w = 0.0f;
        if (live && p_out) p_out[(size_t)b * n_items + j] = p;
    }
    if (live) w_out[(size_t)b * n_items + j] = w;
    double run = 0.0;                                         // index order, the order draw_kernel walks the chunk in
#pragma unroll
    for (int i = 0; i < kChunk; i++) run += (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), i));
    if (lane == 0) chunk_sum[(size_t)b * n_chunks + c] = run;
}

__global__ __launch_bounds__(256) void scan_kernel(double *__restrict__ chunk_sum, int n_chunks) {
    __shared__ double buf[1024];
    double *row = chunk_sum + (size_t)blockIdx.x * n_chunks;
    double run = 0.0;                                         // thread 0's
    for (int base = 0; base < n_chunks; base += 1024) {
        const int n = n_chunks - base < 1024 ? n_chunks - base : 1024;
        for (int k = threadIdx.x; k < n; k += 256) buf[k] = row[base + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < n; k++) { run += buf[k]; buf[k] = run; }
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += 256) row[base + k] = buf[k];
        __syncthreads();
    }
}

// ---- draws ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void draw_kernel(const float *__restrict__ w, const double *__restrict__ csum, int n_items, int n_chunks, int B,
                                                   const int64_t *__restrict__ draw_ptr, int64_t n_draws, const double *__restrict__ uniforms,
                                                   uint64_t seed, uint64_t step, int32_t *__restrict__ samples, double *__restrict__ uniforms_out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_draws) return;
    const int b = row_of(draw_ptr, B, s);
    const double x = uniforms ? uniforms[s] : draw_uniform(seed, step, (uint32_t)b, (uint32_t)(s - draw_ptr[b]));
    if (uniforms_out) { uniforms_out[s] = x; return; }
    const double *cs = csum + (size_t)b * n_chunks;
    const double total = cs[n_chunks - 1];
    if (!(total > 0.0) || !(x >= 0.0)) { samples[s] = -1; return; }          // an all-zero row has no draw (the reference divides 0 by 0)
    double t = x * total;
    if (!(t < total)) t = __longlong_as_double(__double_as_longlong(total) - 1);   // x < 1: stay below the last CDF value
    int lo = 0, hi = n_chunks - 1;                            // first chunk whose inclusive sum exceeds t; cs[last] > t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cs[mid] > t) hi = mid; else lo = mid + 1;
    }
    const double base = lo ? cs[lo - 1] : 0.0;
    const float *wr = w + (size_t)b * n_items;
    double run = 0.0;
    int found = -1, last_nz = -1;
#pragma unroll 8
    for (int i = 0; i < kChunk; i++) {
        const int j = lo * kChunk + i;
        const float wv = j < n_items ? wr[j] : 0.0f;
        run += (double)wv;
        if (wv > 0.0f) last_nz = j;
        if (found < 0 && base + run > t) found = j;
    }
    samples[s] = found >= 0 ? found : last_nz;
}

// ---- reward per sample: one wavefront per draw ------------------------------------------------------------------------------
template <int NK>
__global__ __launch_bounds__(256) void reward_kernel(const float *__restrict__ P, const float *__restrict__ Q, int n_users, int n_items, int d,
                                                     int ld, const int32_t *__restrict__ users, int B, const int64_t *__restrict__ draw_ptr,
                                                     int64_t n_draws, const int32_t *__restrict__ samples, const float *__restrict__ p,
                                                     const float *__restrict__ w, float *__restrict__ reward) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_draws) return;
    const int lane = threadIdx.x & 63;
    const int b = row_of(draw_ptr, B, s);
    const int i = samples[s];
    const bool ok = (unsigned)i < (unsigned)n_items;
    float pu[NK], q[NK], acc = 0.0f;
    load_user_row<NK>(P, n_users, d, ld, users[b], lane, pu);
    load_row<NK>(Q, ld, i, ok, lane, q);
#pragma unroll
    for (int k = 0; k < NK; k++) acc += pu[k] * q[k];
    const float logit = wave_sum_dpp(acc);
    if (lane == 0) {
        float r = 0.0f;
        if (ok) {
            const size_t at = (size_t)b * n_items + i;
            // as the reference's float32 graph forms it: near x = 0 the subtraction cancels, and its recorded losses carry that
            // rounding (tanh(x / 2), the same function without the cancellation, leaves the recorded run by 1.2e-5)
            r = 2.0f * (sigmoidf(logit) - 0.5f) * p[at] / w[at];
        }
        reward[s] = r;
    }
}

// ---- generator step ---------------------------------------------------------------------------------------------------------
struct GenWs {
    int32_t *keys, *keys_sorted, *slots_sorted;   // [K]
    double *term, *l2;                            // [K] log p_i r, 1/2 |Qb[i]|^2
    double *scal;                                 // [2] R, K as counted
    float *c; int32_t *n;                         // [n_items] each, contiguous (one memset)
    float *part;                                  // [n_blocks][ld]
    void *temp; size_t temp_bytes;
};
int gen_sort_bytes(int64_t K, size_t *bytes) {
    size_t tb = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, (const int32_t *)nullptr, (int32_t *)nullptr, rocprim::counting_iterator<int32_t>(0),
                                                   (int32_t *)nullptr, (size_t)(K > 0 ? K : 1), 0u, 32u, (hipStream_t)0);
    QREC_REQUIRE(e == hipSuccess, "irgan: rocprim::radix_sort_pairs size query failed");
    *bytes = align_up(tb ? tb : 256, 256);
    return QREC_OK;
}
inline int gen_blocks(int n_items) { return (n_items + 4 * kItemsPerWave - 1) / (4 * kItemsPerWave); }
// the layout of a generator step's workspace, stated once: sized on a null base, carved on the caller's buffer
int gen_layout(Carver &c, int n_items, int ld, int64_t K, GenWs *g) {
    size_t tb = 0;
    const int rc = gen_sort_bytes(K, &tb);
    if (rc != QREC_OK) return rc;
    const size_t kk = (size_t)(K > 0 ? K : 1), ni = (size_t)n_items;
    g->term = c.take<double>(kk, 256);
    g->l2 = c.take<double>(kk, 256);
    g->scal = c.take<double>(2, 256);
    g->keys = c.take<int32_t>(kk, 256);
    g->keys_sorted = c.take<int32_t>(kk, 256);
    g->slots_sorted = c.take<int32_t>(kk, 256);
    g->c = c.take<float>(ni, 256);
    g->n = c.take<int32_t>(ni);                                    // right behind c: one memset clears both
    // from here on an array is followed by the padding of its own size to 256, wherever it starts (c + n need not end on 256)
    c.take<char>(align_up(ni * 4, 256) - ni * 4);
    const size_t part = (size_t)gen_blocks(n_items) * ld * 4;
    g->part = c.take<float>(part / 4);
    c.take<char>(align_up(part, 256) - part);
    g->temp = c.take<char>(tb);
    g->temp_bytes = tb;
    return QREC_OK;
}

// one wavefront per sample: its sort key, log p_i r_i and 1/2 |Qb[i]|^2 (weights and bias: the padding is zero)
template <int NK>
__global__ __launch_bounds__(256) void gen_prep_kernel(const float *__restrict__ Q, int n_items, int ld, const int32_t *__restrict__ samples,
                                                       const float *__restrict__ reward, int64_t K, const float *__restrict__ p,
                                                       int32_t *__restrict__ keys, double *__restrict__ term, double *__restrict__ l2) {
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const int lane = threadIdx.x & 63;
    const int i = samples[k];
    const bool ok = (unsigned)i < (unsigned)n_items;
    float q[NK];
    load_row<NK>(Q, ld, i, ok, lane, q);
    double sq = 0.0;
#pragma unroll
    for (int c = 0; c < NK; c++) sq += (double)q[c] * (double)q[c];
    sq = wave_sum_dpp(sq);
    if (lane == 0) {
        keys[k] = ok ? i : -1;
        term[k] = ok ? (double)(logf(p[i]) * reward[k]) : 0.0;
        l2[k] = 0.5 * sq;
    }
}

// c_j = sum of the rewards of item j's samples in sample order, n_j = their number: the head of a sorted run walks it
__global__ __launch_bounds__(256) void gen_walk_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ slots, int64_t K,
                                                       const float *__restrict__ reward, float *__restrict__ c, int32_t *__restrict__ n) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= K) return;
    const int32_t item = keys[p];
    if (item < 0 || (p > 0 && keys[p - 1] == item)) return;
    float acc = 0.0f;
    int cnt = 0;
    for (int64_t q = p; q < K && keys[q] == item; q++) { acc += reward[slots[q]]; cnt++; }
    c[item] = acc; n[item] = cnt;
}

// one workgroup: R = sum_k r_k, the loss  -(1/K) sum log p r + reg (1/2 |P[u]|^2 + sum_k 1/2 |Qb[i_k]|^2)
__global__ __launch_bounds__(256) void gen_sums_kernel(const float *__restrict__ P, int n_users, int d, int ld, int user,
                                                       const float *__restrict__ reward, const int32_t *__restrict__ keys,
                                                       const double *__restrict__ term, const double *__restrict__ l2, int64_t K, float reg,
                                                       double *__restrict__ scal, double *__restrict__ loss) {
    __shared__ double lds[256];
    const int t = threadIdx.x;
    double r = 0.0, a = 0.0, s = 0.0;
    for (int64_t k = t; k < K; k += 256) {
        if (keys[k] < 0) continue;
        r += (double)reward[k]; a += term[k]; s += l2[k];
    }
    r = block_sum_fixed(r, lds); a = block_sum_fixed(a, lds); s = block_sum_fixed(s, lds);
    double pu = 0.0;
    if ((unsigned)user < (unsigned)n_users)
        for (int c = t; c < d; c += 256) { const double v = P[(size_t)user * ld + c]; pu += 0.5 * v * v; }
    pu = block_sum_fixed(pu, lds);
    if (t == 0) {
        scal[0] = r;
        if (loss) *loss = -a / (double)(K > 0 ? K : 1) + (double)reg * (pu + s);
    }
}

// the pass over the item table: g_j = -(c_j - R p_j) / K, G = g_j [P[u] | 1] + reg n_j Qb[j], Adam on the row (the arithmetic of
// qrec_adam_step), and sum_j g_j Qb[j] of the workgroup's items from the rows as they were read
template <int NK>
__global__ __launch_bounds__(256) void gen_item_kernel(const float *__restrict__ P, float *__restrict__ Q, float *__restrict__ mQ,
                                                       float *__restrict__ vQ, int n_users, int n_items, int d, int ld, int user,
                                                       const float *__restrict__ p, const float *__restrict__ c, const int32_t *__restrict__ n,
                                                       const double *__restrict__ scal, float Kf, float reg, int apply, float alpha,
                                                       float b1, float b2, float eps, float *__restrict__ part, float *__restrict__ g_out,
                                                       float *__restrict__ gQ_out) {
#pragma clang fp contract(off)
    __shared__ float acc_lds[4][QREC_IRGAN_MAX_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float R = (float)scal[0], omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    float pu[NK], acc[NK];
    load_user_row<NK>(P, n_users, d, ld, user, lane, pu);
#pragma unroll
    for (int k = 0; k < NK; k++) acc[k] = 0.0f;
    const int j0 = (blockIdx.x * 4 + wave) * kItemsPerWave;
    for (int j = j0; j < j0 + kItemsPerWave && j < n_items; j++) {
        const float g = -(c[j] - R * p[j]) / Kf;
        const float rn = reg * (float)n[j];
        if (lane == 0 && g_out) g_out[j] = g;
#pragma unroll
        for (int k = 0; k < NK; k++) {
            const int col = lane + 64 * k;
            if (col >= ld) continue;
            const size_t at = (size_t)j * ld + col;
            const float q = Q[at];
            acc[k] += g * q;
            const float G = g * pu[k] + rn * q;
            if (gQ_out) gQ_out[at] = G;
            if (apply) {
                float m = mQ[at], v = vQ[at];
                m = m + (G - m) * omb1;
                v = v + (G * G - v) * omb2;
                Q[at] = q - (m * alpha) / (sqrtf(v) + eps);
                mQ[at] = m; vQ[at] = v;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int col = lane + 64 * k;
        if (col < ld) acc_lds[wave][col] = acc[k];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < ld; col += 256)
        part[(size_t)blockIdx.x * ld + col] = ((acc_lds[0][col] + acc_lds[1][col]) + acc_lds[2][col]) + acc_lds[3][col];
}

// gP[u] = (the partial rows in workgroup order) + reg P[u]; columns >= d (the bias column and the padding) stay zero
__global__ __launch_bounds__(256) void gen_user_kernel(const float *__restrict__ P, int n_users, int d, int ld, int user,
                                                       const float *__restrict__ part, int n_blocks, float reg, float *__restrict__ gP) {
#pragma clang fp contract(off)
    const int col = threadIdx.x;
    if (col >= ld || (unsigned)user >= (unsigned)n_users) return;
    float s = 0.0f;
    for (int k = 0; k < n_blocks; k++) s += part[(size_t)k * ld + col];
    const size_t at = (size_t)user * ld + col;
    gP[at] = col < d ? s + reg * P[at] : 0.0f;
}

// ---- discriminator: per-slot gradient rows ----------------------------------------------------------------------------------
template <int NK>
__global__ __launch_bounds__(256) void dis_slots_kernel(const float *__restrict__ P, const float *__restrict__ Q, int n_users, int n_items,
                                                        int d, int ld, const int32_t *__restrict__ us, const int32_t *__restrict__ is,
                                                        const float *__restrict__ label, int B, float breg, float *__restrict__ slotP,
                                                        float *__restrict__ slotQ, int32_t *__restrict__ keyP, int32_t *__restrict__ keyQ,
                                                        float *__restrict__ dz_out, double *__restrict__ terms) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= B) return;
    const int lane = threadIdx.x & 63;
    const int u = us[s], i = is[s];
    const bool ok = (unsigned)u < (unsigned)n_users && (unsigned)i < (unsigned)n_items;
    float pu[NK], q[NK], acc = 0.0f;
    double sq = 0.0;
    load_user_row<NK>(P, n_users, d, ld, ok ? u : -1, lane, pu);
    load_row<NK>(Q, ld, i, ok, lane, q);
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int col = lane + 64 * k;
        acc += pu[k] * q[k];
        sq += (double)q[k] * (double)q[k] + (col < d ? (double)pu[k] * (double)pu[k] : 0.0);
    }
    const float x = wave_sum_dpp(acc);
    sq = wave_sum_dpp(sq);
    const float y = label[s];
    const float dz = ok ? sigmoidf(x) - y : 0.0f;
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int col = lane + 64 * k;
        if (col >= ld) continue;
        slotP[(size_t)s * ld + col] = col < d ? dz * q[k] + breg * pu[k] : 0.0f;
        slotQ[(size_t)s * ld + col] = dz * pu[k] + breg * q[k];
    }
    if (lane == 0) {
        keyP[s] = ok ? u : -1; keyQ[s] = ok ? i : -1;
        if (dz_out) dz_out[s] = dz;
        // sigmoid_cross_entropy_with_logits: max(x, 0) - x y + log1p(exp(-|x|)); the regulariser enters once per slot, B times over
        terms[s] = ok ? (double)(fmaxf(x, 0.0f) - x * y + log1pf(expf(-fabsf(x)))) + (double)breg * 0.5 * sq : 0.0;
    }
}

__global__ __launch_bounds__(256) void sum_terms_kernel(const double *__restrict__ terms, int64_t n, double *__restrict__ out) {
    __shared__ double lds[256];
    double a = 0.0;
    for (int64_t k = threadIdx.x; k < n; k += 256) a += terms[k];
    a = block_sum_fixed(a, lds);
    if (threadIdx.x == 0) *out = a;
}

// rows of get_data for a block of users: per user the positives (label 1), then the drawn negatives (label 0)
__global__ __launch_bounds__(256) void assemble_kernel(const int32_t *__restrict__ users, int n_users, int B, const int64_t *__restrict__ pos_indptr,
                                                       const int32_t *__restrict__ pos_items, const int64_t *__restrict__ draw_ptr,
                                                       const int32_t *__restrict__ samples, const int64_t *__restrict__ row_ptr, int64_t n_rows,
                                                       int32_t *__restrict__ out_u, int32_t *__restrict__ out_i, float *__restrict__ out_label) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int b = row_of(row_ptr, B, r);
    const int u = users[b];
    const bool uok = (unsigned)u < (unsigned)n_users;
    const int64_t pbeg = uok ? pos_indptr[u] : 0, plen = uok ? pos_indptr[u + 1] - pbeg : 0;
    const int64_t local = r - row_ptr[b], n_draw = draw_ptr[b + 1] - draw_ptr[b];
    int item = -1;
    float lab = 0.0f;
    if (local < plen) { item = pos_items[pbeg + local]; lab = 1.0f; }
    else if (local - plen < n_draw) item = samples[draw_ptr[b] + local - plen];
    out_u[r] = uok ? u : -1; out_i[r] = item; out_label[r] = lab;
}

int check_shape(const char *who, int n_users, int n_items, int d, int ld) {
    QREC_REQUIRE(n_users > 0 && n_items > 0 && d > 0 && ld > 0 && ld % 32 == 0, "%s: bad shape", who);
    if (ld > QREC_IRGAN_MAX_LD || d + 1 > ld) {
        set_error("%s: rows of %d floats with the bias in column %d; at most %d floats with d + 1 <= ld are supported", who, ld, d, QREC_IRGAN_MAX_LD);
        return QREC_ERR_UNSUPPORTED;
    }
    QREC_REQUIRE(ld == 32 || ld == 64 || ld == 128 || ld == 256, "%s: row stride must be 32, 64, 128 or 256 floats (got %d)", who, ld);
    return QREC_OK;
}

struct RowWs { double *tile_sum, *row_sum; float *tile_max, *row_max; };      // in the order they lie
inline int n_tiles_of(int n_items) { return (n_items + kTile - 1) / kTile; }
inline int n_chunks_of(int n_items) { return (n_items + kChunk - 1) / kChunk; }
RowWs row_layout(Carver &c, int B, int n_items) {
    const size_t nt = (size_t)n_tiles_of(n_items), nb = (size_t)B;
    const RowWs r = {c.take<double>(nb * nt, 256), c.take<double>(nb, 256), c.take<float>(nb * nt, 256), c.take<float>(nb, 256)};
    c.pad(256);
    return r;
}

#define QREC_NK(ld, CALL)                 \
    switch ((ld) <= 64 ? 1 : (ld) / 64) { \
        case 1: { constexpr int NK = 1; CALL; } break; \
        case 2: { constexpr int NK = 2; CALL; } break; \
        default: { constexpr int NK = 4; CALL; } break; \
    }

}  // namespace

extern "C" {

int qrec_irgan_row_workspace_bytes(int32_t B, int32_t n_items, int64_t *bytes) {
    QREC_REQUIRE(bytes && B > 0 && n_items > 0, "qrec_irgan_row_workspace_bytes: bad argument");
    *bytes = layout_bytes(row_layout, B, n_items);
    return QREC_OK;
}

int qrec_irgan_row_weights(const float *d_P, const float *d_Q, int32_t n_users, int32_t n_items, int32_t d, int32_t ld,
                           const int32_t *d_users, int32_t B, const int64_t *d_pos_indptr, const int32_t *d_pos_items, int32_t mode,
                           float temperature, float sample_lambda, float *d_z, float *d_w, float *d_p, double *d_csum, void *d_ws,
                           void *stream) {
    const int rc = check_shape("qrec_irgan_row_weights", n_users, n_items, d, ld);
    if (rc != QREC_OK) return rc;
    QREC_REQUIRE(d_P && d_Q && d_users && d_pos_indptr && d_pos_items && d_z && d_w && d_csum && d_ws && B > 0 && B <= 65535,
                 "qrec_irgan_row_weights: bad argument");
    QREC_REQUIRE(mode == QREC_IRGAN_NEGATIVES || (mode == QREC_IRGAN_MIXTURE && d_p), "qrec_irgan_row_weights: bad mode");
    QREC_REQUIRE(temperature > 0.0f && sample_lambda >= 0.0f && sample_lambda <= 1.0f, "qrec_irgan_row_weights: bad temperature or mixture");
    hipStream_t st = as_stream(stream);
    const RowWs r = carve(d_ws, row_layout, B, n_items);
    const int nt = n_tiles_of(n_items), nc = n_chunks_of(n_items);
    QREC_NK(ld, hipLaunchKernelGGL((logits_kernel<NK>), dim3(nt, B), dim3(256), 0, st, d_P, d_Q, n_users, n_items, d, ld, d_users, temperature,
                                   d_z, r.tile_max, r.tile_sum));
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(rowstat_kernel, dim3(B), dim3(256), 0, st, r.tile_max, r.tile_sum, nt, r.row_max, r.row_sum);
    QREC_LAUNCH_CHECK();
    const float keep = (float)(1.0 - (double)sample_lambda);
    hipLaunchKernelGGL(weights_kernel, dim3((nc + 3) / 4, B), dim3(256), 0, st, d_z, n_items, n_users, d_users, d_pos_indptr, d_pos_items, mode,
                       keep, sample_lambda, r.row_max, r.row_sum, d_w, d_p, nc, d_csum);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel, dim3(B), dim3(256), 0, st, d_csum, nc);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

static int draw_common(const float *d_w, const double *d_csum, int32_t n_items, int32_t B, const int64_t *d_draw_ptr, int64_t n_draws,
                       const double *d_uniforms, uint64_t seed, uint64_t step, int32_t *d_samples, double *d_uniforms_out, void *stream) {
    if (n_draws == 0) return QREC_OK;
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)((n_draws + 255) / 256)), dim3(256), 0, as_stream(stream), d_w, d_csum, n_items,
                       n_chunks_of(n_items), B, d_draw_ptr, n_draws, d_uniforms, seed, step, d_samples, d_uniforms_out);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_irgan_draw(const float *d_w, const double *d_csum, int32_t n_items, int32_t B, const int64_t *d_draw_ptr, int64_t n_draws,
                    const double *d_uniforms, uint64_t seed, uint64_t step, int32_t *d_samples, void *stream) {
    QREC_REQUIRE(d_w && d_csum && d_draw_ptr && d_samples && n_items > 0 && B > 0 && n_draws >= 0 && n_draws < ((int64_t)1 << 31),
                 "qrec_irgan_draw: bad argument");
    return draw_common(d_w, d_csum, n_items, B, d_draw_ptr, n_draws, d_uniforms, seed, step, d_samples, nullptr, stream);
}

int qrec_irgan_uniforms(int32_t B, const int64_t *d_draw_ptr, int64_t n_draws, uint64_t seed, uint64_t step, double *d_out, void *stream) {
    QREC_REQUIRE(d_draw_ptr && d_out && B > 0 && n_draws >= 0 && n_draws < ((int64_t)1 << 31), "qrec_irgan_uniforms: bad argument");
    return draw_common(nullptr, nullptr, 1, B, d_draw_ptr, n_draws, nullptr, seed, step, nullptr, d_out, stream);
}

int qrec_irgan_reward(const float *d_P, const float *d_Q, int32_t n_users, int32_t n_items, int32_t d, int32_t ld, const int32_t *d_users,
                      int32_t B, const int64_t *d_draw_ptr, int64_t n_draws, const int32_t *d_samples, const float *d_p, const float *d_w,
                      float *d_reward, void *stream) {
    const int rc = check_shape("qrec_irgan_reward", n_users, n_items, d, ld);
    if (rc != QREC_OK) return rc;
    QREC_REQUIRE(d_P && d_Q && d_users && d_draw_ptr && d_samples && d_p && d_w && d_reward && B > 0 && n_draws >= 0 &&
                 n_draws < ((int64_t)1 << 31), "qrec_irgan_reward: bad argument");
    if (n_draws == 0) return QREC_OK;
    QREC_NK(ld, hipLaunchKernelGGL((reward_kernel<NK>), dim3((unsigned)((n_draws + 3) / 4)), dim3(256), 0, as_stream(stream), d_P, d_Q, n_users,
                                   n_items, d, ld, d_users, B, d_draw_ptr, n_draws, d_samples, d_p, d_w, d_reward));
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_irgan_gen_workspace_bytes(int32_t n_items, int32_t ld, int64_t K, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_items > 0 && ld > 0 && K >= 0 && K < ((int64_t)1 << 31), "qrec_irgan_gen_workspace_bytes: bad argument");
    GenWs g;
    Carver c(nullptr);
    const int rc = gen_layout(c, n_items, ld, K, &g);
    *bytes = (int64_t)c.bytes();
    return rc;
}

int qrec_irgan_gen_step(const float *d_P, float *d_Q, float *d_mQ, float *d_vQ, int32_t n_users, int32_t n_items, int32_t d, int32_t ld,
                        int32_t user, const int32_t *d_samples, const float *d_reward, int64_t K, const float *d_p, float reg, int32_t apply,
                        float alpha, float beta1, float beta2, float eps, float *d_gP, float *d_g, float *d_gQ, double *d_loss, void *d_ws,
                        int64_t ws_bytes, void *stream) {
    const int rc = check_shape("qrec_irgan_gen_step", n_users, n_items, d, ld);
    if (rc != QREC_OK) return rc;
    QREC_REQUIRE(d_P && d_Q && d_samples && d_reward && d_p && d_gP && d_ws && K > 0 && K < ((int64_t)1 << 31) && (!apply || (d_mQ && d_vQ)),
                 "qrec_irgan_gen_step: bad argument");
    QREC_REQUIRE(user >= 0 && user < n_users, "qrec_irgan_gen_step: user %d outside the table", user);
    GenWs g;
    Carver c(d_ws);
    const int rc2 = gen_layout(c, n_items, ld, K, &g);
    if (rc2 != QREC_OK) return rc2;
    const int64_t need = (int64_t)c.bytes();
    QREC_REQUIRE(ws_bytes >= need, "qrec_irgan_gen_step: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    hipStream_t st = as_stream(stream);
    QREC_NK(ld, hipLaunchKernelGGL((gen_prep_kernel<NK>), dim3((unsigned)((K + 3) / 4)), dim3(256), 0, st, d_Q, n_items, ld, d_samples, d_reward, K,
                                   d_p, g.keys, g.term, g.l2));
    QREC_LAUNCH_CHECK();
    QREC_HIP_CHECK(hipMemsetAsync(g.c, 0, (size_t)n_items * 8, st));          // c and n
    size_t tb = g.temp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs(g.temp, tb, (const int32_t *)g.keys, g.keys_sorted, rocprim::counting_iterator<int32_t>(0),
                                                   g.slots_sorted, (size_t)K, 0u, 32u, st);
    QREC_REQUIRE(e == hipSuccess, "qrec_irgan_gen_step: rocprim::radix_sort_pairs failed");
    hipLaunchKernelGGL(gen_walk_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, g.keys_sorted, g.slots_sorted, K, d_reward, g.c, g.n);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(gen_sums_kernel, dim3(1), dim3(256), 0, st, d_P, n_users, d, ld, user, d_reward, g.keys, g.term, g.l2, K, reg, g.scal, d_loss);
    QREC_LAUNCH_CHECK();
    const int nb = gen_blocks(n_items);
    QREC_NK(ld, hipLaunchKernelGGL((gen_item_kernel<NK>), dim3(nb), dim3(256), 0, st, d_P, d_Q, d_mQ, d_vQ, n_users, n_items, d, ld, user, d_p, g.c,
                                   g.n, g.scal, (float)K, reg, apply, alpha, beta1, beta2, eps, g.part, d_g, d_gQ));
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(gen_user_kernel, dim3(1), dim3(256), 0, st, d_P, n_users, d, ld, user, g.part, nb, reg, d_gP);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_irgan_dis_slots(const float *d_P, const float *d_Q, int32_t n_users, int32_t n_items, int32_t d, int32_t ld, const int32_t *d_u,
                         const int32_t *d_i, const float *d_label, int32_t B, float reg, float *d_slotP, float *d_slotQ, int32_t *d_keyP,
                         int32_t *d_keyQ, float *d_dz, double *d_terms, double *d_loss, void *stream) {
    const int rc = check_shape("qrec_irgan_dis_slots", n_users, n_items, d, ld);
    if (rc != QREC_OK) return rc;
    QREC_REQUIRE(d_P && d_Q && d_u && d_i && d_label && d_slotP && d_slotQ && d_keyP && d_keyQ && d_terms && d_loss && B > 0,
                 "qrec_irgan_dis_slots: bad argument");
    hipStream_t st = as_stream(stream);
    const float breg = (float)B * reg;
    QREC_NK(ld, hipLaunchKernelGGL((dis_slots_kernel<NK>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, d_P, d_Q, n_users, n_items, d, ld, d_u,
                                   d_i, d_label, B, breg, d_slotP, d_slotQ, d_keyP, d_keyQ, d_dz, d_terms));
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_terms_kernel, dim3(1), dim3(256), 0, st, d_terms, (int64_t)B, d_loss);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_irgan_assemble_rows(const int32_t *d_users, int32_t n_users, int32_t B, const int64_t *d_pos_indptr, const int32_t *d_pos_items,
                             const int64_t *d_draw_ptr, const int32_t *d_samples, const int64_t *d_row_ptr, int64_t n_rows, int32_t *d_out_u,
                             int32_t *d_out_i, float *d_out_label, void *stream) {
    QREC_REQUIRE(d_users && d_pos_indptr && d_pos_items && d_draw_ptr && d_samples && d_row_ptr && d_out_u && d_out_i && d_out_label && B > 0 &&
                 n_users > 0 && n_rows >= 0, "qrec_irgan_assemble_rows: bad argument");
    if (n_rows == 0) return QREC_OK;
    hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, as_stream(stream), d_users, n_users, B, d_pos_indptr,
                       d_pos_items, d_draw_ptr, d_samples, d_row_ptr, n_rows, d_out_u, d_out_i, d_out_label);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // extern "C"
