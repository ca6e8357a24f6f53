// APR (model/ranking/APR.py): the per-batch adversarial perturbation and the training step on two objectives, fp32.
//
// Tables are the joint [U; V] pack (item row = n_users + item, row stride ld in {32, 64, 128} floats, pad lanes zero); the
// perturbations D are a second buffer of the same layout, dense as the reference has it, and never swept: a call touches the
// batch's rows and the previous batch's rows, nothing proportional to a table's height.
//
//   x  = p_u . (q_i - q_j)                                 the clean score difference
//   x' = (p_u + D_u) . ((q_i + D_i) - (q_j + D_j))         the perturbed one
//   g  = -sigma(-x),  c' = -regAdv sigma(-x')              d softplus(-x) / dx and regAdv d softplus(-x') / dx'
//
// qrec_apr_perturb (APR.py:43-53): Gamma = d(regAdv sum softplus(-x')) / dD summed per table row, D[row] = eps * l2_normalize(Gamma[row])
// at the batch's rows and 0 everywhere else.  The whole row is needed before it can be scaled, so the pass always takes the
// sorted route of ordered.hip, float atomics in neither mode:
//   1. apr_produce_kernel   a lane group per triplet writes slots k, B + k, 2B + k: c' ((q_v+D_v) - (q_n+D_n)) for row u,
//                           c' (p_u+D_u) for row nu + v, -c' (p_u+D_u) for row nu + n (one class per lookup op: u, v, n)
//   2. apr_clear_kernel     the rows the PREVIOUS call wrote (its run heads, kept in d_touched) become zero
//   3. one stable radix sort of (row, slot)
//   4. apr_walk_kernel      the lane group at the head of a run adds it in slot order, class by class, reduces the row's sum of
//                           squares over the d live lanes and writes eps * Gamma * rsqrt(max(|Gamma|^2, 1e-12)): no Gamma table.
// The producer reads the old D of rows the walker overwrites; they are separate launches on one stream, the producer has
// retired before the clear and the walk start, so the new rows go straight into D.
// With v == n elementwise every slot of row u is c' * 0, and every item row is (sum of its v slots) + (the exact negation of the
// same sum): Gamma is +-0 everywhere and D exactly +0 -- what the reference file's own feed does (APR.py:116-117).
//
// qrec_apr_batch_loss_grad (APR.py:56-64): loss = sum softplus(-x) + reg (l2_loss(p_u) + l2_loss(q_i)) + regAdv sum softplus(-x'),
//   dP[u] += g (q_i-q_j) + reg p_u + c' ((q_i+D_i)-(q_j+D_j));  dQ[i] += g p_u + reg q_i + c' (p_u+D_u);  dQ[j] += -g p_u - c' (p_u+D_u)
// the negative row is not regularised.  A null D or regAdv = 0 is the pretraining step.  Parity mode: the slot rows go through
// ordered_scatter_run with class size B (lookups u, i, j) and the blocks' loss sums are folded in a fixed tree; throughput
// mode: 64-byte-segment float atomics as in bpr_batch_kernel (graph.hip) and one fp64 atomic per block.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.h"

using namespace qrec;

namespace {

constexpr int kMaxLossBlocks = 256;

// log(1 + e^z) without overflow: max(z, 0) + log1p(e^-|z|)
__device__ inline float softplusf(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }
// sigma(-x) = 1 / (1 + e^x): e^x = inf gives 0, e^x = 0 gives 1
__device__ inline float sigmoid_neg(float x) { return 1.0f / (1.0f + expf(x)); }

// Lane r of an LPR-lane group holds columns r, r + LPR, ... (E of them): a group's loads, stores and atomics each cover
// one contiguous 4 * LPR-byte segment.
template <int LPR, int E>
struct Triplet {
    float p[E], qi[E], qj[E];     // the clean rows
    float pa[E], da[E];           // p_u + D_u and (q_i + D_i) - (q_j + D_j)
    float x, xa, sq;              // scores; |p_u|^2 + |q_i|^2
};

template <int LPR, int E, bool ADV>
__device__ inline void load_triplet(const float *__restrict__ S, const float *__restrict__ D, int ru, int ri, int rj, int r,
                                    Triplet<LPR, E> &t) {
#pragma clang fp contract(off)
    constexpr int LD = LPR * E;
    float x = 0.f, xa = 0.f, sq = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int col = r + LPR * e;
        t.p[e] = S[(int64_t)ru * LD + col]; t.qi[e] = S[(int64_t)ri * LD + col]; t.qj[e] = S[(int64_t)rj * LD + col];
        x += t.p[e] * (t.qi[e] - t.qj[e]);
        sq += t.p[e] * t.p[e] + t.qi[e] * t.qi[e];
        if constexpr (ADV) {
            t.pa[e] = t.p[e] + D[(int64_t)ru * LD + col];
            const float via = t.qi[e] + D[(int64_t)ri * LD + col], vja = t.qj[e] + D[(int64_t)rj * LD + col];
            t.da[e] = via - vja;                 // v == n: the same two sums, exactly 0
            xa += t.pa[e] * t.da[e];
        } else {
            t.pa[e] = t.p[e]; t.da[e] = 0.f;
        }
    }
    t.x = row_allreduce_sum<LPR>(x); t.sq = row_allreduce_sum<LPR>(sq);
    t.xa = ADV ? row_allreduce_sum<LPR>(xa) : 0.f;
}

// ---- the perturbation pass ---------------------------------------------------------------------------------------------------
template <int LPR, int E>
__global__ __launch_bounds__(256) void apr_produce_kernel(const float *__restrict__ S, const float *__restrict__ D, int n_users, int64_t n_rows,
                                                          const int32_t *__restrict__ u_idx, const int32_t *__restrict__ v_idx,
                                                          const int32_t *__restrict__ n_idx, int B, float reg_adv,
                                                          float *__restrict__ contrib, int32_t *__restrict__ keys) {
#pragma clang fp contract(off)
    constexpr int GPW = kWave / LPR, LD = LPR * E;
    const int lane = threadIdx.x & 63, g = lane / LPR, r = lane % LPR;
    for (int64_t b = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GPW + g; b < B; b += (int64_t)gridDim.x * 4 * GPW) {
        const int u = u_idx[b], v = v_idx[b], n = n_idx[b];
        const int64_t n_items = n_rows - n_users;
        float *cu = contrib + b * LD, *cv = contrib + ((int64_t)B + b) * LD, *cn = contrib + (2 * (int64_t)B + b) * LD;
        if (u < 0 || u >= n_users || v < 0 || v >= n_items || n < 0 || n >= n_items) {      // no row: the slots are skipped by the walk
            if (r == 0) { keys[b] = -1; keys[(int64_t)B + b] = -1; keys[2 * (int64_t)B + b] = -1; }
            continue;
        }
        const int ru = u, rv = n_users + v, rn = n_users + n;
        Triplet<LPR, E> t;
        load_triplet<LPR, E, true>(S, D, ru, rv, rn, r, t);
        const float c = -reg_adv * sigmoid_neg(t.xa);
        if (r == 0) { keys[b] = ru; keys[(int64_t)B + b] = rv; keys[2 * (int64_t)B + b] = rn; }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const int col = r + LPR * e;
            const float w = c * t.pa[e];
            cu[col] = c * t.da[e]; cv[col] = w; cn[col] = -w;
        }
    }
}

// d_touched = [count, row of sorted position 0, 1, ...]: a run's head holds its row, every other position -1
template <int LPR>
__global__ __launch_bounds__(256) void apr_clear_kernel(const int32_t *__restrict__ touched, int capacity, float *__restrict__ D, int64_t n_rows) {
    constexpr int GPW = kWave / LPR, LD = 4 * LPR;
    const int lane = threadIdx.x & 63, g = lane / LPR, r = lane % LPR;
    int n = touched[0];
    if (n > capacity) n = capacity;
    for (int64_t p = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GPW + g; p < n; p += (int64_t)gridDim.x * 4 * GPW) {
        const int32_t row = touched[1 + p];
        if (row < 0 || row >= n_rows) continue;
        *reinterpret_cast<f32x4 *>(D + (int64_t)row * LD + 4 * r) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int LPR>
__global__ __launch_bounds__(256) void apr_walk_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ slots, int64_t n,
                                                       int64_t class_size, const float *__restrict__ contrib, float *__restrict__ D,
                                                       int64_t n_rows, int d, float eps, int32_t *__restrict__ touched) {
#pragma clang fp contract(off)
    constexpr int GPW = kWave / LPR, LD = 4 * LPR;
    const int lane = threadIdx.x & 63, g = lane / LPR, r = lane % LPR;
    if (blockIdx.x == 0 && threadIdx.x == 0) touched[0] = (int32_t)n;
    for (int64_t p = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GPW + g; p < n; p += (int64_t)gridDim.x * 4 * GPW) {
        const int32_t row = keys[p];
        const bool head = row >= 0 && row < n_rows && (p == 0 || keys[p - 1] != row);
        if (r == 0) touched[1 + p] = head ? row : -1;
        if (!head) continue;
        f32x4 total = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
        int64_t cls = slots[p] / class_size;
        bool first = true;
        for (int64_t q = p; q < n && keys[q] == row; q++) {
            const int64_t s = slots[q];
            const int64_t c = s / class_size;
            if (c != cls) { total = first ? acc : total + acc; first = false; acc = f32x4{0.f, 0.f, 0.f, 0.f}; cls = c; }
            acc = acc + *reinterpret_cast<const f32x4 *>(contrib + s * LD + 4 * r);
        }
        total = first ? acc : total + acc;
        // the pad lanes carry zeros already (c' * 0); masked all the same, so that the norm is over the d live lanes by construction
        if (4 * r + 0 >= d) total.x = 0.f;
        if (4 * r + 1 >= d) total.y = 0.f;
        if (4 * r + 2 >= d) total.z = 0.f;
        if (4 * r + 3 >= d) total.w = 0.f;
        float ss = total.x * total.x + total.y * total.y + total.z * total.z + total.w * total.w;
        ss = row_allreduce_sum<LPR>(ss);
        const float iv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
        // tf.nn.l2_normalize(Gamma, 1) * eps; + 0 turns a row of -0 into +0
        *reinterpret_cast<f32x4 *>(D + (int64_t)row * LD + 4 * r) = (total * iv) * eps + f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// ---- the training step -------------------------------------------------------------------------------------------------------
template <int LPR, int E, bool ADV, bool ORDERED>
__global__ __launch_bounds__(256) void apr_step_kernel(const float *__restrict__ S, const float *__restrict__ D, int n_users, int64_t n_rows,
                                                       const int32_t *__restrict__ u_idx, const int32_t *__restrict__ i_idx,
                                                       const int32_t *__restrict__ j_idx, int B, float reg, float reg_adv,
                                                       float *__restrict__ dE, uint32_t de_bytes, double *__restrict__ loss_out,
                                                       double *__restrict__ partials, float *__restrict__ contrib, int32_t *__restrict__ keys) {
#pragma clang fp contract(off)
    constexpr int GPW = kWave / LPR, LD = LPR * E;
    const int lane = threadIdx.x & 63, g = lane / LPR, r = lane % LPR;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(dE, de_bytes);
    double l_rec = 0.0, l_reg = 0.0, l_adv = 0.0;
    for (int64_t b = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GPW + g; b < B; b += (int64_t)gridDim.x * 4 * GPW) {
        const int ru = u_idx[b], ri = n_users + i_idx[b], rj = n_users + j_idx[b];
        if (ru < 0 || ru >= n_users || ri < n_users || ri >= n_rows || rj < n_users || rj >= n_rows) {      // an index outside its table: no rows
            if constexpr (ORDERED) { if (r == 0) { keys[b] = -1; keys[(int64_t)B + b] = -1; keys[2 * (int64_t)B + b] = -1; } }
            continue;
        }
        Triplet<LPR, E> t;
        load_triplet<LPR, E, ADV>(S, D, ru, ri, rj, r, t);
        const float gs = -sigmoid_neg(t.x);
        const float c = ADV ? -reg_adv * sigmoid_neg(t.xa) : 0.f;
        if (r == 0) {
            l_rec += (double)softplusf(-t.x);
            l_reg += 0.5 * (double)reg * (double)t.sq;
            if (ADV) l_adv += (double)reg_adv * (double)softplusf(-t.xa);
        }
        if constexpr (ORDERED) {
            if (r == 0) { keys[b] = ru; keys[(int64_t)B + b] = ri; keys[2 * (int64_t)B + b] = rj; }
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const int col = r + LPR * e;
            float du = gs * (t.qi[e] - t.qj[e]) + reg * t.p[e];
            float di = gs * t.p[e] + reg * t.qi[e];
            float dj = -(gs * t.p[e]);
            if (ADV) { const float w = c * t.pa[e]; du += c * t.da[e]; di += w; dj -= w; }
            if constexpr (ORDERED) {
                contrib[b * LD + col] = du; contrib[((int64_t)B + b) * LD + col] = di; contrib[(2 * (int64_t)B + b) * LD + col] = dj;
            } else {
                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(du, rs, (int)((uint32_t)ru * LD * 4u + (uint32_t)col * 4u), 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(di, rs, (int)((uint32_t)ri * LD * 4u + (uint32_t)col * 4u), 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(dj, rs, (int)((uint32_t)rj * LD * 4u + (uint32_t)col * 4u), 0, 0);
            }
        }
    }
    // the block's three sums in a fixed tree; parity mode keeps them per block for apr_fold_kernel, throughput mode adds them
    // with one fp64 atomic each
    __shared__ double s_loss[4][3];
    l_rec = wave_sum_dpp(l_rec); l_reg = wave_sum_dpp(l_reg); l_adv = wave_sum_dpp(l_adv);
    if (lane == 0) { s_loss[threadIdx.x >> 6][0] = l_rec; s_loss[threadIdx.x >> 6][1] = l_reg; s_loss[threadIdx.x >> 6][2] = l_adv; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const double tot = (s_loss[0][k] + s_loss[1][k]) + (s_loss[2][k] + s_loss[3][k]);
        if constexpr (ORDERED) partials[(int64_t)blockIdx.x * 3 + k] = tot;
        else if (tot != 0.0) atomicAdd(loss_out + k, tot);
    }
}

// loss_out[k] += the blocks' partial sums of term k, added in one fixed order (one wavefront)
__global__ __launch_bounds__(64) void apr_fold_kernel(const double *__restrict__ partials, int n_blocks, double *__restrict__ loss_out) {
    const int lane = threadIdx.x;
    for (int k = 0; k < 3; k++) {
        double v = 0.0;
        for (int b = lane; b < n_blocks; b += kWave) v += partials[(int64_t)b * 3 + k];
        v = wave_sum_dpp(v);
        if (lane == 0) loss_out[k] += v;
    }
}

struct AprStepWs { void *ordered; int64_t ordered_bytes; double *partials; };

int apr_step_layout(Carver &c, int64_t B, int ld, AprStepWs *w) {
    const int rc = ordered_ws_bytes(3 * B, ld, &w->ordered_bytes);
    if (rc != QREC_OK) return rc;
    w->ordered = c.take<char>((size_t)w->ordered_bytes, 256);
    w->partials = c.take<double>((size_t)3 * kMaxLossBlocks, 256);
    c.pad(256);
    return QREC_OK;
}

bool apr_ld_ok(int ld) { return ld == 32 || ld == 64 || ld == 128; }

}  // namespace

extern "C" {

int qrec_apr_perturb_workspace_bytes(int32_t B, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && B >= 0, "qrec_apr_perturb_workspace_bytes: bad argument");
    QREC_REQUIRE(apr_ld_ok(ld), "qrec_apr_perturb_workspace_bytes: row stride must be 32, 64 or 128 floats (got %d)", ld);
    return ordered_ws_bytes(3 * (int64_t)(B > 0 ? B : 1), ld, bytes);
}

int qrec_apr_perturb(const float *d_E, float *d_D, int32_t n_users, int64_t n_rows, int32_t d, int32_t ld, const int32_t *d_u,
                     const int32_t *d_v, const int32_t *d_n, int32_t B, float reg_adv, float eps, int32_t *d_touched,
                     int32_t touched_capacity, void *d_workspace, int64_t workspace_bytes, float *h_stage_ms, void *stream) {
    QREC_REQUIRE(d_E && d_D, "qrec_apr_perturb: null table");
    QREC_REQUIRE(B >= 0, "qrec_apr_perturb: negative batch size (%d)", B);
    QREC_REQUIRE(apr_ld_ok(ld), "qrec_apr_perturb: row stride must be 32, 64 or 128 floats (got %d)", ld);
    QREC_REQUIRE(d > 0 && d <= ld, "qrec_apr_perturb: %d columns in a row stride of %d floats", d, ld);
    QREC_REQUIRE(n_users >= 0 && n_rows >= n_users && n_rows * (int64_t)ld * 4 < ((int64_t)1 << 32), "qrec_apr_perturb: bad table size");
    QREC_REQUIRE(d_touched && touched_capacity >= 0 && (int64_t)touched_capacity >= 3 * (int64_t)B,
                 "qrec_apr_perturb: the touched-row list holds %d rows, %lld needed (3 B)", touched_capacity, 3 * (long long)B);
    QREC_REQUIRE(B == 0 || (d_u && d_v && d_n), "qrec_apr_perturb: null index array");
    hipStream_t st = as_stream(stream);
    const int64_t n = 3 * (int64_t)B;
    OrderedScatterWs w = {};
    if (B > 0) {
        QREC_REQUIRE(d_workspace && workspace_bytes >= 0, "qrec_apr_perturb: null workspace");
        const int rc = ordered_ws_carve(d_workspace, workspace_bytes, n, ld, &w);
        if (rc != QREC_OK) return rc;
    }
    // h_stage_ms: events around the four stages (a measurement aid; the training path passes null and records nothing)
    hipEvent_t ev[5] = {};
    if (h_stage_ms)
        for (auto &x : ev) QREC_HIP_CHECK(hipEventCreate(&x));
#define QREC_MARK(k) if (h_stage_ms) QREC_HIP_CHECK(hipEventRecord(ev[k], st))
    QREC_MARK(0);
    int64_t blocks;
#define QREC_AP(LPR, E)                                                                                                      \
    if (B > 0) {                                                                                                             \
        blocks = (B + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)); if (blocks > 1024) blocks = 1024;                              \
        hipLaunchKernelGGL((apr_produce_kernel<LPR, E>), dim3((unsigned)blocks), dim3(256), 0, st, d_E, d_D, n_users, n_rows, d_u, d_v, \
                           d_n, B, reg_adv, w.contrib, w.keys);                                                              \
    }                                                                                                                        \
    QREC_MARK(1);                                                                                                            \
    if (touched_capacity > 0) {                                                                                              \
        blocks = ((int64_t)touched_capacity + 4 * (64 / (LPR * E / 4)) - 1) / (4 * (64 / (LPR * E / 4))); if (blocks > 1024) blocks = 1024; \
        hipLaunchKernelGGL((apr_clear_kernel<LPR * E / 4>), dim3((unsigned)blocks), dim3(256), 0, st, d_touched, touched_capacity, d_D, n_rows); \
    }
    switch (ld) {
        case 32: QREC_AP(16, 2); break;
        case 64: QREC_AP(16, 4); break;
        default: QREC_AP(32, 4); break;
    }
#undef QREC_AP
    QREC_LAUNCH_CHECK();
    QREC_MARK(2);
    if (B == 0) QREC_HIP_CHECK(hipMemsetAsync(d_touched, 0, sizeof(int32_t), st));
    if (B > 0) {
        size_t tb = w.temp_bytes;
        const hipError_t e = rocprim::radix_sort_pairs(w.temp, tb, (const int32_t *)w.keys, w.keys_sorted, rocprim::counting_iterator<int32_t>(0),
                                                       w.slots_sorted, (size_t)n, 0u, 32u, st);
        QREC_REQUIRE(e == hipSuccess, "qrec_apr_perturb: rocprim::radix_sort_pairs failed");
        QREC_MARK(3);
#define QREC_AW(LPR)                                                                                                         \
        blocks = (n + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)); if (blocks > 2048) blocks = 2048;                                  \
        hipLaunchKernelGGL((apr_walk_kernel<LPR>), dim3((unsigned)blocks), dim3(256), 0, st, w.keys_sorted, w.slots_sorted, n, (int64_t)B, \
                           w.contrib, d_D, n_rows, d, eps, d_touched)
        switch (ld) {
            case 32: QREC_AW(8); break;
            case 64: QREC_AW(16); break;
            default: QREC_AW(32); break;
        }
#undef QREC_AW
        QREC_LAUNCH_CHECK();
    }
    if (h_stage_ms) {
        if (B == 0) QREC_MARK(3);
        QREC_MARK(4);
        QREC_HIP_CHECK(hipEventSynchronize(ev[4]));
        for (int k = 0; k < 4; k++) QREC_HIP_CHECK(hipEventElapsedTime(h_stage_ms + k, ev[k], ev[k + 1]));
        for (auto &x : ev) QREC_HIP_CHECK(hipEventDestroy(x));
    }
#undef QREC_MARK
    return QREC_OK;
}

int qrec_apr_step_workspace_bytes(int32_t B, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && B >= 0, "qrec_apr_step_workspace_bytes: bad argument");
    QREC_REQUIRE(apr_ld_ok(ld), "qrec_apr_step_workspace_bytes: row stride must be 32, 64 or 128 floats (got %d)", ld);
    AprStepWs w;
    Carver c(nullptr);
    const int rc = apr_step_layout(c, B > 0 ? B : 1, ld, &w);
    *bytes = (int64_t)c.bytes();
    return rc;
}

int qrec_apr_batch_loss_grad(const float *d_E, const float *d_D, int32_t n_users, int64_t n_rows, int32_t d, int32_t ld,
                             const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int32_t B, float reg, float reg_adv,
                             float *d_dE, double *d_loss, void *d_workspace, int64_t workspace_bytes, void *stream) {
    QREC_REQUIRE(d_E && d_dE && d_loss, "qrec_apr_batch_loss_grad: null table, gradient or loss");
    QREC_REQUIRE(B >= 0, "qrec_apr_batch_loss_grad: negative batch size (%d)", B);
    QREC_REQUIRE(apr_ld_ok(ld), "qrec_apr_batch_loss_grad: row stride must be 32, 64 or 128 floats (got %d)", ld);
    QREC_REQUIRE(d > 0 && d <= ld, "qrec_apr_batch_loss_grad: %d columns in a row stride of %d floats", d, ld);
    QREC_REQUIRE(n_users >= 0 && n_rows >= n_users && n_rows * (int64_t)ld * 4 < ((int64_t)1 << 32), "qrec_apr_batch_loss_grad: bad table size");
    QREC_REQUIRE(B == 0 || (d_u && d_i && d_j), "qrec_apr_batch_loss_grad: null index array");
    if (B == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    const uint32_t bytes = (uint32_t)(n_rows * ld * 4);
    const bool adv = d_D != nullptr && reg_adv != 0.f;
    AprStepWs sw = {};
    OrderedScatterWs ow = {};
    if (d_workspace) {
        Carver c(d_workspace);
        int rc = apr_step_layout(c, B, ld, &sw);
        if (rc != QREC_OK) return rc;
        QREC_REQUIRE(workspace_bytes >= (int64_t)c.bytes(), "qrec_apr_batch_loss_grad: workspace of %lld bytes, %lld needed (qrec_apr_step_workspace_bytes)",
                     (long long)workspace_bytes, (long long)c.bytes());
        rc = ordered_ws_carve(sw.ordered, sw.ordered_bytes, 3 * (int64_t)B, ld, &ow);
        if (rc != QREC_OK) return rc;
    }
    int64_t blocks;
#define QREC_AS2(LPR, E, ADV, ORD)                                                                                           \
    hipLaunchKernelGGL((apr_step_kernel<LPR, E, ADV, ORD>), dim3((unsigned)blocks), dim3(256), 0, st, d_E, d_D, n_users, n_rows, d_u, d_i, d_j, B, \
                       reg, reg_adv, d_dE, bytes, d_loss, sw.partials, ow.contrib, ow.keys)
#define QREC_AS(LPR, E)                                                                                                      \
    blocks = (B + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)); if (blocks > kMaxLossBlocks) blocks = kMaxLossBlocks;              \
    if (adv) { if (d_workspace) QREC_AS2(LPR, E, true, true); else QREC_AS2(LPR, E, true, false); }                          \
    else { if (d_workspace) QREC_AS2(LPR, E, false, true); else QREC_AS2(LPR, E, false, false); }
    switch (ld) {
        case 32: QREC_AS(16, 2); break;
        case 64: QREC_AS(16, 4); break;
        default: QREC_AS(32, 4); break;
    }
#undef QREC_AS
#undef QREC_AS2
    QREC_LAUNCH_CHECK();
    if (!d_workspace) return QREC_OK;
    hipLaunchKernelGGL(apr_fold_kernel, dim3(1), dim3(64), 0, st, sw.partials, (int)blocks, d_loss);
    QREC_LAUNCH_CHECK();
    return ordered_scatter_run(ow, 3 * (int64_t)B, ld, B, d_dE, st);     // one class per lookup (u, i, j)
}

}  // extern "C"
