// The dense layer between two sparse products of the diffusion / hypergraph models and its backward pass.
//
//   DiffNet (model/ranking/DiffNet.py:46-49):  u' = relu([S u | u] W_k),  W_k (2d x d)
//   DHCF    (model/ranking/DHCF.py:74-87):     pre = (H E_0) W_k + z_{k-1}; z_k = l2_normalize(dropout(leaky_relu(pre)))
//
//   forward   Y = [X1 | X2] W (+ R), optionally through ReLU                       layer_fwd_*<ConcatOps>     (f32 MFMA)
//   backward  dPre = dY * (Y > 0)                                                  dpre_relu_kernel
//             dPre = normalize_bwd(dWide block + dZ_next) * gate                   dpre_norm_kernel
//             dX1 (=|+=) dPre W[0]^T, dX2 = dPre W[1]^T   (dR is dPre itself)      layer_bwd_*<ConcatOps>     (f32 MFMA)
//             gW = [X1 | X2]^T dPre                                                layer_wgrad_*<ConcatOps> + wgrad_sum_kernel
//
// Tables are [rows][ld] fp32 with ld in {32, 64, 128}.  W is stored zero-padded as NW blocks of [ld][ld] (NW = 2 with X2:
// block 0 multiplies X1, block 1 multiplies X2).  The MFMA kernels are the shared row-tiled layer kernels of mfma_layer.h,
// instantiated with the concatenation policy ConcatOps<NW>; this file keeps the entry points and the pointwise kernels.
#include "mfma_layer.h"

using namespace qrec;

namespace {

// ---- dPre ------------------------------------------------------------------------------------------------------------------
// ReluGrad: dY where Y > 0, else 0
__global__ __launch_bounds__(256) void dpre_relu_kernel(const float *__restrict__ dY, const float *__restrict__ Y, int64_t n4,
                                                        float *__restrict__ dpre) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n4; k += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 g = reinterpret_cast<const f32x4 *>(dY)[k], y = reinterpret_cast<const f32x4 *>(Y)[k];
        const f32x4 o = {y.x > 0.f ? g.x : 0.f, y.y > 0.f ? g.y : 0.f, y.z > 0.f ? g.z : 0.f, y.w > 0.f ? g.w : 0.f};
        reinterpret_cast<f32x4 *>(dpre)[k] = o;
    }
}

// dz = dWide block (+ dZ_next: the next layer reads this layer's NORMALISED rows as its residual, DHCF.py:78-90);
// dpre = (dz - z (z.dz)) * inv * gate      (z: the wide table's block; gate, inv: what qrec_ngcf_activate left)
template <int LPR>
__global__ __launch_bounds__(256) void dpre_norm_kernel(const float *__restrict__ dAll, const float *__restrict__ All, int wide_ld,
                                                        int col_off, const float *__restrict__ dZ_next,
                                                        const float *__restrict__ inv_norm, const float *__restrict__ gate,
                                                        int64_t n_rows, int d, float *__restrict__ dpre) {
    constexpr int GPW = kWave / LPR;
    const int lane = threadIdx.x & 63, g = lane / LPR, r = lane % LPR;
    const int64_t gid = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GPW + g;
    const int64_t n_groups = (int64_t)gridDim.x * 4 * GPW;
    for (int64_t row = gid; row < n_rows; row += n_groups) {
        const int64_t off = row * (4 * LPR) + 4 * r;
        const float *dzp = dAll + row * wide_ld + col_off + 4 * r, *zp = All + row * wide_ld + col_off + 4 * r;
        f32x4 dz = {0.f, 0.f, 0.f, 0.f}, z = dz;
        if (4 * r + 0 < d) { dz.x = dzp[0]; z.x = zp[0]; }
        if (4 * r + 1 < d) { dz.y = dzp[1]; z.y = zp[1]; }
        if (4 * r + 2 < d) { dz.z = dzp[2]; z.z = zp[2]; }
        if (4 * r + 3 < d) { dz.w = dzp[3]; z.w = zp[3]; }
        if (dZ_next) dz = dz + *reinterpret_cast<const f32x4 *>(dZ_next + off);      // padded columns hold zeros
        float dot = z.x * dz.x + z.y * dz.y + z.z * dz.z + z.w * dz.w;
        dot = row_allreduce_sum<LPR>(dot);
        const f32x4 dn = (dz - z * dot) * inv_norm[row];
        const f32x4 gt = *reinterpret_cast<const f32x4 *>(gate + off);
        *reinterpret_cast<f32x4 *>(dpre + off) = dn * gt;
    }
}

// ---- the batch loss in a fixed order ----------------------------------------------------------------------------------------
// qrec_bpr_batch_loss_grad adds its blocks' loss sums with one fp64 atomic per block: right to the last bits but one, in an order that
// changes from launch to launch.  Parity runs of these trainers read the loss from here instead: one wavefront per triplet
// (lane = column, butterfly sum), wavefront w of block k walks triplets k*4 + w, k*4 + w + 4*gridDim, ... in order, the block's four
// sums are added in wave order and ASSIGNED to slot k; the host adds the slots in order.  Same arithmetic per triplet as the
// gradient kernel (graph.hip): fp32 dots, -logf(s + eps) + reg/2 |rows|^2 accumulated in fp64.
__global__ __launch_bounds__(256) void batch_loss_slots_kernel(const float *__restrict__ S, float div, int n_users, int ld,
                                                               const int32_t *__restrict__ u_idx, const int32_t *__restrict__ i_idx,
                                                               const int32_t *__restrict__ j_idx, int B, float eps, float reg,
                                                               double *__restrict__ slots) {
    __shared__ double s_loss[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double loss = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const float *pu = S + (int64_t)u_idx[b] * ld, *pi = S + (int64_t)(n_users + i_idx[b]) * ld, *pj = S + (int64_t)(n_users + j_idx[b]) * ld;
        float di = 0.f, dj = 0.f, sq = 0.f;
        for (int c = lane; c < ld; c += kWave) {
            const float ub = pu[c] / div, ib = pi[c] / div, jb = pj[c] / div;
            di += ub * ib; dj += ub * jb; sq += ub * ub + ib * ib + jb * jb;
        }
        di = row_allreduce_sum<kWave>(di); dj = row_allreduce_sum<kWave>(dj); sq = row_allreduce_sum<kWave>(sq);
        const float sg = 1.0f / (1.0f + expf(-(di - dj)));
        loss += (double)(-logf(sg + eps)) + 0.5 * (double)reg * (double)sq;
    }
    if (lane == 0) s_loss[wave] = loss;
    __syncthreads();
    if (threadIdx.x == 0) slots[blockIdx.x] = ((s_loss[0] + s_loss[1]) + s_loss[2]) + s_loss[3];
}

bool ld_ok(int ld) { return ld == 32 || ld == 64 || ld == 128; }

}  // namespace

extern "C" {

int qrec_dense_layer_fwd(const float *d_X1, const float *d_X2, const float *d_W, const float *d_R, int64_t n_rows, int32_t ld,
                         int32_t relu, float *d_Y, void *stream) {
    QREC_REQUIRE(d_X1 && d_W && d_Y && n_rows >= 0, "qrec_dense_layer_fwd: bad argument");
    QREC_REQUIRE(ld_ok(ld), "qrec_dense_layer_fwd: row stride must be 32, 64 or 128 floats (got %d)", ld);
    if (n_rows == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    const float *W2 = d_X2 ? d_W + (size_t)ld * ld : nullptr;
    const int32_t *no_ids = nullptr;
    return d_X2 ? launch_layer_fwd<ConcatOps<2>>(st, ld, n_rows, d_X1, d_X2, d_W, W2, d_R, n_rows, relu, d_Y, no_ids, no_ids)
                : launch_layer_fwd<ConcatOps<1>>(st, ld, n_rows, d_X1, d_X2, d_W, W2, d_R, n_rows, relu, d_Y, no_ids, no_ids);
}

int qrec_dense_layer_dpre_relu(const float *d_dY, const float *d_Y, int64_t n_rows, int32_t ld, float *d_dpre, void *stream) {
    QREC_REQUIRE(d_dY && d_Y && d_dpre && n_rows >= 0 && ld > 0 && ld % 4 == 0, "qrec_dense_layer_dpre_relu: bad argument");
    if (n_rows == 0) return QREC_OK;
    const int64_t n4 = n_rows * (ld / 4);
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(dpre_relu_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), d_dY, d_Y, n4, d_dpre);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_dense_layer_dpre_norm(const float *d_dWide, const float *d_wide, int32_t wide_ld, int32_t col_off, const float *d_dZ_next,
                               const float *d_inv_norm, const float *d_gate, int64_t n_rows, int32_t d, int32_t ld, float *d_dpre,
                               void *stream) {
    QREC_REQUIRE(d_dWide && d_wide && d_inv_norm && d_gate && d_dpre && n_rows >= 0 && d >= 1 && ld >= d,
                 "qrec_dense_layer_dpre_norm: bad argument");
    QREC_REQUIRE(col_off >= 0 && col_off + d <= wide_ld, "qrec_dense_layer_dpre_norm: column block outside the wide table");
    QREC_REQUIRE(ld_ok(ld), "qrec_dense_layer_dpre_norm: row stride must be 32, 64 or 128 floats (got %d)", ld);
    if (n_rows == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    int64_t blocks;
#define QREC_DP(LPR)                                                                                             \
    blocks = (n_rows + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)); if (blocks > 2048) blocks = 2048;                   \
    hipLaunchKernelGGL((dpre_norm_kernel<LPR>), dim3((unsigned)blocks), dim3(256), 0, st, d_dWide, d_wide, wide_ld, \
                       col_off, d_dZ_next, d_inv_norm, d_gate, n_rows, d, d_dpre)
    if (ld == 32) { QREC_DP(8); } else if (ld == 64) { QREC_DP(16); } else { QREC_DP(32); }
#undef QREC_DP
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_dense_layer_ws_bytes(int64_t n_rows, int32_t ld, int32_t n_w, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_rows >= 0 && (n_w == 1 || n_w == 2), "qrec_dense_layer_ws_bytes: bad argument");
    QREC_REQUIRE(ld_ok(ld), "qrec_dense_layer_ws_bytes: row stride must be 32, 64 or 128 floats (got %d)", ld);
    const int64_t slabs = wgrad_slabs(n_rows, ld);
    *bytes = (slabs > 0 ? slabs : 1) * n_w * (int64_t)ld * ld * 4;
    return QREC_OK;
}

int qrec_dense_layer_bwd(const float *d_dpre, const float *d_X1, const float *d_X2, const float *d_W, int64_t n_rows, int32_t ld,
                         int32_t accumulate_dX1, float *d_dX1, float *d_dX2, float *d_gW, void *d_ws, int64_t ws_bytes,
                         void *stream) {
    QREC_REQUIRE(d_dpre && d_X1 && d_W && d_dX1 && d_gW && n_rows >= 0, "qrec_dense_layer_bwd: bad argument");
    QREC_REQUIRE(!d_X2 == !d_dX2, "qrec_dense_layer_bwd: the second operand and its gradient come together");
    QREC_REQUIRE(ld_ok(ld), "qrec_dense_layer_bwd: row stride must be 32, 64 or 128 floats (got %d)", ld);
    const int nw = d_X2 ? 2 : 1;
    int64_t need = 0;
    int rc = qrec_dense_layer_ws_bytes(n_rows, ld, nw, &need);
    if (rc != QREC_OK) return rc;
    QREC_REQUIRE(d_ws && ws_bytes >= need, "qrec_dense_layer_bwd: workspace of %lld bytes, qrec_dense_layer_ws_bytes asks for %lld",
                 (long long)ws_bytes, (long long)need);
    hipStream_t st = as_stream(stream);
    if (n_rows == 0) {                                 // no rows: the weight gradient is zero, nothing else is written
        QREC_HIP_CHECK(hipMemsetAsync(d_gW, 0, (size_t)nw * ld * ld * sizeof(float), st));
        return QREC_OK;
    }
    float *partial = static_cast<float *>(d_ws), *gW2 = d_X2 ? d_gW + (size_t)ld * ld : nullptr;
    const float *W2 = d_X2 ? d_W + (size_t)ld * ld : nullptr;
    const int32_t *no_ids = nullptr;
    auto run = [&](auto policy) {
        using P = decltype(policy);
        const int brc = launch_layer_bwd<P>(st, ld, n_rows, d_dpre, d_W, W2, d_X1, d_X2, n_rows, accumulate_dX1, d_dX1, d_dX2, no_ids, no_ids);
        return brc != QREC_OK ? brc : launch_layer_wgrad<P>(st, ld, n_rows, d_X1, d_X2, d_dpre, n_rows, partial, no_ids, no_ids, d_gW, gW2);
    };
    return d_X2 ? run(ConcatOps<2>{}) : run(ConcatOps<1>{});
}

int qrec_bpr_batch_loss_slots(const float *d_S, float div, int32_t n_users, int32_t ld, const int32_t *d_u, const int32_t *d_i,
                              const int32_t *d_j, int32_t B, float eps, float reg, double *d_slots, int32_t n_slots, void *stream) {
    QREC_REQUIRE(d_S && d_slots && B >= 0 && div != 0.f && ld > 0 && n_slots >= 1 && n_slots <= 65535, "qrec_bpr_batch_loss_slots: bad argument");
    QREC_REQUIRE(B == 0 || (d_u && d_i && d_j), "qrec_bpr_batch_loss_slots: null index array");
    hipLaunchKernelGGL(batch_loss_slots_kernel, dim3((unsigned)n_slots), dim3(256), 0, as_stream(stream), d_S, div, n_users, ld, d_u, d_i,
                       d_j, B, eps, reg, d_slots);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // extern "C"
