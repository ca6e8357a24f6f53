// The row-tiled fp32 MFMA layer kernels: one set for NGCF's propagation layer (ngcf.hip) and for the dense layer of the
// diffusion / hypergraph models (dense_layer.hip).
//
//   forward   Y[rows][ld] = sum_w a[w] W[w]  (+ R, ReLU)                       layer_fwd_lds_kernel / layer_fwd_wide_kernel
//   backward  dA[w] = dpre W[w]^T, then the policy's epilogue                  layer_bwd_lds_kernel / layer_bwd_wide_kernel
//   weights   partial[slab][w] = a[w]^T dpre over the slab's rows              layer_wgrad_lds_kernel / layer_wgrad_wide_kernel
//             gW[w] = sum_slab partial[slab][w], in a fixed order              wgrad_sum_kernel
//
// Tables are [rows][ld] fp32 with ld in {32, 64, 128}; a weight block is [ld][ld], zero-padded.  One wavefront per 32 rows.
// ld <= 64 (the *_lds kernels): the B fragments sit in registers for the whole launch and the A tile comes through a
// wave-private LDS tile (RowTile).  ld = 128 (the *_wide kernels): the weights are staged in LDS once per block, the A operand
// is the lane's own row.  No atomics anywhere: the weight gradient is per-slab partial products, summed in slab order.
//
// What a model's layer IS -- which tables it reads and how the operands a[w] are formed from them -- is an OPERAND POLICY, a
// compile-time argument of every kernel.  A policy states, and nothing else states:
//   NIN, NW          input tables X[0 .. NIN) and products a[w] W[w], w < NW
//   operand          a[w] from the values of X[0] and X[1] at one place (a float4 of a tile, or one float of a row)
//   staged           the same at one place of the ld <= 64 weight gradient's LDS stage, for a wave-uniform run-time w
//   Epilogue<NT>     what the backward does with dA[0], dA[1] of an element, and which values (C layout, at the table rows
//                    prow(q) of the lane's 16 output rows) it fetches for that BEFORE the MFMA loop: a wavefront owns a
//                    single tile there, nothing else hides their latency
//   kRowSubset       the ld <= 64 kernels take a listed row subset (row_ids, its count on the device)
//   kResidualRelu    the forward adds a residual R (may be null) and applies an optional ReLU
//   kWideBwdUnroll   unroll count of the two 64-column chunks of the ld = 128 backward
// All of it is compile-time: several instantiations sit at exactly 256 VGPRs, and a run-time R or row_ids one model never
// passes would cost the other its registers.  Every kernel takes the same argument list whatever the policy; a policy ignores
// the arguments it has no use for (callers pass null / 0), and the ld = 128 kernels ignore row_ids.
#pragma once
#include "mfma_rows.h"

namespace qrec {

// ---- operand policies --------------------------------------------------------------------------------------------------------
// Concatenation: Y = [X[0] | X[1]] W (+ R), W = NW blocks; the concatenation only ever exists as NW accumulating MFMA chains.
// Backward: dX[0] (=|+=) dA[0], dX[1] = dA[1].
template <int NW_>
struct ConcatOps {
    static constexpr int NIN = NW_, NW = NW_;
    static constexpr bool kRowSubset = false, kResidualRelu = true;
    static constexpr int kWideBwdUnroll = 1;        // a LOOP: unrolled, both chunks' dpre values are live next to the accumulators
    template <typename T>
    __device__ static T operand(int w, T x0, T x1) { return w == 0 ? x0 : x1; }
    __device__ static float staged(int w, const float *p0, const float *p1) { return *(w == 0 ? p0 : p1); }
    template <int NT>
    struct Epilogue {
        // accumulate: what dX[0] holds.  ld <= 64 fetches it early; ld = 128 has 64 accumulator registers per product and
        // reads it in place when it stores
        float old[NT][16];
        template <class F>
        __device__ void fetch(const float *, const float *, const float *dX0, int accumulate, F prow, int r) {
            if constexpr (NT < 4) {
                if (accumulate) {
#pragma unroll
                    for (int q = 0; q < 16; q++)
#pragma unroll
                        for (int t = 0; t < NT; t++) old[t][q] = dX0[prow(q) * (32 * NT) + 32 * t + r];
                }
            }
        }
        __device__ void store(int t, int q, int64_t o, float dA0, float dA1, int accumulate, float *dX0, float *dX1) const {
            if constexpr (NT < 4) dX0[o] = accumulate ? old[t][q] + dA0 : dA0;
            else dX0[o] = accumulate ? dX0[o] + dA0 : dA0;
            if (NW == 2) dX1[o] = dA1;
        }
    };
};

// NGCF (model/ranking/NGCF.py:27-42): X[0] = E, X[1] = side = A E;  a[0] = side + E, a[1] = E * side.
// Backward: dX[1] = dside = dA[0] + dA[1] * E,  dX[0] = dE = dA[0] + dA[1] * side.
struct SumProductOps {
    static constexpr int NIN = 2, NW = 2;
    static constexpr bool kRowSubset = true, kResidualRelu = false;
    static constexpr int kWideBwdUnroll = 2;        // unrolled: the second chunk's dpre loads go out with the epilogue's fetch
    template <typename T>
    __device__ static T operand(int w, T e, T sd) { return w == 0 ? sd + e : e * sd; }
    __device__ static float staged(int w, const float *p0, const float *p1) {
        const float e = *p0, sd = *p1;
        return w == 0 ? sd + e : e * sd;
    }
    template <int NT>
    struct Epilogue {
        float ev[NT][16], sv[NT][16];                  // E and side in C layout: 128-byte runs
        template <class F>
        __device__ void fetch(const float *E, const float *side, const float *, int, F prow, int r) {
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    const int64_t o = prow(q) * (32 * NT) + 32 * t + r;
                    ev[t][q] = E[o]; sv[t][q] = side[o];
                }
        }
        __device__ void store(int t, int q, int64_t o, float dA0, float dA1, int, float *dE, float *dside) const {
            dside[o] = dA0 + dA1 * ev[t][q];
            dE[o] = dA0 + dA1 * sv[t][q];
        }
    };
};

// ---- forward -----------------------------------------------------------------------------------------------------------------
// ld <= 64.  A 32 x LD tile is fetched with LD/8 fully coalesced float4 loads per lane and table, parked in the wave-private LDS
// tile and read back in fragment order; the next tile's global loads are issued before the current tile's MFMA loop.  The
// weights never change inside a launch and a wavefront's B fragments of all NW blocks are NW * NT * 32 values per lane, so
// they live in registers (one wavefront per SIMD, a persistent loop over tiles): the MFMA loop reads nothing from memory.
// (B values read from LDS right before their MFMA -- 64 ds_read2 per tile -- cost 14 us of NGCF's 25 at the Yelp2018 shape.)
// Timeline there (wall_clock64 stamps per wavefront, 1024 wavefronts, 2179 tiles): weights + first tile 3.6 us, then per tile
// 0.6 (park / fragment) + 4.5 (128 MFMAs) + 0.9 (stores); every wavefront has two tiles and 131 have a third: 21.4 us, of which
// 5 are that ragged third round.  Two wavefronts per SIMD without the prefetch: 24.6 us.
template <int NT, class P>
__global__ __launch_bounds__(256) void layer_fwd_lds_kernel(const float *__restrict__ X0, const float *__restrict__ X1,
                                                            const float *__restrict__ W0, const float *__restrict__ W1,
                                                            const float *__restrict__ R, int64_t n_all, int relu,
                                                            float *__restrict__ Y, const int32_t *__restrict__ row_ids,
                                                            const int32_t *__restrict__ n_ids) {
    constexpr int LD = 32 * NT, NIN = P::NIN, NW = P::NW;
    using Tile = RowTile<LD>;
    extern __shared__ float s_mem[];                // one tile per wavefront
    const float *const X[2] = {X0, X1}, *const W[2] = {W0, W1};
    const int32_t *ids = P::kRowSubset ? row_ids : nullptr;
    const float *res = P::kResidualRelu ? R : nullptr;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    float *tile_mem = s_mem + (threadIdx.x >> 6) * (32 * Tile::RS);
    const Tile tl(lane);
    const int kb = 32 * h < LD ? 32 * h : 0;        // ld = 32: the upper k-slot has no columns; its A values are zeros
    const int64_t n_rows = ids ? *n_ids : n_all;    // rows to process: the listed ones, or all
    const int64_t n_tiles = (n_rows + 31) / 32, stride = (int64_t)gridDim.x * 4;
    int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    f32x4 x[NIN][Tile::NV];
    if (tile < n_tiles) {
#pragma unroll
        for (int i = 0; i < NIN; i++) tl.load(X[i], tile * 32, n_rows, x[i], ids);
    }
    float b[NW][NT][32];                            // B fragments: W[w][kb + s][32 t + r], loaded in the order the first tile's MFMAs use them
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int s = 0; s < 32; s++)
#pragma unroll
            for (int w = 0; w < NW; w++) b[w][t][s] = W[w][(kb + s) * LD + 32 * t + r];
    for (; tile < n_tiles; tile += stride) {
        const int64_t row0 = tile * 32;
        float a[NW][32];
#pragma unroll
        for (int w = 0; w < NW; w++) {              // same wavefront, LDS operations complete in order
            f32x4 aw[Tile::NV];
#pragma unroll
            for (int k = 0; k < Tile::NV; k++) aw[k] = P::operand(w, x[0][k], x[NIN - 1][k]);
            tl.park(tile_mem, aw); Tile::fragment(tile_mem, r, h, a[w]);
        }
        // the residual (C layout: 128-byte runs) and the next tile go out before the MFMA loop
        float rv[NT][16];
        if (res) {
#pragma unroll
            for (int q = 0; q < 16; q++) {
                int64_t orow = row0 + cd_row(q, h);
                if (orow >= n_rows) orow = n_rows - 1;
#pragma unroll
                for (int t = 0; t < NT; t++) rv[t][q] = res[orow * LD + 32 * t + r];
            }
        }
        if (tile + stride < n_tiles) {
#pragma unroll
            for (int i = 0; i < NIN; i++) tl.load(X[i], (tile + stride) * 32, n_rows, x[i], ids);
        }
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[t][q] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int s = 0; s < 32; s++)
#pragma unroll
                for (int w = 0; w < NW; w++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[w][s], b[w][t][s], acc[t], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 16; q++) {
            int64_t orow = row0 + cd_row(q, h);
            if (orow < n_rows) {
                if (ids) orow = ids[orow];
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    float v = acc[t][q];
                    if (res) v += rv[t][q];
                    Y[orow * LD + 32 * t + r] = P::kResidualRelu && relu ? fmaxf(v, 0.f) : v;
                }
            }
        }
    }
}

// ld = 128: persistent blocks, the weights staged in LDS once per block (NW x 64 KB); A operand: the lane's own row, 8 float4
// loads per table and 64-column chunk; B operand: ds_read_b32 of W[w][k][32t + r] (consecutive lanes, consecutive banks).
// The 64-column chunks stay a LOOP: unrolled, both chunks' NW x 32 A values are live next to the 64 accumulator registers and
// NGCF's kernel spilled 126 VGPRs (508 B of scratch per lane).
template <class P>
__global__ __launch_bounds__(256) void layer_fwd_wide_kernel(const float *__restrict__ X0, const float *__restrict__ X1,
                                                             const float *__restrict__ W0, const float *__restrict__ W1,
                                                             const float *__restrict__ R, int64_t n_rows, int relu,
                                                             float *__restrict__ Y, const int32_t *, const int32_t *) {
    constexpr int NT = 4, LD = 128, NIN = P::NIN, NW = P::NW;
    extern __shared__ float s_w[];                  // [NW][LD][LD]
    const float *const X[2] = {X0, X1}, *const W[2] = {W0, W1};
    const float *res = P::kResidualRelu ? R : nullptr;
    for (int k = threadIdx.x; k < LD * LD / 4; k += blockDim.x)
#pragma unroll
        for (int w = 0; w < NW; w++) reinterpret_cast<f32x4 *>(s_w + w * LD * LD)[k] = reinterpret_cast<const f32x4 *>(W[w])[k];
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t n_tiles = (n_rows + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t row0 = tile * 32, row = row0 + r;
        const int64_t rowc = row < n_rows ? row : n_rows - 1;      // rows past the end are computed on a copy, not stored
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[t][q] = 0.f;
#pragma unroll 1
        for (int c = 0; c < LD; c += 64) {
            const int kb = c + 32 * h;
            const f32x4 *p0 = reinterpret_cast<const f32x4 *>(X[0] + rowc * LD + kb);
            const f32x4 *p1 = reinterpret_cast<const f32x4 *>(X[NIN - 1] + rowc * LD + kb);
            float a[NW][32];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const f32x4 x0 = p0[q], x1 = NIN == 2 ? p1[q] : x0;
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    const f32x4 v = P::operand(w, x0, x1);
                    a[w][4 * q] = v.x; a[w][4 * q + 1] = v.y; a[w][4 * q + 2] = v.z; a[w][4 * q + 3] = v.w;
                }
            }
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const float *w0 = s_w + kb * LD + 32 * t + r;
#pragma unroll
                for (int s = 0; s < 32; s++)
#pragma unroll
                    for (int w = 0; w < NW; w++)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[w][s], w0[w * LD * LD + s * LD], acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int64_t orow = row0 + cd_row(q, h);
                if (orow < n_rows) {
                    const int64_t o = orow * LD + 32 * t + r;
                    float v = acc[t][q];
                    if (res) v += res[o];
                    Y[o] = P::kResidualRelu && relu ? fmaxf(v, 0.f) : v;
                }
            }
    }
}

// ---- backward: dA[w] = dpre W[w]^T, then the policy's epilogue ------------------------------------------------------------------
// ld <= 64.  B[k][j] = W[w][j][k]: lane (r, h) holds W[w][32 t + r][kb .. kb + 32) -- its own row, 8 float4 loads per block.
template <int NT, class P>
__global__ __launch_bounds__(256) void layer_bwd_lds_kernel(const float *__restrict__ dpre, const float *__restrict__ W0,
                                                            const float *__restrict__ W1, const float *__restrict__ X0,
                                                            const float *__restrict__ X1, int64_t n_all, int accumulate,
                                                            float *__restrict__ dX0, float *__restrict__ dX1,
                                                            const int32_t *__restrict__ row_ids, const int32_t *__restrict__ n_ids) {
    constexpr int LD = 32 * NT, NW = P::NW;
    using Tile = RowTile<LD>;
    extern __shared__ float s_mem[];                // one tile per wavefront
    const float *const W[2] = {W0, W1};
    const int32_t *ids = P::kRowSubset ? row_ids : nullptr;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    float *tile_mem = s_mem + (threadIdx.x >> 6) * (32 * Tile::RS);
    const Tile tl(lane);
    const int kb = 32 * h < LD ? 32 * h : 0;
    const int64_t n_rows = ids ? *n_ids : n_all;
    const int64_t n_tiles = (n_rows + 31) / 32, stride = (int64_t)gridDim.x * 4;
    int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    f32x4 gn[Tile::NV];
    if (tile < n_tiles) tl.load(dpre, tile * 32, n_rows, gn, ids);
    float b[NW][NT][32];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 8; q++)
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(W[w] + (32 * t + r) * LD + kb + 4 * q);
                b[w][t][4 * q] = v.x; b[w][t][4 * q + 1] = v.y; b[w][t][4 * q + 2] = v.z; b[w][t][4 * q + 3] = v.w;
            }
    for (; tile < n_tiles; tile += stride) {
        const int64_t row0 = tile * 32;
        float g[32];
        tl.park(tile_mem, gn); Tile::fragment(tile_mem, r, h, g);
        // prow(q): the table row of this lane's q-th output row (past the end: the last row, never stored).  A subset looks its
        // 16 up once and keeps them; without one they are recomputed where used and nothing stays live over the MFMA loop
        auto clamped = [&](int q) { const int64_t orow = row0 + cd_row(q, h); return orow < n_rows ? orow : n_rows - 1; };
        int64_t listed[P::kRowSubset ? 16 : 1];
        if constexpr (P::kRowSubset) {
#pragma unroll
            for (int q = 0; q < 16; q++) listed[q] = ids ? (int64_t)ids[clamped(q)] : clamped(q);
        }
        auto prow = [&](int q) {
            if constexpr (P::kRowSubset) return listed[q];
            else return clamped(q);
        };
        // the epilogue's values and the next tile go out before the MFMA loop
        typename P::template Epilogue<NT> ep;
        ep.fetch(X0, X1, dX0, accumulate, prow, r);
        if (tile + stride < n_tiles) tl.load(dpre, (tile + stride) * 32, n_rows, gn, ids);
        f32x16 acc[NW][NT];
#pragma unroll
        for (int w = 0; w < NW; w++)
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int q = 0; q < 16; q++) acc[w][t][q] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int s = 0; s < 32; s++)
#pragma unroll
                for (int w = 0; w < NW; w++) acc[w][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[s], b[w][t][s], acc[w][t], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int64_t orow = row0 + cd_row(q, h);
            if (orow < n_rows) {
#pragma unroll
                for (int t = 0; t < NT; t++) ep.store(t, q, prow(q) * LD + 32 * t + r, acc[0][t][q], acc[NW - 1][t][q], accumulate, dX0, dX1);
            }
        }
    }
}

// ld = 128: the weights TRANSPOSED on their way into LDS (s_wt[w][k][j], rows padded by one float: the transposing writes fall
// on distinct banks), B reads consecutive lanes on consecutive banks
template <class P>
__global__ __launch_bounds__(256) void layer_bwd_wide_kernel(const float *__restrict__ dpre, const float *__restrict__ W0,
                                                             const float *__restrict__ W1, const float *__restrict__ X0,
                                                             const float *__restrict__ X1, int64_t n_rows, int accumulate,
                                                             float *__restrict__ dX0, float *__restrict__ dX1,
                                                             const int32_t *, const int32_t *) {
    constexpr int NT = 4, LD = 128, LDP = LD + 1, NW = P::NW;
    extern __shared__ float s_w[];                  // [NW][LD][LDP], transposed
    const float *const W[2] = {W0, W1};
    for (int k = threadIdx.x; k < LD * LD; k += blockDim.x) {
        const int j = k / LD, c = k % LD;           // coalesced read of W[w][j][c], write to s_wt[w][c][j]
#pragma unroll
        for (int w = 0; w < NW; w++) s_w[(w * LD + c) * LDP + j] = W[w][k];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t n_tiles = (n_rows + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t row0 = tile * 32, row = row0 + r;
        const int64_t rowc = row < n_rows ? row : n_rows - 1;
        f32x16 acc[NW][NT];
#pragma unroll
        for (int w = 0; w < NW; w++)
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int q = 0; q < 16; q++) acc[w][t][q] = 0.f;
        auto prow = [&](int q) { const int64_t orow = row0 + cd_row(q, h); return orow < n_rows ? orow : n_rows - 1; };
        typename P::template Epilogue<NT> ep;
        ep.fetch(X0, X1, dX0, accumulate, prow, r);
#pragma unroll P::kWideBwdUnroll
        for (int c = 0; c < LD; c += 64) {
            const int kb = c + 32 * h;
            const f32x4 *pg = reinterpret_cast<const f32x4 *>(dpre + rowc * LD + kb);
            float g[32];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const f32x4 v = pg[q];
                g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const float *w0 = s_w + kb * LDP + 32 * t + r;
#pragma unroll
                for (int s = 0; s < 32; s++)
#pragma unroll
                    for (int w = 0; w < NW; w++)
                        acc[w][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[s], w0[w * LD * LDP + s * LDP], acc[w][t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int64_t orow = row0 + cd_row(q, h);
                if (orow < n_rows) ep.store(t, q, orow * LD + 32 * t + r, acc[0][t][q], acc[NW - 1][t][q], accumulate, dX0, dX1);
            }
    }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
// ld <= 64.  A block owns kBlockRows rows; its 256 threads fetch a stage of 32 rows of the input tables and dpre with
// coalesced float4 loads into a double-buffered LDS stage while the previous stage is being multiplied; wavefront v owns the
// output block (w = v / NT, ti = v % NT) -- 32 rows of gW[w], all LD columns -- so nothing is summed across wavefronts.  Per
// stage and wavefront: 16 k-steps (row 2s + h of the stage), the A value P::staged at column 32 ti + r, NT reads for B, NT MFMAs.
// partial[slab][w][i][j], slab = block (a slab past a row subset's count holds zeros); wgrad_sum_kernel adds the slabs in order.
constexpr int kBlockRows = 128;
template <int NT, class P>
__global__ __launch_bounds__(256) void layer_wgrad_lds_kernel(const float *__restrict__ X0, const float *__restrict__ X1,
                                                              const float *__restrict__ dpre, int64_t n_all,
                                                              float *__restrict__ partial, const int32_t *__restrict__ row_ids,
                                                              const int32_t *__restrict__ n_ids) {
    constexpr int LD = 32 * NT, RS = LD + kTilePad, NIN = P::NIN, NW = P::NW;
    constexpr int NV = 32 * LD / 4 / 256;          // float4 per thread, array and stage (LD = 64: 2, LD = 32: 1)
    constexpr int kStage = 3 * 32 * RS;            // floats per stage buffer: X[0], X[1], dpre
    extern __shared__ float s_mem[];               // [2][3][32][RS]
    const float *const X[2] = {X0, X1};
    const int32_t *ids = P::kRowSubset ? row_ids : nullptr;
    const int64_t n_rows = ids ? *n_ids : n_all;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int which = wave / NT, ti = wave % NT;
    const bool owner = wave < NW * NT;             // the other wavefronts only help fetching
    const int64_t n0 = (int64_t)blockIdx.x * kBlockRows;
    f32x4 vx[NIN][NV], vd[NV];
    auto fetch = [&](int st) {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int idx = threadIdx.x + 256 * k, row = idx / (LD / 4), c4 = 4 * (idx % (LD / 4));
            int64_t n = n0 + 32 * st + row;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NIN; i++) vx[i][k] = zero;             // rows past the end contribute 0
            vd[k] = zero;
            if (n < n_rows) {
                if (ids) n = ids[n];
#pragma unroll
                for (int i = 0; i < NIN; i++) vx[i][k] = *reinterpret_cast<const f32x4 *>(X[i] + n * LD + c4);
                vd[k] = *reinterpret_cast<const f32x4 *>(dpre + n * LD + c4);
            }
        }
    };
    auto park = [&](int buf) {
        float *b = s_mem + buf * kStage;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int idx = threadIdx.x + 256 * k, row = idx / (LD / 4), c4 = 4 * (idx % (LD / 4));
#pragma unroll
            for (int i = 0; i < NIN; i++) *reinterpret_cast<f32x4 *>(b + i * 32 * RS + row * RS + c4) = vx[i][k];
            *reinterpret_cast<f32x4 *>(b + 64 * RS + row * RS + c4) = vd[k];
        }
    };
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 16; q++) acc[t][q] = 0.f;
    constexpr int kStages = kBlockRows / 32;
    fetch(0); park(0);
    __syncthreads();
    for (int st = 0; st < kStages; st++) {
        const bool more = st + 1 < kStages && n0 + 32 * (st + 1) < n_rows;
        if (more) fetch(st + 1);
        if (owner) {
            const float *b = s_mem + (st & 1) * kStage;
            const float *p0 = b + h * RS + 32 * ti + r, *p1 = p0 + 32 * RS, *pd = b + 64 * RS + h * RS + r;
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const float a = P::staged(which, p0 + 2 * s * RS, p1 + 2 * s * RS);
#pragma unroll
                for (int t = 0; t < NT; t++)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pd[2 * s * RS + 32 * t], acc[t], 0, 0, 0);
            }
        }
        if (more) park((st + 1) & 1);
        __syncthreads();
        if (!more) break;
    }
    if (owner) {
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++)
                partial[(((int64_t)blockIdx.x * NW + which) * LD + 32 * ti + cd_row(q, h)) * LD + 32 * t + r] = acc[t][q];
    }
}

// ld = 128.  One wavefront per (128 rows, 32-column block ti of the inputs): it forms ALL NW products for all 4 column tiles of
// dpre, i.e. NW * 4 MFMAs per k-step from NIN + 4 coalesced dword loads (NGCF's first version issued 3 loads per MFMA from one
// wavefront per SIMD and sat in load latency: 98 us for 1.1 GFLOP).  A chunk's 32 k-steps are fetched first, then its MFMAs
// run.  Rows past the end feed a = 0.  A block's four wavefronts (512 rows = one slab) hold the same tiles over different rows
// and are summed through LDS in wave order.
constexpr int kWaveRows = 128;                 // rows one wavefront accumulates (64 gives the same 36 us and doubles the partial slabs)
constexpr int kSlabRows = 4 * kWaveRows;       // rows per block = per partial slab
template <class P>
__global__ __launch_bounds__(256) void layer_wgrad_wide_kernel(const float *__restrict__ X0, const float *__restrict__ X1,
                                                               const float *__restrict__ dpre, int64_t n_rows,
                                                               float *__restrict__ partial, const int32_t *, const int32_t *) {
    constexpr int NT = 4, LD = 128, NIN = P::NIN, NW = P::NW;
    extern __shared__ float s_acc[];               // [4 waves][NW*NT tiles][16][64 lanes]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int slab = blockIdx.x, ti = blockIdx.y;
    const int64_t n0 = (int64_t)slab * kSlabRows + (int64_t)wave * kWaveRows;
    f32x16 acc[NW][NT];
#pragma unroll
    for (int w = 0; w < NW; w++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[w][t][q] = 0.f;
    const float *p0 = X0 + 32 * ti + r, *p1 = (NIN == 2 ? X1 : X0) + 32 * ti + r, *pd = dpre + r;
    for (int c = 0; c < kWaveRows; c += 64) {
        float a[NW][32], b[NT][32];
#pragma unroll
        for (int s = 0; s < 32; s++) {
            const int64_t n = n0 + c + 32 * h + s;
            const int64_t nc = n < n_rows ? n : n_rows - 1;
            const float keep = n < n_rows ? 1.f : 0.f;
            const float x0 = p0[nc * LD], x1 = NIN == 2 ? p1[nc * LD] : x0;
#pragma unroll
            for (int w = 0; w < NW; w++) a[w][s] = P::operand(w, x0, x1) * keep;
#pragma unroll
            for (int t = 0; t < NT; t++) b[t][s] = pd[nc * LD + 32 * t];
        }
#pragma unroll
        for (int s = 0; s < 32; s++)
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int w = 0; w < NW; w++) acc[w][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[w][s], b[t][s], acc[w][t], 0, 0, 0);
    }
#pragma unroll
    for (int w = 0; w < NW; w++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++) s_acc[((wave * NW * NT + w * NT + t) * 16 + q) * 64 + lane] = acc[w][t][q];
    __syncthreads();
    constexpr int kPerWave = NW * NT * 16 * 64;    // floats one wavefront deposited
    for (int k = threadIdx.x; k < kPerWave; k += 256) {
        const float v = ((s_acc[k] + s_acc[kPerWave + k]) + s_acc[2 * kPerWave + k]) + s_acc[3 * kPerWave + k];
        const int ln = k & 63, q = (k >> 6) & 15, wt = k >> 10, w = wt / NT, t = wt % NT;
        partial[(((int64_t)slab * NW + w) * LD + 32 * ti + cd_row(q, ln >> 5)) * LD + 32 * t + (ln & 31)] = v;
    }
}

// gW[e] = sum over the slabs of partial[slab][e], e over the n4 float4 of the NW weight blocks; the first per4 of them are
// gW0's, the rest gW1's (two pointers: the blocks need not be adjacent).  A thread owns four consecutive elements of one of
// kSplit slab classes (slabs c, c + kSplit, ...: coalesced 16-byte loads, added in slab order); the class sums of an element
// meet in LDS and are added in class order -- a fixed tree, the same bits on every launch.
constexpr int kSplit = 16;
static __global__ __launch_bounds__(256) void wgrad_sum_kernel(const float *__restrict__ partial, int n_slabs, int n4, int per4,
                                                               float *__restrict__ gW0, float *__restrict__ gW1) {
    __shared__ f32x4 s_part[256];
    const int e4 = blockIdx.x * (256 / kSplit) + threadIdx.x / kSplit, c = threadIdx.x % kSplit;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (e4 < n4)
        for (int s = c; s < n_slabs; s += kSplit) acc = acc + reinterpret_cast<const f32x4 *>(partial)[(int64_t)s * n4 + e4];
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if (c == 0 && e4 < n4) {
        f32x4 t = s_part[threadIdx.x];
#pragma unroll
        for (int k = 1; k < kSplit; k++) t = t + s_part[threadIdx.x + k];
        reinterpret_cast<f32x4 *>(e4 < per4 ? gW0 : gW1)[e4 < per4 ? e4 : e4 - per4] = t;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// persistent grids: one wavefront per SIMD when the B fragments sit in registers (ld <= 64), one block per CU when the
// weights take up to 128 KB of LDS (ld = 128); never more blocks than there are 128-row groups
inline unsigned layer_grid(int64_t n_rows) {
    const int64_t groups = (n_rows + 127) / 128;
    return (unsigned)(groups < 256 ? groups : 256);
}
inline hipError_t allow_big_lds(const void *kernel, size_t bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// partial slabs of the weight gradient over n_rows rows: one [NW][ld][ld] block each
inline int64_t wgrad_slabs(int64_t n_rows, int ld) {
    const int64_t slab_rows = ld >= 128 ? kSlabRows : kBlockRows;
    return (n_rows + slab_rows - 1) / slab_rows;
}

// One launch of `wide` (ld = 128, with its dynamic LDS allowed first) or of lds32 / lds64 over `grid`; ld is 32, 64 or 128
template <typename KW, typename K1, typename K2, typename... A>
int launch_by_ld(int ld, KW wide, size_t wide_lds, K1 lds32, K2 lds64, size_t lds, dim3 grid, hipStream_t st, A... args) {
    if (ld == 128) {
        QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(wide), wide_lds));
        hipLaunchKernelGGL(wide, grid, dim3(256), wide_lds, st, args...);
    } else if (ld == 64) hipLaunchKernelGGL(lds64, grid, dim3(256), lds, st, args...);
    else hipLaunchKernelGGL(lds32, grid, dim3(256), lds, st, args...);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}
inline size_t wave_tiles_lds(int ld) { return (size_t)4 * 32 * (ld + kTilePad) * sizeof(float); }

// work_rows: the rows the launch is sized for -- all of them, or the host's bound on a row subset's count.
// args: the kernels' argument lists, as above.
template <class P, typename... A>
int launch_layer_fwd(hipStream_t st, int ld, int64_t work_rows, A... args) {
    return launch_by_ld(ld, &layer_fwd_wide_kernel<P>, (size_t)P::NW * ld * ld * sizeof(float), &layer_fwd_lds_kernel<1, P>,
                        &layer_fwd_lds_kernel<2, P>, wave_tiles_lds(ld), dim3(layer_grid(work_rows)), st, args...);
}
template <class P, typename... A>
int launch_layer_bwd(hipStream_t st, int ld, int64_t work_rows, A... args) {
    return launch_by_ld(ld, &layer_bwd_wide_kernel<P>, (size_t)P::NW * ld * (ld + 1) * sizeof(float), &layer_bwd_lds_kernel<1, P>,
                        &layer_bwd_lds_kernel<2, P>, wave_tiles_lds(ld), dim3(layer_grid(work_rows)), st, args...);
}
// the per-slab products over wgrad_slabs(work_rows, ld) slabs, then their sum into gW0 and (NW = 2) gW1
template <class P>
int launch_layer_wgrad(hipStream_t st, int ld, int64_t work_rows, const float *X0, const float *X1, const float *dpre, int64_t n_rows,
                       float *partial, const int32_t *row_ids, const int32_t *n_ids, float *gW0, float *gW1) {
    const int n_slabs = (int)wgrad_slabs(work_rows, ld);
    const int rc = launch_by_ld(ld, &layer_wgrad_wide_kernel<P>, (size_t)4 * P::NW * 4 * 16 * 64 * sizeof(float),
                                &layer_wgrad_lds_kernel<1, P>, &layer_wgrad_lds_kernel<2, P>,
                                (size_t)2 * 3 * 32 * (ld + kTilePad) * sizeof(float), dim3((unsigned)n_slabs, ld == 128 ? 4 : 1), st, X0, X1,
                                dpre, n_rows, partial, row_ids, n_ids);
    if (rc != QREC_OK) return rc;
    const int per4 = ld * ld / 4, n4 = P::NW * per4;
    hipLaunchKernelGGL(wgrad_sum_kernel, dim3((unsigned)((n4 + 256 / kSplit - 1) / (256 / kSplit))), dim3(256), 0, st, partial, n_slabs, n4,
                       per4, gW0, gW1);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // namespace qrec
