// The dense layer between two sparse products of the diffusion / hypergraph models and its backward pass.
//
//   DiffNet (model/ranking/DiffNet.py:46-49):  u' = relu([S u | u] W_k),  W_k (2d x d)
//   DHCF    (model/ranking/DHCF.py:74-87):     pre = (H E_0) W_k + z_{k-1}; z_k = l2_normalize(dropout(leaky_relu(pre)))
//
//   forward   Y = [X1 | X2] W (+ R), optionally through ReLU                       layer_fwd_*     (f32 MFMA)
//   backward  dPre = dY * (Y > 0)                                                  dpre_relu_kernel
//             dPre = normalize_bwd(dWide block + dZ_next) * gate                   dpre_norm_kernel
//             dX1 (=|+=) dPre W[0]^T, dX2 = dPre W[1]^T   (dR is dPre itself)      layer_bwd_*     (f32 MFMA)
//             gW = [X1 | X2]^T dPre                                                layer_wgrad_* + wgrad_sum_kernel
//
// Tables are [rows][ld] fp32 with ld in {32, 64, 128}.  W is stored zero-padded as NW blocks of [ld][ld] (NW = 2 with X2:
// block 0 multiplies X1, block 1 multiplies X2 -- the concatenation only ever exists as two accumulating MFMA chains).
// Same tiling as ngcf.hip: one wavefront per 32 rows; ld <= 64 keeps the B fragments in registers for the whole launch and
// brings the A tile through a wave-private LDS tile (RowTile); ld = 128 stages the weights in LDS.  No atomics anywhere:
// the weight gradient is per-slab partial products in a sized workspace, summed in slab order.
#include "mfma_rows.h"

using namespace qrec;

namespace {

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int NT, int NW>
__global__ __launch_bounds__(256) void layer_fwd_lds_kernel(const float *__restrict__ X1, const float *__restrict__ X2,
                                                            const float *__restrict__ W, const float *__restrict__ R,
                                                            int64_t n_rows, int relu, float *__restrict__ Y) {
    constexpr int LD = 32 * NT;
    using Tile = RowTile<LD>;
    extern __shared__ float s_mem[];                // one tile per wavefront
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    float *tile_mem = s_mem + (threadIdx.x >> 6) * (32 * Tile::RS);
    const Tile tl(lane);
    const int kb = 32 * h < LD ? 32 * h : 0;        // ld = 32: the upper k-slot has no columns; its A values are zeros
    const int64_t n_tiles = (n_rows + 31) / 32, stride = (int64_t)gridDim.x * 4;
    int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    f32x4 x1[Tile::NV], x2[Tile::NV];
    if (tile < n_tiles) {
        tl.load(X1, tile * 32, n_rows, x1);
        if (NW == 2) tl.load(X2, tile * 32, n_rows, x2);
    }
    float b[NW][NT][32];                            // B fragments: W[w][kb + s][32 t + r]
#pragma unroll
    for (int w = 0; w < NW; w++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int s = 0; s < 32; s++) b[w][t][s] = W[(w * LD + kb + s) * LD + 32 * t + r];
    for (; tile < n_tiles; tile += stride) {
        const int64_t row0 = tile * 32;
        float a1[32], a2[32];
        tl.park(tile_mem, x1); Tile::fragment(tile_mem, r, h, a1);
        if (NW == 2) { tl.park(tile_mem, x2); Tile::fragment(tile_mem, r, h, a2); }   // same wavefront, LDS operations complete in order
        // the residual (C layout: 128-byte runs) and the next tile go out before the MFMA loop
        float rv[NT][16];
        if (R) {
#pragma unroll
            for (int q = 0; q < 16; q++) {
                int64_t orow = row0 + cd_row(q, h);
                if (orow >= n_rows) orow = n_rows - 1;
#pragma unroll
                for (int t = 0; t < NT; t++) rv[t][q] = R[orow * LD + 32 * t + r];
            }
        }
        if (tile + stride < n_tiles) {
            tl.load(X1, (tile + stride) * 32, n_rows, x1);
            if (NW == 2) tl.load(X2, (tile + stride) * 32, n_rows, x2);
        }
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[t][q] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int s = 0; s < 32; s++) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b[0][t][s], acc[t], 0, 0, 0);
                if (NW == 2) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[s], b[NW - 1][t][s], acc[t], 0, 0, 0);
            }
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int64_t orow = row0 + cd_row(q, h);
            if (orow < n_rows) {
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    float v = acc[t][q];
                    if (R) v += rv[t][q];
                    Y[orow * LD + 32 * t + r] = relu ? fmaxf(v, 0.f) : v;
                }
            }
        }
    }
}

// ld = 128: persistent blocks, the weights staged in LDS once per block (NW x 64 KB); A operand: the lane's own row.
// The 64-column chunks stay a LOOP: unrolled, both chunks' A values are live next to the 64 accumulator registers.
template <int NW>
__global__ __launch_bounds__(256) void layer_fwd_wide_kernel(const float *__restrict__ X1, const float *__restrict__ X2,
                                                             const float *__restrict__ W, const float *__restrict__ R,
                                                             int64_t n_rows, int relu, float *__restrict__ Y) {
    constexpr int NT = 4, LD = 128;
    extern __shared__ float s_w[];                  // [NW][LD][LD]
    for (int k = threadIdx.x; k < NW * LD * LD / 4; k += blockDim.x)
        reinterpret_cast<f32x4 *>(s_w)[k] = reinterpret_cast<const f32x4 *>(W)[k];
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
            const f32x4 *p1 = reinterpret_cast<const f32x4 *>(X1 + rowc * LD + kb);
            const f32x4 *p2 = reinterpret_cast<const f32x4 *>((NW == 2 ? X2 : X1) + rowc * LD + kb);
            float a1[32], a2[32];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const f32x4 v = p1[q];
                a1[4 * q] = v.x; a1[4 * q + 1] = v.y; a1[4 * q + 2] = v.z; a1[4 * q + 3] = v.w;
                if (NW == 2) {
                    const f32x4 u = p2[q];
                    a2[4 * q] = u.x; a2[4 * q + 1] = u.y; a2[4 * q + 2] = u.z; a2[4 * q + 3] = u.w;
                }
            }
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const float *w1 = s_w + kb * LD + 32 * t + r, *w2 = w1 + (NW - 1) * LD * LD;
#pragma unroll
                for (int s = 0; s < 32; s++) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], w1[s * LD], acc[t], 0, 0, 0);
                    if (NW == 2) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[s], w2[s * LD], acc[t], 0, 0, 0);
                }
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
                    if (R) v += R[o];
                    Y[o] = relu ? fmaxf(v, 0.f) : v;
                }
            }
    }
}

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

// ---- backward: dX_w = dPre W[w]^T --------------------------------------------------------------------------------------------
// B[k][j] = W[w][j][k]: lane (r, h) holds W[w][32 t + r][kb .. kb + 32) -- its own row, 8 float4 loads per block.
template <int NT, int NW>
__global__ __launch_bounds__(256) void layer_bwd_lds_kernel(const float *__restrict__ dpre, const float *__restrict__ W,
                                                            int64_t n_rows, int accumulate, float *__restrict__ dX1,
                                                            float *__restrict__ dX2) {
    constexpr int LD = 32 * NT;
    using Tile = RowTile<LD>;
    extern __shared__ float s_mem[];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    float *tile_mem = s_mem + (threadIdx.x >> 6) * (32 * Tile::RS);
    const Tile tl(lane);
    const int kb = 32 * h < LD ? 32 * h : 0;
    const int64_t n_tiles = (n_rows + 31) / 32, stride = (int64_t)gridDim.x * 4;
    int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    f32x4 gn[Tile::NV];
    if (tile < n_tiles) tl.load(dpre, tile * 32, n_rows, gn);
    float b[NW][NT][32];
#pragma unroll
    for (int w = 0; w < NW; w++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(W + (w * LD + 32 * t + r) * LD + kb + 4 * q);
                b[w][t][4 * q] = v.x; b[w][t][4 * q + 1] = v.y; b[w][t][4 * q + 2] = v.z; b[w][t][4 * q + 3] = v.w;
            }
    for (; tile < n_tiles; tile += stride) {
        const int64_t row0 = tile * 32;
        float g[32];
        tl.park(tile_mem, gn); Tile::fragment(tile_mem, r, h, g);
        float old[NT][16];                              // accumulate: what dX1 holds (C layout), fetched before the MFMA loop
        if (accumulate) {
#pragma unroll
            for (int q = 0; q < 16; q++) {
                int64_t orow = row0 + cd_row(q, h);
                if (orow >= n_rows) orow = n_rows - 1;
#pragma unroll
                for (int t = 0; t < NT; t++) old[t][q] = dX1[orow * LD + 32 * t + r];
            }
        }
        if (tile + stride < n_tiles) tl.load(dpre, (tile + stride) * 32, n_rows, gn);
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
                for (int t = 0; t < NT; t++) {
                    const int64_t o = orow * LD + 32 * t + r;
                    dX1[o] = accumulate ? old[t][q] + acc[0][t][q] : acc[0][t][q];
                    if (NW == 2) dX2[o] = acc[NW - 1][t][q];
                }
            }
        }
    }
}

// ld = 128: the weights TRANSPOSED on their way into LDS (s_wt[w][k][j], rows padded by one float: the transposing writes fall
// on distinct banks), B reads consecutive lanes on consecutive banks
template <int NW>
__global__ __launch_bounds__(256) void layer_bwd_wide_kernel(const float *__restrict__ dpre, const float *__restrict__ W,
                                                             int64_t n_rows, int accumulate, float *__restrict__ dX1,
                                                             float *__restrict__ dX2) {
    constexpr int NT = 4, LD = 128, LDP = LD + 1;
    extern __shared__ float s_w[];                  // [NW][LD][LDP]
    for (int k = threadIdx.x; k < NW * LD * LD; k += blockDim.x) {
        const int w = k / (LD * LD), j = (k / LD) % LD, c = k % LD;       // coalesced read of W[w][j][c]
        s_w[(w * LD + c) * LDP + j] = W[k];
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
#pragma unroll 1
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
                const float *w1 = s_w + kb * LDP + 32 * t + r;
#pragma unroll
                for (int s = 0; s < 32; s++)
#pragma unroll
                    for (int w = 0; w < NW; w++)
                        acc[w][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[s], w1[w * LD * LDP + s * LDP], acc[w][t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int64_t orow = row0 + cd_row(q, h);
                if (orow < n_rows) {
                    const int64_t o = orow * LD + 32 * t + r;
                    dX1[o] = accumulate ? dX1[o] + acc[0][t][q] : acc[0][t][q];
                    if (NW == 2) dX2[o] = acc[NW - 1][t][q];
                }
            }
    }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
// ld <= 64.  A block owns kBlockRows rows; its 256 threads fetch a stage of 32 rows of X1, X2 and dpre with coalesced float4
// loads into a double-buffered LDS stage while the previous stage is being multiplied; wavefront w owns the output block
// (which = w / NT, ti = w % NT) -- 32 rows of gW[which], all LD columns -- so nothing is summed across wavefronts.
// partial[slab][which][i][j], slab = block; wgrad_sum_kernel adds the slabs in order.
constexpr int kBlockRows = 128;
template <int NT, int NW>
__global__ __launch_bounds__(256) void layer_wgrad_lds_kernel(const float *__restrict__ X1, const float *__restrict__ X2,
                                                              const float *__restrict__ dpre, int64_t n_rows,
                                                              float *__restrict__ partial) {
    constexpr int LD = 32 * NT, RS = LD + kTilePad;
    constexpr int NV = 32 * LD / 4 / 256;          // float4 per thread, array and stage (LD = 64: 2, LD = 32: 1)
    constexpr int kStage = 3 * 32 * RS;            // floats per stage buffer: X1, X2, dpre
    extern __shared__ float s_mem[];               // [2][3][32][RS]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int which = wave / NT, ti = wave % NT;
    const bool owner = wave < NW * NT;             // the other wavefronts only help fetching
    const int64_t n0 = (int64_t)blockIdx.x * kBlockRows;
    f32x4 v1[NV], v2[NV], vd[NV];
    auto fetch = [&](int st) {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int idx = threadIdx.x + 256 * k, row = idx / (LD / 4), c4 = 4 * (idx % (LD / 4));
            const int64_t n = n0 + 32 * st + row;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            v1[k] = zero; v2[k] = zero; vd[k] = zero;                  // rows past the end contribute 0
            if (n < n_rows) {
                v1[k] = *reinterpret_cast<const f32x4 *>(X1 + n * LD + c4);
                if (NW == 2) v2[k] = *reinterpret_cast<const f32x4 *>(X2 + n * LD + c4);
                vd[k] = *reinterpret_cast<const f32x4 *>(dpre + n * LD + c4);
            }
        }
    };
    auto park = [&](int buf) {
        float *b = s_mem + buf * kStage;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int idx = threadIdx.x + 256 * k, row = idx / (LD / 4), c4 = 4 * (idx % (LD / 4));
            *reinterpret_cast<f32x4 *>(b + row * RS + c4) = v1[k];
            if (NW == 2) *reinterpret_cast<f32x4 *>(b + 32 * RS + row * RS + c4) = v2[k];
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
            const float *pa = b + which * 32 * RS + h * RS + 32 * ti + r, *pd = b + 64 * RS + h * RS + r;
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const float a = pa[2 * s * RS];
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

// ld = 128.  One wavefront per (128 rows, 32-column block ti of X): it forms the products of BOTH operands for all 4 column
// tiles of dpre; a block's four wavefronts (512 rows = one slab) are summed through LDS in wave order.
constexpr int kWaveRows = 128;
constexpr int kSlabRows = 4 * kWaveRows;
template <int NW>
__global__ __launch_bounds__(256) void layer_wgrad_wide_kernel(const float *__restrict__ X1, const float *__restrict__ X2,
                                                               const float *__restrict__ dpre, int64_t n_rows,
                                                               float *__restrict__ partial) {
    constexpr int NT = 4, LD = 128;
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
    const float *p1 = X1 + 32 * ti + r, *p2 = (NW == 2 ? X2 : X1) + 32 * ti + r, *pd = dpre + r;
    for (int c = 0; c < kWaveRows; c += 64) {
        float a[NW][32], b[NT][32];
#pragma unroll
        for (int s = 0; s < 32; s++) {
            const int64_t n = n0 + c + 32 * h + s;
            const int64_t nc = n < n_rows ? n : n_rows - 1;
            const float keep = n < n_rows ? 1.f : 0.f;
            a[0][s] = p1[nc * LD] * keep;
            if (NW == 2) a[NW - 1][s] = p2[nc * LD] * keep;
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

// gW[e] = sum over the slabs of partial[slab][e], e over the NW * ld * ld elements.  A thread owns four consecutive
// elements of one of kSplit slab classes (slabs c, c + kSplit, ...: added in slab order); the class sums of an element
// meet in LDS and are added in class order -- a fixed tree, the same bits on every launch.
constexpr int kSplit = 16;
__global__ __launch_bounds__(256) void wgrad_sum_kernel(const float *__restrict__ partial, int n_slabs, int n4,
                                                        float *__restrict__ gW) {
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
        reinterpret_cast<f32x4 *>(gW)[e4] = t;
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

// persistent grids: one wavefront per SIMD when the B fragments sit in registers (ld <= 64), one block per CU when the
// weights take up to 128 KB of LDS (ld = 128); never more blocks than there are 128-row groups
unsigned layer_grid(int64_t n_rows) {
    const int64_t groups = (n_rows + 127) / 128;
    return (unsigned)(groups < 256 ? groups : 256);
}
hipError_t allow_big_lds(const void *kernel, size_t bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
int64_t wgrad_slabs(int64_t n_rows, int ld) {
    const int64_t slab_rows = ld >= 128 ? kSlabRows : kBlockRows;
    return (n_rows + slab_rows - 1) / slab_rows;
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
    const unsigned blocks = layer_grid(n_rows);
    const size_t lds_tiles = (size_t)4 * 32 * (ld + kTilePad) * sizeof(float);
    const int nw = d_X2 ? 2 : 1;
    const size_t lds_w = (size_t)nw * ld * ld * sizeof(float);
#define QREC_FWD(K, LDS) hipLaunchKernelGGL(K, dim3(blocks), dim3(256), LDS, st, d_X1, d_X2, d_W, d_R, n_rows, relu, d_Y)
    if (ld == 32) { if (nw == 2) QREC_FWD((layer_fwd_lds_kernel<1, 2>), lds_tiles); else QREC_FWD((layer_fwd_lds_kernel<1, 1>), lds_tiles); }
    else if (ld == 64) { if (nw == 2) QREC_FWD((layer_fwd_lds_kernel<2, 2>), lds_tiles); else QREC_FWD((layer_fwd_lds_kernel<2, 1>), lds_tiles); }
    else if (nw == 2) {
        QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(&layer_fwd_wide_kernel<2>), lds_w));
        QREC_FWD(layer_fwd_wide_kernel<2>, lds_w);
    } else {
        QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(&layer_fwd_wide_kernel<1>), lds_w));
        QREC_FWD(layer_fwd_wide_kernel<1>, lds_w);
    }
#undef QREC_FWD
    QREC_LAUNCH_CHECK();
    return QREC_OK;
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
    float *partial = static_cast<float *>(d_ws);
    const unsigned blocks = layer_grid(n_rows);
    const size_t lds_tiles = (size_t)4 * 32 * (ld + kTilePad) * sizeof(float);
    const size_t lds_w = (size_t)nw * ld * (ld + 1) * sizeof(float);
#define QREC_BWD(K, LDS) hipLaunchKernelGGL(K, dim3(blocks), dim3(256), LDS, st, d_dpre, d_W, n_rows, accumulate_dX1, d_dX1, d_dX2)
    if (ld == 32) { if (nw == 2) QREC_BWD((layer_bwd_lds_kernel<1, 2>), lds_tiles); else QREC_BWD((layer_bwd_lds_kernel<1, 1>), lds_tiles); }
    else if (ld == 64) { if (nw == 2) QREC_BWD((layer_bwd_lds_kernel<2, 2>), lds_tiles); else QREC_BWD((layer_bwd_lds_kernel<2, 1>), lds_tiles); }
    else if (nw == 2) {
        QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(&layer_bwd_wide_kernel<2>), lds_w));
        QREC_BWD(layer_bwd_wide_kernel<2>, lds_w);
    } else {
        QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(&layer_bwd_wide_kernel<1>), lds_w));
        QREC_BWD(layer_bwd_wide_kernel<1>, lds_w);
    }
#undef QREC_BWD
    QREC_LAUNCH_CHECK();
    const int n_slabs = (int)wgrad_slabs(n_rows, ld);
    const size_t wlds = ld == 128 ? (size_t)4 * nw * 4 * 16 * 64 * sizeof(float) : (size_t)2 * 3 * 32 * (ld + kTilePad) * sizeof(float);
#define QREC_WG(K, GRID) hipLaunchKernelGGL(K, GRID, dim3(256), wlds, st, d_X1, d_X2, d_dpre, n_rows, partial)
    if (ld == 32) { if (nw == 2) QREC_WG((layer_wgrad_lds_kernel<1, 2>), dim3((unsigned)n_slabs)); else QREC_WG((layer_wgrad_lds_kernel<1, 1>), dim3((unsigned)n_slabs)); }
    else if (ld == 64) { if (nw == 2) QREC_WG((layer_wgrad_lds_kernel<2, 2>), dim3((unsigned)n_slabs)); else QREC_WG((layer_wgrad_lds_kernel<2, 1>), dim3((unsigned)n_slabs)); }
    else if (nw == 2) {
        QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(&layer_wgrad_wide_kernel<2>), wlds));
        QREC_WG(layer_wgrad_wide_kernel<2>, dim3((unsigned)n_slabs, 4));
    } else {
        QREC_HIP_CHECK(allow_big_lds(reinterpret_cast<const void *>(&layer_wgrad_wide_kernel<1>), wlds));
        QREC_WG(layer_wgrad_wide_kernel<1>, dim3((unsigned)n_slabs, 4));
    }
#undef QREC_WG
    QREC_LAUNCH_CHECK();
    const int n4 = nw * ld * ld / 4;
    hipLaunchKernelGGL(wgrad_sum_kernel, dim3((unsigned)((n4 + 256 / kSplit - 1) / (256 / kSplit))), dim3(256), 0, st, partial, n_slabs,
                       n4, d_gW);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
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
