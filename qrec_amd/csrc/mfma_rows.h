// Pieces the row-tiled fp32 MFMA kernels share (ngcf.hip, dense_layer.hip): the C/D layout of
// v_mfma_f32_32x32x2_f32 and a wavefront's 32 x LD operand tile parked in LDS.
#pragma once
#include "common.h"

namespace qrec {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// C/D layout of v_mfma_f32_32x32x2_f32: col = lane&31, row = (q&3) + 8*(q>>2) + 4*(lane>>5)
__device__ __forceinline__ int cd_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

constexpr int kTilePad = 4;

template <int LD>
struct RowTile {                                  // a wavefront's view of one 32 x LD tile
    static constexpr int RS = LD + kTilePad;      // LDS row stride (floats)
    static constexpr int LPRW = LD / 4;           // lanes per row in the load layout
    static constexpr int RPI = kWave / LPRW;      // rows per load instruction
    static constexpr int NV = 32 / RPI;           // float4 per lane per tile
    int lrow, lcol;
    __device__ explicit RowTile(int lane) : lrow(lane / LPRW), lcol(4 * (lane % LPRW)) {}
    // row_ids (may be null): the tile's rows are row_ids[row0 ...] instead of row0 ... (a listed subset of the table)
    __device__ void load(const float *__restrict__ X, int64_t row0, int64_t n_rows, f32x4 (&v)[NV],
                         const int32_t *__restrict__ row_ids = nullptr) const {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            int64_t row = row0 + k * RPI + lrow;
            if (row >= n_rows) row = n_rows - 1;                 // rows past the end: a copy of the last row, never stored
            if (row_ids) row = row_ids[row];
            v[k] = *reinterpret_cast<const f32x4 *>(X + row * LD + lcol);
        }
    }
    __device__ void park(float *tile, const f32x4 (&v)[NV]) const {
#pragma unroll
        for (int k = 0; k < NV; k++) *reinterpret_cast<f32x4 *>(tile + (k * RPI + lrow) * RS + lcol) = v[k];
    }
    // MFMA A fragment of lane (r, h): columns [32h, 32h + 32) of row r (LD = 32: the upper k-slot feeds zeros)
    __device__ static void fragment(const float *tile, int r, int h, float (&a)[32]) {
        const bool kv = 32 * h < LD;
        const float keep = kv ? 1.f : 0.f;
        const float *p = tile + r * RS + (kv ? 32 * h : 0);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(p + 4 * q);
            a[4 * q] = v.x * keep; a[4 * q + 1] = v.y * keep; a[4 * q + 2] = v.z * keep; a[4 * q + 3] = v.w * keep;
        }
    }
};

}  // namespace qrec
