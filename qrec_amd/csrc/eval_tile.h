// The evaluation's MFMA tile loop, stated once: 32 items x 32 users per tile, the user operand resident in registers, item tiles
// streamed.  The fp32 kernels (score_kernel_f32 of eval_block.hip; sample_max_kernel_f32, score_filter2_kernel_f32 and the
// re-scoring of select_topk_kernel in eval_fused.hip) run v_mfma_f32_32x32x2_f32 over chunks of 64 columns; the bf16 kernels
// (sample_max_bf16_kernel, score_filter_bf16_kernel) run v_mfma_f32_32x32x16_bf16 over slices of 16.  A kernel is these pieces
// plus its own epilogue.  Lane l of a wavefront is (r, h) = (l & 31, l >> 5): operand row r, k-slot h; accumulator register q of
// lane (r, h) is user column r, item row cd_row(q, h) of the tile (mfma_rows.h).  The fp64 loop (16 x 16 tiles, v_mfma_f64_16x16x4_f64)
// is one function with an epilogue functor, score_tiles_f64: score_kernel_f64 of eval_block.hip and score_form_kernel of rank_forms.hip.
//
// Operand fetch: the tables are zero-padded to the row stride ld (a multiple of 32 floats), so a lane reads ITS row's slot with
// unconditional 16-byte loads; rows past the end are clamped (their results are not stored).  (First version: one guarded dword
// load per element, 81 loads and 99 branches per 32 MFMAs.)
#pragma once
#include <type_traits>

#include "mfma_rows.h"

namespace qrec {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// ---- fp32: K consumed 2 slots x 32 columns per 64-chunk; slot h of chunk c owns columns [64c + 32h, 64c + 32h + 32) -- 8 f32x4.
// (the dot product does not care which physical column sits in which MFMA k-slot as long as A and B agree.)
template <int NC>          // chunks c0 .. c0 + NC - 1 of the row
struct F32Slots {
    int kb[NC];            // the slot's first column; 0 where ld = 32 (mod 64) leaves the last chunk's upper slot empty ...
    float keep[NC];        // ... and the USER fragment is multiplied by 0 there (the item side may then hold anything finite)
    __device__ __forceinline__ F32Slots(int ld, int h, int c0 = 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int col0 = 64 * (c0 + c) + 32 * h;
            const bool kv = col0 < ld;
            kb[c] = kv ? col0 : 0;
            keep[c] = kv ? 1.f : 0.f;
        }
    }
    __device__ __forceinline__ void load_user(const float *row, f32x4 (&u)[NC][8]) const {
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int q = 0; q < 8; q++) u[c][q] = reinterpret_cast<const f32x4 *>(row + kb[c])[q] * keep[c];
    }
    // the two 32-user tiles of a wavefront, their loads interleaved
    __device__ __forceinline__ void load_users(const float *row0, const float *row1, f32x4 (&ua)[NC][8],
                                               f32x4 (&ub)[NC][8]) const {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const f32x4 *p0 = reinterpret_cast<const f32x4 *>(row0 + kb[c]), *p1 = reinterpret_cast<const f32x4 *>(row1 + kb[c]);
#pragma unroll
            for (int q = 0; q < 8; q++) { ua[c][q] = p0[q] * keep[c]; ub[c][q] = p1[q] * keep[c]; }
        }
    }
    __device__ __forceinline__ void load_item(const float *row, f32x4 (&v)[NC][8]) const {
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int q = 0; q < 8; q++) v[c][q] = reinterpret_cast<const f32x4 *>(row + kb[c])[q];
    }
};

// item row `item` of V, clamped to the catalogue: rows past the end repeat the last item (never stored, never candidates)
__device__ __forceinline__ const float *item_row_clamped(const float *V, int item, int n_items, int ld) {
    return V + (int64_t)(item < n_items ? item : n_items - 1) * ld;
}

__device__ __forceinline__ void zero(f32x16 &acc) {
#pragma unroll
    for (int q = 0; q < 16; q++) acc[q] = 0.f;
}

// THE fp32 scoring sequence (ids and scores of every route are bit-identical because all of them add in this order): chunk by
// chunk, f32x4 by f32x4, .x .y .z .w.  One accumulator chain (the re-scoring of select_topk_kernel), or two, interleaved element by
// element: one wavefront serves TWO 32-user tiles per item tile, so the item operand (re-read from L2 by every user tile that needs
// it -- 990 user tiles x 9.7 MB at the Yelp shape) is fetched half as often and the matrix pipe always has an independent MFMA to issue
template <int NC>
struct F32Chain { const f32x4 (&u)[NC][8]; f32x16 &acc; };      // a user fragment and the accumulator of its 32 x 32 tile
template <int NC, typename... Chains>
__device__ __forceinline__ void mfma_f32(const f32x4 (&v)[NC][8], Chains... chains) {
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int q = 0; q < 8; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) ((chains.acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[c][q][j], chains.u[c][q][j], chains.acc, 0, 0, 0)), ...);
}

// ---- fp64: 16 items x 16 users per MFMA tile (v_mfma_f64_16x16x4_f64), 4 slots x 16 columns per 64-chunk; the same operand fetch
// (ld a multiple of 16 doubles, unconditional 16-byte loads, clamped rows, the next tile requested before the MFMAs).  Lane l is
// (r, h) = (l & 15, l >> 4): user column r of user tile `utile`, whose operand row is `urow` (U + urow * ld); accumulator register q
// is item row h + 4 q.  Chunks accumulate through the output block; on the LAST chunk epi(dot, item, b) turns the finished inner
// product of (item, user b = utile * 16 + r of the batch) into the stored score.  score_kernel_f64 (eval_block.hip) passes the
// identity and U[user_ids[b]]; the form scoring of rank_forms.hip passes its bias / distance epilogue and row b of a staged operand.
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct PlainScore {
    __device__ __forceinline__ double operator()(double dot, int, int) const { return dot; }
};

template <typename Epi>
__device__ __forceinline__ void score_tiles_f64(const double *__restrict__ U, int64_t urow, const double *__restrict__ V, int ld, int n_items,
                                                int b_pad, int item_tiles_per_wave, double *__restrict__ S_T, const Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, h = lane >> 4;
    const int utile = blockIdx.x;                       // 16 users
    const int n_chunks = (ld + 63) / 64;
    const int n_item_tiles = (n_items + 15) / 16;
    const int t_begin = (blockIdx.y * 4 + wave) * item_tiles_per_wave;
    int t_end = t_begin + item_tiles_per_wave;
    if (t_end > n_item_tiles) t_end = n_item_tiles;
    if (t_begin >= t_end) return;

    for (int c = 0; c < n_chunks; c++) {
        const int col0 = 64 * c + 16 * h;
        const bool kv = col0 < ld;
        const int kb = kv ? col0 : 0;
        const double keep = kv ? 1.0 : 0.0;
        f64x2 ub[8], va[8], vn[8];
        {
            const f64x2 *pu = reinterpret_cast<const f64x2 *>(U + urow * ld + kb);
#pragma unroll
            for (int q = 0; q < 8; q++) ub[q] = pu[q] * keep;
        }
        auto tile_ptr = [&](int t) {
            const int item = t * 16 + r;
            return reinterpret_cast<const f64x2 *>(V + (int64_t)(item < n_items ? item : n_items - 1) * ld + kb);
        };
        {
            const f64x2 *pv = tile_ptr(t_begin);
#pragma unroll
            for (int q = 0; q < 8; q++) va[q] = pv[q];
        }
        for (int t = t_begin; t < t_end; t++) {
            if (t + 1 < t_end) {
                const f64x2 *pv = tile_ptr(t + 1);
#pragma unroll
                for (int q = 0; q < 8; q++) vn[q] = pv[q];
            }
            f64x4 acc;
            double *out = S_T + (int64_t)(t * 16) * b_pad + utile * 16;
            if (c == 0) {
                acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int row = h + 4 * q;
                    acc[q] = (t * 16 + row < n_items) ? out[(int64_t)row * b_pad + r] : 0.0;
                }
            }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[q].x, ub[q].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[q].y, ub[q].y, acc, 0, 0, 0);
            }
            // f64 C/D: col = lane&15 (user), row = (lane>>4) + 4*reg (item)
            if constexpr (!std::is_same<Epi, PlainScore>::value) {
                if (c == n_chunks - 1) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int item = t * 16 + h + 4 * q;
                        if (item < n_items) acc[q] = epi(acc[q], item, utile * 16 + r);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int row = h + 4 * q;
                if (t * 16 + row < n_items) out[(int64_t)row * b_pad + r] = acc[q];
            }
#pragma unroll
            for (int q = 0; q < 8; q++) va[q] = vn[q];
        }
    }
}

// ---- bf16: NM = ld / 16 MFMAs per tile; lane (r, h) holds columns 16 m + 8 h .. + 8 of its row for every slice m
// user b's row of Ub [b_pad][16 NM] (zero rows past n_b)
template <int NM>
__device__ __forceinline__ void load_user_bf16(const __bf16 *Ub, int b_pad, int b, int h, bf16x8 (&u)[NM]) {
    const int bl = b < b_pad ? b : b_pad - 1;
#pragma unroll
    for (int m = 0; m < NM; m++) u[m] = *reinterpret_cast<const bf16x8 *>(Ub + (int64_t)bl * (16 * NM) + 16 * m + 8 * h);
}
// item tile `tile` of Vb: whole 32-item tiles (zero pad rows) in fragment order (to_bf16_kernel<., true>), one KiB per slice
template <int NM>
__device__ __forceinline__ void load_tile_bf16(const __bf16 *Vb, int64_t tile, int lane, bf16x8 (&dst)[NM]) {
    const __bf16 *frag = Vb + ((tile * NM) * 64 + lane) * 8;
#pragma unroll
    for (int m = 0; m < NM; m++) dst[m] = *reinterpret_cast<const bf16x8 *>(frag + m * 512);
}
// The bf16 MFMA step -- NM x NU v_mfma_f32_32x32x16_bf16 from zero accumulators -- is three lines and stays in the two kernels' text:
// as a function taking the tile by reference it made the compiler keep an NM = 8 tile as ONE 64-element vector (shuffles to take the
// slices out: sample_max_bf16_kernel<8, 2> 178 registers for 152, three wavefronts per SIMD down to two).

// ---- accumulator register q of lane (r, h) holds item row cd_row(q, h) = 4 h + (q & 3) + 8 (q >> 2) of the tile: with
// base = (the tile's first item) + 4 h the lane's 16 items are lane_item(base, q), ascending in q
__device__ __forceinline__ int lane_item(int base, int q) { return base + (q & 3) + 8 * (q >> 2); }

// ---- the last, partial tile (items item0 .. item0 + 31 reach past the catalogue): its pad rows are not items -> -inf, so that
// they are neither maxima nor candidates.  The test for the tile is wave-uniform: whole tiles pay one scalar compare.
template <int NU>
__device__ __forceinline__ void pad_rows_to_neg_inf(int item0, int h, int n_items, f32x16 (&acc)[NU]) {
    if (item0 + 32 > n_items) {
        const int base = item0 + 4 * h;
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (lane_item(base, q) >= n_items) {
#pragma unroll
                for (int k = 0; k < NU; k++) acc[k][q] = -__builtin_huge_valf();
            }
    }
}

// ---- the fetch loop of the filter kernels: tiles t_begin, t_begin + t_step, ... < t_end (t_begin < t_end) through two operand
// buffers used alternately (no register copies): tile t from one while tile t + t_step loads into the other.
// The next tile is fetched UNCONDITIONALLY (past the end: the last tile again, unused).  Under `if (t + t_step < t_end)` the
// compiler cannot know at the merge how many loads are outstanding, assumes the fewest, and waits for the tile it has just
// requested together with the one it is about to use (s_waitcnt vmcnt(3..0) in front of the MFMAs): no software pipelining
// (round 6; the same finding as the BPR kernels' 64-bit flavour).  The group loops of the two sample_max kernels fetch the same
// way (there the buffer is copied: the next tile may belong to the wavefront's next group).
template <typename Buf, typename Load, typename Do>          // Buf: the operand array of one tile; load_tile(t, Buf &); do_tile(t, const Buf &)
__device__ __forceinline__ void stream_tiles(int t_begin, int t_step, int t_end, const Load &load_tile, const Do &do_tile) {
    Buf va, vb;
    load_tile(t_begin, va);
    int t = t_begin;
    while (true) {
        load_tile(t + t_step < t_end ? t + t_step : t_end - 1, vb);
        do_tile(t, va);
        t += t_step;
        if (t >= t_end) break;
        load_tile(t + t_step < t_end ? t + t_step : t_end - 1, va);
        do_tile(t, vb);
        t += t_step;
        if (t >= t_end) break;
    }
}

}  // namespace qrec
