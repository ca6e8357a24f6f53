// The exact walk for the fused route's flagged users (eval_fused.hip, stage (D)): util/qmath.py:134-146 run item by item on one
// user's fp32 scores, K <= 64.  A file of its own so that tools/ubench/exact_walk_probe.hip can compile the kernel alone
// (QREC_WALK_PROBE: phase stamps and counts).
//
// User-major rows: a block per user stages the user's row in
// LDS -- 156 KB at a time, all four wavefronts copying with 16-byte accesses, dozens of loads in flight (5 us) -- and its first
// wavefront walks it from there, eight steps tested at a time: late in the row almost no item beats the heap's root.
// Measured at 38,048 items (tools/ubench/exact_walk_probe.hip): exact_wave_kernel 154 us whether a step's 64 loads were 64 cache
// lines or one; this kernel with the level-by-level sift 130 us (walk 119 us for 160 root replacements); with KeyHeap's
// branch-free sift 100 us -- what is left is one wavefront's dependent instruction chain, ~0.3 us per replacement.
#pragma once
#include "eval_heap.h"

namespace qrec {
namespace {

constexpr int kWalkChunk = 39936;      // items per LDS stage
#ifdef QREC_WALK_PROBE                 // phase stamps (100 MHz wall clock) and counts per block
__device__ long long g_walk_probe[8 * 4096];
#define QREC_WP(slot, val) do { if (threadIdx.x == 0) g_walk_probe[blockIdx.x * 8 + (slot)] = (val); } while (0)
#else
#define QREC_WP(slot, val) do { } while (0)
#endif
__global__ __launch_bounds__(256) void exact_walk_lds_kernel(const float *__restrict__ rows, int64_t row_len, int n_items, int K,
                                                             int32_t *__restrict__ ids_out, float *__restrict__ scores_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *stage = reinterpret_cast<float *>(smem);
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *row = rows + (int64_t)b * row_len;               // row_len: a multiple of 32, rows 128-byte aligned
    const int k = K < n_items ? K : n_items;
    KeyHeap kh;
    kh.lane = lane; kh.k = k; kh.key = ~0ull;
    float root = 0.f;
    [[maybe_unused]] long long n_updates = 0, n_groups_hit = 0;
    QREC_WP(0, (long long)wall_clock64());
    for (int c0 = 0; c0 < n_items; c0 += kWalkChunk) {
        const int n = n_items - c0 < kWalkChunk ? n_items - c0 : kWalkChunk;
        __syncthreads();                                          // the previous stage has been walked
        for (int i = threadIdx.x * 4; i < n; i += 1024)           // the row is padded to whole tiles: the last vector may run into the pad
            *reinterpret_cast<f32x4 *>(stage + i) = *reinterpret_cast<const f32x4 *>(row + c0 + i);
        __syncthreads();
        if (wave != 0) continue;
        if (c0 == 0) QREC_WP(1, (long long)wall_clock64());
        int i0 = 0;
        if (c0 == 0) {                                            // heapq.heapify of the first k items (k <= 64 <= n)
            kh.key = lane < k ? KeyHeap::make(stage[lane], lane) : ~0ull;
            for (int t = k / 2 - 1; t >= 0; t--) kh.sift(t, kh.at(t));
            root = KeyHeap::score_of(kh.at(0));
            i0 = k;
            QREC_WP(2, (long long)wall_clock64());
        }
        constexpr int kAhead = 8;
        for (; i0 < n; i0 += 64 * kAhead) {
            float v[kAhead];
            bool any = false;
#pragma unroll
            for (int q = 0; q < kAhead; q++) {
                const int i = i0 + 64 * q + lane;
                v[q] = i < n ? stage[i] : -__builtin_huge_valf();
                any |= v[q] > root;
            }
            if (!__any(any)) continue;
#ifdef QREC_WALK_PROBE
            n_groups_hit++;
#endif
#pragma unroll
            for (int q = 0; q < kAhead; q++) {
                const int t0 = c0 + i0 + 64 * q;
                bool live = true;
                while (true) {
                    const unsigned long long mask = __ballot(live && v[q] > root);
                    if (!mask) break;
                    const int first = __builtin_ctzll(mask);
                    const float fv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[q]), first));
                    kh.sift(0, KeyHeap::make(fv, t0 + first));                     // heapq.heapreplace
                    root = KeyHeap::score_of(kh.at(0));
                    live = live && lane > first;
#ifdef QREC_WALK_PROBE
                    n_updates++;
#endif
                }
            }
        }
    }
    if (wave != 0) return;
    QREC_WP(3, (long long)wall_clock64()); QREC_WP(4, n_updates); QREC_WP(5, n_groups_hit);
    write_sorted(kh, b, K, ids_out, scores_out);
}

}  // namespace
}  // namespace qrec
