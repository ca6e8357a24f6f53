// Full-rank evaluation, the BLOCK route: score every item for a batch of users, mask the user's rated items to 0, keep the N
// largest -- base/recommender.py:143-150, util/qmath.py:134-146.  Every dtype and shape can go this way; the fp32 fused route
// (eval_fused.hip) is held to it bit for bit and sends its flagged users through steps (1) and (2) here.
//
//   (1) score_kernel   S_T[item][b] = V[item] . U[user_ids[b]]       MFMA (the one GEMM on
//       the path): v_mfma_f32_32x32x2_f32 for fp32 tables, v_mfma_f64_16x16x4_f64 for the
//       fp64 tables of the numpy-path models.  A wavefront keeps its 32 (16) users' U
//       fragment in registers and streams item tiles; V (<= tens of MB) is L2/MALL resident.
//       The block is written TRANSPOSED (item-major) so that step (3) reads coalesced.
//       (qrec_score_topk_sigmoid_bias adds a sigmoid pass here; qrec_score_topk_sparse_row_sigmoid_bias fills the block from
//       the rated CSR instead; qrec_score_topk_form fills it with a rating class's fp64 ranking scores, rank_forms.hip.)
//   (2) mask_kernel    S_T[item][b] = 0 for the user's rated train items -- to ZERO, not -inf:
//       the reference lets rated items compete with negative scores (recommender.py:147-149).
//   (3) heap_topk_kernel   one lane per user walks the items in id order and keeps the
//       reference's min-heap of (score, id) tuples -- CPython heapq's exact sift order,
//       strict '>' replacement, stable descending sort -- so ties resolve exactly as in the
//       reference (bit-exact ids).  Per user this is 1 load + 1 compare per item; ~N ln(I/N)
//       heap updates.  From 8,192 items on, (3b) the sliced top-N does the same for the users without ties.
//
// Bytes: (1) writes I*B*s, reads V once per user tile from cache; (3) reads I*B*s.
// FLOPs: 2*B*I*d on the matrix pipe.
#include <type_traits>

#include "eval_heap.h"
#include "eval_tile.h"

using namespace qrec;

namespace {

// ---- (1) fp32: the tile pieces of eval_tile.h, one 64-column chunk at a time, accumulated across chunks through the output.
// The score of (item, user b) goes to S_T[item * b_pad + (b / 64) * upair_stride + (b % 64) * u_stride]: ScoreLayout
// (common.h) -- the plain [rows][b_pad] block here, user-major rows for the fused route's stage (D).
__global__ __launch_bounds__(256) void score_kernel_f32(
    const float *__restrict__ U, const float *__restrict__ V, int ld, int n_items, const int32_t *__restrict__ user_ids, int n_b, int b_pad,
    int item_tiles_per_wave, float *__restrict__ S_T, int64_t upair_stride, int64_t u_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int upair = blockIdx.x;                       // 64 users: two 32-user tiles
    const int b0 = upair * 64 + r, b1 = b0 + 32;
    const int64_t uid0 = user_ids[b0 < n_b ? b0 : n_b - 1], uid1 = user_ids[b1 < n_b ? b1 : n_b - 1];   // columns >= n_b are never read
    const int n_chunks = (ld + 63) / 64;                // 64 columns per chunk
    const int n_item_tiles = (n_items + 31) / 32;
    const int t_begin = (blockIdx.y * 4 + wave) * item_tiles_per_wave;
    int t_end = t_begin + item_tiles_per_wave;
    if (t_end > n_item_tiles) t_end = n_item_tiles;
    if (t_begin >= t_end) return;

    for (int c = 0; c < n_chunks; c++) {
        const F32Slots<1> slots(ld, h, c);
        f32x4 ua[1][8], ub[1][8], va[1][8], vn[1][8];
        slots.load_users(U + uid0 * ld, U + uid1 * ld, ua, ub);
        slots.load_item(item_row_clamped(V, t_begin * 32 + r, n_items, ld), va);
        for (int t = t_begin; t < t_end; t++) {
            // the next item tile's operands are requested before this tile's MFMAs
            if (t + 1 < t_end) slots.load_item(item_row_clamped(V, (t + 1) * 32 + r, n_items, ld), vn);
            f32x16 acc0, acc1;
            float *out = S_T + (int64_t)(t * 32) * b_pad + upair * upair_stride;
            const int item0 = t * 32;
            auto cell = [&](int q) { return out + (int64_t)cd_row(q, h) * b_pad + r * u_stride; };      // user r; user 32 + r: 32 strides on
            if (c == 0) {
                zero(acc0); zero(acc1);
            } else {  // accumulate across column chunks through the output block
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    const bool in = item0 + cd_row(q, h) < n_items;
                    acc0[q] = in ? *cell(q) : 0.f;
                    acc1[q] = in ? cell(q)[32 * u_stride] : 0.f;
                }
            }
            mfma_f32(va, F32Chain<1>{ua, acc0}, F32Chain<1>{ub, acc1});
#pragma unroll
            for (int q = 0; q < 16; q++)
                if (item0 + cd_row(q, h) < n_items) { *cell(q) = acc0[q]; cell(q)[32 * u_stride] = acc1[q]; }
#pragma unroll
            for (int q = 0; q < 8; q++) va[0][q] = vn[0][q];
        }
    }
}

// ---- (1) fp64: the tile loop of eval_tile.h (score_tiles_f64: 16 items x 16 users per MFMA tile) with the identity epilogue, the
// user operand gathered through user_ids
__global__ __launch_bounds__(256) void score_kernel_f64(
    const double *__restrict__ U, const double *__restrict__ V, int ld, int n_items, const int32_t *__restrict__ user_ids, int n_b, int b_pad,
    int item_tiles_per_wave, double *__restrict__ S_T) {
    const int b = blockIdx.x * 16 + (threadIdx.x & 15);
    const int64_t uid = user_ids[b < n_b ? b : n_b - 1];      // columns >= n_b are never read
    score_tiles_f64(U, uid, V, ld, n_items, b_pad, item_tiles_per_wave, S_T, PlainScore{});
}

// ---- (2) rated train items -> score 0
template <typename T>
__global__ __launch_bounds__(256) void mask_kernel(const int32_t *__restrict__ user_ids, int n_b, const int64_t *__restrict__ rated_indptr,
                                                   const int32_t *__restrict__ rated_items, int b_pad, T *__restrict__ S_T,
                                                   int64_t upair_stride, int64_t u_stride) {
    // one wavefront per user of the batch
    const int b = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (b >= n_b) return;
    const int uid = user_ids[b];
    const int64_t beg = rated_indptr[uid], end = rated_indptr[uid + 1];
    for (int64_t e = beg + (threadIdx.x & 63); e < end; e += 64)
        S_T[(int64_t)rated_items[e] * b_pad + (b >> 6) * upair_stride + (b & 63) * u_stride] = T(0);
}

// One lane streams items t .. t_end - 1 of a user's column: AHEAD loads in flight ahead of f(score, item) -- there is at most
// one wavefront per SIMD in these scans (a lane per user), so latency is hidden by depth, not by occupancy
template <int AHEAD, typename T, typename F>
__device__ __forceinline__ void scan_column(const T *col, int b_pad, int t, int t_end, const F &f) {
    for (; t + AHEAD <= t_end; t += AHEAD) {
        T v[AHEAD];
#pragma unroll
        for (int q = 0; q < AHEAD; q++) v[q] = col[(int64_t)(t + q) * b_pad];
#pragma unroll
        for (int q = 0; q < AHEAD; q++) f(v[q], t + q);
    }
    for (; t < t_end; t++) f(col[(int64_t)t * b_pad], t);
}

// ---- (3) the reference's heap top-K, one lane per user ------------------------------------
template <typename T>
__global__ __launch_bounds__(kHeapThreads) void heap_topk_kernel(const T *__restrict__ S_T, int n_items, int b_pad, int n_b, int K,
                                                                 int32_t *__restrict__ ids_out, T *__restrict__ scores_out,
                                                                 const int32_t *__restrict__ flags, const int32_t *__restrict__ n_flagged,
                                                                 int many) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *hs = reinterpret_cast<T *>(smem);
    int32_t *hi = reinterpret_cast<int32_t *>(smem + (size_t)K * kHeapThreads * sizeof(T));
    const int b = blockIdx.x * kHeapThreads + threadIdx.x;
    if (b >= n_b) return;
    // as the fallback of the sliced path: only when MANY users need the sequential emulation (then this coalesced
    // lane-per-user scan is the cheapest way), and only for those users
    if (flags && (*n_flagged <= many || !flags[b])) return;
    Heap<T> hp{hs, hi, (int)threadIdx.x};
    const T *col = S_T + b;
    const int k = K < n_items ? K : n_items;
    for (int t = 0; t < k; t++) hp.set(t, col[(int64_t)t * b_pad], t);
    for (int t = k / 2 - 1; t >= 0; t--) sift_up(hp, k, t);  // heapify
    T root = hp.S(0);
    // main scan: 32 (fp32) / 16 (fp64) loads in flight ahead of the (rarely taken) heap update
    scan_column<sizeof(T) == 4 ? 32 : 16>(col, b_pad, k, n_items, [&](T v, int t) {
        if (v > root) { hp.set(0, v, t); sift_up(hp, k, 0); root = hp.S(0); }
    });
    sort_desc<false>(hp, k);                                  // list.sort(key=score, reverse=True)
    for (int a = 0; a < k; a++) {
        ids_out[(int64_t)b * K + a] = hp.I(a);
        scores_out[(int64_t)b * K + a] = hp.S(a);
    }
    for (int a = k; a < K; a++) { ids_out[(int64_t)b * K + a] = -1; scores_out[(int64_t)b * K + a] = T(0); }
}

// ---- (3b) sliced top-N: the fast path ---------------------------------------------------------
// The lane-per-user scan above leaves half the chip idle (31,668 users = 495 wavefronts for 1,024 SIMDs) and is
// bound by the bytes one lane can keep in flight (0.95 TB/s).  The reference's heap result is history-dependent only
// through TIES: if a user's N+1 largest scores are pairwise distinct, find_k_largest returns exactly the N
// largest in descending order (every one of them enters the heap and stays; the stable sort has nothing to break).
// So: (a) group_max_kernel + threshold_kernel + filter_kernel -- two streaming passes: the (N+1)-th largest of 64
// per-range maxima is a threshold tau that the user's N+1 best all reach, and the second pass keeps the scores >= tau
// (tried before: a per-slice heap -- with 64 users per wavefront some lane updates its heap in almost every step of
// the warm-up, 6x the heap work of the single scan, 3.1 ms -- and the exact heap of a 2,048-item prefix as threshold,
// 1.5 ms of lane-per-user latency plus 400 survivors to merge); (b) merge_topk_kernel -- one
// lane per user builds the global top-(N+1) from the few dozen survivors (as a multiset of values
// it is exact whatever the ties), writes the N best, and FLAGS the user if two of the N+1 values are equal or a slice
// overflowed; (c) flagged users are redone with the exact
// sequential emulation: few of them -> one wavefront each (exact_wave_kernel: 64 items per step, ballot for the
// first item above the heap root, lane 0 runs heapq's sift), many -> the lane-per-user kernel above.
constexpr int kSlices = 16;

// (a1) per-user maxima over kGroups disjoint item ranges (pure streaming, kGroups lanes per user), then tau[b] = the
//      M-th largest of them: M DIFFERENT items reach tau, so the user's M best scores all do -- a valid threshold, and a
//      tight one (about 1.5 M items of 38 k survive it).
constexpr int kGroups = 64;
template <typename T>
__global__ __launch_bounds__(256) void group_max_kernel(const T *__restrict__ S_T, int n_items, int b_pad, int n_b,
                                                        int items_per_group, T *__restrict__ gmax) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x, grp = blockIdx.y;
    if (b >= n_b) return;
    const T *col = S_T + b;
    const int t0 = grp * items_per_group;
    int t1 = t0 + items_per_group;
    if (t1 > n_items) t1 = n_items;
    T best = col[(int64_t)t0 * b_pad];             // every group is non-empty (host guarantees)
    scan_column<sizeof(T) == 4 ? 16 : 8>(col, b_pad, t0 + 1, t1, [&](T v, int) { best = v > best ? v : best; });
    gmax[(int64_t)grp * b_pad + b] = best;
}
template <typename T>
__global__ __launch_bounds__(256) void fill_neg_inf_kernel(T *__restrict__ rows, int b_pad, int n_b) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_b) rows[(int64_t)blockIdx.y * b_pad + b] = -__builtin_huge_val();
}
template <typename T>
__global__ __launch_bounds__(256) void threshold_kernel(const T *__restrict__ gmax, int b_pad, int n_b, int M, T *__restrict__ tau) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_b) return;
    T v[kGroups];
#pragma unroll
    for (int g = 0; g < kGroups; g++) v[g] = gmax[(int64_t)g * b_pad + b];
    // M-th largest of kGroups values: M rounds of "take the maximum out"
    T th = T(0);
    for (int r = 0; r < M; r++) {
        int arg = 0;
        T best = v[0];
#pragma unroll
        for (int g = 1; g < kGroups; g++)
            if (v[g] > best) { best = v[g]; arg = g; }
        th = best;
#pragma unroll
        for (int g = 0; g < kGroups; g++)
            if (g == arg) v[g] = -__builtin_huge_val();
    }
    tau[b] = th;
}

// (a2) kSlices lanes per user stream the catalogue again: an item whose score reaches tau[b] is appended to the lane's
//      candidate rows (a handful per lane); more than kSliceCap of them (a plateau of ties at tau) overflows and sends
//      the user to the exact emulation.
constexpr int kSliceCap = 32;
template <typename T>
__global__ __launch_bounds__(256) void filter_kernel(const T *__restrict__ S_T, int n_items, int b_pad, int n_b,
                                                     int items_per_slice, const T *__restrict__ tau, T *__restrict__ cand_s,
                                                     int32_t *__restrict__ cand_i, int32_t *__restrict__ cand_n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x, slice = blockIdx.y;
    if (b >= n_b) return;
    const T *col = S_T + b;
    const T th = tau[b];
    const int t0 = slice * items_per_slice;
    int t1 = t0 + items_per_slice;
    if (t1 > n_items) t1 = n_items;
    const int64_t row0 = (int64_t)slice * kSliceCap;
    int cnt = 0;
    constexpr int kAhead = sizeof(T) == 4 ? 16 : 8;      // scan_column's loop, written out: through the helper this kernel took 4 more registers
    int t = t0;
    for (; t + kAhead <= t1; t += kAhead) {
        T v[kAhead];
#pragma unroll
        for (int q = 0; q < kAhead; q++) v[q] = col[(int64_t)(t + q) * b_pad];
#pragma unroll
        for (int q = 0; q < kAhead; q++)
            if (v[q] >= th) {
                if (cnt < kSliceCap) { cand_s[(row0 + cnt) * b_pad + b] = v[q]; cand_i[(row0 + cnt) * b_pad + b] = t + q; }
                cnt++;
            }
    }
    for (; t < t1; t++) {
        const T v = col[(int64_t)t * b_pad];
        if (v >= th) {
            if (cnt < kSliceCap) { cand_s[(row0 + cnt) * b_pad + b] = v; cand_i[(row0 + cnt) * b_pad + b] = t; }
            cnt++;
        }
    }
    cand_n[(int64_t)slice * b_pad + b] = cnt;
}

template <typename T>
__global__ __launch_bounds__(kHeapThreads) void merge_topk_kernel(const T *__restrict__ cand_s, const int32_t *__restrict__ cand_i,
                                                                  const int32_t *__restrict__ cand_n, int b_pad, int n_b, int K,
                                                                  int32_t *__restrict__ ids_out, T *__restrict__ scores_out,
                                                                  int32_t *__restrict__ flags, int32_t *__restrict__ n_flagged,
                                                                  int32_t *__restrict__ flagged_list) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = K + 1;
    T *hs = reinterpret_cast<T *>(smem);
    int32_t *hi = reinterpret_cast<int32_t *>(smem + (size_t)M * kHeapThreads * sizeof(T));
    const int b = blockIdx.x * kHeapThreads + threadIdx.x;
    if (b >= n_b) return;
    Heap<T> hp{hs, hi, (int)threadIdx.x};
    // at least M items reach tau, so (unless a slice overflowed) the survivors fill the heap
    int m = 0;
    T rs = T(0);
    int32_t ri = 0;
    bool tie = false;
    for (int sl = 0; sl < kSlices; sl++) {
        int n = cand_n[(int64_t)sl * b_pad + b];
        if (n > kSliceCap) { tie = true; n = kSliceCap; }          // overflow: a plateau at tau -> exact emulation
        const int64_t row0 = (int64_t)sl * kSliceCap;
        for (int c = 0; c < n; c++) {
            const T v = cand_s[(row0 + c) * b_pad + b];
            const int32_t id = cand_i[(row0 + c) * b_pad + b];
            if (m < M) {
                hp.set(m, v, id);
                if (++m == M) {
                    for (int a = M / 2 - 1; a >= 0; a--) sift_up(hp, M, a);
                    rs = hp.S(0); ri = hp.I(0);
                }
            } else if (tuple_lt(rs, ri, v, id)) {
                hp.set(0, v, id); sift_up(hp, M, 0); rs = hp.S(0); ri = hp.I(0);
            }
        }
    }
    if (m < M) {                                    // only possible after an overflow: pad, the user is flagged anyway
        tie = true;
        for (; m < M; m++) hp.set(m, -__builtin_huge_val(), -1);
    }
    sort_desc<true>(hp, M);                         // descending, tuple order
    for (int a = 1; a < M; a++) tie |= hp.S(a) == hp.S(a - 1);
    for (int a = 0; a < K; a++) {
        ids_out[(int64_t)b * K + a] = hp.I(a);
        scores_out[(int64_t)b * K + a] = hp.S(a);
    }
    flags[b] = tie ? 1 : 0;
    if (tie) flagged_list[atomicAdd(n_flagged, 1)] = b;
}

// Exact sequential emulation for ONE user per wavefront (the users merge_topk_kernel flagged, when they are few).
// Same algorithm as heap_topk_kernel, 64 items per step: every lane holds one score, a ballot finds the first lane
// whose score beats the heap root, lane 0 performs heapq's replace in LDS, the root is re-read and the remaining
// lanes of the step are tested again.  The user's scores are b_pad*sizeof(T) bytes apart (64 cache lines per step):
// fine for a handful of users, 16x read amplification if used for all -- hence the `many` gate.
template <typename T, bool REG>      // REG: K <= 64, the heap lives in the wavefront's registers (LaneHeap); else in LDS
__global__ __launch_bounds__(64) void exact_wave_kernel(const T *__restrict__ S_T, int n_items, int b_pad, int K,
                                                        const int32_t *__restrict__ n_flagged, const int32_t *__restrict__ flagged_list,
                                                        int many, int32_t *__restrict__ ids_out, T *__restrict__ scores_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nf = *n_flagged;
    if (nf > many || (int)blockIdx.x >= nf) return;
    const int b = flagged_list[blockIdx.x], lane = threadIdx.x;
    T *hs = reinterpret_cast<T *>(smem);                                       // heap of this wavefront: [K] scores, [K] ids
    int32_t *hi = reinterpret_cast<int32_t *>(smem + (size_t)K * sizeof(T));
    typename std::conditional<REG, LaneHeap<T>, Heap<T, 1>>::type hp;          // Heap<T, 1>: one heap per block
    constexpr bool KEYED = REG && sizeof(T) == 4;                 // fp32, K <= 64: the heap as one 64-bit key per lane
    KeyHeap kh;
    const T *col = S_T + b;
    const int k = K < n_items ? K : n_items;
    if constexpr (KEYED) {
        kh.lane = lane; kh.k = k;
        kh.key = lane < k ? KeyHeap::make((float)col[(int64_t)lane * b_pad], lane) : ~0ull;
        for (int t = k / 2 - 1; t >= 0; t--) kh.sift(t, kh.at(t));                 // heapq.heapify
    } else if constexpr (REG) {
        hp.s = lane < k ? col[(int64_t)lane * b_pad] : T(0); hp.id = lane; hp.lane = lane;
        for (int t = k / 2 - 1; t >= 0; t--) sift_up(hp, k, t);
    } else {
        hp.s = hs; hp.id = hi; hp.t = 0;
        for (int t = lane; t < k; t += 64) hp.set(t, col[(int64_t)t * b_pad], t);
        __syncthreads();
        if (lane == 0)
            for (int t = k / 2 - 1; t >= 0; t--) sift_up(hp, k, t);
        __syncthreads();
    }
    T root;
    if constexpr (KEYED) root = (T)KeyHeap::score_of(kh.at(0)); else root = hp.S(0);
    // One wavefront per user and nothing else on the SIMD: the walk is a chain of memory round trips unless the loads of many
    // steps are in flight.  Steps go in groups of kGroup: the next group's kGroup loads per lane are issued before the
    // current group is examined (8 steps ahead, shifted through registers, measured 0.65 us per step = 0.39 ms per user).
    constexpr int kGroup = 32;
    T cur[kGroup], nxt[kGroup];
    auto fetch = [&](int t0, T (&dst)[kGroup]) {
#pragma unroll
        for (int q = 0; q < kGroup; q++) { const int t = t0 + 64 * q + lane; dst[q] = t < n_items ? col[(int64_t)t * b_pad] : T(0); }
    };
    fetch(k, cur);
    for (int g0 = k; g0 < n_items; g0 += 64 * kGroup) {
        if (g0 + 64 * kGroup < n_items) fetch(g0 + 64 * kGroup, nxt);
#pragma unroll
        for (int q = 0; q < kGroup; q++) {
            const int t0 = g0 + 64 * q, t = t0 + lane;
            const T v = cur[q];
            bool live = t < n_items;
            while (true) {
                const unsigned long long mask = __ballot(live && v > root);
                if (!mask) break;
                const int first = __builtin_ctzll(mask);
                const T fv = __shfl(v, first, kWave);
                if constexpr (KEYED) {
                    kh.sift(0, KeyHeap::make((float)fv, t0 + first));                  // heapq.heapreplace
                    root = (T)KeyHeap::score_of(kh.at(0));
                } else if constexpr (REG) {
                    hp.set(0, fv, t0 + first); sift_up(hp, k, 0);
                    root = hp.S(0);
                } else {
                    if (lane == 0) { hp.set(0, fv, t0 + first); sift_up(hp, k, 0); }
                    __syncthreads();
                    root = hp.S(0);
                }
                live = live && lane > first;
            }
        }
#pragma unroll
        for (int q = 0; q < kGroup; q++) cur[q] = nxt[q];
    }
    if constexpr (KEYED) {
        write_sorted(kh, b, K, ids_out, scores_out);
    } else if constexpr (REG) {
        // list.sort(key=score, reverse=True), stable: entry a's rank = how many entries beat it or tie it from the left
        int rank = 0;
        for (int c = 0; c < k; c++) {
            const T cs = hp.S(c);
            rank += (cs > hp.s || (cs == hp.s && c < lane)) ? 1 : 0;
        }
        if (lane < k) { ids_out[(int64_t)b * K + rank] = hp.id; scores_out[(int64_t)b * K + rank] = hp.s; }
        for (int a = k + lane; a < K; a += 64) { ids_out[(int64_t)b * K + a] = -1; scores_out[(int64_t)b * K + a] = T(0); }
    } else {
        __syncthreads();
        if (lane == 0) sort_desc<false>(hp, k);         // list.sort(key=score, reverse=True)
        __syncthreads();
        for (int a = lane; a < K; a += 64) {
            ids_out[(int64_t)b * K + a] = a < k ? hp.I(a) : -1;
            scores_out[(int64_t)b * K + a] = a < k ? hp.S(a) : T(0);
        }
    }
}

// The block route's scratch: the transposed score block (items padded to the 32-item tile, users to 64), then what the sliced
// top-N keeps behind it.  Below 8,192 items only the block is touched; the size is the same either way.
template <typename T>
struct BlockWs {
    T *S_T, *gmax, *tau, *cand_s;
    int32_t *cand_i, *cand_n, *flags, *flagged_list, *n_flagged;
};
template <typename T>
BlockWs<T> block_layout(Carver &c, int n_items, int n_b) {
    const size_t b_pad = ((size_t)n_b + 63) / 64 * 64, rows = ((size_t)n_items + 31) / 32 * 32, cand_rows = (size_t)kSlices * kSliceCap;
    BlockWs<T> w;
    w.S_T = c.take<T>(rows * b_pad);                       // [rows][b_pad]
    w.gmax = c.take<T>(kGroups * b_pad);                   // group maxima [kGroups][b_pad]
    w.tau = c.take<T>(b_pad);
    w.cand_s = c.take<T>(cand_rows * b_pad);               // candidate rows [kSlices * kSliceCap][b_pad]: scores, ids
    w.cand_i = c.take<int32_t>(cand_rows * b_pad);
    w.cand_n = c.take<int32_t>(kSlices * b_pad);           // per-slice counts [kSlices][b_pad]
    w.flags = c.take<int32_t>(b_pad);
    w.flagged_list = c.take<int32_t>(b_pad);
    w.n_flagged = c.take<int32_t>(16);                     // one counter: 4 of these 64 bytes are used, the rest stays because the size is ABI
    return w;
}

template <typename T>
int launch_mask(const int32_t *user_ids, int n_b, const int64_t *rated_indptr, const int32_t *rated_items, T *S, ScoreLayout lay, hipStream_t st) {
    hipLaunchKernelGGL(mask_kernel<T>, dim3((unsigned)((n_b + 3) / 4)), dim3(256), 0, st, user_ids, n_b, rated_indptr, rated_items, lay.b_pad, S,
                       lay.upair_stride, lay.u_stride);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

template <typename T>
int run_block_topk(const void *U, const void *V, int ld, int n_items, const int32_t *user_ids,
                   int n_b, const int64_t *rated_indptr, const int32_t *rated_items, int K, void *scratch,
                   int32_t *ids_out, void *scores_out, hipStream_t st, const float *item_bias, const SparseRows *sparse,
                   const FormScore *form) {
    const int b_pad = (n_b + 63) / 64 * 64;
    const BlockWs<T> w = carve(scratch, block_layout<T>, n_items, n_b);
    T *S_T = w.S_T;
    if constexpr (sizeof(T) == 4) {
        if (sparse) {          // qrec_score_topk_sparse_row_sigmoid_bias: the block comes from the rated CSR, not from U V^T
            const int rc = score_block_sparse_rows(S_T, *sparse, n_items, user_ids, n_b, b_pad, st);
            if (rc != QREC_OK) return rc;
        } else {
            const int rc = launch_score_block_f32((const float *)U, (const float *)V, ld, n_items, user_ids, n_b, 8, S_T, plain_block(b_pad), st);
            if (rc != QREC_OK) return rc;
        }
        if (item_bias) {       // qrec_score_topk_sigmoid_bias: S = sigmoid(S + bias[item]) before the rated items are set to 0
            const int rc = score_block_sigmoid_bias(S_T, item_bias, n_items, b_pad, st);
            if (rc != QREC_OK) return rc;
        }
    } else if (form) {         // qrec_score_topk_form: the block holds one of the rating classes' ranking scores, not U V^T
        const int rc = score_block_form(S_T, *form, n_items, user_ids, n_b, b_pad, st);
        if (rc != QREC_OK) return rc;
    } else {
        int per_wave;
        const dim3 grid = score_grid(n_b, (n_items + 15) / 16, 16, 8, &per_wave);
        hipLaunchKernelGGL(score_kernel_f64, grid, dim3(256), 0, st, (const double *)U, (const double *)V, ld,
                           n_items, user_ids, n_b, b_pad, per_wave, S_T);
        QREC_LAUNCH_CHECK();
    }
    if (rated_indptr) {
        const int rc = launch_mask(user_ids, n_b, rated_indptr, rated_items, S_T, plain_block(b_pad), st);
        if (rc != QREC_OK) return rc;
    }
    const size_t lds = (size_t)K * kHeapThreads * (sizeof(T) + sizeof(int32_t));
    QREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&heap_topk_kernel<T>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned user_blocks = (unsigned)((n_b + kHeapThreads - 1) / kHeapThreads);
    const int M = K + 1;
    if (n_items < 8192 || M > kGroups) {   // short catalogue, or more candidates wanted than there are group maxima:
                                           // the sequential emulation for everybody
        hipLaunchKernelGGL(heap_topk_kernel<T>, dim3(user_blocks), dim3(kHeapThreads), lds, st, S_T, n_items, b_pad, n_b, K,
                           ids_out, (T *)scores_out, nullptr, nullptr, 0);
        QREC_LAUNCH_CHECK();
        return QREC_OK;
    }
    const int per_group = (n_items + kGroups - 1) / kGroups, n_groups_used = (n_items + per_group - 1) / per_group;
    const int per_slice = (n_items + kSlices - 1) / kSlices;
    QREC_HIP_CHECK(hipMemsetAsync(w.n_flagged, 0, sizeof(int32_t), st));
    const size_t lds_m = (size_t)M * kHeapThreads * (sizeof(T) + sizeof(int32_t));
    QREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&merge_topk_kernel<T>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_m));
    const unsigned lane_blocks = (unsigned)((n_b + 255) / 256);
    if (n_groups_used < kGroups)      // ranges past the end (n_items not a multiple): -inf maxima
        hipLaunchKernelGGL(fill_neg_inf_kernel<T>, dim3(lane_blocks, kGroups - n_groups_used), dim3(256), 0, st,
                           w.gmax + (size_t)n_groups_used * b_pad, b_pad, n_b);
    hipLaunchKernelGGL(group_max_kernel<T>, dim3(lane_blocks, (unsigned)n_groups_used), dim3(256), 0, st, S_T, n_items, b_pad, n_b,
                       per_group, w.gmax);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(threshold_kernel<T>, dim3(lane_blocks), dim3(256), 0, st, w.gmax, b_pad, n_b, M, w.tau);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(filter_kernel<T>, dim3(lane_blocks, kSlices), dim3(256), 0, st, S_T, n_items, b_pad, n_b, per_slice, w.tau,
                       w.cand_s, w.cand_i, w.cand_n);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(merge_topk_kernel<T>, dim3(user_blocks), dim3(kHeapThreads), lds_m, st, w.cand_s, w.cand_i, w.cand_n, b_pad, n_b, K,
                       ids_out, (T *)scores_out, w.flags, w.n_flagged, w.flagged_list);
    QREC_LAUNCH_CHECK();
    // users whose N+1 best scores are not pairwise distinct: exact emulation (device-side choice of the regime)
    const int many = n_b / 16 > 256 ? n_b / 16 : 256;
    const int wave_blocks = n_b < many ? n_b : many;
    if (K <= 64)
        hipLaunchKernelGGL((exact_wave_kernel<T, true>), dim3((unsigned)wave_blocks), dim3(64), 0, st, S_T,
                           n_items, b_pad, K, w.n_flagged, w.flagged_list, many, ids_out, (T *)scores_out);
    else
        hipLaunchKernelGGL((exact_wave_kernel<T, false>), dim3((unsigned)wave_blocks), dim3(64), (size_t)K * (sizeof(T) + sizeof(int32_t)), st, S_T,
                           n_items, b_pad, K, w.n_flagged, w.flagged_list, many, ids_out, (T *)scores_out);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(heap_topk_kernel<T>, dim3(user_blocks), dim3(kHeapThreads), lds, st, S_T, n_items, b_pad, n_b, K, ids_out,
                       (T *)scores_out, w.flags, w.n_flagged, many);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // namespace

namespace qrec {

// users per wavefront (UTILE) x item tiles per wavefront: enough waves to fill 256 CUs x 4 SIMDs a few times over, each streaming
// >= min_per_wave item tiles
dim3 score_grid(int n_b, int n_item_tiles, int UTILE, int min_per_wave, int *per_wave) {
    const int n_utiles = (n_b + UTILE - 1) / UTILE;
    const int splits = (4096 + n_utiles - 1) / n_utiles;    // item-range splits per user tile, in waves
    *per_wave = (n_item_tiles + splits - 1) / splits;
    if (*per_wave < min_per_wave) *per_wave = n_item_tiles < min_per_wave ? n_item_tiles : min_per_wave;
    const int waves_per_utile = (n_item_tiles + *per_wave - 1) / *per_wave;
    return dim3((unsigned)n_utiles, (unsigned)((waves_per_utile + 3) / 4));
}

int64_t block_path_bytes(int dtype, int n_items, int n_b) {
    return dtype == QREC_F64 ? layout_bytes(block_layout<double>, n_items, n_b) : layout_bytes(block_layout<float>, n_items, n_b);
}

int launch_score_block_f32(const float *U, const float *V, int ld, int n_items, const int32_t *user_ids, int n_b, int min_tiles_per_wave,
                           float *S, ScoreLayout lay, hipStream_t st) {
    int per_wave;
    const dim3 grid = score_grid(n_b, (n_items + 31) / 32, 64, min_tiles_per_wave, &per_wave);
    hipLaunchKernelGGL(score_kernel_f32, grid, dim3(256), 0, st, U, V, ld, n_items, user_ids, n_b, lay.b_pad, per_wave, S, lay.upair_stride,
                       lay.u_stride);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int launch_mask_block(const int32_t *user_ids, int n_b, const int64_t *rated_indptr, const int32_t *rated_items, float *S, ScoreLayout lay,
                      hipStream_t st) {
    return launch_mask(user_ids, n_b, rated_indptr, rated_items, S, lay, st);
}

int run_score_topk(int dtype, const void *U, const void *V, int ld, int n_items, const int32_t *user_ids, int n_b,
                   const int64_t *rated_indptr, const int32_t *rated_items, int K, void *scratch, int32_t *ids_out, void *scores_out,
                   hipStream_t st, const float *item_bias, const SparseRows *sparse, const FormScore *form) {
    return dtype == QREC_F64
               ? run_block_topk<double>(U, V, ld, n_items, user_ids, n_b, rated_indptr, rated_items, K, scratch, ids_out, scores_out, st,
                                        nullptr, nullptr, form)
               : run_block_topk<float>(U, V, ld, n_items, user_ids, n_b, rated_indptr, rated_items, K, scratch, ids_out, scores_out, st,
                                       item_bias, sparse, nullptr);
}

}  // namespace qrec
