// The evaluation's heap views: CPython's heapq on (score, id) tuples -- util/qmath.py:134-146 runs heapq.heapify /
// heapq.heapreplace and a stable descending sort -- over three places a heap can live: LDS columns (Heap), the lanes of one
// wavefront (LaneHeap), one 64-bit key per lane (KeyHeap).  Shared by the block route (eval_block.hip), the fused route
// (eval_fused.hip) and tools/ubench/exact_walk_probe.hip.
#pragma once
#include "common.h"

namespace qrec {

constexpr int kHeapThreads = 64;

template <typename T, int THREADS = kHeapThreads>
struct Heap {  // column-per-thread layout in LDS: element k of thread t at [k * THREADS + t]
    T *s;
    int32_t *id;
    int t;
    __device__ T S(int k) const { return s[k * THREADS + t]; }
    __device__ int32_t I(int k) const { return id[k * THREADS + t]; }
    __device__ void set(int k, T sv, int32_t iv) { s[k * THREADS + t] = sv; id[k * THREADS + t] = iv; }
};

// Python tuple order on (score, id)
template <typename T>
__device__ inline bool tuple_lt(T sa, int32_t ia, T sb, int32_t ib) {
    return (sa < sb) || (sa == sb && ia < ib);
}

// heapq._siftdown(heap, startpos, pos)   (H: any heap view with S(k), I(k), set(k, score, id))
template <typename H>
__device__ inline void sift_down(H &hp, int startpos, int pos) {
    const auto ns = hp.S(pos); const int32_t ni = hp.I(pos);
    while (pos > startpos) {
        const int parent = (pos - 1) >> 1;
        const auto ps = hp.S(parent); const int32_t pi = hp.I(parent);
        if (tuple_lt(ns, ni, ps, pi)) { hp.set(pos, ps, pi); pos = parent; continue; }
        break;
    }
    hp.set(pos, ns, ni);
}
// heapq._siftup(heap, pos): bubble the smaller child up to a leaf, then sift the item down
template <typename H>
__device__ inline void sift_up(H &hp, int n, int pos) {
    const int startpos = pos;
    const auto ns = hp.S(pos); const int32_t ni = hp.I(pos);
    int child = 2 * pos + 1;
    while (child < n) {
        const int right = child + 1;
        if (right < n && !tuple_lt(hp.S(child), hp.I(child), hp.S(right), hp.I(right))) child = right;
        hp.set(pos, hp.S(child), hp.I(child));
        pos = child;
        child = 2 * pos + 1;
    }
    hp.set(pos, ns, ni);
    sift_down(hp, startpos, pos);
}

// The first n entries in descending order by a stable insertion sort: on the score alone (list.sort(key=score, reverse=True) of
// util/qmath.py:146) or, BY_TUPLE, in Python's tuple order on (score, id)
template <bool BY_TUPLE, typename H>
__device__ inline void sort_desc(H &hp, int n) {
    for (int a = 1; a < n; a++) {
        const auto xs = hp.S(a); const int32_t xi = hp.I(a);
        int c = a - 1;
        while (c >= 0 && (BY_TUPLE ? tuple_lt(hp.S(c), hp.I(c), xs, xi) : hp.S(c) < xs)) { hp.set(c + 1, hp.S(c), hp.I(c)); c--; }
        hp.set(c + 1, xs, xi);
    }
}

// A heap of <= 64 entries spread over the lanes of one wavefront: entry k lives in lane k's registers and is read
// with v_readlane, written by a per-lane select (k is wave-uniform: every lane runs the same sift).  An update costs a few
// dozen cross-lane moves instead of lane 0 chasing LDS latencies behind a barrier.
template <typename T>
struct LaneHeap {
    T s;             // this lane's entry
    int32_t id;
    int lane;
    static __device__ int rl(int v, int k) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(k)); }
    __device__ T S(int k) const {
        if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, rl(__builtin_bit_cast(int, s), k));
        else {
            const unsigned long long b = __builtin_bit_cast(unsigned long long, s);
            const unsigned lo = (unsigned)rl((int)(unsigned)b, k), hi = (unsigned)rl((int)(unsigned)(b >> 32), k);
            return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
        }
    }
    __device__ int32_t I(int k) const { return rl(id, k); }
    __device__ void set(int k, T sv, int32_t iv) {          // k, sv, iv wave-uniform: lane k takes the value
        const bool me = lane == k;
        s = me ? sv : s; id = me ? iv : id;
    }
};

// rank of this lane's key among the 64 keys of the wavefront (how many are larger): 64 x (2 v_readlane, compare, add) -- no LDS
// round trips, no dependent shuffles
__device__ __forceinline__ int wave_rank_u64(unsigned long long key) {
    const int lo = (int)(unsigned)key, hi = (int)(unsigned)(key >> 32);
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        const unsigned long long o = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, j) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, j);
        rank += o > key ? 1 : 0;
    }
    return rank;
}
__device__ __forceinline__ unsigned long long wave_read_u64(unsigned long long key, int src) {
    const int s = __builtin_amdgcn_readfirstlane(src);
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), s) << 32) |
           (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, s);
}

// The same heap for fp32 scores as ONE 64-bit key per lane: (order-preserving image of the score) << 32 | id, so Python's tuple
// order on (score, id) is the unsigned order of the keys.  heapq._siftup(heap, pos) -- bubble the smaller child up to a leaf, then
// sift the item back down -- nets out to an insertion along the smaller-child path: the path's entries grow downwards (the
// subtree below pos is a heap), so the item passes exactly those smaller than itself, each moving up one level, and lands where
// the next one is larger.  Every lane finds its smaller child at once (two 64-bit cross-lane reads), the path is five chained
// v_readlane, and how far the item travels is one ballot: no loop, no branch (the level-by-level loop over the same data cost
// 0.75 us per root replacement, mostly VALU <-> SALU hand-offs; tools/ubench/exact_walk_probe.hip).
struct KeyHeap {
    unsigned long long key;      // this lane's entry (lanes >= k: unused)
    int lane, k;
    static __device__ unsigned long long make(float s, int32_t id) {
        unsigned u = __float_as_uint(s + 0.f);                     // -0 -> +0: Python compares them equal
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        return ((unsigned long long)u << 32) | (unsigned)id;
    }
    static __device__ float score_of(unsigned long long kk) {
        unsigned u = (unsigned)(kk >> 32);
        u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
        return __uint_as_float(u);
    }
    __device__ unsigned long long at(int i) const { return wave_read_u64(key, i); }
    __device__ void sift(int pos, unsigned long long item) {       // pos, item wave-uniform; heap[pos] is taken to hold `item`
        const int c1 = 2 * lane + 1, c2 = c1 + 1;
        const unsigned long long k1 = __shfl(key, c1 & 63, kWave), k2 = __shfl(key, c2 & 63, kWave);
        const bool right = c2 < k && !(k1 < k2);                   // heapq: the right child unless left < right
        const int sc = c1 < k ? (right ? c2 : c1) : lane;          // a leaf points at itself
        const unsigned long long ck = right ? k2 : k1;             // the smaller child's key
        // the smaller-child path from pos (k <= 64: at most five levels below the root); no branches, five chained v_readlane
        const int p0 = __builtin_amdgcn_readfirstlane(pos);
        const int p1 = __builtin_amdgcn_readlane(sc, p0), p2 = __builtin_amdgcn_readlane(sc, p1), p3 = __builtin_amdgcn_readlane(sc, p2);
        const int p4 = __builtin_amdgcn_readlane(sc, p3), p5 = __builtin_amdgcn_readlane(sc, p4);
        const int rel = (31 - __builtin_clz(lane + 1)) - (31 - __builtin_clz(p0 + 1));      // this lane's level below pos
        const int pl = rel == 0 ? p0 : rel == 1 ? p1 : rel == 2 ? p2 : rel == 3 ? p3 : rel == 4 ? p4 : rel == 5 ? p5 : -1;
        const bool on = pl == lane;                                // the path holds one node per level
        // the path's keys grow downwards: those below `item` are a prefix; each moves up one level, the item lands behind them
        const int f = __popcll(__ballot(on && rel >= 1 && key < item));
        key = on && rel < f ? ck : (on && rel == f ? item : key);
    }
};

// KeyHeap's final list.sort(key=score, reverse=True), stable: entry a's rank = how many entries beat it or tie it from the left.
// Lane a < k writes entry a at its rank of row b; entries k .. K-1 (fewer than K items exist) are (-1, 0).
template <typename T>
__device__ inline void write_sorted(const KeyHeap &kh, int64_t b, int K, int32_t *__restrict__ ids_out, T *__restrict__ scores_out) {
    const float mine = KeyHeap::score_of(kh.key);
    int rank = 0;
    for (int c = 0; c < kh.k; c++) {
        const float cs = KeyHeap::score_of(kh.at(c));
        rank += (cs > mine || (cs == mine && c < kh.lane)) ? 1 : 0;
    }
    if (kh.lane < kh.k) { ids_out[b * K + rank] = (int32_t)(unsigned)(kh.key & 0xffffffffu); scores_out[b * K + rank] = (T)mine; }
    for (int a = kh.k + kh.lane; a < K; a += 64) { ids_out[b * K + a] = -1; scores_out[b * K + a] = T(0); }
}

}  // namespace qrec
