// BPR SGD on embedding rows: model/ranking/BPR.py:45-53 (+ sigmoid util/qmath.py:127-128).
//
//   x = P[u].Q[i] - P[u].Q[j];  s = 1/(1+exp(-x));  g = lr*(1-s)
//   P[u] += g*(Q[i]-Q[j]);  Q[i] += g*P[u];  Q[j] -= g*P[u]      (P[u] already updated)
//   P[u] -= lr*regU*P[u];   Q[i] -= lr*regI*Q[i];   Q[j] -= lr*regI*Q[j];   loss += -log(s)
//
// This file is the throughput mode, fp32 (the order-exact parity mode: bpr_ordered_kernel of sgd_walkers.hip, and
// bpr_exact.hip).  bpr_hogwild_kernel: HBM/L2-latency bound gather + scatter:
//    a group of LPR lanes (16 for d<=64: lane r holds columns r, r+16, r+32, r+48 of one
//    256-B row, 4 rows per wavefront) owns a chunk of consecutive triplets, keeps P[u] in
//    registers along the user run, and applies every row update as the exact per-sample
//    delta (atomic f32 add, so concurrent chunks never lose an update).  Index tiles are
//    staged through LDS per wavefront; dot products reduce inside the LPR-lane row.
//    Algorithmic bytes per triplet: 6*d*4 + 12.
// bpr_hogwild_item_kernel is the same step over an item-major visiting order (see the kernel).
#include <cmath>

#include <algorithm>

#include <cstring>
#include <rocprim/rocprim.hpp>

#include "lane_row.h"   // neg_log_sigmoid(float), nothing else: these kernels want the compiler's contraction

using namespace qrec;

namespace {

// ------------------------------------------------------------------------------------
// throughput kernel
// ------------------------------------------------------------------------------------
// Register layout: a group of LPR lanes owns one row of ld = LPR*E floats; lane r holds
// columns r, r+LPR, ..., r+(E-1)*LPR.  Every load / atomic instruction therefore touches
// one CONTIGUOUS 4*LPR-byte segment per group (64 B for d=64).  Measured on MI355X
// (tools/ubench/atomics.hip): the L2 atomic units retire ~1 dword/clk/channel when a
// request covers a contiguous 64-B segment, 4x less when the same dwords are strided by
// 16 B (the float4-per-lane layout) -- atomic cost is per request, not per byte.
constexpr int kMaxChunk = 64;
constexpr int64_t kBufLimit = (int64_t)1 << 32;   // a buffer descriptor addresses 32-bit byte offsets
// test hook (README switch table): QREC_FORCE_64BIT_ADDRESSING=1 sends tables of any size down the >= 4 GiB flavour (TabPtr), so that
// its parity tests and timings do not need a 4 GiB table
static inline bool force_64bit_addressing() { const char *e = getenv("QREC_FORCE_64BIT_ADDRESSING"); return e && e[0] == '1'; }

enum : int { LD_PLAIN = 0, LD_SC1 = 1 };
enum : int { UP_STORE = 0, UP_STORE_SC1 = 1, UP_ATOMIC = 2 };

template <int E> struct Row { float v[E]; };

// Row access of the throughput kernels, two flavours chosen by table size:
//   TabBuf  a buffer descriptor sized to the table (32-bit byte offsets, so < 4 GiB): out-of-range row ids are
//           dropped by the hardware bounds check instead of corrupting memory, and address arithmetic is one VALU op;
//   TabPtr  64-bit global addressing for tables of 4 GiB and more (measured 2-5% slower: tools/bench_configs.py).
// kPrefetchAlways: how the triplet loops issue the next triplet's row loads (see the item-major kernel)
struct TabBuf {
    static constexpr bool kPrefetchAlways = false;
    __amdgpu_buffer_rsrc_t rs;
    static __device__ inline TabBuf make(float *p, int64_t bytes) { return TabBuf{make_rsrc(p, (uint32_t)bytes)}; }
};
struct TabPtr {
    static constexpr bool kPrefetchAlways = true;
    float *base;
    static __device__ inline TabPtr make(float *p, int64_t) { return TabPtr{p}; }
};

template <int LPR, int E, int LOADP>
__device__ inline Row<E> hw_load_row(TabBuf t, int row, int r) {
    constexpr int aux = (LOADP == LD_SC1) ? kAuxSc1 : kAuxPlain;
    const uint32_t off = ((uint32_t)row * (uint32_t)(LPR * E) + (uint32_t)r) * 4u;
    Row<E> out;
#pragma unroll
    for (int e = 0; e < E; e++)
        out.v[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(t.rs, (int)(off + 4u * LPR * e), 0, aux));
    return out;
}
template <int LPR, int E, int LOADP>
__device__ inline Row<E> hw_load_row(TabPtr t, int row, int r) {
    const float *p = t.base + (int64_t)row * (LPR * E) + r;
    Row<E> out;
#pragma unroll
    for (int e = 0; e < E; e++) {
        if constexpr (LOADP == LD_SC1) out.v[e] = __hip_atomic_load(p + LPR * e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // global_load ... sc1
        else out.v[e] = p[LPR * e];
    }
    return out;
}

template <int LPR, int E, int UPD>
__device__ inline void hw_update_row(TabBuf t, int row, int r, const Row<E> &oldv, const Row<E> &newv) {
    const uint32_t off = ((uint32_t)row * (uint32_t)(LPR * E) + (uint32_t)r) * 4u;
#pragma unroll
    for (int e = 0; e < E; e++) {
        if constexpr (UPD == UP_ATOMIC) {
            // exact per-sample delta (new-old is exact when |delta| << |value|)
            __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(newv.v[e] - oldv.v[e], t.rs, (int)(off + 4u * LPR * e), 0, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, newv.v[e]), t.rs, (int)(off + 4u * LPR * e), 0,
                                                  UPD == UP_STORE_SC1 ? kAuxSc1 : kAuxPlain);
        }
    }
}
template <int LPR, int E, int UPD>
__device__ inline void hw_update_row(TabPtr t, int row, int r, const Row<E> &oldv, const Row<E> &newv) {
    float *p = t.base + (int64_t)row * (LPR * E) + r;
#pragma unroll
    for (int e = 0; e < E; e++) {
        if constexpr (UPD == UP_ATOMIC) (void)__hip_atomic_fetch_add(p + LPR * e, newv.v[e] - oldv.v[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if constexpr (UPD == UP_STORE_SC1) __hip_atomic_store(p + LPR * e, newv.v[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else p[LPR * e] = newv.v[e];
    }
}

// ---- fixed-point rows (QREC_HW_FIXED, item-major atomic-delta policy only) ----------------------------------------------------
// The L2 atomic units retire integer adds faster than float adds (tools/ubench/atomics4_u32.hip: the shipped stream alone, 64-byte
// requests, 0.462 against 0.571 ms).  During a launch a table element is int32 = rint(x * 2^26) (fixed_convert_in_kernel /
// epoch_close_kernel of reduce.hip convert around the SGD launch; the tables are fp32 at rest): range +-32, quantum 1.5e-8 = the fp32
// ulp at 0.25-0.5.  A row is loaded as integers and converted; every delta is rint(delta * 2^26) added with an integer atomic, and the
// copy a group forwards to its own next triplet is old_int + delta_int -- what memory holds when nobody else touched the row -- so a
// forwarded row and a re-read row are the same bits.  Nothing may wrap: a new value with |x| >= 16 (half the range is headroom for
// deltas in flight) or a NaN raises the driver's FAILED flag (kFailedFixed).  The scalar codec: common.h.
template <int E> struct RowI { int32_t v[E]; };

template <int E>
__device__ inline Row<E> fx_row_to_float(const RowI<E> &q) {
    Row<E> out;
#pragma unroll
    for (int e = 0; e < E; e++) out.v[e] = fx_to_float(q.v[e]);
    return out;
}

template <int LPR, int E, int LOADP>
__device__ inline RowI<E> fx_load_row(TabBuf t, int row, int r) {
    constexpr int aux = (LOADP == LD_SC1) ? kAuxSc1 : kAuxPlain;
    const uint32_t off = ((uint32_t)row * (uint32_t)(LPR * E) + (uint32_t)r) * 4u;
    RowI<E> out;
#pragma unroll
    for (int e = 0; e < E; e++) out.v[e] = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(t.rs, (int)(off + 4u * LPR * e), 0, aux);
    return out;
}
template <int LPR, int E, int LOADP>
__device__ inline RowI<E> fx_load_row(TabPtr t, int row, int r) {
    const int32_t *p = reinterpret_cast<const int32_t *>(t.base) + (int64_t)row * (LPR * E) + r;
    RowI<E> out;
#pragma unroll
    for (int e = 0; e < E; e++) {
        if constexpr (LOADP == LD_SC1) out.v[e] = __hip_atomic_load(p + LPR * e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else out.v[e] = p[LPR * e];
    }
    return out;
}
// delta = rint((newv - oldv) * 2^26), added atomically; returns it so that the caller can keep old_int + delta_int
template <int LPR, int E>
__device__ inline RowI<E> fx_add_row(TabBuf t, int row, int r, const Row<E> &oldv, const Row<E> &newv) {
    const uint32_t off = ((uint32_t)row * (uint32_t)(LPR * E) + (uint32_t)r) * 4u;
    RowI<E> dlt;
#pragma unroll
    for (int e = 0; e < E; e++) {
        dlt.v[e] = fx_from_float(newv.v[e] - oldv.v[e]);
        (void)__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(dlt.v[e], t.rs, (int)(off + 4u * LPR * e), 0, 0);
    }
    return dlt;
}
template <int LPR, int E>
__device__ inline RowI<E> fx_add_row(TabPtr t, int row, int r, const Row<E> &oldv, const Row<E> &newv) {
    int32_t *p = reinterpret_cast<int32_t *>(t.base) + (int64_t)row * (LPR * E) + r;
    RowI<E> dlt;
#pragma unroll
    for (int e = 0; e < E; e++) {
        dlt.v[e] = fx_from_float(newv.v[e] - oldv.v[e]);
        (void)__hip_atomic_fetch_add(p + LPR * e, dlt.v[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return dlt;
}
// the range test as a running maximum of magnitude bits (common.h): folded per triplet, tested once per launch
template <int E>
__device__ inline uint32_t fx_row_mag(uint32_t mag, const Row<E> &x) {
#pragma unroll
    for (int e = 0; e < E; e++) mag = max(mag, fx_mag_bits(x.v[e]));
    return mag;
}

// Learning rate of a throughput epoch: either the host's value, or -- when `state` is given -- the device-resident
// bold-driver state written by epoch_close_kernel (reduce.hip; layout in include/qrec_hip.h), so that a whole
// training run can be enqueued without a host round trip per epoch.  A converged / failed run turns the
// remaining enqueued epochs into no-ops.
struct HwRate {
    float lr, regU, regI;
    double *state;      // read by every kernel; the fixed-point flavour also raises its FAILED flag
};
__device__ inline bool hw_rate_resolve(const HwRate &rt, float &lr, float &cu, float &ci) {
    lr = rt.lr;
    if (rt.state) {
        if (rt.state[QREC_DRV_CONVERGED] != 0.0 || rt.state[QREC_DRV_FAILED] != 0.0) return false;
        lr = (float)rt.state[QREC_DRV_LR];
    }
    cu = lr * rt.regU; ci = lr * rt.regI;
    return true;
}

template <int LPR, int E, int LOADP, int UPD, typename TAB>
__global__ __launch_bounds__(256) void bpr_hogwild_kernel(
    float *__restrict__ P, float *__restrict__ Q, int64_t p_bytes, int64_t q_bytes,
    const int32_t *__restrict__ u_idx, const int32_t *__restrict__ i_idx,
    const int32_t *__restrict__ j_idx, int64_t n, int chunk, int64_t n_chunks,
    int64_t groups_active, HwRate rate, double *__restrict__ loss_out) {
    constexpr int GPW = kWave / LPR;  // groups (rows) per wavefront
    float lr, cu, ci;
    if (!hw_rate_resolve(rate, lr, cu, ci)) return;
    __shared__ int32_t s_idx[4][GPW][3][kMaxChunk];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane / LPR, r = lane % LPR;
    const int64_t gid = ((int64_t)blockIdx.x * 4 + wave) * GPW + g;
    int32_t *su = s_idx[wave][g][0], *si = s_idx[wave][g][1], *sj = s_idx[wave][g][2];

    const TAB rsP = TAB::make(P, p_bytes), rsQ = TAB::make(Q, q_bytes);
    float loss = 0.f;
    double loss_acc = 0.0;

    for (int64_t c = gid; c < n_chunks && gid < groups_active; c += groups_active) {
        const int64_t t0 = c * chunk;
        const int len = (int)((n - t0) < chunk ? (n - t0) : chunk);
        // stage this group's (u,i,j) tile in LDS: coalesced 4*LPR-byte segments
        for (int k = r; k < len; k += LPR) {
            su[k] = u_idx[t0 + k]; si[k] = i_idx[t0 + k]; sj[k] = j_idx[t0 + k];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        int cur_u = -1, it = si[0], jt = sj[0];
        Row<E> pu, pu0;
#pragma unroll
        for (int e = 0; e < E; e++) pu.v[e] = pu0.v[e] = 0.f;
        Row<E> qi = hw_load_row<LPR, E, LOADP>(rsQ, it, r);
        Row<E> qj = hw_load_row<LPR, E, LOADP>(rsQ, jt, r);
        for (int k = 0; k < len; k++) {
            const int ut = su[k];
            if (ut != cur_u) {
                if (cur_u >= 0) hw_update_row<LPR, E, UPD>(rsP, cur_u, r, pu0, pu);
                pu = hw_load_row<LPR, E, LOADP>(rsP, ut, r);
                pu0 = pu; cur_u = ut;
            }
            // next triplet's rows are in flight under this one's math (the form of the prefetch per addressing flavour: see the item-major kernel)
            const bool more = (k + 1 < len);
            int in = it, jn = jt;
            Row<E> nqi = qi, nqj = qj;
            if (TAB::kPrefetchAlways || more) {
                const int kn = more ? k + 1 : k;
                in = si[kn]; jn = sj[kn];
                nqi = hw_load_row<LPR, E, LOADP>(rsQ, in, r);
                nqj = hw_load_row<LPR, E, LOADP>(rsQ, jn, r);
            }
            float di = 0.f, dj = 0.f;
#pragma unroll
            for (int e = 0; e < E; e++) { di += pu.v[e] * qi.v[e]; dj += pu.v[e] * qj.v[e]; }
            di = row_allreduce_sum<LPR>(di); dj = row_allreduce_sum<LPR>(dj);
            const float s = 1.0f / (1.0f + expf(-(di - dj)));
            const float gsc = lr * (1.0f - s);
            Row<E> qin, qjn;
#pragma unroll
            for (int e = 0; e < E; e++) {
                const float pun = pu.v[e] + gsc * (qi.v[e] - qj.v[e]);
                float a = qi.v[e] + gsc * pun, b = qj.v[e] - gsc * pun;
                qin.v[e] = a - ci * a; qjn.v[e] = b - ci * b;
                pu.v[e] = pun - cu * pun;
            }
            hw_update_row<LPR, E, UPD>(rsQ, it, r, qi, qin);
            hw_update_row<LPR, E, UPD>(rsQ, jt, r, qj, qjn);
            loss += neg_log_sigmoid(di - dj);
            if (more) {  // rows this group just changed supersede the prefetched copy
#pragma unroll
                for (int e = 0; e < E; e++) {
                    if (in == it) nqi.v[e] = qin.v[e]; else if (in == jt) nqi.v[e] = qjn.v[e];
                    if (jn == it) nqj.v[e] = qin.v[e]; else if (jn == jt) nqj.v[e] = qjn.v[e];
                }
            }
            qi = nqi; qj = nqj; it = in; jt = jn;
        }
        if (cur_u >= 0) hw_update_row<LPR, E, UPD>(rsP, cur_u, r, pu0, pu);
        loss_acc += (double)loss; loss = 0.f;  // <=64 fp32 terms per chunk, fp64 across chunks
        __builtin_amdgcn_wave_barrier();       // tile is re-staged by the next chunk
    }
    if (r != 0) loss_acc = 0.0;  // every lane of a group carries the same value
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) loss_acc += __shfl_xor(loss_acc, m, kWave);
    if (lane == 0 && loss_acc != 0.0) atomicAdd(loss_out, loss_acc);  // one f64 atomic per wavefront
}

// ------------------------------------------------------------------------------------
// Item-major schedule of the same Hogwild epoch.
// The triplets arrive sorted by positive item; a group keeps Q[i] in registers along an item run
// (exact chain on that row), and applies the per-sample deltas of P[u] and Q[j] atomically.
// Why: the atomic units serialise same-line requests.  In the user-major schedule the per-triplet
// atomics land on Q[i] ~ Zipf(0.6) (6.3k touches on the top item per epoch) and Q[j] ~ uniform:
// 3.8 G row-updates/s.  Item-major moves them to P[u] ~ Zipf(0.4) (max 1.35k) and Q[j]: 4.8 G/s,
// the uniform-address rate (tools/ubench/atomics3.hip).  Q[i] itself is flushed as one delta every
// `flush_every` triplets and re-read, so that concurrent runs of the same hot item see each other.
// Chunk c of the item-major list is executed at time slot s with c = (s * stride) mod n_chunks
// (stride coprime to n_chunks, ~0.618 n_chunks), which spreads the ~200 chunks of a hot item over
// the whole epoch instead of running them all at once.
// ------------------------------------------------------------------------------------
// RMW (round 6; bit 0: P[u], bit 1: Q[j]): the row is updated by an sc1 load + an sc1 write-through STORE of the new value instead of
// an atomic delta -- no atomic unit involved, and an update of the same row that lands between this group's load and its store is
// LOST (racy Hogwild).  Measured (tools/probe_item_rmw.py, profiles/r06_item_rmw.json): with P[u] by RMW the Yelp2018-shape epoch
// takes 0.376 ms instead of 0.569 (0.64 of the roofline instead of 0.43) and the HBM-resident slice 15.3 ms instead of 20.9 (0.63
// instead of 0.46); Q[j] by RMW as well adds 1 %.  What it costs is a function of the COLLISION DENSITY c = groups in flight x
// sum_u p_u^2 (the expected number of other groups working on the same user while one holds it): c = 0.008 (650 k users): paired
// Recall@20 gaps equal to the atomic kernel's; c = 0.033 (160 k users): inside the bar, visibly worse (0.0010 vs 0.0001); c = 0.17
// (Yelp2018 shape): inside on the planted-community graph with a 10 % loss gap; lastfm under BPR.conf (1.9 k users): -0.019, far outside.
// So the host selects it by c (engine.resolve_p_update: c <= 0.01), never by shape; bit 1 (Q[j]) is kept for measurements only.
// FIX: the fixed-point rows above (atomic-delta policy only, RMW == 0; needs the device-side driver state).
template <int LPR, int E, typename TAB, int RMW = 0, bool FIX = false>
__global__ __launch_bounds__(256) void bpr_hogwild_item_kernel(
    float *__restrict__ P, float *__restrict__ Q, int64_t p_bytes, int64_t q_bytes,
    const int32_t *__restrict__ u_idx, const int32_t *__restrict__ i_idx,
    const int32_t *__restrict__ j_idx, int64_t n, int chunk, int64_t n_chunks, int64_t chunk_stride,
    int64_t groups_active, int flush_every, HwRate rate, double *__restrict__ loss_out) {
    constexpr int GPW = kWave / LPR;
    float lr, cu, ci;
    static_assert(!FIX || RMW == 0, "fixed-point rows: atomic-delta policy only");
    if (!hw_rate_resolve(rate, lr, cu, ci)) return;
    __shared__ int32_t s_idx[4][GPW][3][kMaxChunk];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane / LPR, r = lane % LPR;
    const int64_t gid = ((int64_t)blockIdx.x * 4 + wave) * GPW + g;
    int32_t *su = s_idx[wave][g][0], *si = s_idx[wave][g][1], *sj = s_idx[wave][g][2];
    const TAB rsP = TAB::make(P, p_bytes), rsQ = TAB::make(Q, q_bytes);
    float loss = 0.f;
    double loss_acc = 0.0;
    [[maybe_unused]] uint32_t fx_mag = 0;

    for (int64_t slot = gid; slot < n_chunks && gid < groups_active; slot += groups_active) {
        const int64_t c = (int64_t)(((unsigned __int128)slot * (unsigned __int128)chunk_stride) % (unsigned __int128)n_chunks);
        const int64_t t0 = c * chunk;
        const int len = (int)((n - t0) < chunk ? (n - t0) : chunk);
        for (int k = r; k < len; k += LPR) { su[k] = u_idx[t0 + k]; si[k] = i_idx[t0 + k]; sj[k] = j_idx[t0 + k]; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        int cur_i = -1, since_flush = 0;
        Row<E> qi, qi0;
#pragma unroll
        for (int e = 0; e < E; e++) qi.v[e] = qi0.v[e] = 0.f;
        int ut = su[0], jt = sj[0];
        constexpr int LDP = (RMW & 1) ? LD_SC1 : LD_PLAIN, LDJ = (RMW & 2) ? LD_SC1 : LD_PLAIN;
        constexpr int UPP = (RMW & 1) ? UP_STORE_SC1 : UP_ATOMIC, UPJ = (RMW & 2) ? UP_STORE_SC1 : UP_ATOMIC;
        // FIX: the rows carried from triplet to triplet are the integers (pui, qji); they are converted where they are used, so that the
        // prefetch below stays in flight under the math exactly as the float rows do
        Row<E> pu, qj;
        [[maybe_unused]] RowI<E> pui, qji;
        if constexpr (FIX) { pui = fx_load_row<LPR, E, LDP>(rsP, ut, r); qji = fx_load_row<LPR, E, LDJ>(rsQ, jt, r); }
        else { pu = hw_load_row<LPR, E, LDP>(rsP, ut, r); qj = hw_load_row<LPR, E, LDJ>(rsQ, jt, r); }
        for (int k = 0; k < len; k++) {
            const int it = si[k];
            if (it != cur_i || since_flush >= flush_every) {
                if constexpr (FIX) {
                    if (cur_i >= 0) (void)fx_add_row<LPR, E>(rsQ, cur_i, r, qi0, qi);
                    qi = fx_row_to_float(fx_load_row<LPR, E, LD_SC1>(rsQ, it, r));
                } else {
                    if (cur_i >= 0) hw_update_row<LPR, E, UP_ATOMIC>(rsQ, cur_i, r, qi0, qi);
                    qi = hw_load_row<LPR, E, LD_SC1>(rsQ, it, r);      // bypass L1: pick up other runs' flushes
                }
                qi0 = qi; cur_i = it; since_flush = 0;
            }
            if constexpr (FIX) { pu = fx_row_to_float(pui); qj = fx_row_to_float(qji); }
            // The next triplet's rows go in flight under this one's math.  The 64-bit addressing flavour (TabPtr) issues them UNCONDITIONALLY
            // (the chunk's last triplet re-reads its own rows, unused): under `if (more)` its loads were if-converted into loads + selects,
            // the selects waited for the loads on the spot (s_waitcnt vmcnt(0) right behind the prefetch) and the software pipelining was
            // gone -- 168.9 instead of 120.5 ms on the 10 M-user HBM-resident slice with P[u] by load + store (round 6,
            // tools/probe_p_table_size.py).  The buffer-descriptor flavour keeps the branch: its loads stay behind a real skip, and the
            // unconditional form measured 11 % slower there (16.6 against 14.9 ms at 1.25 M users).
            const bool more = (k + 1 < len);
            int un = ut, jn = jt;
            Row<E> npu = pu, nqj = qj;
            [[maybe_unused]] RowI<E> npui, nqji;
            if constexpr (FIX) { npui = pui; nqji = qji; }
            if (TAB::kPrefetchAlways || more) {
                const int kn = more ? k + 1 : k;
                un = su[kn]; jn = sj[kn];
                if constexpr (FIX) { npui = fx_load_row<LPR, E, LDP>(rsP, un, r); nqji = fx_load_row<LPR, E, LDJ>(rsQ, jn, r); }
                else { npu = hw_load_row<LPR, E, LDP>(rsP, un, r); nqj = hw_load_row<LPR, E, LDJ>(rsQ, jn, r); }
            }
            float di = 0.f, dj = 0.f;
#pragma unroll
            for (int e = 0; e < E; e++) { di += pu.v[e] * qi.v[e]; dj += pu.v[e] * qj.v[e]; }
            di = row_allreduce_sum<LPR>(di); dj = row_allreduce_sum<LPR>(dj);
            const float s = 1.0f / (1.0f + expf(-(di - dj)));
            const float gsc = lr * (1.0f - s);
            Row<E> pun, qjn;
#pragma unroll
            for (int e = 0; e < E; e++) {
                const float p1 = pu.v[e] + gsc * (qi.v[e] - qj.v[e]);
                float a = qi.v[e] + gsc * p1, b = qj.v[e] - gsc * p1;
                qi.v[e] = a - ci * a; qjn.v[e] = b - ci * b;
                pun.v[e] = p1 - cu * p1;
            }
            if constexpr (FIX) {
                const RowI<E> dp = fx_add_row<LPR, E>(rsP, ut, r, pu, pun), dq = fx_add_row<LPR, E>(rsQ, jt, r, qj, qjn);
#pragma unroll
                for (int e = 0; e < E; e++) { pui.v[e] += dp.v[e]; qji.v[e] += dq.v[e]; }     // what memory holds now, this group alone
                fx_mag = fx_row_mag(fx_row_mag(fx_row_mag(fx_mag, pun), qjn), qi);
            } else {
                hw_update_row<LPR, E, UPP>(rsP, ut, r, pu, pun);
                hw_update_row<LPR, E, UPJ>(rsQ, jt, r, qj, qjn);
            }
            loss += neg_log_sigmoid(di - dj);
            since_flush++;
            if (more) {   // rows this group just changed supersede the prefetched copy
                // FIX: fx_from_float(qi) below serves the rare case jn == cur_i and is if-converted: 16 vector instructions per triplet under
                // an empty exec mask.  It stays that way.  Both ways of putting it behind a skip -- a branch on jn == cur_i around the whole
                // row, and a scalar branch on the wavefront's vote in front of this block -- made the compiler schedule selects right behind
                // the prefetch above, which then waits for its loads on the spot (s_waitcnt vmcnt(0..7) behind the loads) instead of under
                // the math: measured 2.31 against 2.47 G triplet-updates/s (profiles/bpr_wave_stream.json).
#pragma unroll
                for (int e = 0; e < E; e++) {
                    if constexpr (FIX) {
                        if (un == ut) npui.v[e] = pui.v[e];
                        if (jn == jt) nqji.v[e] = qji.v[e]; else if (jn == cur_i) nqji.v[e] = fx_from_float(qi.v[e]);
                    } else {
                        if (un == ut) npu.v[e] = pun.v[e];
                        if (jn == jt) nqj.v[e] = qjn.v[e]; else if (jn == cur_i) nqj.v[e] = qi.v[e];
                    }
                }
            }
            if constexpr (FIX) { pui = npui; qji = nqji; }
            else { pu = npu; qj = nqj; }
            ut = un; jt = jn;
        }
        if constexpr (FIX) { if (cur_i >= 0) (void)fx_add_row<LPR, E>(rsQ, cur_i, r, qi0, qi); }
        else { if (cur_i >= 0) hw_update_row<LPR, E, UP_ATOMIC>(rsQ, cur_i, r, qi0, qi); }
        loss_acc += (double)loss; loss = 0.f;
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (FIX) {
        if (fx_mag_out_of_range(fx_mag)) rate.state[QREC_DRV_FAILED] = kFailedFixed;       // a plain vector store; every writer writes the same value
    }
    if (r != 0) loss_acc = 0.0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) loss_acc += __shfl_xor(loss_acc, m, kWave);
    if (lane == 0 && loss_acc != 0.0) atomicAdd(loss_out, loss_acc);
}

template <int LPR, int E>
int launch_hogwild_item(float *P, float *Q, int64_t pb, int64_t qb, const int32_t *u, const int32_t *i,
                        const int32_t *j, int64_t n, int chunk, int64_t groups, int flush_every, HwRate rate,
                        double *loss, int variant, hipStream_t st) {
    constexpr int GPW = kWave / LPR;
    const int64_t n_chunks = (n + chunk - 1) / chunk;
    const int64_t default_groups = (int64_t)256 * 4 * GPW, max_groups = (int64_t)256 * 8 * 4 * GPW;
    if (groups <= 0) groups = default_groups;
    if (groups > max_groups) groups = max_groups;
    if (groups > n_chunks) groups = n_chunks;
    // stride ~ 0.618 n_chunks, made coprime with n_chunks: consecutive time slots visit far-apart chunks
    int64_t stride = (int64_t)((double)n_chunks * 0.6180339887498949);
    if (stride < 1) stride = 1;
    auto gcd = [](int64_t a, int64_t b) { while (b) { int64_t t = a % b; a = b; b = t; } return a; };
    while (gcd(stride, n_chunks) != 1) stride++;
    const unsigned blocks = (unsigned)((groups + 4 * GPW - 1) / (4 * GPW));
#define QREC_ITEM_LAUNCH(RMW, FIX)                                                                                                   \
    do {                                                                                                                          \
        if (pb < kBufLimit && qb < kBufLimit && !force_64bit_addressing())                                                        \
            hipLaunchKernelGGL((bpr_hogwild_item_kernel<LPR, E, TabBuf, RMW, FIX>), dim3(blocks), dim3(256), 0, st, P, Q, pb, qb, u, i, j, n, \
                               chunk, n_chunks, stride, groups, flush_every, rate, loss);                                         \
        else                                                                                                                      \
            hipLaunchKernelGGL((bpr_hogwild_item_kernel<LPR, E, TabPtr, RMW, FIX>), dim3(blocks), dim3(256), 0, st, P, Q, pb, qb, u, i, j, n, \
                               chunk, n_chunks, stride, groups, flush_every, rate, loss);                                         \
    } while (0)
    switch (variant) {
        case QREC_HW_DEFAULT:
        case QREC_HW_ATOMIC: QREC_ITEM_LAUNCH(0, false); break;
        case QREC_HW_P_RMW: QREC_ITEM_LAUNCH(1, false); break;
        case QREC_HW_PQ_RMW: QREC_ITEM_LAUNCH(3, false); break;
        case QREC_HW_FIXED:
            if (!rate.state) { set_error("qrec_bpr_sgd_hogwild_item_major: QREC_HW_FIXED needs d_driver_state"); return QREC_ERR_INVALID; }
            QREC_ITEM_LAUNCH(0, true);
            break;
        default: set_error("qrec_bpr_sgd_hogwild_item_major: unknown variant %d", variant); return QREC_ERR_INVALID;
    }
#undef QREC_ITEM_LAUNCH
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

template <int LPR, int E>
int launch_hogwild(float *P, float *Q, int64_t pb, int64_t qb, const int32_t *u,
                   const int32_t *i, const int32_t *j, int64_t n, int chunk, int64_t groups,
                   HwRate rate, double *loss, int variant, hipStream_t st) {
    constexpr int GPW = kWave / LPR;
    const int64_t n_chunks = (n + chunk - 1) / chunk;
    // Groups in flight.  The kernel is bound by the L2 atomic units, not by latency: measured at
    // the Yelp2018 shape, 4,096 groups (one 256-thread block per CU) already run at the full
    // 0.70 ms/epoch, and every extra group in flight only adds read staleness on hot rows
    // (deviation from the sequential result 0.11% at 4k groups vs 0.35% at 32k).  So the
    // default is one block per CU; callers may ask for more (up to 8 blocks per CU) or fewer.
    const int64_t default_groups = (int64_t)256 * 4 * GPW;
    const int64_t max_groups = (int64_t)256 * 8 * 4 * GPW;
    if (groups <= 0) groups = default_groups;
    if (groups > max_groups) groups = max_groups;
    if (groups > n_chunks) groups = n_chunks;
    const unsigned blocks = (unsigned)((groups + 4 * GPW - 1) / (4 * GPW));
#define QREC_HW_LAUNCH(LOADP, UPD)                                                                          \
    do {                                                                                                    \
        if (pb < kBufLimit && qb < kBufLimit && !force_64bit_addressing())                                  \
            hipLaunchKernelGGL((bpr_hogwild_kernel<LPR, E, LOADP, UPD, TabBuf>), dim3(blocks), dim3(256), 0, st, \
                               P, Q, pb, qb, u, i, j, n, chunk, n_chunks, groups, rate, loss);              \
        else                                                                                                \
            hipLaunchKernelGGL((bpr_hogwild_kernel<LPR, E, LOADP, UPD, TabPtr>), dim3(blocks), dim3(256), 0, st, \
                               P, Q, pb, qb, u, i, j, n, chunk, n_chunks, groups, rate, loss);              \
    } while (0)
    switch (variant) {
        case QREC_HW_PLAIN_RMW: QREC_HW_LAUNCH(LD_PLAIN, UP_STORE); break;
        case QREC_HW_SC1_RMW: QREC_HW_LAUNCH(LD_SC1, UP_STORE_SC1); break;
        case QREC_HW_DEFAULT:
        case QREC_HW_ATOMIC: QREC_HW_LAUNCH(LD_PLAIN, UP_ATOMIC); break;
        case QREC_HW_SC1_ATOMIC: QREC_HW_LAUNCH(LD_SC1, UP_ATOMIC); break;
        default: set_error("qrec_bpr_sgd_hogwild: unknown variant %d", variant); return QREC_ERR_INVALID;
    }
#undef QREC_HW_LAUNCH
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // namespace

extern "C" {

int qrec_bpr_sgd_hogwild(float *d_P, float *d_Q, int64_t n_users, int64_t n_items, int32_t d, int32_t ld, const int32_t *d_u,
                         const int32_t *d_i, const int32_t *d_j, int64_t n, int32_t chunk,
                         int32_t grid_groups, float lr, float regU, float regI, double *d_loss,
                         int variant, const double *d_driver_state, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_loss && n >= 0, "qrec_bpr_sgd_hogwild: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_j), "qrec_bpr_sgd_hogwild: null index array");
    QREC_REQUIRE(ld >= d && d >= 1, "qrec_bpr_sgd_hogwild: need ld >= d >= 1");
    QREC_REQUIRE(ld == 32 || ld == 64 || ld == 128 || ld == 256,
                 "qrec_bpr_sgd_hogwild: row stride must be 32, 64, 128 or 256 floats (pad d=%d up; got ld=%d)", d, ld);
    QREC_REQUIRE(chunk >= 1 && chunk <= kMaxChunk, "qrec_bpr_sgd_hogwild: chunk must be in 1..%d", kMaxChunk);
    if (n == 0) return QREC_OK;
    // tables below 4 GiB go through a buffer descriptor sized to the table (ids >= rows are dropped by the hardware
    // bounds check); larger ones through 64-bit addressing
    QREC_REQUIRE(n_users >= 1 && n_items >= 1, "qrec_bpr_sgd_hogwild: table row counts must be given");
    const int64_t full_p = n_users * (int64_t)ld * 4, full_q = n_items * (int64_t)ld * 4;
    hipStream_t st = as_stream(stream);
    const HwRate rate{lr, regU, regI, const_cast<double *>(d_driver_state)};
    switch (ld) {
        case 32: return launch_hogwild<16, 2>(d_P, d_Q, full_p, full_q, d_u, d_i, d_j, n, chunk, grid_groups, rate, d_loss, variant, st);
        case 64: return launch_hogwild<16, 4>(d_P, d_Q, full_p, full_q, d_u, d_i, d_j, n, chunk, grid_groups, rate, d_loss, variant, st);
        case 128: return launch_hogwild<32, 4>(d_P, d_Q, full_p, full_q, d_u, d_i, d_j, n, chunk, grid_groups, rate, d_loss, variant, st);
        default: return launch_hogwild<64, 4>(d_P, d_Q, full_p, full_q, d_u, d_i, d_j, n, chunk, grid_groups, rate, d_loss, variant, st);
    }
}

int qrec_bpr_sgd_hogwild_item_major(float *d_P, float *d_Q, int64_t n_users, int64_t n_items, int32_t d, int32_t ld,
                                    const int32_t *d_u,
                                    const int32_t *d_i, const int32_t *d_j, int64_t n, int32_t chunk,
                                    int32_t grid_groups, int32_t flush_every, float lr, float regU, float regI,
                                    double *d_loss, int variant, const double *d_driver_state, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_loss && n >= 0, "qrec_bpr_sgd_hogwild_item_major: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_j), "qrec_bpr_sgd_hogwild_item_major: null index array");
    QREC_REQUIRE(ld >= d && d >= 1, "qrec_bpr_sgd_hogwild_item_major: need ld >= d >= 1");
    QREC_REQUIRE(ld == 32 || ld == 64 || ld == 128 || ld == 256,
                 "qrec_bpr_sgd_hogwild_item_major: row stride must be 32, 64, 128 or 256 floats (got ld=%d)", ld);
    QREC_REQUIRE(chunk >= 1 && chunk <= kMaxChunk && flush_every >= 1, "qrec_bpr_sgd_hogwild_item_major: bad chunk / flush interval");
    if (n == 0) return QREC_OK;
    QREC_REQUIRE(n_users >= 1 && n_items >= 1, "qrec_bpr_sgd_hogwild_item_major: table row counts must be given");
    const int64_t full_p = n_users * (int64_t)ld * 4, full_q = n_items * (int64_t)ld * 4;
    hipStream_t st = as_stream(stream);
    const HwRate rate{lr, regU, regI, const_cast<double *>(d_driver_state)};
    switch (ld) {
        case 32: return launch_hogwild_item<16, 2>(d_P, d_Q, full_p, full_q, d_u, d_i, d_j, n, chunk, grid_groups, flush_every, rate, d_loss, variant, st);
        case 64: return launch_hogwild_item<16, 4>(d_P, d_Q, full_p, full_q, d_u, d_i, d_j, n, chunk, grid_groups, flush_every, rate, d_loss, variant, st);
        case 128: return launch_hogwild_item<32, 4>(d_P, d_Q, full_p, full_q, d_u, d_i, d_j, n, chunk, grid_groups, flush_every, rate, d_loss, variant, st);
        default: return launch_hogwild_item<64, 4>(d_P, d_Q, full_p, full_q, d_u, d_i, d_j, n, chunk, grid_groups, flush_every, rate, d_loss, variant, st);
    }
}

}  // extern "C"
