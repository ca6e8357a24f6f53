// Full-rank evaluation, the FUSED route (fp32, ld <= 128, N + 1 <= 64, >= 16,384 items): score -> mask -> threshold filter in one
// pass, no B x I block.  base/recommender.py:143-150 + util/qmath.py:134-146 again, for the common case that a user's N+1 best
// scores are pairwise distinct (then find_k_largest returns exactly the N best, descending):
//   (A) threshold: score every kSampleStride-th item tile only (bf16 route: every tile, at 1/16 of the matrix-pipe time), keep
//       per range of tiles the largest score and its item, and take tau[b] = the (N+1)-th largest of those range maxima whose
//       item the user has not rated -- N+1 DIFFERENT unrated items reach tau, so the user's N+1 best do;
//       about (N+1) x kSampleStride x 1.1 items of the whole catalogue reach it;
//   (B) score_filter2_kernel_f32: the scoring kernel with the store replaced by a compare against tau in the MFMA
//       accumulators; an item that reaches tau is appended to the lane's private candidate list.  Nothing else is
//       written: the kernel is bound by the matrix pipe.  (Rated items are NOT looked up here: a bisection per hit in
//       the epilogue -- six dependent loads under divergence -- cost 2x the tile's MFMA time, measured 3.6 ms.)
//       (B') by default the same pass on bf16 copies against a lowered threshold, the survivors re-scored in fp32 by (C);
//   (C) select_topk_kernel: one wavefront per user gathers the user's candidates (a few hundred), drops the user's
//       rated items (they count as 0 < tau; bisection, all lanes in parallel) and extracts the N+1 largest by repeated
//       wave-wide maximum; equal scores among them, an overflowed list or tau <= 0 (rated items, masked to 0, would
//       compete) flag the user;
//   (D) flagged users -- the cases where the heap's history matters -- get the block route's MFMA scores and mask (eval_block.hip,
//       through launch_score_block_f32 / launch_mask_block) as user-major rows and the exact heap emulation (eval_walk.h), a few
//       hundred at a time, and their rows are patched in.
// tests/test_gpu_eval.py holds every variant of this route to the block route bit for bit.
#include <cstdlib>

#include "eval_heap.h"
#include "eval_tile.h"
#include "eval_walk.h"

using namespace qrec;

namespace {

constexpr int kSampleStride = 8;
constexpr int kListCap = 48;        // candidates per lane-private list (expected ~10)
constexpr int kMaxGroups = 128;     // range maxima per user in (A)
constexpr int kSelectMax = 64;      // K + 1 <= 64: the walk's KeyHeap and the selection's one-key-per-lane ranks
constexpr int kSelectWaves = 4;

// ---- geometry and scratch ------------------------------------------------------------------------------------------------
struct FusedGeom {
    int b_pad, n_item_tiles, grid_x, grid_y, n_lists, list_cap, nu, n_s_tiles, fb_users;
    bool use_bf16;
};
FusedGeom fused_geometry(int n_items, int n_b, int ld) {
    FusedGeom g;
    g.b_pad = (n_b + 63) / 64 * 64;
    g.n_item_tiles = (n_items + 31) / 32;
    // the bf16 route (default): NU user tiles of 32 per wavefront, short candidate lists (its threshold comes from the whole
    // catalogue: a few dozen candidates per user); the fp32 route (QREC_EVAL_F32_FILTER): two tiles, ~200 candidates per user
    const bool bf16_filter = getenv("QREC_EVAL_F32_FILTER") == nullptr;          // read per call: the tests switch routes in-process
    const int eval_nu = getenv("QREC_EVAL_NU") ? atoi(getenv("QREC_EVAL_NU")) : 4;
    g.use_bf16 = bf16_filter && (ld == 32 || ld == 64 || ld == 128);
    g.nu = g.use_bf16 ? (ld == 128 || (ld == 64 && eval_nu == 2) ? 2 : 4) : 2;
    g.list_cap = g.use_bf16 ? 16 : kListCap;
    g.grid_x = (n_b + 32 * g.nu - 1) / (32 * g.nu);
    int waves = ((g.use_bf16 ? 8192 : 4096) + g.grid_x - 1) / g.grid_x;   // wavefronts per user group: fill 1,024 SIMDs a few times over
    if (waves > g.n_item_tiles / 8) waves = g.n_item_tiles / 8 > 0 ? g.n_item_tiles / 8 : 1;
    if (waves > 32) waves = 32;              // <= 64 candidate lists per user: the selection kernel gathers them in LDS
    g.grid_y = (waves + 3) / 4;
    g.n_lists = g.grid_y * 4 * 2;
    g.n_s_tiles = (g.n_item_tiles + kSampleStride - 1) / kSampleStride;
    g.fb_users = (n_b / 16 > 256 ? n_b / 16 : 256);
    if (g.fb_users > n_b) g.fb_users = n_b;
    g.fb_users = (g.fb_users + 63) / 64 * 64;
    return g;
}

// The fused route's scratch.  Every array starts on a 256-byte boundary and so does the end; v_max and n_flagged are one element each.
struct FusedWs {
    __bf16 *Ub, *Vb;
    float *u_norm, *v_max, *tau_low, *gmax;
    int32_t *garg;
    float *tau, *cand_s;
    int32_t *cand_i, *cand_n, *flags, *flagged_list, *n_flagged, *fb_users, *fb_ids;
    float *fb_sc, *fb_block;
};
FusedWs fused_layout(Carver &c, const FusedGeom &g, int n_items, int ld) {
    const size_t b_pad = g.b_pad, cands = b_pad * g.n_lists * g.list_cap;
    FusedWs w;
    w.Ub = c.take<__bf16>(b_pad * ld, 256);                                   // bf16 copies of the batch's user rows and of the items
    w.Vb = c.take<__bf16>((size_t)g.n_item_tiles * 32 * ld, 256);
    w.u_norm = c.take<float>(b_pad, 256);
    w.v_max = c.take<float>(1, 256);
    w.tau_low = c.take<float>(b_pad, 256);
    w.gmax = c.take<float>(kMaxGroups * b_pad, 256);
    w.garg = c.take<int32_t>(kMaxGroups * b_pad, 256);
    w.tau = c.take<float>(b_pad, 256);
    w.cand_s = c.take<float>(cands, 256);
    w.cand_i = c.take<int32_t>(cands, 256);
    w.cand_n = c.take<int32_t>(b_pad * g.n_lists, 256);
    w.flags = c.take<int32_t>(b_pad, 256);
    w.flagged_list = c.take<int32_t>(b_pad, 256);
    w.n_flagged = c.take<int32_t>(1, 256);
    w.fb_users = c.take<int32_t>(g.fb_users, 256);                            // stage (D), fb_users flagged users at a time: their ids, lists
    w.fb_ids = c.take<int32_t>((size_t)g.fb_users * 100, 256);
    w.fb_sc = c.take<float>((size_t)g.fb_users * 100, 256);
    // ... and their scores, in a region the size of the block layout at fb_users (the size is ABI).  Stage (D) keeps user-major
    // [user][item] rows there: they fill exactly the layout's first array, the score block, and nothing behind it is used.
    w.fb_block = c.take<float>(block_path_bytes(QREC_F32, n_items, g.fb_users) / sizeof(float), 256);
    c.pad(256);
    return w;
}

// ld -> the template arguments of the kernels below, stated once.  fp32 scoring and the selection: NC column chunks of 64.
// bf16 kernels: NM MFMA steps of 16 columns and NU user tiles per wavefront (FusedGeom::nu: 4, or 2 at ld = 128 and under QREC_EVAL_NU=2).
template <typename F> void with_nc(int ld, F f) { if (ld <= 64) f(int_c<1>{}); else f(int_c<2>{}); }
template <typename F> void with_nm_nu(int ld, int nu, F f) {
    if (ld == 32) f(int_c<2>{}, int_c<4>{});
    else if (ld == 64) { if (nu == 2) f(int_c<4>{}, int_c<2>{}); else f(int_c<4>{}, int_c<4>{}); }
    else f(int_c<8>{}, int_c<2>{});
}

// ---- the bf16 copies ---------------------------------------------------------------------------------------------------------
// (B') the scoring pass as a bf16 FILTER.
// The pass only has to find every item whose fp32 score reaches tau; the scores themselves are re-formed afterwards (select
// kernel, the SAME fp32 MFMA sequence as score_kernel_f32, so ids and scores stay bit-identical to the block route).  So it
// runs on bf16 copies of the two tables -- v_mfma_f32_32x32x16_bf16: 1/16 of the matrix-pipe time of the f32 form, half the
// operand bytes -- against a threshold lowered by a bound on what the rounding can cost a score:
//   u^ = u (1 + d), |d| <= 2^-8 (round to nearest, 8-bit significand), same for v  =>  |u^.v^ - u.v| <= (2^-7 + 2^-16) sum |u_k v_k|
//   <= (2^-7 + 2^-16) |u| |v|;  the fp32 accumulation inside the MFMAs adds < 64 * 2^-24 of the same sum.
// eps[b] = 2^-7 * 1.02 * |u_b| * max_items |v| -- every item with u.v >= tau has u^.v^ >= tau - eps.
// The budget behind the 2 %, in units of |u| |v|: the bound proper is 2^-7 = 7.8125e-3 and the slack 0.02 * 2^-7 = 1.56e-4; it
// has to hold (i) the cross term 2^-16 = 1.5e-5, (ii) the fp32 accumulation inside and between the MFMAs, d/16 steps of
// 2^-24 each on the running sum: <= 128 * 2^-24 = 7.6e-6 up to d = 128 -- whatever order the matrix pipe adds in, each partial
// sum is bounded by sum |u^_k v^_k|, (iii) the candidate lists' 4-bit score tag (selection compares re-formed fp32 scores, the
// tag only orders the bf16 ones inside a list: 15 ulp of fp32 = 1.8e-6 relative), (iv) the norms' own rounding, covered by their
// factor 1.0001 (to_bf16_kernel).  Sum ~ 2.5e-5, a sixth of the slack.  tests/test_eval_bf16_bound.py checks the inequality
// numerically on the CPU; tests/test_gpu_eval.py::test_bf16_filter_is_complete_on_adversarial_tables holds the hardware's own
// accumulation to it (item and user norms over six decades, cancelling coordinates, clusters of near-ties at the threshold).
// Non-finite tables (a diverged run -- the reference stops such a run at the loss check, iterativeRecommender.py:84-86, before
// any evaluation): a norm is inf/NaN, tau_low = tau - inf/NaN admits nothing or everything, the user's lists come back empty or
// overflowed and the select kernel flags the user for the exact walk -- slow, not wrong.
//
// rows [rows][ld] fp32 (row_ids: gather, may be null) -> bf16 copy [rows][ld]; norm[row] = |x| (fp32); pad rows (>= rows) zero.
// TILED (the item table): the copy is laid out in the order the MFMA loops fetch it -- 32-row tile t, 16-column slice m, then the
// 64 lanes' 16-byte operand fragments (lane (r, h): columns 16 m + 8 h .. + 8 of row 32 t + r) -- so that one global_load_dwordx4 of
// a wavefront reads ONE contiguous KiB (8 cache lines) instead of 32 bytes from each of 32 rows (32 lines): with the row-major copy
// the two bf16 passes kept the texture-address unit stalled on the L1 half of the time and waited 2,000 cycles for a tile they had
// requested a whole iteration earlier (round 6: TA_ADDR_STALLED_BY_TC, SQ_WAIT_ANY; the matrix pipe at 22 / 35 %)
template <int LPR, bool TILED>
__global__ __launch_bounds__(256) void to_bf16_kernel(const float *__restrict__ X, const int32_t *__restrict__ row_ids, int rows, int rows_pad,
                                                      __bf16 *__restrict__ out, float *__restrict__ norm, float *__restrict__ norm_max) {
    constexpr int GPW = kWave / LPR;
    const int lane = threadIdx.x & 63, g = lane / LPR, r = lane % LPR;
    const int64_t k = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GPW + g;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (k < rows) x = *reinterpret_cast<const f32x4 *>(X + (int64_t)(row_ids ? row_ids[k] : k) * (4 * LPR) + 4 * r);
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    bf16x4 o = {(__bf16)x.x, (__bf16)x.y, (__bf16)x.z, (__bf16)x.w};
    if (k < rows_pad) {
        if constexpr (TILED) {
            constexpr int NM = LPR / 4;
            const int c = 4 * r;
            *reinterpret_cast<bf16x4 *>(out + ((((k >> 5) * NM + (c >> 4)) * 64 + ((c >> 3) & 1) * 32 + (k & 31)) << 3) + (c & 7)) = o;
        } else {
            *reinterpret_cast<bf16x4 *>(out + k * (4 * LPR) + 4 * r) = o;
        }
    }
    float ss = x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
    ss = row_allreduce_sum<LPR>(ss);
    float nrm = sqrtf(ss) * 1.0001f;                               // rows past `rows`: 0
    if (r == 0 && norm && k < rows_pad) norm[k] = nrm;
    if (norm_max) {                                                // one atomic per block (one per row serialises: 110 us for 38,048 rows)
        __shared__ float s_max[4];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nrm = fmaxf(nrm, __shfl_xor(nrm, m, kWave));
        if (lane == 0) s_max[threadIdx.x >> 6] = nrm;
        __syncthreads();
        if (threadIdx.x == 0)
            atomicMax(reinterpret_cast<int *>(norm_max), __float_as_int(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]))));   // non-negative floats order as ints
    }
}

// ---- (A) the threshold without a sampled score block -------------------------------------------------------------------------
// sample_max_kernel_f32: the scoring loop over every kSampleStride-th item tile, but nothing is stored: per GROUP of
// `tiles_per_group` consecutive sampled tiles every user keeps the largest (unmasked) score and its item.
// threshold_var_kernel: a group whose best item is one the user has rated is discarded -- the remaining maxima are
// scores of DISTINCT UNRATED items, so their (N+1)-th largest is a threshold the user's N+1 best masked scores reach.
// (First version: the sampled tiles written out as a 600 MB block, masked there, group maxima in a second streaming pass:
// 0.45 ms of the evaluation; a discarded group only lowers tau a little: ~7 % of the groups of a 40-item user.)
template <int NC>
__global__ __launch_bounds__(256) void sample_max_kernel_f32(
    const float *__restrict__ U, const float *__restrict__ V, int ld, int n_items, const int32_t *__restrict__ user_ids,
    int n_b, int b_pad, int n_s_tiles, int tiles_per_group, int n_groups, float *__restrict__ gmax, int32_t *__restrict__ garg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int upair = blockIdx.x;
    const int b0 = upair * 64 + r, b1 = b0 + 32;
    const bool live0 = b0 < n_b, live1 = b1 < n_b;
    const int64_t uid0 = user_ids[live0 ? b0 : n_b - 1], uid1 = user_ids[live1 ? b1 : n_b - 1];
    const int g_step = gridDim.y * 4;
    int g = blockIdx.y * 4 + wave;
    if (g >= n_groups) return;
    const F32Slots<NC> slots(ld, h);
    f32x4 ua[NC][8], ub[NC][8];
    slots.load_users(U + uid0 * ld, U + uid1 * ld, ua, ub);
    auto load_tile = [&](int s_tile, f32x4 (&dst)[NC][8]) {        // sampled tile s -> item tile s * kSampleStride
        slots.load_item(item_row_clamped(V, s_tile * kSampleStride * 32 + r, n_items, ld), dst);
    };
    f32x4 v[NC][8], vn[NC][8];
    bool first = true;
    for (; g < n_groups; g += g_step) {
        const int s_begin = g * tiles_per_group;
        int s_end = s_begin + tiles_per_group;
        if (s_end > n_s_tiles) s_end = n_s_tiles;
        float m0 = -__builtin_huge_valf(), m1 = m0;
        int a0 = 0, a1 = 0;
        if (first) { load_tile(s_begin, v); first = false; }
        for (int st = s_begin; st < s_end; st++) {
            // the next tile to come (this group's, or the first of the wavefront's next group) loads under this tile's MFMAs
            const int nxt = st + 1 < s_end ? st + 1 : (g + g_step) * tiles_per_group;
            const bool more = nxt < n_s_tiles && (st + 1 < s_end || g + g_step < n_groups);
            load_tile(more ? nxt : st, vn);          // unconditional: see stream_tiles (eval_tile.h)
            f32x16 acc0, acc1;
            zero(acc0); zero(acc1);
            mfma_f32(v, F32Chain<NC>{ua, acc0}, F32Chain<NC>{ub, acc1});
            const int item_base = st * kSampleStride * 32 + 4 * h;
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int item = lane_item(item_base, q);
                const bool in = item < n_items;                    // rows past the catalogue repeat its last item
                if (in && acc0[q] > m0) { m0 = acc0[q]; a0 = item; }
                if (in && acc1[q] > m1) { m1 = acc1[q]; a1 = item; }
            }
#pragma unroll
            for (int c = 0; c < NC; c++)
#pragma unroll
                for (int q = 0; q < 8; q++) v[c][q] = vn[c][q];
        }
        // the two k-slot halves of a column hold different item rows of the same user: fold them
        const float o0 = __shfl_xor(m0, 32, kWave), o1 = __shfl_xor(m1, 32, kWave);
        const int oa0 = __shfl_xor(a0, 32, kWave), oa1 = __shfl_xor(a1, 32, kWave);
        if (o0 > m0) { m0 = o0; a0 = oa0; }
        if (o1 > m1) { m1 = o1; a1 = oa1; }
        if (h == 0) {
            if (live0) { gmax[(int64_t)g * b_pad + b0] = m0; garg[(int64_t)g * b_pad + b0] = a0; }
            if (live1) { gmax[(int64_t)g * b_pad + b1] = m1; garg[(int64_t)g * b_pad + b1] = a1; }
        }
    }
}

// sample_max_kernel_f32 on the bf16 copies, every `stride`-th item tile (stride 1: the whole catalogue -- the pass costs 1/16 of
// the fp32 matrix-pipe time, so a denser sample, a higher threshold and fewer candidates are affordable).  The accumulator
// register number rides in the low 4 mantissa bits of the score (relative 2^-19: inside eps's 2 % slack), so the per-tile
// maximum is 16 v_and_or + 8 v_max3 and the best item is recovered from (tile, register, half).
template <int NM, int NU>      // NU user tiles of 32 per wavefront
__global__ __launch_bounds__(256, 2) void sample_max_bf16_kernel(
    const __bf16 *__restrict__ Ub, const __bf16 *__restrict__ Vb, int n_items, int n_b, int b_pad, int stride, int n_s_tiles,
    int tiles_per_group, int n_groups, float *__restrict__ gmax, int32_t *__restrict__ garg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int g_step = gridDim.y * 4;
    int g = blockIdx.y * 4 + wave;
    if (g >= n_groups) return;
    int bs[NU];
    bf16x8 uu[NU][NM];
#pragma unroll
    for (int k = 0; k < NU; k++) { bs[k] = (blockIdx.x * NU + k) * 32 + r; load_user_bf16<NM>(Ub, b_pad, bs[k], h, uu[k]); }
    auto load_tile = [&](int s_tile, bf16x8 (&dst)[NM]) { load_tile_bf16<NM>(Vb, (int64_t)s_tile * stride, lane, dst); };
    auto tagged_max = [](const f32x16 &a) {
        float t[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = __uint_as_float((__float_as_uint(a[q]) & ~15u) | (unsigned)q);
        const float x0 = fmaxf(fmaxf(t[0], t[1]), t[2]), x1 = fmaxf(fmaxf(t[3], t[4]), t[5]), x2 = fmaxf(fmaxf(t[6], t[7]), t[8]);
        const float x3 = fmaxf(fmaxf(t[9], t[10]), t[11]), x4 = fmaxf(fmaxf(t[12], t[13]), t[14]);
        return fmaxf(fmaxf(fmaxf(x0, x1), fmaxf(x2, x3)), fmaxf(x4, t[15]));
    };
    bf16x8 v[NM], vn[NM];
    bool first = true;
    for (; g < n_groups; g += g_step) {
        const int s_begin = g * tiles_per_group;
        int s_end = s_begin + tiles_per_group;
        if (s_end > n_s_tiles) s_end = n_s_tiles;
        float mx[NU];
        int ts[NU];
#pragma unroll
        for (int k = 0; k < NU; k++) { mx[k] = -__builtin_huge_valf(); ts[k] = s_begin; }
        if (first) { load_tile(s_begin, v); first = false; }
        for (int st = s_begin; st < s_end; st++) {
            const int nxt = st + 1 < s_end ? st + 1 : (g + g_step) * tiles_per_group;
            const bool more = nxt < n_s_tiles && (st + 1 < s_end || g + g_step < n_groups);
            load_tile(more ? nxt : st, vn);          // unconditional: see stream_tiles (eval_tile.h)
            f32x16 acc[NU];
#pragma unroll
            for (int k = 0; k < NU; k++) zero(acc[k]);
#pragma unroll
            for (int m = 0; m < NM; m++)
#pragma unroll
                for (int k = 0; k < NU; k++) acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v[m], uu[k][m], acc[k], 0, 0, 0);
            pad_rows_to_neg_inf(st * stride * 32, h, n_items, acc);
#pragma unroll
            for (int k = 0; k < NU; k++) {
                const float x = tagged_max(acc[k]);
                if (x > mx[k]) { mx[k] = x; ts[k] = st; }
            }
#pragma unroll
            for (int m = 0; m < NM; m++) v[m] = vn[m];
        }
#pragma unroll
        for (int k = 0; k < NU; k++) {
            const int q = (int)(__float_as_uint(mx[k]) & 15u);
            int a = lane_item(ts[k] * stride * 32 + 4 * h, q);
            float m = mx[k];
            const float o = __shfl_xor(m, 32, kWave);
            const int oa = __shfl_xor(a, 32, kWave);
            if (o > m) { m = o; a = oa; }
            if (h == 0 && bs[k] < n_b) { gmax[(int64_t)g * b_pad + bs[k]] = m; garg[(int64_t)g * b_pad + bs[k]] = a; }
        }
    }
}

// tau[b] = the M-th largest of the user's n_groups (<= kMaxGroups) group maxima, not counting groups whose best item is one the
// user has rated (bisection in the user's sorted rated items -- only for the groups that come up, ~M of them: as a kernel of its
// own over all (group, user) pairs the check was 88 us)
__global__ __launch_bounds__(256) void threshold_var_kernel(const float *__restrict__ gmax, const int32_t *__restrict__ garg,
                                                            const int32_t *__restrict__ user_ids, const int64_t *__restrict__ rated_indptr,
                                                            const int32_t *__restrict__ rated_sorted, int b_pad, int n_b, int n_groups, int M,
                                                            float *__restrict__ tau) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_b) return;
    float v[kMaxGroups];
#pragma unroll
    for (int g = 0; g < kMaxGroups; g++) v[g] = g < n_groups ? gmax[(int64_t)g * b_pad + b] : -__builtin_huge_valf();
    int64_t rbeg = 0, rend = 0;
    if (rated_indptr) { const int uid = user_ids[b]; rbeg = rated_indptr[uid]; rend = rated_indptr[uid + 1]; }
    float th = -__builtin_huge_valf();
    int found = 0;
    for (int it = 0; it < n_groups && found < M; it++) {
        int arg = 0;
        float best = v[0];
#pragma unroll
        for (int g = 1; g < kMaxGroups; g++)
            if (v[g] > best) { best = v[g]; arg = g; }
#pragma unroll
        for (int g = 0; g < kMaxGroups; g++)
            if (g == arg) v[g] = -__builtin_huge_valf();
        if (!(best > -__builtin_huge_valf())) break;
        if (rated_indptr) {
            const int item = garg[(int64_t)arg * b_pad + b];
            if (sorted_find(rated_sorted + rbeg, rend - rbeg, item) >= 0) continue;   // the group's best is a rated item: the group is out
        }
        th = best;
        found++;
    }
    tau[b] = found == M ? th : -__builtin_huge_valf();            // fewer than M groups left: tau <= 0, the user goes the exact way
}

__global__ __launch_bounds__(256) void lowered_tau_kernel(const float *__restrict__ tau, const float *__restrict__ u_norm,
                                                          const float *__restrict__ v_norm_max, int n_b, float *__restrict__ tau_low) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_b) tau_low[b] = tau[b] - 0x1p-7f * 1.02f * u_norm[b] * *v_norm_max;
}

// the same when tau_hat itself comes from bf16 scores (sample_max_bf16_kernel): N + 1 distinct unrated items have bf16 scores
// >= tau_hat, so fp32 scores >= tau_hat - eps =: tau (a threshold the user's N + 1 best fp32 scores reach); every item whose
// fp32 score reaches tau has a bf16 score >= tau - eps =: tau_low
__global__ __launch_bounds__(256) void lowered_tau2_kernel(float *__restrict__ tau, const float *__restrict__ u_norm,
                                                           const float *__restrict__ v_norm_max, int n_b, float *__restrict__ tau_low) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_b) {
        const float eps = 0x1p-7f * 1.02f * u_norm[b] * *v_norm_max, t = tau[b] - eps;
        tau[b] = t;
        tau_low[b] = t - eps;
    }
}

// ---- (B) the fp32 filter: two 32-user tiles per wavefront (two interleaved accumulator chains); OCC = wavefronts per SIMD the
// registers are capped for
template <int NC, int OCC>
__global__ __launch_bounds__(256, OCC) void score_filter2_kernel_f32(
    const float *__restrict__ U, const float *__restrict__ V, int ld, int n_items, const int32_t *__restrict__ user_ids,
    int n_b, const float *__restrict__ tau, int n_lists, float *__restrict__ cand_s,
    int32_t *__restrict__ cand_i, int32_t *__restrict__ cand_n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int upair = blockIdx.x;
    const int b0 = upair * 64 + r, b1 = b0 + 32;
    const int list = (blockIdx.y * 4 + wave) * 2 + h;
    // wavefront w of the user pair takes item tiles w, w + W, w + 2W, ... (W = wavefronts per user pair): every candidate
    // list samples the whole catalogue, so ids that correlate with popularity cannot overflow one list
    const int n_item_tiles = (n_items + 31) / 32;
    const int t_step = gridDim.y * 4;
    const int t_begin = blockIdx.y * 4 + wave, t_end = n_item_tiles;
    const bool live0 = b0 < n_b, live1 = b1 < n_b;
    const int64_t uid0 = user_ids[live0 ? b0 : n_b - 1], uid1 = user_ids[live1 ? b1 : n_b - 1];
    int cnt0 = 0, cnt1 = 0;
    if (t_begin < t_end) {
        const float th0 = live0 ? tau[b0] : __builtin_huge_valf(), th1 = live1 ? tau[b1] : __builtin_huge_valf();
        const F32Slots<NC> slots(ld, h);
        f32x4 ua[NC][8], ub[NC][8];
        slots.load_users(U + uid0 * ld, U + uid1 * ld, ua, ub);
        auto load_tile = [&](int t, f32x4 (&dst)[NC][8]) { slots.load_item(item_row_clamped(V, t * 32 + r, n_items, ld), dst); };
        float *cs0 = cand_s + ((int64_t)b0 * n_lists + list) * kListCap, *cs1 = cand_s + ((int64_t)b1 * n_lists + list) * kListCap;
        int32_t *ci0 = cand_i + ((int64_t)b0 * n_lists + list) * kListCap, *ci1 = cand_i + ((int64_t)b1 * n_lists + list) * kListCap;
        // one item tile: 64 MFMAs, then the accumulators against the two thresholds.  Every executed VALU instruction of
        // the epilogue costs matrix-pipe time (measured), so: the element tests are entered only when some lane's
        // 16-element maximum reaches its threshold, the item-range test exists only in the catalogue's last tile.
        auto do_tile = [&](int t, const f32x4 (&v)[NC][8]) {
            f32x16 acc[2];
            zero(acc[0]); zero(acc[1]);
            mfma_f32(v, F32Chain<NC>{ua, acc[0]}, F32Chain<NC>{ub, acc[1]});
            pad_rows_to_neg_inf(t * 32, h, n_items, acc);          // rows past the catalogue repeat its last item
            const f32x16 &acc0 = acc[0], &acc1 = acc[1];
            const int item_base = t * 32 + 4 * h;         
            float m0 = acc0[0], m1 = acc1[0];
#pragma unroll
            for (int q = 1; q < 16; q++) { m0 = fmaxf(m0, acc0[q]); m1 = fmaxf(m1, acc1[q]); }
            auto append = [&](const f32x16 &a, float th, int &cnt, float *cs, int32_t *ci) {      // ascending id per lane
#pragma unroll
                for (int q = 0; q < 16; q++)
                    if (a[q] >= th) {
                        if (cnt < kListCap) { cs[cnt] = a[q]; ci[cnt] = lane_item(item_base, q); }
                        cnt++;
                    }
            };
            if (m0 >= th0) append(acc0, th0, cnt0, cs0, ci0);
            if (m1 >= th1) append(acc1, th1, cnt1, cs1, ci1);
        };
        stream_tiles<f32x4[NC][8]>(t_begin, t_step, t_end, load_tile, do_tile);
    }
    if (live0) cand_n[(int64_t)b0 * n_lists + list] = cnt0;
    if (live1) cand_n[(int64_t)b1 * n_lists + list] = cnt1;
}

// ---- (B') score_filter2_kernel_f32's loop on the bf16 copies: what reaches the LOWERED threshold goes to the lane-private lists as
// an id (its approximate score only for inspection)
template <int NM, int NU>      // NU user tiles of 32 per wavefront: one fetched item tile feeds NU * NM MFMAs
__global__ __launch_bounds__(256, 2) void score_filter_bf16_kernel(
    const __bf16 *__restrict__ Ub, int b_pad, const __bf16 *__restrict__ Vb, int n_items, int n_b, const float *__restrict__ tau_low, int n_lists,
    int list_cap, float *__restrict__ cand_s, int32_t *__restrict__ cand_i, int32_t *__restrict__ cand_n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int list = (blockIdx.y * 4 + wave) * 2 + h;
    const int n_item_tiles = (n_items + 31) / 32;
    const int t_step = gridDim.y * 4;
    const int t_begin = blockIdx.y * 4 + wave, t_end = n_item_tiles;
    int bs[NU], cnt[NU];
    bool live[NU];
#pragma unroll
    for (int k = 0; k < NU; k++) { bs[k] = (blockIdx.x * NU + k) * 32 + r; live[k] = bs[k] < n_b; cnt[k] = 0; }
    if (t_begin < t_end) {
        float th[NU];
        bf16x8 uu[NU][NM];
        float *cs[NU];
        int32_t *ci[NU];
#pragma unroll
        for (int k = 0; k < NU; k++) {
            th[k] = live[k] ? tau_low[bs[k]] : __builtin_huge_valf();
            load_user_bf16<NM>(Ub, b_pad, bs[k], h, uu[k]);
            cs[k] = cand_s + ((int64_t)bs[k] * n_lists + list) * list_cap;
            ci[k] = cand_i + ((int64_t)bs[k] * n_lists + list) * list_cap;
        }
        auto load_tile = [&](int t, bf16x8 (&dst)[NM]) { load_tile_bf16<NM>(Vb, t, lane, dst); };
        auto do_tile = [&](int t, const bf16x8 (&v)[NM]) {
            f32x16 acc[NU];
#pragma unroll
            for (int k = 0; k < NU; k++) zero(acc[k]);
#pragma unroll
            for (int m = 0; m < NM; m++)
#pragma unroll
                for (int k = 0; k < NU; k++) acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v[m], uu[k][m], acc[k], 0, 0, 0);
            pad_rows_to_neg_inf(t * 32, h, n_items, acc);
            const int item_base = t * 32 + 4 * h;
            // hits are rare (about one per 32 x 32 tile): a tile is tested by the maximum of its 16 accumulator registers (v_max3
            // chains, one compare, one scalar branch on the wave's mask); a tile with a hit narrows down by register quads --
            // not 16 dependent compare / branch pairs per tile, which cost 2.5x the tile's MFMA time
#pragma unroll
            for (int k = 0; k < NU; k++) {
                const f32x16 &a = acc[k];
                float gq[4];
#pragma unroll
                for (int j = 0; j < 4; j++) gq[j] = fmaxf(fmaxf(fmaxf(a[4 * j], a[4 * j + 1]), a[4 * j + 2]), a[4 * j + 3]);
                const float mx = fmaxf(fmaxf(fmaxf(gq[0], gq[1]), gq[2]), gq[3]);
                if (__ballot(mx >= th[k])) {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (__ballot(gq[j] >= th[k])) {
#pragma unroll
                            for (int q = 4 * j; q < 4 * j + 4; q++)
                                if (a[q] >= th[k]) {
                                    if (cnt[k] < list_cap) { cs[k][cnt[k]] = a[q]; ci[k][cnt[k]] = lane_item(item_base, q); }
                                    cnt[k]++;
                                }
                        }
                }
            }
        };
        stream_tiles<bf16x8[NM]>(t_begin, t_step, t_end, load_tile, do_tile);
    }
#pragma unroll
    for (int k = 0; k < NU; k++)
        if (live[k]) cand_n[(int64_t)bs[k] * n_lists + list] = cnt[k];
}

// ---- (C) one wavefront per user: gather the candidates of the user's lists into LDS, take the K+1 largest by repeated
// wave-wide maximum of (score, lower id first); flag ties among them / overflow / tau <= 0.
template <int NC>       // column chunks of 64 in the re-scoring (ld <= 64: 1, ld = 128: 2)
__global__ __launch_bounds__(64 * kSelectWaves) void select_topk_kernel(
    const float *__restrict__ cand_s, const int32_t *__restrict__ cand_i, const int32_t *__restrict__ cand_n, int n_lists,
    const float *__restrict__ tau, const int32_t *__restrict__ user_ids, const int64_t *__restrict__ rated_indptr,
    const int32_t *__restrict__ rated_sorted, int n_b, int K, int32_t *__restrict__ ids_out, float *__restrict__ scores_out,
    int32_t *__restrict__ flags, int32_t *__restrict__ n_flagged, int32_t *__restrict__ flagged_list,
    const float *__restrict__ U, const float *__restrict__ V, int ld, int pool_cap, const float *__restrict__ tau_low, int list_cap) {
    // pool_cap: LDS entries per user (a user with more candidates is flagged and redone exactly); the lists' worst case,
    // n_lists * list_cap, would leave one wavefront per SIMD.
    // U != null: the candidates come from the bf16 filter -- their fp32 scores are formed here, by the MFMA sequence of
    // score_kernel_f32 (32 candidates as the item rows of a tile, the user's row broadcast over its 32 columns)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSelectWaves + wave;
    if (b >= n_b) return;                                         // whole wavefront
    unsigned long long *pool = reinterpret_cast<unsigned long long *>(smem) + (int64_t)wave * pool_cap;
    // the re-scoring's user operand (the same for every tile): fetched first, its latency under the pooling below
    const int r = lane & 31, h = lane >> 5;
    const F32Slots<NC> slots(ld, h);
    f32x4 uu[NC][8];
    slots.load_user((U ? U : V) + (U ? (int64_t)user_ids[b] : 0) * ld, uu);
    // key: score mapped to an order-preserving unsigned, then ~id so that among equal scores the LOWER id is larger
    auto key_of = [](float s, int32_t id) {
        unsigned u = __float_as_uint(s);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        return ((unsigned long long)u << 32) | (unsigned)(0x7fffffff - id);
    };
    bool bad = !(tau[b] > 0.f);
    int64_t rbeg = 0, rend = 0;
    if (rated_indptr) { const int uid = user_ids[b]; rbeg = rated_indptr[uid]; rend = rated_indptr[uid + 1]; }
    int total = 0, kept = 0;
    for (int l0 = 0; l0 < n_lists; l0 += 64) {                    // counts -> offsets (wave scan), candidates -> pool
        const int l = l0 + lane;
        int n = l < n_lists ? cand_n[(int64_t)b * n_lists + l] : 0;
        if (n > list_cap) { bad = true; n = list_cap; }
        int inc = n;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const int o = __shfl_up(inc, sft, 64);
            if (lane >= sft) inc += o;
        }
        const int off = total + inc - n;
        for (int c = 0; c < n; c++) {
            const int64_t at = ((int64_t)b * n_lists + l) * list_cap + c;
            if (off + c < pool_cap) pool[off + c] = key_of(cand_s[at], cand_i[at]);
        }
        total += __shfl(inc, 63, 64);
    }
    if (total > pool_cap) { bad = true; total = pool_cap; }
    // rated items are masked to 0 < tau: not candidates.  The lists are uneven, the pool is not: every lane bisects its
    // share of the pool (a few elements each)
    for (int e = lane; e < total; e += 64) {
        const int32_t item = 0x7fffffff - (int32_t)(unsigned)(pool[e] & 0xffffffffu);
        const bool rated = sorted_find(rated_sorted + rbeg, rend - rbeg, item) >= 0;
        if (rated) pool[e] = 0ull;
        kept += rated ? 0 : 1;
    }
    if (U) {
        // Which candidates can still be among the N + 1 best?  Their bf16 scores s^ are within eps of the fp32 scores.  Let L be
        // the (N+1)-th largest s^: N + 1 candidates have fp32 scores >= L - eps, so the fp32 (N+1)-th best is >= L - eps and a
        // candidate with s^ < L - 2 eps (fp32 score < L - eps) is out.  Only the others are re-scored: ~30 of ~250.
        const float eps = (tau[b] - tau_low[b]) * 1.01f;
        const int Mq = K + 1;
        unsigned long long below = ~0ull;
        if (total <= 64) {                                         // the usual case: one key per lane, ranks by v_readlane
            const unsigned long long key = lane < total ? pool[lane] : 0ull;
            const int rk = wave_rank_u64(key);
            const unsigned long long at = __ballot(key != 0ull && rk == Mq - 1);
            below = at ? wave_read_u64(key, __builtin_ctzll(at)) : 0ull;
        } else
        for (int rank = 0; rank < Mq; rank++) {                    // the Mq-th largest key, non-destructively
            unsigned long long best = 0;
            for (int e = lane; e < total; e += 64) {
                const unsigned long long k = pool[e];
                if (k < below && k > best) best = k;
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const unsigned long long o = __shfl_xor(best, m, 64);
                best = o > best ? o : best;
            }
            below = best;
            if (!best) break;                                      // fewer than Mq candidates (only after an overflow)
        }
        if (below) {
            unsigned ub_ = (unsigned)(below >> 32);
            ub_ = (ub_ & 0x80000000u) ? (ub_ & 0x7fffffffu) : ~ub_;
            const float cut = __uint_as_float(ub_) - 2.f * eps;
            const unsigned long long cut_key = key_of(cut, 0x7fffffff);          // the smallest key with that score
            int n_keep = 0;
            for (int e0 = 0; e0 < total; e0 += 64) {               // in-place forward compaction, chunk by chunk
                const int e = e0 + lane;
                const unsigned long long k = e < total ? pool[e] : 0ull;
                const bool keep = k != 0ull && k >= cut_key;
                const unsigned long long mask = __ballot(keep);
                const int pos = n_keep + __popcll(mask & ((1ull << lane) - 1ull));
                if (keep) pool[pos] = k;                           // pos <= e: never ahead of what is still to be read
                n_keep += __popcll(mask);
            }
            total = n_keep;
            kept = lane == 0 ? n_keep : 0;                         // survivors are unrated: the count the checks below sum up
        }
        auto item_of = [&](int e) -> int64_t {
            const unsigned long long k = e < total ? pool[e] : 0ull;
            return k ? (int64_t)(0x7fffffff - (int32_t)(unsigned)(k & 0xffffffffu)) : 0;
        };
        f32x4 vv[NC][8], vn[NC][8];
        slots.load_item(V + item_of(r) * ld, vv);
        for (int e0 = 0; e0 < total; e0 += 32) {
            if (e0 + 32 < total) slots.load_item(V + item_of(e0 + 32 + r) * ld, vn);      // the next tile's rows under this tile's MFMAs
            f32x16 acc;
            zero(acc);
            mfma_f32(vv, F32Chain<NC>{uu, acc});                                // the operand walk of score_kernel_f32, term for term
            // every column of the tile is this user: lanes 0 and 32 hold the 32 rows between them
            if (r == 0) {
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    const int ee = e0 + cd_row(q, h);
                    if (ee < total) {
                        const unsigned long long old = pool[ee];
                        if (old) pool[ee] = key_of(acc[q], 0x7fffffff - (int32_t)(unsigned)(old & 0xffffffffu));
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NC; c++)
#pragma unroll
                for (int q = 0; q < 8; q++) vv[c][q] = vn[c][q];
        }
    }
    bad = __any(bad);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) kept += __shfl_xor(kept, m, 64);
    const int M = K + 1;
    if (kept < M) bad = true;                                     // only after an overflow
    // each lane owns pool[lane], pool[lane + 64], ...
    unsigned long long prev = 0;
    bool tie = false;
    const int take = kept < M ? kept : M;
    if (total <= 64) {                                            // one key per lane: its rank is its place in the output
        const unsigned long long key = lane < total ? pool[lane] : 0ull;
        const int rk = wave_rank_u64(key);                        // rated / empty slots (0) rank behind every candidate
        if (key != 0ull && rk < take) pool[rk] = key;             // every lane has read its key: the pool can take the sorted run
        if (key != 0ull && rk < K && rk < take) {
            unsigned u = (unsigned)(key >> 32);
            u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
            ids_out[(int64_t)b * K + rk] = 0x7fffffff - (int32_t)(unsigned)(key & 0xffffffffu);
            scores_out[(int64_t)b * K + rk] = __uint_as_float(u);
        }
        tie = __any(lane >= 1 && lane < take && (pool[lane] >> 32) == (pool[lane - 1] >> 32));
    } else
    for (int rank = 0; rank < take; rank++) {
        unsigned long long best = 0;
        int where = -1;
        for (int e = lane; e < total; e += 64) {
            const unsigned long long k = pool[e];
            if (k > best) { best = k; where = e; }
        }
        unsigned long long wbest = best;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = __shfl_xor(wbest, m, 64);
            wbest = o > wbest ? o : wbest;
        }
        if (best == wbest && where >= 0) pool[where] = 0;          // keys are unique (ids differ): exactly one lane
        if (rank > 0 && (wbest >> 32) == (prev >> 32)) tie = true;
        prev = wbest;
        if (rank < K && lane == 0) {
            unsigned u = (unsigned)(wbest >> 32);
            u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
            ids_out[(int64_t)b * K + rank] = 0x7fffffff - (int32_t)(unsigned)(wbest & 0xffffffffu);
            scores_out[(int64_t)b * K + rank] = __uint_as_float(u);
        }
    }
    if (lane == 0) {
        const bool flag = bad || tie;
        flags[b] = flag ? 1 : 0;
        if (flag) flagged_list[atomicAdd(n_flagged, 1)] = b;
    }
}

// ---- (D) the flagged users' ids in, their exact lists out (the walk between them: eval_walk.h)
__global__ void gather_user_ids_kernel(const int32_t *__restrict__ user_ids, const int32_t *__restrict__ flagged_list, int off, int n,
                                       int32_t *__restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = user_ids[flagged_list[off + k]];
}
__global__ void scatter_rows_kernel(const int32_t *__restrict__ flagged_list, int off, int n, int K, const int32_t *__restrict__ ids_in,
                                    const float *__restrict__ sc_in, int32_t *__restrict__ ids_out, float *__restrict__ sc_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * K) return;
    const int64_t dst = (int64_t)flagged_list[off + t / K] * K + t % K;
    ids_out[dst] = ids_in[t];
    sc_out[dst] = sc_in[t];
}

}  // namespace

namespace qrec {

bool fused_ok(int dtype, int ld, int n_items, int K) {
    // QREC_EVAL_BLOCK_PATH forces the block route, in the scratch-size query and in the launch
    return dtype == QREC_F32 && ld <= 128 && K + 1 <= kSelectMax && n_items >= 64 * kSampleStride * 32 && !getenv("QREC_EVAL_BLOCK_PATH");
}

int64_t fused_path_bytes(int n_items, int n_b, int ld) { return layout_bytes(fused_layout, fused_geometry(n_items, n_b, ld), n_items, ld); }

int run_fused_topk_f32(const float *U, const float *V, int ld, int n_items, const int32_t *user_ids, int n_b,
                       const int64_t *rated_indptr, const int32_t *rated_sorted, int K, void *scratch, int32_t *ids_out,
                       float *scores_out, hipStream_t st) {
    const FusedGeom g = fused_geometry(n_items, n_b, ld);
    const FusedWs w = carve(scratch, fused_layout, g, n_items, ld);
    const int M = K + 1;
    const int bf16_stride_env = getenv("QREC_EVAL_BF16_STRIDE") ? atoi(getenv("QREC_EVAL_BF16_STRIDE")) : 1;
    const bool use_bf16 = g.use_bf16;
    const int bf16_stride = bf16_stride_env < 1 ? 1 : (bf16_stride_env > kSampleStride ? kSampleStride : bf16_stride_env);
    if (use_bf16) {
        // bf16 copies of the batch's user rows (gathered) and of the items, with |u_b| and max |v|
        QREC_HIP_CHECK(hipMemsetAsync(w.v_max, 0, sizeof(float), st));
        const int v_rows_pad = g.n_item_tiles * 32;
        with_nm_nu(ld, g.nu, [&](auto nm, auto) {
            constexpr int LPR = 4 * nm(), rows = 4 * (64 / LPR);              // lanes per row (ld / 4), rows per block
            hipLaunchKernelGGL((to_bf16_kernel<LPR, false>), dim3((unsigned)((g.b_pad + rows - 1) / rows)), dim3(256), 0, st, U,
                               user_ids, n_b, g.b_pad, w.Ub, w.u_norm, (float *)nullptr);
            hipLaunchKernelGGL((to_bf16_kernel<LPR, true>), dim3((unsigned)((v_rows_pad + rows - 1) / rows)), dim3(256), 0, st, V,
                               (const int32_t *)nullptr, n_items, v_rows_pad, w.Vb, (float *)nullptr, w.v_max);
        });
        QREC_LAUNCH_CHECK();
    }
    // (A) threshold: group maxima straight from a scoring loop -- fp32 over every kSampleStride-th item tile, or (bf16 route)
    // bf16 over every bf16_stride-th tile (default: all of them)
    {
        const int n_s_tiles = use_bf16 ? (g.n_item_tiles + bf16_stride - 1) / bf16_stride : g.n_s_tiles;
        int tpg = use_bf16 ? (n_s_tiles + kMaxGroups - 1) / kMaxGroups : n_s_tiles / 64;
        if (tpg < 1) tpg = 1;
        int n_groups = (n_s_tiles + tpg - 1) / tpg;
        while (n_groups > kMaxGroups) { tpg++; n_groups = (n_s_tiles + tpg - 1) / tpg; }
        int waves = ((use_bf16 ? 8192 : 2048) + g.grid_x - 1) / g.grid_x;           // a few groups per wavefront: its user rows are fetched once
        if (waves > n_groups) waves = n_groups;
        if (waves < 1) waves = 1;
        const dim3 sgrid((unsigned)g.grid_x, (unsigned)((waves + 3) / 4));
        if (use_bf16)
            with_nm_nu(ld, g.nu, [&](auto nm, auto nu) {
                hipLaunchKernelGGL((sample_max_bf16_kernel<nm(), nu()>), sgrid, dim3(256), 0, st, w.Ub, w.Vb, n_items, n_b, g.b_pad,
                                   bf16_stride, n_s_tiles, tpg, n_groups, w.gmax, w.garg);
            });
        else
            with_nc(ld, [&](auto nc) {
                hipLaunchKernelGGL(sample_max_kernel_f32<nc()>, sgrid, dim3(256), 0, st, U, V, ld, n_items, user_ids, n_b, g.b_pad, n_s_tiles,
                                   tpg, n_groups, w.gmax, w.garg);
            });
        QREC_LAUNCH_CHECK();
        const unsigned lane_blocks = (unsigned)((n_b + 255) / 256);
        hipLaunchKernelGGL(threshold_var_kernel, dim3(lane_blocks), dim3(256), 0, st, w.gmax, w.garg, user_ids, rated_indptr, rated_sorted, g.b_pad,
                           n_b, n_groups, M, w.tau);
        QREC_LAUNCH_CHECK();
        if (use_bf16) {
            hipLaunchKernelGGL(lowered_tau2_kernel, dim3(lane_blocks), dim3(256), 0, st, w.tau, w.u_norm, w.v_max, n_b, w.tau_low);
            QREC_LAUNCH_CHECK();
        }
    }
    // (B) score + filter, (C) select
    QREC_HIP_CHECK(hipMemsetAsync(w.n_flagged, 0, sizeof(int32_t), st));
    // measured at the Yelp2018 shape (kernel time of this pass; 0.98 ms of pure MFMA time): one user tile per wavefront at 4
    // wavefronts per SIMD 2.49 ms (twice the operand loads per MFMA); two tiles at one wavefront per SIMD 1.72, at two
    // wavefronts per SIMD 1.67 (launched here); the item tile shared by a block's wavefronts through LDS (coalesced fetch,
    // one barrier per tile) 1.89; the epilogue software-pipelined under the next tile's MFMAs over two accumulator pairs
    // 1.92 (448 registers, accumulators shuttling between AGPRs and VGPRs) although the same loop shape gains 22 % in
    // tools/ubench/mfma_tile.hip; thresholds at +inf (no element ever appended) 1.66: the pass is bound by the per-lane-row
    // operand fetch interleaved with the accumulator read-out, not by the compare / append work
    const dim3 grid((unsigned)g.grid_x, (unsigned)g.grid_y);
    if (use_bf16)
        // (B') the filter on v_mfma_f32_32x32x16_bf16 against the lowered thresholds
        with_nm_nu(ld, g.nu, [&](auto nm, auto nu) {
            hipLaunchKernelGGL((score_filter_bf16_kernel<nm(), nu()>), grid, dim3(256), 0, st, w.Ub, (int)g.b_pad, w.Vb, n_items, n_b, w.tau_low,
                               g.n_lists, g.list_cap, w.cand_s, w.cand_i, w.cand_n);
        });
    else
        with_nc(ld, [&](auto nc) {                                // registers: two wavefronts per SIMD at one chunk, one at two
            hipLaunchKernelGGL((score_filter2_kernel_f32<nc(), 2 / nc()>), grid, dim3(256), 0, st, U, V, ld, n_items, user_ids, n_b, w.tau,
                               g.n_lists, w.cand_s, w.cand_i, w.cand_n);
        });
    QREC_LAUNCH_CHECK();
    // candidates per user: ~ (N + 1) * kSampleStride * 1.1, times ~1.4 behind the bf16 filter; the pool holds 4x that
    int pool_cap = g.n_lists * g.list_cap;
    const int want = 4 * (int)((K + 1) * (use_bf16 ? bf16_stride : kSampleStride) * 1.6);
    if (pool_cap > want) pool_cap = want < 512 ? 512 : want;      // trained tables (uneven item norms) loosen the bound: keep room
    const size_t lds = (size_t)kSelectWaves * pool_cap * sizeof(unsigned long long);
    const dim3 sgrid((unsigned)((n_b + kSelectWaves - 1) / kSelectWaves));
    const float *Ur = use_bf16 ? U : (const float *)nullptr;
    decltype(&select_topk_kernel<1>) select = nullptr;
    with_nc(ld, [&](auto nc) { select = select_topk_kernel<nc()>; });
    QREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(select, sgrid, dim3(64 * kSelectWaves), lds, st, w.cand_s, w.cand_i, w.cand_n, g.n_lists, w.tau, user_ids, rated_indptr,
                       rated_sorted, n_b, K, ids_out, scores_out, w.flags, w.n_flagged, w.flagged_list, Ur, V, ld, pool_cap, w.tau_low, g.list_cap);
    QREC_LAUNCH_CHECK();
    // (D) users whose heap history matters: the block path, fb_users at a time
    int32_t h_nf = 0;
    QREC_HIP_CHECK(hipMemcpyAsync(&h_nf, w.n_flagged, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipStreamSynchronize(st));
    // Their scores as USER-MAJOR rows ([user][item]: a step of the walk -- 64 consecutive items -- is one 256-B access), masked,
    // then the exact sequential emulation, one wavefront per user: three launches.  (History: through the whole block route --
    // sliced top-N, flags, exact_wave_kernel on an [item][b_pad] block, every load of a step its own cache line -- the fallback
    // was 0.8 ms of the evaluation's 3.05; as [panel][item][64] panels, a column striding 256 B, 0.18 ms for a handful of users.)
    const int64_t row_len = (int64_t)g.n_item_tiles * 32;
    for (int off = 0; off < h_nf; off += g.fb_users) {
        const int n = h_nf - off < g.fb_users ? h_nf - off : g.fb_users;
        hipLaunchKernelGGL(gather_user_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, user_ids, w.flagged_list, off, n, w.fb_users);
        QREC_LAUNCH_CHECK();
        // a handful of users: many short wavefronts (>= 2 item tiles each)
        int rc = launch_score_block_f32(U, V, ld, n_items, w.fb_users, n, 2, w.fb_block, user_major_rows(row_len), st);
        if (rc == QREC_OK && rated_indptr) rc = launch_mask_block(w.fb_users, n, rated_indptr, rated_sorted, w.fb_block, user_major_rows(row_len), st);
        if (rc != QREC_OK) return rc;
        {                                                         // fused route: K + 1 <= 64
            const int stage_items = n_items < kWalkChunk ? (n_items + 3) / 4 * 4 : kWalkChunk;
            const size_t walk_lds = (size_t)stage_items * sizeof(float);
            QREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&exact_walk_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)walk_lds));
            hipLaunchKernelGGL(exact_walk_lds_kernel, dim3((unsigned)n), dim3(256), walk_lds, st, w.fb_block, row_len, n_items, K, w.fb_ids, w.fb_sc);
        }
        QREC_LAUNCH_CHECK();
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((n * K + 255) / 256)), dim3(256), 0, st, w.flagged_list, off, n, K, w.fb_ids, w.fb_sc,
                           ids_out, scores_out);
        QREC_LAUNCH_CHECK();
    }
    return QREC_OK;
}

}  // namespace qrec
