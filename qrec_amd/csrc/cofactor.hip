// CoFactor (model/ranking/CoFactor.py), fp64: the item-item co-occurrence counts behind its SPPMI matrix (:36-56) and the
// context-augmented item step of its ALS sweep (:116-159).
//
// Co-occurrence.  count(i, j) = the number of users who rated both; a pair of distinct items is kept when count > filter
// and both have >= filter raters.  One block per (item i, tile of QREC_COOC_TILE candidate items): 32-bit counters of the
// tile in LDS, the raters of i walked one per wavefront, each rater's ascending item list searched for the tile's first item
// and walked to its last, LDS integer adds (integers: any order gives the same bits).  Two passes over the same tiles: the
// first counts the kept pairs of every (item, tile), a one-block scan turns them into offsets, the second fills a CSR whose
// rows have ascending columns -- the output is allocated exactly.
//
// Item step.  For item i with contexts k (SPPMI row of i, in the reference's order; s = the SPPMI value):
//     A  = X^T X + sum_u c_u x_u x_u^T + lambda I + sum_k g_k g_k^T        b  = sum_u (1 + c_u) x_u + sum_k (s - w_i - c_k) g_k
//     A2 = sum_k y_k y_k^T + gamma I                                        b2 = sum_k (s - w_k - c_i) y_k
//     y_i = A^-1 b,  g_i = A2^-1 b2,  w_i = mean_k (s - y_i . g_k - c_k),  c_i = mean_k (s - y_k . g_i - w_k)     (old y_i, g_i, w_i, c_i)
// It is a Gauss-Seidel sweep: the step reads the rows of its contexts, some already updated.  The caller passes a level
// schedule (no two items of a level are contexts of each other); one launch per level on one stream, one block per item.
// The rating part of A and b does not depend on the sweep and is computed for all those items by one launch ahead of the
// levels.  Items without contexts are plain ALS rows and go in one launch.  Layout as als.hip: 256 threads, thread (ty, tx)
// owns the entries (ty + 16a, tx + 16b) of the accumulator, neighbour rows staged in LDS 16 at a time, every sum in the
// neighbours' order, chol_lds.h for both solves.  The sweep runs on copies of the tables inside the workspace and is copied
// back only when every system was positive definite, so an error leaves the tables as they were.
#include <algorithm>
#include <climits>

#include "chol_lds.h"
#include "common.h"

using namespace qrec;

namespace {

constexpr int kThreads = 256;
constexpr int kStage = 16;
constexpr int kTile = QREC_COOC_TILE;
constexpr int kWaves = kThreads / kWave;
constexpr int kTilePerWave = kTile / kWaves;

enum Status { kOk = 0, kNotSpd = 1, kBadIndex = 3, kBadIndptr = 4 };
enum Mode { kPre = 0, kSolo = 1, kLevel = 2 };

__global__ void status_reset_kernel(int *status) {
    if (threadIdx.x == 0) { status[0] = kOk; status[1] = INT_MAX; }
}

// ---- co-occurrence -------------------------------------------------------------------------------------------------------
struct CoocArgs {
    const int64_t *i_indptr; const int32_t *i_users; int64_t n_items, i_nnz;
    const int64_t *u_indptr; const int32_t *u_items; int64_t n_users, u_nnz;
    int32_t filter; int64_t n_tiles;
};

inline int64_t cooc_tiles(int64_t n_items) { return std::max<int64_t>(1, (n_items + kTile - 1) / kTile); }
struct CoocWs { int *status; int64_t *offs; };      // offs [n_items * tiles + 1]: the kept pairs per (item, tile), then their scan
CoocWs cooc_layout(Carver &c, int64_t n_items) {
    const CoocWs w = {c.take<int>(2, 256), c.take<int64_t>((size_t)(n_items * cooc_tiles(n_items) + 1), 256)};
    c.pad(256);
    return w;
}

// The counters of tile [lo, hi) for item i into s_cnt; returns whether i has enough raters to keep any pair.
__device__ inline bool cooc_tile(const CoocArgs &a, int64_t i, int64_t lo, int64_t hi, unsigned *s_cnt, int *status) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < kTile; e += kThreads) s_cnt[e] = 0;
    __syncthreads();
    const int64_t rb = a.i_indptr[i], re = a.i_indptr[i + 1];
    if (rb < 0 || re < rb || re > a.i_nnz) {
        if (tid == 0) atomicCAS(status, kOk, kBadIndptr);
        return false;
    }
    if (re - rb < a.filter) return false;
    for (int64_t k = rb + wave; k < re; k += kWaves) {
        const int64_t u = a.i_users[k];
        if (u < 0 || u >= a.n_users) {
            if (lane == 0) atomicCAS(status, kOk, kBadIndex);
            continue;
        }
        const int64_t ub = a.u_indptr[u], ue = a.u_indptr[u + 1];
        if (ub < 0 || ue < ub || ue > a.u_nnz) {
            if (lane == 0) atomicCAS(status, kOk, kBadIndptr);
            continue;
        }
        int64_t p = ub, q = ue;                     // the first entry >= lo
        while (p < q) {
            const int64_t m = (p + q) >> 1;
            if (a.u_items[m] < lo) p = m + 1; else q = m;
        }
        for (p += lane; p < ue; p += kWave) {
            const int64_t v = a.u_items[p];
            if (v >= hi) break;
            if (v >= lo) atomicAdd(&s_cnt[v - lo], 1u);
        }
    }
    __syncthreads();
    return true;
}

__device__ inline bool cooc_kept(const CoocArgs &a, int64_t i, int64_t lo, int64_t hi, int e, const unsigned *s_cnt) {
    const int64_t j = lo + e;
    return j < hi && j != i && (int64_t)s_cnt[e] > (int64_t)a.filter;
}

// FILL = false: the number of kept pairs of the block's (item, tile) into offs[block]; FILL = true: the pairs themselves, from
// offs[block] on, in ascending column order (wave w owns the w-th quarter of the tile; ballots order the lanes).
template <bool FILL>
__global__ __launch_bounds__(kThreads) void cooc_kernel(CoocArgs a, int64_t *__restrict__ offs, int *status,
                                                         int64_t *__restrict__ out_indptr, int32_t *__restrict__ out_cols,
                                                         int32_t *__restrict__ out_counts, int64_t capacity) {
    __shared__ unsigned s_cnt[kTile];
    __shared__ int s_wsum[kWaves];
    const int64_t blk = blockIdx.x, i = blk / a.n_tiles, t = blk % a.n_tiles;
    const int64_t lo = t * kTile, hi = min<int64_t>(lo + kTile, a.n_items);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (FILL && tid == 0) {
        if (t == 0) out_indptr[i] = offs[blk];
        if (blk == a.n_items * a.n_tiles - 1) out_indptr[a.n_items] = offs[blk + 1];
    }
    const bool any = cooc_tile(a, i, lo, hi, s_cnt, status);
    int n = 0;
    if (any)
        for (int r = 0; r < kTilePerWave / kWave; ++r)
            n += __popcll(__ballot(cooc_kept(a, i, lo, hi, wave * kTilePerWave + r * kWave + lane, s_cnt)));
    if (lane == 0) s_wsum[wave] = n;
    __syncthreads();
    if (!FILL) {
        if (tid == 0) {
            int s = 0;
            for (int w = 0; w < kWaves; ++w) s += s_wsum[w];
            offs[blk] = s;
        }
        return;
    }
    if (!any) return;
    int64_t base = offs[blk];
    for (int w = 0; w < wave; ++w) base += s_wsum[w];
    for (int r = 0; r < kTilePerWave / kWave; ++r) {
        const int e = wave * kTilePerWave + r * kWave + lane;
        const bool k = cooc_kept(a, i, lo, hi, e, s_cnt);
        const unsigned long long mask = __ballot(k);
        const int64_t pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (k && pos < capacity) { out_cols[pos] = (int32_t)(lo + e); out_counts[pos] = (int32_t)s_cnt[e]; }
        base += __popcll(mask);
    }
}

// One block: offs[0 .. n) (counts) into their exclusive scan, offs[n] = the total.
__global__ __launch_bounds__(1024) void cooc_scan_kernel(int64_t *__restrict__ offs, int64_t n) {
    __shared__ int64_t s_sum[1024];
    const int tid = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = min<int64_t>(tid * per, n), hi = min<int64_t>(lo + per, n);
    int64_t s = 0;
    for (int64_t r = lo; r < hi; ++r) s += offs[r];
    s_sum[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int t = 0; t < 1024; ++t) { const int64_t v = s_sum[t]; s_sum[t] = run; run += v; }
        offs[n] = run;
    }
    __syncthreads();
    int64_t run = s_sum[tid];
    for (int64_t r = lo; r < hi; ++r) { const int64_t v = offs[r]; offs[r] = run; run += v; }
}

int cooc_check(const char *who, const CoocArgs &a, void *d_ws, int64_t ws_bytes, CoocWs *w) {
    QREC_REQUIRE(a.n_items >= 1 && a.n_users >= 0 && a.i_nnz >= 0 && a.u_nnz >= 0 && a.n_items <= INT_MAX && a.n_users <= INT_MAX,
                 "%s: bad sizes (items %lld, users %lld)", who, (long long)a.n_items, (long long)a.n_users);
    QREC_REQUIRE(a.filter >= 0, "%s: filter must be >= 0 (%d)", who, a.filter);
    QREC_REQUIRE(a.i_indptr && a.u_indptr && (a.i_users || a.i_nnz == 0) && (a.u_items || a.u_nnz == 0) && d_ws, "%s: null pointer", who);
    Carver c(d_ws);
    *w = cooc_layout(c, a.n_items);
    QREC_REQUIRE(ws_bytes >= (int64_t)c.bytes(), "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes, (long long)c.bytes());
    QREC_REQUIRE(a.n_items * a.n_tiles <= INT_MAX, "%s: too many (item, tile) blocks", who);
    return QREC_OK;
}

int cooc_status(const char *who, int status) {
    if (status == kOk) return QREC_OK;
    if (status == kBadIndex) set_error("%s: a user index is outside [0, n_users)", who);
    else set_error("%s: an indptr decreases or passes the end of its index array", who);
    return QREC_ERR_INVALID;
}

// ---- the item step -------------------------------------------------------------------------------------------------------
struct ItemArgs {
    const double *X; int64_t n_users; const double *XtX;
    double *Y, *G, *w, *c;                      // the sweep's working copies
    int64_t n_items; int d;
    const int64_t *r_indptr; const int32_t *r_users; const double *r_conf; int64_t r_nnz;
    const int64_t *s_indptr; const int32_t *s_items; const double *s_vals; int64_t s_nnz;
    double lambda, gamma;
    double *pre;                                // [n_ctx][ld * ld + ld]: the rating part of A and b
    int *status;                                // [0] Status, [1] smallest item whose pivot failed
};

// acc += sum_k a_k f_k f_k^T,  bacc (thread tid < ld: column tid) += sum_k b_k f_k,  esum (thread 0) += sum_k e_k  over the
// entries k in [beg, end), f_k = row idx[k] of F, in CSR order with one FMA chain per accumulator entry.
//   KIND 0 (ratings):        a = val,  b = 1 + val
//   KIND 1 (contexts for y): a = 1,    b = (val - self_bias) - bias[idx],   e = (val - s_self . f) - bias[idx]
//   KIND 2 (contexts for g): a = 1,    b = (val - bias[idx]) - self_bias,   e = (val - s_self . f) - bias[idx]
template <int T, int KIND>
__device__ inline void accumulate(const double *F, int64_t f_rows, const int32_t *__restrict__ idx, const double *__restrict__ val,
                                  int64_t beg, int64_t end, const double *bias, double self_bias, const double *s_self,
                                  double (&acc)[T][T], double &bacc, double &esum, double *s_f, double *s_af, double *s_bk,
                                  double *s_e, int *status) {
    constexpr int ld = 16 * T;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const double *s_l = KIND == 0 ? s_af : s_f;
    for (int64_t base = beg; base < end; base += kStage) {
        const int nk = (int)min<int64_t>(kStage, end - base);
        {   // stage: neighbour k = ty, columns tx + 16 b
            const int k = ty;
            bool ok = k < nk;
            int64_t g = 0;
            double v = 0.0, bk = 0.0, ek = 0.0, t = 0.0;
            if (ok) {
                g = idx[base + k];
                if (g < 0 || g >= f_rows) {
                    ok = false;
                    if (tx == 0) atomicCAS(status, kOk, kBadIndex);
                }
            }
            if (ok) {
                v = val[base + k];
                if (KIND != 0) t = bias[g];
            }
            double f[T], dot = 0.0;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                f[b] = ok ? F[g * ld + tx + 16 * b] : 0.0;
                s_f[k * ld + tx + 16 * b] = f[b];
                if (KIND == 0) s_af[k * ld + tx + 16 * b] = v * f[b];
                else dot = fma(s_self[tx + 16 * b], f[b], dot);
            }
            if (KIND == 0) {
                bk = ok ? 1.0 + v : 0.0;
            } else {
                dot = row_allreduce_sum<16>(dot);
                if (ok) {
                    bk = KIND == 1 ? (v - self_bias) - t : (v - t) - self_bias;
                    ek = (v - dot) - t;
                }
            }
            if (tx == 0) { s_bk[k] = bk; s_e[k] = ek; }
        }
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            double li[T], fj[T];
#pragma unroll
            for (int a = 0; a < T; ++a) li[a] = s_l[k * ld + ty + 16 * a];
#pragma unroll
            for (int b = 0; b < T; ++b) fj[b] = s_f[k * ld + tx + 16 * b];
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int b = 0; b < T; ++b) acc[a][b] = fma(li[a], fj[b], acc[a][b]);
            if (tid < ld) bacc = fma(s_bk[k], s_f[k * ld + tid], bacc);
        }
        if (KIND != 0 && tid == 0)
            for (int k = 0; k < nk; ++k) esum += s_e[k];
        __syncthreads();
    }
}

template <int T>
__device__ inline void zero(double (&acc)[T][T]) {
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) acc[a][b] = 0.0;
}

// One block per item list[pos0 + blockIdx.x].  kPre: the rating part of A and b into pre[pos]; kSolo: an item without
// contexts, accumulated and solved; kLevel: the context sums on top of pre[pos], both solves, both biases.
template <int T>
__global__ __launch_bounds__(kThreads) void cofactor_item_kernel(ItemArgs a, int mode, const int32_t *__restrict__ list, int64_t pos0) {
    constexpr int ld = 16 * T, lda = ld + 1;
    constexpr int kA = ld * lda > 2 * kStage * ld ? ld * lda : 2 * kStage * ld;
    __shared__ double s_mem[kA];                 // staging while accumulating, then A
    __shared__ double s_y[ld], s_g[ld], s_b[ld], s_diag[ld], s_bk[kStage], s_e[kStage];
    __shared__ int s_status;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    if (tid == 0) s_status = a.status[0];        // read once: another block of this launch may flag an error meanwhile
    __syncthreads();
    if (s_status != kOk) return;
    const int64_t pos = pos0 + blockIdx.x, i = list[pos];
    if (i < 0 || i >= a.n_items) {
        if (tid == 0) atomicCAS(a.status, kOk, kBadIndex);
        return;
    }
    const int d = a.d;
    double acc[T][T];
    zero<T>(acc);
    double bacc = 0.0, esum = 0.0;
    double *pre = a.pre + pos * (int64_t)(ld * ld + ld);
    if (mode != kLevel) {
        const int64_t rb = a.r_indptr[i], re = a.r_indptr[i + 1];
        if (rb < 0 || re < rb || re > a.r_nnz) {
            if (tid == 0) atomicCAS(a.status, kOk, kBadIndptr);
            return;
        }
        accumulate<T, 0>(a.X, a.n_users, a.r_users, a.r_conf, rb, re, nullptr, 0.0, nullptr, acc, bacc, esum, s_mem,
                         s_mem + kStage * ld, s_bk, s_e, a.status);
        if (mode == kPre) {
#pragma unroll
            for (int p = 0; p < T; ++p)
#pragma unroll
                for (int q = 0; q < T; ++q) pre[(ty + 16 * p) * ld + tx + 16 * q] = acc[p][q];
            if (tid < ld) pre[ld * ld + tid] = bacc;
            return;
        }
    }
    int64_t sb = 0, se = 0;
    double w_i = 0.0, c_i = 0.0, esum_w = 0.0;
    if (mode == kLevel) {
        sb = a.s_indptr[i]; se = a.s_indptr[i + 1];
        if (sb < 0 || se < sb || se > a.s_nnz) {
            if (tid == 0) atomicCAS(a.status, kOk, kBadIndptr);
            return;
        }
        if (tid < ld) { s_y[tid] = a.Y[i * ld + tid]; s_g[tid] = a.G[i * ld + tid]; }
        w_i = a.w[i]; c_i = a.c[i];
        __syncthreads();
        accumulate<T, 1>(a.G, a.n_items, a.s_items, a.s_vals, sb, se, a.c, w_i, s_y, acc, bacc, esum_w, s_mem, nullptr, s_bk,
                         s_e, a.status);
    }
    double *A = s_mem;
#pragma unroll
    for (int p = 0; p < T; ++p)
#pragma unroll
        for (int q = 0; q < T; ++q) {
            const int r = ty + 16 * p, s = tx + 16 * q;
            if (r < d && s < d) {
                const double lam = r == s ? a.lambda : 0.0;
                A[r * lda + s] = mode == kLevel ? ((a.XtX[r * ld + s] + pre[r * ld + s]) + lam) + acc[p][q]
                                                : (a.XtX[r * ld + s] + acc[p][q]) + lam;
            }
        }
    if (tid < ld) s_b[tid] = mode == kLevel ? pre[ld * ld + tid] + bacc : bacc;
    __syncthreads();
    if (!chol_factor_lds(A, lda, d, s_diag)) {
        if (tid == 0) { atomicCAS(a.status, kOk, kNotSpd); atomicMin(a.status + 1, (int)i); }
        return;
    }
    if (tid < kWave) chol_solve_wave(A, lda, d, ld, s_b, s_diag, a.Y + i * ld);
    if (mode != kLevel || se == sb) return;
    __syncthreads();
    zero<T>(acc);
    bacc = 0.0;
    accumulate<T, 2>(a.Y, a.n_items, a.s_items, a.s_vals, sb, se, a.w, c_i, s_g, acc, bacc, esum, s_mem, nullptr, s_bk, s_e,
                     a.status);
#pragma unroll
    for (int p = 0; p < T; ++p)
#pragma unroll
        for (int q = 0; q < T; ++q) {
            const int r = ty + 16 * p, s = tx + 16 * q;
            if (r < d && s < d) A[r * lda + s] = acc[p][q] + (r == s ? a.gamma : 0.0);
        }
    if (tid < ld) s_b[tid] = bacc;
    __syncthreads();
    if (!chol_factor_lds(A, lda, d, s_diag)) {
        if (tid == 0) { atomicCAS(a.status, kOk, kNotSpd); atomicMin(a.status + 1, (int)i); }
        return;
    }
    if (tid < kWave) chol_solve_wave(A, lda, d, ld, s_b, s_diag, a.G + i * ld);
    if (tid == 0) {
        const double n = (double)(se - sb);
        a.w[i] = esum_w / n;
        a.c[i] = esum / n;
    }
}

__global__ __launch_bounds__(kThreads) void cofactor_commit_kernel(ItemArgs a, int ld, double *__restrict__ Y, double *__restrict__ G,
                                                                    double *__restrict__ w, double *__restrict__ c) {
    if (a.status[0] != kOk) return;              // every launch of the sweep is complete: the status is final
    const int64_t n = a.n_items * ld, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) { Y[e] = a.Y[e]; G[e] = a.G[e]; }
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n_items; e += stride) { w[e] = a.w[e]; c[e] = a.c[e]; }
}

bool valid_ld(int ld) { return ld == 16 || ld == 32 || ld == 64 || ld == 128; }

// the working copies and `pre` of ItemArgs
void item_layout(Carver &c, int64_t n_items, int64_t n_ctx, int ld, ItemArgs *a) {
    a->status = c.take<int>(2, 256);
    a->Y = c.take<double>((size_t)(n_items * ld), 256);
    a->G = c.take<double>((size_t)(n_items * ld), 256);
    a->w = c.take<double>((size_t)n_items, 256);
    a->c = c.take<double>((size_t)n_items, 256);
    a->pre = c.take<double>((size_t)(n_ctx * ((int64_t)ld * ld + ld)), 256);
    c.pad(256);
}

template <int T>
void launch_item(const ItemArgs &a, int mode, const int32_t *list, int64_t pos0, int64_t n, hipStream_t st) {
    cofactor_item_kernel<T><<<(unsigned)n, kThreads, 0, st>>>(a, mode, list, pos0);
}

void launch_item_ld(int ld, const ItemArgs &a, int mode, const int32_t *list, int64_t pos0, int64_t n, hipStream_t st) {
    switch (ld) {
        case 16: launch_item<1>(a, mode, list, pos0, n, st); break;
        case 32: launch_item<2>(a, mode, list, pos0, n, st); break;
        case 64: launch_item<4>(a, mode, list, pos0, n, st); break;
        default: launch_item<8>(a, mode, list, pos0, n, st); break;
    }
}

}  // namespace

extern "C" int qrec_cooc_workspace_bytes(int64_t n_items, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_items >= 1 && n_items <= INT_MAX, "qrec_cooc_workspace_bytes: bad arguments (n_items %lld)", (long long)n_items);
    *bytes = layout_bytes(cooc_layout, n_items);
    return QREC_OK;
}

extern "C" int qrec_cooc_count(const int64_t *d_i_indptr, const int32_t *d_i_users, int64_t n_items, int64_t i_nnz,
                               const int64_t *d_u_indptr, const int32_t *d_u_items, int64_t n_users, int64_t u_nnz, int32_t filter,
                               int64_t *kept, void *d_ws, int64_t ws_bytes, void *stream) {
    QREC_REQUIRE(kept, "qrec_cooc_count: null pointer");
    const CoocArgs a{d_i_indptr, d_i_users, n_items, i_nnz, d_u_indptr, d_u_items, n_users, u_nnz, filter, cooc_tiles(std::max<int64_t>(n_items, 1))};
    CoocWs w;
    if (int rc = cooc_check("qrec_cooc_count", a, d_ws, ws_bytes, &w)) return rc;
    hipStream_t st = as_stream(stream);
    const int64_t n = n_items * a.n_tiles;
    status_reset_kernel<<<1, 64, 0, st>>>(w.status);
    QREC_LAUNCH_CHECK();
    cooc_kernel<false><<<(unsigned)n, kThreads, 0, st>>>(a, w.offs, w.status, nullptr, nullptr, nullptr, 0);
    QREC_LAUNCH_CHECK();
    cooc_scan_kernel<<<1, 1024, 0, st>>>(w.offs, n);
    QREC_LAUNCH_CHECK();
    int h_status = 0;
    int64_t total = 0;
    QREC_HIP_CHECK(hipMemcpyAsync(&h_status, w.status, sizeof(int), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipMemcpyAsync(&total, w.offs + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipStreamSynchronize(st));
    if (int rc = cooc_status("qrec_cooc_count", h_status)) return rc;
    *kept = total;
    return QREC_OK;
}

extern "C" int qrec_cooc_fill(const int64_t *d_i_indptr, const int32_t *d_i_users, int64_t n_items, int64_t i_nnz,
                              const int64_t *d_u_indptr, const int32_t *d_u_items, int64_t n_users, int64_t u_nnz, int32_t filter,
                              int64_t *d_out_indptr, int32_t *d_out_cols, int32_t *d_out_counts, int64_t capacity, void *d_ws,
                              int64_t ws_bytes, void *stream) {
    const CoocArgs a{d_i_indptr, d_i_users, n_items, i_nnz, d_u_indptr, d_u_items, n_users, u_nnz, filter, cooc_tiles(std::max<int64_t>(n_items, 1))};
    CoocWs w;
    if (int rc = cooc_check("qrec_cooc_fill", a, d_ws, ws_bytes, &w)) return rc;
    QREC_REQUIRE(d_out_indptr && capacity >= 0 && ((d_out_cols && d_out_counts) || capacity == 0), "qrec_cooc_fill: null pointer or capacity < 0");
    hipStream_t st = as_stream(stream);
    const int64_t n = n_items * a.n_tiles;
    int64_t total = 0;
    QREC_HIP_CHECK(hipMemcpyAsync(&total, w.offs + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipStreamSynchronize(st));
    QREC_REQUIRE(total >= 0 && total <= capacity, "qrec_cooc_fill: %lld kept pairs, room for %lld; nothing written (qrec_cooc_count of the same "
                 "inputs must come first)", (long long)total, (long long)capacity);
    status_reset_kernel<<<1, 64, 0, st>>>(w.status);
    QREC_LAUNCH_CHECK();
    cooc_kernel<true><<<(unsigned)n, kThreads, 0, st>>>(a, w.offs, w.status, d_out_indptr, d_out_cols, d_out_counts, capacity);
    QREC_LAUNCH_CHECK();
    int h_status = 0;
    QREC_HIP_CHECK(hipMemcpyAsync(&h_status, w.status, sizeof(int), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipStreamSynchronize(st));
    return cooc_status("qrec_cooc_fill", h_status);
}

extern "C" int qrec_cofactor_item_workspace_bytes(int64_t n_items, int64_t n_ctx_items, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_items >= 0 && n_ctx_items >= 0 && n_ctx_items <= n_items && valid_ld(ld),
                 "qrec_cofactor_item_workspace_bytes: bad arguments (n_items %lld, n_ctx_items %lld, ld %d)", (long long)n_items,
                 (long long)n_ctx_items, ld);
    ItemArgs a{};
    *bytes = layout_bytes(item_layout, n_items, n_ctx_items, ld, &a);
    return QREC_OK;
}

extern "C" int qrec_cofactor_item_rows(const double *d_X, int64_t n_users, const double *d_XtX, double *d_Y, double *d_G, double *d_w,
                                       double *d_c, int64_t n_items, int32_t d, int32_t ld, const int64_t *d_r_indptr,
                                       const int32_t *d_r_users, const double *d_r_conf, int64_t r_nnz, const int64_t *d_s_indptr,
                                       const int32_t *d_s_items, const double *d_s_vals, int64_t s_nnz, const int32_t *d_order,
                                       const int32_t *h_level_ptr, int32_t n_levels, const int32_t *d_solo, int64_t n_solo,
                                       double lambda, double gamma, void *d_ws, int64_t ws_bytes, void *stream) {
    const char *who = "qrec_cofactor_item_rows";
    QREC_REQUIRE(d >= 1 && d <= QREC_ALS_MAX_D && valid_ld(ld) && d <= ld, "%s: need 1 <= d <= ld, ld in {16,32,64,128} (d %d, ld %d)", who, d, ld);
    QREC_REQUIRE(n_items >= 0 && n_users >= 0 && r_nnz >= 0 && s_nnz >= 0 && n_levels >= 0 && n_solo >= 0 && n_items <= INT_MAX,
                 "%s: negative count", who);
    QREC_REQUIRE(lambda >= 0.0 && lambda <= 1.79769313486231570e308 && gamma >= 0.0 && gamma <= 1.79769313486231570e308,
                 "%s: lambda and gamma must be finite and >= 0 (%g, %g)", who, lambda, gamma);
    QREC_REQUIRE(d_XtX && d_Y && d_G && d_w && d_c && d_r_indptr && d_s_indptr && d_ws && (d_X || n_users == 0) &&
                 (d_r_users && d_r_conf || r_nnz == 0) && (d_s_items && d_s_vals || s_nnz == 0) && (h_level_ptr || n_levels == 0) &&
                 (d_solo || n_solo == 0), "%s: null pointer", who);
    int64_t n_ctx = 0;
    if (n_levels > 0) {
        QREC_REQUIRE(h_level_ptr[0] == 0, "%s: level_ptr must start at 0", who);
        for (int l = 0; l < n_levels; ++l)
            QREC_REQUIRE(h_level_ptr[l + 1] >= h_level_ptr[l], "%s: level_ptr decreases at level %d", who, l);
        n_ctx = h_level_ptr[n_levels];
    }
    QREC_REQUIRE(n_ctx + n_solo <= n_items && (d_order || n_ctx == 0), "%s: %lld scheduled + %lld other items, %lld in the table", who,
                 (long long)n_ctx, (long long)n_solo, (long long)n_items);
    ItemArgs a{};
    Carver c(d_ws);
    item_layout(c, n_items, n_ctx, ld, &a);
    QREC_REQUIRE(ws_bytes >= (int64_t)c.bytes(), "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes, (long long)c.bytes());
    if (n_items == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    a.X = d_X; a.n_users = n_users; a.XtX = d_XtX; a.n_items = n_items; a.d = d;
    a.r_indptr = d_r_indptr; a.r_users = d_r_users; a.r_conf = d_r_conf; a.r_nnz = r_nnz;
    a.s_indptr = d_s_indptr; a.s_items = d_s_items; a.s_vals = d_s_vals; a.s_nnz = s_nnz;
    a.lambda = lambda; a.gamma = gamma;
    status_reset_kernel<<<1, 64, 0, st>>>(a.status);
    QREC_LAUNCH_CHECK();
    QREC_HIP_CHECK(hipMemcpyAsync(a.Y, d_Y, 8 * n_items * ld, hipMemcpyDeviceToDevice, st));
    QREC_HIP_CHECK(hipMemcpyAsync(a.G, d_G, 8 * n_items * ld, hipMemcpyDeviceToDevice, st));
    QREC_HIP_CHECK(hipMemcpyAsync(a.w, d_w, 8 * n_items, hipMemcpyDeviceToDevice, st));
    QREC_HIP_CHECK(hipMemcpyAsync(a.c, d_c, 8 * n_items, hipMemcpyDeviceToDevice, st));
    if (n_ctx > 0) {
        launch_item_ld(ld, a, kPre, d_order, 0, n_ctx, st);
        QREC_LAUNCH_CHECK();
    }
    if (n_solo > 0) {
        launch_item_ld(ld, a, kSolo, d_solo, 0, n_solo, st);
        QREC_LAUNCH_CHECK();
    }
    for (int l = 0; l < n_levels; ++l) {
        const int64_t n = h_level_ptr[l + 1] - h_level_ptr[l];
        if (n == 0) continue;
        launch_item_ld(ld, a, kLevel, d_order, h_level_ptr[l], n, st);
        QREC_LAUNCH_CHECK();
    }
    cofactor_commit_kernel<<<(unsigned)std::min<int64_t>((n_items * ld + kThreads - 1) / kThreads, 2048), kThreads, 0, st>>>(a, ld, d_Y, d_G, d_w, d_c);
    QREC_LAUNCH_CHECK();
    int status[2];
    QREC_HIP_CHECK(hipMemcpyAsync(status, a.status, sizeof(status), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipStreamSynchronize(st));
    switch (status[0]) {
        case kOk: return QREC_OK;
        case kNotSpd:
            set_error("%s: a system of item %d is not positive definite (non-positive pivot); nothing written", who, status[1]);
            return QREC_ERR_NOT_SPD;
        case kBadIndex:
            set_error("%s: a user, context or item index is outside its table; nothing written", who);
            return QREC_ERR_INVALID;
        default:
            set_error("%s: an indptr decreases or passes the end of its index array; nothing written", who);
            return QREC_ERR_INVALID;
    }
}
