// Exposure-weighted ALS, fp64 (model/ranking/ExpoMF.py, model/ranking/SERec.py): per row r of the side being solved, over
// every column c of the other side's table F (rows f_c),
//     B_r = sum_c A_rc f_c f_c^T + lambda I,   b_r = sum_{c observed in r} f_c,   x_r = B_r^-1 b_r   (Cholesky)
// with the exposure posterior  A_rc = (pEX + EPS) / (pEX + EPS + (1 - mu_rc) / mu_rc),  pEX = sqrt(lam_y / 2 pi)
// exp(-lam_y (x_r . f_c)^2 / 2)  from the row's old x_r, and A_rc = 1 on the row's observed columns.  The prior pass sums
// A_uc over the users for every item c (new tables, old prior) and forms ExpoMF's mu_c or SERec's A_sum_c.
//
// Work layout: B_r is a GEMM with K running over the columns, F^T diag(A_r) F, on v_mfma_f64_16x16x4_f64.
// One 256-thread block owns R = 4 * RW rows (RW per wave); the columns stream through LDS 64 at a time and every wave reuses
// a staged chunk for its RW rows.  Per chunk, lane j of a wave forms the posterior of column j for each of its rows (one
// sequential FMA chain for x_r . f_c); per 4-column k-step each lane loads f[c = 4s + (lane >> 4)][16P + (lane & 15)] and
// issues one MFMA per lower-triangle 16 x 16 tile (P >= Q) of each row.  The observed columns then add (1 - A_rc) f f^T on
// the same MFMA path (gathered from global memory), and the rows are factored and solved one after another in LDS
// (chol_lds.h).  No users x items array exists anywhere; every sum has a fixed order, so two runs are bit-identical.
#include <algorithm>
#include <climits>
#include <cmath>

#include "chol_lds.h"
#include "common.h"

using namespace qrec;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kChunk = 64;             // columns staged per step (one posterior per lane)
constexpr double kEps = 1e-8;          // ExpoMF.py:7, SERec.py:7
constexpr int kPriorSegment = 2048;    // rows (users) per partial of the prior pass
constexpr int kPriorStage = 32;

enum Status { kOk = 0, kNotSpd = 1, kBadIndex = 2, kBadIndptr = 3 };

struct Prior {
    int mode;
    const double *v, *t, *a_sum;
    double a, b, s, n, lam_y, c0;
};

// mu of (row r, column c) -- the modes of qrec_expo_prior_t
__device__ inline double prior_mu(const Prior &p, int64_t r, int64_t c) {
    if (p.mode == QREC_EXPO_PRIOR_COL) return p.v[c];
    if (p.mode == QREC_EXPO_PRIOR_ROW) return p.v[r];
    const bool t_row = p.mode == QREC_EXPO_PRIOR_SOCIAL_T_ROW;
    const double t = t_row ? p.t[r] : p.t[c];
    const double A = t_row ? p.a_sum[c] : p.a_sum[r];
    const double S = t * A;                  // T.dot(tile(A_sum))[u, i] = t_u A_i (SERec.py:92-94)
    return (p.a + A + (p.s - 1.0) * S - 1.0) / (p.a + p.b + (p.s - 1.0) * S + p.n - 2.0);
}

__device__ inline double posterior(const Prior &p, double s, double mu) {
    const double pex = p.c0 * exp(-p.lam_y * (s * s) / 2.0);
    return (pex + kEps) / (pex + kEps + (1.0 - mu) / mu);
}

__device__ inline f64x4 mfma(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

struct SolveWs {
    int *status;         // [0] Status of the call, [1] smallest row whose pivot failed, [2] Status of the checks (fixed before the solve)
    double *x_new;       // [n_rows][ld]
};
SolveWs solve_layout(Carver &c, int64_t n_rows, int ld) {
    const SolveWs w = {c.take<int>(4, 256), c.take<double>((size_t)(n_rows * ld), 256)};
    c.pad(256);
    return w;
}

// status as in SolveWs; partial [n_seg][n_cols], one row per kPriorSegment users; a_new and mu_new [n_cols]
struct PriorWs { int *status; double *partial, *a_new, *mu_new; int n_seg; };
PriorWs prior_layout(Carver &c, int64_t n_rows, int64_t n_cols) {
    PriorWs w;
    w.n_seg = (int)std::max<int64_t>(1, (n_rows + kPriorSegment - 1) / kPriorSegment);
    w.status = c.take<int>(4, 256);
    w.partial = c.take<double>((size_t)(w.n_seg * n_cols), 256);
    w.a_new = c.take<double>((size_t)n_cols, 256);
    w.mu_new = c.take<double>((size_t)n_cols, 256);
    c.pad(256);
    return w;
}

// One block: status reset and the indptr checks (starts at 0, never decreases).
__global__ __launch_bounds__(kThreads) void expo_check_kernel(const int64_t *__restrict__ indptr, int64_t n_rows, int *status) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = indptr[0] != 0;
    __syncthreads();
    int bad = 0;
    for (int64_t r = threadIdx.x; r < n_rows; r += kThreads) bad |= indptr[r + 1] < indptr[r];
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) { status[0] = status[2] = s_bad ? kBadIndptr : kOk; status[1] = INT_MAX; }
}

template <int T, int RW>
__global__ __launch_bounds__(kThreads) void expo_solve_kernel(const double *__restrict__ F, int64_t n_cols,
                                                                const double *__restrict__ X, int64_t n_rows, int d,
                                                                const int64_t *__restrict__ indptr, const int32_t *__restrict__ idx,
                                                                Prior pr, double lambda, SolveWs w) {
    constexpr int ld = 16 * T, lds = ld + 1, NT = T * (T + 1) / 2, R = kWaves * RW;
    constexpr int kMem = ld * lds > kChunk * lds ? ld * lds : kChunk * lds;
    constexpr int kPer = kChunk * ld / kThreads;      // staged doubles per thread per chunk
    __shared__ double s_mem[kMem];                    // the staged chunk, then one row's system
    __shared__ double s_x[R * ld], s_rhs[R * ld], s_diag[ld];
    if (w.status[2] != kOk) return;                   // (status[0] may change under this launch: not read here)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, ii = lane & 15;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    for (int e = tid; e < R * ld; e += kThreads) {
        const int64_t r = r0 + e / ld;
        s_x[e] = r < n_rows ? X[r * ld + e % ld] : 0.0;
    }
    f64x4 acc[RW][NT];
#pragma unroll
    for (int q = 0; q < RW; ++q)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[q][t] = f64x4{0.0, 0.0, 0.0, 0.0};

    // ---- dense pass: every column, weight A_rc, chunk by chunk (the next chunk's loads in flight under the MFMAs) ----
    const int64_t n_chunks = (n_cols + kChunk - 1) / kChunk;
    double pre[kPer];
    auto load = [&](int64_t c0) {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int e = tid + q * kThreads;
            const int64_t g = c0 + e / ld;
            pre[q] = g < n_cols ? F[g * ld + e % ld] : 0.0;
        }
    };
    if (n_chunks > 0) load(0);
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int e = tid + q * kThreads;
            s_mem[(e / ld) * lds + e % ld] = pre[q];
        }
        __syncthreads();
        if (ch + 1 < n_chunks) load((ch + 1) * kChunk);
        const int64_t c = ch * kChunk + lane;
        double wt[RW];
#pragma unroll
        for (int q = 0; q < RW; ++q) {
            const int64_t r = r0 + wave * RW + q;
            const double *xr = s_x + (wave * RW + q) * ld;
            double s = 0.0;
            for (int p = 0; p < d; ++p) s = fma(xr[p], s_mem[lane * lds + p], s);
            wt[q] = c < n_cols && r < n_rows ? posterior(pr, s, prior_mu(pr, r, c)) : 0.0;
        }
        for (int st = 0; st < kChunk / 4; ++st) {
            double f[T];
#pragma unroll
            for (int P = 0; P < T; ++P) f[P] = s_mem[(4 * st + kk) * lds + 16 * P + ii];
#pragma unroll
            for (int q = 0; q < RW; ++q) {
                const double wk = __shfl(wt[q], 4 * st + kk, kWave);
                int t = 0;
#pragma unroll
                for (int P = 0; P < T; ++P) {
                    const double a = wk * f[P];
#pragma unroll
                    for (int Q = 0; Q <= P; ++Q, ++t) acc[q][t] = mfma(a, f[Q], acc[q][t]);
                }
            }
        }
    }
    __syncthreads();

    // ---- observed columns: (1 - A_rc) f f^T on the same path, b = sum f; 64 entries per posterior batch ----
#pragma unroll
    for (int q = 0; q < RW; ++q) {
        const int64_t r = r0 + wave * RW + q;
        double bs[T];
#pragma unroll
        for (int P = 0; P < T; ++P) bs[P] = 0.0;
        if (r < n_rows) {
            const double *xr = s_x + (wave * RW + q) * ld;
            const int64_t beg = indptr[r], end = indptr[r + 1];
            for (int64_t b0 = beg; b0 < end; b0 += kWave) {
                const int64_t e = b0 + lane;
                int c = -1;
                if (e < end) {
                    c = idx[e];
                    if (c < 0 || c >= n_cols) { atomicCAS(w.status, kOk, kBadIndex); c = -1; }
                }
                double wt = 0.0;
                if (c >= 0) {
                    double s = 0.0;
                    for (int p = 0; p < d; ++p) s = fma(xr[p], F[(int64_t)c * ld + p], s);
                    wt = 1.0 - posterior(pr, s, prior_mu(pr, r, c));
                }
                const int n_in = (int)min<int64_t>(kWave, end - b0);
                for (int st = 0; st < (n_in + 3) / 4; ++st) {
                    const int src = 4 * st + kk;
                    const double wk = __shfl(wt, src, kWave);
                    const int cc = __shfl(c, src, kWave);
                    double f[T];
#pragma unroll
                    for (int P = 0; P < T; ++P) {
                        f[P] = cc >= 0 ? F[(int64_t)cc * ld + 16 * P + ii] : 0.0;
                        bs[P] += f[P];
                    }
                    int t = 0;
#pragma unroll
                    for (int P = 0; P < T; ++P) {
                        const double a = wk * f[P];
#pragma unroll
                        for (int Q = 0; Q <= P; ++Q, ++t) acc[q][t] = mfma(a, f[Q], acc[q][t]);
                    }
                }
            }
        }
#pragma unroll
        for (int P = 0; P < T; ++P) {      // the four k-lanes' sums, in k order
            double v = __shfl(bs[P], ii, kWave);
            v += __shfl(bs[P], ii + 16, kWave);
            v += __shfl(bs[P], ii + 32, kWave);
            v += __shfl(bs[P], ii + 48, kWave);
            if (kk == 0) s_rhs[(wave * RW + q) * ld + 16 * P + ii] = v;
        }
    }

    // ---- the rows' systems one after another: lower-triangle tiles into LDS, Cholesky, both solves ----
    double *A = s_mem;
    constexpr int lda = lds;
    for (int wv = 0; wv < kWaves; ++wv) {
#pragma unroll
        for (int q = 0; q < RW; ++q) {
            const int slot = wv * RW + q;
            const int64_t r = r0 + slot;
            if (r >= n_rows) continue;              // uniform over the block
            __syncthreads();
            if (wave == wv) {
                int t = 0;
#pragma unroll
                for (int P = 0; P < T; ++P)
#pragma unroll
                    for (int Q = 0; Q <= P; ++Q, ++t)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int i = 16 * P + kk + 4 * g, j = 16 * Q + ii;
                            if (i < d && j < d) A[i * lda + j] = acc[q][t][g] + (i == j ? lambda : 0.0);
                        }
            }
            __syncthreads();
            if (!chol_factor_lds(A, lda, d, s_diag)) {
                if (tid == 0) { atomicCAS(w.status, kOk, kNotSpd); atomicMin(w.status + 1, (int)r); }
                continue;
            }
            if (tid < kWave) chol_solve_wave(A, lda, d, ld, s_rhs + slot * ld, s_diag, w.x_new + r * ld);
        }
    }
}

__global__ __launch_bounds__(kThreads) void expo_commit_kernel(double *__restrict__ dst, const double *__restrict__ src,
                                                                 int64_t n, const int *__restrict__ status) {
    if (status[0] != kOk) return;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) dst[e] = src[e];
}

// ---- prior pass ---------------------------------------------------------------------------------------------------------
// partial[y][c] = sum over rows u of segment y (kPriorSegment rows, in order) of A_uc, thread = column c.
template <int T>
__global__ __launch_bounds__(kThreads) void expo_prior_partial_kernel(const double *__restrict__ X, int64_t n_rows,
                                                                        const double *__restrict__ F, int64_t n_cols, int d,
                                                                        Prior pr, double *__restrict__ partial) {
    constexpr int ld = 16 * T;
    __shared__ double s_x[kPriorStage * ld];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * kThreads + tid;
    const int64_t u0 = (int64_t)blockIdx.y * kPriorSegment, u1 = min<int64_t>(u0 + kPriorSegment, n_rows);
    double f[ld];
#pragma unroll
    for (int p = 0; p < ld; ++p) f[p] = c < n_cols ? F[c * ld + p] : 0.0;
    double acc = 0.0;
    for (int64_t b = u0; b < u1; b += kPriorStage) {
        const int nb = (int)min<int64_t>(kPriorStage, u1 - b);
        __syncthreads();
        for (int e = tid; e < nb * ld; e += kThreads) s_x[e] = X[b * ld + e];
        __syncthreads();
        if (c < n_cols)
            for (int k = 0; k < nb; ++k) {
                double s = 0.0;
#pragma unroll
                for (int p = 0; p < ld; ++p)
                    if (p < d) s = fma(s_x[k * ld + p], f[p], s);
                acc += posterior(pr, s, prior_mu(pr, b + k, c));
            }
    }
    if (c < n_cols) partial[(int64_t)blockIdx.y * n_cols + c] = acc;
}

// A_c = the partials in segment order, then (1 - A_uc) for the observed users of c in CSR order; ExpoMF's mu_c from it.
__global__ __launch_bounds__(kThreads) void expo_prior_final_kernel(const double *__restrict__ X, int64_t n_rows,
                                                                      const double *__restrict__ F, int64_t n_cols, int d, int ld,
                                                                      const int64_t *__restrict__ indptr,
                                                                      const int32_t *__restrict__ idx, Prior pr,
                                                                      const double *__restrict__ partial, int n_seg,
                                                                      double *__restrict__ a_new, double *__restrict__ mu_new,
                                                                      int *status) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n_cols) return;
    double A = 0.0;
    for (int y = 0; y < n_seg; ++y) A += partial[(int64_t)y * n_cols + c];
    for (int64_t e = indptr[c]; e < indptr[c + 1]; ++e) {
        const int64_t u = idx[e];
        if (u < 0 || u >= n_rows) { atomicCAS(status, kOk, kBadIndex); continue; }
        double s = 0.0;
        for (int p = 0; p < d; ++p) s = fma(X[u * ld + p], F[c * ld + p], s);
        A += 1.0 - posterior(pr, s, prior_mu(pr, u, c));
    }
    a_new[c] = A;
    if (mu_new) mu_new[c] = (pr.a + A - 1.0) / (pr.a + pr.b + pr.n - 2.0);     // ExpoMF.py:73
}

bool valid_ld(int ld) { return ld == 16 || ld == 32 || ld == 64 || ld == 128; }

int to_prior(const qrec_expo_prior_t *p, const char *who, Prior *out) {
    QREC_REQUIRE(p, "%s: null prior", who);
    QREC_REQUIRE(p->mode >= QREC_EXPO_PRIOR_COL && p->mode <= QREC_EXPO_PRIOR_SOCIAL_T_COL, "%s: unknown prior mode %d", who, p->mode);
    QREC_REQUIRE(p->mode > QREC_EXPO_PRIOR_ROW || p->v, "%s: prior mode %d needs v", who, p->mode);
    QREC_REQUIRE(p->mode < QREC_EXPO_PRIOR_SOCIAL_T_ROW || (p->t && p->a_sum), "%s: a social prior needs t and a_sum", who);
    QREC_REQUIRE(p->lam_y > 0.0 && std::isfinite(p->lam_y) && std::isfinite(p->a) && std::isfinite(p->b) && std::isfinite(p->s) &&
                     std::isfinite(p->n_users),
                 "%s: lam_y must be finite and > 0, a, b, s, n_users finite", who);
    *out = Prior{p->mode, p->v, p->t, p->a_sum, p->a, p->b, p->s, p->n_users, p->lam_y, std::sqrt(p->lam_y / 2.0 / M_PI)};
    return QREC_OK;
}

template <int T, int RW>
void launch_solve(const double *F, int64_t n_cols, const double *X, int64_t n_rows, int d, const int64_t *indptr,
                  const int32_t *idx, const Prior &pr, double lambda, const SolveWs &w, hipStream_t st) {
    constexpr int R = kWaves * RW;
    expo_solve_kernel<T, RW><<<(unsigned)((n_rows + R - 1) / R), kThreads, 0, st>>>(F, n_cols, X, n_rows, d, indptr, idx, pr,
                                                                                     lambda, w);
}

}  // namespace

extern "C" int qrec_expo_solve_workspace_bytes(int64_t n_rows, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_rows >= 0 && valid_ld(ld), "qrec_expo_solve_workspace_bytes: bad arguments (n_rows %lld, ld %d)",
                 (long long)n_rows, ld);
    *bytes = layout_bytes(solve_layout, n_rows, ld);
    return QREC_OK;
}

extern "C" int qrec_expo_solve_rows(const double *d_F, int64_t n_cols, double *d_X, int64_t n_rows, int32_t d, int32_t ld,
                                    const int64_t *d_indptr, const int32_t *d_indices, const qrec_expo_prior_t *prior,
                                    double lambda, void *d_ws, int64_t ws_bytes, void *stream) {
    if (d > QREC_ALS_MAX_D) {
        set_error("qrec_expo_solve_rows: d = %d is above QREC_ALS_MAX_D (%d)", d, QREC_ALS_MAX_D);
        return QREC_ERR_UNSUPPORTED;
    }
    QREC_REQUIRE(d >= 1 && valid_ld(ld) && d <= ld, "qrec_expo_solve_rows: need 1 <= d <= ld, ld in {16,32,64,128} (d %d, ld %d)", d, ld);
    QREC_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows < INT_MAX, "qrec_expo_solve_rows: bad row counts");
    QREC_REQUIRE(lambda >= 0.0 && std::isfinite(lambda), "qrec_expo_solve_rows: lambda must be finite and >= 0 (%g)", lambda);
    QREC_REQUIRE(d_X && d_indptr && d_indices && d_ws && (d_F || n_cols == 0), "qrec_expo_solve_rows: null pointer");
    Carver c(d_ws);
    const SolveWs w = solve_layout(c, n_rows, ld);
    QREC_REQUIRE(ws_bytes >= (int64_t)c.bytes(), "qrec_expo_solve_rows: workspace of %lld bytes is too small", (long long)ws_bytes);
    Prior pr;
    if (int e = to_prior(prior, "qrec_expo_solve_rows", &pr)) return e;
    if (n_rows == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    expo_check_kernel<<<1, kThreads, 0, st>>>(d_indptr, n_rows, w.status);
    QREC_LAUNCH_CHECK();
    switch (ld) {
        case 16: launch_solve<1, 4>(d_F, n_cols, d_X, n_rows, d, d_indptr, d_indices, pr, lambda, w, st); break;
        case 32: launch_solve<2, 4>(d_F, n_cols, d_X, n_rows, d, d_indptr, d_indices, pr, lambda, w, st); break;
        case 64: launch_solve<4, 2>(d_F, n_cols, d_X, n_rows, d, d_indptr, d_indices, pr, lambda, w, st); break;
        default: launch_solve<8, 1>(d_F, n_cols, d_X, n_rows, d, d_indptr, d_indices, pr, lambda, w, st); break;
    }
    QREC_LAUNCH_CHECK();
    const int64_t n = n_rows * ld;
    expo_commit_kernel<<<(unsigned)std::min<int64_t>((n + kThreads - 1) / kThreads, 2048), kThreads, 0, st>>>(d_X, w.x_new, n, w.status);
    QREC_LAUNCH_CHECK();
    int status[2];
    QREC_HIP_CHECK(hipMemcpyAsync(status, w.status, sizeof(status), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipStreamSynchronize(st));
    switch (status[0]) {
        case kOk: return QREC_OK;
        case kNotSpd:
            set_error("qrec_expo_solve_rows: the system of row %d is not positive definite (non-positive pivot); nothing written", status[1]);
            return QREC_ERR_NOT_SPD;
        case kBadIndex:
            set_error("qrec_expo_solve_rows: a column index is outside [0, n_cols); nothing written");
            return QREC_ERR_INVALID;
        default:
            set_error("qrec_expo_solve_rows: indptr must start at 0 and never decrease; nothing written");
            return QREC_ERR_INVALID;
    }
}

extern "C" int qrec_expo_prior_workspace_bytes(int64_t n_rows, int64_t n_cols, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_rows >= 0 && n_cols >= 0, "qrec_expo_prior_workspace_bytes: bad arguments");
    *bytes = layout_bytes(prior_layout, n_rows, n_cols);
    return QREC_OK;
}

extern "C" int qrec_expo_prior(const double *d_X, int64_t n_rows, const double *d_F, int64_t n_cols, int32_t d, int32_t ld,
                               const int64_t *d_col_indptr, const int32_t *d_col_indices, const qrec_expo_prior_t *prior,
                               double *d_a_sum, double *d_mu, void *d_ws, int64_t ws_bytes, void *stream) {
    if (d > QREC_ALS_MAX_D) {
        set_error("qrec_expo_prior: d = %d is above QREC_ALS_MAX_D (%d)", d, QREC_ALS_MAX_D);
        return QREC_ERR_UNSUPPORTED;
    }
    QREC_REQUIRE(d >= 1 && valid_ld(ld) && d <= ld, "qrec_expo_prior: need 1 <= d <= ld, ld in {16,32,64,128} (d %d, ld %d)", d, ld);
    QREC_REQUIRE(n_rows >= 0 && n_cols >= 0, "qrec_expo_prior: bad sizes");
    QREC_REQUIRE(d_col_indptr && d_col_indices && d_a_sum && d_ws && (d_X || n_rows == 0) && (d_F || n_cols == 0),
                 "qrec_expo_prior: null pointer");
    Carver c(d_ws);
    const PriorWs w = prior_layout(c, n_rows, n_cols);
    QREC_REQUIRE(ws_bytes >= (int64_t)c.bytes(), "qrec_expo_prior: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)c.bytes());
    Prior pr;
    if (int e = to_prior(prior, "qrec_expo_prior", &pr)) return e;
    if (n_cols == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    expo_check_kernel<<<1, kThreads, 0, st>>>(d_col_indptr, n_cols, w.status);
    QREC_LAUNCH_CHECK();
    const dim3 grid((unsigned)((n_cols + kThreads - 1) / kThreads), (unsigned)w.n_seg);
    if (n_rows == 0) {
        QREC_HIP_CHECK(hipMemsetAsync(w.partial, 0, 8 * n_cols, st));
    } else {
        switch (ld) {
            case 16: expo_prior_partial_kernel<1><<<grid, kThreads, 0, st>>>(d_X, n_rows, d_F, n_cols, d, pr, w.partial); break;
            case 32: expo_prior_partial_kernel<2><<<grid, kThreads, 0, st>>>(d_X, n_rows, d_F, n_cols, d, pr, w.partial); break;
            case 64: expo_prior_partial_kernel<4><<<grid, kThreads, 0, st>>>(d_X, n_rows, d_F, n_cols, d, pr, w.partial); break;
            default: expo_prior_partial_kernel<8><<<grid, kThreads, 0, st>>>(d_X, n_rows, d_F, n_cols, d, pr, w.partial); break;
        }
        QREC_LAUNCH_CHECK();
    }
    expo_prior_final_kernel<<<grid.x, kThreads, 0, st>>>(d_X, n_rows, d_F, n_cols, d, ld, d_col_indptr, d_col_indices, pr, w.partial,
                                                         w.n_seg, w.a_new, d_mu ? w.mu_new : nullptr, w.status);
    QREC_LAUNCH_CHECK();
    const unsigned nb = (unsigned)std::min<int64_t>((n_cols + kThreads - 1) / kThreads, 2048);
    expo_commit_kernel<<<nb, kThreads, 0, st>>>(d_a_sum, w.a_new, n_cols, w.status);
    if (d_mu) expo_commit_kernel<<<nb, kThreads, 0, st>>>(d_mu, w.mu_new, n_cols, w.status);
    QREC_LAUNCH_CHECK();
    int h_status = 0;
    QREC_HIP_CHECK(hipMemcpyAsync(&h_status, w.status, sizeof(int), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipStreamSynchronize(st));
    if (h_status == kOk) return QREC_OK;
    set_error(h_status == kBadIndex ? "qrec_expo_prior: a row index is outside [0, n_rows); nothing written"
                                    : "qrec_expo_prior: indptr must start at 0 and never decrease; nothing written");
    return QREC_ERR_INVALID;
}
