// Alternating least squares, fp64 (model/ranking/WRMF.py:17-67): per row r of a CSR over the other side's table F,
//     A_r = G + sum_k c_k f_k f_k^T + lambda I,   b_r = sum_k (1 + c_k) f_k,   x_r = A_r^-1 b_r   (Cholesky)
// with G = F^T F.  Every sum is taken in a fixed order with a fixed partition, so a run is bit-identical to the next.
//
// Work layout: 256 threads per row, a 16 x 16 thread grid, thread (ty, tx) owning the entries
// (ty + 16a, tx + 16b) of the ld x ld accumulator in registers (T = ld / 16 per side).  Neighbour rows are staged in LDS
// 16 at a time; the rank-1 updates are VALU FMAs (fp64 FMA and fp64 MFMA have the same peak rate on this chip:
// tools/ubench/fp64_rate.hip).  The factorisation and both triangular solves run on A in LDS.  Rows with more than
// QREC_ALS_SPLIT_DEGREE neighbours are accumulated by QREC_ALS_SEGMENT-neighbour segments in a kernel of their own, and
// their solve adds the segments' partials in segment order.
#include <algorithm>
#include <climits>

#include "chol_lds.h"
#include "common.h"

using namespace qrec;

namespace {

constexpr int kThreads = 256;
constexpr int kStage = 16;           // neighbour rows staged per step
constexpr int kGramRowsPerBlock = 256;
constexpr int kGramMaxBlocks = 256;

enum Status { kOk = 0, kNotSpd = 1, kWorkspace = 2, kBadIndex = 3, kBadIndptr = 4 };

// One block accumulates  acc += sum_k c_k f_k f_k^T,  bacc (thread tid < ld: column tid) += sum_k (1 + c_k) f_k,
// loss (thread 0) += sum_k (1 - x_old . f_k)^2  over neighbours k in [beg, end) (rows idx[k] of F, or rows k when idx is
// NULL; c_k = 1 when c is NULL).  Order: neighbours in CSR order, one FMA chain per accumulator entry.
template <int T>
__device__ inline void accumulate(const double *__restrict__ F, int64_t f_rows, const int32_t *__restrict__ idx,
                                  const double *__restrict__ c, int64_t beg, int64_t end, const double *s_x,
                                  double (&acc)[T][T], double &bacc, double &loss, double *s_f, double *s_cf,
                                  double *s_c1, double *s_err, int *status) {
    constexpr int ld = 16 * T;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    for (int64_t base = beg; base < end; base += kStage) {
        const int nk = (int)min<int64_t>(kStage, end - base);
        {   // stage: neighbour k = ty, columns tx + 16 b
            const int k = ty;
            double f[T];
            double ck = 0.0;
            bool ok = k < nk;
            int64_t g = 0;
            if (ok) {
                g = idx ? (int64_t)idx[base + k] : base + k;
                if (g < 0 || g >= f_rows) {
                    ok = false;
                    if (tx == 0) atomicCAS(status, kOk, kBadIndex);
                }
                ck = c ? c[base + k] : 1.0;
            }
            double dot = 0.0;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                f[b] = ok ? F[g * ld + tx + 16 * b] : 0.0;
                if (s_x) dot = fma(s_x[tx + 16 * b], f[b], dot);
                s_f[k * ld + tx + 16 * b] = f[b];
                s_cf[k * ld + tx + 16 * b] = ck * f[b];
            }
            if (s_x) {
                dot = row_allreduce_sum<16>(dot);
                if (tx == 0) s_err[k] = (1.0 - dot) * (1.0 - dot);
            }
            if (tx == 0) s_c1[k] = 1.0 + ck;
        }
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            double ci[T], fj[T];
#pragma unroll
            for (int a = 0; a < T; ++a) ci[a] = s_cf[k * ld + ty + 16 * a];
#pragma unroll
            for (int b = 0; b < T; ++b) fj[b] = s_f[k * ld + tx + 16 * b];
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int b = 0; b < T; ++b) acc[a][b] = fma(ci[a], fj[b], acc[a][b]);
            if (tid < ld) bacc = fma(s_c1[k], s_f[k * ld + tid], bacc);
        }
        if (s_x && tid == 0)
            for (int k = 0; k < nk; ++k) loss += s_err[k];
        __syncthreads();
    }
}

// ---- G = F^T F ----------------------------------------------------------------------------------------------------------
// Block b sums rows [b * per, (b + 1) * per) into partial b; the reduce kernel adds the partials in block order.
inline int gram_blocks(int64_t rows) {
    if (rows <= 0) return 1;
    const int64_t nb = (rows + kGramRowsPerBlock - 1) / kGramRowsPerBlock;
    return (int)std::min<int64_t>(nb, kGramMaxBlocks);
}

template <int T>
__global__ __launch_bounds__(kThreads) void als_gram_partial_kernel(const double *__restrict__ F, int64_t rows, int64_t per,
                                                                      double *__restrict__ partial) {
    constexpr int ld = 16 * T;
    __shared__ double s_f[kStage * ld], s_cf[kStage * ld], s_c1[kStage];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    double acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) acc[a][b] = 0.0;
    double bacc = 0.0, loss = 0.0;
    const int64_t beg = min<int64_t>((int64_t)blockIdx.x * per, rows), end = min<int64_t>(beg + per, rows);
    accumulate<T>(F, rows, nullptr, nullptr, beg, end, nullptr, acc, bacc, loss, s_f, s_cf, s_c1, nullptr, nullptr);
    double *out = partial + (int64_t)blockIdx.x * ld * ld;
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) out[(ty + 16 * a) * ld + tx + 16 * b] = acc[a][b];
}

__global__ __launch_bounds__(kThreads) void als_gram_reduce_kernel(const double *__restrict__ partial, int n_parts, int ld2,
                                                                     double *__restrict__ G) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= ld2) return;
    double s = 0.0;
    for (int p = 0; p < n_parts; ++p) s += partial[(int64_t)p * ld2 + e];
    G[e] = s;
}

// ---- the row solves -----------------------------------------------------------------------------------------------------
struct SolveWs {
    int *status;            // [0] Status of the call, [1] smallest row whose pivot failed, [2] Status of the plan (fixed once planned)
    int64_t *seg_off;       // [n_rows + 1] first split segment of each row (exclusive scan of the segment counts)
    double *row_loss;       // [n_rows]
    double *x_new;          // [n_rows][ld] the solutions, copied into the table only when every row succeeded
    double *partial;        // [capacity][seg_stride] per segment: ld x ld sum, ld b, 1 loss
    int64_t capacity, seg_stride;
};

inline int64_t seg_stride_of(int ld) { return ((int64_t)ld * ld + ld + 1 + 31) & ~int64_t(31); }
__host__ __device__ inline int64_t segments_of(int64_t deg) {
    return deg > QREC_ALS_SPLIT_DEGREE ? (deg + QREC_ALS_SEGMENT - 1) / QREC_ALS_SEGMENT : 0;
}

// The fixed part of the layout; `partial` is whatever the buffer holds behind it, counted in whole segments.
SolveWs solve_layout(Carver &c, int64_t ws_bytes, int64_t n_rows, int ld) {
    SolveWs w;
    w.status = c.take<int>(4, 256);
    w.seg_off = c.take<int64_t>((size_t)(n_rows + 1), 256);
    w.row_loss = c.take<double>((size_t)n_rows, 256);
    w.x_new = c.take<double>((size_t)(n_rows * ld), 256);
    w.partial = c.take<double>(0, 256);
    w.seg_stride = seg_stride_of(ld);
    w.capacity = (ws_bytes - (int64_t)c.bytes()) / (8 * w.seg_stride);
    return w;
}

// One block: status reset, indptr checks, the exclusive scan of the per-row segment counts.
__global__ __launch_bounds__(1024) void als_plan_kernel(const int64_t *__restrict__ indptr, int64_t n_rows, SolveWs w) {
    __shared__ int64_t s_sum[1024];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) { s_bad = 0; w.status[0] = kOk; w.status[1] = INT_MAX; w.status[2] = kOk; }
    const int64_t per = (n_rows + 1023) / 1024, lo = min<int64_t>(tid * per, n_rows), hi = min<int64_t>(lo + per, n_rows);
    int64_t s = 0;
    for (int64_t r = lo; r < hi; ++r) {
        const int64_t deg = indptr[r + 1] - indptr[r];
        if (deg < 0) s_bad = 1;
        s += segments_of(deg);
    }
    s_sum[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int t = 0; t < 1024; ++t) { const int64_t v = s_sum[t]; s_sum[t] = run; run += v; }
        w.seg_off[n_rows] = run;
        const int plan = indptr[0] != 0 || s_bad ? kBadIndptr : run > w.capacity ? kWorkspace : kOk;
        w.status[0] = plan; w.status[2] = plan;
    }
    __syncthreads();
    int64_t run = s_sum[tid];
    for (int64_t r = lo; r < hi; ++r) {
        w.seg_off[r] = run;
        run += segments_of(indptr[r + 1] - indptr[r]);
    }
}

// Segment s of a split row (grid = the workspace's capacity; segments past the plan's count return at once).
template <int T>
__global__ __launch_bounds__(kThreads) void als_segment_kernel(const double *__restrict__ F, int64_t f_rows,
                                                                 const double *__restrict__ X, int64_t n_rows,
                                                                 const int64_t *__restrict__ indptr, const int32_t *__restrict__ idx,
                                                                 const double *__restrict__ c, int with_loss, SolveWs w) {
    constexpr int ld = 16 * T;
    __shared__ double s_f[kStage * ld], s_cf[kStage * ld], s_c1[kStage], s_err[kStage], s_x[ld];
    const int64_t s = blockIdx.x;
    if (w.status[2] != kOk || s >= w.seg_off[n_rows]) return;     // (status[0] may change under this launch: not read here)
    int64_t lo = 0, hi = n_rows - 1;            // the row r with seg_off[r] <= s < seg_off[r + 1]
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (w.seg_off[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const int64_t r = lo;
    const int64_t beg = indptr[r] + (s - w.seg_off[r]) * QREC_ALS_SEGMENT;
    const int64_t end = min<int64_t>(beg + QREC_ALS_SEGMENT, indptr[r + 1]);
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    if (with_loss && tid < ld) s_x[tid] = X[r * ld + tid];
    __syncthreads();
    double acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) acc[a][b] = 0.0;
    double bacc = 0.0, loss = 0.0;
    accumulate<T>(F, f_rows, idx, c, beg, end, with_loss ? s_x : nullptr, acc, bacc, loss, s_f, s_cf, s_c1, s_err, w.status);
    double *out = w.partial + s * w.seg_stride;
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) out[(ty + 16 * a) * ld + tx + 16 * b] = acc[a][b];
    if (tid < ld) out[ld * ld + tid] = bacc;
    if (tid == 0) out[ld * ld + ld] = loss;
}

// One block per row: accumulate (or add the row's segment partials in order), form A and b, Cholesky, two triangular
// solves, the solution into x_new.  A non-positive (or NaN) pivot stops the row and flags the call.
template <int T>
__global__ __launch_bounds__(kThreads) void als_solve_kernel(const double *__restrict__ F, int64_t f_rows,
                                                               const double *__restrict__ G, const double *__restrict__ X,
                                                               int64_t n_rows, int d, const int64_t *__restrict__ indptr,
                                                               const int32_t *__restrict__ idx, const double *__restrict__ c,
                                                               double lambda, int with_loss, SolveWs w) {
    constexpr int ld = 16 * T, lda = ld + 1;
    constexpr int kA = ld * lda > 2 * kStage * ld ? ld * lda : 2 * kStage * ld;
    __shared__ double s_mem[kA];                 // staging while accumulating, then A
    __shared__ double s_x[ld], s_b[ld], s_diag[ld], s_c1[kStage], s_err[kStage];
    const int64_t r = blockIdx.x;
    if (w.status[2] != kOk) return;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    if (with_loss && tid < ld) s_x[tid] = X[r * ld + tid];
    __syncthreads();
    double acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) acc[a][b] = 0.0;
    double bacc = 0.0, loss = 0.0;
    const int64_t s0 = w.seg_off[r], s1 = w.seg_off[r + 1];
    if (s0 == s1) {
        accumulate<T>(F, f_rows, idx, c, indptr[r], indptr[r + 1], with_loss ? s_x : nullptr, acc, bacc, loss,
                      s_mem, s_mem + kStage * ld, s_c1, s_err, w.status);
    } else {
        for (int64_t s = s0; s < s1; ++s) {
            const double *p = w.partial + s * w.seg_stride;
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int b = 0; b < T; ++b) acc[a][b] += p[(ty + 16 * a) * ld + tx + 16 * b];
            if (tid < ld) bacc += p[ld * ld + tid];
            if (tid == 0) loss += p[ld * ld + ld];
        }
        __syncthreads();
    }
    double *A = s_mem;
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) {
            const int i = ty + 16 * a, j = tx + 16 * b;
            if (i < d && j < d) A[i * lda + j] = G[i * ld + j] + acc[a][b] + (i == j ? lambda : 0.0);
        }
    if (tid < ld) s_b[tid] = bacc;
    if (tid == 0 && with_loss) w.row_loss[r] = loss;
    __syncthreads();
    // Cholesky (chol_lds.h): L overwrites the strict lower triangle, the diagonal goes to s_diag
    if (!chol_factor_lds(A, lda, d, s_diag)) {
        if (tid == 0) { atomicCAS(w.status, kOk, kNotSpd); atomicMin(w.status + 1, (int)r); }
        return;
    }
    if (tid >= 64) return;
    chol_solve_wave(A, lda, d, ld, s_b, s_diag, w.x_new + r * ld);
}

// The solutions into the table, the loss partials into one sum (fixed order) -- only when every row succeeded.
__global__ __launch_bounds__(kThreads) void als_commit_kernel(double *__restrict__ X, int64_t n_elems, SolveWs w) {
    if (w.status[0] != kOk) return;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n_elems; e += (int64_t)gridDim.x * kThreads)
        X[e] = w.x_new[e];
}

__global__ __launch_bounds__(kThreads) void als_loss_kernel(int64_t n_rows, SolveWs w, double *__restrict__ out) {
    if (w.status[0] != kOk) return;
    double s = 0.0;
    for (int64_t r = threadIdx.x; r < n_rows; r += kThreads) s += w.row_loss[r];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, kWave);
    __shared__ double s_part[kThreads / kWave];
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

bool valid_ld(int ld) { return ld == 16 || ld == 32 || ld == 64 || ld == 128; }

template <int T>
void launch_gram(const double *F, int64_t rows, double *partial, int nb, int64_t per, hipStream_t st) {
    als_gram_partial_kernel<T><<<nb, kThreads, 0, st>>>(F, rows, per, partial);
}

template <int T>
void launch_solve(const double *F, int64_t f_rows, const double *G, double *X, int64_t n_rows, int d,
                  const int64_t *indptr, const int32_t *idx, const double *c, double lambda, int with_loss,
                  const SolveWs &w, hipStream_t st) {
    if (w.capacity > 0)
        als_segment_kernel<T><<<(unsigned)w.capacity, kThreads, 0, st>>>(F, f_rows, X, n_rows, indptr, idx, c, with_loss, w);
    if (n_rows > 0)
        als_solve_kernel<T><<<(unsigned)n_rows, kThreads, 0, st>>>(F, f_rows, G, X, n_rows, d, indptr, idx, c, lambda, with_loss, w);
}

}  // namespace

extern "C" int qrec_als_gram_workspace_bytes(int64_t rows, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && rows >= 0 && valid_ld(ld), "qrec_als_gram_workspace_bytes: bad arguments (rows %lld, ld %d)",
                 (long long)rows, ld);
    *bytes = (int64_t)gram_blocks(rows) * ld * ld * 8;
    return QREC_OK;
}

extern "C" int qrec_als_gram(const double *d_F, int64_t rows, int32_t d, int32_t ld, double *d_G, void *d_ws, int64_t ws_bytes,
                             void *stream) {
    QREC_REQUIRE(d >= 1 && d <= QREC_ALS_MAX_D && valid_ld(ld) && d <= ld, "qrec_als_gram: need 1 <= d <= ld, ld in {16,32,64,128} (d %d, ld %d)", d, ld);
    QREC_REQUIRE(rows >= 0 && d_G && d_ws && (d_F || rows == 0), "qrec_als_gram: null pointer or rows < 0");
    const int nb = gram_blocks(rows);
    QREC_REQUIRE(ws_bytes >= (int64_t)nb * ld * ld * 8, "qrec_als_gram: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                 (long long)nb * ld * ld * 8);
    const int64_t per = rows > 0 ? (rows + nb - 1) / nb : 0;
    hipStream_t st = as_stream(stream);
    double *partial = static_cast<double *>(d_ws);
    switch (ld) {
        case 16: launch_gram<1>(d_F, rows, partial, nb, per, st); break;
        case 32: launch_gram<2>(d_F, rows, partial, nb, per, st); break;
        case 64: launch_gram<4>(d_F, rows, partial, nb, per, st); break;
        default: launch_gram<8>(d_F, rows, partial, nb, per, st); break;
    }
    QREC_LAUNCH_CHECK();
    als_gram_reduce_kernel<<<(ld * ld + kThreads - 1) / kThreads, kThreads, 0, st>>>(partial, nb, ld * ld, d_G);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

extern "C" int qrec_als_solve_workspace_bytes(const int64_t *h_indptr, int64_t n_rows, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_rows >= 0 && valid_ld(ld) && (h_indptr || n_rows == 0),
                 "qrec_als_solve_workspace_bytes: bad arguments (n_rows %lld, ld %d)", (long long)n_rows, ld);
    int64_t segs = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t deg = h_indptr[r + 1] - h_indptr[r];
        QREC_REQUIRE(deg >= 0, "qrec_als_solve_workspace_bytes: indptr decreases at row %lld", (long long)r);
        segs += segments_of(deg);
    }
    Carver c(nullptr);
    const SolveWs w = solve_layout(c, 0, n_rows, ld);
    *bytes = (int64_t)c.bytes() + segs * 8 * w.seg_stride;
    return QREC_OK;
}

extern "C" int qrec_als_solve_rows(const double *d_F, int64_t f_rows, const double *d_G, double *d_X, int64_t n_rows, int32_t d,
                                   int32_t ld, const int64_t *d_indptr, const int32_t *d_indices, const double *d_c, double lambda,
                                   double *d_loss, void *d_ws, int64_t ws_bytes, void *stream) {
    QREC_REQUIRE(d >= 1 && d <= QREC_ALS_MAX_D && valid_ld(ld) && d <= ld,
                 "qrec_als_solve_rows: need 1 <= d <= ld, ld in {16,32,64,128} (d %d, ld %d)", d, ld);
    QREC_REQUIRE(n_rows >= 0 && f_rows >= 0, "qrec_als_solve_rows: negative row count");
    QREC_REQUIRE(lambda >= 0.0 && lambda <= 1.79769313486231570e308, "qrec_als_solve_rows: lambda must be finite and >= 0 (%g)", lambda);
    QREC_REQUIRE(d_G && d_X && d_indptr && d_ws && (d_F || f_rows == 0) && d_indices && d_c,
                 "qrec_als_solve_rows: null pointer");
    Carver c(d_ws);
    const SolveWs w = solve_layout(c, ws_bytes, n_rows, ld);
    QREC_REQUIRE(ws_bytes >= (int64_t)c.bytes(), "qrec_als_solve_rows: workspace of %lld bytes is too small", (long long)ws_bytes);
    if (n_rows == 0) {
        if (d_loss) QREC_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), as_stream(stream)));
        return QREC_OK;
    }
    hipStream_t st = as_stream(stream);
    const int with_loss = d_loss != nullptr;
    als_plan_kernel<<<1, 1024, 0, st>>>(d_indptr, n_rows, w);
    QREC_LAUNCH_CHECK();
    switch (ld) {
        case 16: launch_solve<1>(d_F, f_rows, d_G, d_X, n_rows, d, d_indptr, d_indices, d_c, lambda, with_loss, w, st); break;
        case 32: launch_solve<2>(d_F, f_rows, d_G, d_X, n_rows, d, d_indptr, d_indices, d_c, lambda, with_loss, w, st); break;
        case 64: launch_solve<4>(d_F, f_rows, d_G, d_X, n_rows, d, d_indptr, d_indices, d_c, lambda, with_loss, w, st); break;
        default: launch_solve<8>(d_F, f_rows, d_G, d_X, n_rows, d, d_indptr, d_indices, d_c, lambda, with_loss, w, st); break;
    }
    QREC_LAUNCH_CHECK();
    const int64_t n_elems = n_rows * ld;
    als_commit_kernel<<<(unsigned)std::min<int64_t>((n_elems + kThreads - 1) / kThreads, 2048), kThreads, 0, st>>>(d_X, n_elems, w);
    QREC_LAUNCH_CHECK();
    if (with_loss) {
        als_loss_kernel<<<1, kThreads, 0, st>>>(n_rows, w, d_loss);
        QREC_LAUNCH_CHECK();
    }
    int status[2];
    QREC_HIP_CHECK(hipMemcpyAsync(status, w.status, sizeof(status), hipMemcpyDeviceToHost, st));
    QREC_HIP_CHECK(hipStreamSynchronize(st));
    switch (status[0]) {
        case kOk: return QREC_OK;
        case kNotSpd:
            set_error("qrec_als_solve_rows: the system of row %d is not positive definite (non-positive pivot); nothing written", status[1]);
            return QREC_ERR_NOT_SPD;
        case kWorkspace:
            set_error("qrec_als_solve_rows: workspace too small for the split rows (see qrec_als_solve_workspace_bytes); nothing written");
            return QREC_ERR_INVALID;
        case kBadIndex:
            set_error("qrec_als_solve_rows: a column index is outside [0, f_rows); nothing written");
            return QREC_ERR_INVALID;
        default:
            set_error("qrec_als_solve_rows: indptr must start at 0 and never decrease; nothing written");
            return QREC_ERR_INVALID;
    }
}
