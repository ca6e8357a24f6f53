// Evaluation of the rating models on the device (base/recommender.py:88-110, base/iterativeRecommender.py:65-73,103-113 and
// every rating class's predictForRating), fp64, no float atomics, the same bits from launch to launch.
//
//   * rating_implicit_kernel: SVD++'s imp[u] = (...((Y[j0] + Y[j1]) + Y[j2])...) / count over the user's rated items in
//     userRated order (SVDPlusPlus.py:72-81), once per distinct test user.  Element-wise sequential adds: the host's bits.
//   * rating_predict_kernel: one wavefront per test pair, lane = column (lane_row.h), in a grid-stride loop.  A dot product
//     is row_dot's fixed tree, every scalar sum after it is added left to right as the class's predictForRating adds it.
//   * rating_metric_kernel: SocialFD's form.  H is staged in LDS as [d][d | 1] doubles (the odd row stride of social.hip:
//     lane = column reads consecutive addresses, lane = row reads stride d | 1, both conflict-free) once per workgroup;
//     each wavefront then evaluates its pairs on its own, handing diff and diff.H to its other lanes through two LDS
//     vectors of its own.  Every lane's sum runs over k = 0 .. d-1 in order, so the bits depend on d alone.
//   * rating_boundary_kernel: checkRatingBoundary in place -- clamp to the scale, else Python's round(x, 3).
//   * rating_errors_kernel: |r - p| and (r - p)(r - p) per pair into two slot arrays, which qrec_loss_fold (social.hip) adds
//     in pair order, as Python's sum() does.
// An id of -1 is a name the training set does not know; any id outside its table is treated the same way and never
// dereferenced (the engine refuses such ids before anything is launched).
#include "lane_row.h"

using namespace qrec;

namespace {

constexpr int kWaves = QREC_RATING_BLOCK_WAVES;      // wavefronts (= pairs in flight) per workgroup
constexpr int kBlock = 64 * kWaves;

struct RatingArgs {
    const double *P, *Q, *Bu, *Bi, *aux;             // aux: imp [n_users][ld] (SVDPP) or H [d][d] (METRIC)
    const int64_t *fe_ptr; const int32_t *fe_ids; const double *fe_w, *fe_den;
    const double *umean, *imean; double gmean, alpha;
    const int32_t *uid, *iid; int64_t n; double *pred;
    int n_users, n_items, d, ld;
};

inline int rating_grid(int64_t work_items, int per_block) {
    const int64_t blocks = (work_items + per_block - 1) / per_block;
    return (int)(blocks < QREC_RATING_MAX_BLOCKS ? blocks : QREC_RATING_MAX_BLOCKS);
}

// a value every lane of the wavefront holds, as a scalar: the branches on it are then uniform for the compiler too
__device__ inline int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// what one wavefront hands its own lanes through LDS: the LDS unit serves a wavefront's accesses in issue order
__device__ inline void wave_lds_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

template <int EPL>
__global__ __launch_bounds__(kBlock) void rating_implicit_kernel(const double *__restrict__ Y, int d, int ld, int n_items,
                                                                 const int64_t *__restrict__ indptr, const int32_t *__restrict__ items,
                                                                 const int32_t *__restrict__ users, int64_t n, int n_users,
                                                                 double *__restrict__ imp) {
#pragma clang fp contract(off)
    const LaneRow<double, EPL> R(threadIdx.x & 63, d, ld);
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t < n; t += stride) {
        const int u = wave_uniform(users[t]);
        if (u < 0 || u >= n_users) continue;
        const int64_t b = indptr[u], en = indptr[u + 1];
        double acc[EPL], y[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) acc[e] = 0.0;
        for (int64_t k = b; k < en; k++) {
            const int j = wave_uniform(items[k]);
            if (j < 0 || j >= n_items) continue;
            R.load(y, Y, j);
#pragma unroll
            for (int e = 0; e < EPL; e++) acc[e] = acc[e] + y[e];
        }
        const double cnt = (double)(en - b);
        if (en > b) {
#pragma unroll
            for (int e = 0; e < EPL; e++) acc[e] = acc[e] / cnt;
        }
        R.store(imp, u, acc);
    }
}

template <int EPL, int FORM>
__global__ __launch_bounds__(kBlock) void rating_predict_kernel(const RatingArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const LaneRow<double, EPL> R(lane, a.d, a.ld);
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t < a.n; t += stride) {
        const int u = wave_uniform(a.uid[t]), i = wave_uniform(a.iid[t]);
        const bool ku = u >= 0 && u < a.n_users, ki = i >= 0 && i < a.n_items;
        double pred;
        if (!(ku && ki)) {
            if constexpr (FORM == QREC_RATING_DOT) pred = ku ? a.umean[u] : ki ? a.imean[i] : a.gmean;
            else pred = a.gmean;
        } else {
            double p[EPL], q[EPL];
            R.load2(p, a.P, u, q, a.Q, i);
            if constexpr (FORM == QREC_RATING_DOT) {
                pred = row_dot(p, q);
            } else if constexpr (FORM == QREC_RATING_BIASED) {
                pred = ((row_dot(p, q) + a.gmean) + a.Bi[i]) + a.Bu[u];
            } else if constexpr (FORM == QREC_RATING_SVDPP) {
                double m[EPL];
                R.load(m, a.aux, u);
                const double imp = row_dot(m, q);
                pred = imp + (((row_dot(p, q) + a.gmean) + a.Bi[i]) + a.Bu[u]);
            } else if constexpr (FORM == QREC_RATING_EUCLID) {
                double df[EPL];
#pragma unroll
                for (int e = 0; e < EPL; e++) df[e] = p[e] - q[e];
                pred = ((a.gmean + a.Bi[i]) + a.Bu[u]) - row_dot(df, df);
            } else {                                                       // QREC_RATING_RSTE, as rste_ordered_kernel predicts
                const double dot = row_dot(p, q), den = a.fe_den[u];
                pred = dot;
                if (den != 0.0) {
                    double fpred = 0.0, f[EPL];
                    for (int64_t k = a.fe_ptr[u]; k < a.fe_ptr[u + 1]; k++) {
                        const int v = wave_uniform(a.fe_ids[k]);
                        if (v < 0 || v >= a.n_users) continue;
                        R.load(f, a.P, v);
                        fpred += a.fe_w[k] * row_dot(f, q);
                    }
                    pred = a.alpha * dot + ((1.0 - a.alpha) * fpred) / den;
                }
            }
        }
        if (lane == 0) a.pred[t] = pred;
    }
}

size_t metric_lds_bytes(int d) { return ((size_t)d * (d | 1) + 2 * (size_t)kWaves * d) * sizeof(double); }

// ((Bi + Bu) + mean) - ((diff.H).H^T).diff (SocialFD.py:104-108)
template <int EPL>
__global__ __launch_bounds__(kBlock) void rating_metric_kernel(const RatingArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int d = a.d, ldh = d | 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *H = reinterpret_cast<double *>(smem);
    double *xv = H + (size_t)d * ldh + (size_t)wave * 2 * d, *tv = xv + d;
    for (int idx = threadIdx.x; idx < d * d; idx += kBlock) H[(idx / d) * ldh + idx % d] = a.aux[idx];
    __syncthreads();
    const LaneRow<double, EPL> R(lane, d, a.ld);
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < a.n; t += stride) {
        const int u = wave_uniform(a.uid[t]), i = wave_uniform(a.iid[t]);
        double pred = a.gmean;
        if (u >= 0 && u < a.n_users && i >= 0 && i < a.n_items) {
            double p[EPL], q[EPL], df[EPL], s[EPL];
            R.load2(p, a.P, u, q, a.Q, i);
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                df[e] = p[e] - q[e];
                if (R.valid(e)) xv[lane + 64 * e] = df[e];
            }
            wave_lds_fence();
#pragma unroll
            for (int e = 0; e < EPL; e++) {                          // diff.H: lane = column
                const int o = lane + 64 * e;
                if (o < d) {
                    double acc = 0.0;
                    for (int k = 0; k < d; k++) acc += xv[k] * H[k * ldh + o];
                    tv[o] = acc;
                }
            }
            wave_lds_fence();
#pragma unroll
            for (int e = 0; e < EPL; e++) {                          // (diff.H).H^T: lane = row
                const int o = lane + 64 * e;
                double acc = 0.0;
                if (o < d)
                    for (int k = 0; k < d; k++) acc += tv[k] * H[o * ldh + k];
                s[e] = acc;
            }
            wave_lds_fence();                                        // the next pair rewrites xv and tv
            pred = ((a.Bi[i] + a.Bu[u]) + a.gmean) - row_dot(s, df);
        }
        if (lane == 0) a.pred[t] = pred;
    }
}

// checkRatingBoundary (base/recommender.py:88-95): above hi -> hi, below lo -> lo, else round(x, 3).  Python rounds the
// exact decimal value of the double half to even.  y = x * 1000 rounded and e = the exact residual of that product place
// x * 1000 against k + 1/2 exactly (k + 1/2 is a double, and rounding is monotonic); k / 1000 is then the double nearest
// the decimal, IEEE division being correctly rounded.
__device__ inline double rating_boundary(double x, double lo, double hi) {
#pragma clang fp contract(off)
    if (x > hi) return hi;
    if (x < lo) return lo;
    const double y = x * 1000.0;
    const double e = __builtin_fma(x, 1000.0, -y);
    const double k = floor(y), f = y - k;
    const bool odd = ((long long)k & 1) != 0;
    const bool up = f > 0.5 || (f == 0.5 && (e > 0.0 || (e == 0.0 && odd)));
    return (up ? k + 1.0 : k) / 1000.0;
}

__global__ __launch_bounds__(kBlock) void rating_boundary_kernel(double *__restrict__ x, int64_t n, double lo, double hi) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += stride) x[t] = rating_boundary(x[t], lo, hi);
}

__global__ __launch_bounds__(kBlock) void rating_errors_kernel(const double *__restrict__ rating, const double *__restrict__ pred,
                                                               int64_t n, double *__restrict__ abs_err, double *__restrict__ sq_err) {
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += stride) {
        const double e = rating[t] - pred[t];
        abs_err[t] = fabs(e);
        sq_err[t] = e * e;
    }
}

}  // namespace

int qrec_rating_implicit(const double *d_Y, int32_t dtype, int32_t n_items, int32_t d, int32_t ld, const int64_t *d_rated_indptr,
                         const int32_t *d_rated_items, const int32_t *d_users, int64_t n, int32_t n_users, double *d_imp,
                         void *stream) {
    QREC_REQUIRE(dtype == QREC_F64, "qrec_rating_implicit: fp64 tables only (got dtype %d)", dtype);
    QREC_REQUIRE(d_Y && d_imp && n >= 0 && n_users >= 0 && n_items >= 0, "qrec_rating_implicit: null argument");
    QREC_REQUIRE(n == 0 || (d_rated_indptr && d_rated_items && d_users), "qrec_rating_implicit: null index array");
    if (int rc = check_lane_row("qrec_rating_implicit", QREC_F64, d, ld)) return rc;
    if (n == 0) return QREC_OK;
    return with_epl(d, [&](auto epl) {
        hipLaunchKernelGGL(rating_implicit_kernel<epl()>, dim3(rating_grid(n, kWaves)), dim3(kBlock), 0, as_stream(stream), d_Y, d, ld,
                           n_items, d_rated_indptr, d_rated_items, d_users, n, n_users, d_imp);
        QREC_LAUNCH_CHECK();
        return (int)QREC_OK;
    });
}

int qrec_rating_predict(int32_t form, int32_t dtype, const double *d_P, const double *d_Q, int32_t n_users, int32_t n_items, int32_t d,
                        int32_t ld, const double *d_Bu, const double *d_Bi, const double *d_aux, const int64_t *d_fe_indptr,
                        const int32_t *d_fe_ids, const double *d_fe_w, const double *d_fe_den, const double *d_user_mean,
                        const double *d_item_mean, double global_mean, double alpha, const int32_t *d_uid, const int32_t *d_iid,
                        int64_t n, double *d_pred, void *stream) {
    QREC_REQUIRE(form >= QREC_RATING_DOT && form <= QREC_RATING_RSTE, "qrec_rating_predict: unknown form %d", form);
    QREC_REQUIRE(dtype == QREC_F64, "qrec_rating_predict: fp64 tables only (got dtype %d)", dtype);
    QREC_REQUIRE(d_P && d_Q && n >= 0 && n_users >= 0 && n_items >= 0, "qrec_rating_predict: null argument");
    QREC_REQUIRE(n == 0 || (d_uid && d_iid && d_pred), "qrec_rating_predict: null pair array");
    if (int rc = check_lane_row("qrec_rating_predict", QREC_F64, d, ld)) return rc;
    if (form == QREC_RATING_METRIC && d > QREC_SOCIAL_H_MAX_D) {
        set_error("qrec_rating_predict: width %d above the supported %d (H stays in LDS)", d, QREC_SOCIAL_H_MAX_D);
        return QREC_ERR_UNSUPPORTED;
    }
    QREC_REQUIRE(form != QREC_RATING_DOT || (d_user_mean && d_item_mean), "qrec_rating_predict: DOT needs the user and item means");
    QREC_REQUIRE(form == QREC_RATING_DOT || form == QREC_RATING_RSTE || (d_Bu && d_Bi), "qrec_rating_predict: form %d needs Bu and Bi", form);
    QREC_REQUIRE((form != QREC_RATING_SVDPP && form != QREC_RATING_METRIC) || d_aux, "qrec_rating_predict: form %d needs its table (imp or H)",
                 form);
    QREC_REQUIRE(form != QREC_RATING_RSTE || (d_fe_indptr && d_fe_ids && d_fe_w && d_fe_den), "qrec_rating_predict: RSTE needs the followee CSR");
    if (n == 0) return QREC_OK;
    const RatingArgs a{d_P, d_Q, d_Bu, d_Bi, d_aux, d_fe_indptr, d_fe_ids, d_fe_w, d_fe_den, d_user_mean, d_item_mean, global_mean, alpha,
                       d_uid, d_iid, n, d_pred, n_users, n_items, d, ld};
    const dim3 grid(rating_grid(n, kWaves)), block(kBlock);
    hipStream_t st = as_stream(stream);
    if (form == QREC_RATING_METRIC) {
        const size_t lds = metric_lds_bytes(d);
        return with_epl<2>(d, [&](auto epl) {
            if (lds > 64 * 1024)
                QREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rating_metric_kernel<epl()>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(rating_metric_kernel<epl()>, grid, block, lds, st, a);
            QREC_LAUNCH_CHECK();
            return (int)QREC_OK;
        });
    }
    return with_epl(d, [&](auto epl) {
        auto launch = [&](auto f) {
            hipLaunchKernelGGL((rating_predict_kernel<epl(), f()>), grid, block, 0, st, a);
            QREC_LAUNCH_CHECK();
            return (int)QREC_OK;
        };
        switch (form) {
            case QREC_RATING_DOT: return launch(int_c<QREC_RATING_DOT>{});
            case QREC_RATING_BIASED: return launch(int_c<QREC_RATING_BIASED>{});
            case QREC_RATING_SVDPP: return launch(int_c<QREC_RATING_SVDPP>{});
            case QREC_RATING_EUCLID: return launch(int_c<QREC_RATING_EUCLID>{});
            default: return launch(int_c<QREC_RATING_RSTE>{});
        }
    });
}

int qrec_rating_boundary(double *d_x, int64_t n, double lo, double hi, void *stream) {
    QREC_REQUIRE(n >= 0 && (n == 0 || d_x), "qrec_rating_boundary: null argument");
    QREC_REQUIRE(lo <= hi, "qrec_rating_boundary: need lo <= hi (got %g, %g)", lo, hi);
    if (n == 0) return QREC_OK;
    hipLaunchKernelGGL(rating_boundary_kernel, dim3(rating_grid(n, kBlock)), dim3(kBlock), 0, as_stream(stream), d_x, n, lo, hi);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_rating_errors(const double *d_rating, const double *d_pred, int64_t n, double *d_abs, double *d_sq, void *stream) {
    QREC_REQUIRE(n >= 0 && (n == 0 || (d_rating && d_pred && d_abs && d_sq)), "qrec_rating_errors: null argument");
    if (n == 0) return QREC_OK;
    hipLaunchKernelGGL(rating_errors_kernel, dim3(rating_grid(n, kBlock)), dim3(kBlock), 0, as_stream(stream), d_rating, d_pred, n, d_abs,
                       d_sq);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}
