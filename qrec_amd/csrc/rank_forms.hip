// Ranking of the rating models whose score is not one plain inner product (predictForRanking of model/rating/{SVD,SVDPlusPlus,
// EE,SREE,RSTE,SocialFD}.py), fp64, no float atomics, the same bits from launch to launch.  Every one of the six scores is an
// inner product or a squared distance of two tables plus rank-one terms, so the block route of the evaluation (eval_block.hip)
// ranks them with its scoring step replaced by the one in this file; mask and top-N run unchanged.
//
//   form      score of (user u, item i)                                        user operand row             item operand
//   DOT       Q[i].P[u]                                                        P[u]                         Q
//   BIASED    ((Q[i].e + mu) + Bi[i]) + Bu[u]                     (SVD)        e = P[u]                     Q
//   SVDPP     the same                                            (SVD++)      e = P[u] + (sum_j Y[j]) / w  Q
//   EUCLID    ((sign * |Q[i] - P[u]|^2 + Bi[i]) + Bu[u]) + mu     (EE, SREE)   P[u]                         Q
//   METRIC    the same on the projected rows                      (SocialFD)   P[u].H                       Q.H
//   RSTE      Q[i].e                                                           e = alpha P[u] + ((1 - alpha) sum_f w_f P[f]) / den[u],
//                                                                              P[u] where den[u] == 0       Q
// with |x - y|^2 = (|y|^2 - 2 y.x) + |x|^2 taken from the inner product the MFMA tile loop forms: the distance costs the matrix
// pipe what a dot costs and two loads per stored score (DESIGN.md on why not direct differences).
//
//   * rank_user_rows_kernel: one wavefront per batch row b (lane = column, lane_row.h) writes the operand row, its squared norm
//     and Bu[u] into the call's workspace, in batch order; rows b >= n_b of the 64-user pad are written as zeros.  SVD++'s sum
//     runs over the user's rated items in userRated order, RSTE's over its followees in CSR order, element-wise sequential adds.
//   * rank_project_kernel: rows . H with H staged in LDS as [d][d | 1] doubles (social.hip's odd row stride), every output
//     column a sum over k = 0 .. d-1 in order; Q.H once per table upload (qrec_rank_form_prepare), P[u].H per batch.
//   * rank_row_norms_kernel: |row|^2 of the item operand, once per table upload.
//   * score_form_kernel: score_tiles_f64 (eval_tile.h) -- the tile loop of score_kernel_f64 -- over the staged operand with the
//     form's epilogue applied to the finished accumulator before the transposed store.
#include "eval_tile.h"
#include "lane_row.h"

using namespace qrec;

namespace {

constexpr int kWaves = 8;                 // wavefronts (= rows in flight) per workgroup of the row kernels
constexpr int kBlock = 64 * kWaves;
constexpr int kMaxBlocks = 1024;

inline int row_grid(int64_t rows) {
    const int64_t blocks = (rows + kWaves - 1) / kWaves;
    return (int)(blocks < kMaxBlocks ? (blocks > 0 ? blocks : 1) : kMaxBlocks);
}

__device__ inline int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// what one wavefront hands its own lanes through LDS: the LDS unit serves a wavefront's accesses in issue order
__device__ inline void wave_lds_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// the staged user side of one call: operand rows [b_pad][ld] in batch order, their squared norms and Bu[user] per batch slot
struct FormWs { double *rows, *norm, *bu; };
FormWs form_layout(Carver &c, int n_b, int ld) {
    const size_t b_pad = ((size_t)n_b + 63) / 64 * 64;
    FormWs w;
    w.rows = c.take<double>(b_pad * (size_t)ld, 256);
    w.norm = c.take<double>(b_pad);
    w.bu = c.take<double>(b_pad);
    c.pad(256);
    return w;
}

// columns [d, ld) of a staged row: the tile loop reads whole 16-column slots
__device__ inline void zero_pad_columns(double *row, int lane, int d, int ld) {
    for (int cidx = d + lane; cidx < ld; cidx += 64) row[cidx] = 0.0;
}

template <int EPL, int FORM>      // FORM: QREC_RATING_DOT (plain gather: DOT, BIASED, EUCLID), QREC_RATING_SVDPP, QREC_RATING_RSTE
__global__ __launch_bounds__(kBlock) void rank_user_rows_kernel(const FormScore f, const int32_t *__restrict__ user_ids, int n_b, int b_pad,
                                                                int n_items, FormWs w) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const LaneRow<double, EPL> R(lane, f.d, f.ld);
    const int stride = gridDim.x * kWaves;
    for (int b = blockIdx.x * kWaves + (threadIdx.x >> 6); b < b_pad; b += stride) {
        double e[EPL];
#pragma unroll
        for (int k = 0; k < EPL; k++) e[k] = 0.0;
        double bu = 0.0;
        const int u = b < n_b ? wave_uniform(user_ids[b]) : -1;
        if (u >= 0 && u < f.n_users) {
            R.load(e, f.P, u);
            if (f.Bu) bu = f.Bu[u];
            if constexpr (FORM == QREC_RATING_SVDPP) {
                const int64_t beg = f.y_indptr[u], end = f.y_indptr[u + 1];
                if (end > beg) {
                    double acc[EPL], y[EPL];
#pragma unroll
                    for (int k = 0; k < EPL; k++) acc[k] = 0.0;
                    for (int64_t t = beg; t < end; t++) {
                        const int j = wave_uniform(f.y_items[t]);
                        if (j < 0 || j >= n_items) continue;
                        R.load(y, f.Y, j);
#pragma unroll
                        for (int k = 0; k < EPL; k++) acc[k] = acc[k] + y[k];
                    }
                    const double cnt = (double)(end - beg);
#pragma unroll
                    for (int k = 0; k < EPL; k++) e[k] = e[k] + acc[k] / cnt;
                }
            } else if constexpr (FORM == QREC_RATING_RSTE) {
                const double den = f.fe_den[u];
                if (den != 0.0) {
                    double acc[EPL], p[EPL];
#pragma unroll
                    for (int k = 0; k < EPL; k++) acc[k] = 0.0;
                    for (int64_t t = f.fe_indptr[u]; t < f.fe_indptr[u + 1]; t++) {
                        const int v = wave_uniform(f.fe_ids[t]);
                        if (v < 0 || v >= f.n_users) continue;
                        const double wt = f.fe_w[t];
                        R.load(p, f.P, v);
#pragma unroll
                        for (int k = 0; k < EPL; k++) acc[k] = acc[k] + wt * p[k];
                    }
#pragma unroll
                    for (int k = 0; k < EPL; k++) e[k] = f.alpha * e[k] + ((1.0 - f.alpha) * acc[k]) / den;
                }
            }
        }
        R.store(w.rows, b, e);
        zero_pad_columns(w.rows + (int64_t)b * f.ld, lane, f.d, f.ld);
        const double nrm = row_dot(e, e);
        if (lane == 0) { w.norm[b] = nrm; w.bu[b] = bu; }
    }
}

size_t project_lds_bytes(int d) { return ((size_t)d * (d | 1) + (size_t)kWaves * d) * sizeof(double); }

// out[r] = X[src(r)] . H for r < n (src = ids[r], or r itself when ids is null), zero rows for n <= r < n_out; norm[r] = |out[r]|^2;
// bu_out[r] = Bu[src(r)] when asked for.  A source row outside [0, n_src) gives a zero row and is never dereferenced.
template <int EPL>
__global__ __launch_bounds__(kBlock) void rank_project_kernel(const double *__restrict__ X, int n_src, const int32_t *__restrict__ ids, int n,
                                                              int n_out, const double *__restrict__ Hg, int d, int ld,
                                                              double *__restrict__ out, double *__restrict__ norm,
                                                              const double *__restrict__ Bu, double *__restrict__ bu_out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int ldh = d | 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *H = reinterpret_cast<double *>(smem);
    double *xv = H + (size_t)d * ldh + (size_t)wave * d;
    for (int idx = threadIdx.x; idx < d * d; idx += kBlock) H[(idx / d) * ldh + idx % d] = Hg[idx];
    __syncthreads();
    const LaneRow<double, EPL> R(lane, d, ld);
    const int stride = gridDim.x * kWaves;
    for (int r = blockIdx.x * kWaves + wave; r < n_out; r += stride) {
        double y[EPL];
#pragma unroll
        for (int k = 0; k < EPL; k++) y[k] = 0.0;
        double bu = 0.0;
        const int src = r < n ? (ids ? wave_uniform(ids[r]) : r) : -1;
        if (src >= 0 && src < n_src) {
            double x[EPL];
            R.load(x, X, src);
            if (Bu) bu = Bu[src];
#pragma unroll
            for (int k = 0; k < EPL; k++)
                if (R.valid(k)) xv[lane + 64 * k] = x[k];
            wave_lds_fence();
#pragma unroll
            for (int k = 0; k < EPL; k++) {                         // x.H: lane = column
                const int o = lane + 64 * k;
                if (o < d) {
                    double acc = 0.0;
                    for (int j = 0; j < d; j++) acc += xv[j] * H[j * ldh + o];
                    y[k] = acc;
                }
            }
            wave_lds_fence();                                        // the next row rewrites xv
        }
        R.store(out, r, y);
        zero_pad_columns(out + (int64_t)r * ld, lane, d, ld);
        const double nrm = row_dot(y, y);
        if (lane == 0) {
            norm[r] = nrm;
            if (bu_out) bu_out[r] = bu;
        }
    }
}

template <int EPL>
__global__ __launch_bounds__(kBlock) void rank_row_norms_kernel(const double *__restrict__ X, int n, int d, int ld, double *__restrict__ norm) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const LaneRow<double, EPL> R(lane, d, ld);
    const int stride = gridDim.x * kWaves;
    for (int r = blockIdx.x * kWaves + (threadIdx.x >> 6); r < n; r += stride) {
        double x[EPL];
        R.load(x, X, r);
        const double nrm = row_dot(x, x);
        if (lane == 0) norm[r] = nrm;
    }
}

// ---- the epilogues: (inner product, item, batch slot) -> score.  2 * dot and sign * dist are exact, so the value does not depend
// on whether the compiler contracts them into the neighbouring add.
struct BiasedScore {            // SVD.py:88, SVDPlusPlus.py:103
    const double *Bi, *bu; double mu;
    __device__ __forceinline__ double operator()(double dot, int item, int b) const { return ((dot + mu) + Bi[item]) + bu[b]; }
};
struct DistanceScore {          // EE.py:93, SREE.py:77 (sign +1); SocialFD.py:111 (sign -1, projected rows)
    const double *nq, *np, *Bi, *bu; double mu, sign;
    __device__ __forceinline__ double operator()(double dot, int item, int b) const {
        const double dist = (nq[item] - 2.0 * dot) + np[b];
        return ((sign * dist + Bi[item]) + bu[b]) + mu;
    }
};

template <typename Epi>
__global__ __launch_bounds__(256) void score_form_kernel(const double *__restrict__ rows, const double *__restrict__ V, int ld, int n_items,
                                                         int b_pad, int item_tiles_per_wave, double *__restrict__ S_T, const Epi epi) {
    // the staged operand is in batch order and padded to b_pad zero rows: lane (r, h) reads row utile * 16 + r
    score_tiles_f64(rows, (int64_t)blockIdx.x * 16 + (threadIdx.x & 15), V, ld, n_items, b_pad, item_tiles_per_wave, S_T, epi);
}

template <typename Epi>
int launch_score_form(const double *rows, const double *V, int ld, int n_items, int n_b, int b_pad, double *S_T, const Epi &epi, hipStream_t st) {
    int per_wave;
    const dim3 grid = score_grid(n_b, (n_items + 15) / 16, 16, 8, &per_wave);
    hipLaunchKernelGGL(score_form_kernel<Epi>, grid, dim3(256), 0, st, rows, V, ld, n_items, b_pad, per_wave, S_T, epi);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int launch_project(const double *X, int n_src, const int32_t *ids, int n, int n_out, const double *H, int d, int ld, double *out, double *norm,
                   const double *Bu, double *bu_out, hipStream_t st) {
    const size_t lds = project_lds_bytes(d);
    return with_epl<2>(d, [&](auto epl) {
        if (lds > 64 * 1024)
            QREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rank_project_kernel<epl()>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(rank_project_kernel<epl()>, dim3(row_grid(n_out)), dim3(kBlock), lds, st, X, n_src, ids, n, n_out, H, d, ld, out,
                           norm, Bu, bu_out);
        QREC_LAUNCH_CHECK();
        return (int)QREC_OK;
    });
}

// the item side of a form, made once per table upload: METRIC: Q.H [n_items][ld] then its norms; EUCLID: the norms of Q; else nothing
struct PrepWs { double *rows, *norm; };
PrepWs prep_layout(Carver &c, int form, int n_items, int ld) {
    PrepWs w{nullptr, nullptr};
    if (form == QREC_RATING_METRIC) w.rows = c.take<double>((size_t)n_items * ld, 256);
    if (form == QREC_RATING_METRIC || form == QREC_RATING_EUCLID) { w.norm = c.take<double>((size_t)n_items, 256); c.pad(256); }
    return w;
}

bool known_form(int form) { return form >= QREC_RATING_DOT && form <= QREC_RATING_RSTE; }

int refuse_wide_metric(const char *fn, int form, int d) {
    if (form == QREC_RATING_METRIC && d > QREC_SOCIAL_H_MAX_D) {
        set_error("%s: width %d above the supported %d (H stays in LDS)", fn, d, QREC_SOCIAL_H_MAX_D);
        return QREC_ERR_UNSUPPORTED;
    }
    return QREC_OK;
}

}  // namespace

namespace qrec {

int64_t form_operand_bytes(int n_b, int ld) { return layout_bytes(form_layout, n_b, ld); }

int score_block_form(double *S_T, const FormScore &f, int n_items, const int32_t *user_ids, int n_b, int b_pad, hipStream_t st) {
    const FormWs w = carve(f.ws, form_layout, n_b, f.ld);
    if (f.form == QREC_RATING_METRIC) {
        const int rc = launch_project(f.P, f.n_users, user_ids, n_b, b_pad, f.H, f.d, f.ld, w.rows, w.norm, f.Bu, w.bu, st);
        if (rc != QREC_OK) return rc;
    } else {
        const int rc = with_epl(f.d, [&](auto epl) {
            auto launch = [&](auto fc) {
                hipLaunchKernelGGL((rank_user_rows_kernel<epl(), fc()>), dim3(row_grid(b_pad)), dim3(kBlock), 0, st, f, user_ids, n_b, b_pad,
                                   n_items, w);
                QREC_LAUNCH_CHECK();
                return (int)QREC_OK;
            };
            switch (f.form) {
                case QREC_RATING_SVDPP: return launch(int_c<QREC_RATING_SVDPP>{});
                case QREC_RATING_RSTE: return launch(int_c<QREC_RATING_RSTE>{});
                default: return launch(int_c<QREC_RATING_DOT>{});
            }
        });
        if (rc != QREC_OK) return rc;
    }
    switch (f.form) {
        case QREC_RATING_BIASED:
        case QREC_RATING_SVDPP:
            return launch_score_form(w.rows, f.item_op, f.ld, n_items, n_b, b_pad, S_T, BiasedScore{f.Bi, w.bu, f.mu}, st);
        case QREC_RATING_EUCLID:
        case QREC_RATING_METRIC:
            return launch_score_form(w.rows, f.item_op, f.ld, n_items, n_b, b_pad, S_T, DistanceScore{f.item_norm, w.norm, f.Bi, w.bu, f.mu, f.sign},
                                     st);
        default:
            return launch_score_form(w.rows, f.item_op, f.ld, n_items, n_b, b_pad, S_T, PlainScore{}, st);
    }
}

}  // namespace qrec

extern "C" {

int qrec_rank_form_prepare_bytes(int32_t form, int32_t n_items, int32_t ld, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_items >= 0 && ld >= 1, "qrec_rank_form_prepare_bytes: bad arguments");
    QREC_REQUIRE(known_form(form), "qrec_rank_form_prepare_bytes: unknown form %d", form);
    *bytes = layout_bytes(prep_layout, form, n_items, ld);
    return QREC_OK;
}

int qrec_rank_form_prepare(int32_t form, const double *d_Q, const double *d_H, int32_t d, int32_t ld, int32_t n_items, void *d_prep,
                           int64_t prep_bytes, void *stream) {
    QREC_REQUIRE(known_form(form), "qrec_rank_form_prepare: unknown form %d", form);
    QREC_REQUIRE(d_Q && n_items >= 1, "qrec_rank_form_prepare: null table or no items");
    if (int rc = check_lane_row("qrec_rank_form_prepare", QREC_F64, d, ld)) return rc;
    QREC_REQUIRE(ld % 16 == 0, "qrec_rank_form_prepare: the row stride must be a multiple of 16 doubles, pad columns zero (got ld=%d)", ld);
    if (int rc = refuse_wide_metric("qrec_rank_form_prepare", form, d)) return rc;
    QREC_REQUIRE(form != QREC_RATING_METRIC || d_H, "qrec_rank_form_prepare: METRIC needs H");
    const int64_t need = layout_bytes(prep_layout, form, n_items, ld);
    QREC_REQUIRE(prep_bytes >= need && (need == 0 || d_prep), "qrec_rank_form_prepare: the buffer holds %lld bytes, the form needs %lld",
                 (long long)prep_bytes, (long long)need);
    if (need == 0) return QREC_OK;
    const PrepWs w = carve(d_prep, prep_layout, form, n_items, ld);
    hipStream_t st = as_stream(stream);
    if (form == QREC_RATING_METRIC)
        return launch_project(d_Q, n_items, nullptr, n_items, n_items, d_H, d, ld, w.rows, w.norm, nullptr, nullptr, st);
    return with_epl(d, [&](auto epl) {
        hipLaunchKernelGGL(rank_row_norms_kernel<epl()>, dim3(row_grid(n_items)), dim3(kBlock), 0, st, d_Q, n_items, d, ld, w.norm);
        QREC_LAUNCH_CHECK();
        return (int)QREC_OK;
    });
}

int qrec_score_topk_form_scratch_bytes(int32_t form, int32_t n_items, int32_t n_batch_users, int32_t ld, int32_t N, int64_t *bytes) {
    QREC_REQUIRE(bytes && n_items >= 0 && n_batch_users >= 0 && ld >= 1, "qrec_score_topk_form_scratch_bytes: bad arguments");
    QREC_REQUIRE(known_form(form), "qrec_score_topk_form_scratch_bytes: unknown form %d", form);
    (void)N;                                    // the block route's scratch does not depend on N; kept for the neighbouring query's shape
    *bytes = (int64_t)align_up((size_t)block_path_bytes(QREC_F64, n_items, n_batch_users), 256) + form_operand_bytes(n_batch_users, ld);
    return QREC_OK;
}

int qrec_score_topk_form(int32_t form, double sign, const double *d_P, const double *d_Q, int32_t d, int32_t ld, int32_t n_users,
                         int32_t n_items, const double *d_Bu, const double *d_Bi, double mu, const double *d_Y,
                         const int64_t *d_y_indptr, const int32_t *d_y_items, const double *d_H, const int64_t *d_fe_indptr,
                         const int32_t *d_fe_ids, const double *d_fe_w, const double *d_fe_den, double alpha, const void *d_prep,
                         int64_t prep_bytes, const int32_t *d_user_ids, int32_t n_batch_users, const int64_t *d_rated_indptr,
                         const int32_t *d_rated_items, int32_t N, void *d_scratch, int64_t scratch_bytes, int32_t *d_ids_out,
                         double *d_scores_out, void *stream) {
    QREC_REQUIRE(known_form(form), "qrec_score_topk_form: unknown form %d", form);
    QREC_REQUIRE(d_P && d_Q && d_user_ids && d_scratch && d_ids_out && d_scores_out, "qrec_score_topk_form: null argument");
    QREC_REQUIRE(n_users >= 1 && n_items >= 1 && n_batch_users >= 0, "qrec_score_topk_form: bad sizes");
    if (int rc = check_lane_row("qrec_score_topk_form", QREC_F64, d, ld)) return rc;
    QREC_REQUIRE(ld % 16 == 0, "qrec_score_topk_form: the row stride must be a multiple of 16 doubles, pad columns zero (got ld=%d)", ld);
    QREC_REQUIRE(N >= 1 && N <= 100, "qrec_score_topk_form: N must be in 1..100 (base/recommender.py:132-134)");
    QREC_REQUIRE((d_rated_indptr == nullptr) == (d_rated_items == nullptr), "qrec_score_topk_form: rated CSR incomplete");
    if (int rc = refuse_wide_metric("qrec_score_topk_form", form, d)) return rc;
    const bool biased = form != QREC_RATING_DOT && form != QREC_RATING_RSTE, distance = form == QREC_RATING_EUCLID || form == QREC_RATING_METRIC;
    QREC_REQUIRE(!biased || (d_Bu && d_Bi), "qrec_score_topk_form: form %d needs Bu and Bi", form);
    QREC_REQUIRE(!distance || sign == 1.0 || sign == -1.0, "qrec_score_topk_form: the distance forms take sign +1 or -1 (got %g)", sign);
    QREC_REQUIRE(form != QREC_RATING_SVDPP || (d_Y && d_y_indptr && d_y_items), "qrec_score_topk_form: SVDPP needs Y and the userRated CSR");
    QREC_REQUIRE(form != QREC_RATING_METRIC || d_H, "qrec_score_topk_form: METRIC needs H");
    QREC_REQUIRE(form != QREC_RATING_RSTE || (d_fe_indptr && d_fe_ids && d_fe_w && d_fe_den), "qrec_score_topk_form: RSTE needs the followee CSR");
    const int64_t need_prep = layout_bytes(prep_layout, form, n_items, ld);
    QREC_REQUIRE(prep_bytes >= need_prep && (need_prep == 0 || d_prep),
                 "qrec_score_topk_form: the prepared item buffer holds %lld bytes, the form needs %lld (qrec_rank_form_prepare)",
                 (long long)prep_bytes, (long long)need_prep);
    const size_t block_bytes = align_up((size_t)block_path_bytes(QREC_F64, n_items, n_batch_users), 256);
    const int64_t need = (int64_t)block_bytes + form_operand_bytes(n_batch_users, ld);
    QREC_REQUIRE(scratch_bytes >= need, "qrec_score_topk_form: the scratch holds %lld bytes, the call needs %lld", (long long)scratch_bytes,
                 (long long)need);
    if (n_batch_users == 0) return QREC_OK;
    const PrepWs prep = carve(const_cast<void *>(d_prep), prep_layout, form, n_items, ld);
    const FormScore f{form, sign, mu, alpha, d_P, form == QREC_RATING_METRIC ? prep.rows : d_Q, prep.norm, d, ld, n_users, d_Bu, d_Bi, d_Y,
                      d_y_indptr, d_y_items, d_H, d_fe_indptr, d_fe_ids, d_fe_w, d_fe_den, static_cast<char *>(d_scratch) + block_bytes};
    return run_score_topk(QREC_F64, nullptr, nullptr, ld, n_items, d_user_ids, n_batch_users, d_rated_indptr, d_rated_items, N, d_scratch,
                          d_ids_out, d_scores_out, as_stream(stream), nullptr, nullptr, &f);
}

}  // extern "C"
