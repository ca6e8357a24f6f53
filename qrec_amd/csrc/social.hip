// Social-trust rating models (model/rating/{SoRec,SoReg,SocialMF,RSTE,SREE}.py), fp64, order-exact.
//
// The rating passes of SoRec / SoReg (PMF), SREE (EE) and SocialMF (PMF on copies) are mf_ordered_kernel of bpr_sgd.hip.
// Here are the rest:
//   * rste_ordered_kernel: RSTE's rating pass (RSTE.py:22-40,42-62), whose prediction blends P[u].Q[i] with the
//     followees' P[f].Q[i] -- one wavefront, lane = column, like mf_ordered_kernel;
//   * social_user_levels_kernel: the per-user social pass of SocialMF (SocialMF.py:25-41), SoReg (SoReg.py:58-74) and
//     SREE (SREE.py:50-63), one step per user of social.user that trains;
//   * sorec_levels_kernel: SoRec's pass over social.relation (SoRec.py:41-58), one step per relation;
//   * loss_fold_kernel: adds the per-step loss slots onto the running loss in the reference's order.
// The two social kernels run a LEVEL SCHEDULE (qrec_amd/social.py) in ONE workgroup of up to 16 wavefronts: every step of a
// level is independent of the others (no two touch a row one of them writes), every conflict points at least one level
// back.  Wavefront w applies steps w, w + NW, ... of the level, then the workgroup barrier hands the rewritten rows to the
// next level: the wavefronts share one CU and one L1, stores issued before a barrier are observed by loads issued after it
// (LLVM AMDGPU memory model, workgroup scope, as bpr_exact.hip relies on), and nothing else touches the tables during the
// launch.  A step's arithmetic is the reference's sequential arithmetic, followees walked in dict order, so a schedule of
// width 1 (one step per level) is the plain sequential walk and every schedule gives the same bits.  Each step writes its
// loss term(s) to slots indexed by their position in the reference order; loss_fold_kernel adds them one after the other.
#include "common.h"

using namespace qrec;

namespace {

__device__ inline double wsum(double v) { return wave_sum_dpp(v); }

template <int EPL>
__device__ inline void load_row(double (&x)[EPL], const double *row, int lane, int d) {
#pragma unroll
    for (int e = 0; e < EPL; e++) x[e] = (lane + 64 * e) < d ? row[lane + 64 * e] : 0.0;
}

template <int EPL>
__device__ inline void store_row(double *row, const double (&x)[EPL], int lane, int d) {
#pragma unroll
    for (int e = 0; e < EPL; e++)
        if ((lane + 64 * e) < d) row[lane + 64 * e] = x[e];
}

// RSTE.py:26-37 with predictForRating :42-62.  den[u] = the followees' weight sum as numpy's weights.sum() gives it (host);
// den != 0: pred = alpha*P[u].Q[i] + ((1-alpha)*sum_f w_f (P[f].Q[i])) / den, else pred = P[u].Q[i].  p, q are views.
template <int EPL>
__global__ __launch_bounds__(64) void rste_ordered_kernel(double *__restrict__ P, double *__restrict__ Q, int d, int ld,
                                                          const int64_t *__restrict__ fe_ptr, const int32_t *__restrict__ fe_ids,
                                                          const double *__restrict__ fe_w, const double *__restrict__ den_u,
                                                          const int32_t *__restrict__ u_idx, const int32_t *__restrict__ i_idx,
                                                          const double *__restrict__ rating, int64_t n, double lr, double alpha,
                                                          double regU, double regI, double *__restrict__ loss_out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    double loss = 0.0;
    for (int64_t t = 0; t < n; t++) {
        const int u = u_idx[t], i = i_idx[t];
        double *p = P + (int64_t)u * ld;
        double *q = Q + (int64_t)i * ld;
        double pv[EPL], qv[EPL];
        load_row(pv, p, lane, d);
        load_row(qv, q, lane, d);
        double dot = 0.0;
#pragma unroll
        for (int e = 0; e < EPL; e++) dot += pv[e] * qv[e];
        dot = wsum(dot);
        const double den = den_u[u];
        double pred = dot;
        if (den != 0.0) {
            double fpred = 0.0;
            for (int64_t k = fe_ptr[u]; k < fe_ptr[u + 1]; k++) {
                const double *f = P + (int64_t)fe_ids[k] * ld;
                double s = 0.0;
#pragma unroll
                for (int e = 0; e < EPL; e++) s += ((lane + 64 * e) < d ? f[lane + 64 * e] : 0.0) * qv[e];
                fpred += fe_w[k] * wsum(s);
            }
            pred = alpha * dot + ((1.0 - alpha) * fpred) / den;
        }
        const double err = rating[t] - pred;
        loss += err * err;
        const double ae = alpha * err;
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            pv[e] += lr * (ae * qv[e] - regU * pv[e]);
            qv[e] += lr * (ae * pv[e] - regI * qv[e]);
        }
        store_row(p, pv, lane, d);
        store_row(q, qv, lane, d);
    }
    if (lane == 0) *loss_out = loss;
}

// One user's step of the per-user pass; MODE 0 = SocialMF, 1 = SoReg, 2 = SREE (QREC_SOCIAL_* of qrec_hip.h).
//   SocialMF  fPred = sum w P[f], denom = sum w; rl = P[u] - fPred/denom (0 if denom == 0);
//             slot[k] = regS * rl.rl; P[u] -= (lr*regS) * rl                                   (coef = regS)
//   SoReg     f1 = sum_followees Sim (P[u]-P[f]), simSum += Sim |P[u]-P[f]|^2, slot[edge] = simSum (once per followee);
//             f2 = sum_followers Sim (P[u]-P[g]); P[u] += lr * (-alpha * (f1 + f2))           (coef = alpha)
//   SREE      per followee v: P[u] -= ((lr*alpha)*w) (P[u]-P[v]); slot[edge] = (alpha*w) |P[u]-P[v]|^2 with the
//             updated P[u]                                                                         (coef = alpha)
// A followee (or follower) that is the user itself is the user's own row: read from the registers.
template <int EPL, int MODE>
__device__ inline void user_step(double *__restrict__ P, int d, int ld, int lane, int k, const int32_t *__restrict__ step_user,
                                 const int64_t *__restrict__ fe_ptr, const int32_t *__restrict__ fe_ids, const double *__restrict__ fe_w,
                                 const int64_t *__restrict__ fr_ptr, const int32_t *__restrict__ fr_ids, const double *__restrict__ fr_w,
                                 double lr, double coef, double *__restrict__ slots) {
#pragma clang fp contract(off)
    const int u = step_user[k];
    double *prow = P + (int64_t)u * ld;
    double p[EPL];
    load_row(p, prow, lane, d);
    const int64_t b = fe_ptr[k], en = fe_ptr[k + 1];
    if constexpr (MODE == 0) {
        double fp[EPL], denom = 0.0;
#pragma unroll
        for (int e = 0; e < EPL; e++) fp[e] = 0.0;
        for (int64_t j = b; j < en; j++) {
            const int f = fe_ids[j];
            const double w = fe_w[j];
            double x[EPL];
            if (f == u) {
#pragma unroll
                for (int e = 0; e < EPL; e++) x[e] = p[e];
            } else {
                load_row(x, P + (int64_t)f * ld, lane, d);
            }
#pragma unroll
            for (int e = 0; e < EPL; e++) fp[e] += w * x[e];
            denom += w;
        }
        double rl[EPL], dd = 0.0;
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            rl[e] = denom != 0.0 ? p[e] - fp[e] / denom : 0.0;
            dd += rl[e] * rl[e];
        }
        dd = wsum(dd);
        if (lane == 0) slots[k] = coef * dd;
        const double c = lr * coef;
#pragma unroll
        for (int e = 0; e < EPL; e++) p[e] -= c * rl[e];
    } else if constexpr (MODE == 1) {
        double f1[EPL], f2[EPL], simsum = 0.0;
#pragma unroll
        for (int e = 0; e < EPL; e++) { f1[e] = 0.0; f2[e] = 0.0; }
        for (int64_t j = b; j < en; j++) {
            const int f = fe_ids[j];
            const double s = fe_w[j];
            double x[EPL], dd = 0.0;
            if (f == u) {
#pragma unroll
                for (int e = 0; e < EPL; e++) x[e] = p[e];
            } else {
                load_row(x, P + (int64_t)f * ld, lane, d);
            }
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                const double df = p[e] - x[e];
                f1[e] += s * df;
                dd += df * df;
            }
            simsum += s * wsum(dd);
            if (lane == 0) slots[j] = simsum;
        }
        for (int64_t j = fr_ptr[k]; j < fr_ptr[k + 1]; j++) {
            const int g = fr_ids[j];
            const double s = fr_w[j];
            double x[EPL];
            if (g == u) {
#pragma unroll
                for (int e = 0; e < EPL; e++) x[e] = p[e];
            } else {
                load_row(x, P + (int64_t)g * ld, lane, d);
            }
#pragma unroll
            for (int e = 0; e < EPL; e++) f2[e] += s * (p[e] - x[e]);
        }
        const double na = -coef;
#pragma unroll
        for (int e = 0; e < EPL; e++) p[e] += lr * (na * (f1[e] + f2[e]));
    } else {
        const double la = lr * coef;
        for (int64_t j = b; j < en; j++) {
            const int v = fe_ids[j];
            const double w = fe_w[j];
            const bool self = v == u;
            double z[EPL], dd = 0.0;
            if (self) {
#pragma unroll
                for (int e = 0; e < EPL; e++) z[e] = p[e];
            } else {
                load_row(z, P + (int64_t)v * ld, lane, d);
            }
            const double c = la * w;
#pragma unroll
            for (int e = 0; e < EPL; e++) p[e] -= c * (p[e] - z[e]);
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                const double df = p[e] - (self ? p[e] : z[e]);
                dd += df * df;
            }
            dd = wsum(dd);
            if (lane == 0) slots[j] = (coef * w) * dd;
        }
    }
    store_row(prow, p, lane, d);
}

template <int EPL, int MODE>
__global__ __launch_bounds__(1024) void social_user_levels_kernel(
    double *__restrict__ P, int d, int ld, const int32_t *__restrict__ step_user, const int64_t *__restrict__ fe_ptr,
    const int32_t *__restrict__ fe_ids, const double *__restrict__ fe_w, const int64_t *__restrict__ fr_ptr,
    const int32_t *__restrict__ fr_ids, const double *__restrict__ fr_w, const int32_t *__restrict__ order,
    const int32_t *__restrict__ level_ptr, int n_levels, double lr, double coef, double *__restrict__ slots) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int L = 0; L < n_levels; L++) {
        const int e = level_ptr[L + 1];
        for (int s = level_ptr[L] + w; s < e; s += nw)
            user_step<EPL, MODE>(P, d, ld, lane, order[s], step_user, fe_ptr, fe_ids, fe_w, fr_ptr, fr_ids, fr_w, lr, coef, slots);
        __syncthreads();
    }
}

// SoRec.py:41-58, one relation k = (u, v, t) with the host's weight: euv = weight*t - P[u].Z[v];
// slot[k] = regS*euv^2; P[u] += lr*((regS*euv)*z); Z[v] += lr*((regS*euv)*p - regZ*z) with the updated p.
template <int EPL>
__global__ __launch_bounds__(1024) void sorec_levels_kernel(double *__restrict__ P, double *__restrict__ Z, int d, int ld,
                                                            const int32_t *__restrict__ rel_u, const int32_t *__restrict__ rel_v,
                                                            const double *__restrict__ rel_t, const double *__restrict__ rel_w,
                                                            const int32_t *__restrict__ order, const int32_t *__restrict__ level_ptr,
                                                            int n_levels, double lr, double regS, double regZ,
                                                            double *__restrict__ slots) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int L = 0; L < n_levels; L++) {
        const int end = level_ptr[L + 1];
        for (int s = level_ptr[L] + w; s < end; s += nw) {
            const int k = order[s];
            double *prow = P + (int64_t)rel_u[k] * ld;
            double *zrow = Z + (int64_t)rel_v[k] * ld;
            double p[EPL], z[EPL], dot = 0.0;
            load_row(p, prow, lane, d);
            load_row(z, zrow, lane, d);
#pragma unroll
            for (int e = 0; e < EPL; e++) dot += p[e] * z[e];
            const double euv = rel_w[k] * rel_t[k] - wsum(dot);
            if (lane == 0) slots[k] = regS * (euv * euv);
            const double c = regS * euv;
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                p[e] += lr * (c * z[e]);
                z[e] += lr * (c * p[e] - regZ * z[e]);
            }
            store_row(prow, p, lane, d);
            store_row(zrow, z, lane, d);
        }
        __syncthreads();
    }
}

// running = ((running + slots[0]) + slots[1]) + ... : the reference's association of `self.loss += term`.
__global__ __launch_bounds__(64) void loss_fold_kernel(double *__restrict__ running, const double *__restrict__ slots, int64_t n) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    double acc = *running;
    for (int64_t k = 0; k < n; k++) acc += slots[k];
    *running = acc;
}

template <int EPL>
int launch_user_levels(int mode, int nw, double *P, int d, int ld, const int32_t *su, const int64_t *fe_ptr, const int32_t *fe_ids,
                       const double *fe_w, const int64_t *fr_ptr, const int32_t *fr_ids, const double *fr_w, const int32_t *order,
                       const int32_t *level_ptr, int n_levels, double lr, double coef, double *slots, hipStream_t st) {
#define QREC_USER_LAUNCH(M)                                                                                                     \
    hipLaunchKernelGGL((social_user_levels_kernel<EPL, M>), dim3(1), dim3(64 * nw), 0, st, P, d, ld, su, fe_ptr, fe_ids, fe_w, \
                       fr_ptr, fr_ids, fr_w, order, level_ptr, n_levels, lr, coef, slots)
    if (mode == QREC_SOCIAL_SOCIALMF) QREC_USER_LAUNCH(0);
    else if (mode == QREC_SOCIAL_SOREG) QREC_USER_LAUNCH(1);
    else QREC_USER_LAUNCH(2);
#undef QREC_USER_LAUNCH
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // namespace

extern "C" {

int qrec_rste_sgd_ordered(double *d_P, double *d_Q, int32_t d, int32_t ld, const int64_t *d_fe_indptr, const int32_t *d_fe_ids,
                          const double *d_fe_w, const double *d_fe_den, const int32_t *d_u, const int32_t *d_i,
                          const double *d_rating, int64_t n, double lr, double alpha, double regU, double regI, double *d_loss,
                          void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_loss && n >= 0, "qrec_rste_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_rating && d_fe_indptr && d_fe_den), "qrec_rste_sgd_ordered: null index array");
    QREC_REQUIRE(d >= 1 && d <= 256 && ld >= d, "qrec_rste_sgd_ordered: need 1 <= d <= 256, ld >= d (got d=%d ld=%d)", d, ld);
    hipStream_t st = as_stream(stream);
    if (n == 0) { QREC_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), st)); return QREC_OK; }
#define QREC_RSTE_LAUNCH(EPL)                                                                                                  \
    hipLaunchKernelGGL((rste_ordered_kernel<EPL>), dim3(1), dim3(64), 0, st, d_P, d_Q, d, ld, d_fe_indptr, d_fe_ids, d_fe_w,   \
                       d_fe_den, d_u, d_i, d_rating, n, lr, alpha, regU, regI, d_loss)
    if (d <= 64) QREC_RSTE_LAUNCH(1);
    else if (d <= 128) QREC_RSTE_LAUNCH(2);
    else QREC_RSTE_LAUNCH(4);
#undef QREC_RSTE_LAUNCH
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_social_user_pass(int mode, double *d_P, int32_t d, int32_t ld, const int32_t *d_step_user, int64_t n_steps,
                          const int64_t *d_fe_indptr, const int32_t *d_fe_ids, const double *d_fe_w, const int64_t *d_fr_indptr,
                          const int32_t *d_fr_ids, const double *d_fr_w, const int32_t *d_order, const int32_t *d_level_ptr,
                          int32_t n_levels, int32_t n_waves, double lr, double coef, double *d_slots, void *stream) {
    QREC_REQUIRE(mode == QREC_SOCIAL_SOCIALMF || mode == QREC_SOCIAL_SOREG || mode == QREC_SOCIAL_SREE,
                 "qrec_social_user_pass: mode must be 0 (SocialMF), 1 (SoReg) or 2 (SREE), got %d", mode);
    QREC_REQUIRE(d_P && n_steps >= 0 && n_steps < (int64_t)1 << 31 && n_levels >= 0, "qrec_social_user_pass: null argument");
    QREC_REQUIRE(n_steps == 0 || (d_step_user && d_fe_indptr && d_order && d_level_ptr && d_slots),
                 "qrec_social_user_pass: null step array");
    QREC_REQUIRE(mode != QREC_SOCIAL_SOREG || n_steps == 0 || d_fr_indptr, "qrec_social_user_pass: SoReg needs the follower CSR");
    QREC_REQUIRE(d >= 1 && d <= 256 && ld >= d, "qrec_social_user_pass: need 1 <= d <= 256, ld >= d (got d=%d ld=%d)", d, ld);
    QREC_REQUIRE(n_waves >= 1 && n_waves <= QREC_SOCIAL_MAX_WAVES, "qrec_social_user_pass: need 1 <= n_waves <= %d, got %d",
                 QREC_SOCIAL_MAX_WAVES, n_waves);
    if (n_steps == 0 || n_levels == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
    if (d <= 64) return launch_user_levels<1>(mode, n_waves, d_P, d, ld, d_step_user, d_fe_indptr, d_fe_ids, d_fe_w, d_fr_indptr, d_fr_ids,
                                              d_fr_w, d_order, d_level_ptr, n_levels, lr, coef, d_slots, st);
    if (d <= 128) return launch_user_levels<2>(mode, n_waves, d_P, d, ld, d_step_user, d_fe_indptr, d_fe_ids, d_fe_w, d_fr_indptr, d_fr_ids,
                                               d_fr_w, d_order, d_level_ptr, n_levels, lr, coef, d_slots, st);
    return launch_user_levels<4>(mode, n_waves, d_P, d, ld, d_step_user, d_fe_indptr, d_fe_ids, d_fe_w, d_fr_indptr, d_fr_ids, d_fr_w,
                                 d_order, d_level_ptr, n_levels, lr, coef, d_slots, st);
}

int qrec_sorec_relation_pass(double *d_P, double *d_Z, int32_t d, int32_t ld, const int32_t *d_rel_u, const int32_t *d_rel_v,
                             const double *d_rel_t, const double *d_rel_w, int64_t n_rel, const int32_t *d_order,
                             const int32_t *d_level_ptr, int32_t n_levels, int32_t n_waves, double lr, double regS, double regZ,
                             double *d_slots, void *stream) {
    QREC_REQUIRE(d_P && d_Z && n_rel >= 0 && n_rel < (int64_t)1 << 31 && n_levels >= 0, "qrec_sorec_relation_pass: null argument");
    QREC_REQUIRE(n_rel == 0 || (d_rel_u && d_rel_v && d_rel_t && d_rel_w && d_order && d_level_ptr && d_slots),
                 "qrec_sorec_relation_pass: null relation array");
    QREC_REQUIRE(d >= 1 && d <= 256 && ld >= d, "qrec_sorec_relation_pass: need 1 <= d <= 256, ld >= d (got d=%d ld=%d)", d, ld);
    QREC_REQUIRE(n_waves >= 1 && n_waves <= QREC_SOCIAL_MAX_WAVES, "qrec_sorec_relation_pass: need 1 <= n_waves <= %d, got %d",
                 QREC_SOCIAL_MAX_WAVES, n_waves);
    if (n_rel == 0 || n_levels == 0) return QREC_OK;
    hipStream_t st = as_stream(stream);
#define QREC_SOREC_LAUNCH(EPL)                                                                                                   \
    hipLaunchKernelGGL((sorec_levels_kernel<EPL>), dim3(1), dim3(64 * n_waves), 0, st, d_P, d_Z, d, ld, d_rel_u, d_rel_v, d_rel_t, \
                       d_rel_w, d_order, d_level_ptr, n_levels, lr, regS, regZ, d_slots)
    if (d <= 64) QREC_SOREC_LAUNCH(1);
    else if (d <= 128) QREC_SOREC_LAUNCH(2);
    else QREC_SOREC_LAUNCH(4);
#undef QREC_SOREC_LAUNCH
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_loss_fold(double *d_running, const double *d_slots, int64_t n, void *stream) {
    QREC_REQUIRE(d_running && n >= 0 && (n == 0 || d_slots), "qrec_loss_fold: null argument");
    if (n == 0) return QREC_OK;
    hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(64), 0, as_stream(stream), d_running, d_slots, n);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

}  // extern "C"
