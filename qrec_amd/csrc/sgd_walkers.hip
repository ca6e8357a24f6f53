// The order-exact SGD walkers: the reference's updates applied strictly in array order, fp64 or fp32 tables.
//
// The conflict DAG of an epoch is ~n/6 deep (every user run is a chain through P[u], popular items link the runs), so the
// order-exact mode has no exploitable parallelism beyond the d lanes of one row: ONE wavefront walks the list, lane = column
// (lane_row.h).  This is the parity mode of BPR (bpr_ordered_kernel; bpr_exact.hip runs the same arithmetic by a schedule,
// bpr_sgd.hip is the throughput mode), TBPR, SBPR, the rating-prediction MF family and SVD++.
#include "lane_row.h"

// numpy rounds every product and sum separately, and so does every kernel of this file (lane_row.h: CONTRACTION)
#pragma clang fp contract(off)

using namespace qrec;

namespace {

// model/ranking/BPR.py:45-53 (+ sigmoid util/qmath.py:127-128):
//   x = P[u].Q[i] - P[u].Q[j];  s = 1/(1+exp(-x));  g = lr*(1-s)
//   P[u] += g*(Q[i]-Q[j]);  Q[i] += g*P[u];  Q[j] -= g*P[u]      (P[u] already updated)
//   P[u] -= lr*regU*P[u];   Q[i] -= lr*regI*Q[i];   Q[j] -= lr*regI*Q[j];   loss += -log(s)
// with the next triplet's rows prefetched and patched from registers when they alias.
template <typename T, int EPL>
__global__ __launch_bounds__(64) void bpr_ordered_kernel(
    T *__restrict__ P, T *__restrict__ Q, int d, int ld, const int32_t *__restrict__ u_idx,
    const int32_t *__restrict__ i_idx, const int32_t *__restrict__ j_idx, int64_t n, T lr, T cu,
    T ci, double *__restrict__ loss_out) {
    const LaneRow<T, EPL> R(threadIdx.x, d, ld);
    T pu[EPL], qi[EPL], qj[EPL], nqi[EPL], nqj[EPL];
    double loss = 0.0;
    int cur_u = -1;
    if (n > 0) R.load2(qi, Q, i_idx[0], qj, Q, j_idx[0]);
    for (int64_t t = 0; t < n; t++) {
        const int ut = u_idx[t], it = i_idx[t], jt = j_idx[t];
        if (ut != cur_u) {
            if (cur_u >= 0) R.store(P, cur_u, pu);
            R.load(pu, P, ut);
            cur_u = ut;
        }
        int in = -1, jn = -1;
        if (t + 1 < n) {  // prefetch the next triplet's item rows under this one's math
            in = i_idx[t + 1]; jn = j_idx[t + 1];
            R.load2(nqi, Q, in, nqj, Q, jn);
        }
        // both dot products in ONE loop and their two cross-lane sums side by side: as two row_dot() calls the second DPP chain
        // came after the first instead of between its steps (measured: 1 % of the step at d = 64)
        T di = 0, dj = 0;
#pragma unroll
        for (int e = 0; e < EPL; e++) { di += pu[e] * qi[e]; dj += pu[e] * qj[e]; }
        di = wave_sum_dpp(di); dj = wave_sum_dpp(dj);
        const T s = T(1) / (T(1) + dev_exp<T>(-(di - dj)));
        const T g = lr * (T(1) - s);
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            pu[e] += g * (qi[e] - qj[e]);
            qi[e] += g * pu[e];
            qj[e] -= g * pu[e];
            pu[e] -= cu * pu[e];
            qi[e] -= ci * qi[e];
            qj[e] -= ci * qj[e];
        }
        R.store(Q, it, qi); R.store(Q, jt, qj);
        // fp64 tables: the reference's own expression (model/ranking/BPR.py:53); fp32: stable form
        if constexpr (sizeof(T) == 8) loss += -log((double)s);
        else loss += neg_log_sigmoid((double)(di - dj));
        if (t + 1 < n) {  // rows just written supersede what the prefetch saw
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                T a = nqi[e], b = nqj[e];
                if (in == it) a = qi[e]; else if (in == jt) a = qj[e];
                if (jn == it) b = qi[e]; else if (jn == jt) b = qj[e];
                qi[e] = a; qj[e] = b;
            }
        }
    }
    if (cur_u >= 0) R.store(P, cur_u, pu);
    if (R.lane == 0) *loss_out = loss;
}

// TBPR (model/ranking/TBPR.py:40-48,131-159), order-exact: the same per-triplet arithmetic over the chained
// (u, a, b) updates, with two things BPR never needs:
//   * a == b happens (the closing random item may repeat the chain's last social item): the two row updates then hit
//     ONE row in sequence, as numpy's in-place row statements do;
//   * the loss takes regU*sum(P*P) + regI*sum(Q*Q) over the WHOLE tables after every user (TBPR.py:159 is inside the
//     user loop).  The sums are carried along instead of recomputed: sums_in = {sum P*P, sum Q*Q} before the launch,
//     every row update adds (|new row|^2 - |old row|^2) in fp64.
// loss_out[0] = sum(-log s), loss_out[1] = sum over users of (regU*sumP2 + regI*sumQ2).
template <typename T, int EPL>
__global__ __launch_bounds__(64) void tbpr_ordered_kernel(
    T *__restrict__ P, T *__restrict__ Q, int d, int ld, const int32_t *__restrict__ u_idx,
    const int32_t *__restrict__ a_idx, const int32_t *__restrict__ b_idx, int64_t n, T lr, T cu, T ci,
    double regU, double regI, const double *__restrict__ sums_in, double *__restrict__ loss_out) {
    const LaneRow<T, EPL> R(threadIdx.x, d, ld);
    T pu[EPL], qa[EPL], qb[EPL], nqa[EPL], nqb[EPL];
    double loss = 0.0, reg = 0.0, sP = sums_in[0], sQ = sums_in[1], pu_loaded = 0.0;
    int cur_u = -1;
    if (n > 0) { R.load(qa, Q, a_idx[0]); R.load(qb, Q, b_idx[0]); }
    for (int64_t t = 0; t < n; t++) {
        const int ut = u_idx[t], at = a_idx[t], bt = b_idx[t];
        if (ut != cur_u) {
            if (cur_u >= 0) {
                R.store(P, cur_u, pu);
                sP += row_norm2(pu) - pu_loaded;
                reg += regU * sP + regI * sQ;
            }
            R.load(pu, P, ut);
            pu_loaded = row_norm2(pu);
            cur_u = ut;
        }
        int an = -1, bn = -1;
        if (t + 1 < n) { an = a_idx[t + 1]; bn = b_idx[t + 1]; R.load(nqa, Q, an); R.load(nqb, Q, bn); }
        const bool alias = at == bt;
        const double q_old = row_norm2(qa) + (alias ? 0.0 : row_norm2(qb));
        const T da = row_dot(pu, qa), db = row_dot(pu, qb);
        const T s = T(1) / (T(1) + dev_exp<T>(-(da - db)));
        const T g = lr * (T(1) - s);
        if (!alias) {
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                pu[e] += g * (qa[e] - qb[e]);
                qa[e] += g * pu[e];
                qb[e] -= g * pu[e];
                pu[e] -= cu * pu[e];
                qa[e] -= ci * qa[e];
                qb[e] -= ci * qb[e];
            }
            R.store(Q, at, qa); R.store(Q, bt, qb);
        } else {
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                T r = qa[e];
                pu[e] += g * (r - r);
                r += g * pu[e];
                r -= g * pu[e];
                pu[e] -= cu * pu[e];
                r -= ci * r;
                r -= ci * r;
                qa[e] = r; qb[e] = r;
            }
            R.store(Q, at, qa);
        }
        sQ += row_norm2(qa) + (alias ? 0.0 : row_norm2(qb)) - q_old;
        if constexpr (sizeof(T) == 8) loss += -log((double)s);
        else loss += neg_log_sigmoid((double)(da - db));
        if (t + 1 < n) {
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                T x = nqa[e], y = nqb[e];
                if (an == at) x = qa[e]; else if (an == bt) x = qb[e];
                if (bn == at) y = qa[e]; else if (bn == bt) y = qb[e];
                qa[e] = x; qb[e] = y;
            }
        }
    }
    if (cur_u >= 0) {
        R.store(P, cur_u, pu);
        sP += row_norm2(pu) - pu_loaded;
        reg += regU * sP + regI * sQ;
    }
    if (R.lane == 0) { loss_out[0] = loss; loss_out[1] = reg; }
}

// SBPR (model/ranking/SBPR.py:41-74, numpy path), order-exact, one wavefront, lane = column.  Rows (u, i, k, j, Suk) in the
// reference's visiting order; k < 0: the user has no social feedback (:68-73, plain BPR step with the item biases in the
// score and NO decay); i < 0: a bare visit of a user without positives (only the per-user loss terms).  With k >= 0 the two
// chained pairs of :45-55 -- (i over k) scaled by 1 / (Suk + 1), then (k over j) -- then the four decays (:56-59, in the
// order P[u], Q[i], Q[j], Q[k]) and the loss of :57-58 from the UPDATED rows, without the biases.  j == k happens (the
// negative's rejection test does not look at the user's own feedback list): the row is then updated in sequence, as numpy's
// in-place statements do, and decays twice.  The biases b never change (no statement updates them).  After every user:
// regU*sum(P*P) + regI*sum(Q*Q) + b.b over the WHOLE tables (:74 sits inside the user loop) -- sums carried along as in
// tbpr_ordered_kernel.  loss_out[0] = sum of the -log terms, loss_out[1] = sum over users of the table terms.
template <typename T, int EPL>
__global__ __launch_bounds__(64) void sbpr_ordered_kernel(
    T *__restrict__ P, T *__restrict__ Q, const T *__restrict__ bias, int d, int ld, const int32_t *__restrict__ rows, int64_t n, T lr, T cu, T ci,
    double regU, double regI, double bb, const double *__restrict__ sums_in, double *__restrict__ loss_out) {
    const LaneRow<T, EPL> R(threadIdx.x, d, ld);
    // a pairwise step on (pu, hi, lo) with coefficient c: P[u] += c (hi - lo); hi += c P[u]; lo -= c P[u]   (:46-48, :53-55, :70-72)
    auto pair_step = [&](T (&pu)[EPL], T (&hi)[EPL], T (&lo)[EPL], T c) {
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            pu[e] += c * (hi[e] - lo[e]);
            hi[e] += c * pu[e];
            lo[e] -= c * pu[e];
        }
    };
    auto decay = [&](T (&r)[EPL], T c) {
#pragma unroll
        for (int e = 0; e < EPL; e++) r[e] -= c * r[e];
    };
    auto sigmoid = [&](T x) { return T(1) / (T(1) + dev_exp<T>(-x)); };
    T pu[EPL], qi[EPL], qk[EPL], qj[EPL];
    double loss = 0.0, reg = 0.0, sP = sums_in[0], sQ = sums_in[1], pu_loaded = 0.0;
    int cur_u = -1;
    for (int64_t t = 0; t < n; t++) {
        const int32_t *row = rows + 5 * t;
        const int ut = row[0], it = row[1], kt = row[2], jt = row[3];
        const T scale = T(1) / (T)(row[4] + 1);
        if (ut != cur_u) {
            if (cur_u >= 0) {
                R.store(P, cur_u, pu);
                sP += row_norm2(pu) - pu_loaded;
                reg += regU * sP + regI * sQ + bb;
            }
            R.load(pu, P, ut);
            pu_loaded = row_norm2(pu);
            cur_u = ut;
        }
        if (it < 0) continue;
        R.load(qi, Q, it); R.load(qj, Q, jt);
        if (kt < 0) {
            const double q_old = row_norm2(qi) + row_norm2(qj);
            const T x = ((row_dot(pu, qi) - row_dot(pu, qj)) + bias[it]) - bias[jt];
            const T s = sigmoid(x);
            pair_step(pu, qi, qj, lr * (T(1) - s));
            R.store(Q, it, qi); R.store(Q, jt, qj);
            sQ += row_norm2(qi) + row_norm2(qj) - q_old;
            if constexpr (sizeof(T) == 8) loss += -log((double)s);
            else loss += neg_log_sigmoid((double)x);      // fp32 tables: the stable form of -log(sigmoid(x)) (bpr_ordered_kernel)
            continue;
        }
        const bool alias = jt == kt;
        R.load(qk, Q, kt);
        const double q_old = row_norm2(qi) + row_norm2(qk) + (alias ? 0.0 : row_norm2(qj));
        const T s = sigmoid((((row_dot(pu, qi) - row_dot(pu, qk)) + bias[it]) - bias[kt]) / (T)(row[4] + 1));     // the reference divides (:45) ...
        pair_step(pu, qi, qk, (scale * lr) * (T(1) - s));                                  // ... and multiplies here: 1 / (Suk+1) * lRate * (1 - s), left to right (:46)
        if (alias) {
            const T s2 = sigmoid(((row_dot(pu, qk) - row_dot(pu, qk)) + bias[kt]) - bias[jt]);
            const T c2 = lr * (T(1) - s2);
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                pu[e] += c2 * (qk[e] - qk[e]);
                qk[e] += c2 * pu[e];
                qk[e] -= c2 * pu[e];
            }
            decay(pu, cu); decay(qi, ci); decay(qk, ci); decay(qk, ci);
        } else {
            const T s2 = sigmoid(((row_dot(pu, qk) - row_dot(pu, qj)) + bias[kt]) - bias[jt]);
            pair_step(pu, qk, qj, lr * (T(1) - s2));
            decay(pu, cu); decay(qi, ci); decay(qj, ci); decay(qk, ci);
        }
        const T x1 = (row_dot(pu, qi) - row_dot(pu, qk)) / (T)(row[4] + 1);
        const T x2 = alias ? (row_dot(pu, qk) - row_dot(pu, qk)) : (row_dot(pu, qk) - row_dot(pu, qj));
        if constexpr (sizeof(T) == 8) loss += -log((double)sigmoid(x1)) - log((double)sigmoid(x2));
        else loss += neg_log_sigmoid((double)x1) + neg_log_sigmoid((double)x2);
        R.store(Q, it, qi); R.store(Q, kt, qk);
        if (!alias) R.store(Q, jt, qj);
        sQ += row_norm2(qi) + row_norm2(qk) + (alias ? 0.0 : row_norm2(qj)) - q_old;
    }
    if (cur_u >= 0) {
        R.store(P, cur_u, pu);
        sP += row_norm2(pu) - pu_loaded;
        reg += regU * sP + regI * sQ + bb;
    }
    if (R.lane == 0) { loss_out[0] = loss; loss_out[1] = reg; }
}

// Rating-prediction MF family, order-exact, same structure (one wavefront, lane = column):
//   VAR 0  model/rating/BasicMF.py:9-26   P[u] += (lr*e)*q ;            Q[i] += (lr*e)*p
//   VAR 1  model/rating/PMF.py:9-28       P[u] += lr*(e*q - regU*p) ;   Q[i] += lr*(e*p - regI*q)
//   VAR 2  model/rating/SVD.py:13-35      as PMF with e = r - (((P[u].Q[i] + mean) + Bi[i]) + Bu[u]),
//                                         Bu[u] += lr*(e - regB*bu) ; Bi[i] += lr*(e - regB*bi)
//   VAR 3  model/rating/EE.py:15-34       diff = P[u]-Q[i]; e = r - (((mean + Bi[i]) + Bu[u]) - diff.diff);
//                                         loss += e*e + regU*diff.diff; P[u] -= (lr*(e+regU))*diff;
//                                         Q[i] += (lr*(e+regI))*(P[u]-Q[i]); biases as SVD
//   VAR 4  model/rating/SocialMF.py:14-24 PMF's arithmetic on COPIES: p, q are taken before the updates, so the
//                                         Q[i] update sees the old P[u]
// p is a VIEW of P[u] in the reference (VAR 0-3), so the Q[i] update sees the already updated P[u].
template <typename T, int EPL, int VAR>
__global__ __launch_bounds__(64) void mf_ordered_kernel(
    T *__restrict__ P, T *__restrict__ Q, T *__restrict__ Bu, T *__restrict__ Bi, int d, int ld,
    const int32_t *__restrict__ u_idx, const int32_t *__restrict__ i_idx, const double *__restrict__ rating,
    int64_t n, T lr, T regU, T regI, T regB, T gmean, double *__restrict__ loss_out) {
    const LaneRow<T, EPL> R(threadIdx.x, d, ld);
    double loss = 0.0;
    for (int64_t t = 0; t < n; t++) {
        const int u = u_idx[t], i = i_idx[t];
        T pv[EPL], qv[EPL], dot;
        R.load2(pv, P, u, qv, Q, i);
        if constexpr (VAR == 3) {
            T df[EPL];
#pragma unroll
            for (int e = 0; e < EPL; e++) df[e] = pv[e] - qv[e];
            dot = row_dot(df, df);
        } else {
            dot = row_dot(pv, qv);
        }
        T pred = dot, bu = 0, bi = 0;
        if constexpr (VAR == 2) { bu = Bu[u]; bi = Bi[i]; pred = ((dot + gmean) + bi) + bu; }
        if constexpr (VAR == 3) { bu = Bu[u]; bi = Bi[i]; pred = ((gmean + bi) + bu) - dot; }
        const T err = (T)rating[t] - pred;
        loss += (double)err * (double)err;
        if constexpr (VAR == 3) loss += (double)(regU * dot);
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            if constexpr (VAR == 0) {
                pv[e] += (lr * err) * qv[e];
                qv[e] += (lr * err) * pv[e];
            } else if constexpr (VAR == 3) {
                pv[e] -= (lr * (err + regU)) * (pv[e] - qv[e]);
                qv[e] += (lr * (err + regI)) * (pv[e] - qv[e]);
            } else if constexpr (VAR == 4) {
                const T p0 = pv[e];
                pv[e] += lr * (err * qv[e] - regU * p0);
                qv[e] += lr * (err * p0 - regI * qv[e]);
            } else {
                pv[e] += lr * (err * qv[e] - regU * pv[e]);
                qv[e] += lr * (err * pv[e] - regI * qv[e]);
            }
        }
        R.store(P, u, pv); R.store(Q, i, qv);
        if constexpr (VAR == 2 || VAR == 3) {
            if (R.lane == 0) { Bu[u] = bu + lr * (err - regB * bu); Bi[i] = bi + lr * (err - regB * bi); }
        }
    }
    if (R.lane == 0) *loss_out = loss;
}

// model/rating/SVDPlusPlus.py:25-62,70-86, order-exact (one wavefront, lane = column).  Per rating the user's
// rated items (data.userRated order, CSR) are walked twice: sum_j Y[j] for the prediction, then -- over the OTHER
// items -- their sum, the Y updates and the implicit-feedback term of Q[i].  p and q are views in the reference: the
// P[u] update sees the already updated Q[i], the final Q[i] update the updated P[u].
template <typename T, int EPL>
__global__ __launch_bounds__(64) void svdpp_ordered_kernel(
    T *__restrict__ P, T *__restrict__ Q, T *__restrict__ Y, T *__restrict__ Bu, T *__restrict__ Bi, int d, int ld,
    const int64_t *__restrict__ rated_indptr, const int32_t *__restrict__ rated_items,
    const int32_t *__restrict__ u_idx, const int32_t *__restrict__ i_idx, const double *__restrict__ rating, int64_t n,
    T lr, T regU, T regI, T regB, T regY, T gmean, double *__restrict__ loss_out) {
    const LaneRow<T, EPL> R(threadIdx.x, d, ld);
    double loss = 0.0;
    for (int64_t t = 0; t < n; t++) {
        const int u = u_idx[t], i = i_idx[t];
        const int64_t b = rated_indptr[u], e_ = rated_indptr[u + 1];
        const T w = (T)(e_ - b);
        T pv[EPL], qv[EPL], yv[EPL], sum[EPL] = {};
        R.load2(pv, P, u, qv, Q, i);
        for (int64_t k = b; k < e_; k++) {
            R.load(yv, Y, rated_items[k]);
#pragma unroll
            for (int e = 0; e < EPL; e++) sum[e] += yv[e];
        }
        T a = 0, dot = 0;      // as in bpr_ordered_kernel: one loop, the two cross-lane sums side by side
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            if (e_ > b) a += (sum[e] / w) * qv[e];
            dot += pv[e] * qv[e];
        }
        a = wave_sum_dpp(a); dot = wave_sum_dpp(dot);
        const T bu = Bu[u], bi = Bi[i];
        const T pred = a + (((dot + gmean) + bi) + bu);
        const T err = (T)rating[t] - pred;
        loss += (double)err * (double)err;
        if (R.lane == 0) { Bu[u] = bu + lr * (err - regB * bu); Bi[i] = bi + lr * (err - regB * bi); }
        if (e_ - b > 1) {
            const T wm1 = (T)(e_ - b - 1);
            bool first = true;
            for (int64_t k = b; k < e_; k++) {
                const int j = rated_items[k];
                if (j == i) continue;
                R.load(yv, Y, j);
#pragma unroll
                for (int e = 0; e < EPL; e++) {
                    sum[e] = first ? yv[e] : sum[e] + yv[e];
                    yv[e] = yv[e] + lr * ((err * qv[e]) / wm1 - regY * yv[e]);
                }
                R.store(Y, j, yv);
                first = false;
            }
            if (!first) {
#pragma unroll
                for (int e = 0; e < EPL; e++) qv[e] += ((lr * err) * sum[e]) / wm1;
            }
        }
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            pv[e] += lr * (err * qv[e] - regU * pv[e]);
            qv[e] += lr * (err * pv[e] - regI * qv[e]);
        }
        R.store(P, u, pv); R.store(Q, i, qv);
    }
    if (R.lane == 0) *loss_out = loss;
}

}  // namespace

extern "C" {

int qrec_bpr_sgd_ordered(void *d_P, void *d_Q, int dtype, int32_t d, int32_t ld,
                         const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int64_t n,
                         double lr, double regU, double regI, double *d_loss, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_loss && n >= 0, "qrec_bpr_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_j), "qrec_bpr_sgd_ordered: null index array");
    if (int rc = check_lane_row("qrec_bpr_sgd_ordered", dtype, d, ld)) return rc;
    hipStream_t st = as_stream(stream);
    if (n == 0) { QREC_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), st)); return QREC_OK; }
    return with_row_type(dtype, d, [&](auto t, auto epl) {
        using T = decltype(t);
        return launch_waves(bpr_ordered_kernel<T, epl()>, 1, st, (T *)d_P, (T *)d_Q, d, ld, d_u, d_i, d_j, n, (T)lr, (T)lr * (T)regU,
                             (T)lr * (T)regI, d_loss);      // numpy: (lr*reg)*row
    });
}

int qrec_sbpr_sgd_ordered(void *d_P, void *d_Q, const void *d_bias, int dtype, int32_t d, int32_t ld, const int32_t *d_rows, int64_t n, double lr,
                          double regU, double regI, double bias_sumsq, const double *d_sums_in, double *d_loss2, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_bias && d_sums_in && d_loss2 && n >= 0, "qrec_sbpr_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || d_rows, "qrec_sbpr_sgd_ordered: null row array");
    if (int rc = check_lane_row("qrec_sbpr_sgd_ordered", dtype, d, ld)) return rc;
    return with_row_type(dtype, d, [&](auto t, auto epl) {
        using T = decltype(t);
        return launch_waves(sbpr_ordered_kernel<T, epl()>, 1, as_stream(stream), (T *)d_P, (T *)d_Q, (const T *)d_bias, d, ld, d_rows, n, (T)lr,
                             (T)lr * (T)regU, (T)lr * (T)regI, regU, regI, bias_sumsq, d_sums_in, d_loss2);
    });
}

int qrec_tbpr_sgd_ordered(void *d_P, void *d_Q, int dtype, int32_t d, int32_t ld, const int32_t *d_u, const int32_t *d_a,
                          const int32_t *d_b, int64_t n, double lr, double regU, double regI, const double *d_sums_in,
                          double *d_loss2, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_sums_in && d_loss2 && n >= 0, "qrec_tbpr_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_a && d_b), "qrec_tbpr_sgd_ordered: null index array");
    if (int rc = check_lane_row("qrec_tbpr_sgd_ordered", dtype, d, ld)) return rc;
    hipStream_t st = as_stream(stream);
    if (n == 0) { QREC_HIP_CHECK(hipMemsetAsync(d_loss2, 0, 2 * sizeof(double), st)); return QREC_OK; }
    return with_row_type(dtype, d, [&](auto t, auto epl) {
        using T = decltype(t);
        return launch_waves(tbpr_ordered_kernel<T, epl()>, 1, st, (T *)d_P, (T *)d_Q, d, ld, d_u, d_a, d_b, n, (T)lr, (T)lr * (T)regU,
                             (T)lr * (T)regI, regU, regI, d_sums_in, d_loss2);
    });
}

int qrec_mf_sgd_ordered(void *d_P, void *d_Q, int dtype, int32_t d, int32_t ld,
                        const int32_t *d_u, const int32_t *d_i, const double *d_rating, int64_t n,
                        double lr, double *d_loss, int variant, double regU, double regI, void *d_Bu,
                        void *d_Bi, double regB, double global_mean, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_loss && n >= 0, "qrec_mf_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_rating), "qrec_mf_sgd_ordered: null index array");
    if (int rc = check_lane_row("qrec_mf_sgd_ordered", dtype, d, ld)) return rc;
    QREC_REQUIRE(variant >= 0 && variant <= 4,
                 "qrec_mf_sgd_ordered: variant must be 0 (BasicMF), 1 (PMF), 2 (SVD), 3 (EE) or 4 (SocialMF)");
    QREC_REQUIRE(variant < 2 || variant > 3 || (d_Bu && d_Bi), "qrec_mf_sgd_ordered: SVD and EE need the bias vectors");
    hipStream_t st = as_stream(stream);
    if (n == 0) { QREC_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), st)); return QREC_OK; }
    return with_row_type(dtype, d, [&](auto t, auto epl) {
        using T = decltype(t);
        auto launch = [&](auto var) {
            return launch_waves(mf_ordered_kernel<T, epl(), var()>, 1, st, (T *)d_P, (T *)d_Q, (T *)d_Bu, (T *)d_Bi, d, ld, d_u, d_i, d_rating, n,
                                 (T)lr, (T)regU, (T)regI, (T)regB, (T)global_mean, d_loss);
        };
        switch (variant) {
            case 0: return launch(int_c<0>{});
            case 1: return launch(int_c<1>{});
            case 2: return launch(int_c<2>{});
            case 3: return launch(int_c<3>{});
            default: return launch(int_c<4>{});
        }
    });
}

int qrec_svdpp_sgd_ordered(void *d_P, void *d_Q, void *d_Y, void *d_Bu, void *d_Bi, int dtype, int32_t d, int32_t ld,
                           const int64_t *d_rated_indptr, const int32_t *d_rated_items, const int32_t *d_u,
                           const int32_t *d_i, const double *d_rating, int64_t n, double lr, double regU, double regI,
                           double regB, double regY, double global_mean, double *d_loss, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_Y && d_Bu && d_Bi && d_rated_indptr && d_loss && n >= 0, "qrec_svdpp_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_rating && d_rated_items), "qrec_svdpp_sgd_ordered: null index array");
    if (int rc = check_lane_row("qrec_svdpp_sgd_ordered", dtype, d, ld)) return rc;
    hipStream_t st = as_stream(stream);
    if (n == 0) { QREC_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), st)); return QREC_OK; }
    return with_row_type(dtype, d, [&](auto t, auto epl) {
        using T = decltype(t);
        return launch_waves(svdpp_ordered_kernel<T, epl()>, 1, st, (T *)d_P, (T *)d_Q, (T *)d_Y, (T *)d_Bu, (T *)d_Bi, d, ld, d_rated_indptr,
                             d_rated_items, d_u, d_i, d_rating, n, (T)lr, (T)regU, (T)regI, (T)regB, (T)regY, (T)global_mean, d_loss);
    });
}

}  // extern "C"
