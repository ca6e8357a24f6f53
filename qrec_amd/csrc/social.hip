// Social-trust rating models (model/rating/{SoRec,SoReg,SocialMF,RSTE,SREE,LOCABAL,SocialFD}.py), fp64, order-exact.
// LOCABAL and SocialFD, whose passes carry a dense d x d matrix, have their own section further down.
//
// The rating passes of SoRec / SoReg (PMF), SREE (EE) and SocialMF (PMF on copies) are mf_ordered_kernel of sgd_walkers.hip.
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
#include "lane_row.h"

using namespace qrec;

namespace {

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
    const LaneRow<double, EPL> R(threadIdx.x, d, ld);
    double loss = 0.0;
    for (int64_t t = 0; t < n; t++) {
        const int u = u_idx[t], i = i_idx[t];
        double pv[EPL], qv[EPL], fv[EPL];
        R.load(pv, P, u);
        R.load(qv, Q, i);
        const double dot = row_dot(pv, qv);
        const double den = den_u[u];
        double pred = dot;
        if (den != 0.0) {
            double fpred = 0.0;
            for (int64_t k = fe_ptr[u]; k < fe_ptr[u + 1]; k++) {
                R.load(fv, P, fe_ids[k]);
                fpred += fe_w[k] * row_dot(fv, qv);
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
        R.store(P, u, pv);
        R.store(Q, i, qv);
    }
    if (R.lane == 0) *loss_out = loss;
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
    const LaneRow<double, EPL> R(lane, d, ld);
    const int u = step_user[k];
    double p[EPL];
    R.load(p, P, u);
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
                R.load(x, P, f);
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
        dd = wave_sum_dpp(dd);
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
                R.load(x, P, f);
            }
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                const double df = p[e] - x[e];
                f1[e] += s * df;
                dd += df * df;
            }
            simsum += s * wave_sum_dpp(dd);
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
                R.load(x, P, g);
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
                R.load(z, P, v);
            }
            const double c = la * w;
#pragma unroll
            for (int e = 0; e < EPL; e++) p[e] -= c * (p[e] - z[e]);
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                const double df = p[e] - (self ? p[e] : z[e]);
                dd += df * df;
            }
            dd = wave_sum_dpp(dd);
            if (lane == 0) slots[j] = (coef * w) * dd;
        }
    }
    R.store(P, u, p);
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
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const LaneRow<double, EPL> R(threadIdx.x & 63, d, ld);
    for (int L = 0; L < n_levels; L++) {
        const int end = level_ptr[L + 1];
        for (int s = level_ptr[L] + w; s < end; s += nw) {
            const int k = order[s], u = rel_u[k], v = rel_v[k];
            double p[EPL], z[EPL];
            R.load(p, P, u);
            R.load(z, Z, v);
            const double euv = rel_w[k] * rel_t[k] - row_dot(p, z);
            if (R.lane == 0) slots[k] = regS * (euv * euv);
            const double c = regS * euv;
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                p[e] += lr * (c * z[e]);
                z[e] += lr * (c * p[e] - regZ * z[e]);
            }
            R.store(P, u, p);
            R.store(Z, v, z);
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

// ---- LOCABAL and SocialFD: passes that carry a dense d x d matrix H ---------------------------------------------------------
// Every step of these passes reads and writes all of H, so there is nothing to run side by side between steps; one
// workgroup runs a pass and the parallelism comes from inside a step.  H lives in LDS for the whole launch as [d][ldh]
// doubles with ldh = d | 1: an odd row stride makes both H^T v (lane = column, consecutive addresses) and H v (lane = row,
// stride ldh doubles) conflict-free for ds_read_b64, whose 32-lane halves then touch 32 distinct even banks.
// A matrix-vector product is cut into work items (chunk c, output o): the sum over KCH = 16 consecutive terms, added one
// after the other; the C = ceil(d / 16) partial sums of an output are then added in chunk order.  Scalar dot products are
// cut the same way.  The association depends on d alone, never on the number of wavefronts, which only decides how many
// work items run side by side: any wave count gives the same bits.  Element j of every P / Q row is read and written by
// thread j only (so a workgroup has at least ceil(d / 64) wavefronts), and a row handed from one step to the next crosses
// no thread boundary in global memory; vectors and scalars that other threads need go through LDS behind a workgroup barrier.
constexpr int KCH = 16;

// Everything one thread hands to another inside these kernels goes through LDS, so a barrier waits for the LDS counter
// only: the rows a thread stores to global memory are read back by that thread alone, and a step need not wait for its
// stores to land before the next one starts (__syncthreads() would drain the vector-memory counter as well).
__device__ inline void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

struct HLds {
    double *H;        // [d][ldh]
    double *vec[8];   // [d] each
    double *part[2];  // [C][d] each: partial sums of two concurrent products
    double *sc;       // 32 scalars: [0..C) and [16..16+C) partial sums of two dot products, [8..16) broadcast values
    int d, ldh, C;
};

__device__ inline HLds carve_h(unsigned char *smem, int d) {
    HLds s;
    s.d = d; s.ldh = d | 1; s.C = (d + KCH - 1) / KCH;
    double *p = reinterpret_cast<double *>(smem);
    s.H = p; p += (size_t)d * s.ldh;
    for (int k = 0; k < 8; k++) { s.vec[k] = p; p += d; }
    s.part[0] = p; p += s.C * d;
    s.part[1] = p; p += s.C * d;
    s.sc = p;
    return s;
}

size_t h_lds_bytes(int d) {
    const int ldh = d | 1, C = (d + KCH - 1) / KCH;
    return ((size_t)d * ldh + 8 * (size_t)d + 2 * (size_t)C * d + 32) * sizeof(double);
}

// f(i, j, H[i][j] by reference) for this thread's share of the d x d elements, idx = tid, tid + T, ... without a division
// per element
template <typename F>
__device__ inline void h_each(const HLds &s, F f) {
    const int T = blockDim.x, di = T / s.d, dj = T - di * s.d;
    int i = threadIdx.x / s.d, j = threadIdx.x - i * s.d;
    while (i < s.d) {
        f(i, j, s.H[i * s.ldh + j]);
        i += di; j += dj;
        if (j >= s.d) { j -= s.d; i++; }
    }
}

__device__ inline void h_load(const HLds &s, const double *__restrict__ Hg) {
    for (int idx = threadIdx.x; idx < s.d * s.d; idx += blockDim.x) s.H[(idx / s.d) * s.ldh + idx % s.d] = Hg[idx];
}

__device__ inline void h_store(const HLds &s, double *__restrict__ Hg) {
    for (int idx = threadIdx.x; idx < s.d * s.d; idx += blockDim.x) Hg[idx] = s.H[(idx / s.d) * s.ldh + idx % s.d];
}

// the partial sums of up to two products, v -> H v (TRANS = false: out[o] = sum_k H[o][k] v[k]) or H^T v (TRANS = true:
// out[o] = sum_k H[k][o] v[k]); with C == 1 the one partial sum is the result and goes straight to out
template <bool T0, bool T1>
__device__ inline void mv_partials(const HLds &s, int n_products, const double *v0, double *out0, const double *v1, double *out1) {
#pragma clang fp contract(off)
    const int d = s.d, per = s.C * d;
    for (int it = threadIdx.x; it < n_products * per; it += blockDim.x) {
        const int which = it >= per, r = which ? it - per : it;
        const int c = r / d, o = r - c * d;
        const bool tr = which ? T1 : T0;
        const double *v = which ? v1 : v0;
        const int k0 = c * KCH, k1 = min(k0 + KCH, d);
        double acc = 0.0;
        if (tr) for (int k = k0; k < k1; k++) acc += s.H[k * s.ldh + o] * v[k];
        else    for (int k = k0; k < k1; k++) acc += s.H[o * s.ldh + k] * v[k];
        double *dst = s.C == 1 ? (which ? out1 : out0) : s.part[which];
        dst[r] = acc;
    }
}

__device__ inline void mv_combine(const HLds &s, int n_products, double *out0, double *out1) {
#pragma clang fp contract(off)
    if (s.C == 1) return;                                // uniform: the partials already are the results
    lds_barrier();
    for (int it = threadIdx.x; it < n_products * s.d; it += blockDim.x) {
        const int which = it >= s.d, o = which ? it - s.d : it;
        double acc = 0.0;
        for (int c = 0; c < s.C; c++) acc += s.part[which][c * s.d + o];
        (which ? out1 : out0)[o] = acc;
    }
}

// out0 = op0(H) v0 (and out1 = op1(H) v1), complete and visible to the whole workgroup on return
template <bool T0, bool T1>
__device__ inline void matvec(const HLds &s, int n_products, const double *v0, double *out0, const double *v1 = nullptr,
                              double *out1 = nullptr) {
    mv_partials<T0, T1>(s, n_products, v0, out0, v1, out1);
    mv_combine(s, n_products, out0, out1);
    lds_barrier();
}

// partial sums of a . b into sc[base .. base + C); dot_total adds them in chunk order (every thread, after a barrier)
__device__ inline void dot_partials(const HLds &s, const double *a, const double *b, int base) {
#pragma clang fp contract(off)
    if ((int)threadIdx.x < s.C) {
        const int k0 = threadIdx.x * KCH, k1 = min(k0 + KCH, s.d);
        double acc = 0.0;
        for (int k = k0; k < k1; k++) acc += a[k] * b[k];
        s.sc[base + threadIdx.x] = acc;
    }
}

__device__ inline double dot_total(const HLds &s, int base) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int c = 0; c < s.C; c++) acc += s.sc[base + c];
    return acc;
}

// LOCABAL.py:50-67, one wavefront, lane = column.  w_user[u] = W[user], or 0 for a user outside W (a real weight is > 0).
// p, q are copies: the weighted update and then the plain one (the reference's `else` is commented out) both use them.
template <int EPL>
__global__ __launch_bounds__(64) void locabal_ordered_kernel(double *__restrict__ P, double *__restrict__ Q, int d, int ld,
                                                             const double *__restrict__ w_user, const int32_t *__restrict__ u_idx,
                                                             const int32_t *__restrict__ i_idx, const double *__restrict__ rating,
                                                             int64_t n, double lr, double regU, double regI,
                                                             double *__restrict__ loss_out) {
#pragma clang fp contract(off)
    const LaneRow<double, EPL> R(threadIdx.x, d, ld);
    double loss = 0.0;
    for (int64_t t = 0; t < n; t++) {
        const int u = u_idx[t], i = i_idx[t];
        double p[EPL], q[EPL], pn[EPL], qn[EPL];
        R.load(p, P, u);
        R.load(q, Q, i);
        const double err = rating[t] - row_dot(p, q);
        const double w = w_user[u];
        loss += w != 0.0 ? w * (err * err) : err * err;
#pragma unroll
        for (int e = 0; e < EPL; e++) { pn[e] = p[e]; qn[e] = q[e]; }
        if (w != 0.0) {
            const double we = w * err;
#pragma unroll
            for (int e = 0; e < EPL; e++) {
                pn[e] += lr * (we * q[e] - regU * p[e]);
                qn[e] += lr * (we * p[e] - regI * q[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            pn[e] += lr * (err * q[e] - regU * p[e]);
            qn[e] += lr * (err * p[e] - regI * q[e]);
        }
        R.store(P, u, pn);
        R.store(Q, i, qn);
    }
    if (R.lane == 0) *loss_out = loss;
}

// LOCABAL.py:68-80, edge by edge: p = P[u], q = P[k] (copies); e = sim - (p^T H) . q; slot = alpha*e^2;
// H += ((lr*alpha)*e) * (p_i*q_j); H -= (lr*regS) * H; P[u] += ((lr*alpha)*e) * (H q); P[k] += ((lr*alpha)*e) * (H^T p)
// with the new H, the old p, and P[k] being the just-updated row when k == u.
__global__ __launch_bounds__(1024) void locabal_social_kernel(double *__restrict__ P, double *__restrict__ Hg, int d, int ld,
                                                              const int32_t *__restrict__ eu, const int32_t *__restrict__ ek,
                                                              const double *__restrict__ esim, int64_t n_edges, double lr,
                                                              double alpha, double regS, double *__restrict__ slots) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const HLds s = carve_h(smem, d);
    const int tid = threadIdx.x;
    double *pv = s.vec[0], *qv = s.vec[1], *tv = s.vec[2], *hq = s.vec[3], *hp = s.vec[4];
    h_load(s, Hg);
    const double la = lr * alpha, decay = lr * regS;
    const bool col = tid < d;
    for (int64_t t = 0; t < n_edges; t++) {
        const int u = eu[t], k = ek[t];
        double p = 0.0, q = 0.0;
        if (col) {
            p = P[(int64_t)u * ld + tid]; q = P[(int64_t)k * ld + tid];
            pv[tid] = p; qv[tid] = q;
        }
        lds_barrier();                                           // also orders h_load before the first product
        matvec<true, true>(s, 1, pv, tv);                          // p^T H
        dot_partials(s, tv, qv, 0);
        lds_barrier();
        const double e = esim[t] - dot_total(s, 0);
        if (tid == 0) slots[t] = alpha * (e * e);
        const double ce = la * e;
        h_each(s, [&](int i, int j, double &hij) {
            double h = hij;
            h += ce * (pv[i] * qv[j]);
            h -= decay * h;
            hij = h;
        });
        lds_barrier();
        matvec<false, true>(s, 2, qv, hq, pv, hp);                 // H q and H^T p
        if (col) {
            const double pu = p + ce * hq[tid];
            P[(int64_t)u * ld + tid] = pu;
            P[(int64_t)k * ld + tid] = (k == u ? pu : q) + ce * hp[tid];      // k == u: onto the row just written
        }
    }
    lds_barrier();
    h_store(s, Hg);
}

// out = 2 * H (H^T v): the reference's (H.H^T + (H.H^T)^T) . v without forming the d x d product (tmp: scratch vector)
__device__ inline void metric_times(const HLds &s, const double *v, double *tmp, double *out) {
    matvec<true, true>(s, 1, v, tmp);
    matvec<false, false>(s, 1, tmp, out);
}

// SocialFD.py:28-72, rating by rating.  x = P[u] and y = Q[i] are VIEWS in the reference: Q[i]'s update sees the new P[u],
// and the trailing P[u] += lr*(err*x - regU*x), Q[i] += lr*(err*y - regI*y) see the updated rows.  v = x - y;
// dist = ((v H) H^T) . v, c = v . v; err = r - (((Bi + Bu) + mean) - dist); loss += err^2, then the band's term.
//   r > 0.7        H -= lr*((err+ea)*(H*c));  P[u] -= lr*((err+ea)*g);         Q[i] += lr*((err+ea)*g')
//   r <= 0.5, <1   H += lr*((ea-err)*(H*c));  P[u] += lr*((ea-err)*g);         Q[i] += lr*((err-ea)*g')
//   r <= 0.5, >=1  H -= (lr*err)*(H*c);       P[u] += lr*((-err)*g);           Q[i] += lr*(err*g')
//   otherwise      H -= lr*(err*(H*c));       P[u] += lr*((-err)*g - regU*x);  Q[i] += lr*(err*g' - regI*y)
// with ea = eta*alpha, g = 2 H (H^T v) on the new H and g' the same on v' = P[u]_new - y.
__global__ __launch_bounds__(1024) void socialfd_ordered_kernel(double *__restrict__ P, double *__restrict__ Q, double *__restrict__ Bu,
                                                                double *__restrict__ Bi, double *__restrict__ Hg, int d, int ld,
                                                                const int32_t *__restrict__ u_idx, const int32_t *__restrict__ i_idx,
                                                                const double *__restrict__ rating, int64_t n, double lr, double regU,
                                                                double regI, double ea, double mean, double *__restrict__ loss_out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const HLds s = carve_h(smem, d);
    const int tid = threadIdx.x;
    double *vv = s.vec[0], *tv = s.vec[1], *sv = s.vec[2], *g1 = s.vec[3], *v2 = s.vec[4], *g2 = s.vec[5];
    h_load(s, Hg);
    double loss = 0.0;                                              // thread 0's is the pass' loss
    const bool col = tid < d;
    for (int64_t t = 0; t < n; t++) {
        const int u = u_idx[t], i = i_idx[t];
        const double r = rating[t];
        double x = 0.0, y = 0.0;
        if (col) {
            x = P[(int64_t)u * ld + tid]; y = Q[(int64_t)i * ld + tid];
            vv[tid] = x - y;
        }
        if (tid == 0) { s.sc[8] = Bu[u]; s.sc[9] = Bi[i]; }      // the biases belong to thread 0
        lds_barrier();
        metric_times(s, vv, tv, sv);                                // sv = H (H^T v) with the old H (tv = v H)
        dot_partials(s, sv, vv, 0);
        dot_partials(s, vv, vv, 16);
        lds_barrier();
        const double dist = dot_total(s, 0), c = dot_total(s, 16);
        const double bu = s.sc[8], bi = s.sc[9];
        const double err = r - (((bi + bu) + mean) - dist);
        const bool high = r > 0.7, low = !high && r <= 0.5, within = dist < 1.0;
        loss += err * err;
        if (high) loss += ea * dist;
        else if (low) loss += ea * fabs(1.0 - fmin(dist, 1.0));
        h_each(s, [&](int, int, double &hij) {
            double h = hij;
            const double dh = h * c;
            if (high) h -= lr * ((err + ea) * dh);
            else if (low && within) h += lr * ((ea - err) * dh);
            else if (low) h -= (lr * err) * dh;
            else h -= lr * (err * dh);
            hij = h;
        });
        lds_barrier();
        metric_times(s, vv, tv, g1);
        double xn = x;
        if (col) {
            const double g = 2.0 * g1[tid];
            if (high) xn = x - lr * ((err + ea) * g);
            else if (low && within) xn = x + lr * ((ea - err) * g);
            else if (low) xn = x + lr * ((-err) * g);
            else xn = x + lr * ((-err) * g - regU * x);
            v2[tid] = xn - y;
        }
        lds_barrier();
        metric_times(s, v2, tv, g2);
        if (col) {
            const double g = 2.0 * g2[tid];
            double yn;
            if (high) yn = y + lr * ((err + ea) * g);
            else if (low && within) yn = y + lr * ((err - ea) * g);
            else if (low) yn = y + lr * (err * g);
            else yn = y + lr * (err * g - regI * y);
            P[(int64_t)u * ld + tid] = xn + lr * (err * xn - regU * xn);
            Q[(int64_t)i * ld + tid] = yn + lr * (err * yn - regI * yn);
        }
        if (tid == 0) {
            Bu[u] = bu + lr * (err - regU * bu);
            Bi[i] = bi + lr * (err - regI * bi);
        }
        lds_barrier();                                            // sc[8..9] and the vectors are rewritten by the next rating
    }
    if (tid == 0) *loss_out = loss;
    h_store(s, Hg);
}

// SocialFD.py:74-86: step k = user step_user[k] (data.user order), x = P[u] a view that moves as the followees go by.
// Per followee f (w = x - P[f]): slot = ((w H) H^T) . w; delta = H (H^T w) + H^T (H w); c = w . w;
// P[u] -= ((lr*eta)*beta) * delta; H -= ((lr*eta)*beta) * (H*c).  f == u reads the moving row itself (w = 0).
__global__ __launch_bounds__(1024) void socialfd_social_kernel(double *__restrict__ P, double *__restrict__ Hg, int d, int ld,
                                                               const int32_t *__restrict__ step_user, int64_t n_steps,
                                                               const int64_t *__restrict__ fe_ptr, const int32_t *__restrict__ fe_ids,
                                                               double coef, double *__restrict__ slots) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const HLds s = carve_h(smem, d);
    const int tid = threadIdx.x;
    double *wv = s.vec[0], *tv = s.vec[1], *av = s.vec[2], *sv = s.vec[3], *bv = s.vec[4];
    h_load(s, Hg);
    lds_barrier();
    for (int64_t k = 0; k < n_steps; k++) {
        const int u = step_user[k];
        const int64_t b0 = fe_ptr[k], b1 = fe_ptr[k + 1];
        if (b0 == b1) continue;                                     // uniform
        const bool col = tid < d;
        double x = col ? P[(int64_t)u * ld + tid] : 0.0;
        for (int64_t j = b0; j < b1; j++) {
            const int f = fe_ids[j];
            if (col) wv[tid] = x - (f == u ? x : P[(int64_t)f * ld + tid]);
            lds_barrier();
            matvec<true, false>(s, 2, wv, tv, wv, av);              // H^T w and H w
            matvec<false, true>(s, 2, tv, sv, av, bv);              // H (H^T w) and H^T (H w)
            dot_partials(s, sv, wv, 0);
            dot_partials(s, wv, wv, 16);
            lds_barrier();
            const double term = dot_total(s, 0), c = dot_total(s, 16);
            if (tid == 0) slots[j] = term;
            if (col) x -= coef * (sv[tid] + bv[tid]);
            h_each(s, [&](int, int, double &hij) { hij = hij - coef * (hij * c); });
            lds_barrier();
        }
        if (tid < d) P[(int64_t)u * ld + tid] = x;
    }
    h_store(s, Hg);
}

inline int h_auto_waves(int d) {
    // eight elements of H per thread: measured at d = 10 / 64 / 128, 1 / 8 / 16 wavefronts are within
    // a few percent of the best count; fewer leave the d^2 update and the products to too few lanes
    return std::max(1, std::min(QREC_SOCIAL_MAX_WAVES, (d * d + 511) / 512));
}

}  // namespace

extern "C" {

int qrec_rste_sgd_ordered(double *d_P, double *d_Q, int32_t d, int32_t ld, const int64_t *d_fe_indptr, const int32_t *d_fe_ids,
                          const double *d_fe_w, const double *d_fe_den, const int32_t *d_u, const int32_t *d_i,
                          const double *d_rating, int64_t n, double lr, double alpha, double regU, double regI, double *d_loss,
                          void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_loss && n >= 0, "qrec_rste_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_rating && d_fe_indptr && d_fe_den), "qrec_rste_sgd_ordered: null index array");
    if (int rc = check_lane_row("qrec_rste_sgd_ordered", QREC_F64, d, ld)) return rc;
    hipStream_t st = as_stream(stream);
    if (n == 0) { QREC_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), st)); return QREC_OK; }
    return with_epl(d, [&](auto epl) {
        return launch_waves(rste_ordered_kernel<epl()>, 1, st, d_P, d_Q, d, ld, d_fe_indptr, d_fe_ids, d_fe_w, d_fe_den, d_u, d_i, d_rating, n,
                            lr, alpha, regU, regI, d_loss);
    });
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
    if (int rc = check_lane_row("qrec_social_user_pass", QREC_F64, d, ld)) return rc;
    QREC_REQUIRE(n_waves >= 1 && n_waves <= QREC_SOCIAL_MAX_WAVES, "qrec_social_user_pass: need 1 <= n_waves <= %d, got %d",
                 QREC_SOCIAL_MAX_WAVES, n_waves);
    if (n_steps == 0 || n_levels == 0) return QREC_OK;
    return with_epl(d, [&](auto epl) {
        auto launch = [&](auto m) {
            return launch_waves(social_user_levels_kernel<epl(), m()>, n_waves, as_stream(stream), d_P, d, ld, d_step_user, d_fe_indptr, d_fe_ids,
                                d_fe_w, d_fr_indptr, d_fr_ids, d_fr_w, d_order, d_level_ptr, n_levels, lr, coef, d_slots);
        };
        return mode == QREC_SOCIAL_SOCIALMF ? launch(int_c<0>{}) : mode == QREC_SOCIAL_SOREG ? launch(int_c<1>{}) : launch(int_c<2>{});
    });
}

int qrec_sorec_relation_pass(double *d_P, double *d_Z, int32_t d, int32_t ld, const int32_t *d_rel_u, const int32_t *d_rel_v,
                             const double *d_rel_t, const double *d_rel_w, int64_t n_rel, const int32_t *d_order,
                             const int32_t *d_level_ptr, int32_t n_levels, int32_t n_waves, double lr, double regS, double regZ,
                             double *d_slots, void *stream) {
    QREC_REQUIRE(d_P && d_Z && n_rel >= 0 && n_rel < (int64_t)1 << 31 && n_levels >= 0, "qrec_sorec_relation_pass: null argument");
    QREC_REQUIRE(n_rel == 0 || (d_rel_u && d_rel_v && d_rel_t && d_rel_w && d_order && d_level_ptr && d_slots),
                 "qrec_sorec_relation_pass: null relation array");
    if (int rc = check_lane_row("qrec_sorec_relation_pass", QREC_F64, d, ld)) return rc;
    QREC_REQUIRE(n_waves >= 1 && n_waves <= QREC_SOCIAL_MAX_WAVES, "qrec_sorec_relation_pass: need 1 <= n_waves <= %d, got %d",
                 QREC_SOCIAL_MAX_WAVES, n_waves);
    if (n_rel == 0 || n_levels == 0) return QREC_OK;
    return with_epl(d, [&](auto epl) {
        return launch_waves(sorec_levels_kernel<epl()>, n_waves, as_stream(stream), d_P, d_Z, d, ld, d_rel_u, d_rel_v, d_rel_t, d_rel_w, d_order,
                            d_level_ptr, n_levels, lr, regS, regZ, d_slots);
    });
}

int qrec_loss_fold(double *d_running, const double *d_slots, int64_t n, void *stream) {
    QREC_REQUIRE(d_running && n >= 0 && (n == 0 || d_slots), "qrec_loss_fold: null argument");
    if (n == 0) return QREC_OK;
    hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(64), 0, as_stream(stream), d_running, d_slots, n);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

// d_H is one dense row-major [d][d] matrix; all four entries refuse d > QREC_SOCIAL_H_MAX_D before touching anything
#define QREC_H_WIDTH(name)                                                                                                      \
    do {                                                                                                                        \
        QREC_REQUIRE(d >= 1 && ld >= d, name ": need d >= 1, ld >= d (got d=%d ld=%d)", d, ld);                                   \
        if (d > QREC_SOCIAL_H_MAX_D) {                                                                                          \
            ::qrec::set_error(name ": width %d above the supported %d (H stays in LDS)", d, QREC_SOCIAL_H_MAX_D);                \
            return QREC_ERR_UNSUPPORTED;                                                                                        \
        }                                                                                                                       \
    } while (0)
#define QREC_H_WAVES(name)                                                                                                      \
    QREC_REQUIRE(n_waves >= 0 && n_waves <= QREC_SOCIAL_MAX_WAVES, name ": need 0 (auto) <= n_waves <= %d, got %d",               \
                 QREC_SOCIAL_MAX_WAVES, n_waves);                                                                               \
    const int nw = std::max(n_waves ? n_waves : h_auto_waves(d), (d + 63) / 64); /* thread j owns element j of a row */         \
    const size_t lds = h_lds_bytes(d)
#define QREC_H_LDS(kernel)                                                                                                      \
    if (lds > 64 * 1024)                                                                                                        \
    QREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))

int qrec_locabal_sgd_ordered(double *d_P, double *d_Q, int32_t d, int32_t ld, const double *d_w_user, const int32_t *d_u,
                             const int32_t *d_i, const double *d_rating, int64_t n, double lr, double regU, double regI,
                             double *d_loss, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_loss && n >= 0, "qrec_locabal_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_rating && d_w_user), "qrec_locabal_sgd_ordered: null index array");
    QREC_H_WIDTH("qrec_locabal_sgd_ordered");
    hipStream_t st = as_stream(stream);
    if (n == 0) { QREC_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), st)); return QREC_OK; }
    return with_epl<2>(d, [&](auto epl) {       // QREC_H_WIDTH has refused d > 128
        return launch_waves(locabal_ordered_kernel<epl()>, 1, st, d_P, d_Q, d, ld, d_w_user, d_u, d_i, d_rating, n, lr, regU, regI, d_loss);
    });
}

int qrec_locabal_social_pass(double *d_P, double *d_H, int32_t d, int32_t ld, const int32_t *d_edge_u, const int32_t *d_edge_k,
                             const double *d_edge_sim, int64_t n_edges, int32_t n_waves, double lr, double alpha, double regS,
                             double *d_slots, void *stream) {
    QREC_REQUIRE(d_P && d_H && n_edges >= 0, "qrec_locabal_social_pass: null argument");
    QREC_REQUIRE(n_edges == 0 || (d_edge_u && d_edge_k && d_edge_sim && d_slots), "qrec_locabal_social_pass: null edge array");
    QREC_H_WIDTH("qrec_locabal_social_pass");
    QREC_H_WAVES("qrec_locabal_social_pass");
    if (n_edges == 0) return QREC_OK;
    QREC_H_LDS(locabal_social_kernel);
    hipLaunchKernelGGL(locabal_social_kernel, dim3(1), dim3(64 * nw), lds, as_stream(stream), d_P, d_H, d, ld, d_edge_u, d_edge_k,
                       d_edge_sim, n_edges, lr, alpha, regS, d_slots);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_socialfd_sgd_ordered(double *d_P, double *d_Q, double *d_Bu, double *d_Bi, double *d_H, int32_t d, int32_t ld,
                              const int32_t *d_u, const int32_t *d_i, const double *d_rating, int64_t n, int32_t n_waves, double lr,
                              double regU, double regI, double eta, double alpha, double global_mean, double *d_loss, void *stream) {
    QREC_REQUIRE(d_P && d_Q && d_Bu && d_Bi && d_H && d_loss && n >= 0, "qrec_socialfd_sgd_ordered: null argument");
    QREC_REQUIRE(n == 0 || (d_u && d_i && d_rating), "qrec_socialfd_sgd_ordered: null index array");
    QREC_H_WIDTH("qrec_socialfd_sgd_ordered");
    QREC_H_WAVES("qrec_socialfd_sgd_ordered");
    hipStream_t st = as_stream(stream);
    if (n == 0) { QREC_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), st)); return QREC_OK; }
    QREC_H_LDS(socialfd_ordered_kernel);
    hipLaunchKernelGGL(socialfd_ordered_kernel, dim3(1), dim3(64 * nw), lds, st, d_P, d_Q, d_Bu, d_Bi, d_H, d, ld, d_u, d_i, d_rating, n,
                       lr, regU, regI, eta * alpha, global_mean, d_loss);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_socialfd_social_pass(double *d_P, double *d_H, int32_t d, int32_t ld, const int32_t *d_step_user, int64_t n_steps,
                              const int64_t *d_fe_indptr, const int32_t *d_fe_ids, int32_t n_waves, double lr, double eta, double beta,
                              double *d_slots, void *stream) {
    QREC_REQUIRE(d_P && d_H && n_steps >= 0, "qrec_socialfd_social_pass: null argument");
    QREC_REQUIRE(n_steps == 0 || (d_step_user && d_fe_indptr && d_fe_ids && d_slots), "qrec_socialfd_social_pass: null step array");
    QREC_H_WIDTH("qrec_socialfd_social_pass");
    QREC_H_WAVES("qrec_socialfd_social_pass");
    if (n_steps == 0) return QREC_OK;
    QREC_H_LDS(socialfd_social_kernel);
    hipLaunchKernelGGL(socialfd_social_kernel, dim3(1), dim3(64 * nw), lds, as_stream(stream), d_P, d_H, d, ld, d_step_user, n_steps,
                       d_fe_indptr, d_fe_ids, (lr * eta) * beta, d_slots);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}
#undef QREC_H_WIDTH
#undef QREC_H_WAVES
#undef QREC_H_LDS

}  // extern "C"
