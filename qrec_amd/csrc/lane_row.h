// The lane-per-column row of the order-exact walkers (sgd_walkers.hip, social.hip, bpr_exact.hip), stated once.
//
// One wavefront owns an embedding row of d <= 256 columns: lane l holds columns l, l + 64, ... in EPL = 1, 2 or 4 registers
// (T v[EPL], column l + 64 e in v[e]; columns past d hold 0 and are never stored, so a table's pad columns stay as they were).
// Every sum is taken in one fixed order -- per lane e = 0 ... EPL-1, then wave_sum_dpp's tree over the lanes -- and every
// product and sum is rounded on its own, as numpy does it: that is what makes the walkers reproduce the reference bit for bit
// between each other and to 1e-11 against it.
//
// CONTRACTION.  HIP compiles with -ffp-contract=fast, and `#pragma clang fp contract(off)` covers the statements of the
// compound statement it opens, NOT the functions called from there: a namespace-scope __device__ inline helper doing
// p[e] += g * q[e] compiles to v_fmac_f64 even when its caller has the pragma (probed on this compiler), and to v_mul_f64 +
// v_add_f64 with the pragma as the first line of its OWN body -- as a lambda inside such a kernel does.  So every helper here
// whose body has a multiply feeding an add carries the pragma itself, and so must any helper that is lifted out of a walker.
// The pragma is not at file scope: it would reach every translation unit that includes this header.
#pragma once
#include "common.h"

namespace qrec {

template <typename T> __device__ inline T dev_exp(T x);
template <> __device__ inline float dev_exp<float>(float x) { return expf(x); }
template <> __device__ inline double dev_exp<double>(double x) { return exp(x); }

// -log(sigmoid(x)) = softplus(-x), evaluated without forming sigmoid first: in fp32 sigmoid(x)
// underflows to 0 for x < -88.7 and -log(0) = inf, while the reference's fp64 value (= -x) is
// finite down to x ~ -745.  Same value to rounding wherever the direct form is finite.
//
// The float overload (the throughput kernels of bpr_sgd.hip) is ONE evaluation, log1p(exp(-|x|)) + max(-x, 0), and not the two-armed
// form of the double overload below: a wavefront of those kernels carries several groups with unrelated x, the compiler keeps the
// two arms as a real branch on the sign, and with mixed signs both arms run -- 235 of the item-major loop's ~450 vector instructions
// per triplet.  It is the two-armed form bit for bit: with L = log1pf(expf(-|x|)) >= +0 (expf >= +0, log1pf(+0) = +0),
//   x >= 0 (and +-0): -|x| = -x, and the added term is max(-x, 0) = +-0, which leaves L as it is (L is never -0);
//   x < 0:            -|x| = x, and L + (-x) is the arm's -x + L, one commutative add of the same two addends;
//   x = +inf: 0 + 0;  x = -inf: 0 + inf;  NaN: L is NaN and NaN + 0 is NaN, as the x < 0 arm gave.
__device__ inline float neg_log_sigmoid(float x) {
    return log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f);
}
__device__ inline double neg_log_sigmoid(double x) {
    return x >= 0.0 ? log1p(exp(-x)) : (-x + log1p(exp(x)));
}

// this lane's view of [rows][ld] tables of width d
template <typename T, int EPL>
struct LaneRow {
    int lane, d, ld;
    __device__ LaneRow(int lane_, int d_, int ld_) : lane(lane_), d(d_), ld(ld_) {}
    __device__ bool valid(int e) const { return lane + 64 * e < d; }
    __device__ void load(T (&v)[EPL], const T *tab, int64_t row) const {      // 0 past d
        const T *p = tab + row * ld;
#pragma unroll
        for (int e = 0; e < EPL; e++) v[e] = valid(e) ? p[lane + 64 * e] : T(0);
    }
    // two rows under ONE mask test: a masked load is a branch, and with one branch per row the second row's index load and
    // its wait come after the first row's load instead of beside it (measured: 6 % of mf_ordered_kernel's step at d = 10)
    __device__ void load2(T (&a)[EPL], const T *ta, int64_t ra, T (&b)[EPL], const T *tb, int64_t rb) const {
        const T *pa = ta + ra * ld, *pb = tb + rb * ld;
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            const bool ok = valid(e);
            a[e] = ok ? pa[lane + 64 * e] : T(0);
            b[e] = ok ? pb[lane + 64 * e] : T(0);
        }
    }
    __device__ void store(T *tab, int64_t row, const T (&v)[EPL]) const {     // masked past d
        T *p = tab + row * ld;
#pragma unroll
        for (int e = 0; e < EPL; e++)
            if (valid(e)) p[lane + 64 * e] = v[e];
    }
};

// a . b over the whole row, in every lane (wave_sum_dpp, common.h: DPP, not the LDS crossbar)
template <typename T, int EPL>
__device__ inline T row_dot(const T (&a)[EPL], const T (&b)[EPL]) {
#pragma clang fp contract(off)
    T v = 0;
#pragma unroll
    for (int e = 0; e < EPL; e++) v += a[e] * b[e];
    return wave_sum_dpp(v);
}

// |r|^2 accumulated in fp64 whatever the tables' type: the running sums of squares of TBPR / SBPR
template <typename T, int EPL>
__device__ inline double row_norm2(const T (&r)[EPL]) {
#pragma clang fp contract(off)
    double v = 0.0;
#pragma unroll
    for (int e = 0; e < EPL; e++) v += (double)r[e] * (double)r[e];
    return wave_sum_dpp(v);
}

// ---- host side: d -> EPL and dtype -> T, and the argument check that goes with them
inline int lane_row_epl(int d) { return d <= 64 ? 1 : d <= 128 ? 2 : 4; }

// f(int_c<EPL>{}); MAX_EPL = 2 for an entry point that refuses d > 128 and has no EPL = 4 kernel
template <int MAX_EPL = 4, typename F>
auto with_epl(int d, F f) {
    const int epl = lane_row_epl(d);
    if (epl == 1) return f(int_c<1>{});
    if constexpr (MAX_EPL >= 4) {
        if (epl == 4) return f(int_c<4>{});
    }
    return f(int_c<2>{});
}

// f(T{}, int_c<EPL>{}) with T = double or float: `using T = decltype(t)` names the tables' type
template <typename F>
auto with_row_type(int dtype, int d, F f) {
    return with_epl(d, [&](auto epl) { return dtype == QREC_F64 ? f(double{}, epl) : f(float{}, epl); });
}

// a walker's launch: ONE workgroup of `waves` wavefronts, no dynamic LDS
template <typename K, typename... A>
int launch_waves(K kernel, int waves, hipStream_t st, A... args) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64 * waves), 0, st, args...);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

// the walkers' common refusal; fn is the entry point's name (an fp64-only entry point passes QREC_F64)
inline int check_lane_row(const char *fn, int dtype, int d, int ld) {
    QREC_REQUIRE(d >= 1 && d <= 256 && ld >= d, "%s: need 1 <= d <= 256, ld >= d (got d=%d ld=%d)", fn, d, ld);
    QREC_REQUIRE(dtype == QREC_F32 || dtype == QREC_F64, "%s: bad dtype %d", fn, dtype);
    return QREC_OK;
}

}  // namespace qrec
