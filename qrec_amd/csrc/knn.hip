// Memory-based rating models, fp64 (model/rating/{UserKNN,ItemKNN,SlopeOne}.py, util/qmath.py:19-115): co-rating
// similarities between every query (a test user or item) and every candidate (a training user or item), the stable
// top-K of each query's neighbour sequence, and the predictions that walk those neighbours.  Every product and sum is
// rounded on its own (no FMA contraction) and every sum runs in the reference's order, so a run is bit-identical to the
// reference's arithmetic and to the next run.  DESIGN.md s5.7 has the contract.
//
// The reference squares with Python's ``x ** 2``, i.e. the C library's pow(x, 2.0), which is not always the correctly rounded
// x * x.  The squares are therefore inputs: d_q_sq / d_c_sq hold pow(a - m1, 2) / pow(b - m2, 2) (pcc) or pow(a, 2) /
// pow(b, 2) (cos, euclidean) per entry, computed on the host by the same pow (engine.libm_squares).
//
// Sweep: one workgroup per (query, tile of QREC_KNN_TILE candidates).  The query's row is walked in dict order; each row
// entry's key (item or user) owns a column of (candidate label, value) sorted by label, so a binary search finds the
// tile's range in it.  The entries of one range are distinct candidates (no conflicts); a barrier separates one row
// entry from the next, so every candidate's accumulators see the row in order.  The accumulators live in LDS.
// Top-K: one workgroup per query, a radix select over the 96-bit key (value descending, then sequence position), then a
// bitonic sort of the <= QREC_KNN_MAX_K survivors.
#include <algorithm>
#include <climits>

#include "common.h"

#pragma clang fp contract(off)

using namespace qrec;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = QREC_KNN_TILE;
constexpr int kMaxK = QREC_KNN_MAX_K;
constexpr int kBuckets = 2048;

static_assert(kMaxK == kThreads, "the bitonic sort puts one survivor on each thread");

// first position p in [lo, hi) with a[p] >= x (a ascending)
__device__ inline int64_t lower_bound_i32(const int32_t *__restrict__ a, int64_t lo, int64_t hi, int32_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <int M>
__global__ __launch_bounds__(kThreads) void knn_sweep_kernel(int64_t n_tiles, const int64_t *__restrict__ q_indptr,
                                                             const int32_t *__restrict__ q_keys, const double *__restrict__ q_vals,
                                                             const double *__restrict__ q_means, const double *__restrict__ q_sq,
                                                             int64_t n_keys,
                                                             const int64_t *__restrict__ c_indptr, const int32_t *__restrict__ c_labels,
                                                             const double *__restrict__ c_vals, const double *__restrict__ c_sq,
                                                             int64_t n_cands,
                                                             const double *__restrict__ c_means, double *__restrict__ out, int64_t ld_out,
                                                             int32_t *__restrict__ count_out, int64_t ld_count) {
    __shared__ double s_a[kTile], s_b[(M == QREC_KNN_PCC || M == QREC_KNN_COS) ? kTile : 1],
        s_c[(M == QREC_KNN_PCC || M == QREC_KNN_COS) ? kTile : 1];
    __shared__ int32_t s_n[(M == QREC_KNN_PCC || M == QREC_KNN_SLOPEONE) ? kTile : 1];
    __shared__ int64_t s_lo[kThreads], s_hi[kThreads];
    __shared__ double s_v[kThreads], s_sq[kThreads];
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x / n_tiles, tile = (int64_t)blockIdx.x % n_tiles;
    const int64_t c0 = tile * kTile, c1 = min<int64_t>(c0 + kTile, n_cands);
    const int width = (int)(c1 - c0);
    for (int l = tid; l < width; l += kThreads) {
        s_a[l] = 0.0;
        if constexpr (M == QREC_KNN_PCC || M == QREC_KNN_COS) { s_b[l] = 0.0; s_c[l] = 0.0; }
        if constexpr (M == QREC_KNN_PCC || M == QREC_KNN_SLOPEONE) s_n[l] = 0;
    }
    const int64_t row_beg = q_indptr[t], row_end = q_indptr[t + 1];
    const double m1 = (M == QREC_KNN_PCC) ? q_means[t] : 0.0;
    for (int64_t base = row_beg; base < row_end; base += kThreads) {
        const int n = (int)min<int64_t>(kThreads, row_end - base);
        __syncthreads();                   // the previous chunk's walk is done with s_lo / s_hi / s_v (and the init)
        if (tid < n) {
            const int32_t key = q_keys[base + tid];
            int64_t lo = 0, hi = 0;
            if (key >= 0 && key < n_keys) {
                const int64_t b = c_indptr[key], e = c_indptr[key + 1];
                lo = lower_bound_i32(c_labels, b, e, (int32_t)c0);
                hi = lower_bound_i32(c_labels, lo, e, (int32_t)c1);
            }
            s_lo[tid] = lo; s_hi[tid] = hi;
            const double a = q_vals[base + tid];
            s_v[tid] = (M == QREC_KNN_PCC) ? a - m1 : a;
            s_sq[tid] = (M == QREC_KNN_SLOPEONE) ? 0.0 : q_sq[base + tid];
        }
        __syncthreads();
        for (int e = 0; e < n; ++e) {
            const int64_t lo = s_lo[e], hi = s_hi[e];
            if (lo == hi) continue;        // uniform: every thread reads the same LDS words
            const double a = s_v[e], a2 = s_sq[e];
            for (int64_t idx = lo + tid; idx < hi; idx += kThreads) {
                const int64_t lab = c_labels[idx];
                const int l = (int)(lab - c0);
                if (lab < c0 || lab >= c1) continue;      // an unsorted column cannot write outside the tile
                const double b = c_vals[idx];
                if constexpr (M == QREC_KNN_PCC) {
                    const double db = b - c_means[lab];
                    s_a[l] = s_a[l] + a * db;
                    s_b[l] = s_b[l] + a2;
                    s_c[l] = s_c[l] + c_sq[idx];
                    s_n[l] += 1;
                } else if constexpr (M == QREC_KNN_COS) {
                    s_a[l] = s_a[l] + a * b;
                    s_b[l] = s_b[l] + a2;
                    s_c[l] = s_c[l] + c_sq[idx];
                } else if constexpr (M == QREC_KNN_EUCLIDEAN) {
                    s_a[l] = s_a[l] + (a2 - c_sq[idx]);
                } else {
                    s_a[l] = s_a[l] + (a - b);
                    s_n[l] += 1;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    double *o = out + t * ld_out + c0;
    for (int l = tid; l < width; l += kThreads) {
        double r;
        if constexpr (M == QREC_KNN_PCC) {
            const double den = sqrt(s_b[l]) * sqrt(s_c[l]);
            r = den == 0.0 ? (s_n[l] > 0 ? 1.0 : 0.0) : s_a[l] / den;
        } else if constexpr (M == QREC_KNN_COS) {
            const double den = sqrt(s_b[l]) * sqrt(s_c[l]);
            r = den == 0.0 ? 0.0 : s_a[l] / den;
        } else if constexpr (M == QREC_KNN_EUCLIDEAN) {
            r = s_a[l] == 0.0 ? 0.0 : 1.0 / s_a[l];
        } else {
            const int32_t c = s_n[l];
            r = c == 0 ? 0.0 : s_a[l] / (double)c;
            count_out[t * ld_count + c0 + l] = c;
        }
        o[l] = r;
    }
}

// BT[j][s] = S[s][j] for j < m, s < n_rows: the test x test block, transposed through LDS in 32 x 32 tiles
__global__ __launch_bounds__(kThreads) void knn_transpose_kernel(const double *__restrict__ S, int64_t n_rows, int64_t ld_S, int64_t m,
                                                                 double *__restrict__ BT) {
    __shared__ double tileb[32][33];
    const int64_t j0 = (int64_t)blockIdx.x * 32, s0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;        // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int64_t s = s0 + r, j = j0 + tx;
        tileb[r][tx] = (s < n_rows && j < m) ? S[s * ld_S + j] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t j = j0 + r, s = s0 + tx;
        if (j < m && s < n_rows) BT[j * n_rows + s] = tileb[tx][r];
    }
}

struct Key {
    uint64_t hi;   // value, descending: a smaller key is a larger similarity
    uint32_t lo;   // position in the candidate sequence
};

__device__ inline Key make_key(double v, uint32_t pos) {
    if (v == 0.0) v = 0.0;                                   // -0.0 == 0.0 in the reference's sort
    const uint64_t bits = __builtin_bit_cast(uint64_t, v);
    const uint64_t asc = (bits >> 63) ? ~bits : (bits | (1ull << 63));
    return Key{~asc, pos};
}

__device__ inline bool key_less(const Key &a, const Key &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// passes over the 96-bit key from its most significant bit: {start bit, width}
__constant__ int kPassStart[9] = {0, 11, 22, 33, 44, 54, 64, 75, 86};
__constant__ int kPassWidth[9] = {11, 11, 11, 11, 10, 10, 11, 11, 10};

__device__ inline uint32_t key_digit(const Key &k, int start, int width) {
    const uint32_t mask = (1u << width) - 1;
    if (start < 64) return (uint32_t)(k.hi >> (64 - start - width)) & mask;
    return (k.lo >> (96 - start - width)) & mask;
}

// top F bits of k compared with those of p: -1, 0, 1
__device__ inline int key_cmp_top(const Key &k, const Key &p, int F) {
    if (F == 0) return 0;
    if (F <= 64) {
        const uint64_t a = k.hi >> (64 - F), b = p.hi >> (64 - F);
        return a < b ? -1 : (a > b ? 1 : 0);
    }
    if (k.hi != p.hi) return k.hi < p.hi ? -1 : 1;
    const uint32_t a = k.lo >> (96 - F), b = p.lo >> (96 - F);
    return a < b ? -1 : (a > b ? 1 : 0);
}

__device__ inline void set_digit(Key &p, int start, int width, uint32_t d) {
    if (start < 64) p.hi |= (uint64_t)d << (64 - start - width);
    else p.lo |= d << (96 - start - width);
}

struct Seq {
    const double *S, *BT;
    const int32_t *test_code, *lab2id;
    int64_t t, ld_S, n_queries;
    int64_t n1, start2, total;
    int64_t j;
    __device__ inline void at(int64_t e, double &v, uint32_t &pos, int32_t &code) const {
        if (e < n1) {
            v = BT[j * n_queries + e];
            pos = (uint32_t)e;
            code = test_code[e];
        } else {
            const int64_t L = start2 + (e - n1);
            v = S[t * ld_S + L];
            code = lab2id[L];
            pos = (uint32_t)(n1 + code);
        }
    }
};

__global__ __launch_bounds__(kThreads) void knn_topk_kernel(int64_t n_queries, const double *__restrict__ S, int64_t ld_S,
                                                            const double *__restrict__ BT, const int32_t *__restrict__ q_label,
                                                            const int32_t *__restrict__ test_code, const int32_t *__restrict__ lab2id,
                                                            int64_t n_cands, int k, int32_t *__restrict__ ids,
                                                            double *__restrict__ vals, int32_t *__restrict__ counts) {
    __shared__ uint32_t hist[kBuckets];
    __shared__ uint32_t s_part[kThreads];
    __shared__ uint32_t s_digit, s_before, s_cnt, s_n;
    __shared__ uint64_t k_hi[kMaxK];
    __shared__ uint32_t k_lo[kMaxK];
    __shared__ int32_t k_code[kMaxK];
    __shared__ double k_val[kMaxK];
    const int tid = threadIdx.x;
    Seq q;
    q.S = S; q.BT = BT; q.test_code = test_code; q.lab2id = lab2id; q.ld_S = ld_S; q.n_queries = n_queries;
    q.t = blockIdx.x;
    q.j = q_label[q.t];
    q.n1 = q.j >= 0 ? q.t : 0;
    q.start2 = q.j >= 0 ? q.j + 1 : 0;
    q.total = q.n1 + (n_cands - q.start2);
    const int64_t want = min<int64_t>(k, q.total);
    Key prefix{0, 0};
    int F = 0;
    if (q.total > k) {
        uint32_t need = (uint32_t)k;
        for (int p = 0; p < 9; ++p) {
            const int start = kPassStart[p], width = kPassWidth[p];
            for (int b = tid; b < kBuckets; b += kThreads) hist[b] = 0;
            __syncthreads();
            for (int64_t e = tid; e < q.total; e += kThreads) {
                double v; uint32_t pos; int32_t code;
                q.at(e, v, pos, code);
                const Key key = make_key(v, pos);
                if (key_cmp_top(key, prefix, F) == 0) atomicAdd(&hist[key_digit(key, start, width)], 1u);
            }
            __syncthreads();
            // the bucket where the running count reaches `need`: each thread sums 8 consecutive buckets, then a scan
            constexpr int per = kBuckets / kThreads;
            uint32_t local = 0;
            for (int b = 0; b < per; ++b) local += hist[tid * per + b];
            s_part[tid] = local;
            __syncthreads();
            if (tid == 0) {
                uint32_t run = 0;
                int owner = kThreads - 1;
                for (int w = 0; w < kThreads; ++w) {
                    if (run + s_part[w] >= need) { owner = w; break; }
                    run += s_part[w];
                }
                int d = owner * per;
                for (int b = 0; b < per; ++b, ++d) {
                    if (run + hist[d] >= need) break;
                    run += hist[d];
                }
                s_digit = (uint32_t)d; s_before = run; s_cnt = hist[d];
            }
            __syncthreads();
            set_digit(prefix, start, width, s_digit);
            F = start + width;
            need -= s_before;
            const bool done = s_cnt == need;
            __syncthreads();
            if (done) break;
        }
    }
    // survivors: every element whose top F bits do not exceed the prefix's (exactly `want` of them)
    if (tid == 0) s_n = 0;
    k_hi[tid] = ~0ull; k_lo[tid] = ~0u; k_code[tid] = 0; k_val[tid] = 0.0;
    __syncthreads();
    for (int64_t e = tid; e < q.total; e += kThreads) {
        double v; uint32_t pos; int32_t code;
        q.at(e, v, pos, code);
        const Key key = make_key(v, pos);
        if (key_cmp_top(key, prefix, F) <= 0) {
            const uint32_t slot = atomicAdd(&s_n, 1u);
            if (slot < (uint32_t)kMaxK) { k_hi[slot] = key.hi; k_lo[slot] = key.lo; k_code[slot] = code; k_val[slot] = v; }
        }
    }
    __syncthreads();
    // bitonic sort of the kMaxK slots by (hi, lo) ascending; empty slots carry the largest key
    for (int size = 2; size <= kMaxK; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int other = tid ^ stride;
            if (other > tid) {
                const bool up = (tid & size) == 0;
                const Key a{k_hi[tid], k_lo[tid]}, b{k_hi[other], k_lo[other]};
                if (key_less(b, a) == up) {
                    k_hi[tid] = b.hi; k_lo[tid] = b.lo; k_hi[other] = a.hi; k_lo[other] = a.lo;
                    const int32_t c = k_code[tid]; k_code[tid] = k_code[other]; k_code[other] = c;
                    const double v = k_val[tid]; k_val[tid] = k_val[other]; k_val[other] = v;
                }
            }
            __syncthreads();
        }
    }
    if (tid < want) {
        ids[q.t * k + tid] = k_code[tid];
        vals[q.t * k + tid] = k_val[tid];
    }
    if (tid == 0) counts[q.t] = (int32_t)want;
}

__device__ inline int64_t find_key(const int32_t *__restrict__ keys, int64_t lo, int64_t hi, int32_t x) {
    const int64_t p = lower_bound_i32(keys, lo, hi, x);
    return (p < hi && keys[p] == x) ? p : -1;
}

__global__ __launch_bounds__(kThreads) void knn_predict_kernel(int mode, int64_t n_rows, const int32_t *__restrict__ row_query,
                                                               const int32_t *__restrict__ row_other, const double *__restrict__ row_base,
                                                               const int32_t *__restrict__ nb_ids, const double *__restrict__ nb_vals,
                                                               const int32_t *__restrict__ nb_counts, int64_t n_queries, int k,
                                                               int64_t n_members, const int64_t *__restrict__ m_indptr,
                                                               const int32_t *__restrict__ m_keys, const double *__restrict__ m_vals,
                                                               int64_t n_nb, const double *__restrict__ nb_means, double *__restrict__ pred,
                                                               int32_t *__restrict__ status) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_rows) return;
    const int32_t t = row_query[r], other = row_other[r];
    double sum = 0.0, denom = 0.0;
    if (t >= 0 && t < n_queries && other >= 0) {
        const int cnt = min(nb_counts[t], k);
        for (int n = 0; n < cnt; ++n) {
            const int32_t code = nb_ids[(int64_t)t * k + n];
            if (code < 0 || code >= n_nb) continue;         // a test-only neighbour has no ratings
            const int32_t row = mode == 0 ? code : other, key = mode == 0 ? other : code;
            if (row >= n_members) continue;
            const int64_t p = find_key(m_keys, m_indptr[row], m_indptr[row + 1], key);
            if (p < 0) continue;
            const double s = nb_vals[(int64_t)t * k + n];
            sum = sum + s * (m_vals[p] - nb_means[code]);
            denom = denom + s;
        }
    }
    if (sum == 0.0) {
        pred[r] = row_base[r];
        status[r] = QREC_KNN_FALLBACK;
    } else if (denom == 0.0) {
        pred[r] = 0.0;
        status[r] = QREC_KNN_ZERO_DIVISION;
    } else {
        pred[r] = row_base[r] + sum / denom;
        status[r] = QREC_KNN_COMPUTED;
    }
}

__global__ __launch_bounds__(kThreads) void slopeone_predict_kernel(int64_t n_rows, const int32_t *__restrict__ row_query,
                                                                    const int32_t *__restrict__ row_user, const double *__restrict__ row_base,
                                                                    int64_t q0, int64_t nq, const double *__restrict__ dev,
                                                                    const int32_t *__restrict__ freq, int64_t n_items,
                                                                    int64_t n_users, const int64_t *__restrict__ u_indptr,
                                                                    const int32_t *__restrict__ u_items, const double *__restrict__ u_vals,
                                                                    double *__restrict__ pred, int32_t *__restrict__ status) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t t = row_query[r];
    if (t < q0 || t >= q0 + nq) return;
    const int32_t u = row_user[r];
    if (u < 0 || u >= n_users) {
        pred[r] = row_base[r];
        status[r] = QREC_KNN_FALLBACK;
        return;
    }
    const double *d = dev + (t - q0) * n_items;
    const int32_t *f = freq + (t - q0) * n_items;
    double sum = 0.0;
    int64_t fs = 0;
    for (int64_t p = u_indptr[u]; p < u_indptr[u + 1]; ++p) {
        const int32_t j = u_items[p];
        if (j < 0 || j >= n_items) continue;
        const int32_t c = f[j];
        sum = sum + (u_vals[p] + d[j]) * (double)c;
        fs += c;
    }
    if (fs == 0) {
        pred[r] = row_base[r];
        status[r] = QREC_KNN_FALLBACK;
    } else {
        pred[r] = sum / (double)fs;
        status[r] = QREC_KNN_COMPUTED;
    }
}

// the two workspaces; neither is stated smaller than 256 bytes
double *topk_layout(Carver &c, int64_t n_queries, int64_t m) {       // [m][n_queries], the similarity block transposed
    double *BT = c.take<double>((size_t)(n_queries * m));
    c.off = std::max<size_t>(c.off, 256);
    return BT;
}
struct SlopeWs { double *dev; int32_t *freq; };                      // [batch][n_items] each
SlopeWs slope_layout(Carver &c, int64_t batch, int64_t n_items) {
    const SlopeWs w = {c.take<double>((size_t)(batch * n_items)), c.take<int32_t>((size_t)(batch * n_items))};
    c.off = std::max<size_t>(c.off, 256);
    return w;
}

}  // namespace

extern "C" int qrec_knn_sweep(int32_t measure, int64_t n_queries, const int64_t *d_q_indptr, const int32_t *d_q_keys,
                              const double *d_q_vals, const double *d_q_means, const double *d_q_sq, int64_t n_keys,
                              const int64_t *d_c_indptr, const int32_t *d_c_labels, const double *d_c_vals, const double *d_c_sq,
                              int64_t n_cands, const double *d_c_means,
                              double *d_out, int64_t ld_out, int32_t *d_count_out, int64_t ld_count, void *stream) {
    QREC_REQUIRE(measure >= QREC_KNN_PCC && measure <= QREC_KNN_SLOPEONE, "qrec_knn_sweep: unknown measure %d", measure);
    QREC_REQUIRE(n_queries >= 0 && n_cands >= 0 && n_keys >= 0 && n_cands <= INT_MAX, "qrec_knn_sweep: bad sizes");
    QREC_REQUIRE(ld_out >= n_cands, "qrec_knn_sweep: ld_out %lld < n_cands %lld", (long long)ld_out, (long long)n_cands);
    QREC_REQUIRE(measure != QREC_KNN_PCC || (d_q_means && d_c_means), "qrec_knn_sweep: pcc needs both mean arrays");
    QREC_REQUIRE(measure == QREC_KNN_SLOPEONE || (d_q_sq && d_c_sq), "qrec_knn_sweep: the measure needs both square arrays");
    QREC_REQUIRE(measure != QREC_KNN_SLOPEONE || (d_count_out && ld_count >= n_cands), "qrec_knn_sweep: SlopeOne needs d_count_out");
    if (n_queries == 0 || n_cands == 0) return QREC_OK;
    const int64_t n_tiles = (n_cands + kTile - 1) / kTile;
    QREC_REQUIRE(n_queries * n_tiles <= INT_MAX, "qrec_knn_sweep: too many (query, tile) pairs in one call");
    hipStream_t st = as_stream(stream);
    const unsigned grid = (unsigned)(n_queries * n_tiles);
#define QREC_KNN_SWEEP(M)                                                                                                   \
    knn_sweep_kernel<M><<<grid, kThreads, 0, st>>>(n_tiles, d_q_indptr, d_q_keys, d_q_vals, d_q_means, d_q_sq, n_keys, d_c_indptr, \
                                                   d_c_labels, d_c_vals, d_c_sq, n_cands, d_c_means, d_out, ld_out, d_count_out,   \
                                                   ld_count)
    switch (measure) {
        case QREC_KNN_PCC: QREC_KNN_SWEEP(QREC_KNN_PCC); break;
        case QREC_KNN_COS: QREC_KNN_SWEEP(QREC_KNN_COS); break;
        case QREC_KNN_EUCLIDEAN: QREC_KNN_SWEEP(QREC_KNN_EUCLIDEAN); break;
        default: QREC_KNN_SWEEP(QREC_KNN_SLOPEONE); break;
    }
#undef QREC_KNN_SWEEP
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

extern "C" int qrec_knn_topk_workspace_bytes(int64_t n_queries, int64_t m, int64_t *bytes) {
    QREC_REQUIRE(n_queries >= 0 && m >= 0 && bytes, "qrec_knn_topk_workspace_bytes: bad arguments");
    *bytes = layout_bytes(topk_layout, n_queries, m);
    return QREC_OK;
}

extern "C" int qrec_knn_topk(int64_t n_queries, const double *d_S, int64_t ld_S, int64_t m, const int32_t *d_q_label,
                             const int32_t *d_test_code, const int32_t *d_lab2id, int64_t n_cands, int32_t k, int32_t *d_ids,
                             double *d_vals, int32_t *d_counts, void *d_ws, int64_t ws_bytes, void *stream) {
    if (k > kMaxK) {
        set_error("qrec_knn_topk: k = %d is above the supported maximum %d", k, kMaxK);
        return QREC_ERR_UNSUPPORTED;
    }
    QREC_REQUIRE(k >= 1, "qrec_knn_topk: k = %d", k);
    QREC_REQUIRE(n_queries >= 0 && m >= 0 && m <= n_cands && ld_S >= n_cands, "qrec_knn_topk: bad sizes");
    QREC_REQUIRE(n_queries + n_cands < (int64_t)UINT_MAX, "qrec_knn_topk: sequence positions need 32 bits");
    Carver c(d_ws);
    double *BT = topk_layout(c, n_queries, m);
    const int64_t need = (int64_t)c.bytes();
    QREC_REQUIRE(ws_bytes >= need && d_ws, "qrec_knn_topk: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    if (n_queries == 0) return QREC_OK;
    QREC_REQUIRE(n_queries <= INT_MAX, "qrec_knn_topk: too many queries");
    hipStream_t st = as_stream(stream);
    if (m > 0) {
        dim3 g((unsigned)((m + 31) / 32), (unsigned)((n_queries + 31) / 32));
        QREC_REQUIRE(g.y <= 65535, "qrec_knn_topk: too many queries for the transpose grid");
        knn_transpose_kernel<<<g, kThreads, 0, st>>>(d_S, n_queries, ld_S, m, BT);
        QREC_LAUNCH_CHECK();
    }
    knn_topk_kernel<<<(unsigned)n_queries, kThreads, 0, st>>>(n_queries, d_S, ld_S, BT, d_q_label, d_test_code, d_lab2id, n_cands, k,
                                                             d_ids, d_vals, d_counts);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

extern "C" int qrec_knn_predict(int32_t mode, int64_t n_rows, const int32_t *d_row_query, const int32_t *d_row_other,
                                const double *d_row_base, const int32_t *d_nb_ids, const double *d_nb_vals, const int32_t *d_nb_counts,
                                int64_t n_queries, int32_t k, int64_t n_members, const int64_t *d_m_indptr, const int32_t *d_m_keys,
                                const double *d_m_vals, int64_t n_nb, const double *d_nb_means, double *d_pred, int32_t *d_status,
                                void *stream) {
    QREC_REQUIRE(mode == 0 || mode == 1, "qrec_knn_predict: mode %d", mode);
    QREC_REQUIRE(n_rows >= 0 && k >= 1 && k <= kMaxK && n_members >= 0 && n_nb >= 0, "qrec_knn_predict: bad sizes");
    if (n_rows == 0) return QREC_OK;
    knn_predict_kernel<<<(unsigned)((n_rows + kThreads - 1) / kThreads), kThreads, 0, as_stream(stream)>>>(
        mode, n_rows, d_row_query, d_row_other, d_row_base, d_nb_ids, d_nb_vals, d_nb_counts, n_queries, k, n_members, d_m_indptr,
        d_m_keys, d_m_vals, n_nb, d_nb_means, d_pred, d_status);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

extern "C" int qrec_slopeone_workspace_bytes(int64_t batch, int64_t n_items, int64_t *bytes) {
    QREC_REQUIRE(batch >= 0 && n_items >= 0 && bytes, "qrec_slopeone_workspace_bytes: bad arguments");
    *bytes = layout_bytes(slope_layout, batch, n_items);
    return QREC_OK;
}

extern "C" int qrec_slopeone_batch(int64_t q0, int64_t nq, const int64_t *d_q_indptr, const int32_t *d_q_keys, const double *d_q_vals,
                                   int64_t n_users, const int64_t *d_u_indptr_sorted, const int32_t *d_u_items_sorted,
                                   const double *d_u_vals_sorted, int64_t n_items, int64_t n_rows, const int32_t *d_row_query,
                                   const int32_t *d_row_user, const double *d_row_base, const int64_t *d_u_indptr,
                                   const int32_t *d_u_items, const double *d_u_vals, double *d_pred, int32_t *d_status, void *d_ws,
                                   int64_t ws_bytes, void *stream) {
    QREC_REQUIRE(q0 >= 0 && nq >= 0 && n_users >= 0 && n_items >= 0 && n_rows >= 0, "qrec_slopeone_batch: bad sizes");
    Carver c(d_ws);
    const SlopeWs w = slope_layout(c, nq, n_items);
    const int64_t need = (int64_t)c.bytes();
    QREC_REQUIRE(ws_bytes >= need && d_ws, "qrec_slopeone_batch: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    if (nq == 0) return QREC_OK;
    int rc = qrec_knn_sweep(QREC_KNN_SLOPEONE, nq, d_q_indptr + q0, d_q_keys, d_q_vals, nullptr, nullptr, n_users, d_u_indptr_sorted,
                            d_u_items_sorted, d_u_vals_sorted, nullptr, n_items, nullptr, w.dev, n_items, w.freq, n_items, stream);
    if (rc != QREC_OK) return rc;
    if (n_rows == 0) return QREC_OK;
    slopeone_predict_kernel<<<(unsigned)((n_rows + kThreads - 1) / kThreads), kThreads, 0, as_stream(stream)>>>(
        n_rows, d_row_query, d_row_user, d_row_base, q0, nq, w.dev, w.freq, n_items, n_users, d_u_indptr, d_u_items, d_u_vals, d_pred,
        d_status);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}
