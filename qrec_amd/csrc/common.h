// Shared helpers for libqrec_hip.so (gfx950 only; no other target is supported).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "../../include/qrec_hip.h"

namespace qrec {

void set_error(const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

#define QREC_HIP_CHECK(expr)                                                             \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            ::qrec::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),     \
                              __FILE__, __LINE__);                                       \
            return QREC_ERR_HIP;                                                         \
        }                                                                                \
    } while (0)

#define QREC_REQUIRE(cond, ...)                 \
    do {                                        \
        if (!(cond)) {                          \
            ::qrec::set_error(__VA_ARGS__);     \
            return QREC_ERR_INVALID;            \
        }                                       \
    } while (0)

#define QREC_LAUNCH_CHECK() QREC_HIP_CHECK(hipGetLastError())

constexpr int kWave = 64;  // gfx950 wavefront

// a runtime value -> a template argument, stated once per ladder: `with_x(value, [&](auto c) { kernel<c()> ... })`
// (with_nc of eval_fused.hip, with_epl of lane_row.h)
template <int V> using int_c = std::integral_constant<int, V>;

// ---- workspaces: a file states each layout ONCE, as a function (Carver &, shape...) that returns or fills the file's Ws
// struct.  layout_bytes runs it on a null base for the *_bytes entry point, carve on the caller's buffer; an entry point that
// is told the buffer's size runs it on a Carver of its own and checks the size against bytes() of that same walk.
// Where a layout is a braced list of take() calls, the list is evaluated left to right: the arrays lie in the order of the fields.
__host__ __device__ constexpr size_t align_up(size_t b, size_t a) { return (b + a - 1) & ~(a - 1); }   // a: a power of two
struct Carver {
    char *base; size_t off = 0;
    __host__ __device__ explicit Carver(void *ws) : base(static_cast<char *>(ws)) {}
    // the next `count` elements of T, starting at the next multiple of `align` bytes; null on a null base
    template <typename T>
    __host__ __device__ T *take(size_t count, size_t align = alignof(T)) {
        pad(align);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    __host__ __device__ void pad(size_t align) { off = align_up(off, align); }   // also: a layout that ends on a padded array
    __host__ __device__ size_t bytes() const { return off; }
};
template <typename F, typename... A>
int64_t layout_bytes(F layout, A... a) { Carver c(nullptr); layout(c, a...); return (int64_t)c.bytes(); }
template <typename F, typename... A>
auto carve(void *ws, F layout, A... a) { Carver c(ws); return layout(c, a...); }

// ---- ordered scatter-add (ordered.hip): the deterministic counterpart of the float-atomic gradient scatters.  A producer
// writes slot s's row to contrib[s][ld] and its destination row to keys[s] (< 0: none); ordered_scatter_run sorts (key, slot)
// stably and adds each row's slots in ascending slot order, class by class (class = slot / class_size; 0: one class).
struct OrderedScatterWs {
    float *contrib; int32_t *keys, *keys_sorted, *slots_sorted; void *temp; size_t temp_bytes;
};
int ordered_ws_bytes(int64_t n_slots, int ld, int64_t *bytes);
int ordered_ws_carve(void *ws, int64_t ws_bytes, int64_t n_slots, int ld, OrderedScatterWs *w);
int ordered_scatter_run(const OrderedScatterWs &w, int64_t n_slots, int ld, int64_t class_size, float *out, hipStream_t st);

// S = sigmoid(S + bias[item]) over the evaluation's transposed [n_items][b_pad] fp32 score block (autoencoder.hip; the pass
// qrec_score_topk_sigmoid_bias runs between scoring and masking)
int score_block_sigmoid_bias(float *S_T, const float *bias, int n_items, int b_pad, hipStream_t st);

// S[item][b] = sum over the rated items i of user_ids[b], in CSR order, of vals * W[i][item]: the fill pass of
// qrec_score_topk_sparse_row_sigmoid_bias (cfgan.hip), in the place of the MFMA scoring of the block route
struct SparseRows { const float *W; int ld; const int64_t *indptr; const int32_t *items; const float *vals; };
int score_block_sparse_rows(float *S_T, const SparseRows &r, int n_items, const int32_t *user_ids, int n_b, int b_pad, hipStream_t st);

// S[item][b] = the ranking score of one of the QREC_RATING_* forms for user user_ids[b]: the fill pass of qrec_score_topk_form
// (rank_forms.hip), fp64, in the place of the plain MFMA scoring of the block route.  It stages the users' operand rows, their
// norms and biases in `ws` (form_operand_bytes), then runs the block route's own tile loop (eval_tile.h) with the form's epilogue.
// item_op: the item-side operand [n_items][ld] (Q, or Q.H of qrec_rank_form_prepare), item_norm: its squared row norms (distance forms).
struct FormScore {
    int form; double sign, mu, alpha;
    const double *P, *item_op, *item_norm; int d, ld, n_users;
    const double *Bu, *Bi, *Y; const int64_t *y_indptr; const int32_t *y_items;
    const double *H;
    const int64_t *fe_indptr; const int32_t *fe_ids; const double *fe_w, *fe_den;
    void *ws;
};
int64_t form_operand_bytes(int n_b, int ld);
int score_block_form(double *S_T, const FormScore &f, int n_items, const int32_t *user_ids, int n_b, int b_pad, hipStream_t st);

// ---- what crosses between the evaluation's translation units: eval_topk.hip (entry points, dispatch) calls the two routes, the
// fused route's stage (D) calls two launches of the block route.  Kernels stay private to their files.
// eval_block.hip: score block -> mask -> heap top-N (fp32 and fp64).  item_bias: qrec_score_topk_sigmoid_bias; sparse:
// qrec_score_topk_sparse_row_sigmoid_bias (then U, V are unused); both fp32 only.  form: qrec_score_topk_form (U, V unused), fp64 only
int64_t block_path_bytes(int dtype, int n_items, int n_b);
int run_score_topk(int dtype, const void *U, const void *V, int ld, int n_items, const int32_t *user_ids, int n_b,
                   const int64_t *rated_indptr, const int32_t *rated_items, int K, void *scratch, int32_t *ids_out, void *scores_out,
                   hipStream_t st, const float *item_bias = nullptr, const SparseRows *sparse = nullptr, const FormScore *form = nullptr);
// users per wavefront (UTILE) x item tiles per wavefront of a scoring launch (eval_block.hip)
dim3 score_grid(int n_b, int n_item_tiles, int UTILE, int min_per_wave, int *per_wave);
// Where the fp32 score of (item, user b of the batch) goes: S[item * b_pad + (b / 64) * upair_stride + (b % 64) * u_stride].
struct ScoreLayout { int b_pad; int64_t upair_stride, u_stride; };
// the block route's transposed block [rows][b_pad]: what its lane-per-user scans read coalesced
inline ScoreLayout plain_block(int b_pad) { return {b_pad, 64, 1}; }
// user-major rows [user][row_len], a user's scores contiguous: what the exact per-user walk of a handful of flagged users wants
inline ScoreLayout user_major_rows(int64_t row_len) { return {1, 64 * row_len, row_len}; }
// S = V U[user_ids]^T by score_kernel_f32, every wavefront streaming at least min_tiles_per_wave item tiles (fewer users: shorter
// wavefronts); the users' rated items -> 0 by mask_kernel<float>
int launch_score_block_f32(const float *U, const float *V, int ld, int n_items, const int32_t *user_ids, int n_b, int min_tiles_per_wave,
                           float *S, ScoreLayout lay, hipStream_t st);
int launch_mask_block(const int32_t *user_ids, int n_b, const int64_t *rated_indptr, const int32_t *rated_items, float *S, ScoreLayout lay,
                      hipStream_t st);
// eval_fused.hip: threshold -> filter -> select, no B x I block (fp32, ld <= 128)
bool fused_ok(int dtype, int ld, int n_items, int K);      // one predicate for the scratch-size query and the launch
int64_t fused_path_bytes(int n_items, int n_b, int ld);
int run_fused_topk_f32(const float *U, const float *V, int ld, int n_items, const int32_t *user_ids, int n_b, const int64_t *rated_indptr,
                       const int32_t *rated_sorted, int K, void *scratch, int32_t *ids_out, float *scores_out, hipStream_t st);

// ---- buffer resources: the only way to get 16-byte loads/stores with an explicit cache
// policy (sc1 = bypass the non-coherent per-XCD caches) and compiler-tracked waitcnts.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAuxPlain = 0;
constexpr int kAuxSc1 = 16;  // gfx940+ cache-policy bit 4 = sc1

__device__ inline __amdgpu_buffer_rsrc_t make_rsrc(const void *base, uint32_t bytes) {
    // raw buffer, no swizzle, bounds-checked against `bytes`
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}

template <int AUX>
__device__ inline f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
    u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, AUX);
    return __builtin_bit_cast(f32x4, v);
}
template <int AUX>
__device__ inline void buf_store4(__amdgpu_buffer_rsrc_t r, uint32_t byte_off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)byte_off, 0, AUX);
}

// Sum across the lanes of one row of WIDTH (power of two <= 64) consecutive lanes; every
// lane of the row receives the total.  xor-butterfly: the compiler lowers the small
// strides to DPP and the rest to ds_bpermute/permlane.
template <int WIDTH, typename T>
__device__ inline T row_allreduce_sum(T v) {
#pragma unroll
    for (int m = WIDTH / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// Sum over the 64 lanes of a wavefront, every lane receives it.  DPP adds inside the 16-lane rows (row_shr 1,2,3 of the
// input, then row_shr 4 and 8 of the running sum), row_bcast 15 / 31 across the rows, total read from lane 63: six
// VALU-rate steps.  The xor butterfly this replaces goes through ds_bpermute -- the LDS crossbar, >100 clocks per step and
// two of them per fp64 value: a third of the order-exact kernels' per-triplet chain (measured).
// A fixed summation tree, so the result is deterministic; it is NOT the butterfly's tree (last-bit differences).
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ inline float dpp_take(float v) {      // lanes without a source (bounds, masks) receive 0
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, BANK_MASK, true));
}
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ inline double dpp_take(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, BANK_MASK, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROW_MASK, BANK_MASK, true);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ inline float read_lane63(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63)); }
__device__ inline double read_lane63(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 63);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <typename T>
__device__ inline T wave_sum_dpp(T v) {
    T t = v + dpp_take<0x111, 0xf, 0xf>(v);          // row_shr:1
    t = t + dpp_take<0x112, 0xf, 0xf>(v);            // row_shr:2
    t = t + dpp_take<0x113, 0xf, 0xf>(v);            // row_shr:3   -> lanes 3, 7, 11, 15 of a row hold their quad's sum
    t = t + dpp_take<0x114, 0xf, 0xe>(t);            // row_shr:4, banks 1-3
    t = t + dpp_take<0x118, 0xf, 0xc>(t);            // row_shr:8, banks 2-3 -> lane 15 of a row holds the row's sum
    t = t + dpp_take<0x142, 0xa, 0xf>(t);            // row_bcast:15 into rows 1 and 3
    t = t + dpp_take<0x143, 0xc, 0xf>(t);            // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
    return read_lane63(t);
}

// ---- device helpers more than one kernel file needs; each exists once, here
// Philox4x32-10 (Salmon et al., SC'11): c = the four counter words in and the four random words out, (k0, k1) the key.  Every
// device stream of the library is this function of a counter and key its caller builds; oracle/c.py::philox4x32_10 and
// tests/device_stream.py restate it bit for bit.
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0], hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// the uniform in [0, 1) of a random word's top 24 bits: exact in fp32
__device__ inline float uniform24(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

__device__ inline float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// Sum of a double over the workgroup (any size; lds holds blockDim.x doubles) in one fixed tree, so the bits do not depend on
// the launch.  Every thread calls it, every thread receives the total, and back-to-back calls on one lds array are safe: the
// leading barrier keeps a call from overwriting lds[0] while a thread still reads the previous call's total from it.
__device__ inline double block_sum_fixed(double v, double *lds) {
    const int t = threadIdx.x, n = (int)blockDim.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    int top = 1;
    while (top < n) top <<= 1;                        // blockDim need not be a power of two
    for (int s = top >> 1; s >= 1; s >>= 1) {
        if (t < s && t + s < n) lds[t] += lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

// Fixed-point table elements of the BPR throughput epoch (QREC_HW_FIXED: bpr_sgd.hip, reduce.hip): int32 = rint(x * 2^26) while an
// epoch's launches run, fp32 at rest.  Range +-32, quantum 2^-26; |x| >= kFixLimit (half the range: headroom for deltas in flight) or
// a NaN fails the run.  The float is clamped before it is converted (one v_med3_f32; a NaN comes out as the lower bound), so the
// conversion itself is defined for every input and saturates: a table element out of range at convert-in never wraps.  A DELTA is
// converted the same way but added in two's complement: an element can only be carried past +-32 by a step that produced |new| >= 16
// first, which raises FAILED -- such an element may wrap in memory, never silently.
// QREC_DRV_FAILED = kFailedFixed: "failed while the tables hold integers" -- raised by the epoch's own launches only, and turned into
// 1 by the epoch close once it has written the tables back as fp32.
constexpr float kFixScale = 67108864.f, kFixInv = 1.f / 67108864.f, kFixLimit = 16.f;
constexpr double kFailedFixed = 2.0;
__device__ inline int32_t fx_from_float(float x) { return __float2int_rn(__builtin_amdgcn_fmed3f(x * kFixScale, -2147483648.f, 2147483520.f)); }
__device__ inline float fx_to_float(int32_t q) { return (float)q * kFixInv; }
__device__ inline bool fx_out_of_range(float x) { return !(fabsf(x) < kFixLimit); }      // true for a NaN as well
// The same predicate over many values with ONE test at the end: keep the running unsigned maximum of the magnitude bits.  Non-negative
// floats order as their bit patterns do, and +inf (0x7f800000) and every NaN (above it) have larger magnitude bits than any finite
// value, so  max_k fx_mag_bits(x_k) >= bits(16.0f)  <=>  some x_k has !(|x_k| < 16): the flag is raised in exactly the same runs.  (A
// float maximum with abs modifiers would not do: v_max3_f32 drops NaNs.)  Per value: one v_and_b32 and a third of a v_max3_u32.
constexpr uint32_t kFixLimitBits = 0x41800000u;      // 16.0f
__device__ inline uint32_t fx_mag_bits(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7fffffffu; }
__device__ inline bool fx_mag_out_of_range(uint32_t mag) { return mag >= kFixLimitBits; }

// index of item in the ascending row[0, len), or -1
template <typename Len>
__device__ inline Len sorted_find(const int32_t *__restrict__ row, Len len, int item) {
    Len lo = 0, hi = len;
    while (lo < hi) {
        const Len mid = (lo + hi) >> 1;
        if (row[mid] < item) lo = mid + 1; else hi = mid;
    }
    return lo < len && row[lo] == item ? lo : -1;
}

}  // namespace qrec
