// CFGAN (model/ranking/CFGAN.py): a one-layer generator r^ = sigmoid(C G_W1 + b) over the whole item table, a one-layer
// discriminator over [r^ * mask | C], Adam on both.  G_W1 is n_items x n_items; the reference forms C @ G_W1 densely and TF's
// Adam makes ten element-wise passes over it.  Everything that multiplies by an exact zero is dropped here: the forward pass is
// evaluated at the mask positions only, the gradient of G_W1 is non-zero only on (rated item of a batch row) x (mask position of
// that row), and what remains is ONE streaming read-modify-write of W, m, v with the sparse gradient injected on the fly
// (sweep_kernel: 24 bytes per entry, memory-bound).  fp32, fp64 for the loss sums.  No float atomic: every sum has one fixed
// order (list order inside a batch row, ascending batch row inside an item), so two launches give the same bits.
//
// The batch comes as CDAE's lists (include/qrec_hip.h) with everything kept: "in" = the rated entries of the batch rows, "live" =
// the mask positions, lv_label = 1 where the position is in N_zr as well.  Tables [n_items][ld], ld a multiple of 32, columns
// [n_items, ld) zero and kept zero (their gradient, m and v are zero, so Adam leaves them).  The discriminator's 2 n_items + 1
// values lie in one array: D_W1 flat, then D_b1.
#include "common.h"

namespace {

using namespace qrec;

constexpr int kChunk = QREC_CFGAN_CHUNK;             // columns of one sweep tile: 256 threads x one 16-byte access
constexpr float kGuard = 10e-5f;                     // CFGAN.py:106-107
static_assert(kChunk == 1024, "sweep_kernel: one f32x4 per thread of a 256-thread workgroup");

// workspace layout (qrec_cfgan_workspace_bytes): the doubles first
struct Ws {
    double *terms;     // [3][B]  log(D_real + e) + log(1 - D_fake + e),  log(1 - D_fake + e),  sum of r^2 over N_zr and mask
    float *a_r, *a_f;  // [B]     d D_loss / d (real logit), d D_loss / d (fake logit)
    float *rhat;       // [n_live]
    float *delta;      // [n_live] d G_loss / d z at the slot
};
__host__ __device__ inline Ws ws_layout(Carver &c, int B, int64_t n_live) {
    return {c.take<double>(3 * (size_t)B), c.take<float>((size_t)B), c.take<float>((size_t)B), c.take<float>((size_t)n_live),
            c.take<float>((size_t)n_live)};
}

struct AdamArgs { float alpha, b1, b2, eps; };

// training_ops.cc ApplyAdam, the arithmetic of qrec_adam_step
template <typename T>
__device__ inline void adam_update(T &theta, T &m, T &v, T g, const AdamArgs &a) {
#pragma clang fp contract(off)
    m = m + (g - m) * (1.0f - a.b1);
    v = v + (g * g - v) * (1.0f - a.b2);
    if constexpr (sizeof(T) == sizeof(float)) {
        theta -= (m * a.alpha) / (sqrtf(v) + a.eps);
    } else {
        theta.x -= (m.x * a.alpha) / (sqrtf(v.x) + a.eps); theta.y -= (m.y * a.alpha) / (sqrtf(v.y) + a.eps);
        theta.z -= (m.z * a.alpha) / (sqrtf(v.z) + a.eps); theta.w -= (m.w * a.alpha) / (sqrtf(v.w) + a.eps);
    }
}

// ---- sampled forward + discriminator: one workgroup per batch row ------------------------------------------------------
// r^ at the row's live slots (the sum over its rated items in list order = ascending item id), the two discriminator logits
// (fp64 partial sums in one fixed tree), a_r, a_f, the row's loss terms, then delta at the live slots.
__global__ __launch_bounds__(256) void row_kernel(const float *__restrict__ W, const float *__restrict__ bias, const float *__restrict__ thetaD,
                                                  int n_items, int ld, int B, int64_t n_in, int64_t n_live, const int32_t *__restrict__ in_ptr,
                                                  const int32_t *__restrict__ in_item, const float *__restrict__ in_val,
                                                  const int32_t *__restrict__ lv_ptr, const int32_t *__restrict__ lv_item,
                                                  const int32_t *__restrict__ lv_flag, float alpha, float inv_B, Ws w) {
    __shared__ double red[256];
    const int n = blockIdx.x, t = threadIdx.x;
    const float *Dw = thetaD;
    const float Db = thetaD[2 * (size_t)n_items];
    int64_t ib = in_ptr[n], ie = in_ptr[n + 1], lb = lv_ptr[n], le = lv_ptr[n + 1];
    ib = ib < 0 ? 0 : ib; lb = lb < 0 ? 0 : lb;
    ie = ie < n_in ? ie : n_in; le = le < n_live ? le : n_live;
    double p_fake = 0.0, p_zr = 0.0, p_lo = 0.0, p_hi = 0.0;
    for (int64_t s = lb + t; s < le; s += 256) {
        const int j = lv_item[s];
        const bool ok = (unsigned)j < (unsigned)n_items;
        float z = 0.0f;
        int64_t e = ib;
        for (; e + 4 <= ie; e += 4) {        // four independent reads in flight, added in list order
            int it[4]; float x[4], wv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { it[q] = in_item[e + q]; x[q] = in_val[e + q]; }
#pragma unroll
            for (int q = 0; q < 4; q++) wv[q] = ok && (unsigned)it[q] < (unsigned)n_items ? W[(size_t)it[q] * ld + j] : 0.0f;
#pragma unroll
            for (int q = 0; q < 4; q++) z += x[q] * wv[q];
        }
        for (; e < ie; e++) {
            const int it = in_item[e];
            if (ok && (unsigned)it < (unsigned)n_items) z += in_val[e] * W[(size_t)it * ld + j];
        }
        const float r = ok ? sigmoidf(z + bias[j]) : 0.0f;
        w.rhat[s] = r;
        if (ok) p_fake += (double)(r * Dw[j]);
        if (lv_flag[s]) p_zr += (double)r * (double)r;
    }
    for (int64_t e = ib + t; e < ie; e += 256) {
        const int it = in_item[e];
        if ((unsigned)it >= (unsigned)n_items) continue;
        const float x = in_val[e];
        p_lo += (double)(x * Dw[it]);
        p_hi += (double)(x * Dw[(size_t)n_items + it]);
    }
    const double s_fake = block_sum_fixed(p_fake, red), s_zr = block_sum_fixed(p_zr, red);
    const double s_lo = block_sum_fixed(p_lo, red), s_hi = block_sum_fixed(p_hi, red);
    const float logit_r = (float)(s_lo + s_hi) + Db, logit_f = (float)(s_fake + s_hi) + Db;
    // 1 - sigmoid(x) as sigmoid(-x): past |x| = 17 the subtraction would give an exact 0 and lose the gradient's last digits
    const float Dr = sigmoidf(logit_r), oDr = sigmoidf(-logit_r), Df = sigmoidf(logit_f), oDf = sigmoidf(-logit_f);
    const float a_r = -inv_B * (Dr * oDr / (Dr + kGuard)), a_f = inv_B * (Df * oDf / (oDf + kGuard));
    if (t == 0) {
        w.a_r[n] = a_r; w.a_f[n] = a_f;
        w.terms[n] = (double)logf(Dr + kGuard) + (double)logf(oDf + kGuard);
        w.terms[(size_t)B + n] = (double)logf(oDf + kGuard);
        w.terms[2 * (size_t)B + n] = s_zr;
    }
    for (int64_t s = lb + t; s < le; s += 256) {         // the slots this thread wrote above
        const int j = lv_item[s];
        const float r = w.rhat[s];
        const float up = (unsigned)j < (unsigned)n_items ? -a_f * Dw[j] + (lv_flag[s] ? alpha * r : 0.0f) : 0.0f;
        w.delta[s] = up * (r * (1.0f - r));              // r (1 - r) as the reference forms it: an exact 0 once r rounds to 1
    }
}

// D_loss = -mean(log(D_real + e) + log(1 - D_fake + e));  G_loss = mean log(1 - D_fake + e) + alpha/2 sum (N_zr r^ mask)^2
__global__ __launch_bounds__(256) void loss_kernel(const double *__restrict__ terms, int B, double alpha, double *__restrict__ out) {
    __shared__ double red[256];
    double d = 0.0, g = 0.0, zr = 0.0;
    for (int k = threadIdx.x; k < B; k += 256) { d += terms[k]; g += terms[(size_t)B + k]; zr += terms[2 * (size_t)B + k]; }
    d = block_sum_fixed(d, red); g = block_sum_fixed(g, red); zr = block_sum_fixed(zr, red);
    if (threadIdx.x == 0) { out[0] = -d / (double)B; out[1] = g / (double)B + alpha * 0.5 * zr; }
}

// ---- discriminator step: one thread per value, the item-major sums in ascending batch row, Adam in the same pass --------
// g D_W1[j] = sum a_r C[n,j] + sum a_f r^[n,j] (mask positions);  g D_W1[ni + j] = sum a_r C[n,j] + sum a_f C[n,j];
// g D_b1 = sum a_r + sum a_f -- the real pass's sum and the fake pass's sum formed apart and added, as TF adds the two gradients.
__global__ __launch_bounds__(256) void dis_step_kernel(float *__restrict__ thetaD, float *__restrict__ mD, float *__restrict__ vD, int n_items,
                                                       int B, int64_t n_in, int64_t n_live, const int32_t *__restrict__ in_cptr,
                                                       const int32_t *__restrict__ in_crow, const float *__restrict__ in_cval,
                                                       const int32_t *__restrict__ lv_cptr, const int32_t *__restrict__ lv_crow,
                                                       const int32_t *__restrict__ lv_cslot, Ws w, AdamArgs adam, float *__restrict__ g_out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > 2 * (int64_t)n_items) return;
    float real = 0.0f, fake = 0.0f;
    if (k == 2 * (int64_t)n_items) {
        for (int n = 0; n < B; n++) { real += w.a_r[n]; fake += w.a_f[n]; }
    } else {
        const int j = (int)(k < n_items ? k : k - n_items);
        int64_t eb = in_cptr[j], ee = in_cptr[j + 1];
        ee = ee < n_in ? ee : n_in;
        for (int64_t e = eb < 0 ? 0 : eb; e < ee; e++) {
            const int n = in_crow[e];
            if ((unsigned)n >= (unsigned)B) continue;
            real += w.a_r[n] * in_cval[e];
            if (k >= n_items) fake += w.a_f[n] * in_cval[e];
        }
        if (k < n_items) {
            eb = lv_cptr[j]; ee = lv_cptr[j + 1];
            ee = ee < n_live ? ee : n_live;
            for (int64_t e = eb < 0 ? 0 : eb; e < ee; e++) {
                const int n = lv_crow[e], s = lv_cslot[e];
                if ((unsigned)n >= (unsigned)B || (uint64_t)(int64_t)s >= (uint64_t)n_live) continue;
                fake += w.a_f[n] * w.rhat[s];
            }
        }
    }
    const float g = real + fake;
    float th = thetaD[k], m = mD[k], v = vD[k];
    adam_update(th, m, v, g, adam);
    thetaD[k] = th; mD[k] = m; vD[k] = v;
    if (g_out) g_out[k] = g;
}

// ---- generator sweep: W, m, v read once and written once, the sparse gradient staged per tile in LDS ---------------------
// A tile is (row i, kChunk columns).  Rows [0, n_items) are G_W1's: the batch rows that rated i (item-major "in" list, ascending
// batch row) each add C[n,i] delta[n,j] at their live slots inside the tile -- slots of one batch row have distinct columns, a
// barrier separates the batch rows, so every column has one fixed order of additions.  A row no batch user rated stages nothing
// and still takes the Adam update: momentum from earlier steps moves it.  Row n_items is the bias: g b[j] = sum of delta over
// the item-major live list of j.  A capped grid (256 CUs x 8 workgroups) walks the tiles by stride; every access of the
// three tables is 16 bytes per lane, 4 KiB of LDS per workgroup leave the occupancy to the 32 waves per CU.
__global__ __launch_bounds__(256) void sweep_kernel(float *__restrict__ W, float *__restrict__ mW, float *__restrict__ vW, float *__restrict__ bias,
                                                    float *__restrict__ mb, float *__restrict__ vb, int n_items, int ld, int B, int64_t n_in,
                                                    int64_t n_live, const int32_t *__restrict__ in_cptr, const int32_t *__restrict__ in_crow,
                                                    const float *__restrict__ in_cval, const int32_t *__restrict__ lv_ptr,
                                                    const int32_t *__restrict__ lv_item, const int32_t *__restrict__ lv_cptr,
                                                    const int32_t *__restrict__ lv_cslot, const float *__restrict__ delta, AdamArgs adam,
                                                    float *__restrict__ gW_out, float *__restrict__ gb_out) {
    __shared__ __attribute__((aligned(16))) float g_lds[kChunk];
    const int t = threadIdx.x;
    const int n_chunks = (ld + kChunk - 1) / kChunk;
    const int64_t n_tiles = ((int64_t)n_items + 1) * n_chunks;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int row = (int)(tile / n_chunks), c0 = (int)(tile % n_chunks) * kChunk, c = c0 + 4 * t;
        f32x4 g = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row < n_items) {
            int64_t eb = in_cptr[row], ee = in_cptr[row + 1];
            eb = eb < 0 ? 0 : eb; ee = ee < n_in ? ee : n_in;
            if (eb < ee) {                                   // the same for the whole workgroup
                *reinterpret_cast<f32x4 *>(&g_lds[4 * t]) = g;
                __syncthreads();
                for (int64_t e = eb; e < ee; e++) {
                    const int n = in_crow[e];
                    if ((unsigned)n < (unsigned)B) {
                        const float x = in_cval[e];
                        int64_t lo = lv_ptr[n], hi = lv_ptr[n + 1];
                        lo = lo < 0 ? 0 : lo; hi = hi < n_live ? hi : n_live;
                        int64_t a = lo, z = hi;              // first slot of the batch row at or behind column c0
                        while (a < z) {
                            const int64_t mid = (a + z) >> 1;
                            if (lv_item[mid] < c0) a = mid + 1; else z = mid;
                        }
                        for (int64_t s = a + t; s < hi; s += 256) {
                            const unsigned off = (unsigned)(lv_item[s] - c0);
                            if (off >= (unsigned)kChunk) break;
                            g_lds[off] += x * delta[s];
                        }
                    }
                    __syncthreads();
                }
                g = *reinterpret_cast<const f32x4 *>(&g_lds[4 * t]);     // this thread's own four columns: the next tile's clear needs no barrier
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int j = c + q;
                if (j >= n_items) continue;
                int64_t eb = lv_cptr[j], ee = lv_cptr[j + 1];
                ee = ee < n_live ? ee : n_live;
                float acc = 0.0f;
                for (int64_t e = eb < 0 ? 0 : eb; e < ee; e++) {
                    const int s = lv_cslot[e];
                    if ((uint64_t)(int64_t)s < (uint64_t)n_live) acc += delta[s];
                }
                g[q] = acc;
            }
        }
        if (c >= ld) continue;
        const size_t at = row < n_items ? (size_t)row * ld + c : (size_t)c;
        f32x4 *pt = reinterpret_cast<f32x4 *>((row < n_items ? W : bias) + at);
        f32x4 *pm = reinterpret_cast<f32x4 *>((row < n_items ? mW : mb) + at);
        f32x4 *pv = reinterpret_cast<f32x4 *>((row < n_items ? vW : vb) + at);
        f32x4 th = *pt, mm = *pm, vv = *pv;
        adam_update(th, mm, vv, g, adam);
        *pt = th; *pm = mm; *pv = vv;
        float *go = row < n_items ? gW_out : gb_out;
        if (go) *reinterpret_cast<f32x4 *>(go + at) = g;
    }
}

// ---- evaluation: the block route's transposed score block from the rated CSR --------------------------------------------
// S_T[item][b] = sum over the rated items i of user b, ascending i, of C[u,i] W[i][item]: an SpMM whose dense operand has row
// stride ld.  A workgroup owns 64 items x 64 users: a wavefront reads W rows with its lanes across the items (256 contiguous
// bytes per read), 16 users one after another; the tile is turned in LDS so that the block is written with the lanes across
// the users.  No users x items input exists.
__global__ __launch_bounds__(256) void sparse_row_fill_kernel(const float *__restrict__ W, int ld, int n_items, const int64_t *__restrict__ indptr,
                                                              const int32_t *__restrict__ items, const float *__restrict__ vals,
                                                              const int32_t *__restrict__ user_ids, int n_b, int b_pad, float *__restrict__ S_T) {
    __shared__ float tile[64][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
    const int item = item0 + lane;
    for (int k = 0; k < 16; k++) {
        const int bl = wave * 16 + k, b = b0 + bl;
        float acc = 0.0f;
        if (b < n_b && item < n_items) {
            const int u = user_ids[b];
            for (int64_t e = indptr[u], end = indptr[u + 1]; e < end; e++) {
                const int i = items[e];
                if ((unsigned)i < (unsigned)n_items) acc += vals[e] * W[(size_t)i * ld + item];
            }
        }
        tile[lane][bl] = acc;
    }
    __syncthreads();
    for (int k = 0; k < 16; k++) {
        const int it = wave * 16 + k;
        if (item0 + it < n_items) S_T[(size_t)(item0 + it) * b_pad + b0 + lane] = tile[it][lane];
    }
}

bool shape_ok(int n_items, int ld) { return n_items >= 1 && ld >= n_items && ld % 32 == 0; }

}  // namespace

namespace qrec {
// the fill pass of qrec_score_topk_sparse_row_sigmoid_bias; S_T is the block route's [n_items][b_pad] score block
int score_block_sparse_rows(float *S_T, const SparseRows &r, int n_items, const int32_t *user_ids, int n_b, int b_pad, hipStream_t st) {
    const dim3 grid((unsigned)((n_items + 63) / 64), (unsigned)(b_pad / 64));
    hipLaunchKernelGGL(sparse_row_fill_kernel, grid, dim3(256), 0, st, r.W, r.ld, n_items, r.indptr, r.items, r.vals, user_ids, n_b, b_pad, S_T);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}
}  // namespace qrec

extern "C" {

#define QREC_CFGAN_SHAPE(name)                                                                                                   \
    do {                                                                                                                         \
        QREC_REQUIRE(shape_ok(n_items, ld), name ": bad shape (n_items=%d, ld=%d; ld must be a multiple of 32 and >= n_items)",  \
                     n_items, ld);                                                                                               \
        if (n_items > QREC_CFGAN_MAX_ITEMS) {                                                                                    \
            ::qrec::set_error(name ": %d items above the supported %d", n_items, QREC_CFGAN_MAX_ITEMS);                          \
            return QREC_ERR_UNSUPPORTED;                                                                                         \
        }                                                                                                                        \
    } while (0)

int qrec_cfgan_workspace_bytes(int32_t B, int64_t n_live, int64_t *bytes) {
    QREC_REQUIRE(bytes && B >= 0 && n_live >= 0, "qrec_cfgan_workspace_bytes: bad arguments");
    *bytes = layout_bytes(ws_layout, B, n_live);
    return QREC_OK;
}

int qrec_cfgan_forward(const float *d_W, const float *d_b, const float *d_thetaD, int32_t n_items, int32_t ld, int32_t B, int64_t n_in,
                       int64_t n_live, const int32_t *d_in_ptr, const int32_t *d_in_item, const float *d_in_val, const int32_t *d_lv_ptr,
                       const int32_t *d_lv_item, const int32_t *d_lv_flag, float alpha, void *d_ws, double *d_losses, void *stream) {
    QREC_CFGAN_SHAPE("qrec_cfgan_forward");
    QREC_REQUIRE(B >= 1 && n_in >= 0 && n_live >= 0 && n_live <= INT32_MAX && n_in <= INT32_MAX, "qrec_cfgan_forward: bad sizes");
    QREC_REQUIRE(d_W && d_b && d_thetaD && d_in_ptr && d_lv_ptr && d_ws && d_losses && (n_in == 0 || (d_in_item && d_in_val)) &&
                     (n_live == 0 || (d_lv_item && d_lv_flag)),
                 "qrec_cfgan_forward: null argument");
    const Ws w = carve(d_ws, ws_layout, B, n_live);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(row_kernel, dim3((unsigned)B), dim3(256), 0, st, d_W, d_b, d_thetaD, n_items, ld, B, n_in, n_live, d_in_ptr, d_in_item,
                       d_in_val, d_lv_ptr, d_lv_item, d_lv_flag, alpha, (float)(1.0 / (double)B), w);
    QREC_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(256), 0, st, w.terms, B, (double)alpha, d_losses);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_cfgan_dis_step(float *d_thetaD, float *d_mD, float *d_vD, int32_t n_items, int32_t B, int64_t n_in, int64_t n_live,
                        const int32_t *d_in_cptr, const int32_t *d_in_crow, const float *d_in_cval, const int32_t *d_lv_cptr,
                        const int32_t *d_lv_crow, const int32_t *d_lv_cslot, void *d_ws, float adam_alpha, float beta1, float beta2, float eps,
                        float *d_grad_out, void *stream) {
    const int32_t ld = (n_items + 31) / 32 * 32;
    QREC_CFGAN_SHAPE("qrec_cfgan_dis_step");
    QREC_REQUIRE(B >= 1 && n_in >= 0 && n_live >= 0, "qrec_cfgan_dis_step: bad sizes");
    QREC_REQUIRE(d_thetaD && d_mD && d_vD && d_in_cptr && d_lv_cptr && d_ws && (n_in == 0 || (d_in_crow && d_in_cval)) &&
                     (n_live == 0 || (d_lv_crow && d_lv_cslot)),
                 "qrec_cfgan_dis_step: null argument");
    const Ws w = carve(d_ws, ws_layout, B, n_live);
    const unsigned blocks = (unsigned)((2 * (int64_t)n_items + 1 + 255) / 256);
    hipLaunchKernelGGL(dis_step_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_thetaD, d_mD, d_vD, n_items, B, n_in, n_live, d_in_cptr,
                       d_in_crow, d_in_cval, d_lv_cptr, d_lv_crow, d_lv_cslot, w, AdamArgs{adam_alpha, beta1, beta2, eps}, d_grad_out);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_cfgan_gen_sweep(float *d_W, float *d_mW, float *d_vW, float *d_b, float *d_mb, float *d_vb, int32_t n_items, int32_t ld, int32_t B,
                         int64_t n_in, int64_t n_live, const int32_t *d_in_cptr, const int32_t *d_in_crow, const float *d_in_cval,
                         const int32_t *d_lv_ptr, const int32_t *d_lv_item, const int32_t *d_lv_cptr, const int32_t *d_lv_cslot, void *d_ws,
                         float adam_alpha, float beta1, float beta2, float eps, float *d_gradW_out, float *d_gradb_out, void *stream) {
    QREC_CFGAN_SHAPE("qrec_cfgan_gen_sweep");
    QREC_REQUIRE(B >= 1 && n_in >= 0 && n_live >= 0, "qrec_cfgan_gen_sweep: bad sizes");
    QREC_REQUIRE(d_W && d_mW && d_vW && d_b && d_mb && d_vb && d_in_cptr && d_lv_ptr && d_lv_cptr && d_ws &&
                     (n_in == 0 || (d_in_crow && d_in_cval)) && (n_live == 0 || (d_lv_item && d_lv_cslot)),
                 "qrec_cfgan_gen_sweep: null argument");
    const Ws w = carve(d_ws, ws_layout, B, n_live);
    const int64_t n_tiles = ((int64_t)n_items + 1) * ((ld + kChunk - 1) / kChunk);
    const unsigned blocks = (unsigned)(n_tiles < 2048 ? n_tiles : 2048);         // 256 CUs x 8 workgroups, the rest by stride
    hipLaunchKernelGGL(sweep_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_W, d_mW, d_vW, d_b, d_mb, d_vb, n_items, ld, B, n_in,
                       n_live, d_in_cptr, d_in_crow, d_in_cval, d_lv_ptr, d_lv_item, d_lv_cptr, d_lv_cslot, w.delta,
                       AdamArgs{adam_alpha, beta1, beta2, eps}, d_gradW_out, d_gradb_out);
    QREC_LAUNCH_CHECK();
    return QREC_OK;
}

int qrec_cfgan_read_slots(const void *d_ws, int32_t B, int64_t n_live, float *d_rhat, float *d_delta, float *d_a_r, float *d_a_f, void *stream) {
    QREC_REQUIRE(d_ws && B >= 1 && n_live >= 0, "qrec_cfgan_read_slots: bad arguments");
    const Ws w = carve(const_cast<void *>(d_ws), ws_layout, B, n_live);
    hipStream_t st = as_stream(stream);
    if (d_rhat && n_live) QREC_HIP_CHECK(hipMemcpyAsync(d_rhat, w.rhat, sizeof(float) * (size_t)n_live, hipMemcpyDeviceToDevice, st));
    if (d_delta && n_live) QREC_HIP_CHECK(hipMemcpyAsync(d_delta, w.delta, sizeof(float) * (size_t)n_live, hipMemcpyDeviceToDevice, st));
    if (d_a_r) QREC_HIP_CHECK(hipMemcpyAsync(d_a_r, w.a_r, sizeof(float) * (size_t)B, hipMemcpyDeviceToDevice, st));
    if (d_a_f) QREC_HIP_CHECK(hipMemcpyAsync(d_a_f, w.a_f, sizeof(float) * (size_t)B, hipMemcpyDeviceToDevice, st));
    return QREC_OK;
}

#undef QREC_CFGAN_SHAPE

}  // extern "C"
