// Microbenchmark 4b: the "ATOMICS ONLY" replay of atomics4.hip -- the shipped item-major stream at the Yelp2018 shape, the same
// triplets (same generator, same seed), the same chunks and stride, 16 lanes x 4 contiguous-segment dword atomics (64-byte
// requests) per row update, no row loads -- with the adds issued as f32 (global_atomic_add_f32) and as u32
// (global_atomic_add_u32, the delta converted as a fixed-point kernel would: rint(delta * 2^26)).  f32 and u32 alternate in one
// process, at 256 and at 1,024 blocks.  Beside them, the passes a fixed-point epoch would add around the kernel, timed the same
// way: fp32 -> int32 in place over both tables (convert-in), and the epoch close's read of both tables with and without the
// int32 -> fp32 write-back (convert-out).  Gate of DESIGN s5.1: u32 gain at 256 blocks > 2 x (convert-in + write-back surcharge).
// Two more u32 rows in the same rounds: HALF-POPULATED wavefronts (lanes 32-63 idle, two groups per wavefront, so a wave instruction
// carries two 64-byte requests) at 512 blocks -- the 4,096 groups of the 256-block row on twice the wavefronts -- and at 2,048 blocks,
// the groups of the 1,024-block row.  Gate of the two-groups-per-wavefront kernel: the 512-block half row's lowest time must beat the
// 256-block full row's lowest by more than twice that row's own max - min.
// Usage: atomics4_u32 [result.json]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>
constexpr int LD = 64;
constexpr float kScale = 67108864.f;      // 2^26
__device__ inline void row_atomic(float* tab, int row, int r, float v) { float* p = tab + (long)row * LD; for (int e = 0; e < 4; e++) unsafeAtomicAdd(p + r + 16 * e, v); }
__device__ inline void row_atomic(unsigned* tab, int row, int r, float v) { unsigned* p = tab + (long)row * LD; const unsigned q = (unsigned)__float2int_rn(v * kScale); for (int e = 0; e < 4; e++) atomicAdd(p + r + 16 * e, q); }
// walk_t<false> of atomics4.hip, the element type a parameter
template <typename T, int ACTIVE = 4>          // ACTIVE: groups of a wavefront that work (4: all; 2: lanes 32-63 idle)
__global__ __launch_bounds__(256) void walk_atomics(T* A, T* B, T* C, const int* a_row, const int* b_row, const int* c_row, long n, int CH, int flush, long stride) {
  const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
  if (g >= ACTIVE) return;
  const long grp = (((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * ACTIVE + g, ngrp = (((long)gridDim.x * blockDim.x) >> 6) * ACTIVE;
  const long nch = (n + CH - 1) / CH;
  for (long s = grp; s < nch; s += ngrp) {
    const long c = (s * stride) % nch;
    const long t0 = c * CH, t1 = t0 + CH < n ? t0 + CH : n;
    int cur = a_row[t0], since = 0; float acc = 1.f;
    for (long t = t0; t < t1; t++) {
      const int a = a_row[t];
      if (a != cur || since == flush) { row_atomic(A, cur, r, acc * 1e-7f); cur = a; since = 0; }
      acc += 2.f; since++;
      row_atomic(B, b_row[t], r, 1e-7f);
      row_atomic(C, c_row[t], r, 1e-7f);
    }
    row_atomic(A, cur, r, acc * 1e-7f);
  }
}
// convert-in: fp32 -> int32 in place; a value out of range or not finite raises the flag (plain store)
__global__ __launch_bounds__(256) void convert_in(float4* P, long p4, float4* Q, long q4, double* flag) {
  bool bad = false;
  for (int tab = 0; tab < 2; tab++) {
    float4* x = tab ? Q : P; const long n4 = tab ? q4 : p4;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n4; k += (long)gridDim.x * blockDim.x) {
      const float4 v = x[k];
      bad |= !(fabsf(v.x) < 16.f) | !(fabsf(v.y) < 16.f) | !(fabsf(v.z) < 16.f) | !(fabsf(v.w) < 16.f);
      reinterpret_cast<int4*>(x)[k] = make_int4(__float2int_rn(v.x * kScale), __float2int_rn(v.y * kScale), __float2int_rn(v.z * kScale), __float2int_rn(v.w * kScale));
    }
  }
  if (bad) *flag = 1.0;
}
// the epoch close's table pass: sum of squares of both tables, one partial per block; OUT: the tables hold int32, are written back as fp32
template <bool OUT>
__device__ inline double table_pass(float4* x, long n4) {
  double acc = 0.0;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n4; k += (long)gridDim.x * blockDim.x) {
    float4 v;
    if (OUT) { const int4 q = reinterpret_cast<const int4*>(x)[k]; v = make_float4(q.x * (1.f / kScale), q.y * (1.f / kScale), q.z * (1.f / kScale), q.w * (1.f / kScale)); x[k] = v; }
    else v = x[k];
    acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  return acc;
}
template <bool OUT>
__global__ __launch_bounds__(256) void close_pass(float4* P, long p4, float4* Q, long q4, double* part) {
  const double sp = table_pass<OUT>(P, p4), sq = table_pass<OUT>(Q, q4);
  __shared__ double s[2][4];
  if ((threadIdx.x & 63) == 0) { s[0][threadIdx.x >> 6] = sp; s[1][threadIdx.x >> 6] = sq; }
  __syncthreads();
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s[0][0] + s[0][1] + s[0][2] + s[0][3]; part[2 * blockIdx.x + 1] = s[1][0] + s[1][1] + s[1][2] + s[1][3]; }
}
static std::vector<double> zipf_cdf(long n, double a) { std::vector<double> c(n); double s = 0; for (long k = 0; k < n; k++) { s += pow(k + 1.0, -a); c[k] = s; } return c; }
template <typename F> float once_ms(F f) { static hipEvent_t a = nullptr, b = nullptr; if (!a) { hipEventCreate(&a); hipEventCreate(&b); } hipEventRecord(a); f(); hipEventRecord(b); hipEventSynchronize(b); float ms; hipEventElapsedTime(&ms, a, b); return ms; }
struct Series { std::vector<float> v; float lo() const { return *std::min_element(v.begin(), v.end()); } float hi() const { return *std::max_element(v.begin(), v.end()); } float med() const { auto s = v; std::sort(s.begin(), s.end()); return s[s.size() / 2]; } };
int main(int argc, char** argv) {
  const long U = 31668, I = 38048, n = 1252669;
  std::mt19937_64 rng(1);
  auto cu = zipf_cdf(U, 0.4), ci = zipf_cdf(I, 0.6);
  std::vector<int> pu(U), pi(I); std::iota(pu.begin(), pu.end(), 0); std::iota(pi.begin(), pi.end(), 0);
  std::shuffle(pu.begin(), pu.end(), rng); std::shuffle(pi.begin(), pi.end(), rng);
  auto draw = [&](const std::vector<double>& c) { std::uniform_real_distribution<double> d(0, c.back()); return (long)(std::lower_bound(c.begin(), c.end(), d(rng)) - c.begin()); };
  std::vector<int> u(n), i(n), j(n);
  for (long t = 0; t < n; t++) { u[t] = pu[draw(cu)]; i[t] = pi[draw(ci)]; j[t] = rng() % I; }
  std::vector<long> o(n); std::iota(o.begin(), o.end(), 0L); std::stable_sort(o.begin(), o.end(), [&](long a, long b) { return i[a] < i[b]; });
  std::vector<int> iu(n), ii(n), ij(n); for (long t = 0; t < n; t++) { iu[t] = u[o[t]]; ii[t] = i[o[t]]; ij[t] = j[o[t]]; }
  float *P, *Q; double *part, *flag; hipMalloc(&P, U * LD * 4); hipMalloc(&Q, I * LD * 4); hipMalloc(&part, 2 * 4096 * 8); hipMalloc(&flag, 8);
  int *du, *di, *dj; hipMalloc(&du, n * 4); hipMalloc(&di, n * 4); hipMalloc(&dj, n * 4);
  hipMemcpy(du, iu.data(), n * 4, hipMemcpyHostToDevice); hipMemcpy(di, ii.data(), n * 4, hipMemcpyHostToDevice); hipMemcpy(dj, ij.data(), n * 4, hipMemcpyHostToDevice);
  const int CH = 34; const long nch = (n + CH - 1) / CH; long stride = (long)(nch * 0.6180339887); while (std::gcd(stride, nch) != 1) stride++;
  const int ROUNDS = 7;             // round 0 warms up and is dropped
  Series f32[2], u32[2], half[2], cin, cf, co; const int blocks[2] = {256, 1024};
  for (int rep = 0; rep < ROUNDS; rep++)
    for (int b = 0; b < 2; b++) {
      hipMemset(P, 0, U * LD * 4); hipMemset(Q, 0, I * LD * 4);
      const float mf = once_ms([&] { hipLaunchKernelGGL(walk_atomics<float>, dim3(blocks[b]), dim3(256), 0, 0, Q, P, Q, di, du, dj, n, CH, 16, stride); });
      hipMemset(P, 0, U * LD * 4); hipMemset(Q, 0, I * LD * 4);
      const float mu = once_ms([&] { hipLaunchKernelGGL(walk_atomics<unsigned>, dim3(blocks[b]), dim3(256), 0, 0, (unsigned*)Q, (unsigned*)P, (unsigned*)Q, di, du, dj, n, CH, 16, stride); });
      hipMemset(P, 0, U * LD * 4); hipMemset(Q, 0, I * LD * 4);
      const float mh = once_ms([&] { hipLaunchKernelGGL((walk_atomics<unsigned, 2>), dim3(2 * blocks[b]), dim3(256), 0, 0, (unsigned*)Q, (unsigned*)P, (unsigned*)Q, di, du, dj, n, CH, 16, stride); });
      if (rep) { f32[b].v.push_back(mf); u32[b].v.push_back(mu); half[b].v.push_back(mh); }
    }
  // the passes on the grids the library gives them: the close 256 blocks (QREC_STATS_MAX_BLOCKS), convert-in up to 1,024
  const long p4 = U * LD / 4, q4 = I * LD / 4; const int cb = (int)std::min<long>(256, (std::max(p4, q4) + 255) / 256), ib = (int)std::min<long>(1024, (std::max(p4, q4) + 255) / 256);
  for (int rep = 0; rep < ROUNDS; rep++) {
    hipMemset(P, 0, U * LD * 4); hipMemset(Q, 0, I * LD * 4);
    hipLaunchKernelGGL(walk_atomics<float>, dim3(256), dim3(256), 0, 0, Q, P, Q, di, du, dj, n, CH, 16, stride);     // the tables as an epoch leaves them
    const float a = once_ms([&] { hipLaunchKernelGGL(close_pass<false>, dim3(cb), dim3(256), 0, 0, (float4*)P, p4, (float4*)Q, q4, part); });
    const float c = once_ms([&] { hipLaunchKernelGGL(convert_in, dim3(ib), dim3(256), 0, 0, (float4*)P, p4, (float4*)Q, q4, flag); });
    hipLaunchKernelGGL(walk_atomics<unsigned>, dim3(256), dim3(256), 0, 0, (unsigned*)Q, (unsigned*)P, (unsigned*)Q, di, du, dj, n, CH, 16, stride);
    const float d = once_ms([&] { hipLaunchKernelGGL(close_pass<true>, dim3(cb), dim3(256), 0, 0, (float4*)P, p4, (float4*)Q, q4, part); });
    if (rep) { cf.v.push_back(a); cin.v.push_back(c); co.v.push_back(d); }
  }
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) { fprintf(stderr, "HIP error\n"); return 1; }
  const float pass_cost = cin.lo() + (co.lo() - cf.lo()), gain256 = f32[0].lo() - u32[0].lo();
  FILE* out = argc > 1 ? fopen(argv[1], "w") : stdout; if (!out) return 2;
  fprintf(out, "{\"probe\": \"tools/ubench/atomics4_u32.hip\", \"timing\": \"hipEvent around one launch, lowest and median of %d alternating rounds after one warm-up round\",\n \"replay_atomics_only_ms\": {\n", ROUNDS - 1);
  for (int b = 0; b < 2; b++)
    fprintf(out, "  \"%d_blocks\": {\"f32_min\": %.4f, \"f32_median\": %.4f, \"u32_min\": %.4f, \"u32_median\": %.4f, \"u32_faster_by\": %.4f}%s\n", blocks[b], f32[b].lo(), f32[b].med(), u32[b].lo(),
            u32[b].med(), 1.0 - u32[b].lo() / f32[b].lo(), b ? "" : ",");
  fprintf(out, " },\n \"passes_ms\": {\"close_read_f32_min\": %.4f, \"close_read_i32_write_f32_min\": %.4f, \"convert_in_both_tables_min\": %.4f, \"cost_of_the_passes\": %.4f},\n", cf.lo(), co.lo(), cin.lo(), pass_cost);
  fprintf(out, " \"gate\": {\"u32_gain_at_256_blocks_ms\": %.4f, \"twice_the_passes_ms\": %.4f, \"passed\": %s},\n", gain256, 2 * pass_cost, gain256 > 2 * pass_cost ? "true" : "false");
  const float spread256 = u32[0].hi() - u32[0].lo(), half_gain = u32[0].lo() - half[0].lo();
  fprintf(out, " \"half_populated_wavefronts_u32_ms\": {\"512_blocks\": {\"min\": %.4f, \"median\": %.4f, \"max\": %.4f}, \"2048_blocks\": {\"min\": %.4f, \"median\": %.4f, \"max\": %.4f},\n"
               "  \"full_256_blocks\": {\"min\": %.4f, \"max\": %.4f}, \"full_1024_blocks\": {\"min\": %.4f, \"max\": %.4f},\n"
               "  \"gate\": {\"gain_of_512_half_over_256_full_ms\": %.4f, \"twice_the_256_block_spread_ms\": %.4f, \"passed\": %s}}}\n",
          half[0].lo(), half[0].med(), half[0].hi(), half[1].lo(), half[1].med(), half[1].hi(), u32[0].lo(), u32[0].hi(), u32[1].lo(), u32[1].hi(), half_gain, 2 * spread256,
          half_gain > 2 * spread256 ? "true" : "false");
  if (out != stdout) fclose(out);
  return 0;
}
