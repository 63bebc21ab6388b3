// Value tokens (gfx950): low-dimensional numbers (proprioception: joint angles, gripper opening,
// end-effector pose, the previous action) as sequence rows. The reference's Gato-style pieces
// (tokenizers/numeric_values/value_tokenizer.py:18-34): mu_law_encoder companding, uniform bins,
// one nn.Embed table over the discrete ids. Semantics in include/mmt_api.h ("value tokens").
//
// Forward: one thread per (sample, value, 8 columns) encodes the value and writes
// table[token] + pe[row] into the value's row of x0 (the rows mmt_seq_assemble_fwd leaves alone,
// kind 3); the thread of column chunk 0 also saves the token for the backward.
// Backward: one wave owns one table entry x one 64-column slice, walks every saved token in
// ascending (b, j) order and adds the matching rows of dx0 into its register accumulator, then
// adds the accumulator once into dtable. One writer per entry and a fixed order: no
// float atomics, so the result does not depend on the deterministic mode and equals a sequential
// fp32 sum bit for bit.
#include <math.h>

#include <cmath>

#include "common.h"

using namespace mmt;

namespace {

// value -> token. fp32 throughout; the products and quotients are the explicitly rounded
// intrinsics, so -ffp-contract=fast cannot fuse mu * |s| into log1pf's first add.
__device__ __forceinline__ int value_token(float v, int encoding, float mu, int N) {
  const float s = fminf(fmaxf(v, -1.f), 1.f);  // IEEE fmax / fmin: NaN -> -1
  float y = s;
  if (encoding == MMT_VALUE_MU_LAW)
    y = copysignf(__fdiv_rn(log1pf(__fmul_rn(mu, fabsf(s))), log1pf(mu)), s);
  const int t = (int)floorf(__fmul_rn(__fmul_rn(y + 1.f, 0.5f), (float)N));
  return max(0, min(N - 1, t));
}

// A value row of a (B, L, D) sequence addressed without L: row r of a sample lies inside the
// sample's xs_b elements iff r >= 0 and r * xs_t + D <= xs_b.
__device__ __forceinline__ bool row_inside(int r, int64_t xs_b, int64_t xs_t, int D) {
  return r >= 0 && (int64_t)r * xs_t + D <= xs_b;
}

__global__ void value_tokens_fwd_kernel(const float* __restrict__ values, int64_t ld_v, int B, int n,
                                        int encoding, float mu, int N,
                                        const float* __restrict__ table,
                                        const float* __restrict__ pe,
                                        const int32_t* __restrict__ rows, int D,
                                        float* __restrict__ x0, int64_t xs_b, int64_t xs_t,
                                        int32_t* __restrict__ tok, unsigned int* fault) {
  const int cpr = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * n * cpr) return;
  const int ch = idx % cpr;
  const int j = (idx / cpr) % n;
  const int b = idx / ((int64_t)cpr * n);
  const int d0 = ch * 8;
  const int t = value_token(values[(int64_t)b * ld_v + j], encoding, mu, N);
  if (ch == 0) tok[(int64_t)b * n + j] = t;
  const int row = rows[j];
  if (!row_inside(row, xs_b, xs_t, D)) {  // never written outside the sample
    if (ch == 0) record_fault(fault, MMT_FAULT_ROW_INDEX);
    return;
  }
  const float* tp = table + (int64_t)t * D + d0;
  const float4 a = *reinterpret_cast<const float4*>(tp), c = *reinterpret_cast<const float4*>(tp + 4);
  float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] += pe[(int64_t)row * D + d0 + e];
  float* xo = x0 + (int64_t)b * xs_b + (int64_t)row * xs_t + d0;
  *reinterpret_cast<float4*>(xo) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(xo + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

constexpr int VT_COLS = 64;   // columns per wave: one per lane, a 256-B piece of a row
constexpr int VT_AHEAD = 8;   // matching rows loaded before their adds (the adds keep their order)

__global__ __launch_bounds__(64) void value_tokens_bwd_kernel(
    const float* __restrict__ dx0, int64_t xs_b, int64_t xs_t, int B, int n,
    const int32_t* __restrict__ tok, const int32_t* __restrict__ rows, int D, int N,
    float* __restrict__ dtable, unsigned int* fault) {
  const int lane = threadIdx.x;
  const int col = blockIdx.x * VT_COLS + lane;
  const int k = blockIdx.y;  // this wave's table entry
  const bool live = col < D;
  const bool reporter = blockIdx.x == 0 && blockIdx.y == 0;  // one wave reports, all skip
  float acc = 0.f;
  const int total = B * n;
  for (int i0 = 0; i0 < total; i0 += 64) {
    // lane l holds token i0 + l: whether it is this wave's entry, and the element offset of its
    // row in dx0
    const int i = i0 + lane;
    bool mine = false;
    int64_t off = 0;
    if (i < total) {
      const int t = tok[i];
      const int b = i / n, row = rows[i - b * n];
      const bool ok = (unsigned)t < (unsigned)N && row_inside(row, xs_b, xs_t, D);
      if (!ok && reporter) record_fault(fault, MMT_FAULT_ROW_INDEX);
      mine = ok && t == k;
      off = (int64_t)b * xs_b + (int64_t)row * xs_t;
    }
    unsigned long long m = __ballot(mine);
    while (m) {  // the matching tokens of this chunk, ascending; m is wave-uniform
      float v[VT_AHEAD];
#pragma unroll
      for (int u = 0; u < VT_AHEAD; ++u) {
        v[u] = 0.f;
        if (m) {
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)off, l);
          const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)off >> 32), l);
          const int64_t o = (int64_t)(((uint64_t)hi << 32) | lo);
          if (live) v[u] = dx0[o + col];
        }
      }
      // a slot past the chunk's last match adds +0, which changes no fp32 value the accumulator
      // can hold (it starts at +0 and round-to-nearest sums never give -0)
#pragma unroll
      for (int u = 0; u < VT_AHEAD; ++u) acc += v[u];
    }
  }
  if (live) dtable[(int64_t)k * D + col] += acc;
}

}  // namespace

extern "C" int mmt_value_tokens_fwd(const float* values, int64_t ld_v, int B, int n, int encoding,
                                    float mu, int num_bins, const float* table, const float* pe,
                                    const int32_t* rows, int D, void* x0, int64_t xs_b,
                                    int64_t xs_t, int32_t* tok, mmt_stream_t stream) {
  MMT_CHECK_ARG(values && table && pe && rows && x0 && tok, "mmt_value_tokens_fwd: null pointer");
  MMT_CHECK_ARG(B > 0 && n > 0 && (int64_t)B * n <= INT32_MAX && ld_v >= n,
                "mmt_value_tokens_fwd: B, n must be > 0 (B * n < 2^31), ld_v >= n");
  MMT_CHECK_ARG(D > 0 && D % 8 == 0, "mmt_value_tokens_fwd: D must be > 0 and a multiple of 8");
  MMT_CHECK_ARG(num_bins >= MMT_VALUE_MIN_BINS && num_bins <= MMT_VALUE_MAX_BINS,
                "mmt_value_tokens_fwd: num_bins %d outside %d .. %d", num_bins, MMT_VALUE_MIN_BINS,
                MMT_VALUE_MAX_BINS);
  MMT_CHECK_ARG(encoding == MMT_VALUE_UNIFORM || encoding == MMT_VALUE_MU_LAW,
                "mmt_value_tokens_fwd: unknown encoding %d", encoding);
  MMT_CHECK_ARG(encoding != MMT_VALUE_MU_LAW || (std::isfinite(mu) && mu > 0.f),
                "mmt_value_tokens_fwd: mu must be finite and > 0");
  MMT_CHECK_ARG(aligned_to(x0, 16) && aligned_to(table, 16),
                "mmt_value_tokens_fwd: x0 and table must be 16-B aligned");
  MMT_CHECK_ARG(xs_t >= D && xs_t % 4 == 0 && xs_b % 4 == 0,
                "mmt_value_tokens_fwd: strides (xs_t >= D, xs_b and xs_t multiples of 4)");
  const int64_t total = (int64_t)B * n * (D / 8);
  hipLaunchKernelGGL(value_tokens_fwd_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     as_stream(stream), values, ld_v, B, n, encoding, mu, num_bins, table, pe, rows,
                     D, (float*)x0, xs_b, xs_t, tok, fault_word());
  MMT_CHECK_LAUNCH("mmt_value_tokens_fwd");
  return MMT_OK;
}

extern "C" int mmt_value_tokens_bwd(const void* dx0, int64_t xs_b, int64_t xs_t, int B, int n,
                                    const int32_t* tok, const int32_t* rows, int D, int num_bins,
                                    float* dtable, mmt_stream_t stream) {
  MMT_CHECK_ARG(dx0 && tok && rows && dtable, "mmt_value_tokens_bwd: null pointer");
  MMT_CHECK_ARG(B > 0 && n > 0 && (int64_t)B * n <= INT32_MAX - 64,
                "mmt_value_tokens_bwd: B, n must be > 0 (B * n < 2^31)");
  MMT_CHECK_ARG(D > 0 && D % 8 == 0, "mmt_value_tokens_bwd: D must be > 0 and a multiple of 8");
  MMT_CHECK_ARG(num_bins >= MMT_VALUE_MIN_BINS && num_bins <= MMT_VALUE_MAX_BINS,
                "mmt_value_tokens_bwd: num_bins %d outside %d .. %d", num_bins, MMT_VALUE_MIN_BINS,
                MMT_VALUE_MAX_BINS);
  MMT_CHECK_ARG(aligned_to(dx0, 16) && aligned_to(dtable, 16),
                "mmt_value_tokens_bwd: dx0 and dtable must be 16-B aligned");
  MMT_CHECK_ARG(xs_t >= D && xs_t % 4 == 0 && xs_b % 4 == 0,
                "mmt_value_tokens_bwd: strides (xs_t >= D, xs_b and xs_t multiples of 4)");
  const dim3 grid((D + VT_COLS - 1) / VT_COLS, num_bins);
  hipLaunchKernelGGL(value_tokens_bwd_kernel, grid, dim3(64), 0, as_stream(stream),
                     (const float*)dx0, xs_b, xs_t, B, n, tok, rows, D, num_bins, dtable,
                     fault_word());
  MMT_CHECK_LAUNCH("mmt_value_tokens_bwd");
  return MMT_OK;
}
