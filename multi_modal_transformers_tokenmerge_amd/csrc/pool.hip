// Multi-head attention pooling of the readout tokens (gfx950): the reference's
// MultiHeadAttentionPooling (attention_blocks/attention.py:122-150) around the GEMMs —
//   * readout row gather (fp32 residual stream -> contiguous bf16 GEMM operand) and its backward,
//     which writes the whole (B, L, D) gradient (mmt_rows_mean_bwd's contract);
//   * the single-query attention core: one learnt query shared by the batch against the n <= 64
//     projected readout keys / values of each sample, forward and backward;
//   * flax.linen.LayerNorm over the FEATURE axis of (B, D) rows, forward and backward.
// None of them accumulates across workgroups: every batch reduction (d(query), d(scale),
// d(bias)) is a per-sample fp32 array here, summed by mmt_colsum.
#include <math.h>

#include <type_traits>

#include "common.h"

using namespace mmt;

namespace {

__device__ __forceinline__ void unpack8(const uint4& u, float* f) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f[2 * q] = __uint_as_float(w[q] << 16);
    f[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = (uint32_t)f2bf(f[2 * q]) | ((uint32_t)f2bf(f[2 * q + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void load8(const bf16_t* p, float* f) {
  unpack8(*reinterpret_cast<const uint4*>(p), f);
}
__device__ __forceinline__ void load8(const float* p, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(p), c = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = c.x; f[5] = c.y; f[6] = c.z; f[7] = c.w;
}
__device__ __forceinline__ void store8(bf16_t* p, const float* f) {
  *reinterpret_cast<uint4*>(p) = pack8(f);
}
__device__ __forceinline__ void store8(float* p, const float* f) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// r[b, i, :] = bf16(x[b, rows[i], :]); one 8-element vector per thread
__global__ void rows_gather_bf16_kernel(const float* __restrict__ x, int64_t xs_b, int64_t xs_t,
                                        int B, int L, int D, const int32_t* __restrict__ rows,
                                        int n, bf16_t* __restrict__ r, unsigned int* fault) {
  const int cpr = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * n * cpr) return;
  const int c = (idx % cpr) * 8;
  const int i = (idx / cpr) % n;
  const int b = idx / ((int64_t)cpr * n);
  const int row = checked_index(rows[i], L, fault, MMT_FAULT_ROW_INDEX);
  float f[8];
  load8(x + b * xs_b + (int64_t)row * xs_t + c, f);
  store8(r + ((int64_t)b * n + i) * D + c, f);
}

// dx[b, l, :] = dr[b, row_flag[l], :] for row_flag[l] >= 0, 0 otherwise (the whole buffer)
__global__ void rows_scatter_bwd_kernel(const bf16_t* __restrict__ dr, int B, int L, int D,
                                        const int32_t* __restrict__ row_flag, int n,
                                        float* __restrict__ dx, unsigned int* fault) {
  const int cpr = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * L * cpr) return;
  const int c = (idx % cpr) * 8;
  const int l = (idx / cpr) % L;
  const int b = idx / ((int64_t)cpr * L);
  const int flag = row_flag[l];
  float f[8] = {};
  if (flag >= 0) {
    const int i = checked_index(flag, n, fault, MMT_FAULT_ROW_INDEX);
    load8(dr + ((int64_t)b * n + i) * D + c, f);
  }
  store8(dx + ((int64_t)b * L + l) * D + c, f);
}

// ---------------------------------------------------------------- single-query attention core
// One wave per (sample, head); a workgroup = one sample, its 4 waves stride over the heads.
// Lane layout: G = pow2ceil(Dh / 8) lanes (<= 64) cover one key row in 16-B vectors, KP = 64 / G
// keys are processed side by side: lane = ks * G + c (key slot ks, vector c). Sums over Dh are
// xor shuffles inside a G-lane group, sums over keys xor shuffles across the groups. Softmax:
// lane j holds key j's score (n <= 64), max / sum over the wave. Every shuffle is executed by all
// 64 lanes; only loads and stores are predicated.
constexpr int POOL_WAVES = 4;

__device__ __forceinline__ float group_sum(float v, int G) {  // all lanes of a G-group get the sum
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float across_groups_sum(float v, int G) {  // over the KP key slots
  for (int o = G; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64 * POOL_WAVES) void attn_pool_fwd_kernel(
    const float* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    int64_t ld_kv, int n, int H, int Dh, int G, bf16_t* __restrict__ ctx, int64_t ld_ctx,
    float* __restrict__ p) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int KP = 64 / G;
  const int c = lane % G, ks = lane / G;
  const bool cok = c * 8 < Dh;
  for (int h = wave; h < H; h += POOL_WAVES) {
    const int64_t col = (int64_t)h * Dh + c * 8;
    float qv[8] = {};
    if (cok) load8(q + col, qv);
    float score = -INFINITY;  // lane j: key j's score
    for (int jb = 0; jb * KP < n; ++jb) {
      const int j = jb * KP + ks;
      float s = 0.f;
      if (cok && j < n) {
        float kv[8];
        load8(k + ((int64_t)b * n + j) * ld_kv + col, kv);
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(qv[e], kv[e], s);
      }
      s = group_sum(s, G);
      const float t = __shfl(s, (lane % KP) * G, 64);  // key jb * KP + lane % KP
      if (lane / KP == jb && lane < n) score = t;
    }
    const float mx = wave_max(score);
    const float ex = lane < n ? expf(score - mx) : 0.f;
    const float den = wave_sum(ex);
    const float pj = ex / den;
    if (lane < n) p[((int64_t)b * H + h) * n + lane] = pj;
    float acc[8] = {};
    for (int jb = 0; jb * KP < n; ++jb) {
      const int j = jb * KP + ks;
      const float w = __shfl(pj, j & 63, 64);  // 0 for j >= n (ex = 0 there)
      if (cok && j < n) {
        float vv[8];
        load8(v + ((int64_t)b * n + j) * ld_kv + col, vv);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, vv[e], acc[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = across_groups_sum(acc[e], G);
    if (cok && ks == 0) store8(ctx + (int64_t)b * ld_ctx + col, acc);
  }
}

__global__ __launch_bounds__(64 * POOL_WAVES) void attn_pool_bwd_kernel(
    const bf16_t* __restrict__ dctx, int64_t ld_dctx, const float* __restrict__ p,
    const float* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    int64_t ld_kv, int n, int H, int Dh, int G, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv,
    int64_t ld_dkv, float* __restrict__ dqb) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int KP = 64 / G;
  const int c = lane % G, ks = lane / G;
  const bool cok = c * 8 < Dh;
  for (int h = wave; h < H; h += POOL_WAVES) {
    const int64_t col = (int64_t)h * Dh + c * 8;
    float qv[8] = {}, dc[8] = {};
    if (cok) {
      load8(q + col, qv);
      load8(dctx + (int64_t)b * ld_dctx + col, dc);
    }
    const float pj = lane < n ? p[((int64_t)b * H + h) * n + lane] : 0.f;
    float dp = 0.f;  // lane j: dctx . v_j
    for (int jb = 0; jb * KP < n; ++jb) {
      const int j = jb * KP + ks;
      const float w = __shfl(pj, j & 63, 64);
      float s = 0.f;
      if (cok && j < n) {
        float vv[8], o[8];
        load8(v + ((int64_t)b * n + j) * ld_kv + col, vv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          s = fmaf(dc[e], vv[e], s);
          o[e] = w * dc[e];
        }
        store8(dv + ((int64_t)b * n + j) * ld_dkv + col, o);
      }
      s = group_sum(s, G);
      const float t = __shfl(s, (lane % KP) * G, 64);
      if (lane / KP == jb && lane < n) dp = t;
    }
    const float dot = wave_sum(pj * dp);
    const float ds = pj * (dp - dot);
    float acc[8] = {};
    for (int jb = 0; jb * KP < n; ++jb) {
      const int j = jb * KP + ks;
      const float w = __shfl(ds, j & 63, 64);
      if (cok && j < n) {
        float kv[8], o[8];
        load8(k + ((int64_t)b * n + j) * ld_kv + col, kv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          acc[e] = fmaf(w, kv[e], acc[e]);
          o[e] = w * qv[e];
        }
        store8(dk + ((int64_t)b * n + j) * ld_dkv + col, o);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = across_groups_sum(acc[e], G);
    if (cok && ks == 0) store8(dqb + (int64_t)b * H * Dh + col, acc);
  }
}

// ---------------------------------------------------------------- feature-axis LayerNorm
// flax.linen.LayerNorm(reduction_axes=[-1]) on (B, D) rows, one wave per row (4 rows per
// workgroup): fast variance max(0, E[x^2] - E[x]^2), y = (x - mu) (rsqrt(var + eps) gamma) + beta.
constexpr int LN_ROWS = 4;

template <typename TX>
__global__ __launch_bounds__(64 * LN_ROWS) void layernorm_fwd_kernel(
    const TX* __restrict__ x, int64_t ldx, int B, int D, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, bf16_t* __restrict__ y, int64_t ldy,
    float* __restrict__ mean, float* __restrict__ rstd) {
  const int row = blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;
  const TX* xr = x + (int64_t)row * ldx;
  float s = 0.f, ss = 0.f;
  for (int c = lane * 8; c < D; c += 512) {
    float f[8];
    load8(xr + c, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s += f[e];
      ss = fmaf(f[e], f[e], ss);
    }
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  const float mu = s / D;
  const float var = fmaxf(0.f, ss / D - mu * mu);
  const float rs = rsqrtf(var + eps);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
  for (int c = lane * 8; c < D; c += 512) {
    float f[8], g[8], bb[8];
    load8(xr + c, f);
    load8(gamma + c, g);
    load8(beta + c, bb);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (f[e] - mu) * (rs * g[e]) + bb[e];
    store8(y + (int64_t)row * ldy + c, f);
  }
}

// g = dy gamma; dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ addend); dyxhat = dy xhat (fp32
// rows: d(scale) is their column sum, d(bias) the column sum of dy). x, addend and dx share TX.
template <typename TDY, typename TX>
__global__ __launch_bounds__(64 * LN_ROWS) void layernorm_bwd_kernel(
    const TDY* __restrict__ dy, int64_t ld_dy, const TX* __restrict__ x, int64_t ldx, int B, int D,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const TX* addend, int64_t ld_add, TX* dx, int64_t ld_dx,
    float* __restrict__ dyxhat) {
  const int row = blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;
  const TX* xr = x + (int64_t)row * ldx;
  const TDY* dr = dy + (int64_t)row * ld_dy;
  const float mu = mean[row], rs = rstd[row];
  float sg = 0.f, sgx = 0.f;
  for (int c = lane * 8; c < D; c += 512) {
    float f[8], d[8], g[8];
    load8(xr + c, f);
    load8(dr + c, d);
    load8(gamma + c, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (f[e] - mu) * rs;
      const float gg = d[e] * g[e];
      sg += gg;
      sgx = fmaf(gg, xh, sgx);
    }
  }
  const float mg = wave_sum(sg) / D, mgx = wave_sum(sgx) / D;
  for (int c = lane * 8; c < D; c += 512) {
    float f[8], d[8], g[8], a[8] = {}, o[8];
    load8(xr + c, f);
    load8(dr + c, d);
    load8(gamma + c, g);
    if (addend) load8(addend + (int64_t)row * ld_add + c, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (f[e] - mu) * rs;
      o[e] = d[e] * xh;
      f[e] = rs * (d[e] * g[e] - mg - xh * mgx) + a[e];
    }
    store8(dx + (int64_t)row * ld_dx + c, f);
    store8(dyxhat + (int64_t)row * D + c, o);
  }
}

inline bool is_dt(int d) { return d == MMT_F32 || d == MMT_BF16; }
inline bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }

// lanes per key row: the power of two >= Dh / 8 (Dh <= 512: at most the whole wave)
inline int pool_group(int Dh) {
  int g = 1;
  while (g * 8 < Dh) g <<= 1;
  return g;
}

}  // namespace

extern "C" int mmt_rows_gather_bf16(const void* x, int64_t xs_b, int64_t xs_t, int B, int L, int D,
                                    const int32_t* rows, int n, void* r, mmt_stream_t stream) {
  MMT_CHECK_ARG(x && rows && r, "mmt_rows_gather_bf16: null pointer");
  MMT_CHECK_ARG(B > 0 && L > 0 && n > 0 && D > 0 && D % 8 == 0,
                "mmt_rows_gather_bf16: B %d, L %d, n %d, D %d (positive, D %% 8 == 0)", B, L, n, D);
  MMT_CHECK_ARG(xs_t >= D && xs_b >= 0 && xs_b % 4 == 0 && xs_t % 4 == 0 && al16(x) && al16(r),
                "mmt_rows_gather_bf16: x strides must be multiples of 4 (xs_t >= D), x and r 16-B aligned");
  const int64_t t = (int64_t)B * n * (D / 8);
  hipLaunchKernelGGL(rows_gather_bf16_kernel, dim3((t + 255) / 256), dim3(256), 0,
                     as_stream(stream), (const float*)x, xs_b, xs_t, B, L, D, rows, n, (bf16_t*)r,
                     fault_word());
  MMT_CHECK_LAUNCH("mmt_rows_gather_bf16");
  return MMT_OK;
}

extern "C" int mmt_rows_scatter_bwd(const void* dr, int B, int L, int D, const int32_t* row_flag,
                                    int n, void* dx, mmt_stream_t stream) {
  MMT_CHECK_ARG(dr && row_flag && dx, "mmt_rows_scatter_bwd: null pointer");
  MMT_CHECK_ARG(B > 0 && L > 0 && n > 0 && D > 0 && D % 8 == 0,
                "mmt_rows_scatter_bwd: B %d, L %d, n %d, D %d (positive, D %% 8 == 0)", B, L, n, D);
  MMT_CHECK_ARG(al16(dr) && al16(dx), "mmt_rows_scatter_bwd: dr and dx must be 16-B aligned");
  const int64_t t = (int64_t)B * L * (D / 8);
  hipLaunchKernelGGL(rows_scatter_bwd_kernel, dim3((t + 255) / 256), dim3(256), 0,
                     as_stream(stream), (const bf16_t*)dr, B, L, D, row_flag, n, (float*)dx,
                     fault_word());
  MMT_CHECK_LAUNCH("mmt_rows_scatter_bwd");
  return MMT_OK;
}

extern "C" int mmt_attn_pool_fwd(const float* q, const void* k, const void* v, int64_t ld_kv,
                                 int B, int n, int H, int Dh, void* ctx, int64_t ld_ctx, float* p,
                                 mmt_stream_t stream) {
  MMT_CHECK_ARG(q && k && v && ctx && p, "mmt_attn_pool_fwd: null pointer");
  MMT_CHECK_ARG(B > 0 && H > 0 && Dh > 0 && Dh % 8 == 0 && Dh <= 512,
                "mmt_attn_pool_fwd: B %d, H %d, Dh %d (positive, Dh %% 8 == 0, Dh <= 512)", B, H, Dh);
  MMT_CHECK_ARG(n >= 1 && n <= 64, "mmt_attn_pool_fwd: n %d not in [1, 64]", n);
  MMT_CHECK_ARG(ld_kv >= (int64_t)H * Dh && ld_kv % 8 == 0 && ld_ctx >= (int64_t)H * Dh &&
                    ld_ctx % 8 == 0,
                "mmt_attn_pool_fwd: row strides must be >= H * Dh and multiples of 8");
  MMT_CHECK_ARG(al16(q) && al16(k) && al16(v) && al16(ctx),
                "mmt_attn_pool_fwd: q, k, v and ctx must be 16-B aligned");
  hipLaunchKernelGGL(attn_pool_fwd_kernel, dim3(B), dim3(64 * POOL_WAVES), 0, as_stream(stream), q,
                     (const bf16_t*)k, (const bf16_t*)v, ld_kv, n, H, Dh, pool_group(Dh),
                     (bf16_t*)ctx, ld_ctx, p);
  MMT_CHECK_LAUNCH("mmt_attn_pool_fwd");
  return MMT_OK;
}

extern "C" int mmt_attn_pool_bwd(const void* dctx, int64_t ld_dctx, const float* p, const float* q,
                                 const void* k, const void* v, int64_t ld_kv, int B, int n, int H,
                                 int Dh, void* dk, void* dv, int64_t ld_dkv, float* dqb,
                                 mmt_stream_t stream) {
  MMT_CHECK_ARG(dctx && p && q && k && v && dk && dv && dqb, "mmt_attn_pool_bwd: null pointer");
  MMT_CHECK_ARG(B > 0 && H > 0 && Dh > 0 && Dh % 8 == 0 && Dh <= 512,
                "mmt_attn_pool_bwd: B %d, H %d, Dh %d (positive, Dh %% 8 == 0, Dh <= 512)", B, H, Dh);
  MMT_CHECK_ARG(n >= 1 && n <= 64, "mmt_attn_pool_bwd: n %d not in [1, 64]", n);
  const int64_t D = (int64_t)H * Dh;
  MMT_CHECK_ARG(ld_kv >= D && ld_kv % 8 == 0 && ld_dkv >= D && ld_dkv % 8 == 0 && ld_dctx >= D &&
                    ld_dctx % 8 == 0,
                "mmt_attn_pool_bwd: row strides must be >= H * Dh and multiples of 8");
  MMT_CHECK_ARG(al16(dctx) && al16(q) && al16(k) && al16(v) && al16(dk) && al16(dv) && al16(dqb),
                "mmt_attn_pool_bwd: dctx, q, k, v, dk, dv and dqb must be 16-B aligned");
  hipLaunchKernelGGL(attn_pool_bwd_kernel, dim3(B), dim3(64 * POOL_WAVES), 0, as_stream(stream),
                     (const bf16_t*)dctx, ld_dctx, p, q, (const bf16_t*)k, (const bf16_t*)v, ld_kv,
                     n, H, Dh, pool_group(Dh), (bf16_t*)dk, (bf16_t*)dv, ld_dkv, dqb);
  MMT_CHECK_LAUNCH("mmt_attn_pool_bwd");
  return MMT_OK;
}

extern "C" int mmt_layernorm_fwd(const void* x, int x_dtype, int64_t ldx, int B, int D,
                                 const float* gamma, const float* beta, float eps, void* y,
                                 int64_t ldy, float* mean, float* rstd, mmt_stream_t stream) {
  MMT_CHECK_ARG(x && gamma && beta && y && mean && rstd, "mmt_layernorm_fwd: null pointer");
  MMT_CHECK_ARG(is_dt(x_dtype), "mmt_layernorm_fwd: x_dtype %d", x_dtype);
  MMT_CHECK_ARG(B > 0 && D > 0 && D % 8 == 0 && ldx >= D && ldx % 8 == 0 && ldy >= D && ldy % 8 == 0,
                "mmt_layernorm_fwd: B %d, D %d (positive, D %% 8 == 0), row strides >= D and "
                "multiples of 8", B, D);
  MMT_CHECK_ARG(al16(x) && al16(y) && al16(gamma) && al16(beta),
                "mmt_layernorm_fwd: x, y, gamma and beta must be 16-B aligned");
  const dim3 grid((B + LN_ROWS - 1) / LN_ROWS), block(64 * LN_ROWS);
  if (x_dtype == MMT_F32)
    hipLaunchKernelGGL(layernorm_fwd_kernel<float>, grid, block, 0, as_stream(stream),
                       (const float*)x, ldx, B, D, gamma, beta, eps, (bf16_t*)y, ldy, mean, rstd);
  else
    hipLaunchKernelGGL(layernorm_fwd_kernel<bf16_t>, grid, block, 0, as_stream(stream),
                       (const bf16_t*)x, ldx, B, D, gamma, beta, eps, (bf16_t*)y, ldy, mean, rstd);
  MMT_CHECK_LAUNCH("mmt_layernorm_fwd");
  return MMT_OK;
}

extern "C" int mmt_layernorm_bwd(const void* dy, int dy_dtype, int64_t ld_dy, const void* x,
                                 int x_dtype, int64_t ldx, int B, int D, const float* mean,
                                 const float* rstd, const float* gamma, const void* addend,
                                 int64_t ld_add, void* dx, int64_t ld_dx, float* dyxhat,
                                 mmt_stream_t stream) {
  MMT_CHECK_ARG(dy && x && mean && rstd && gamma && dx && dyxhat, "mmt_layernorm_bwd: null pointer");
  MMT_CHECK_ARG(is_dt(dy_dtype) && is_dt(x_dtype), "mmt_layernorm_bwd: dtypes %d, %d", dy_dtype,
                x_dtype);
  MMT_CHECK_ARG(B > 0 && D > 0 && D % 8 == 0 && ld_dy >= D && ld_dy % 8 == 0 && ldx >= D &&
                    ldx % 8 == 0 && ld_dx >= D && ld_dx % 8 == 0 &&
                    (!addend || (ld_add >= D && ld_add % 8 == 0)),
                "mmt_layernorm_bwd: B %d, D %d (positive, D %% 8 == 0), row strides >= D and "
                "multiples of 8", B, D);
  MMT_CHECK_ARG(al16(dy) && al16(x) && al16(gamma) && al16(addend) && al16(dx) && al16(dyxhat),
                "mmt_layernorm_bwd: dy, x, gamma, addend, dx and dyxhat must be 16-B aligned");
  const dim3 grid((B + LN_ROWS - 1) / LN_ROWS), block(64 * LN_ROWS);
  hipStream_t s = as_stream(stream);
#define LNB(TDY, TX)                                                                              \
  hipLaunchKernelGGL((layernorm_bwd_kernel<TDY, TX>), grid, block, 0, s, (const TDY*)dy, ld_dy,   \
                     (const TX*)x, ldx, B, D, mean, rstd, gamma, (const TX*)addend, ld_add,       \
                     (TX*)dx, ld_dx, dyxhat)
  if (dy_dtype == MMT_F32 && x_dtype == MMT_F32) LNB(float, float);
  else if (dy_dtype == MMT_BF16 && x_dtype == MMT_F32) LNB(bf16_t, float);
  else if (dy_dtype == MMT_F32 && x_dtype == MMT_BF16) LNB(float, bf16_t);
  else LNB(bf16_t, bf16_t);
#undef LNB
  MMT_CHECK_LAUNCH("mmt_layernorm_bwd");
  return MMT_OK;
}
