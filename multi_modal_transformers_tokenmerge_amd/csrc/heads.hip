// Continuous and categorical action heads for gfx950 with action chunks, a pad mask and decoding
// (include/mmt_api.h mmt_head_continuous, mmt_head_categorical, mmt_head_categorical_decode).
// The reference heads (multi_modal_transformers/action_heads/continuous.py:19-26,
// categorical.py:12-40) and their losses (models/octo/octo.py:167-198, :262, :302) predict one
// action; the chunk axis they already carry (`seq` of continuous.py:24, `action` of
// categorical.py:32-36) takes its general value h here. action_head_kernel (glue.hip) stays the
// path of h = 1, no mask, squared error.
//
// Form: one wave per row, four rows per 256-thread workgroup (action_head_kernel's). Launches of a
// loss entry: (1) one workgroup counts the mask's ones into scratch[0] (integer adds; the element
// count without a mask); (2) the row kernel: forward, the row's fp32 loss partial (scratch[1 + r])
// and dz scaled by the normaliser from the count; (3) one workgroup adds the partials in a fixed
// order (head_loss_sum_kernel) and applies the normaliser. No float atomics, no host
// synchronisation: two calls on the same inputs agree bit for bit, and the step stays capturable.
//
// Rounding: everything is fp32 (tanhf / expf / logf of the device library); the only bf16
// rounding is the store of dz.
#include <math.h>

#include "common.h"

using namespace mmt;

namespace {

constexpr int HD_NT = 256;       // 4 waves = 4 rows per workgroup
constexpr int HD_MAXW = 4096;    // continuous width h A
constexpr int HD_MAXN = 1024;    // categorical classes
constexpr int HD_MAXRUN = HD_MAXN / 64;  // classes per lane of the decode scan

// sum of the mask's n bytes (each counted as 0 / 1; n itself without a mask): integer adds, so
// any order gives the same (launch_mask_count, common.h: the diffusion loss counts with it too)
__global__ __launch_bounds__(HD_NT) void mask_count_kernel(const uint8_t* __restrict__ m, int64_t n,
                                                           uint32_t* __restrict__ count) {
  __shared__ uint32_t red[HD_NT / 64];
  if (!m) {
    if (threadIdx.x == 0) count[0] = (uint32_t)n;
    return;
  }
  uint32_t s = 0;
  for (int64_t i = threadIdx.x; i < n; i += HD_NT) s += m[i] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) count[0] = red[0] + red[1] + red[2] + red[3];
}

// loss[0] = width / max(count, 1) * sum(part[0 .. n)): thread t adds part[t], part[t + 256], ...
// in ascending order, then the 256 sums are folded in halves (s[t] += s[t + 128], 64, ... 1)
__global__ __launch_bounds__(HD_NT) void head_loss_sum_kernel(const float* __restrict__ part, int n,
                                                              float width,
                                                              const uint32_t* __restrict__ count,
                                                              float* __restrict__ loss) {
  __shared__ float buf[HD_NT];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += HD_NT) s += part[i];
  buf[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int o = HD_NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) buf[threadIdx.x] += buf[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint32_t c = count[0];
    loss[0] = buf[0] * (width / (float)(c > 0u ? c : 1u));
  }
}

// Row b = one sample's chunk of W = h A components. L1: |p - y| in place of (p - y)^2.
template <bool L1>
__global__ __launch_bounds__(HD_NT) void head_continuous_kernel(
    const float* __restrict__ z, int64_t ldz, int B, int W, float width, const float* __restrict__ y,
    const uint8_t* __restrict__ mask, float max_action, const uint32_t* __restrict__ count,
    float* __restrict__ pred, float* __restrict__ part, bf16_t* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (HD_NT / 64) + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* const zr = z + (int64_t)r * ldz;
  const int64_t o = (int64_t)r * W;
  float norm = 0.f;
  if (y) {
    const uint32_t c = count[0];
    norm = width / (float)(c > 0u ? c : 1u);
  }
  float row_loss = 0.f;
  for (int a = lane; a < W; a += 64) {
    const float th = tanhf(zr[a] / max_action);
    const float p = th * max_action;
    if (pred) pred[o + a] = p;
    if (y) {
      const float m = mask ? (mask[o + a] ? 1.f : 0.f) : 1.f;
      const float d = p - y[o + a];
      float e, de;
      if (L1) {
        e = fabsf(d);
        de = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      } else {
        e = d * d;
        de = 2.f * d;
      }
      row_loss += m * e;
      dz[o + a] = f2bf(m * de * (1.f - th * th) * norm);
    }
  }
  if (!y) return;
  row_loss = wave_sum(row_loss);
  if (lane == 0) part[r] = row_loss;
}

// (value, index) argmax over the wave, the smaller index on equal values
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

// Row r = one (sample, step, component) group's N logits.
__global__ __launch_bounds__(HD_NT) void head_categorical_kernel(
    const float* __restrict__ z, int64_t ldz, int R, int N, const float* __restrict__ y,
    const uint8_t* __restrict__ mask, const float* __restrict__ edges, int n_edges,
    const uint32_t* __restrict__ count, float* __restrict__ part, bf16_t* __restrict__ dz,
    int32_t* __restrict__ cls) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (HD_NT / 64) + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* const zr = z + (int64_t)r * ldz;
  // classes lane, lane + 64, ... ascending: a strict > keeps the lane's first maximum
  float mx = -INFINITY;
  int arg = 0x7fffffff;
  for (int c = lane; c < N; c += 64) {
    const float v = zr[c];
    if (v > mx || arg == 0x7fffffff) {
      mx = v;
      arg = c;
    }
  }
  wave_argmax(mx, arg);
  if (cls && lane == 0) cls[r] = arg;

  const float yv = y[r];
  int bin = 0;  // #edges <= y (jnp.digitize)
  for (int i = lane; i < n_edges; i += 64) bin += edges[i] <= yv ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bin += __shfl_xor(bin, o, 64);
  const float has = bin < N ? 1.f : 0.f;
  const float m = mask ? (mask[r] ? 1.f : 0.f) : 1.f;
  const uint32_t cnt = count[0];
  const float norm = 1.f / (float)(cnt > 0u ? cnt : 1u);
  float se = 0.f;
  for (int c = lane; c < N; c += 64) se += expf(zr[c] - mx);
  se = wave_sum(se);
  const float lse = mx + logf(se);
  const float g = m * norm;
  for (int c = lane; c < N; c += 64) {
    const float lab = (c == bin) ? 1.f : 0.f;
    dz[(int64_t)r * N + c] = f2bf((has * expf(zr[c] - lse) - lab) * g);
  }
  if (lane == 0) part[r] = bin < N ? m * (lse - zr[bin]) : 0.f;
}

// Row r: argmax, or one inverse-CDF draw from softmax(z / T). Lane l holds the contiguous classes
// [l per, (l + 1) per), per = ceil(N / 64) <= 16.
__global__ __launch_bounds__(HD_NT) void head_categorical_decode_kernel(
    const float* __restrict__ z, int64_t ldz, int R, int N, int G, const float* __restrict__ values,
    int mode, float inv_t, const uint32_t* __restrict__ rng, int64_t sample_offset,
    int32_t* __restrict__ cls, float* __restrict__ actions) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (HD_NT / 64) + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* const zr = z + (int64_t)r * ldz;
  const int per = (N + 63) / 64;
  const int c0 = lane * per;
  float zv[HD_MAXRUN];
  float mx = -INFINITY;
  int arg = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < HD_MAXRUN; ++k) {
    const int c = c0 + k;
    const bool live = k < per && c < N;
    zv[k] = live ? zr[c] : -INFINITY;
    if (live && (zv[k] > mx || arg == 0x7fffffff)) {
      mx = zv[k];
      arg = c;
    }
  }
  wave_argmax(mx, arg);
  int pick = arg;
  if (mode == MMT_DECODE_SAMPLE) {
    // the lane's run in ascending order; classes past N add exp(-inf) = 0
    float run = 0.f;
#pragma unroll
    for (int k = 0; k < HD_MAXRUN; ++k) {
      zv[k] = expf((zv[k] - mx) * inv_t);
      run += zv[k];
    }
    float incl = run;  // inclusive scan over the lanes (Hillis-Steele, 6 steps)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const float total = __shfl(incl, 63, 64);
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    const uint32_t key = stream_key(rng[0], rng[1], 0xFFF8u, 1);
    const uint32_t ctr = (uint32_t)(sample_offset * (int64_t)G + r);
    const float u = ((float)(draw_u32(key, ctr) >> 8) + 0.5f) * (1.f / 16777216.f);
    const float thr = u * total;  // CDF(c) > u as prefix(c) > u total
    int cand = 0x7fffffff;
    float cum = excl;
#pragma unroll
    for (int k = 0; k < HD_MAXRUN; ++k) {
      cum += zv[k];
      const int c = c0 + k;
      if (k < per && c < N && cum > thr && cand == 0x7fffffff) cand = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    pick = cand < N ? cand : N - 1;
  }
  if (lane == 0) {
    cls[r] = pick;
    actions[r] = values[pick];
  }
}

}  // namespace

void mmt::launch_mask_count(const uint8_t* mask, int64_t n, uint32_t* count, hipStream_t s) {
  hipLaunchKernelGGL(mask_count_kernel, dim3(1), dim3(HD_NT), 0, s, mask, n, count);
}

extern "C" int mmt_head_continuous(const float* z, int64_t ldz, int B, int h, int A, const float* y,
                                   const uint8_t* mask, int loss_kind, float max_action,
                                   float* pred, float* scratch, float* loss, void* dz,
                                   mmt_stream_t stream) {
  MMT_CHECK_ARG(z && B > 0, "mmt_head_continuous: args");
  MMT_CHECK_ARG(h >= 1 && A >= 1 && (int64_t)h * A <= HD_MAXW,
                "mmt_head_continuous: width h A = %d x %d not in [1, %d]", h, A, HD_MAXW);
  const int W = h * A;
  MMT_CHECK_ARG(ldz >= W, "mmt_head_continuous: ldz %lld < width %d", (long long)ldz, W);
  MMT_CHECK_ARG(max_action > 0.f, "mmt_head_continuous: max_action must be > 0");
  MMT_CHECK_ARG(loss_kind == MMT_HEAD_LOSS_MSE || loss_kind == MMT_HEAD_LOSS_L1,
                "mmt_head_continuous: loss_kind %d is neither MSE (0) nor L1 (1)", loss_kind);
  MMT_CHECK_ARG(y || !mask, "mmt_head_continuous: a mask needs targets");
  MMT_CHECK_ARG(y ? (scratch && loss && dz) : pred != nullptr,
                "mmt_head_continuous: a loss needs scratch, loss and dz; a forward needs pred");
  MMT_CHECK_ARG((int64_t)B * W <= 0x7fffffff, "mmt_head_continuous: B h A must fit an int");
  hipStream_t s = as_stream(stream);
  uint32_t* const count = reinterpret_cast<uint32_t*>(scratch);
  if (y) {
    launch_mask_count(mask, (int64_t)B * W, count, s);
    MMT_CHECK_LAUNCH("mmt_head_continuous");
  }
  const dim3 grid((B + HD_NT / 64 - 1) / (HD_NT / 64));
  float* const part = y ? scratch + 1 : nullptr;
  if (loss_kind == MMT_HEAD_LOSS_L1)
    hipLaunchKernelGGL((head_continuous_kernel<true>), grid, dim3(HD_NT), 0, s, z, ldz, B, W,
                       (float)A, y, mask, max_action, count, pred, part, (bf16_t*)dz);
  else
    hipLaunchKernelGGL((head_continuous_kernel<false>), grid, dim3(HD_NT), 0, s, z, ldz, B, W,
                       (float)A, y, mask, max_action, count, pred, part, (bf16_t*)dz);
  MMT_CHECK_LAUNCH("mmt_head_continuous");
  if (y) {
    hipLaunchKernelGGL(head_loss_sum_kernel, dim3(1), dim3(HD_NT), 0, s, part, B, (float)A, count,
                       loss);
    MMT_CHECK_LAUNCH("mmt_head_continuous");
  }
  return MMT_OK;
}

extern "C" int mmt_head_categorical(const float* z, int64_t ldz, int R, int N, const float* y,
                                    const uint8_t* mask, const float* edges, int n_edges,
                                    float* scratch, float* loss, void* dz, int32_t* cls,
                                    mmt_stream_t stream) {
  MMT_CHECK_ARG(z && R > 0 && scratch && loss && dz, "mmt_head_categorical: args");
  MMT_CHECK_ARG(N >= 2 && N <= HD_MAXN, "mmt_head_categorical: %d classes not in [2, %d]", N,
                HD_MAXN);
  MMT_CHECK_ARG(ldz >= N, "mmt_head_categorical: ldz %lld < classes %d", (long long)ldz, N);
  MMT_CHECK_ARG(y && edges && n_edges > 1, "mmt_head_categorical: the loss needs targets and edges");
  MMT_CHECK_ARG((int64_t)R * N <= 0x7fffffff, "mmt_head_categorical: R N must fit an int");
  hipStream_t s = as_stream(stream);
  uint32_t* const count = reinterpret_cast<uint32_t*>(scratch);
  launch_mask_count(mask, (int64_t)R, count, s);
  MMT_CHECK_LAUNCH("mmt_head_categorical");
  float* const part = scratch + 1;
  hipLaunchKernelGGL(head_categorical_kernel, dim3((R + HD_NT / 64 - 1) / (HD_NT / 64)),
                     dim3(HD_NT), 0, s, z, ldz, R, N, y, mask, edges, n_edges, count, part,
                     (bf16_t*)dz, cls);
  MMT_CHECK_LAUNCH("mmt_head_categorical");
  hipLaunchKernelGGL(head_loss_sum_kernel, dim3(1), dim3(HD_NT), 0, s, part, R, 1.f, count, loss);
  MMT_CHECK_LAUNCH("mmt_head_categorical");
  return MMT_OK;
}

extern "C" int mmt_head_categorical_decode(const float* z, int64_t ldz, int R, int N, int G,
                                           const float* values, int mode, float temperature,
                                           const uint32_t* rng, int64_t sample_offset,
                                           int32_t* cls, float* actions, mmt_stream_t stream) {
  MMT_CHECK_ARG(z && values && cls && actions && R > 0, "mmt_head_categorical_decode: args");
  MMT_CHECK_ARG(N >= 2 && N <= HD_MAXN, "mmt_head_categorical_decode: %d classes not in [2, %d]", N,
                HD_MAXN);
  MMT_CHECK_ARG(ldz >= N, "mmt_head_categorical_decode: ldz %lld < classes %d", (long long)ldz, N);
  MMT_CHECK_ARG(mode == MMT_DECODE_ARGMAX || mode == MMT_DECODE_SAMPLE,
                "mmt_head_categorical_decode: mode %d is neither argmax (0) nor sample (1)", mode);
  MMT_CHECK_ARG(temperature > 0.f && temperature < INFINITY,
                "mmt_head_categorical_decode: temperature %g must be a finite value > 0",
                (double)temperature);
  if (mode == MMT_DECODE_SAMPLE) {
    MMT_CHECK_ARG(rng != nullptr, "mmt_head_categorical_decode: sampling needs rng");
    MMT_CHECK_ARG(G >= 1 && R % G == 0 && sample_offset >= 0,
                  "mmt_head_categorical_decode: %d rows are no multiple of %d groups per sample", R,
                  G);
  }
  hipLaunchKernelGGL(head_categorical_decode_kernel, dim3((R + HD_NT / 64 - 1) / (HD_NT / 64)),
                     dim3(HD_NT), 0, as_stream(stream), z, ldz, R, N, G, values, mode,
                     mode == MMT_DECODE_SAMPLE ? 1.f / temperature : 1.f, rng, sample_offset, cls,
                     actions);
  MMT_CHECK_LAUNCH("mmt_head_categorical_decode");
  return MMT_OK;
}
