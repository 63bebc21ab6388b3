// Multi-draw diffusion loss for gfx950: DiffusionActionHead.denoise_loss (reference
// multi_modal_transformers/action_heads/diffusion.py:110-143) with K independent (t, eps) draws
// per sample and a pad mask over the action components, forward and the head's backward operands
// in one fused launch (mmt_diffusion_loss_multi), plus the segment sum of the hidden gradient over
// the diffusion steps (mmt_diffusion_loss_dq).
//
// As in the sampler (sampler.hip) the denoiser's first Dense is split along its input,
//   W1 [noisy | temb_t | r] + b1 = W1x noisy + Q[t] + P[b],
// with P (B, H) and Q (steps, H) plain GEMMs of the caller: the time encoder costs `steps` rows and
// the readout product B rows whatever K is, and only this kernel scales with K. Per sample b and
// draw k:
//   t = t_in[k, b] or U{0..steps-1};  eps = eps_in[k, b] or N(0, 1) (Box-Muller, as
//   diffusion_prep_kernel);  noisy = sqrt(abar_t) a_b + sqrt(1 - abar_t) eps
//   pre = W1x noisy + Q[t] + P[b];  h = relu(pre);  pred = W2 h + b2;  d = pred - eps
//   loss  = A / (K max(sum m, 1)) sum_{k,b,j} m[b,j] 0.5 d[k,b,j]^2
//   dpred = grad_scale A / (K max(sum m, 1)) m d;  dh = (W2^T dpred) [pre > 0];  dP[b] = sum_k dh
//
// Launches of the entry: (1) one workgroup counts the mask's ones into scratch[0] (integer adds;
// B A without a mask); (2) the fused kernel on the wave-per-sample denoiser core of
// denoiser_wave.h (its layout, LDS budget and lane reduction), with the loop over the K draws where
// the sampler loops over its steps; (3) one workgroup adds the B per-sample loss partials
// (scratch[1 + b]) in ascending order. No float atomics: a sample belongs to one wave, every sum
// has a fixed order, two calls on the same inputs agree bit for bit.
//
// Kernel forms (mmt_diffusion_loss_last_route; MMT_DIFFUSION_LOSS_ROUTE_NONE after a call rejected
// before its launch): _LDS while the weights fit the core's LDS budget (dw::fits_lds), else
// _STREAM. The Q[t] slots of the wave's LDS rows are reused for the pre-activations.
//
// Rounding model: all forward arithmetic is fp32 on exactly widened bf16 weights (as the
// sampler). The only bf16 roundings are the five backward outputs noisy, h, dh, dpred (rows
// k B + b) and dP; dP is accumulated over the draws in fp32 registers from the unrounded dh and
// rounded once.
//
// Random streams: draw 0 uses the training keys of mmt_diffusion_prep (t: stream_key(seed, step,
// 0xFFFE, 1) at counter g; eps: site 2 at counter g A + j; g = sample_offset + b), so K = 1
// reproduces its draws bit for bit. Draw k >= 1 uses layer word 0xFFF9 (no other stream does:
// 0xFFFA .. 0xFFFE are the head's and the sampler's, 0xFFFF the stem's) with site 2 k for t and
// 2 k + 1 for eps at the same counters.
#include <math.h>

#include "denoiser_wave.h"

using namespace mmt;

namespace {

constexpr int DL_MAXK = 64;

// keys of draw k: k = 0 the training streams of mmt_diffusion_prep, k >= 1 layer 0xFFF9
__device__ __forceinline__ uint32_t dl_t_key(uint32_t seed, uint32_t step, int k) {
  return k == 0 ? stream_key(seed, step, 0xFFFEu, 1) : stream_key(seed, step, 0xFFF9u, 2u * k);
}
__device__ __forceinline__ uint32_t dl_eps_key(uint32_t seed, uint32_t step, int k) {
  return k == 0 ? stream_key(seed, step, 0xFFFEu, 2) : stream_key(seed, step, 0xFFF9u, 2u * k + 1u);
}

struct LossArgs {
  const uint32_t* rng;
  int B, K, steps, H;
  int64_t sample_offset;
  const float* actions;
  const uint8_t* pad_mask;
  const float* alpha_hats;
  const float* P;
  int64_t ld_p;
  const float* Q;
  int64_t ld_q;
  const bf16_t* w1;
  int64_t ld_w1;
  const bf16_t* w2;
  const float* b2;
  const int32_t* t_in;
  const float* eps_in;
  float grad_scale;
  const uint32_t* count;  // scratch[0]: sum of the mask
  float* part;            // scratch[1 ..]: per-sample loss partials
  int32_t* t_out;
  float* eps_out;
  bf16_t* noisy;
  bf16_t* h;
  bf16_t* dh;
  bf16_t* dpred;
  bf16_t* dP;
  unsigned int* fault;
};

// loss[0] = A / (K max(count, 1)) * (part[0] + part[1] + ... + part[B-1]), added in that order
__global__ __launch_bounds__(dw::NT) void loss_sum_kernel(const float* __restrict__ part, int B,
                                                         float A_over_K,
                                                         const uint32_t* __restrict__ count,
                                                         float* __restrict__ loss) {
  __shared__ float buf[dw::NT];
  float s = 0.f;
  for (int b0 = 0; b0 < B; b0 += dw::NT) {
    const int n = min(dw::NT, B - b0);
    if ((int)threadIdx.x < n) buf[threadIdx.x] = part[b0 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < n; ++i) s += buf[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint32_t c = count[0];
    loss[0] = s * (A_over_K / (float)(c > 0u ? c : 1u));
  }
}

template <int A8, bool LDSW>
__global__ __launch_bounds__(dw::NT) void diffusion_loss_multi_kernel(const LossArgs p) {
  constexpr int A = 8 * A8;
  const int H = p.H, nu = (H + 63) / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const dw::Lds s = dw::carve<A8>(H, nu, wave);  // s.hq: Q[t] of my units, then their pre
  if (LDSW) dw::stage_weights<A8>(s, p.w1, p.ld_w1, p.w2, H);
  const int b = blockIdx.x * (dw::NT / 64) + wave;
  if (b >= p.B) return;  // wave-uniform, after the only barrier

  const int64_t gsample = p.sample_offset + b;
  const dw::Lanes<A8> L(lane, gsample);
  const int sub = L.sub, a0 = L.a0;
  const bool bwd = p.dP != nullptr;

  float act[A8], msk[A8], b2r[A8];
#pragma unroll
  for (int i = 0; i < A8; ++i) {
    act[i] = p.actions[(int64_t)b * A + a0 + i];
    msk[i] = p.pad_mask ? (p.pad_mask[(int64_t)b * A + a0 + i] ? 1.f : 0.f) : 1.f;
    b2r[i] = p.b2[a0 + i];
  }
  const uint32_t cnt = p.count[0];
  // A / (K max(sum m, 1)): the loss's normaliser, applied to the partials' sum by loss_sum_kernel
  const float norm = (float)A / ((float)p.K * (float)(cnt > 0u ? cnt : 1u));
  const float gscale = p.grad_scale * norm;

  dw::park_p(s.hp, p.P + (int64_t)b * p.ld_p, H, nu, lane);

  float dp[dw::MAXNU];  // dP[b] of my units, summed over the draws
#pragma unroll
  for (int u = 0; u < dw::MAXNU; ++u) dp[u] = 0.f;
  float loss_acc = 0.f;

#pragma unroll 1
  for (int k = 0; k < p.K; ++k) {
    const int64_t row = (int64_t)k * p.B + b;
    int t;
    if (p.t_in) {
      t = p.t_in[row];
    } else {
      const uint32_t key = dl_t_key(p.rng[0], p.rng[1], k);
      t = (int)(((uint64_t)draw_u32(key, (uint32_t)gsample) * (uint32_t)p.steps) >> 32);
    }
    t = dw::checked_row(t, p.steps, lane, p.fault);
    {  // Q[t] of my units: all loads issued together, then parked
      float qn[dw::MAXNU];
      dw::load_units(p.Q + (int64_t)t * p.ld_q, H, lane, qn);
      dw::park_units(s.hq, qn, nu, lane);
    }

    float eps[A8], x[A8];
    if (p.eps_in) {
#pragma unroll
      for (int i = 0; i < A8; ++i) eps[i] = p.eps_in[row * A + a0 + i];
    } else {
      L.spread(normal_draw(dl_eps_key(p.rng[0], p.rng[1], k), L.ctr), eps);
    }
    const float ah = p.alpha_hats[t];
    const float c1 = sqrtf(ah), c2 = sqrtf(1.f - ah);
#pragma unroll
    for (int i = 0; i < A8; ++i) x[i] = c1 * act[i] + c2 * eps[i];
    if (sub == 0) {
      if (lane == 0) p.t_out[row] = t;
#pragma unroll
      for (int i = 0; i < A8; ++i) {
        if (p.eps_out) p.eps_out[row * A + a0 + i] = eps[i];
        if (bwd) p.noisy[row * A + a0 + i] = f2bf(x[i]);
      }
    }

    float xb[A];  // noisy as wave-uniform values
    dw::broadcast<A8>(x, xb);

    float e[A];
#pragma unroll
    for (int a = 0; a < A; ++a) e[a] = 0.f;
#pragma unroll 1
    for (int u = 0; u < nu; ++u) {
      const int j = lane + 64 * u;
      const bool live = j < H;
      const int jj = live ? j : H - 1;  // clamped, its hidden value zeroed below
      float pre = s.hp[64 * u + lane] + s.hq[64 * u + lane];
      pre = dw::row_dot<A8>(dw::w1_row<A8, LDSW>(s, p.w1, p.ld_w1, jj), xb, pre);
      s.hq[64 * u + lane] = pre;  // parked for the backward pass's gate
      const float hv = live ? fmaxf(pre, 0.f) : 0.f;
      if (bwd && live) p.h[row * H + j] = f2bf(hv);
      dw::w2_accumulate<A8, LDSW>(s, p.w2, H, jj, hv, e);
    }
    dw::reduce<A8>(e, lane);

    float dpr[A8], lk = 0.f;
#pragma unroll
    for (int i = 0; i < A8; ++i) {
      const float d = e[i] + b2r[i] - eps[i];
      lk += msk[i] * 0.5f * d * d;
      dpr[i] = gscale * msk[i] * d;
    }
    // the 8 lane groups hold distinct components: a butterfly over lane bits 3 .. 5 adds them
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) lk += __shfl_xor(lk, o, 64);
    loss_acc += lk;
    if (!bwd) continue;

    if (sub == 0) {
#pragma unroll
      for (int i = 0; i < A8; ++i) p.dpred[row * A + a0 + i] = f2bf(dpr[i]);
    }
    float db[A];  // dpred as wave-uniform values
    dw::broadcast<A8>(dpr, db);
    // dh of unit lane + 64 u: its W2 column against dpred, gated by the sign of the parked pre
    auto unit_dh = [&](int u) {
      const int j = lane + 64 * u;
      const bool live = j < H;
      const int jj = live ? j : H - 1;
      float g = 0.f;
      if (LDSW) {
        g = dw::row_dot<A8>(dw::w2_row<A8>(s, jj), db, g);
      } else {
#pragma unroll
        for (int a = 0; a < A; ++a) g = fmaf(db[a], bf2f(p.w2[(int64_t)a * H + jj]), g);
      }
      g = (live && s.hq[64 * u + lane] > 0.f) ? g : 0.f;
      if (live) p.dh[row * H + j] = f2bf(g);
      return g;
    };
    if (LDSW) {  // unrolled: dp[u] is a register
#pragma unroll
      for (int u = 0; u < dw::MAXNU; ++u)
        if (u < nu) dp[u] += unit_dh(u);  // wave-uniform
    } else {
      // streamed weights: a rolled loop (unrolled, the A global loads of all 16 units are hoisted
      // together and spill); dp[u] is reached by a select chain, 16 of the unit's 2 A + 16 ops
#pragma unroll 1
      for (int u = 0; u < nu; ++u) {
        const float g = unit_dh(u);
#pragma unroll
        for (int v = 0; v < dw::MAXNU; ++v) dp[v] += v == u ? g : 0.f;
      }
    }
  }

  if (lane == 0) p.part[b] = loss_acc;
  if (bwd) {
#pragma unroll
    for (int u = 0; u < dw::MAXNU; ++u) {
      const int j = lane + 64 * u;
      if (u < nu && j < H) p.dP[(int64_t)b * H + j] = f2bf(dp[u]);
    }
  }
}

// dQ[t][c] = sum over the rows r (ascending) with t_rows[r] == t of dh[r][c]: one workgroup (one
// wave) per (t, 64-column block), one column per lane, no atomics. The rows are walked in tiles of
// DQ_TILE: the wave reads the tile's t values (16 independent loads per lane), ballots the matches
// into an ascending row list in LDS, then adds the listed dh rows in that order, eight loads in
// flight at a time (a plain row-by-row scan is one dependent load and branch per row: 207 us
// against the fused kernel's 72 us at K B = 4096).
constexpr int DQ_TILE = 1024;
__global__ __launch_bounds__(64) void diffusion_loss_dq_kernel(const int32_t* __restrict__ t_rows,
                                                               const bf16_t* __restrict__ dh,
                                                               int64_t ld_dh, int rows, int H,
                                                               float* __restrict__ dQ,
                                                               int64_t ld_dq) {
  __shared__ int list[DQ_TILE];
  const int t = blockIdx.x, lane = threadIdx.x, c = blockIdx.y * 64 + lane;
  const int cc = min(c, H - 1);  // lanes past H help with the list and drop their sum
  const uint64_t below = (1ull << lane) - 1ull;
  float s = 0.f;
  for (int r0 = 0; r0 < rows; r0 += DQ_TILE) {
    int tv[DQ_TILE / 64];
#pragma unroll
    for (int i = 0; i < DQ_TILE / 64; ++i) {
      const int r = r0 + 64 * i + lane;
      tv[i] = r < rows ? t_rows[r] : -1;  // -1 matches no step
    }
    int n = 0;  // wave-uniform
#pragma unroll
    for (int i = 0; i < DQ_TILE / 64; ++i) {
      const bool m = tv[i] == t;
      const uint64_t mask = __ballot(m);
      if (m) list[n + __popcll(mask & below)] = r0 + 64 * i + lane;
      n += __popcll(mask);
    }
    __syncthreads();
    int i = 0;
    for (; i + 8 <= n; i += 8) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = bf2f(dh[(int64_t)list[i + k] * ld_dh + cc]);
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; i < n; ++i) s += bf2f(dh[(int64_t)list[i] * ld_dh + cc]);
    __syncthreads();
  }
  if (c < H) dQ[(int64_t)t * ld_dq + c] = s;
}

int g_loss_route = MMT_DIFFUSION_LOSS_ROUTE_NONE;

struct LossKernel {
  template <int A8, bool LDSW>
  static auto kernel() { return diffusion_loss_multi_kernel<A8, LDSW>; }
};

}  // namespace

extern "C" int mmt_diffusion_loss_last_route(void) { return g_loss_route; }

extern "C" int mmt_diffusion_loss_multi(
    const uint32_t* rng, int B, int A, int K, int steps, int H, int64_t sample_offset,
    const float* actions, const uint8_t* pad_mask, const float* alpha_hats, const float* P,
    int64_t ld_p, const float* Q, int64_t ld_q, const void* w1, int64_t ld_w1, const void* w2,
    const float* b2, const int32_t* t_in, const float* eps_in, float grad_scale, float* scratch,
    float* loss, int32_t* t_out, float* eps_out, void* noisy, void* h, void* dh, void* dpred,
    void* dP, mmt_stream_t stream) {
  g_loss_route = MMT_DIFFUSION_LOSS_ROUTE_NONE;  // a call rejected before its launch reports none
  MMT_CHECK_ARG(actions && alpha_hats && P && Q && w1 && w2 && b2 && scratch && loss && t_out &&
                    B > 0,
                "mmt_diffusion_loss_multi: args");
  MMT_CHECK_ARG(A % 8 == 0 && A >= 8 && A <= 64,
                "mmt_diffusion_loss_multi: action width %d is not a multiple of 8 in [8, 64]", A);
  MMT_CHECK_ARG(H % 8 == 0 && H >= 8 && H <= 1024,
                "mmt_diffusion_loss_multi: hidden width %d is not a multiple of 8 in [8, 1024]", H);
  MMT_CHECK_ARG(K >= 1 && K <= DL_MAXK, "mmt_diffusion_loss_multi: K %d not in [1, %d]", K, DL_MAXK);
  MMT_CHECK_ARG(steps >= 1, "mmt_diffusion_loss_multi: steps %d < 1", steps);
  MMT_CHECK_ARG(rng || (t_in && eps_in),
                "mmt_diffusion_loss_multi: need rng or injected (t, eps)");
  MMT_CHECK_ARG(ld_p >= H && ld_q >= H && ld_w1 >= A, "mmt_diffusion_loss_multi: leading dims");
  MMT_CHECK_ARG(ld_w1 % 8 == 0 && ((uintptr_t)w1 & 15) == 0 && ((uintptr_t)w2 & 15) == 0,
                "mmt_diffusion_loss_multi: W1 rows and W2 must start on 16-B boundaries");
  const int n_bwd = (noisy != nullptr) + (h != nullptr) + (dh != nullptr) + (dpred != nullptr) +
                    (dP != nullptr);
  MMT_CHECK_ARG(n_bwd == 0 || n_bwd == 5,
                "mmt_diffusion_loss_multi: the five backward outputs are given together or not at all");
  MMT_CHECK_ARG((int64_t)B * A <= 0x7fffffff && (int64_t)K * B <= 0x7fffffff,
                "mmt_diffusion_loss_multi: B * A and K * B must fit an int");
  hipStream_t s = as_stream(stream);
  uint32_t* const count = reinterpret_cast<uint32_t*>(scratch);
  launch_mask_count(pad_mask, (int64_t)B * A, count, s);
  MMT_CHECK_LAUNCH("mmt_diffusion_loss_multi");
  LossArgs p{rng, B, K, steps, H, sample_offset, actions, pad_mask, alpha_hats, P, ld_p, Q, ld_q,
             (const bf16_t*)w1, ld_w1, (const bf16_t*)w2, b2, t_in, eps_in, grad_scale, count,
             scratch + 1, t_out, eps_out, (bf16_t*)noisy, (bf16_t*)h, (bf16_t*)dh, (bf16_t*)dpred,
             (bf16_t*)dP, fault_word()};
  const bool lds = dw::dispatch<LossKernel>(A, H, B, s, p);
  MMT_CHECK_LAUNCH("mmt_diffusion_loss_multi");
  hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(dw::NT), 0, s, scratch + 1, B,
                     (float)A / (float)K, count, loss);
  MMT_CHECK_LAUNCH("mmt_diffusion_loss_multi");
  g_loss_route = lds ? MMT_DIFFUSION_LOSS_ROUTE_LDS : MMT_DIFFUSION_LOSS_ROUTE_STREAM;
  return MMT_OK;
}

extern "C" int mmt_diffusion_loss_dq(const int32_t* t_rows, const void* dh, int64_t ld_dh, int rows,
                                     int steps, int H, float* dQ, int64_t ld_dq,
                                     mmt_stream_t stream) {
  MMT_CHECK_ARG(t_rows && dh && dQ && rows > 0 && steps > 0 && H > 0,
                "mmt_diffusion_loss_dq: args");
  MMT_CHECK_ARG(ld_dh >= H && ld_dq >= H, "mmt_diffusion_loss_dq: leading dims");
  hipLaunchKernelGGL(diffusion_loss_dq_kernel, dim3(steps, (H + 63) / 64), dim3(64), 0,
                     as_stream(stream), t_rows, (const bf16_t*)dh, ld_dh, rows, H, dQ, ld_dq);
  MMT_CHECK_LAUNCH("mmt_diffusion_loss_dq");
  return MMT_OK;
}
