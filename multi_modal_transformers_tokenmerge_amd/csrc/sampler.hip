// DDPM inference sampler for gfx950: DiffusionActionHead.predict_action
// (reference multi_modal_transformers/action_heads/diffusion.py:146-209) as ONE launch.
//
// The denoiser's first Dense acts on concatenate([noisy, time_emb, readout]) (OctoDenoise :61),
// so it splits along its input:
//   W1 [x | temb_t | r] + b1 = W1x x + (W1t temb_t + b1) + W1r r = W1x x + Q[t] + P[b]
// Q (steps, H) and P (B, H) are plain GEMMs issued by the host wrapper before this call (the
// library's MFMA GEMM); what remains per step and sample is an (H x 8) and an (8 x H)
// matrix-vector product, a ReLU and the update
//   x <- clip(c1_t (x - c2_t eps_hat) + c3_t z, -5, 5)                      (:182-188)
// This kernel runs all steps for a sample with its state in registers: one wave per sample, the
// H hidden units spread over the lanes (unit j = lane + 64 u), W1x rows and W2 columns of those
// units in registers, Q[t] read from L2 each step. eps_hat needs one wave reduction per action
// component per step; no LDS, no barriers, no global writes until the end.
//
// Reference quirks kept: z is drawn once per sample (:198-200) and, because the scan never splits
// the keys (:178, :190), reused as every step's noise; noise is added at t = 0 too; the action
// dimension is hard-coded to 8 (:200).
#include <math.h>

#include "denoiser_wave.h"

using namespace mmt;

namespace {

constexpr int SA = 8;     // action dimension (diffusion.py:200)
constexpr int SNT = 256;  // threads per workgroup: 4 samples

template <int NU>
__global__ __launch_bounds__(SNT) void diffusion_sample_kernel(
    const uint32_t* __restrict__ rng, int B, int steps, int64_t sample_offset,
    const float* __restrict__ P, int64_t ld_p, const float* __restrict__ Q, int64_t ld_q,
    const bf16_t* __restrict__ w1, int64_t ld_w1, const bf16_t* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ coef, const float* __restrict__ z_in,
    int H, float* __restrict__ actions, float* __restrict__ z_out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (SNT / 64) + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform: the whole wave leaves

  float w1x[NU][SA], w2c[NU][SA], pb[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int j = lane + 64 * u;
    const int jj = j < H ? j : H - 1;  // clamped, zeroed below
    const float keep = j < H ? 1.f : 0.f;
    const uint4 row = *reinterpret_cast<const uint4*>(w1 + (int64_t)jj * ld_w1);  // W1[j][0:8]
    const uint32_t rw[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w1x[u][2 * q] = keep * __uint_as_float(rw[q] << 16);
      w1x[u][2 * q + 1] = keep * __uint_as_float(rw[q] & 0xffff0000u);
    }
#pragma unroll
    for (int a = 0; a < SA; ++a) w2c[u][a] = keep * bf2f(w2[(int64_t)a * H + jj]);
    pb[u] = keep * P[(int64_t)b * ld_p + jj];
  }

  float z[SA], x[SA];
  if (z_in) {
#pragma unroll
    for (int a = 0; a < SA; ++a) z[a] = z_in[(int64_t)b * SA + a];
  } else {
    const uint32_t key = stream_key(rng[0], rng[1], 0xFFFEu, 3);
#pragma unroll
    for (int a = 0; a < SA; ++a) {
      const uint32_t c = (uint32_t)((sample_offset + b) * SA + a);
      z[a] = normal_draw(key, c);
    }
  }
#pragma unroll
  for (int a = 0; a < SA; ++a) x[a] = z[a];  // x_T = z

  float b2r[SA];
#pragma unroll
  for (int a = 0; a < SA; ++a) b2r[a] = b2[a];

#pragma unroll 1
  for (int t = steps - 1; t >= 0; --t) {
    const float* q = Q + (int64_t)t * ld_q;
    float e[SA];
#pragma unroll
    for (int a = 0; a < SA; ++a) e[a] = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int j = lane + 64 * u;
      float h = pb[u] + (j < H ? 1.f : 0.f) * q[j < H ? j : H - 1];
#pragma unroll
      for (int a = 0; a < SA; ++a) h = fmaf(x[a], w1x[u][a], h);
      h = fmaxf(h, 0.f);
#pragma unroll
      for (int a = 0; a < SA; ++a) e[a] = fmaf(h, w2c[u][a], e[a]);
    }
    const float c1 = coef[3 * t], c2 = coef[3 * t + 1], c3 = coef[3 * t + 2];
#pragma unroll
    for (int a = 0; a < SA; ++a) {
      const float eps = wave_sum(e[a]) + b2r[a];
      x[a] = fminf(fmaxf(c1 * (x[a] - c2 * eps) + c3 * z[a], -5.f), 5.f);
    }
  }

  if (lane < SA) {
    float xv = 0.f, zv = 0.f;
#pragma unroll
    for (int a = 0; a < SA; ++a)
      if (a == lane) {
        xv = x[a];
        zv = z[a];
      }
    actions[(int64_t)b * SA + lane] = xv;
    if (z_out) z_out[(int64_t)b * SA + lane] = zv;
  }
}

// ---------------------------------------------------------------- step-table sampler
// mmt_diffusion_sample_steps: K table rows x <- clip(a x + b eps_hat(x, t) + c n) in one launch,
// for any action width A = 8 .. 64, on the wave-per-sample denoiser core of denoiser_wave.h (the
// layout, the LDS and the streamed form of the weights, the lane reduction): lane l keeps its A8
// components of x, z and the step noise. What is written here is the walk over the table.
//
// Rounding model: fp32 operands throughout. The weights are the bf16 shadow, widened exactly;
// x, the hidden layer and every accumulation are fp32 (nothing is rounded to bf16).

// Key of step k's noise stream. stream_key keeps 8 bits of its site, so k is split: the site
// carries 16 + k % 240 (16 .. 255: clear of the head's sites 1 .. 3, the training draws and z) and
// the layer word steps down from 0xFFFE once per 240 steps (0xFFFD .. 0xFFFA up to k = 1023; no
// other stream uses those layers). Every k of a table gets a stream of its own; k < 240 is
// stream_key(seed, step, 0xFFFE, 16 + k).
__device__ __forceinline__ uint32_t step_noise_key(uint32_t seed, uint32_t step, int k) {
  return stream_key(seed, step, 0xFFFEu - (uint32_t)(k / 240), 16u + (uint32_t)(k % 240));
}

struct StepArgs {
  const uint32_t* rng;
  int B, n_steps, q_rows, H, flags;
  int64_t sample_offset;
  const float* P;
  int64_t ld_p;
  const float* Q;
  int64_t ld_q;
  const bf16_t* w1;
  int64_t ld_w1;
  const bf16_t* w2;
  const float* b2;
  const int32_t* step_t;
  const float* step_coef;
  float clip;
  const float* z_in;
  const float* noise_in;
  float* actions;
  float* z_out;
  float* noise_out;
  unsigned int* fault;
};

template <int A8, bool LDSW>
__global__ __launch_bounds__(dw::NT) void diffusion_sample_steps_kernel(const StepArgs p) {
  constexpr int A = 8 * A8;
  const int H = p.H, nu = (H + 63) / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const dw::Lds s = dw::carve<A8>(H, nu, wave);
  if (LDSW) dw::stage_weights<A8>(s, p.w1, p.ld_w1, p.w2, H);
  const int b = blockIdx.x * (dw::NT / 64) + wave;
  if (b >= p.B) return;  // wave-uniform, after the only barrier

  const dw::Lanes<A8> L(lane, p.sample_offset + b);
  const int sub = L.sub, a0 = L.a0;
  const bool fresh = (p.flags & MMT_SAMPLE_FRESH_NOISE) != 0;

  float x[A8], z[A8], nz[A8], b2r[A8];
  if (p.z_in) {
#pragma unroll
    for (int i = 0; i < A8; ++i) z[i] = p.z_in[(int64_t)b * A + a0 + i];
  } else {
    L.spread(normal_draw(stream_key(p.rng[0], p.rng[1], 0xFFFEu, 3), L.ctr), z);
  }
#pragma unroll
  for (int i = 0; i < A8; ++i) {
    x[i] = z[i];
    nz[i] = z[i];
    b2r[i] = p.b2[a0 + i];
  }
  if (p.z_out && sub == 0) {
#pragma unroll
    for (int i = 0; i < A8; ++i) p.z_out[(int64_t)b * A + a0 + i] = z[i];
  }

  // P[b] of this lane's units is parked in LDS once, Q[t_k] every step. The Q row, the table row
  // and the step index after it are fetched a step ahead with plain unconditional loads (clamped
  // addresses, nothing computed on them before the next step), so no step waits on memory. All
  // MAXNU loads are issued whatever nu is: a `u < nu` guard costs more than it saves, because
  // each guarded block ends in a wait for its own loads (32 steps at H = 384, launch alone:
  // 46.7 us as here, 53.8 us with a guard per unit, 48.9 us with one per four units, at A = 8;
  // 112.5 / 120.0 / 114.3 us at A = 32).
  dw::park_p(s.hp, p.P + (int64_t)b * p.ld_p, H, nu, lane);
  float qn[dw::MAXNU];
  auto load_q = [&](int t) {  // t raw: checked when its Q row is fetched
    t = dw::checked_row(t, p.q_rows, lane, p.fault);
    dw::load_units(p.Q + (int64_t)t * p.ld_q, H, lane, qn);
  };
  const int last = p.n_steps - 1;
  load_q(p.step_t[0]);
  int t_next = p.step_t[min(1, last)];
  float can = p.step_coef[0], cbn = p.step_coef[1], ccn = p.step_coef[2];

#pragma unroll 1
  for (int k = 0; k < p.n_steps; ++k) {
#pragma unroll
    for (int u = 0; u < dw::MAXNU; ++u)
      if (u < nu) s.hq[64 * u + lane] = qn[u];
    const float ca = can, cb = cbn, cc = ccn;
    {  // step k + 1's operands (the last step refetches its own)
      const int kn = min(k + 1, last);
      load_q(t_next);
      t_next = p.step_t[min(k + 2, last)];
      can = p.step_coef[3 * kn];
      cbn = p.step_coef[3 * kn + 1];
      ccn = p.step_coef[3 * kn + 2];
    }

    if (fresh) {
      if (p.noise_in) {
#pragma unroll
        for (int i = 0; i < A8; ++i) nz[i] = p.noise_in[((int64_t)k * p.B + b) * A + a0 + i];
      } else {
        L.spread(normal_draw(step_noise_key(p.rng[0], p.rng[1], k), L.ctr), nz);
      }
      if (p.noise_out && sub == 0) {
#pragma unroll
        for (int i = 0; i < A8; ++i) p.noise_out[((int64_t)k * p.B + b) * A + a0 + i] = nz[i];
      }
    }

    float xb[A];  // x as wave-uniform values
    dw::broadcast<A8>(x, xb);

    float e[A];
#pragma unroll
    for (int a = 0; a < A; ++a) e[a] = 0.f;
#pragma unroll 1
    for (int u = 0; u < nu; ++u) {
      const int j = lane + 64 * u;
      const bool live = j < H;
      const int jj = live ? j : H - 1;  // clamped, its hidden value zeroed below
      float h = s.hp[64 * u + lane] + s.hq[64 * u + lane];
      h = dw::row_dot<A8>(dw::w1_row<A8, LDSW>(s, p.w1, p.ld_w1, jj), xb, h);
      h = live ? fmaxf(h, 0.f) : 0.f;
      dw::w2_accumulate<A8, LDSW>(s, p.w2, H, jj, h, e);
    }
    // dw::reduce, written out, and the park of qn above not through dw::park_units: through the
    // helpers this kernel is scheduled with one more full vmcnt / lgkmcnt wait per step (launch
    // alone, 32 steps, H = 384, B = 1 / 64 / 512: 47.9 / 50.7 / 51.1 us against 47.2 / 49.6 /
    // 50.0 us as here at A = 8; 113.7 / 118.0 / 119.7 against 112.1 / 116.0 / 117.8 us at A = 32)
#pragma unroll
    for (int st = 0; st < 3; ++st) {
      const int o = 32 >> st, n = A >> (st + 1);
      const bool up = (lane & o) != 0;
#pragma unroll
      for (int i = 0; i < n; ++i) e[i] = dw::exchange(e[i], e[i + n], up, o);
    }
#pragma unroll
    for (int i = 0; i < A8; ++i) {
#pragma unroll
      for (int o = 4; o > 0; o >>= 1) e[i] += __shfl_xor(e[i], o, 64);
    }

#pragma unroll
    for (int i = 0; i < A8; ++i) {
      const float eps = e[i] + b2r[i];
      const float v = fmaf(cc, nz[i], fmaf(cb, eps, ca * x[i]));
      x[i] = fminf(fmaxf(v, -p.clip), p.clip);
    }
  }

  if (sub == 0) {
#pragma unroll
    for (int i = 0; i < A8; ++i) p.actions[(int64_t)b * A + a0 + i] = x[i];
  }
}

// MMT_SAMPLE_DRAWS_ONLY: z and the step noise a full call would use, one thread per (b, a), with
// the sampler kernel's own draw (same keys, counters and arithmetic) and nothing else.
__global__ __launch_bounds__(dw::NT) void diffusion_sample_draws_kernel(
    const uint32_t* __restrict__ rng, int B, int A, int n_steps, int64_t sample_offset,
    bool fresh, const float* __restrict__ z_in, const float* __restrict__ noise_in,
    float* __restrict__ z_out, float* __restrict__ noise_out) {
  const int idx = blockIdx.x * dw::NT + threadIdx.x;  // b * A + a
  if (idx >= B * A) return;
  const uint32_t ctr = (uint32_t)(sample_offset * A + idx);
  if (z_out)
    z_out[idx] = z_in ? z_in[idx] : normal_draw(stream_key(rng[0], rng[1], 0xFFFEu, 3), ctr);
  if (!fresh || !noise_out) return;
  for (int k = 0; k < n_steps; ++k) {
    const int64_t o = (int64_t)k * B * A + idx;
    noise_out[o] = noise_in ? noise_in[o] : normal_draw(step_noise_key(rng[0], rng[1], k), ctr);
  }
}

int g_sampler_route = MMT_SAMPLER_ROUTE_NONE;

struct StepKernel {
  template <int A8, bool LDSW>
  static auto kernel() { return diffusion_sample_steps_kernel<A8, LDSW>; }
};

}  // namespace

extern "C" int mmt_sampler_last_route(void) { return g_sampler_route; }

extern "C" int mmt_diffusion_sample_steps(const uint32_t* rng, int B, int A, int n_steps,
                                          int64_t sample_offset, const float* P, int64_t ld_p,
                                          const float* Q, int64_t ld_q, int q_rows, const void* w1,
                                          int64_t ld_w1, const void* w2, const float* b2,
                                          const int32_t* step_t, const float* step_coef, float clip,
                                          int flags, const float* z_in, const float* noise_in,
                                          int H, float* actions, float* z_out, float* noise_out,
                                          mmt_stream_t stream) {
  g_sampler_route = MMT_SAMPLER_ROUTE_NONE;  // a call rejected before its launch reports no kernel
  MMT_CHECK_ARG(B > 0, "mmt_diffusion_sample_steps: args");
  MMT_CHECK_ARG(A % 8 == 0 && A >= 8 && A <= 64,
                "mmt_diffusion_sample_steps: action width %d is not a multiple of 8 in [8, 64]", A);
  MMT_CHECK_ARG(n_steps >= 1 && n_steps <= 1024,
                "mmt_diffusion_sample_steps: n_steps %d not in [1, 1024]", n_steps);
  MMT_CHECK_ARG((flags & ~(MMT_SAMPLE_FRESH_NOISE | MMT_SAMPLE_DRAWS_ONLY)) == 0,
                "mmt_diffusion_sample_steps: flags");
  const bool fresh = (flags & MMT_SAMPLE_FRESH_NOISE) != 0;
  MMT_CHECK_ARG(z_in || rng, "mmt_diffusion_sample_steps: need rng or an injected initial sample");
  MMT_CHECK_ARG(!fresh || noise_in || rng,
                "mmt_diffusion_sample_steps: fresh noise needs rng or injected step noise");
  MMT_CHECK_ARG(fresh || (!noise_in && !noise_out),
                "mmt_diffusion_sample_steps: step noise buffers need MMT_SAMPLE_FRESH_NOISE");
  hipStream_t s = as_stream(stream);
  if (flags & MMT_SAMPLE_DRAWS_ONLY) {  // the draws alone: the denoiser's operands are not read
    MMT_CHECK_ARG(z_out || noise_out,
                  "mmt_diffusion_sample_steps: MMT_SAMPLE_DRAWS_ONLY needs z_out or noise_out");
    MMT_CHECK_ARG((int64_t)B * A <= 0x7fffffff,
                  "mmt_diffusion_sample_steps: MMT_SAMPLE_DRAWS_ONLY needs B * A to fit an int");
    hipLaunchKernelGGL(diffusion_sample_draws_kernel, dim3((B * A + dw::NT - 1) / dw::NT),
                       dim3(dw::NT), 0, s, rng, B, A, n_steps, sample_offset, fresh, z_in, noise_in,
                       z_out, noise_out);
    MMT_CHECK_LAUNCH("mmt_diffusion_sample_steps");
    g_sampler_route = MMT_SAMPLER_ROUTE_STEPS_DRAWS;
    return MMT_OK;
  }
  MMT_CHECK_ARG(P && Q && w1 && w2 && b2 && step_t && step_coef && actions,
                "mmt_diffusion_sample_steps: args");
  MMT_CHECK_ARG(H % 8 == 0 && H >= 8 && H <= 1024,
                "mmt_diffusion_sample_steps: hidden width %d is not a multiple of 8 in [8, 1024]", H);
  MMT_CHECK_ARG(q_rows >= 1, "mmt_diffusion_sample_steps: q_rows %d < 1", q_rows);
  MMT_CHECK_ARG(clip > 0.f, "mmt_diffusion_sample_steps: clip must be positive");
  MMT_CHECK_ARG(ld_p >= H && ld_q >= H && ld_w1 >= A, "mmt_diffusion_sample_steps: leading dims");
  MMT_CHECK_ARG(ld_w1 % 8 == 0 && ((uintptr_t)w1 & 15) == 0 && ((uintptr_t)w2 & 15) == 0,
                "mmt_diffusion_sample_steps: W1 rows and W2 must start on 16-B boundaries");
  StepArgs p{rng, B, n_steps, q_rows, H, flags, sample_offset, P, ld_p, Q, ld_q,
             (const bf16_t*)w1, ld_w1, (const bf16_t*)w2, b2, step_t, step_coef, clip, z_in,
             noise_in, actions, z_out, noise_out, fault_word()};
  const bool lds = dw::dispatch<StepKernel>(A, H, B, s, p);
  MMT_CHECK_LAUNCH("mmt_diffusion_sample_steps");
  g_sampler_route = lds ? MMT_SAMPLER_ROUTE_STEPS_LDS : MMT_SAMPLER_ROUTE_STEPS_STREAM;
  return MMT_OK;
}

extern "C" int mmt_diffusion_sample(const uint32_t* rng, int B, int A, int steps,
                                    int64_t sample_offset, const float* P, int64_t ld_p,
                                    const float* Q, int64_t ld_q, const void* w1, int64_t ld_w1,
                                    const void* w2, const float* b2, const float* coef,
                                    const float* z_in, int H, float* actions, float* z_out,
                                    mmt_stream_t stream) {
  g_sampler_route = MMT_SAMPLER_ROUTE_NONE;
  MMT_CHECK_ARG(P && Q && w1 && w2 && b2 && coef && actions && B > 0 && steps > 0 && H > 0,
                "mmt_diffusion_sample: args");
  MMT_CHECK_ARG(A == SA, "mmt_diffusion_sample: the action dimension must be %d (diffusion.py:200)",
                SA);
  MMT_CHECK_ARG(z_in || rng, "mmt_diffusion_sample: need rng or an injected initial sample");
  MMT_CHECK_ARG(ld_p >= H && ld_q >= H && ld_w1 >= SA, "mmt_diffusion_sample: leading dims");
  MMT_CHECK_ARG(ld_w1 % 8 == 0 && ((uintptr_t)w1 & 15) == 0,
                "mmt_diffusion_sample: W1 rows must start on 16-B boundaries");
  MMT_CHECK_ARG(H <= 1024, "mmt_diffusion_sample: hidden width %d > 1024", H);
  const int nu = (H + 63) / 64;
  const dim3 grid((B + SNT / 64 - 1) / (SNT / 64));
  hipStream_t s = as_stream(stream);
#define MMT_SAMPLE(NU_)                                                                        \
  hipLaunchKernelGGL(diffusion_sample_kernel<NU_>, grid, dim3(SNT), 0, s, rng, B, steps,        \
                     sample_offset, P, ld_p, Q, ld_q, (const bf16_t*)w1, ld_w1,                \
                     (const bf16_t*)w2, b2, coef, z_in, H, actions, z_out)
  if (nu <= 2) MMT_SAMPLE(2);
  else if (nu <= 4) MMT_SAMPLE(4);
  else if (nu <= 6) MMT_SAMPLE(6);
  else if (nu <= 8) MMT_SAMPLE(8);
  else if (nu <= 12) MMT_SAMPLE(12);
  else MMT_SAMPLE(16);
#undef MMT_SAMPLE
  MMT_CHECK_LAUNCH("mmt_diffusion_sample");
  g_sampler_route = MMT_SAMPLER_ROUTE_LEGACY_WAVE;
  return MMT_OK;
}
