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

#include "common.h"

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
      const float u1 = ((draw_u32(key, 2 * c) >> 8) + 1) * (1.f / 16777216.f);  // (0, 1]
      const float u2 = (draw_u32(key, 2 * c + 1) >> 8) * (1.f / 16777216.f);
      z[a] = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
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
// for any action width A = 8 .. 64. Still one wave per sample with the hidden units over the
// lanes, but nothing per-unit lives in registers (2 NU A weights would not fit): the bf16 W1x rows
// and W2 columns of all H units sit in LDS, staged once per workgroup as [H][AP] rows (AP = A, or
// A + 8 when A / 8 is even, so a lane's 16-B pieces land on distinct banks), and each lane reads
// the rows of its unit as 16-B vectors. When they do not fit (STEPS_LDS_LIMIT) the same loop reads
// them from global memory, where L2 holds them (256 KB at A = 64, H = 1024).
//
// Rounding model: fp32 operands throughout. The weights are the bf16 shadow, widened exactly;
// x, the hidden layer and every accumulation are fp32 (nothing is rounded to bf16).
//
// Sample state: with A8 = A / 8, lane l keeps the A8 components a = A8 (l >> 3) + i, i < A8, of
// x, z and the step noise (the 8 lanes of a group hold copies). That is where the reduction of
// the A per-lane partial sums of eps_hat leaves them: three exchange stages (lane bits 5, 4, 3),
// each halving the vector a lane carries, then three butterflies on the A8 survivors: 5A/4
// exchanges, not 6A. The matvec takes x[a] as a wave-uniform value (readlane from lane 8 (a / A8)).
constexpr int ST_NT = 256;                 // 4 waves = 4 samples per workgroup
constexpr int ST_MAXNU = 16;               // H <= 1024
constexpr int STEPS_LDS_LIMIT = 160 * 1024;

inline int steps_ap(int A) { return (A / 8) % 2 ? A : A + 8; }
// dynamic LDS of the step kernel: hp, hq [4][64 nu] fp32, then (LDS form) w1s, w2s [H][AP] bf16
inline size_t steps_lds_bytes(int A, int H, bool weights) {
  const size_t hq = (size_t)(ST_NT / 64) * 128 * ((H + 63) / 64) * sizeof(float);
  return hq + (weights ? (size_t)4 * H * steps_ap(A) : 0);
}

__device__ __forceinline__ float normal_draw(uint32_t key, uint32_t c) {
  const float u1 = ((draw_u32(key, 2 * c) >> 8) + 1) * (1.f / 16777216.f);  // (0, 1]
  const float u2 = (draw_u32(key, 2 * c + 1) >> 8) * (1.f / 16777216.f);
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

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
__global__ __launch_bounds__(ST_NT) void diffusion_sample_steps_kernel(const StepArgs p) {
  constexpr int A = 8 * A8;
  constexpr int AP = A8 % 2 ? A : A + 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char st_smem[];
  const int H = p.H, nu = (H + 63) / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* const hp = reinterpret_cast<float*>(st_smem) + wave * 128 * nu;  // P[b] of my units
  float* const hq = hp + 64 * nu;                                         // Q[t_k] of my units
  const bf16_t* const w1s =
      reinterpret_cast<const bf16_t*>(st_smem + (size_t)(ST_NT / 64) * 128 * nu * sizeof(float));
  const bf16_t* const w2s = w1s + (size_t)H * AP;

  if (LDSW) {  // every wave of the workgroup stages, including those past the batch
    bf16_t* const d1 = const_cast<bf16_t*>(w1s);
    bf16_t* const d2 = const_cast<bf16_t*>(w2s);
    for (int i = threadIdx.x; i < H * A8; i += ST_NT) {
      const int j = i / A8, c = i - j * A8;
      *reinterpret_cast<uint4*>(d1 + j * AP + 8 * c) =
          *reinterpret_cast<const uint4*>(p.w1 + (int64_t)j * p.ld_w1 + 8 * c);
    }
    for (int i = threadIdx.x; i < H * A; i += ST_NT) {
      const int a = i / H, j = i - a * H;
      d2[j * AP + a] = p.w2[i];  // transposed: unit j's column of W2 as a row
    }
    __syncthreads();
  }
  const int b = blockIdx.x * (ST_NT / 64) + wave;
  if (b >= p.B) return;  // wave-uniform, after the only barrier

  const int grp = lane >> 3, sub = lane & 7;
  const int a0 = A8 * grp;  // first action component this lane keeps
  const bool fresh = (p.flags & MMT_SAMPLE_FRESH_NOISE) != 0;
  const int64_t gsample = p.sample_offset + b;
  const int a_draw = a0 + (sub < A8 ? sub : A8 - 1);  // the component this lane draws for its group
  const uint32_t ctr = (uint32_t)(gsample * A + a_draw);

  float x[A8], z[A8], nz[A8], b2r[A8];
  if (p.z_in) {
#pragma unroll
    for (int i = 0; i < A8; ++i) z[i] = p.z_in[(int64_t)b * A + a0 + i];
  } else {
    const float v = normal_draw(stream_key(p.rng[0], p.rng[1], 0xFFFEu, 3), ctr);
#pragma unroll
    for (int i = 0; i < A8; ++i) z[i] = __shfl(v, (lane & ~7) | i, 64);
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

  // P[b] of this lane's units is parked in LDS once, Q[t_k] every step (each lane reads back only
  // what it wrote, so no barrier): the unit loop can then index them. The Q row, the table row
  // and the step index after it are fetched a step ahead with plain unconditional loads (clamped
  // addresses, nothing computed on them before the next step), so no step waits on memory. All
  // ST_MAXNU loads are issued whatever nu is: those past nu re-read Q[t][H-1], one cached word
  // for the whole wave, and a `u < nu` guard costs more than it saves, because each guarded
  // block ends in a wait for its own loads (32 steps at H = 384, launch alone: 46.7 us as here,
  // 53.8 us with a guard per unit, 48.9 us with one per four units, at A = 8; 112.5 / 120.0 /
  // 114.3 us at A = 32).
  const float* const prow = p.P + (int64_t)b * p.ld_p;
#pragma unroll
  for (int u = 0; u < ST_MAXNU; ++u)
    if (u < nu) hp[64 * u + lane] = prow[min(lane + 64 * u, H - 1)];
  auto checked_t = [&](int t) {
    if ((unsigned)t >= (unsigned)p.q_rows) {
      if (lane == 0) record_fault(p.fault, MMT_FAULT_ROW_INDEX);
      t = 0;
    }
    return __builtin_amdgcn_readfirstlane(t);
  };
  float qn[ST_MAXNU];
  auto load_q = [&](int t) {
    const float* const q = p.Q + (int64_t)t * p.ld_q;
#pragma unroll
    for (int u = 0; u < ST_MAXNU; ++u) qn[u] = q[min(lane + 64 * u, H - 1)];
  };
  const int last = p.n_steps - 1;
  load_q(checked_t(p.step_t[0]));
  int t_next = p.step_t[min(1, last)];  // raw: checked when its Q row is fetched
  float can = p.step_coef[0], cbn = p.step_coef[1], ccn = p.step_coef[2];

#pragma unroll 1
  for (int k = 0; k < p.n_steps; ++k) {
#pragma unroll
    for (int u = 0; u < ST_MAXNU; ++u)
      if (u < nu) hq[64 * u + lane] = qn[u];
    const float ca = can, cb = cbn, cc = ccn;
    {  // step k + 1's operands (the last step refetches its own)
      const int kn = min(k + 1, last);
      load_q(checked_t(t_next));
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
        const float v = normal_draw(step_noise_key(p.rng[0], p.rng[1], k), ctr);
#pragma unroll
        for (int i = 0; i < A8; ++i) nz[i] = __shfl(v, (lane & ~7) | i, 64);
      }
      if (p.noise_out && sub == 0) {
#pragma unroll
        for (int i = 0; i < A8; ++i) p.noise_out[((int64_t)k * p.B + b) * A + a0 + i] = nz[i];
      }
    }

    float xb[A];  // x as wave-uniform values
#pragma unroll
    for (int a = 0; a < A; ++a)
      xb[a] = __builtin_bit_cast(
          float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x[a % A8]), 8 * (a / A8)));

    float e[A];
#pragma unroll
    for (int a = 0; a < A; ++a) e[a] = 0.f;
#pragma unroll 1
    for (int u = 0; u < nu; ++u) {
      const int j = lane + 64 * u;
      const bool live = j < H;
      const int jj = live ? j : H - 1;  // clamped, its hidden value zeroed below
      float h = hp[64 * u + lane] + hq[64 * u + lane];
      const bf16_t* const r1 = LDSW ? w1s + jj * AP : p.w1 + (int64_t)jj * p.ld_w1;
#pragma unroll
      for (int c = 0; c < A8; ++c) {
        const uint4 row = *reinterpret_cast<const uint4*>(r1 + 8 * c);
        const uint32_t rw[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          h = fmaf(xb[8 * c + 2 * q], __uint_as_float(rw[q] << 16), h);
          h = fmaf(xb[8 * c + 2 * q + 1], __uint_as_float(rw[q] & 0xffff0000u), h);
        }
      }
      h = live ? fmaxf(h, 0.f) : 0.f;
      if (LDSW) {
#pragma unroll
        for (int c = 0; c < A8; ++c) {
          const uint4 row = *reinterpret_cast<const uint4*>(w2s + jj * AP + 8 * c);
          const uint32_t rw[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            e[8 * c + 2 * q] = fmaf(h, __uint_as_float(rw[q] << 16), e[8 * c + 2 * q]);
            e[8 * c + 2 * q + 1] =
                fmaf(h, __uint_as_float(rw[q] & 0xffff0000u), e[8 * c + 2 * q + 1]);
          }
        }
      } else {
#pragma unroll
        for (int a = 0; a < A; ++a) e[a] = fmaf(h, bf2f(p.w2[(int64_t)a * H + jj]), e[a]);
      }
    }

    // sum over the 64 lanes; lane l ends with components A8 (l >> 3) + i
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int o = 32 >> s, n = A >> (s + 1);
      const bool up = (lane & o) != 0;
#pragma unroll
      for (int i = 0; i < n; ++i) {
        float lo = e[i], hi = e[i + n];
        // opaque to the optimiser: it otherwise folds the two selects into e[i + (up ? 0 : n)], a
        // lane-varying index into the register array (a compare-select chain over all of e)
        asm volatile("" : "+v"(lo), "+v"(hi));
        const float send = up ? lo : hi;
        const float keep = up ? hi : lo;
        e[i] = keep + __shfl_xor(send, o, 64);
      }
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
__global__ __launch_bounds__(ST_NT) void diffusion_sample_draws_kernel(
    const uint32_t* __restrict__ rng, int B, int A, int n_steps, int64_t sample_offset,
    bool fresh, const float* __restrict__ z_in, const float* __restrict__ noise_in,
    float* __restrict__ z_out, float* __restrict__ noise_out) {
  const int idx = blockIdx.x * ST_NT + threadIdx.x;  // b * A + a
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

template <int A8>
void launch_steps(bool lds, dim3 grid, size_t smem, hipStream_t s, const StepArgs& p) {
  if (lds) {
    static const bool attr_ =
        (hipFuncSetAttribute((const void*)diffusion_sample_steps_kernel<A8, true>,
                             hipFuncAttributeMaxDynamicSharedMemorySize, STEPS_LDS_LIMIT), true);
    (void)attr_;
    hipLaunchKernelGGL((diffusion_sample_steps_kernel<A8, true>), grid, dim3(ST_NT), smem, s, p);
  } else {
    hipLaunchKernelGGL((diffusion_sample_steps_kernel<A8, false>), grid, dim3(ST_NT), smem, s, p);
  }
}

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
    hipLaunchKernelGGL(diffusion_sample_draws_kernel, dim3((B * A + ST_NT - 1) / ST_NT),
                       dim3(ST_NT), 0, s, rng, B, A, n_steps, sample_offset, fresh, z_in, noise_in,
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
  const bool lds = steps_lds_bytes(A, H, true) <= (size_t)STEPS_LDS_LIMIT;
  StepArgs p{rng, B, n_steps, q_rows, H, flags, sample_offset, P, ld_p, Q, ld_q,
             (const bf16_t*)w1, ld_w1, (const bf16_t*)w2, b2, step_t, step_coef, clip, z_in,
             noise_in, actions, z_out, noise_out, fault_word()};
  const dim3 grid((B + ST_NT / 64 - 1) / (ST_NT / 64));
  const size_t smem = steps_lds_bytes(A, H, lds);
  switch (A / 8) {
    case 1: launch_steps<1>(lds, grid, smem, s, p); break;
    case 2: launch_steps<2>(lds, grid, smem, s, p); break;
    case 3: launch_steps<3>(lds, grid, smem, s, p); break;
    case 4: launch_steps<4>(lds, grid, smem, s, p); break;
    case 5: launch_steps<5>(lds, grid, smem, s, p); break;
    case 6: launch_steps<6>(lds, grid, smem, s, p); break;
    case 7: launch_steps<7>(lds, grid, smem, s, p); break;
    default: launch_steps<8>(lds, grid, smem, s, p); break;
  }
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
