// Small fused kernels around the hot path (gfx950): sequence assembly (token_sequencer.py
// :255-269 + readout.py:18-33 + attention.py:71-85 position embedding + image_tokenizer.py:300-307
// row/col embeddings), readout mean (diffusion.py:102), diffusion noising / Fourier features /
// loss (diffusion.py:17-143), T5 RMS-norm and embedding gather, fused AdamW over the flat
// parameter buffer, and the device-side step counter that keys every random stream.
#include <math.h>

#include <algorithm>

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

// row descriptor: kind << 24 | index   (kind 0 text row, 1 image row, 2 readout row, 3 value row,
// 4 point-cloud row: written and differentiated by values.hip's and pointcloud.hip's kernels,
// skipped here by one kind >= KIND_VALUE compare)
constexpr int KIND_TEXT = 0, KIND_IMAGE = 1, KIND_READOUT = 2, KIND_VALUE = 3, KIND_POINT = 4;
static_assert(KIND_POINT == KIND_VALUE + 1, "the skipped kinds are the highest");

__global__ void seq_assemble_fwd_kernel(int B, int L, int D, const int32_t* __restrict__ row_src,
                                        const bf16_t* __restrict__ text, int T,
                                        const bf16_t* __restrict__ img, int NI,
                                        const int32_t* __restrict__ rtok,
                                        const int32_t* __restrict__ ctok,
                                        const float* __restrict__ row_emb,
                                        const float* __restrict__ col_emb,
                                        const float* __restrict__ readout_pe,
                                        const float* __restrict__ pe, float* __restrict__ x0) {
  const int cpr = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * L * cpr) return;
  const int ch = idx % cpr;
  const int l = (idx / cpr) % L;
  const int b = idx / ((int64_t)cpr * L);
  const int d0 = ch * 8;
  const int desc = row_src[l];
  const int kind = desc >> 24, j = desc & 0xffffff;
  if (kind >= KIND_VALUE) return;  // mmt_value_tokens_fwd / mmt_pc_embed_fwd own the row
  float v[8];
  if (kind == KIND_TEXT) {
    unpack8(*reinterpret_cast<const uint4*>(text + ((int64_t)b * T + j) * D + d0), v);
  } else if (kind == KIND_IMAGE) {
    unpack8(*reinterpret_cast<const uint4*>(img + ((int64_t)b * NI + j) * D + d0), v);
    const int rt = rtok[(int64_t)b * NI + j], ct = ctok[(int64_t)b * NI + j];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += row_emb[(int64_t)rt * D + d0 + e] + col_emb[(int64_t)ct * D + d0 + e];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = readout_pe[(int64_t)j * D + d0 + e];  // zeros + embedding
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] += pe[(int64_t)l * D + d0 + e];
  float* xo = x0 + ((int64_t)b * L + l) * D + d0;
  *reinterpret_cast<float4*>(xo) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(xo + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

__global__ void seq_assemble_bwd_kernel(int B, int L, int D, const int32_t* __restrict__ row_src,
                                        const float* __restrict__ dx0, bf16_t* __restrict__ dtext,
                                        int T, bf16_t* __restrict__ dimg, int NI,
                                        const int32_t* __restrict__ rtok,
                                        const int32_t* __restrict__ ctok,
                                        float* __restrict__ drow_emb, float* __restrict__ dcol_emb,
                                        float* __restrict__ dreadout_pe) {
  const int cpr = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * L * cpr) return;
  const int ch = idx % cpr;
  const int l = (idx / cpr) % L;
  const int b = idx / ((int64_t)cpr * L);
  const int d0 = ch * 8;
  const int desc = row_src[l];
  const int kind = desc >> 24, j = desc & 0xffffff;
  if (kind >= KIND_VALUE) return;  // mmt_value_tokens_bwd / mmt_pc_embed_bwd read the row
  float v[8];
  {
    const float* gp = dx0 + ((int64_t)b * L + l) * D + d0;
    const float4 a = *reinterpret_cast<const float4*>(gp), c = *reinterpret_cast<const float4*>(gp + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
  }
  if (kind == KIND_TEXT) {
    if (dtext) *reinterpret_cast<uint4*>(dtext + ((int64_t)b * T + j) * D + d0) = pack8(v);
  } else if (kind == KIND_IMAGE) {
    *reinterpret_cast<uint4*>(dimg + ((int64_t)b * NI + j) * D + d0) = pack8(v);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) grad_add(dreadout_pe + (int64_t)j * D + d0 + e, v[e]);
  }
}

// d(row_emb)[tok] += dx0[b, l(j)] over every image token (b, j) with rtok == tok (same for col).
// One workgroup = 64 columns x a slice of the image tokens; the two (Q x 64) partial tables are
// accumulated with LDS atomics and flushed with one global atomic per table entry. Measured:
// bound by the LDS float atomics (~50 M per step at B = 256); fewer, longer workgroups were slower.
constexpr int EMB_COLS = 64, EMB_SPLIT = 128;
// DET (deterministic mode): the table holds 64-bit fixed-point sums (integer LDS atomics,
// order-independent) and each entry goes to the gradient's fixed-point shadow (grad_add).
template <bool DET>
__global__ __launch_bounds__(256) void embed_grad_kernel(int B, int L, int D, int NI, int Q,
                                                         const int32_t* __restrict__ img_rows,
                                                         const float* __restrict__ dx0,
                                                         const int32_t* __restrict__ rtok,
                                                         const int32_t* __restrict__ ctok,
                                                         float* __restrict__ drow_emb,
                                                         float* __restrict__ dcol_emb) {
  extern __shared__ float tab[];  // [2][Q][EMB_COLS] (DET: long long)
  long long* tab64 = reinterpret_cast<long long*>(tab);
  const int c0 = blockIdx.x * EMB_COLS;
  for (int i = threadIdx.x; i < 2 * Q * EMB_COLS; i += blockDim.x) {
    if constexpr (DET) tab64[i] = 0;
    else tab[i] = 0.f;
  }
  __syncthreads();
  const int64_t total = (int64_t)B * NI;
  const int64_t per = (total + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = blockIdx.y * per, r1 = min(total, r0 + per);
  const int cv = threadIdx.x & 7, rg = threadIdx.x >> 3;  // 8 x 8 columns, 32 row groups
  const int col = c0 + cv * 8;
  if (col < D) {
    for (int64_t rr = r0 + rg; rr < r1; rr += 32) {
      const int b = rr / NI, j = rr % NI;
      const float* gp = dx0 + ((int64_t)b * L + img_rows[j]) * D + col;
      const float4 a = *reinterpret_cast<const float4*>(gp), c = *reinterpret_cast<const float4*>(gp + 4);
      const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
      const int rt = rtok[rr], ct = ctok[rr];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if constexpr (DET) {
          if (det_fits(v[e])) {
            const unsigned long long q = (unsigned long long)det_fixed(v[e]);
            atomicAdd(reinterpret_cast<unsigned long long*>(&tab64[rt * EMB_COLS + cv * 8 + e]), q);
            atomicAdd(reinterpret_cast<unsigned long long*>(&tab64[(Q + ct) * EMB_COLS + cv * 8 + e]), q);
          } else {  // NaN / Inf / out of the shadow's range: straight to the fp32 gradient (visible)
            atomicAdd(drow_emb + (int64_t)rt * D + col + e, v[e]);
            atomicAdd(dcol_emb + (int64_t)ct * D + col + e, v[e]);
          }
        } else {
          atomicAdd(&tab[rt * EMB_COLS + cv * 8 + e], v[e]);
          atomicAdd(&tab[(Q + ct) * EMB_COLS + cv * 8 + e], v[e]);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * Q * EMB_COLS; i += blockDim.x) {
    const int which = i / (Q * EMB_COLS), rem = i % (Q * EMB_COLS);
    const int tok = rem / EMB_COLS, cc = c0 + rem % EMB_COLS;
    float* dst = (which ? dcol_emb : drow_emb) + (int64_t)tok * D + cc;
    if constexpr (DET) {  // the fixed-point partial straight into the shadow (exact)
      const long long q = tab64[i];
      const int64_t gi = dst - g_det.base;
      if (cc < D && q != 0) {
        if (g_det.fx != nullptr && gi >= 0 && gi < g_det.n)
          atomicAdd(reinterpret_cast<unsigned long long*>(g_det.fx + gi), (unsigned long long)q);
        else
          atomicAdd(dst, (float)((double)q * (1.0 / DET_SCALE)));
      }
    } else {
      const float val = tab[i];
      if (cc < D && val != 0.f) atomicAdd(dst, val);
    }
  }
}

// Position-embedding gradients by window (mmt_patch_embed_grad). A patch in patch-row ri draws its
// row token from the window [q(ri P), q((ri + 1) P)) of patch_positions_kernel (likewise columns),
// so the image tokens of one patch row touch only that window's few table rows. One workgroup =
// one window x 64 columns x a slice of the batch: each thread keeps a register accumulator per
// window token (select + add per row, no atomics), the 32 row groups meet by shuffles and in LDS,
// and the workgroup adds its WMAX x 64 partial table with one global atomic per entry.
template <int WMAX>
__global__ __launch_bounds__(256) void embed_grad_win_kernel(
    int B, int L, int D, int I, int PPD, int Himg, int P, int Q, int splits,
    const int32_t* __restrict__ img_rows, const float* __restrict__ dx0,
    const int32_t* __restrict__ rtok, const int32_t* __restrict__ ctok, float* __restrict__ drow,
    float* __restrict__ dcol) {
  __shared__ float part[4][WMAX][EMB_COLS];
  const int w = blockIdx.x, c0 = blockIdx.y * EMB_COLS;
  const int z = blockIdx.z % 2, sp = blockIdx.z / 2;  // table (0 rows, 1 columns), batch slice
  const int NP = PPD * PPD, NI = I * NP, RPS = I * PPD;  // image tokens per sample in the window
  auto q = [&](int v) { return (int)floorf(((float)v / (float)Himg) * (float)(Q - 1)); };
  const int ws = q(w * P), wn = max(1, q((w + 1) * P) - ws);
  const int bper = (B + splits - 1) / splits, b0 = sp * bper, b1 = min(B, b0 + bper);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cv = threadIdx.x & 7, rg = threadIdx.x >> 3;
  const int col = c0 + cv * 8;
  const int32_t* tok = z == 0 ? rtok : ctok;
  float acc[WMAX][8];
#pragma unroll
  for (int t = 0; t < WMAX; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[t][e] = 0.f;
  if (col < D && b0 < b1) {
    const int nrows = (b1 - b0) * RPS;
    for (int r = rg; r < nrows; r += 32) {
      const int b = b0 + r / RPS, rem = r % RPS, i = rem / PPD, k = rem % PPD;
      const int p = z == 0 ? k * PPD + w : w * PPD + k;  // patch_positions_kernel: ri = p % PPD
      const int j = i * NP + p;
      const int t = tok[(int64_t)b * NI + j] - ws;
      const float* gp = dx0 + ((int64_t)b * L + img_rows[j]) * D + col;
      const float4 a = *reinterpret_cast<const float4*>(gp), c = *reinterpret_cast<const float4*>(gp + 4);
      const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
      for (int u = 0; u < WMAX; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[u][e] += t == u ? v[e] : 0.f;
    }
  }
#pragma unroll
  for (int u = 0; u < WMAX; ++u)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = acc[u][e];
      x += __shfl_xor(x, 8, 64);
      x += __shfl_xor(x, 16, 64);
      x += __shfl_xor(x, 32, 64);
      acc[u][e] = x;
    }
  if (lane < 8)
#pragma unroll
    for (int u = 0; u < WMAX; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) part[wave][u][cv * 8 + e] = acc[u][e];
  __syncthreads();
  float* table = z == 0 ? drow : dcol;
  for (int i = threadIdx.x; i < WMAX * EMB_COLS; i += blockDim.x) {
    const int u = i / EMB_COLS, cc = c0 + i % EMB_COLS;
    if (u < wn && cc < D) {
      const float val = part[0][u][i % EMB_COLS] + part[1][u][i % EMB_COLS] +
                        part[2][u][i % EMB_COLS] + part[3][u][i % EMB_COLS];
      if (val != 0.f) grad_add(table + (int64_t)(ws + u) * D + cc, val);
    }
  }
}

// e[b, :] = mean over the listed rows of x[b] ; written as bf16 into out (row stride ld_out)
__global__ void rows_mean_fwd_kernel(const float* __restrict__ x, int64_t xs_b, int64_t xs_t,
                                     int D, const int32_t* __restrict__ rows, int nrows,
                                     bf16_t* __restrict__ out, int64_t ld_out) {
  const int b = blockIdx.x;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f;
    for (int i = 0; i < nrows; ++i) s += x[b * xs_b + (int64_t)rows[i] * xs_t + d];
    out[b * ld_out + d] = f2bf(s / nrows);
  }
}

// dx[b, l, :] = de[b, :] / n for listed rows (row_flag[l] >= 0), 0 otherwise (whole buffer)
__global__ void rows_mean_bwd_kernel(const bf16_t* __restrict__ de, int64_t ld_de, int B, int L,
                                     int D, const int32_t* __restrict__ row_flag, int nrows,
                                     float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * L * D) return;
  const int d = idx % D;
  const int l = (idx / D) % L;
  const int b = idx / ((int64_t)D * L);
  dx[idx] = row_flag[l] >= 0 ? bf2f(de[b * ld_de + d]) / nrows : 0.f;
}

// Grouped readout means (categorical.py:32-37: "batch (action timestep) embeddings -> batch action
// timestep embeddings", mean over timestep): out[b, g, :] = mean of the rows l with
// row_group[l] == g (counts[g] of them); bf16 (B, G, D). Backward: dx[b, l, :] = de[b, g(l), :] /
// counts[g], 0 for rows in no group (whole fp32 buffer).
__global__ void rows_group_mean_fwd_kernel(const float* __restrict__ x, int64_t xs_b, int64_t xs_t,
                                           int L, int D, const int32_t* __restrict__ row_group,
                                           int G, const int32_t* __restrict__ counts,
                                           bf16_t* __restrict__ out) {
  const int b = blockIdx.x, g = blockIdx.y;
  const float inv = 1.f / (float)counts[g];
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f;
    for (int l = 0; l < L; ++l)
      if (row_group[l] == g) s += x[b * xs_b + (int64_t)l * xs_t + d];
    out[((int64_t)b * G + g) * D + d] = f2bf(s * inv);
  }
}

__global__ void rows_group_mean_bwd_kernel(const bf16_t* __restrict__ de, int B, int L, int D,
                                           const int32_t* __restrict__ row_group, int G,
                                           const int32_t* __restrict__ counts,
                                           float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * L * D) return;
  const int d = idx % D;
  const int l = (idx / D) % L;
  const int b = idx / ((int64_t)D * L);
  const int g = row_group[l];
  dx[idx] = g >= 0 ? bf2f(de[((int64_t)b * G + g) * D + d]) / (float)counts[g] : 0.f;
}

// Continuous and categorical action-head losses, one wave per row of z (fp32, row stride ldz):
// kind 0 — ContinuousActionHead (continuous.py:19-26) + compute_l2_loss (octo.py:167-174), rows = B,
//   N = A: p = tanh(z / m) m (written to pred if non-NULL); loss += inv_count sum_a (p - y)^2;
//   dz = 2 (p - y)(1 - tanh^2) inv_count.
// kind 1 — CategoricalActionHead + compute_ce_loss (octo.py:187-198), rows = B*A, N = num_bins:
//   bin = jnp.digitize(y, edges) = #edges <= y (edges = linspace(-m, m, N+1)), label =
//   one_hot(bin, N) — all zero when bin >= N, the reference's off-by-one kept; loss += inv_count
//   (sum(label) logsumexp(z) - label . z); dz = (sum(label) softmax(z) - label) inv_count.
// y NULL: forward only (kind 0 writes pred). loss is accumulated atomically (zero it first).
__global__ __launch_bounds__(256) void action_head_kernel(
    int kind, const float* __restrict__ z, int64_t ldz, int R, int N, const float* __restrict__ y,
    const float* __restrict__ edges, int n_edges, float max_action, float inv_count,
    float* __restrict__ pred, float* __restrict__ loss, bf16_t* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* zr = z + (int64_t)r * ldz;
  float row_loss = 0.f;
  if (kind == 0) {
    for (int a = lane; a < N; a += 64) {
      const float th = tanhf(zr[a] / max_action);
      const float p = th * max_action;
      if (pred) pred[(int64_t)r * N + a] = p;
      if (y) {
        const float d = p - y[(int64_t)r * N + a];
        row_loss += d * d;
        dz[(int64_t)r * N + a] = f2bf(2.f * d * (1.f - th * th) * inv_count);
      }
    }
  } else {
    const float yv = y[r];
    int bin = 0;
    for (int i = 0; i < n_edges; ++i) bin += edges[i] <= yv ? 1 : 0;
    const float has = bin < N ? 1.f : 0.f;
    float mx = -INFINITY;
    for (int c = lane; c < N; c += 64) mx = fmaxf(mx, zr[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float se = 0.f;
    for (int c = lane; c < N; c += 64) se += expf(zr[c] - mx);
    se = wave_sum(se);
    const float lse = mx + logf(se);
    for (int c = lane; c < N; c += 64) {
      const float lab = (c == bin) ? 1.f : 0.f;
      dz[(int64_t)r * N + c] = f2bf((has * expf(zr[c] - lse) - lab) * inv_count);
    }
    if (lane == 0 && bin < N) row_loss = lse - zr[bin];
  }
  if (!y) return;
  row_loss = wave_sum(row_loss);
  if (lane == 0) atomicAdd(loss, row_loss * inv_count);
}

// Diffusion noising + Fourier features (diffusion.py:41-51, 110-131):
//   t ~ U{0..steps-1}, eps ~ N(0, 1) (Box-Muller on the counter stream) unless injected;
//   noisy = sqrt(abar_t) a + sqrt(1 - abar_t) eps  -> cat[:, 0:A]  (bf16)
//   h = 2 pi t W^T (W: (F,) = fourier kernel (F, 1)), feats = [cos h, sin h] (bf16, 2F)
__global__ void diffusion_prep_kernel(const uint32_t* __restrict__ rng, int B, int A, int steps,
                                      int64_t sample_offset, const float* __restrict__ actions,
                                      const float* __restrict__ alpha_hats,
                                      const float* __restrict__ fw, int F,
                                      const int32_t* __restrict__ t_in,
                                      const float* __restrict__ eps_in, int32_t* __restrict__ t_out,
                                      float* __restrict__ eps_out, bf16_t* __restrict__ cat,
                                      int64_t ld_cat, bf16_t* __restrict__ feats) {
  const int b = blockIdx.x;
  __shared__ int s_t;
  if (threadIdx.x == 0) {
    int t;
    if (t_in) {
      t = t_in[b];
    } else {
      const uint32_t key = stream_key(rng[0], rng[1], 0xFFFEu, 1);
      t = (int)(((uint64_t)draw_u32(key, (uint32_t)(sample_offset + b)) * (uint32_t)steps) >> 32);
    }
    s_t = t;
    t_out[b] = t;
  }
  __syncthreads();
  const int t = s_t;
  const float ah = alpha_hats[t];
  const float a1 = sqrtf(ah), a2 = sqrtf(1.f - ah);
  for (int j = threadIdx.x; j < A; j += blockDim.x) {
    float e;
    if (eps_in) {
      e = eps_in[b * A + j];
    } else {
      const uint32_t key = stream_key(rng[0], rng[1], 0xFFFEu, 2);
      const uint32_t c = (uint32_t)((sample_offset + b) * A + j);
      e = normal_draw(key, c);
    }
    eps_out[b * A + j] = e;
    cat[b * ld_cat + j] = f2bf(a1 * actions[b * A + j] + a2 * e);
  }
  const float tf = (float)t;
  for (int k = threadIdx.x; k < F; k += blockDim.x) {
    const float h = 2.f * 3.141592653589793f * tf * fw[k];
    feats[(int64_t)b * 2 * F + k] = f2bf(cosf(h));
    feats[(int64_t)b * 2 * F + F + k] = f2bf(sinf(h));
  }
}

// dW[k] += sum_b 2 pi t_b (cos(h) dsin - sin(h) dcos); the batch is split over grid.y
// (FB_B samples per workgroup, fp32 atomics into dw) so the launch is not one serial loop over B.
constexpr int FB_B = 8;
__global__ void fourier_bwd_kernel(const bf16_t* __restrict__ dfeats, int B, int F,
                                   const int32_t* __restrict__ t, const float* __restrict__ fw,
                                   float* __restrict__ dw) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= F) return;
  const int b0 = blockIdx.y * FB_B;
  const float w = fw[k];
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < FB_B; ++i) {
    const int b = b0 + i;
    if (b < B) {
      const float tt = 2.f * 3.141592653589793f * (float)t[b];
      const float h = tt * w;
      const float dc = bf2f(dfeats[(int64_t)b * 2 * F + k]), ds = bf2f(dfeats[(int64_t)b * 2 * F + F + k]);
      acc += tt * (cosf(h) * ds - sinf(h) * dc);
    }
  }
  grad_add(dw + k, acc);
}

// loss = mean_b sum_j 0.5 (pred - eps)^2 (optax.l2_loss, diffusion.py:141-142);
// dpred = (pred - eps) * grad_scale / B  (bf16). One workgroup; loss[0] is overwritten.
__global__ void diffusion_loss_kernel(const float* __restrict__ pred, int64_t ld_pred,
                                      const float* __restrict__ eps, int B, int A,
                                      float grad_scale, float* __restrict__ loss,
                                      bf16_t* __restrict__ dpred) {
  __shared__ float red[1024 / 64];
  float s = 0.f;
  for (int i = threadIdx.x; i < B * A; i += blockDim.x) {
    const int b = i / A, j = i % A;
    const float d = pred[b * ld_pred + j] - eps[i];
    s += 0.5f * d * d;
    dpred[i] = f2bf(d * grad_scale / B);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    loss[0] = t / B;
  }
}

// T5LayerNorm: y = x * rsqrt(mean(x^2) + eps) * w   (one wave per row, D % 8 == 0)
__global__ void rmsnorm_fwd_kernel(const bf16_t* __restrict__ x, int64_t rows, int D,
                                   const bf16_t* __restrict__ w, float eps, bf16_t* __restrict__ y) {
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const bf16_t* xr = x + row * D;
  float s = 0.f;
  if (D <= 1024) {
    // the row read once: both of a lane's chunks (and the weight's) loaded together, unconditional
    // (a lane past D reads chunk 0 and drops it); same sums in the same order as the loop below
    const int c0 = lane * 8, c1 = c0 + 512;
    const bool h0 = c0 < D, h1 = c1 < D;
    const uint4 u0 = *reinterpret_cast<const uint4*>(xr + (h0 ? c0 : 0));
    const uint4 u1 = *reinterpret_cast<const uint4*>(xr + (h1 ? c1 : 0));
    const uint4 w0 = *reinterpret_cast<const uint4*>(w + (h0 ? c0 : 0));
    const uint4 w1 = *reinterpret_cast<const uint4*>(w + (h1 ? c1 : 0));
    float f0[8], f1[8];
    unpack8(u0, f0);
    unpack8(u1, f1);
    if (h0)
#pragma unroll
      for (int e = 0; e < 8; ++e) s += f0[e] * f0[e];
    if (h1)
#pragma unroll
      for (int e = 0; e < 8; ++e) s += f1[e] * f1[e];
    s = wave_sum(s);
    const float rs = rsqrtf(s / D + eps);
    float g[8];
    if (h0) {
      unpack8(w0, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) f0[e] = f0[e] * rs * g[e];
      *reinterpret_cast<uint4*>(y + row * D + c0) = pack8(f0);
    }
    if (h1) {
      unpack8(w1, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) f1[e] = f1[e] * rs * g[e];
      *reinterpret_cast<uint4*>(y + row * D + c1) = pack8(f1);
    }
    return;
  }
  for (int c = lane * 8; c < D; c += 512) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(xr + c), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += f[e] * f[e];
  }
  s = wave_sum(s);
  const float rs = rsqrtf(s / D + eps);
  for (int c = lane * 8; c < D; c += 512) {
    float f[8], g[8];
    unpack8(*reinterpret_cast<const uint4*>(xr + c), f);
    unpack8(*reinterpret_cast<const uint4*>(w + c), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = f[e] * rs * g[e];
    *reinterpret_cast<uint4*>(y + row * D + c) = pack8(f);
  }
}

// out[r, :] = table[clamp(ids[r], 0, vocab - 1), :] (jnp.take's clamp: no id forms an address
// outside the table), one 16-B vector per thread
__global__ void embedding_gather_kernel(const int32_t* __restrict__ ids, int64_t n, int D,
                                        const bf16_t* __restrict__ table, int vocab,
                                        bf16_t* __restrict__ out) {
  const int cpr = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * cpr) return;
  const int64_t r = idx / cpr;
  const int c = (idx % cpr) * 8;
  int id = ids[r];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  *reinterpret_cast<uint4*>(out + r * D + c) = *reinterpret_cast<const uint4*>(table + (int64_t)id * D + c);
}

// AdamW (optax.adamw semantics, decoupled weight decay on every parameter unless a group table
// says otherwise: adamw_groups_kernel; bias-corrected moments) over the flat fp32 master buffer; writes the bf16 shadow used by the GEMMs.
// One update function for both kernels below, so their arithmetic is the same instructions.
// The grid-stride bounds come from the kernels: blockDim / gridDim read inside a kernel body
// fold to the uniform-workgroup form, read in a device function they do not.
struct AdamwCoef {
  float b1, b2, bc1, bc2, omb1, omb2;
};

__device__ __forceinline__ AdamwCoef adamw_coef(double b1d, double b2d, const int step) {
  // the betas arrive in double (optax / torch hold them as Python floats): 1 - b and the bias
  // corrections are formed in double and rounded once (fp32 1.f - 0.999f would differ from
  // (float)0.001 by 1.3e-5 relative)
  AdamwCoef c;
  c.b1 = (float)b1d;
  c.b2 = (float)b2d;
  c.bc1 = (float)(1.0 - pow(b1d, (double)step));
  c.bc2 = (float)(1.0 - pow(b2d, (double)step));
  c.omb1 = (float)(1.0 - b1d);
  c.omb2 = (float)(1.0 - b2d);
  return c;
}

// Parameter EMA (include/mmt_api.h mmt_adamw_ema): the decay of s = state[1] and 1 - decay,
// formed in double and each rounded once, as adamw_coef treats the betas.
struct EmaCoef {
  float d, omd;
};

__device__ __forceinline__ EmaCoef ema_coef(const mmt_ema_decay_t& dc, const int s) {
  double d = dc.value;
  if (dc.kind == MMT_EMA_WARMUP) {
    const int64_t k = (int64_t)s - dc.update_after_step - 1;
    d = 0.0;
    if (k > 0)
      d = fmin(dc.max_value, fmax(dc.min_value, 1.0 - pow(1.0 + (double)k / dc.inv_gamma, -dc.power)));
  }
  return EmaCoef{(float)d, (float)(1.0 - d)};
}

// One element's update: the only place the arithmetic is written, shared by every AdamW kernel.
// EMA: also ema[i] = d * ema[i] + (1 - d) * p_new (one product and one fused multiply-add, two
// fp32 roundings). Its load joins the other four ahead of the first store, and the empty asm
// holds the loaded value in its register there: left to itself the compiler sinks the use of
// ema[i] below the stores of m, v and p, where the wait for the load also waits for those
// stores to complete before the next iteration's loads can be issued (measured: 197 us against
// 140 us for the plain kernel at 22.5 M elements, slower than AdamW followed by a separate pass).
template <bool EMA = false>
__device__ __forceinline__ void adamw_elem(float* __restrict__ p, const float* __restrict__ g,
                                           float* __restrict__ m, float* __restrict__ v,
                                           bf16_t* __restrict__ shadow, const int64_t i,
                                           const AdamwCoef& c, float lr, float eps, float wd,
                                           float grad_scale, float* __restrict__ ema = nullptr,
                                           const EmaCoef ec = EmaCoef{}) {
  const float gi = g[i] * grad_scale;
  const float mi = c.b1 * m[i] + c.omb1 * gi;
  const float vi = c.b2 * v[i] + c.omb2 * (gi * gi);
  float pi = 0.f, e = 0.f;
  if (EMA) {
    pi = p[i];
    e = ema[i];
    asm volatile("" : "+v"(e), "+v"(pi));
  }
  m[i] = mi;
  v[i] = vi;
  // the plain kernels read p[i] here, as they always have
  const float upd = (mi / c.bc1) / (sqrtf(vi / c.bc2) + eps) + wd * (EMA ? pi : p[i]);
  const float pn = (EMA ? pi : p[i]) - lr * upd;
  p[i] = pn;
  if (shadow) shadow[i] = f2bf(pn);
  if (EMA) ema[i] = __builtin_fmaf(ec.d, e, ec.omd * pn);
}

template <bool EMA = false>
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g,
                                             float* __restrict__ m, float* __restrict__ v,
                                             bf16_t* __restrict__ shadow, int64_t n,
                                             const int step, float lr,
                                             double b1d, double b2d, float eps, float wd,
                                             float grad_scale, int64_t first, int64_t stride,
                                             float* __restrict__ ema = nullptr,
                                             const EmaCoef ec = EmaCoef{}) {
  const AdamwCoef c = adamw_coef(b1d, b2d, step);
  for (int64_t i = first; i < n; i += stride)
    adamw_elem<EMA>(p, g, m, v, shadow, i, c, lr, eps, wd, grad_scale, ema, ec);
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                             float* __restrict__ m, float* __restrict__ v,
                             bf16_t* __restrict__ shadow, int64_t n, const int32_t* __restrict__ state,
                             float lr, double b1d, double b2d, float eps, float wd, float grad_scale) {
  adamw_update(p, g, m, v, shadow, n, state[1] + 1, lr, b1d, b2d, eps, wd, grad_scale,
               (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// AdamW with the learning rate, the gradient factor and the skip flag read from the device
// words mmt_optim_prepare wrote (include/mmt_api.h: opt[3], opt[2], opt[6]). The skip test is
// uniform over the grid. The four device scalars are loaded side by side before it (the empty
// asm pins them there): tested first, opt[6] is one more dependent scalar load from memory in
// front of every wave, ahead of the one for state[1].
__global__ void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                 float* __restrict__ m, float* __restrict__ v,
                                 bf16_t* __restrict__ shadow, int64_t n,
                                 const int32_t* __restrict__ state, const float* __restrict__ opt,
                                 double b1d, double b2d, float eps, float wd) {
  const float skip = opt[6], lr = opt[3], gmul = opt[2];
  const int step = state[1] + 1;
  asm volatile("" ::"s"(skip), "s"(lr), "s"(gmul), "s"(step));
  if (skip != 0.f) return;
  adamw_update(p, g, m, v, shadow, n, step, lr, b1d, b2d, eps, wd, gmul,
               (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// mmt_adamw_ema without groups: adamw_kernel (DEV false: lr and the gradient factor from the
// host) or adamw_dev_kernel (DEV true: from the opt words, with the skip test) plus the EMA
// update. The decay descriptor travels by value; its decay is evaluated here from state[1], so
// a captured launch follows the schedule.
template <bool DEV>
__global__ void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                 float* __restrict__ m, float* __restrict__ v,
                                 bf16_t* __restrict__ shadow, float* __restrict__ ema, int64_t n,
                                 const int32_t* __restrict__ state, const float* __restrict__ opt,
                                 float lr_host, double b1d, double b2d, float eps, float wd,
                                 float gs_host, const mmt_ema_decay_t decay) {
  float lr = lr_host, gmul = gs_host;
  int step;
  if (DEV) {
    const float skip = opt[6];
    lr = opt[3];
    gmul = opt[2];
    step = state[1] + 1;
    asm volatile("" ::"s"(skip), "s"(lr), "s"(gmul), "s"(step));
    if (skip != 0.f) return;
  } else {
    step = state[1] + 1;
  }
  adamw_update<true>(p, g, m, v, shadow, n, step, lr, b1d, b2d, eps, wd, gmul,
                     (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                     (int64_t)gridDim.x * blockDim.x, ema, ema_coef(decay, step - 1));
}

// AdamW with parameter groups (optax.adamw(mask=...) inside optax.multi_transform with
// set_to_zero for the frozen group): one flag byte per 64-element chunk of the flat buffer,
// bit 0 = no weight decay, bit 1 = frozen (include/mmt_api.h MMT_GROUP_*). The launch geometry is
// the plain kernels': 256 lanes and a grid stride that is a multiple of 64, so in every
// iteration a wave covers exactly one chunk and its flag is wave-uniform. A wave fetches the
// flags of its next 64 iterations with one load (lane k holds iteration k's), turns them into two
// 64-bit scalar masks by ballot, and the loop branches on their bits: no memory wait stands
// between one iteration's stores and the next one's loads, as in the plain loop. (A flag load inside the loop made the compiler
// wait for every outstanding vector memory operation, the stores included, at the loop's head:
// +16 % at 22.5 M elements.) A frozen chunk is skipped before any load of p, g, m, v or the
// shadow; an undecayed one runs adamw_elem with wd = 0.
// DEV: lr, the gradient factor and the skip flag come from the opt words, as adamw_dev_kernel.
// EMA: the update of mmt_adamw_ema on top (a frozen chunk issues no load or store of ema either).
// The body is shared by both kernels below; first / stride come from them (see above).
template <bool DEV, bool EMA>
__device__ __forceinline__ void adamw_groups_body(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, bf16_t* __restrict__ shadow, float* __restrict__ ema, int64_t n,
    const int32_t* __restrict__ state, const float* __restrict__ opt, float lr_host, double b1d,
    double b2d, float eps, float wd, float gs_host, const uint8_t* __restrict__ flags,
    const mmt_ema_decay_t& decay, const int64_t first, const int64_t stride) {
  float lr = lr_host, gmul = gs_host;
  int step;
  if (DEV) {
    const float skip = opt[6];
    lr = opt[3];
    gmul = opt[2];
    step = state[1] + 1;
    asm volatile("" ::"s"(skip), "s"(lr), "s"(gmul), "s"(step));
    if (skip != 0.f) return;
  } else {
    step = state[1] + 1;
  }
  const AdamwCoef c = adamw_coef(b1d, b2d, step);
  const EmaCoef ec = EMA ? ema_coef(decay, step - 1) : EmaCoef{};
  const int lane = threadIdx.x & 63;
  const int64_t nc = (n + MMT_GROUP_CHUNK - 1) >> MMT_GROUP_CHUNK_SHIFT;  // chunks; < 2^31
  // the wave's first chunk and its chunk stride, as scalars (the host bounds the grid, so a
  // chunk index fits an int)
  const int64_t c0 = __builtin_amdgcn_readfirstlane((int)((first - lane) >> MMT_GROUP_CHUNK_SHIFT));
  const int64_t cs = stride >> MMT_GROUP_CHUNK_SHIFT;
  for (int64_t k0 = 0; c0 + k0 * cs < nc; k0 += 64) {
    const int64_t cl = c0 + (k0 + lane) * cs;  // lane k fetches the flag of iteration k0 + k
    const unsigned fv = cl < nc ? flags[cl] : (unsigned)MMT_GROUP_FROZEN;
    // two 64-bit scalar masks, bit k = iteration k0 + k: the loop below depends on no register
    // a load wrote
    const uint64_t frozen = __ballot((fv & MMT_GROUP_FROZEN) != 0);
    const uint64_t no_decay = __ballot((fv & MMT_GROUP_NO_DECAY) != 0);
    for (int k = 0; k < 64; ++k) {
      if (c0 + (k0 + k) * cs >= nc) break;
      if ((frozen >> k) & 1) continue;
      const int64_t i = first + (k0 + k) * stride;
      if (i < n)
        adamw_elem<EMA>(p, g, m, v, shadow, i, c, lr, eps, ((no_decay >> k) & 1) ? 0.f : wd, gmul,
                        ema, ec);
    }
  }
}

template <bool DEV>
__global__ void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                    float* __restrict__ m, float* __restrict__ v,
                                    bf16_t* __restrict__ shadow, int64_t n,
                                    const int32_t* __restrict__ state,
                                    const float* __restrict__ opt, float lr_host, double b1d,
                                    double b2d, float eps, float wd, float gs_host,
                                    const uint8_t* __restrict__ flags) {
  adamw_groups_body<DEV, false>(p, g, m, v, shadow, nullptr, n, state, opt, lr_host, b1d, b2d, eps,
                                wd, gs_host, flags, mmt_ema_decay_t{},
                                (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                                (int64_t)gridDim.x * blockDim.x);
}

template <bool DEV>
__global__ void adamw_groups_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                        float* __restrict__ m, float* __restrict__ v,
                                        bf16_t* __restrict__ shadow, float* __restrict__ ema,
                                        int64_t n, const int32_t* __restrict__ state,
                                        const float* __restrict__ opt, float lr_host, double b1d,
                                        double b2d, float eps, float wd, float gs_host,
                                        const uint8_t* __restrict__ flags,
                                        const mmt_ema_decay_t decay) {
  adamw_groups_body<DEV, true>(p, g, m, v, shadow, ema, n, state, opt, lr_host, b1d, b2d, eps, wd,
                               gs_host, flags, decay,
                               (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                               (int64_t)gridDim.x * blockDim.x);
}

// mmt_ema_swap: p <-> ema with the bf16 shadow of the new p, skipping frozen chunks (their EMA
// equals their parameter). The geometry of the AdamW kernels, so a wave's flag is uniform.
__global__ void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema,
                                bf16_t* __restrict__ shadow, int64_t n,
                                const uint8_t* __restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (flags && (flags[i >> MMT_GROUP_CHUNK_SHIFT] & MMT_GROUP_FROZEN)) continue;
    const float a = p[i], b = ema[i];
    p[i] = b;
    ema[i] = a;
    if (shadow) shadow[i] = f2bf(b);
  }
}

// Sum of squares of the flat gradient, launch 1 of mmt_optim_prepare: GN_GRID workgroups (a
// constant, so the partition depends on n alone), workgroup b owns the 16-B vectors
// [b * per, (b + 1) * per) clipped to n / 4, per = ceil((n / 4) / GN_GRID); the n % 4 tail
// elements go to the last workgroup. A lane keeps 4 independent 16-B loads in flight, each with
// its own 4 accumulators (one fused multiply-add per element), then fixed trees: the lane's 16
// accumulators (4 levels), the wave's 64 lanes by xor shuffles (6), the 4 waves through LDS (2).
// Longest chain of fp32 roundings on any path: ceil(per / 1024) + 1 (tail) + 4 + 6 + 2.
// No atomics; every workgroup stores its partial, an empty chunk stores 0.
constexpr int GN_GRID = MMT_GRAD_NORM_GRID;

__device__ __forceinline__ void sumsq_acc(float4& a, const float4 x) {
  a.x = fmaf(x.x, x.x, a.x);
  a.y = fmaf(x.y, x.y, a.y);
  a.z = fmaf(x.z, x.z, a.z);
  a.w = fmaf(x.w, x.w, a.w);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                         float* __restrict__ partial) {
  __shared__ float wsum[4];
  const int64_t n4 = n >> 2;
  const int64_t per = (n4 + GN_GRID - 1) / GN_GRID;
  const int64_t lo = std::min<int64_t>((int64_t)blockIdx.x * per, n4);
  const int64_t hi = std::min<int64_t>(lo + per, n4);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
  int64_t i = lo + threadIdx.x;
  for (; i + 768 < hi; i += 1024) {
    const float4 x0 = g4[i], x1 = g4[i + 256], x2 = g4[i + 512], x3 = g4[i + 768];
    sumsq_acc(a0, x0);
    sumsq_acc(a1, x1);
    sumsq_acc(a2, x2);
    sumsq_acc(a3, x3);
  }
  if (i < hi) sumsq_acc(a0, g4[i]);
  if (i + 256 < hi) sumsq_acc(a1, g4[i + 256]);
  if (i + 512 < hi) sumsq_acc(a2, g4[i + 512]);
  if (blockIdx.x == GN_GRID - 1 && (int64_t)threadIdx.x < (n & 3)) {
    const float t = g[4 * n4 + threadIdx.x];
    a0.x = fmaf(t, t, a0.x);
  }
  const float sx = (a0.x + a1.x) + (a2.x + a3.x), sy = (a0.y + a1.y) + (a2.y + a3.y);
  const float sz = (a0.z + a1.z) + (a2.z + a3.z), sw = (a0.w + a1.w) + (a2.w + a3.w);
  float s = (sx + sy) + (sz + sw);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// grad_sumsq_kernel over the trainable chunks only (launch 1 of mmt_optim_prepare_groups): the
// same partition, the same accumulators and the same trees; a 16-B vector of a frozen chunk
// (16 vectors per 64-element chunk, so a vector never straddles two) is not loaded and enters
// as zeros, which leaves its accumulator's bits as they are (fma(0, 0, a) = a for a >= +0).
// With no frozen bit set every partial is bit-identical to grad_sumsq_kernel's; chains only get
// shorter otherwise.
__device__ __forceinline__ float4 load_trainable(const float4* __restrict__ g4,
                                                 const uint8_t* __restrict__ flags, int64_t i) {
  if (flags[i >> (MMT_GROUP_CHUNK_SHIFT - 2)] & MMT_GROUP_FROZEN) return make_float4(0.f, 0.f, 0.f, 0.f);
  return g4[i];
}

__global__ __launch_bounds__(256) void grad_sumsq_groups_kernel(const float* __restrict__ g,
                                                                int64_t n,
                                                                const uint8_t* __restrict__ flags,
                                                                float* __restrict__ partial) {
  __shared__ float wsum[4];
  const int64_t n4 = n >> 2;
  const int64_t per = (n4 + GN_GRID - 1) / GN_GRID;
  const int64_t lo = std::min<int64_t>((int64_t)blockIdx.x * per, n4);
  const int64_t hi = std::min<int64_t>(lo + per, n4);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
  int64_t i = lo + threadIdx.x;
  for (; i + 768 < hi; i += 1024) {
    const float4 x0 = load_trainable(g4, flags, i), x1 = load_trainable(g4, flags, i + 256);
    const float4 x2 = load_trainable(g4, flags, i + 512), x3 = load_trainable(g4, flags, i + 768);
    sumsq_acc(a0, x0);
    sumsq_acc(a1, x1);
    sumsq_acc(a2, x2);
    sumsq_acc(a3, x3);
  }
  if (i < hi) sumsq_acc(a0, load_trainable(g4, flags, i));
  if (i + 256 < hi) sumsq_acc(a1, load_trainable(g4, flags, i + 256));
  if (i + 512 < hi) sumsq_acc(a2, load_trainable(g4, flags, i + 512));
  if (blockIdx.x == GN_GRID - 1 && (int64_t)threadIdx.x < (n & 3)) {
    const int64_t e = 4 * n4 + threadIdx.x;
    if (!(flags[e >> MMT_GROUP_CHUNK_SHIFT] & MMT_GROUP_FROZEN)) {
      const float t = g[e];
      a0.x = fmaf(t, t, a0.x);
    }
  }
  const float sx = (a0.x + a1.x) + (a2.x + a3.x), sy = (a0.y + a1.y) + (a2.y + a3.y);
  const float sz = (a0.z + a1.z) + (a2.z + a3.z), sw = (a0.w + a1.w) + (a2.w + a3.w);
  float s = (sx + sy) + (sz + sw);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

struct OptimCtl {
  mmt_lr_schedule_t sched;
  double grad_scale, max_norm;
  int skip_nonfinite;
};

__device__ double lr_schedule(const mmt_lr_schedule_t& sc, int64_t s) {
  if (sc.kind == MMT_SCHED_CONSTANT) return sc.peak_value;
  const int64_t W = sc.warmup_steps;
  if (s < W) return sc.init_value + (sc.peak_value - sc.init_value) * (double)s / (double)W;
  if (sc.kind == MMT_SCHED_WARMUP_COSINE) {
    const int64_t span = sc.decay_steps - W;
    const double c = (double)std::min<int64_t>(s - W, span);
    const double alpha = sc.end_value / sc.peak_value;
    const double cosine = 0.5 * (1.0 + cos(3.141592653589793 * c / (double)span));
    return sc.peak_value * ((1.0 - alpha) * cosine + alpha);
  }
  return sc.peak_value * sqrt(sc.timescale / ((double)(s - W) + sc.timescale));
}

// Launch 2 of mmt_optim_prepare: one workgroup adds the GN_GRID partials in double in a fixed
// order (a lane's GN_GRID / 256 partials in sequence, then a halving tree through LDS) and lane
// 0 writes the 8 opt words (include/mmt_api.h).
__global__ __launch_bounds__(256) void optim_finalise_kernel(const float* __restrict__ partial,
                                                             const int32_t* __restrict__ state,
                                                             float* __restrict__ opt,
                                                             const OptimCtl ctl) {
  __shared__ double red[256];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < GN_GRID / 256; ++j) acc += (double)partial[threadIdx.x + 256 * j];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double sumsq = red[0];
  const bool nonfinite = !isfinite(sumsq);
  const double norm = ctl.grad_scale * sqrt(sumsq);
  double clip = 1.0;
  if (ctl.max_norm > 0.0 && !(norm < ctl.max_norm)) clip = ctl.max_norm / norm;
  const bool skip = nonfinite && ctl.skip_nonfinite;
  opt[0] = (float)norm;
  opt[1] = (float)clip;
  opt[2] = (float)(ctl.grad_scale * clip);
  opt[3] = (float)lr_schedule(ctl.sched, (int64_t)state[1]);
  opt[4] = nonfinite ? 1.f : 0.f;
  opt[5] += skip ? 1.f : 0.f;
  opt[6] = skip ? 1.f : 0.f;
  opt[7] = 0.f;
}

// Transposed bf16 weight shadows: dst (cols, rows) = src (rows, cols)^T for a batch of matrices
// (desc: n x {src_off, dst_off, rows, cols, first_tile} elements / tiles), 64 x 64 tiles through a
// padded LDS tile; grid-stride over all tiles. Lets every dX product run as an NT GEMM.
__global__ __launch_bounds__(256) void transpose_bf16_batched_kernel(
    const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, const int64_t* __restrict__ desc,
    int n, int64_t total_tiles) {
  __shared__ bf16_t tile[64][66];
  for (int64_t t = blockIdx.x; t < total_tiles; t += gridDim.x) {
    int m = 0;
    while (m + 1 < n && desc[5 * (m + 1) + 4] <= t) ++m;
    const int64_t so = desc[5 * m], dso = desc[5 * m + 1];
    const int rows = (int)desc[5 * m + 2], cols = (int)desc[5 * m + 3];
    const int64_t lt = t - desc[5 * m + 4];
    const int tcols = (cols + 63) / 64;
    const int r0 = (int)(lt / tcols) * 64, c0 = (int)(lt % tcols) * 64;
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
      const int rr = i >> 6, cc = i & 63;
      if (r0 + rr < rows && c0 + cc < cols) tile[rr][cc] = src[so + (int64_t)(r0 + rr) * cols + c0 + cc];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
      const int cc = i >> 6, rr = i & 63;  // dst row = source column
      if (r0 + rr < rows && c0 + cc < cols) dst[dso + (int64_t)(c0 + cc) * rows + r0 + rr] = tile[rr][cc];
    }
  }
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ a, bf16_t* __restrict__ b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    b[i] = f2bf(a[i]);
}

__global__ void step_advance_kernel(int32_t* state) { state[1] += 1; }


// The LDS-table embedding-gradient kernel, in its deterministic form when the mode is on.
void launch_embed_table(dim3 grid, hipStream_t s, int B, int L, int D, int NI, int Q,
                        const int32_t* img_rows, const float* dx0, const int32_t* rtok,
                        const int32_t* ctok, float* drow_emb, float* dcol_emb) {
  static const bool attr_ = (hipFuncSetAttribute((const void*)embed_grad_kernel<false>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 160 * 1024) == hipSuccess &&
                             hipFuncSetAttribute((const void*)embed_grad_kernel<true>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 160 * 1024) == hipSuccess);
  (void)attr_;
  if (g_det_host.fx)
    hipLaunchKernelGGL(embed_grad_kernel<true>, grid, dim3(256), sizeof(long long) * 2 * Q * EMB_COLS,
                       s, B, L, D, NI, Q, img_rows, dx0, rtok, ctok, drow_emb, dcol_emb);
  else
    hipLaunchKernelGGL(embed_grad_kernel<false>, grid, dim3(256), sizeof(float) * 2 * Q * EMB_COLS,
                       s, B, L, D, NI, Q, img_rows, dx0, rtok, ctok, drow_emb, dcol_emb);
}

// deterministic mode: grad += shadow x 2^-36, shadow = 0 (elementwise: the result is independent
// of every ordering)
__global__ void det_flush_kernel(float* __restrict__ grad, long long* __restrict__ fx, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const long long q = fx[i];
    if (q != 0) {
      grad[i] += (float)((double)q * (1.0 / DET_SCALE));
      fx[i] = 0;
    }
  }
}

}  // namespace

extern "C" int mmt_seq_assemble_fwd(int B, int L, int D, const int32_t* row_src, const void* text,
                                    int T, const void* img, int NI, const int32_t* rtok,
                                    const int32_t* ctok, const float* row_emb, const float* col_emb,
                                    const float* readout_pe, const float* pe, void* x0,
                                    mmt_stream_t stream) {
  MMT_CHECK_ARG(row_src && x0 && pe && D > 0 && D % 8 == 0 && B > 0 && L > 0,
                "mmt_seq_assemble_fwd: args (D > 0, D %% 8 == 0)");
  MMT_CHECK_ARG((uintptr_t)text % 16 == 0 && (uintptr_t)img % 16 == 0 && (uintptr_t)x0 % 16 == 0,
                "mmt_seq_assemble_fwd: text, img and x0 must be 16-B aligned");
  const int64_t n = (int64_t)B * L * (D / 8);
  hipLaunchKernelGGL(seq_assemble_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     as_stream(stream), B, L, D, row_src, (const bf16_t*)text, T,
                     (const bf16_t*)img, NI, rtok, ctok, row_emb, col_emb, readout_pe, pe,
                     (float*)x0);
  MMT_CHECK_LAUNCH("mmt_seq_assemble_fwd");
  return MMT_OK;
}

extern "C" int mmt_seq_assemble_bwd(int B, int L, int D, const int32_t* row_src, const void* dx0,
                                    void* dtext, int T, void* dimg, int NI, const int32_t* rtok,
                                    const int32_t* ctok, const int32_t* img_rows, int Q,
                                    float* drow_emb, float* dcol_emb, float* dreadout_pe,
                                    mmt_stream_t stream) {
  MMT_CHECK_ARG(row_src && dx0 && D > 0 && D % 8 == 0 && B > 0 && L > 0,
                "mmt_seq_assemble_bwd: args (D > 0, D %% 8 == 0)");
  MMT_CHECK_ARG((uintptr_t)dx0 % 16 == 0 && (uintptr_t)dtext % 16 == 0 && (uintptr_t)dimg % 16 == 0,
                "mmt_seq_assemble_bwd: dx0, dtext and dimg must be 16-B aligned");
  // drow_emb = dcol_emb = NULL: the image tokens' gradients only (the position-embedding
  // gradients then come from mmt_patch_embed_grad)
  const bool emb = drow_emb || dcol_emb;
  MMT_CHECK_ARG(NI == 0 || !emb || (img_rows && rtok && ctok && drow_emb && dcol_emb && Q > 0 &&
                                    2 * Q * EMB_COLS * 4 <= 160 * 1024),
                "mmt_seq_assemble_bwd: image embedding arguments");
  MMT_CHECK_ARG(NI == 0 || !emb || !g_det_host.fx || 2 * Q * EMB_COLS * 8 <= 160 * 1024,
                "mmt_seq_assemble_bwd: Q too large for the deterministic table");
  const int64_t n = (int64_t)B * L * (D / 8);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(seq_assemble_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, s, B, L, D,
                     row_src, (const float*)dx0, (bf16_t*)dtext, T, (bf16_t*)dimg, NI, rtok, ctok,
                     drow_emb, dcol_emb, dreadout_pe);
  MMT_CHECK_LAUNCH("mmt_seq_assemble_bwd");
  if (NI > 0 && emb) {
    launch_embed_table(dim3((D + EMB_COLS - 1) / EMB_COLS, EMB_SPLIT), s, B, L, D, NI, Q, img_rows,
                       (const float*)dx0, rtok, ctok, drow_emb, dcol_emb);
    MMT_CHECK_LAUNCH("mmt_seq_assemble_bwd(embedding grads)");
  }
  return MMT_OK;
}

extern "C" int mmt_patch_embed_grad(int B, int L, int D, int I, int Himg, int P, int Q,
                                    const int32_t* img_rows, const void* dx0, const int32_t* rtok,
                                    const int32_t* ctok, float* drow_emb, float* dcol_emb,
                                    mmt_stream_t stream) {
  MMT_CHECK_ARG(img_rows && dx0 && rtok && ctok && drow_emb && dcol_emb && B > 0 && L > 0 &&
                    D > 0 && D % 8 == 0 && I > 0 && P > 0 && Himg >= P && Himg % P == 0 && Q > 1,
                "mmt_patch_embed_grad: args");
  const int PPD = Himg / P;
  int wmax = 1;  // widest token window (host float arithmetic = patch_positions_kernel's)
  for (int w = 0; w < PPD; ++w) {
    auto q = [&](int v) { return (int)floorf(((float)v / (float)Himg) * (float)(Q - 1)); };
    wmax = std::max(wmax, q((w + 1) * P) - q(w * P));
  }
  hipStream_t s = as_stream(stream);
  const int chunks = (D + EMB_COLS - 1) / EMB_COLS;
  const int splits = std::max(1, std::min(B, 1024 / (PPD * chunks * 2)));
  const dim3 grid(PPD, chunks, 2 * splits);
#define EGW(WM)                                                                                   \
  hipLaunchKernelGGL(embed_grad_win_kernel<WM>, grid, dim3(256), 0, s, B, L, D, I, PPD, Himg, P, \
                     Q, splits, img_rows, (const float*)dx0, rtok, ctok, drow_emb, dcol_emb)
  if (wmax <= 8) EGW(8);
  else if (wmax <= 16) EGW(16);
  else {  // wide windows: the LDS-atomic table kernel
    const int NI = I * PPD * PPD;
    MMT_CHECK_ARG(2 * Q * EMB_COLS * (g_det_host.fx ? 8 : 4) <= 160 * 1024,
                  "mmt_patch_embed_grad: Q too large%s", g_det_host.fx ? " for the deterministic table" : "");
    launch_embed_table(dim3(chunks, EMB_SPLIT), s, B, L, D, NI, Q, img_rows, (const float*)dx0, rtok,
                       ctok, drow_emb, dcol_emb);
  }
#undef EGW
  MMT_CHECK_LAUNCH("mmt_patch_embed_grad");
  return MMT_OK;
}

extern "C" int mmt_rows_mean_fwd(const void* x, int64_t xs_b, int64_t xs_t, int B, int D,
                                 const int32_t* rows, int nrows, void* out, int64_t ld_out,
                                 mmt_stream_t stream) {
  MMT_CHECK_ARG(x && rows && out && B > 0 && D > 0 && nrows > 0, "mmt_rows_mean_fwd: args");
  hipLaunchKernelGGL(rows_mean_fwd_kernel, dim3(B), dim3(256), 0, as_stream(stream),
                     (const float*)x, xs_b, xs_t, D, rows, nrows, (bf16_t*)out, ld_out);
  MMT_CHECK_LAUNCH("mmt_rows_mean_fwd");
  return MMT_OK;
}

extern "C" int mmt_rows_mean_bwd(const void* de, int64_t ld_de, int B, int L, int D,
                                 const int32_t* row_flag, int nrows, void* dx, mmt_stream_t stream) {
  MMT_CHECK_ARG(de && row_flag && dx && B > 0 && L > 0 && D > 0 && nrows > 0,
                "mmt_rows_mean_bwd: args");
  const int64_t n = (int64_t)B * L * D;
  hipLaunchKernelGGL(rows_mean_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream),
                     (const bf16_t*)de, ld_de, B, L, D, row_flag, nrows, (float*)dx);
  MMT_CHECK_LAUNCH("mmt_rows_mean_bwd");
  return MMT_OK;
}

extern "C" int mmt_rows_group_mean_fwd(const void* x, int64_t xs_b, int64_t xs_t, int B, int L,
                                       int D, const int32_t* row_group, int G,
                                       const int32_t* counts, void* out, mmt_stream_t stream) {
  MMT_CHECK_ARG(x && row_group && counts && out && B > 0 && L > 0 && D > 0 && G > 0,
                "mmt_rows_group_mean_fwd: args");
  hipLaunchKernelGGL(rows_group_mean_fwd_kernel, dim3(B, G), dim3(256), 0, as_stream(stream),
                     (const float*)x, xs_b, xs_t, L, D, row_group, G, counts, (bf16_t*)out);
  MMT_CHECK_LAUNCH("mmt_rows_group_mean_fwd");
  return MMT_OK;
}

extern "C" int mmt_rows_group_mean_bwd(const void* de, int B, int L, int D, const int32_t* row_group,
                                       int G, const int32_t* counts, void* dx, mmt_stream_t stream) {
  MMT_CHECK_ARG(de && row_group && counts && dx && B > 0 && L > 0 && D > 0 && G > 0,
                "mmt_rows_group_mean_bwd: args");
  const int64_t n = (int64_t)B * L * D;
  hipLaunchKernelGGL(rows_group_mean_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     as_stream(stream), (const bf16_t*)de, B, L, D, row_group, G, counts,
                     (float*)dx);
  MMT_CHECK_LAUNCH("mmt_rows_group_mean_bwd");
  return MMT_OK;
}

extern "C" int mmt_action_head(int kind, const float* z, int64_t ldz, int R, int N, const float* y,
                               const float* edges, int n_edges, float max_action, float inv_count,
                               float* pred, float* loss, void* dz, mmt_stream_t stream) {
  MMT_CHECK_ARG(z && R > 0 && N > 0 && ldz >= N && (kind == 0 || kind == 1),
                "mmt_action_head: args");
  MMT_CHECK_ARG(!y || (loss && dz), "mmt_action_head: a loss needs loss and dz outputs");
  MMT_CHECK_ARG(kind == 0 ? (max_action > 0.f && (y || pred)) : (y && edges && n_edges > 1),
                "mmt_action_head: kind %d arguments", kind);
  hipLaunchKernelGGL(action_head_kernel, dim3((R + 3) / 4), dim3(256), 0, as_stream(stream), kind,
                     z, ldz, R, N, y, edges, n_edges, max_action, inv_count, pred, loss,
                     (bf16_t*)dz);
  MMT_CHECK_LAUNCH("mmt_action_head");
  return MMT_OK;
}

extern "C" int mmt_transpose_bf16_batched(const void* src, void* dst, const int64_t* desc, int n,
                                          int64_t total_tiles, mmt_stream_t stream) {
  MMT_CHECK_ARG(src && dst && desc && n > 0 && total_tiles > 0, "mmt_transpose_bf16_batched: args");
  const int grid = (int)std::min<int64_t>(total_tiles, 4096);
  hipLaunchKernelGGL(transpose_bf16_batched_kernel, dim3(grid), dim3(256), 0, as_stream(stream),
                     (const bf16_t*)src, (bf16_t*)dst, desc, n, total_tiles);
  MMT_CHECK_LAUNCH("mmt_transpose_bf16_batched");
  return MMT_OK;
}

extern "C" int mmt_diffusion_prep(const uint32_t* rng, int B, int A, int steps,
                                  int64_t sample_offset, const float* actions,
                                  const float* alpha_hats, const float* fourier_w, int F,
                                  const int32_t* t_in, const float* eps_in, int32_t* t_out,
                                  float* eps_out, void* cat, int64_t ld_cat, void* feats,
                                  mmt_stream_t stream) {
  MMT_CHECK_ARG(actions && alpha_hats && fourier_w && t_out && eps_out && cat && feats && B > 0,
                "mmt_diffusion_prep: args");
  MMT_CHECK_ARG((t_in && eps_in) || rng, "mmt_diffusion_prep: need rng or injected (t, eps)");
  MMT_CHECK_ARG(steps > 0 && A > 0 && F > 0 && ld_cat >= A,
                "mmt_diffusion_prep: steps %d, A %d, F %d must be positive, ld_cat %lld >= A", steps,
                A, F, (long long)ld_cat);
  hipLaunchKernelGGL(diffusion_prep_kernel, dim3(B), dim3(256), 0, as_stream(stream), rng, B, A,
                     steps, sample_offset, actions, alpha_hats, fourier_w, F, t_in, eps_in, t_out,
                     eps_out, (bf16_t*)cat, ld_cat, (bf16_t*)feats);
  MMT_CHECK_LAUNCH("mmt_diffusion_prep");
  return MMT_OK;
}

extern "C" int mmt_fourier_bwd(const void* dfeats, int B, int F, const int32_t* t,
                               const float* fourier_w, float* dw, mmt_stream_t stream) {
  MMT_CHECK_ARG(dfeats && t && fourier_w && dw && B > 0 && F > 0, "mmt_fourier_bwd: args");
  hipLaunchKernelGGL(fourier_bwd_kernel, dim3((F + 63) / 64, (B + FB_B - 1) / FB_B), dim3(64), 0,
                     as_stream(stream),
                     (const bf16_t*)dfeats, B, F, t, fourier_w, dw);
  MMT_CHECK_LAUNCH("mmt_fourier_bwd");
  return MMT_OK;
}

extern "C" int mmt_diffusion_loss(const float* pred, int64_t ld_pred, const float* eps, int B,
                                  int A, float grad_scale, float* loss, void* dpred,
                                  mmt_stream_t stream) {
  MMT_CHECK_ARG(pred && eps && loss && dpred && B > 0 && A > 0, "mmt_diffusion_loss: args");
  MMT_CHECK_ARG(ld_pred >= A, "mmt_diffusion_loss: ld_pred %lld < A %d", (long long)ld_pred, A);
  MMT_CHECK_ARG((int64_t)B * A <= INT32_MAX, "mmt_diffusion_loss: B * A = %lld overflows int",
                (long long)B * A);
  hipLaunchKernelGGL(diffusion_loss_kernel, dim3(1), dim3(1024), 0, as_stream(stream), pred,
                     ld_pred, eps, B, A, grad_scale, loss, (bf16_t*)dpred);
  MMT_CHECK_LAUNCH("mmt_diffusion_loss");
  return MMT_OK;
}

extern "C" int mmt_rmsnorm_fwd(const void* x, int64_t rows, int D, const void* w, float eps,
                               void* y, mmt_stream_t stream) {
  MMT_CHECK_ARG(x && w && y && rows > 0 && D > 0 && D % 8 == 0,
                "mmt_rmsnorm_fwd: args (D > 0, D %% 8 == 0)");
  MMT_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)y % 16 == 0,
                "mmt_rmsnorm_fwd: x, w and y must be 16-B aligned");
  hipLaunchKernelGGL(rmsnorm_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream),
                     (const bf16_t*)x, rows, D, (const bf16_t*)w, eps, (bf16_t*)y);
  MMT_CHECK_LAUNCH("mmt_rmsnorm_fwd");
  return MMT_OK;
}

extern "C" int mmt_embedding_gather(const int32_t* ids, int64_t n, int D, const void* table,
                                    int vocab, void* out, mmt_stream_t stream) {
  MMT_CHECK_ARG(ids && table && out && n > 0 && D > 0 && D % 8 == 0 && vocab > 0,
                "mmt_embedding_gather: args (D > 0, D %% 8 == 0)");
  MMT_CHECK_ARG((uintptr_t)table % 16 == 0 && (uintptr_t)out % 16 == 0,
                "mmt_embedding_gather: table and out must be 16-B aligned");
  const int64_t t = n * (D / 8);
  hipLaunchKernelGGL(embedding_gather_kernel, dim3((t + 255) / 256), dim3(256), 0,
                     as_stream(stream), ids, n, D, (const bf16_t*)table, vocab, (bf16_t*)out);
  MMT_CHECK_LAUNCH("mmt_embedding_gather");
  return MMT_OK;
}

extern "C" int mmt_adamw(float* p, const float* g, float* m, float* v, void* shadow_bf16,
                         int64_t n, const int32_t* state, double lr, double b1, double b2,
                         double eps, double wd, float grad_scale, mmt_stream_t stream) {
  MMT_CHECK_ARG(p && g && m && v && state && n > 0, "mmt_adamw: args");
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 8);
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), p, g, m, v,
                     (bf16_t*)shadow_bf16, n, state, (float)lr, b1, b2, (float)eps, (float)wd,
                     grad_scale);
  MMT_CHECK_LAUNCH("mmt_adamw");
  return MMT_OK;
}

// Both prepare entry points: `who` names the caller in the messages, flags == nullptr is the
// plain form.
static int optim_prepare(const char* who, const float* g, int64_t n, float grad_scale,
                         double max_norm, int skip_nonfinite, const mmt_lr_schedule_t* sched,
                         const int32_t* state, float* opt, void* workspace, int64_t ws_bytes,
                         const uint8_t* flags, mmt_stream_t stream) {
  MMT_CHECK_ARG(g && sched && state && opt && workspace, "%s: null argument", who);
  MMT_CHECK_ARG(n > 0, "%s: n = %lld", who, (long long)n);
  MMT_CHECK_ARG((reinterpret_cast<uintptr_t>(g) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
                "%s: g must be 16-B aligned (workspace 4-B)", who);
  MMT_CHECK_ARG(ws_bytes >= mmt::grad_norm_workspace(n),
                "%s: workspace %lld B < %lld B (mmt_workspace_size)", who,
                (long long)ws_bytes, (long long)mmt::grad_norm_workspace(n));
  const mmt_lr_schedule_t& sc = *sched;
  MMT_CHECK_ARG(sc.kind == MMT_SCHED_CONSTANT || sc.kind == MMT_SCHED_WARMUP_COSINE ||
                    sc.kind == MMT_SCHED_WARMUP_RSQRT,
                "%s: unknown schedule kind %d", who, sc.kind);
  if (sc.kind != MMT_SCHED_CONSTANT)
    MMT_CHECK_ARG(sc.warmup_steps >= 1, "%s: warmup_steps %lld < 1", who,
                  (long long)sc.warmup_steps);
  if (sc.kind == MMT_SCHED_WARMUP_COSINE) {
    MMT_CHECK_ARG(sc.peak_value != 0.0, "%s: cosine peak_value 0 (alpha = end / peak)", who);
    MMT_CHECK_ARG(sc.decay_steps > sc.warmup_steps,
                  "%s: cosine decay_steps %lld <= warmup_steps %lld", who,
                  (long long)sc.decay_steps, (long long)sc.warmup_steps);
  }
  if (sc.kind == MMT_SCHED_WARMUP_RSQRT)
    MMT_CHECK_ARG(sc.timescale > 0.0, "%s: rsqrt timescale %g <= 0", who, sc.timescale);
  float* partial = static_cast<float*>(workspace);
  if (flags)
    hipLaunchKernelGGL(grad_sumsq_groups_kernel, dim3(GN_GRID), dim3(256), 0, as_stream(stream),
                       g, n, flags, partial);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(GN_GRID), dim3(256), 0, as_stream(stream), g, n,
                       partial);
  MMT_CHECK_LAUNCH(flags ? "mmt_optim_prepare_groups (partial sums)"
                         : "mmt_optim_prepare (partial sums)");
  const OptimCtl ctl{sc, (double)grad_scale, max_norm, skip_nonfinite != 0};
  hipLaunchKernelGGL(optim_finalise_kernel, dim3(1), dim3(256), 0, as_stream(stream),
                     (const float*)partial, state, opt, ctl);
  MMT_CHECK_LAUNCH(flags ? "mmt_optim_prepare_groups (finalise)" : "mmt_optim_prepare (finalise)");
  return MMT_OK;
}

extern "C" int mmt_optim_prepare(const float* g, int64_t n, float grad_scale, double max_norm,
                                 int skip_nonfinite, const mmt_lr_schedule_t* sched,
                                 const int32_t* state, float* opt, void* workspace,
                                 int64_t ws_bytes, mmt_stream_t stream) {
  return optim_prepare("mmt_optim_prepare", g, n, grad_scale, max_norm, skip_nonfinite, sched,
                       state, opt, workspace, ws_bytes, nullptr, stream);
}

extern "C" int mmt_optim_prepare_groups(const float* g, int64_t n, float grad_scale,
                                        double max_norm, int skip_nonfinite,
                                        const mmt_lr_schedule_t* sched, const int32_t* state,
                                        float* opt, void* workspace, int64_t ws_bytes,
                                        const uint8_t* chunk_flags, int chunk,
                                        mmt_stream_t stream) {
  MMT_CHECK_ARG(chunk_flags, "mmt_optim_prepare_groups: null chunk_flags");
  MMT_CHECK_ARG(chunk == MMT_GROUP_CHUNK, "mmt_optim_prepare_groups: chunk %d != %d", chunk,
                MMT_GROUP_CHUNK);
  return optim_prepare("mmt_optim_prepare_groups", g, n, grad_scale, max_norm, skip_nonfinite,
                       sched, state, opt, workspace, ws_bytes, chunk_flags, stream);
}

extern "C" int mmt_adamw_dev(float* p, const float* g, float* m, float* v, void* shadow_bf16,
                             int64_t n, const int32_t* state, const float* opt, double b1,
                             double b2, double eps, double wd, mmt_stream_t stream) {
  MMT_CHECK_ARG(p && g && m && v && state && opt && n > 0, "mmt_adamw_dev: args");
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 8);
  hipLaunchKernelGGL(adamw_dev_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), p, g, m, v,
                     (bf16_t*)shadow_bf16, n, state, opt, b1, b2, (float)eps, (float)wd);
  MMT_CHECK_LAUNCH("mmt_adamw_dev");
  return MMT_OK;
}

extern "C" int mmt_adamw_groups(float* p, const float* g, float* m, float* v, void* shadow_bf16,
                                int64_t n, const int32_t* state, const float* opt, double lr,
                                double b1, double b2, double eps, double wd, float grad_scale,
                                const uint8_t* chunk_flags, int chunk, mmt_stream_t stream) {
  MMT_CHECK_ARG(p && g && m && v && state && n > 0, "mmt_adamw_groups: args");
  MMT_CHECK_ARG(chunk_flags, "mmt_adamw_groups: null chunk_flags");
  MMT_CHECK_ARG(chunk == MMT_GROUP_CHUNK, "mmt_adamw_groups: chunk %d != %d", chunk,
                MMT_GROUP_CHUNK);
  // the same geometry as mmt_adamw: 256 lanes, so a wave's 64 elements are one chunk
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 8);
  if (opt)
    hipLaunchKernelGGL(adamw_groups_kernel<true>, dim3(blocks), dim3(256), 0, as_stream(stream), p,
                       g, m, v, (bf16_t*)shadow_bf16, n, state, opt, 0.f, b1, b2, (float)eps,
                       (float)wd, 0.f, chunk_flags);
  else
    hipLaunchKernelGGL(adamw_groups_kernel<false>, dim3(blocks), dim3(256), 0, as_stream(stream),
                       p, g, m, v, (bf16_t*)shadow_bf16, n, state, opt, (float)lr, b1, b2,
                       (float)eps, (float)wd, grad_scale, chunk_flags);
  MMT_CHECK_LAUNCH("mmt_adamw_groups");
  return MMT_OK;
}

extern "C" int mmt_adamw_ema(float* p, const float* g, float* m, float* v, void* shadow_bf16,
                             float* ema, int64_t n, const int32_t* state, const float* opt,
                             double lr, double b1, double b2, double eps, double wd,
                             float grad_scale, const uint8_t* chunk_flags, int chunk,
                             const mmt_ema_decay_t* decay, mmt_stream_t stream) {
  MMT_CHECK_ARG(p && g && m && v && state, "mmt_adamw_ema: null p, g, m, v or state");
  MMT_CHECK_ARG(ema, "mmt_adamw_ema: null ema");
  MMT_CHECK_ARG(decay, "mmt_adamw_ema: null decay");
  MMT_CHECK_ARG(n > 0, "mmt_adamw_ema: n = %lld", (long long)n);
  if (chunk_flags)
    MMT_CHECK_ARG(chunk == MMT_GROUP_CHUNK, "mmt_adamw_ema: chunk %d != %d", chunk,
                  MMT_GROUP_CHUNK);
  const mmt_ema_decay_t& dc = *decay;
  MMT_CHECK_ARG(dc.kind == MMT_EMA_CONSTANT || dc.kind == MMT_EMA_WARMUP,
                "mmt_adamw_ema: unknown decay kind %d", dc.kind);
  // negated comparisons: a NaN field is rejected too
  MMT_CHECK_ARG(dc.value >= 0.0 && dc.value <= 1.0, "mmt_adamw_ema: value %g outside [0, 1]",
                dc.value);
  MMT_CHECK_ARG(dc.max_value >= 0.0 && dc.max_value <= 1.0,
                "mmt_adamw_ema: max_value %g outside [0, 1]", dc.max_value);
  MMT_CHECK_ARG(dc.min_value >= 0.0 && dc.min_value <= 1.0,
                "mmt_adamw_ema: min_value %g outside [0, 1]", dc.min_value);
  if (dc.kind == MMT_EMA_WARMUP) {
    MMT_CHECK_ARG(dc.min_value <= dc.max_value, "mmt_adamw_ema: min_value %g > max_value %g",
                  dc.min_value, dc.max_value);
    MMT_CHECK_ARG(dc.inv_gamma > 0.0, "mmt_adamw_ema: inv_gamma %g <= 0", dc.inv_gamma);
    MMT_CHECK_ARG(dc.power >= 0.0, "mmt_adamw_ema: power %g < 0", dc.power);
    MMT_CHECK_ARG(dc.update_after_step >= 0, "mmt_adamw_ema: update_after_step %lld < 0",
                  (long long)dc.update_after_step);
  }
  // the geometry of mmt_adamw / mmt_adamw_dev / mmt_adamw_groups
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 8);
  bf16_t* sh = (bf16_t*)shadow_bf16;
  const float lrf = opt ? 0.f : (float)lr, gs = opt ? 0.f : grad_scale;
#define MMT_EMA_LAUNCH(kernel, ...)                                                            \
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, as_stream(stream), p, g, m, v, sh, ema, \
                     n, state, opt, lrf, b1, b2, (float)eps, (float)wd, gs, __VA_ARGS__)
  if (chunk_flags && opt)
    MMT_EMA_LAUNCH(adamw_groups_ema_kernel<true>, chunk_flags, dc);
  else if (chunk_flags)
    MMT_EMA_LAUNCH(adamw_groups_ema_kernel<false>, chunk_flags, dc);
  else if (opt)
    MMT_EMA_LAUNCH(adamw_ema_kernel<true>, dc);
  else
    MMT_EMA_LAUNCH(adamw_ema_kernel<false>, dc);
#undef MMT_EMA_LAUNCH
  MMT_CHECK_LAUNCH("mmt_adamw_ema");
  return MMT_OK;
}

extern "C" int mmt_ema_swap(float* p, float* ema, void* shadow_bf16, int64_t n,
                            const uint8_t* chunk_flags, int chunk, mmt_stream_t stream) {
  MMT_CHECK_ARG(p && ema, "mmt_ema_swap: null p or ema");
  MMT_CHECK_ARG(n > 0, "mmt_ema_swap: n = %lld", (long long)n);
  if (chunk_flags)
    MMT_CHECK_ARG(chunk == MMT_GROUP_CHUNK, "mmt_ema_swap: chunk %d != %d", chunk,
                  MMT_GROUP_CHUNK);
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 8);
  hipLaunchKernelGGL(ema_swap_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), p, ema,
                     (bf16_t*)shadow_bf16, n, chunk_flags);
  MMT_CHECK_LAUNCH("mmt_ema_swap");
  return MMT_OK;
}

extern "C" int mmt_cast_f32_bf16(const float* a, void* b, int64_t n, mmt_stream_t stream) {
  MMT_CHECK_ARG(a && b && n > 0, "mmt_cast_f32_bf16: args");
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 8);
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), a,
                     (bf16_t*)b, n);
  MMT_CHECK_LAUNCH("mmt_cast_f32_bf16");
  return MMT_OK;
}

extern "C" int mmt_step_advance(int32_t* state, mmt_stream_t stream) {
  MMT_CHECK_ARG(state, "mmt_step_advance: null");
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), state);
  MMT_CHECK_LAUNCH("mmt_step_advance");
  return MMT_OK;
}

// AddPositionEmbedding (tokenizers/readout/readout.py:18-33, attention.py:71-85): out[b, l, :] =
// x[b, l, :] + pe[l, :] (fp32, float4 lanes; x may alias out). The backward is the identity for x
// and mmt_colsum over the batch for pe.
__global__ void add_pe_kernel(const float4* __restrict__ x, const float4* __restrict__ pe,
                              float4* __restrict__ out, int64_t n4, int64_t per4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = x[i], p = pe[i % per4];
    out[i] = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
  }
}

extern "C" int mmt_add_position_embedding(const float* x, const float* pe, float* out, int B, int L,
                                          int D, mmt_stream_t stream) {
  MMT_CHECK_ARG(x && pe && out && B > 0 && L > 0 && D > 0 && D % 4 == 0 &&
                    (uintptr_t)x % 16 == 0 && (uintptr_t)pe % 16 == 0 && (uintptr_t)out % 16 == 0,
                "mmt_add_position_embedding: args (D %% 4 == 0, 16-B aligned)");
  const int64_t per4 = (int64_t)L * D / 4, n4 = per4 * B;
  const int64_t blocks = std::min<int64_t>((n4 + 255) / 256, 256 * 8);
  hipLaunchKernelGGL(add_pe_kernel, dim3(blocks), dim3(256), 0, as_stream(stream),
                     (const float4*)x, (const float4*)pe, (float4*)out, n4, per4);
  MMT_CHECK_LAUNCH("mmt_add_position_embedding");
  return MMT_OK;
}

namespace mmt {
int det_set_glue(const DetState& st) { return det_set_unit(st); }
}  // namespace mmt

extern "C" int mmt_det_flush(float* grad, long long* fx, int64_t n, mmt_stream_t stream) {
  MMT_CHECK_ARG(grad && fx && n >= 0, "mmt_det_flush: args");
  if (n == 0) return MMT_OK;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(det_flush_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), grad, fx, n);
  MMT_CHECK_LAUNCH("mmt_det_flush");
  return MMT_OK;
}
