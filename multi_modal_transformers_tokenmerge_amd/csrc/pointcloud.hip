// Point-cloud tokens (gfx950): a cloud (P, C) fp32 becomes n sequence rows, one per sampled
// centroid with its neighbourhood. The reference's tokenizers/pointclouds/point_cloud_tokenizer.py
// (farthest-point sampling :42-92, kNN grouping :106-116, SampleAndGroupModule :119-198), restated:
// semantics in include/mmt_api.h ("point-cloud tokens").
//
// mmt_pc_sample_group: one workgroup of 256 per cloud. Each thread keeps its points' xyz and
//   running distance in registers (xyz also in LDS, for the centroid broadcast and the grouping).
//   One FPS iteration = distance update, wave arg-max by shuffles over a packed u64
//   ((bits + 1) << 32 | ~index, 0 for a sampled point: one max gives the value and the lowest
//   index on ties), cross-wave arg-max through a double-buffered LDS slot with ONE barrier.
//   Grouping in the same launch: one wave per centroid holds the packed (d, index) keys of the
//   whole cloud in registers and takes k wave arg-mins, each over the keys above the last one.
//   mmt_pc_sample_group_counts: the same kernel's RAGGED instantiation, the leading counts[cloud]
//   rows of a cloud are its points (centroids repeat past the count, neighbour slots repeat slot 0).
// mmt_pc_embed_fwd: a group of F2 threads per token (thread = output column of layer 2, the k
//   neighbours in its registers, so the max over neighbours needs no exchange), two groups per
//   workgroup, 8 tokens per workgroup, W1 staged in LDS; the output Dense then runs for the 8
//   tokens together so one W_out load serves 8 FMAs.
// mmt_pc_embed_bwd: token chunks with one owner per partial-gradient element (registers),
//   partials to the workspace, then an ordered sum over the chunks added once into the gradients:
//   no float atomics, bitwise reproducible, independent of the deterministic mode.
#include <math.h>

#include <algorithm>

#include "common.h"

using namespace mmt;

namespace {

typedef unsigned long long u64;

// d(p, c): every operation individually rounded, so no FMA contraction (numpy float32 restates it).
// The __f*_rn intrinsics are plain operators in the HIP headers, and -ffp-contract=fast ignores
// `#pragma clang fp contract(off)`: compiled that way this became fma(dz, dz, dx dx) + dy dy, and
// two neighbours whose distances lie a rounding apart could change places against the restatement.
// So csrc/build.py compiles this file with -ffp-contract=off (every FMA in it is an explicit fmaf).
__device__ __forceinline__ float dist3(float px, float py, float pz, float cx, float cy, float cz) {
  const float dx = __fsub_rn(px, cx), dy = __fsub_rn(py, cy), dz = __fsub_rn(pz, cz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o) {
  const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = shfl_xor_u64(v, o);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = shfl_xor_u64(v, o);
    v = t < v ? t : v;
  }
  return v;
}

// PPT points per thread in the sampling phase (P <= 256 * PPT), 4 * PPT per lane in the grouping.
// RAGGED: counts[cloud] = c leading rows are points (clamped into [0, P]; outside:
// MMT_FAULT_ROW_INDEX); the rows >= c are never loaded. P stays the row stride and the sizing.
// Every `idx < Pv` below is `idx < P` in the instantiation without counts.
//   start    an injected start >= c: 0 and MMT_FAULT_ROW_INDEX; the draw is (u32 * c) >> 32
//   sampling the rule above over the rows < c for i < min(n, c); ids[i] = ids[i - c] past it
//   grouping the min(k, c) nearest among the rows < c; the slots r >= c repeat slot 0
//   c == 0   every index 0
template <int PPT, bool RAGGED>
__global__ __launch_bounds__(256) void pc_sample_group_kernel(
    const float* __restrict__ points, int64_t ld_b, int64_t ld_s, int S, int P, int C, int n, int k,
    const int32_t* __restrict__ start, const uint32_t* __restrict__ rng, int64_t sample_offset,
    const int32_t* __restrict__ counts, int32_t* __restrict__ cidx, int32_t* __restrict__ nidx,
    unsigned int* fault) {
  extern __shared__ __align__(16) unsigned char pc_smem[];
  u64* red = reinterpret_cast<u64*>(pc_smem);            // [2][4]
  int* cid = reinterpret_cast<int*>(pc_smem + 64);       // [n] (n <= 256)
  float* sx = reinterpret_cast<float*>(pc_smem + 64 + 1024);
  float* sy = sx + P;
  float* sz = sy + P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cloud = blockIdx.x, b = cloud / S, s = cloud - b * S;
  const float* base = points + (int64_t)b * ld_b + (int64_t)s * ld_s;

  int Pv = P;  // the rows that are points; block-uniform
  if (RAGGED) {
    Pv = counts[cloud];
    if ((unsigned)Pv > (unsigned)P) {
      Pv = Pv < 0 ? 0 : P;
      if (tid == 0) record_fault(fault, MMT_FAULT_ROW_INDEX);
    }
    if (Pv == 0) {  // an empty cloud: every index 0 (a start, any start, is outside it)
      if (start != nullptr && tid == 0) record_fault(fault, MMT_FAULT_ROW_INDEX);
      for (int e = tid; e < n; e += 256) cidx[(int64_t)cloud * n + e] = 0;
      for (int e = tid; e < n * k; e += 256) nidx[(int64_t)cloud * n * k + e] = 0;
      return;
    }
  }
  const int ns = RAGGED ? min(n, Pv) : n;  // sampled centroids, the rest repeat them
  const int kk = RAGGED ? min(k, Pv) : k;  // searched neighbours, the rest repeat slot 0

  float px[PPT], py[PPT], pz[PPT], dist[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int idx = j * 256 + tid;
    px[j] = py[j] = pz[j] = 0.f;
    dist[j] = INFINITY;
    if (idx < Pv) {
      const float* p = base + (int64_t)idx * C;
      px[j] = p[0], py[j] = p[1], pz[j] = p[2];
      sx[idx] = px[j], sy[idx] = py[j], sz[idx] = pz[j];
    }
  }
  int last = 0;
  if (start != nullptr) {
    last = start[cloud];
    if ((unsigned)last >= (unsigned)Pv) {
      last = 0;
      if (tid == 0) record_fault(fault, MMT_FAULT_ROW_INDEX);
    }
  } else if (rng != nullptr) {
    const uint32_t key = stream_key(rng[0], rng[1], 0xFFF7u, 1u);
    const uint32_t g = (uint32_t)((sample_offset + b) * S + s);
    last = (int)(((u64)draw_u32(key, g) * (u64)Pv) >> 32);
  }
  if (tid == 0) {
    cid[0] = last;
    cidx[(int64_t)cloud * n] = last;
  }
  __syncthreads();

  for (int i = 1; i < ns; ++i) {
    const float cx = sx[last], cy = sy[last], cz = sz[last];
    u64 best = 0;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int idx = j * 256 + tid;
      if (idx < Pv) {
        // a sampled point holds -1 from here on: fminf(-1, d) = -1 for every d >= 0 and for NaN
        const float d = idx == last ? -1.f
                                    : fminf(dist[j], dist3(px[j], py[j], pz[j], cx, cy, cz));
        dist[j] = d;
        const u64 key = d < 0.f ? 0ull
                                : ((u64)(__float_as_uint(d) + 1u) << 32) | (0xFFFFFFFFu - (uint32_t)idx);
        best = key > best ? key : best;
      }
    }
    best = wave_max_u64(best);
    u64* slot = red + (i & 1) * 4;  // double-buffered: one barrier per iteration is enough
    if (lane == 0) slot[wave] = best;
    __syncthreads();
    u64 m = slot[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = slot[w] > m ? slot[w] : m;
    last = (int)(0xFFFFFFFFu - (uint32_t)m);
    if ((unsigned)last >= (unsigned)Pv) last = 0;  // unreachable for n <= P; never out of bounds
    if (tid == 0) {
      cid[i] = last;
      cidx[(int64_t)cloud * n + i] = last;
    }
  }
  __syncthreads();
  if (RAGGED && ns < n) {  // ids[i] = ids[i - c] = ids[i mod c]: n <= 256, one thread per slot
    if (tid >= ns && tid < n) {
      const int v = cid[tid % ns];
      cid[tid] = v;
      cidx[(int64_t)cloud * n + tid] = v;
    }
    __syncthreads();
  }

  // grouping: wave per centroid, the k smallest (d, index) in ascending order
  constexpr int PPL = PPT * 4;
  for (int ci = wave; ci < n; ci += 4) {
    const int c = cid[ci];
    const float cx = sx[c], cy = sy[c], cz = sz[c];
    u64 key[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int idx = j * 64 + lane;
      key[j] = ~0ull;
      if (idx < Pv)
        key[j] = ((u64)__float_as_uint(dist3(sx[idx], sy[idx], sz[idx], cx, cy, cz)) << 32) |
                 (uint32_t)idx;
    }
    u64 lastk = 0;
    int first = 0;
    for (int r = 0; r < kk; ++r) {
      u64 loc = ~0ull;
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        const bool cand = r == 0 || key[j] > lastk;
        loc = (cand && key[j] < loc) ? key[j] : loc;
      }
      loc = wave_min_u64(loc);
      lastk = loc;
      int idx = (int)(uint32_t)loc;
      if ((unsigned)idx >= (unsigned)Pv) idx = 0;  // unreachable for k <= P
      if (RAGGED && r == 0) first = idx;
      if (lane == 0) nidx[((int64_t)cloud * n + ci) * k + r] = idx;
    }
    if (RAGGED && lane < k - kk)  // the slots past the cloud repeat slot 0 (k <= 32 < 64 lanes)
      nidx[((int64_t)cloud * n + ci) * k + kk + lane] = first;
  }
}

// A row of a (B, L, D) sequence addressed without L: row r of a sample lies inside the sample's
// xs_b elements iff r >= 0 and r * xs_t + D <= xs_b.
__device__ __forceinline__ bool row_inside(int r, int64_t xs_b, int64_t xs_t, int D) {
  return r >= 0 && (int64_t)r * xs_t + D <= xs_b;
}

constexpr int PC_TPB = 8;   // tokens per workgroup of the forward
constexpr int PC_PAD = 4;   // floats of padding per h1 row in LDS (keeps 16-B alignment)

struct PcShape {
  int S, P, C, n, k, F1, F2, D;
  int64_t T;  // tokens: B * S * n
};

// feat[j] = [points[nb_j] - points[c], points[nb_j]] of token tok into LDS (2C floats per row)
__device__ __forceinline__ void pc_features(const PcShape& sh, const float* __restrict__ points,
                                            int64_t ld_b, int64_t ld_s, int64_t tok,
                                            const int32_t* __restrict__ cidx,
                                            const int32_t* __restrict__ nidx, float* feat, int t0,
                                            int nt, unsigned int* fault) {
  const int64_t cloud = tok / sh.n;
  const int b = (int)(cloud / sh.S), s = (int)(cloud - (int64_t)b * sh.S);
  const float* base = points + (int64_t)b * ld_b + (int64_t)s * ld_s;
  const int pc = checked_index(cidx[tok], sh.P, fault, MMT_FAULT_ROW_INDEX);
  for (int e = t0; e < sh.k * sh.C; e += nt) {
    const int j = e / sh.C, c = e - j * sh.C;
    const int pj = checked_index(nidx[tok * sh.k + j], sh.P, fault, MMT_FAULT_ROW_INDEX);
    const float v = base[(int64_t)pj * sh.C + c], cv = base[(int64_t)pc * sh.C + c];
    feat[j * 2 * sh.C + c] = __fsub_rn(v, cv);
    feat[j * 2 * sh.C + sh.C + c] = v;
  }
}

// h1[j][i] = relu(feat[j] . W1[:, i] + b1[i]) into LDS rows of F1 + PC_PAD floats
__device__ __forceinline__ void pc_layer1(const PcShape& sh, const float* feat, const float* W1s,
                                          const float* b1s, float* h1, int t0, int nt) {
  const int C2 = 2 * sh.C;
  for (int e = t0; e < sh.k * sh.F1; e += nt) {
    const int j = e / sh.F1, i = e - j * sh.F1;
    float z = 0.f;
    for (int c = 0; c < C2; ++c) z = fmaf(feat[j * C2 + c], W1s[c * sh.F1 + i], z);
    h1[j * (sh.F1 + PC_PAD) + i] = fmaxf(z + b1s[i], 0.f);
  }
}

// z2 of one (neighbour row, column): the order of the forward's accumulation, so the backward's
// recomputed maximum has the forward's bits
__device__ __forceinline__ float pc_z2(const PcShape& sh, const float* h1row, const float* W2s,
                                       int ld_w2, const float* __restrict__ b2, int f) {
  float acc = 0.f;
#pragma unroll 8
  for (int i = 0; i < sh.F1; ++i) acc = fmaf(h1row[i], W2s[i * ld_w2 + f], acc);
  return acc + b2[f];
}

template <int KT>
__global__ __launch_bounds__(256) void pc_embed_fwd_kernel(PcShape sh, const float* __restrict__ points, int64_t ld_b,
                                    int64_t ld_s, const int32_t* __restrict__ cidx,
                                    const int32_t* __restrict__ nidx, const float* __restrict__ W1,
                                    const float* __restrict__ b1, const float* __restrict__ W2,
                                    const float* __restrict__ b2, const float* __restrict__ Wo,
                                    const float* __restrict__ bo, const float* __restrict__ pe,
                                    const int32_t* __restrict__ rows, float* __restrict__ x0,
                                    int64_t xs_b, int64_t xs_t, uint8_t* __restrict__ argmax,
                                    unsigned int* fault) {
  extern __shared__ __align__(16) unsigned char pc_smem[];
  const int C2 = 2 * sh.C, F1 = sh.F1, F2 = sh.F2, k = sh.k, HS = F1 + PC_PAD;
  float* W1s = reinterpret_cast<float*>(pc_smem);  // [2C][F1]
  float* b1s = W1s + C2 * F1;                      // [F1]
  float* gbuf = b1s + F1;                          // [PC_TPB][F2]
  float* grp0 = gbuf + PC_TPB * F2;                // per group: feat [32 * 2C] | h1 [KT][HS]
  const int gsz = 32 * C2 + KT * HS;
  const int tid = threadIdx.x, nthr = blockDim.x;  // 2 * F2 threads: two groups of F2
  const int grp = tid / F2, f = tid - grp * F2;
  float* feat = grp0 + grp * gsz;
  float* h1 = feat + 32 * C2;
  for (int e = tid; e < C2 * F1; e += nthr) W1s[e] = W1[e];
  for (int e = tid; e < F1; e += nthr) b1s[e] = b1[e];
  __syncthreads();

  for (int it = 0; it < PC_TPB / 2; ++it) {
    const int tl = it * 2 + grp;
    const int64_t tok = (int64_t)blockIdx.x * PC_TPB + tl;
    const bool valid = tok < sh.T;
    if (valid) pc_features(sh, points, ld_b, ld_s, tok, cidx, nidx, feat, f, F2, fault);
    __syncthreads();
    if (valid) pc_layer1(sh, feat, W1s, b1s, h1, f, F2);
    __syncthreads();
    float gmax = 0.f;
    if (valid) {
      float acc[KT];
#pragma unroll
      for (int j = 0; j < KT; ++j) acc[j] = 0.f;
      for (int i0 = 0; i0 < F1; i0 += 4) {
        // W2 from global memory (16 - 64 KB, L1 / L2 resident): staging it in LDS cost more in
        // occupancy than it saved in latency (measured)
        const float w0 = W2[(int64_t)(i0 + 0) * F2 + f], w1 = W2[(int64_t)(i0 + 1) * F2 + f];
        const float w2 = W2[(int64_t)(i0 + 2) * F2 + f], w3 = W2[(int64_t)(i0 + 3) * F2 + f];
        // all KT rows, no branch on k (the loads stay in flight together): the rows j >= k of
        // the LDS tile hold leftovers, their accumulators are never read
#pragma unroll
        for (int j = 0; j < KT; ++j) {
          const float4 h = *reinterpret_cast<const float4*>(h1 + j * HS + i0);
          acc[j] = fmaf(h.x, w0, acc[j]);
          acc[j] = fmaf(h.y, w1, acc[j]);
          acc[j] = fmaf(h.z, w2, acc[j]);
          acc[j] = fmaf(h.w, w3, acc[j]);
        }
      }
      const float bias = b2[f];
      int am = 0;
      gmax = fmaxf(acc[0] + bias, 0.f);
#pragma unroll
      for (int j = 1; j < KT; ++j) {
        if (j < k) {
          const float h2 = fmaxf(acc[j] + bias, 0.f);
          if (h2 > gmax) gmax = h2, am = j;  // the first neighbour that attains the maximum
        }
      }
      argmax[tok * F2 + f] = (uint8_t)am;
    }
    gbuf[tl * F2 + f] = gmax;
  }
  __syncthreads();

  // output Dense for the workgroup's tokens together: x0 row = (g . W_out + b_out) + pe[row]
  const int64_t tok0 = (int64_t)blockIdx.x * PC_TPB;
  const int SN = sh.S * sh.n;
  for (int d = tid; d < sh.D; d += nthr) {
    float acc[PC_TPB];
#pragma unroll
    for (int t = 0; t < PC_TPB; ++t) acc[t] = 0.f;
    for (int i0 = 0; i0 < F2; i0 += 8) {  // 8 loads of W_out in flight (F2 is a multiple of 32)
      float w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = Wo[(int64_t)(i0 + u) * sh.D + d];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int t = 0; t < PC_TPB; ++t) acc[t] = fmaf(gbuf[t * F2 + i0 + u], w[u], acc[t]);
    }
    const float bias = bo[d];
#pragma unroll
    for (int t = 0; t < PC_TPB; ++t) {
      const int64_t tok = tok0 + t;
      if (tok >= sh.T) break;
      const int64_t b = tok / SN;
      const int row = rows[tok - b * SN];
      if (!row_inside(row, xs_b, xs_t, sh.D)) {  // never written outside the sample
        if (d == 0) record_fault(fault, MMT_FAULT_ROW_INDEX);
        continue;
      }
      const float v = acc[t] + bias;
      x0[b * xs_b + (int64_t)row * xs_t + d] = v + pe[(int64_t)row * sh.D + d];
    }
  }
}

// ------------------------------------------------------------------------------------ backward
constexpr int PCB_NT = 256;   // threads of the token kernel
constexpr int PCB_TB = 8;     // tokens whose dg = dy . W_out^T is formed together
constexpr int PCB_A1 = 9;     // (2C + 1) * F1 <= 17 * 128 accumulators over 256 threads

// One workgroup = one chunk of `tpc` consecutive tokens, walked in ascending order. Every partial
// gradient element has one owner thread and lives in its registers: dW2 (EPT = F1 F2 / 256
// elements per thread: column f = tid % F2, rows tid / F2 + m 256 / F2), db2, dW1, db1. W2 sits
// in LDS with rows of F2 + 1 floats, conflict-free for lanes over f (z2) and over i (dh1). Also
// writes g (T, F2), the pooled activations, for the output Dense's gradient.
template <int EPT>
__global__ __launch_bounds__(PCB_NT) void pc_embed_bwd_token_kernel(
    PcShape sh, int tpc, const float* __restrict__ points, int64_t ld_b, int64_t ld_s,
    const int32_t* __restrict__ cidx, const int32_t* __restrict__ nidx,
    const uint8_t* __restrict__ argmax, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ Wo, const float* __restrict__ dx0, int64_t xs_b, int64_t xs_t,
    const int32_t* __restrict__ rows, float* __restrict__ g_ws, float* __restrict__ part,
    int64_t part_stride, unsigned int* fault) {
  extern __shared__ __align__(16) unsigned char pc_smem[];
  const int C2 = 2 * sh.C, F1 = sh.F1, F2 = sh.F2, k = sh.k, D = sh.D, HS = F1 + PC_PAD;
  const int LW = F2 + 1;
  float* W2s = reinterpret_cast<float*>(pc_smem);    // [F1][F2 + 1]
  float* W1s = W2s + (F1 * LW + 3) / 4 * 4;          // [2C][F1]
  float* b1s = W1s + C2 * F1;                        // [F1]
  float* feat = b1s + F1;                            // [32][2C]
  float* h1 = feat + 32 * C2;                        // [k][HS]
  const int ns = PCB_NT / F1;                        // slices of f in the dh1 step
  float* dh1 = h1 + k * HS;                          // [ns][k][HS]: one copy per slice of f
  float* dys = dh1 + ns * k * HS;                    // [PCB_TB][D]
  float* dgs = dys + PCB_TB * D;                     // [PCB_TB][F2]
  float* dz2s = dgs + PCB_TB * F2;                   // [F2]
  int* js = reinterpret_cast<int*>(dz2s + F2);       // [F2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int SN = sh.S * sh.n;
  const int64_t tok0 = (int64_t)blockIdx.x * tpc;
  const int64_t tok1 = tok0 + tpc < sh.T ? tok0 + tpc : sh.T;

  for (int e = tid; e < F1 * F2; e += PCB_NT) W2s[(e / F2) * LW + e % F2] = W2[e];
  for (int e = tid; e < C2 * F1; e += PCB_NT) W1s[e] = W1[e];
  for (int e = tid; e < F1; e += PCB_NT) b1s[e] = b1[e];
  float db2acc = 0.f;
  float acc2[EPT];
#pragma unroll
  for (int m = 0; m < EPT; ++m) acc2[m] = 0.f;
  const int f2 = tid % F2, q2 = tid / F2, st2 = PCB_NT / F2;  // this thread's dW2 elements
  float acc1[PCB_A1];
#pragma unroll
  for (int m = 0; m < PCB_A1; ++m) acc1[m] = 0.f;
  const int n1 = (C2 + 1) * F1;  // dW1 rows, then db1 as the row of an all-ones feature
  __syncthreads();

  for (int64_t tb = tok0; tb < tok1; tb += PCB_TB) {
    const int nb = (int)(tok1 - tb < PCB_TB ? tok1 - tb : PCB_TB);
    // the rows of dx0 of these tokens
    for (int e = tid; e < PCB_TB * D; e += PCB_NT) {
      const int t = e / D, d = e - t * D;
      float v = 0.f;
      if (t < nb) {
        const int64_t tok = tb + t, b = tok / SN;
        const int row = rows[tok - b * SN];
        if (row_inside(row, xs_b, xs_t, D)) v = dx0[b * xs_b + (int64_t)row * xs_t + d];
        else if (d == 0) record_fault(fault, MMT_FAULT_ROW_INDEX);
      }
      dys[e] = v;
    }
    __syncthreads();
    // dg[t][f] = sum_d dy[t][d] W_out[f][d]: wave per f, lanes over d, fixed shuffle tree
    for (int f = wave; f < F2; f += PCB_NT / 64) {
      float a[PCB_TB];
#pragma unroll
      for (int t = 0; t < PCB_TB; ++t) a[t] = 0.f;
#pragma unroll 2
      for (int d = lane; d < D; d += 64) {
        const float w = Wo[(int64_t)f * D + d];
#pragma unroll
        for (int t = 0; t < PCB_TB; ++t) a[t] = fmaf(dys[t * D + d], w, a[t]);
      }
      // 8 partials per lane -> one sum per token in a fixed tree of 10 shuffles: each of the
      // first three steps halves the tokens a lane carries, the last three sum the 8 lanes left
      float h4[4], h2[2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool hi = lane & 32;
        const float got = __shfl_xor(hi ? a[u] : a[u + 4], 32, 64);
        h4[u] = (hi ? a[u + 4] : a[u]) + got;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bool hi = lane & 16;
        const float got = __shfl_xor(hi ? h4[u] : h4[u + 2], 16, 64);
        h2[u] = (hi ? h4[u + 2] : h4[u]) + got;
      }
      float h1v;
      {
        const bool hi = lane & 8;
        const float got = __shfl_xor(hi ? h2[0] : h2[1], 8, 64);
        h1v = (hi ? h2[1] : h2[0]) + got;
      }
#pragma unroll
      for (int o = 4; o > 0; o >>= 1) h1v += __shfl_xor(h1v, o, 64);
      if ((lane & 7) == 0) {
        const int t = ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
        dgs[t * F2 + f] = h1v;
      }
    }
    __syncthreads();

    for (int t = 0; t < nb; ++t) {
      const int64_t tok = tb + t;
      pc_features(sh, points, ld_b, ld_s, tok, cidx, nidx, feat, tid, PCB_NT, fault);
      __syncthreads();
      pc_layer1(sh, feat, W1s, b1s, h1, tid, PCB_NT);
      for (int e = tid; e < ns * k * HS; e += PCB_NT) dh1[e] = 0.f;
      __syncthreads();
      if (tid < F2) {
        const int f = tid;
        const int j = checked_index((int)argmax[tok * F2 + f], k, fault, MMT_FAULT_ROW_INDEX);
        const float gv = fmaxf(pc_z2(sh, h1 + j * HS, W2s, LW, b2, f), 0.f);
        g_ws[tok * F2 + f] = gv;
        const float dz = gv > 0.f ? dgs[t * F2 + f] : 0.f;  // relu'(0) = 0
        dz2s[f] = dz;
        js[f] = j;
        db2acc += dz;
      }
      __syncthreads();
      // dW2[i][f] += h1[j*(f)][i] dz2[f]
      {
        const float dz = dz2s[f2];
        const float* hr = h1 + js[f2] * HS + q2;
#pragma unroll
        for (int m = 0; m < EPT; ++m) acc2[m] = fmaf(hr[m * st2], dz, acc2[m]);
      }
      // dh1[j*(f)][i] += dz2[f] W2[i][f]: thread (i, sl) walks slice sl of f in ascending order
      // into copy sl
      {
        const int i = tid % F1, sl = tid / F1, fs = F2 / ns;
        float* mine = dh1 + sl * k * HS + i;
        for (int f = sl * fs; f < (sl + 1) * fs; ++f) {
          float* p = mine + js[f] * HS;
          *p = fmaf(dz2s[f], W2s[i * LW + f], *p);
        }
      }
      __syncthreads();
      for (int e = tid; e < k * F1; e += PCB_NT) {  // dz1 = sum of the copies where z1 > 0
        const int j = e / F1, i = e - j * F1;
        float v = dh1[j * HS + i];
        for (int c = 1; c < ns; ++c) v += dh1[(c * k + j) * HS + i];
        dh1[j * HS + i] = h1[j * HS + i] > 0.f ? v : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < PCB_A1; ++m) {
        const int e = tid + PCB_NT * m;
        if (e < n1) {
          const int c = e / F1, i = e - c * F1;
          float a = acc1[m];
          if (c < C2) {
            for (int j = 0; j < k; ++j) a = fmaf(feat[j * C2 + c], dh1[j * HS + i], a);
          } else {
            for (int j = 0; j < k; ++j) a += dh1[j * HS + i];
          }
          acc1[m] = a;
        }
      }
      __syncthreads();
    }
  }
  // partials: dW2 (F1 F2) | db2 (F2) | dW1 (2C F1) | db1 (F1)
  float* out = part + (int64_t)blockIdx.x * part_stride;
#pragma unroll
  for (int m = 0; m < EPT; ++m) out[tid + PCB_NT * m] = acc2[m];  // = (q2 + m st2) * F2 + f2
  if (tid < F2) out[F1 * F2 + tid] = db2acc;
#pragma unroll
  for (int m = 0; m < PCB_A1; ++m) {
    const int e = tid + PCB_NT * m;
    if (e < n1) out[F1 * F2 + F2 + e] = acc1[m];
  }
}

// dW_out (F2, D) and db_out (D) partials of one token chunk x 64 columns: wave w holds the rows
// [w RPW, (w + 1) RPW) of the (F2 + 1, D) product [g | 1]^T dy, RPW = ceil((F2 + 1) / 4). The g
// values of a token are wave-uniform (scalar loads); 8 tokens' rows of dy are in flight at a time,
// added in ascending token order.
constexpr int PCB_OT = 8;
template <int PCB_RW>  // rows per wave: 9, 17, 33 for F2 = 32, 64, 128
__global__ __launch_bounds__(256) void pc_embed_bwd_out_kernel(
    PcShape sh, int tpc, const float* __restrict__ g_ws, const float* __restrict__ dx0,
    int64_t xs_b, int64_t xs_t, const int32_t* __restrict__ rows, float* __restrict__ part,
    int64_t part_stride) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int d = blockIdx.x * 64 + lane, F2 = sh.F2, D = sh.D, SN = sh.S * sh.n;
  const int r0 = wave * PCB_RW;
  const int64_t tok0 = (int64_t)blockIdx.y * tpc;
  const int64_t tok1 = tok0 + tpc < sh.T ? tok0 + tpc : sh.T;
  float acc[PCB_RW];
#pragma unroll
  for (int m = 0; m < PCB_RW; ++m) acc[m] = 0.f;
  for (int64_t tb = tok0; tb < tok1; tb += PCB_OT) {
    float dy[PCB_OT];
#pragma unroll
    for (int u = 0; u < PCB_OT; ++u) {
      const int64_t tok = tb + u < tok1 ? tb + u : tok1 - 1;
      const int64_t b = tok / SN;
      const int row = rows[tok - b * SN];
      dy[u] = 0.f;
      if (tb + u < tok1 && d < D && row_inside(row, xs_b, xs_t, D))
        dy[u] = dx0[b * xs_b + (int64_t)row * xs_t + d];
    }
#pragma unroll
    for (int u = 0; u < PCB_OT; ++u) {
      const int64_t tok = tb + u < tok1 ? tb + u : tok1 - 1;  // a slot past the end adds 0
      const float* g = g_ws + tok * F2;
#pragma unroll
      for (int m = 0; m < PCB_RW; ++m) {  // branch-free: row F2 is the all-ones column (db_out)
        const int r = r0 + m;
        const float gv = r < F2 ? g[r] : (r == F2 ? 1.f : 0.f);
        acc[m] = fmaf(gv, dy[u], acc[m]);
      }
    }
  }
  if (d < D) {
    float* out = part + (int64_t)blockIdx.y * part_stride;
#pragma unroll
    for (int m = 0; m < PCB_RW; ++m) {
      const int r = r0 + m;
      if (r <= F2) out[(int64_t)r * D + d] = acc[m];
    }
  }
}

// grad element += its partials summed over the chunks in ascending order (one writer, one add)
__global__ void pc_reduce_kernel(const float* __restrict__ part, int64_t part_stride, int nchunks,
                                 int64_t total, int64_t n0, float* __restrict__ g0, int64_t n1,
                                 float* __restrict__ g1, int64_t n2, float* __restrict__ g2,
                                 float* __restrict__ g3) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  float s = 0.f;
  for (int c = 0; c < nchunks; ++c) s += part[(int64_t)c * part_stride + e];
  if (e < n0) g0[e] += s;
  else if (e < n0 + n1) g1[e - n0] += s;
  else if (e < n0 + n1 + n2) g2[e - n0 - n1] += s;
  else g3[e - n0 - n1 - n2] += s;
}

bool pc_dims_ok(int P, int C, int n, int k) {
  return C >= MMT_PC_MIN_FEATURES && C <= MMT_PC_MAX_FEATURES && n >= 1 && n <= MMT_PC_MAX_TOKENS &&
         k >= 1 && k <= MMT_PC_MAX_NEIGHBOURS && P <= MMT_PC_MAX_POINTS && P >= std::max(n, k);
}
bool pc_width_ok(int F) { return F == 32 || F == 64 || F == 128; }
bool pc_raise_lds(const void* kernel) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) ==
         hipSuccess;
}

// token chunks of the backward: (chunks of the token kernel, its tokens per chunk, chunks of the
// output-Dense kernel, its tokens per chunk), functions of T alone
void pc_bwd_chunks(int64_t T, int* nch1, int* tpc1, int* nch2, int* tpc2) {
  int64_t t1 = (T + 511) / 512;
  t1 = (t1 + PCB_TB - 1) / PCB_TB * PCB_TB;
  *tpc1 = (int)t1;
  *nch1 = (int)((T + t1 - 1) / t1);
  int64_t t2 = std::max<int64_t>(16, (T + 255) / 256);
  *tpc2 = (int)t2;
  *nch2 = (int)((T + t2 - 1) / t2);
}

size_t pc_bwd_lds_bytes(int C, int k, int F1, int F2, int D) {
  const int C2 = 2 * C, HS = F1 + PC_PAD;
  return sizeof(float) * ((size_t)(F1 * (F2 + 1) + 3) / 4 * 4 + C2 * F1 + F1 + 32 * C2 +
                          (1 + PCB_NT / F1) * k * HS + PCB_TB * D + PCB_TB * F2 + 2 * F2);
}

}  // namespace

extern "C" int mmt_pc_sample_group_counts(const float* points, int64_t ld_b, int64_t ld_s, int B,
                                          int S, int P, int C, int n, int k, const int32_t* start,
                                          const uint32_t* rng, int64_t sample_offset,
                                          const int32_t* counts, int32_t* centroid_idx,
                                          int32_t* neighbour_idx, mmt_stream_t stream) {
  MMT_CHECK_ARG(points && centroid_idx && neighbour_idx, "mmt_pc_sample_group: null pointer");
  MMT_CHECK_ARG(B > 0 && S > 0 && (int64_t)B * S <= (1 << 24),
                "mmt_pc_sample_group: B, S must be > 0 (B * S <= 2^24)");
  MMT_CHECK_ARG(pc_dims_ok(P, C, n, k),
                "mmt_pc_sample_group: need max(n, k) <= P <= %d, 1 <= n <= %d, 1 <= k <= %d, "
                "%d <= C <= %d (P %d, C %d, n %d, k %d)", MMT_PC_MAX_POINTS, MMT_PC_MAX_TOKENS,
                MMT_PC_MAX_NEIGHBOURS, MMT_PC_MIN_FEATURES, MMT_PC_MAX_FEATURES, P, C, n, k);
  MMT_CHECK_ARG(ld_s >= (int64_t)P * C && (B == 1 || ld_b >= (S - 1) * ld_s + (int64_t)P * C) &&
                    sample_offset >= 0,
                "mmt_pc_sample_group: strides (ld_s >= P * C, ld_b covers the S clouds)");
  const size_t lds = 64 + 1024 + 3 * sizeof(float) * (size_t)P;
  const dim3 grid(B * S);
  // without counts: the instantiation in which every count is the constant P (the kernel as it
  // was before counts existed)
#define PC_SG(PPT, RAGGED)                                                                        \
  hipLaunchKernelGGL((pc_sample_group_kernel<PPT, RAGGED>), grid, dim3(256), lds,                 \
                     as_stream(stream), points, ld_b, ld_s, S, P, C, n, k, start, rng,            \
                     sample_offset, counts, centroid_idx, neighbour_idx, fault_word())
  if (counts == nullptr) {
    if (P <= 256) PC_SG(1, false);
    else if (P <= 1024) PC_SG(4, false);
    else PC_SG(16, false);
  } else {
    if (P <= 256) PC_SG(1, true);
    else if (P <= 1024) PC_SG(4, true);
    else PC_SG(16, true);
  }
#undef PC_SG
  MMT_CHECK_LAUNCH("mmt_pc_sample_group");
  return MMT_OK;
}

extern "C" int mmt_pc_sample_group(const float* points, int64_t ld_b, int64_t ld_s, int B, int S,
                                   int P, int C, int n, int k, const int32_t* start,
                                   const uint32_t* rng, int64_t sample_offset,
                                   int32_t* centroid_idx, int32_t* neighbour_idx,
                                   mmt_stream_t stream) {
  return mmt_pc_sample_group_counts(points, ld_b, ld_s, B, S, P, C, n, k, start, rng, sample_offset,
                                    nullptr, centroid_idx, neighbour_idx, stream);
}

#define PC_CHECK_EMBED(name, D)                                                                   \
  MMT_CHECK_ARG(B > 0 && S > 0 && (int64_t)B * S * n <= (1 << 28), name ": B, S must be > 0");    \
  MMT_CHECK_ARG(pc_dims_ok(P, C, n, k) && pc_width_ok(F1) && pc_width_ok(F2),                     \
                name ": limits (P %d, C %d, n %d, k %d, F1 %d, F2 %d)", P, C, n, k, F1, F2);      \
  MMT_CHECK_ARG(D > 0 && D % 4 == 0 && D <= MMT_PC_MAX_WIDTH,                                     \
                name ": D must be a multiple of 4 in 4 .. %d", MMT_PC_MAX_WIDTH);                 \
  MMT_CHECK_ARG(ld_s >= (int64_t)P * C && (B == 1 || ld_b >= (S - 1) * ld_s + (int64_t)P * C),    \
                name ": strides (ld_s >= P * C, ld_b covers the S clouds)");                      \
  MMT_CHECK_ARG(xs_t >= D && xs_b >= 0, name ": strides (xs_t >= D)")

extern "C" int mmt_pc_embed_fwd(const float* points, int64_t ld_b, int64_t ld_s, int B, int S,
                                int P, int C, int n, int k, const int32_t* centroid_idx,
                                const int32_t* neighbour_idx, int F1, int F2, const float* w1,
                                const float* b1, const float* w2, const float* b2,
                                const float* w_out, const float* b_out, const float* pe,
                                const int32_t* rows, int D, void* x0, int64_t xs_b, int64_t xs_t,
                                uint8_t* argmax, mmt_stream_t stream) {
  MMT_CHECK_ARG(points && centroid_idx && neighbour_idx && w1 && b1 && w2 && b2 && w_out && b_out &&
                    pe && rows && x0 && argmax, "mmt_pc_embed_fwd: null pointer");
  PC_CHECK_EMBED("mmt_pc_embed_fwd", D);
  PcShape sh{S, P, C, n, k, F1, F2, D, (int64_t)B * S * n};
  const int KT = k <= 16 ? 16 : 32, C2 = 2 * C;
  const size_t lds = sizeof(float) * ((size_t)C2 * F1 + F1 + PC_TPB * F2 +
                                      2 * (32 * C2 + KT * (F1 + PC_PAD)));
  const dim3 grid((unsigned)((sh.T + PC_TPB - 1) / PC_TPB)), block(2 * F2);
#define PC_FWD(KT_)                                                                               \
  hipLaunchKernelGGL(pc_embed_fwd_kernel<KT_>, grid, block, lds, as_stream(stream), sh, points,  \
                     ld_b, ld_s, centroid_idx, neighbour_idx, w1, b1, w2, b2, w_out, b_out, pe,   \
                     rows, (float*)x0, xs_b, xs_t, argmax, fault_word())
  if (KT == 16) PC_FWD(16);
  else PC_FWD(32);
#undef PC_FWD
  MMT_CHECK_LAUNCH("mmt_pc_embed_fwd");
  return MMT_OK;
}

extern "C" int64_t mmt_pc_embed_bwd_workspace(int B, int S, int n, int C, int F1, int F2, int D) {
  if (B <= 0 || S <= 0 || n <= 0 || C <= 0 || F1 <= 0 || F2 <= 0 || D <= 0) return MMT_ERR_INVALID;
  const int64_t T = (int64_t)B * S * n;
  int nch1, tpc1, nch2, tpc2;
  pc_bwd_chunks(T, &nch1, &tpc1, &nch2, &tpc2);
  const int64_t p1 = (int64_t)F1 * F2 + F2 + (2 * C + 1) * (int64_t)F1, p2 = (int64_t)(F2 + 1) * D;
  return (int64_t)sizeof(float) * (T * F2 + nch1 * p1 + nch2 * p2);
}

extern "C" int mmt_pc_embed_bwd(const void* dx0, int64_t xs_b, int64_t xs_t, const int32_t* rows,
                                int D, const float* points, int64_t ld_b, int64_t ld_s, int B, int S,
                                int P, int C, int n, int k, const int32_t* centroid_idx,
                                const int32_t* neighbour_idx, const uint8_t* argmax, int F1, int F2,
                                const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* w_out, float* dw1, float* db1, float* dw2, float* db2,
                                float* dw_out, float* db_out, void* workspace,
                                int64_t workspace_bytes, mmt_stream_t stream) {
  MMT_CHECK_ARG(dx0 && rows && points && centroid_idx && neighbour_idx && argmax && w1 && b1 && w2 &&
                    b2 && w_out && dw1 && db1 && dw2 && db2 && dw_out && db_out && workspace,
                "mmt_pc_embed_bwd: null pointer");
  PC_CHECK_EMBED("mmt_pc_embed_bwd", D);
  MMT_CHECK_ARG(workspace_bytes >= mmt_pc_embed_bwd_workspace(B, S, n, C, F1, F2, D) &&
                    aligned_to(workspace, 16),
                "mmt_pc_embed_bwd: workspace smaller than mmt_pc_embed_bwd_workspace or unaligned");
  PcShape sh{S, P, C, n, k, F1, F2, D, (int64_t)B * S * n};
  int nch1, tpc1, nch2, tpc2;
  pc_bwd_chunks(sh.T, &nch1, &tpc1, &nch2, &tpc2);
  const int64_t p1 = (int64_t)F1 * F2 + F2 + (2 * C + 1) * (int64_t)F1, p2 = (int64_t)(F2 + 1) * D;
  float* g_ws = (float*)workspace;
  float* part1 = g_ws + sh.T * F2;
  float* part2 = part1 + nch1 * p1;
  const size_t lds = pc_bwd_lds_bytes(C, k, F1, F2, D);
  MMT_CHECK_ARG(lds <= 160 * 1024, "mmt_pc_embed_bwd: D %d too wide for the token kernel's LDS", D);
  if (lds > 64 * 1024) {  // above the default dynamic-LDS limit: raise it for the kernel, once
    static bool raised = false;
    if (!raised) {
      if (!pc_raise_lds((const void*)pc_embed_bwd_token_kernel<4>) ||
          !pc_raise_lds((const void*)pc_embed_bwd_token_kernel<8>) ||
          !pc_raise_lds((const void*)pc_embed_bwd_token_kernel<16>) ||
          !pc_raise_lds((const void*)pc_embed_bwd_token_kernel<32>) ||
          !pc_raise_lds((const void*)pc_embed_bwd_token_kernel<64>)) {
        set_error("mmt_pc_embed_bwd: cannot raise the dynamic LDS limit");
        return MMT_ERR_HIP;
      }
      raised = true;
    }
  }
  hipStream_t s = as_stream(stream);
#define PC_BWD(EPT)                                                                               \
  hipLaunchKernelGGL(pc_embed_bwd_token_kernel<EPT>, dim3(nch1), dim3(PCB_NT), lds, s, sh, tpc1,  \
                     points, ld_b, ld_s, centroid_idx, neighbour_idx, argmax, w1, b1, w2, b2,     \
                     w_out, (const float*)dx0, xs_b, xs_t, rows, g_ws, part1, p1, fault_word())
  switch (F1 * F2 / PCB_NT) {  // dW2 elements per thread: 4 .. 64 for widths in {32, 64, 128}
    case 4: PC_BWD(4); break;
    case 8: PC_BWD(8); break;
    case 16: PC_BWD(16); break;
    case 32: PC_BWD(32); break;
    default: PC_BWD(64); break;
  }
#undef PC_BWD
#define PC_OUT(RW)                                                                              \
  hipLaunchKernelGGL(pc_embed_bwd_out_kernel<RW>, dim3((D + 63) / 64, nch2), dim3(256), 0, s, sh, \
                     tpc2, g_ws, (const float*)dx0, xs_b, xs_t, rows, part2, p2)
  if (F2 == 32) PC_OUT(9);
  else if (F2 == 64) PC_OUT(17);
  else PC_OUT(33);
#undef PC_OUT
  hipLaunchKernelGGL(pc_reduce_kernel, dim3((unsigned)((p1 + 255) / 256)), dim3(256), 0, s, part1,
                     p1, nch1, p1, (int64_t)F1 * F2, dw2, (int64_t)F2, db2, (int64_t)2 * C * F1, dw1,
                     db1);
  hipLaunchKernelGGL(pc_reduce_kernel, dim3((unsigned)((p2 + 255) / 256)), dim3(256), 0, s, part2,
                     p2, nch2, p2, (int64_t)F2 * D, dw_out, (int64_t)D, db_out, (int64_t)0,
                     (float*)nullptr, (float*)nullptr);
  MMT_CHECK_LAUNCH("mmt_pc_embed_bwd");
  return MMT_OK;
}
