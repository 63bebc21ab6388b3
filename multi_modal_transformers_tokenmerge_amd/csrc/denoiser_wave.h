// One wave per sample through the one-block denoiser: the core that the step-table sampler
// (sampler.hip) and the multi-draw diffusion loss (diffusion_loss.hip) are built around. Each of
// them wraps its own inner step (a table update, a (t, eps) draw with its backward) around
//   pre = W1x x + Q[t] + P[b];  h = relu(pre);  out = W2 h            (x, out: A values, H units)
//
// Layout: 256 threads = 4 waves = 4 samples per workgroup, the H hidden units spread over the
// lanes (unit j = lane + 64 u, u < nu = ceil(H / 64) <= 16). Nothing per-unit lives in registers
// (2 nu A weights would not fit): the bf16 W1x rows and W2 columns of all H units sit in LDS,
// staged once per workgroup as [H][AP] rows (AP = A, or A + 8 when A / 8 is even, so a lane's
// 16-B pieces land on distinct banks), and each lane reads the rows of its unit as 16-B vectors
// (LDSW). When they do not fit beside the waves' P and Q rows,
//   4 waves * 128 * nu * 4 B + 4 H AP B > 160 KB,
// the same loops read them from global memory, where L2 holds them (256 KB at A = 64, H = 1024).
// P[b] and Q[t] of a lane's units are parked in LDS (each lane reads back only what it wrote, so no
// barrier), so the rolled unit loop can index them.
//
// Sample state: with A8 = A / 8, lane l keeps the A8 components a = A8 (l >> 3) + i, i < A8, of
// the sample's vectors (the 8 lanes of a group hold copies). That is where the reduction of the A
// per-lane partial sums leaves them: three exchange stages (lane bits 5, 4, 3), each halving the
// vector a lane carries, then three butterflies on the A8 survivors: 5A/4 exchanges, not 6A. The
// matvec takes x[a] as a wave-uniform value (readlane from lane 8 (a / A8)).
//
// Every device helper is force-inlined into its kernel; operands are fp32, the weights the bf16
// shadow widened exactly.
#pragma once
#include "common.h"

namespace mmt {
namespace dw {

constexpr int NT = 256;                // 4 waves = 4 samples per workgroup
constexpr int MAXNU = 16;              // units per lane: H <= 1024
constexpr int LDS_LIMIT = 160 * 1024;  // dynamic LDS a workgroup may ask for

inline int ap(int A) { return (A / 8) % 2 ? A : A + 8; }
// dynamic LDS: hp, hq [4][64 nu] fp32, then (LDS form) w1s, w2s [H][AP] bf16
inline size_t lds_bytes(int A, int H, bool weights) {
  const size_t hq = (size_t)(NT / 64) * 128 * ((H + 63) / 64) * sizeof(float);
  return hq + (weights ? (size_t)4 * H * ap(A) : 0);
}
inline bool fits_lds(int A, int H) { return lds_bytes(A, H, true) <= (size_t)LDS_LIMIT; }
inline dim3 grid(int B) { return dim3((B + NT / 64 - 1) / (NT / 64)); }

template <int A8> constexpr int row_pitch() { return A8 % 2 ? 8 * A8 : 8 * A8 + 8; }  // AP

struct Lds {
  float* hp;          // P[b] of this wave's units
  float* hq;          // Q[t] of this wave's units
  const bf16_t* w1s;  // [H][AP] W1x rows
  const bf16_t* w2s;  // [H][AP] W2 columns, as rows
};

template <int A8>
__device__ __forceinline__ Lds carve(int H, int nu, int wave) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dw_smem[];
  Lds s;
  s.hp = reinterpret_cast<float*>(dw_smem) + wave * 128 * nu;
  s.hq = s.hp + 64 * nu;
  s.w1s = reinterpret_cast<const bf16_t*>(dw_smem + (size_t)(NT / 64) * 128 * nu * sizeof(float));
  s.w2s = s.w1s + (size_t)H * row_pitch<A8>();
  return s;
}

// Every wave of the workgroup stages, including those past the batch; ends in the kernel's only
// barrier, so a wave may leave right after it.
template <int A8>
__device__ __forceinline__ void stage_weights(const Lds& s, const bf16_t* w1, int64_t ld_w1,
                                              const bf16_t* w2, int H) {
  constexpr int A = 8 * A8, AP = row_pitch<A8>();
  bf16_t* const d1 = const_cast<bf16_t*>(s.w1s);
  bf16_t* const d2 = const_cast<bf16_t*>(s.w2s);
  for (int i = threadIdx.x; i < H * A8; i += NT) {
    const int j = i / A8, c = i - j * A8;
    *reinterpret_cast<uint4*>(d1 + j * AP + 8 * c) =
        *reinterpret_cast<const uint4*>(w1 + (int64_t)j * ld_w1 + 8 * c);
  }
  for (int i = threadIdx.x; i < H * A; i += NT) {
    const int a = i / H, j = i - a * H;
    d2[j * AP + a] = w2[i];  // transposed: unit j's column of W2 as a row
  }
  __syncthreads();
}

// Lane l of sample g (the global sample index): its place in its group of 8, the first component
// it keeps, and the counter of the one component it draws for its group.
template <int A8>
struct Lanes {
  int lane, sub, a0;
  uint32_t ctr;
  __device__ __forceinline__ Lanes(int lane_, int64_t g) : lane(lane_), sub(lane_ & 7) {
    a0 = A8 * (lane >> 3);
    const int a_draw = a0 + (sub < A8 ? sub : A8 - 1);
    ctr = (uint32_t)(g * (8 * A8) + a_draw);
  }
  // the group's A8 draws (lane sub drew component a0 + sub) to every lane of the group
  __device__ __forceinline__ void spread(float v, float (&out)[A8]) const {
#pragma unroll
    for (int i = 0; i < A8; ++i) out[i] = __shfl(v, (lane & ~7) | i, 64);
  }
};

// row[j] of this lane's units: hp at once, a row of Q in two halves so that the loads can be issued
// well before the values are parked. The addresses are clamped: all MAXNU loads of load_units are
// issued whatever nu is (those past nu re-read row[H-1], one cached word for the whole wave).
__device__ __forceinline__ void park_p(float* hp, const float* row, int H, int nu, int lane) {
#pragma unroll
  for (int u = 0; u < MAXNU; ++u)
    if (u < nu) hp[64 * u + lane] = row[min(lane + 64 * u, H - 1)];
}
__device__ __forceinline__ void load_units(const float* row, int H, int lane, float (&qn)[MAXNU]) {
#pragma unroll
  for (int u = 0; u < MAXNU; ++u) qn[u] = row[min(lane + 64 * u, H - 1)];
}
__device__ __forceinline__ void park_units(float* hq, const float (&qn)[MAXNU], int nu, int lane) {
#pragma unroll
  for (int u = 0; u < MAXNU; ++u)
    if (u < nu) hq[64 * u + lane] = qn[u];
}

// A row index of Q from the caller's data: out of range it is reported (MMT_FAULT_ROW_INDEX),
// replaced by row 0 and never followed. Wave-uniform by contract: returned in an SGPR.
__device__ __forceinline__ int checked_row(int t, int rows, int lane, unsigned int* fault) {
  if ((unsigned)t >= (unsigned)rows) {
    if (lane == 0) record_fault(fault, MMT_FAULT_ROW_INDEX);
    t = 0;
  }
  return __builtin_amdgcn_readfirstlane(t);
}

// the lane-held vector (component a in lane 8 (a / A8), slot a % A8) as A wave-uniform values
template <int A8>
__device__ __forceinline__ void broadcast(const float (&x)[A8], float (&xb)[8 * A8]) {
#pragma unroll
  for (int a = 0; a < 8 * A8; ++a)
    xb[a] = __builtin_bit_cast(
        float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x[a % A8]), 8 * (a / A8)));
}

// unit jj's W1x row / W2 column: a padded LDS row, or (streamed W1 only) the global row
template <int A8, bool LDSW>
__device__ __forceinline__ const bf16_t* w1_row(const Lds& s, const bf16_t* w1, int64_t ld_w1,
                                                int jj) {
  return LDSW ? s.w1s + jj * row_pitch<A8>() : w1 + (int64_t)jj * ld_w1;
}
template <int A8>
__device__ __forceinline__ const bf16_t* w2_row(const Lds& s, int jj) {
  return s.w2s + jj * row_pitch<A8>();
}

// acc + sum_a xb[a] r[a] over a row of A bf16 values read as 16-B pieces, in ascending a
template <int A8>
__device__ __forceinline__ float row_dot(const bf16_t* r, const float (&xb)[8 * A8], float acc) {
#pragma unroll
  for (int c = 0; c < A8; ++c) {
    const uint4 row = *reinterpret_cast<const uint4*>(r + 8 * c);
    const uint32_t rw[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc = fmaf(xb[8 * c + 2 * q], __uint_as_float(rw[q] << 16), acc);
      acc = fmaf(xb[8 * c + 2 * q + 1], __uint_as_float(rw[q] & 0xffff0000u), acc);
    }
  }
  return acc;
}

// e[a] += h W2[a][jj]: the unit's LDS row, or its column of the global (A, H) matrix
template <int A8, bool LDSW>
__device__ __forceinline__ void w2_accumulate(const Lds& s, const bf16_t* w2, int H, int jj, float h,
                                              float (&e)[8 * A8]) {
  if (LDSW) {
#pragma unroll
    for (int c = 0; c < A8; ++c) {
      const uint4 row = *reinterpret_cast<const uint4*>(w2_row<A8>(s, jj) + 8 * c);
      const uint32_t rw[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        e[8 * c + 2 * q] = fmaf(h, __uint_as_float(rw[q] << 16), e[8 * c + 2 * q]);
        e[8 * c + 2 * q + 1] = fmaf(h, __uint_as_float(rw[q] & 0xffff0000u), e[8 * c + 2 * q + 1]);
      }
    }
  } else {
#pragma unroll
    for (int a = 0; a < 8 * A8; ++a) e[a] = fmaf(h, bf2f(w2[(int64_t)a * H + jj]), e[a]);
  }
}

// One exchange of a reduction stage over lane bit o (up: this lane has it set): the lane keeps the
// half of the pair that its side of the bit owns and adds the partner's copy of that half.
__device__ __forceinline__ float exchange(float lo, float hi, bool up, int o) {
  // opaque to the optimiser: it otherwise folds the two selects into e[i + (up ? 0 : n)], a
  // lane-varying index into the register array (a compare-select chain over all of e)
  asm volatile("" : "+v"(lo), "+v"(hi));
  const float send = up ? lo : hi;
  const float keep = up ? hi : lo;
  return keep + __shfl_xor(send, o, 64);
}

// sum over the 64 lanes; lane l ends with components A8 (l >> 3) + i in e[i], i < A8
template <int A8>
__device__ __forceinline__ void reduce(float (&e)[8 * A8], int lane) {
  constexpr int A = 8 * A8;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int o = 32 >> s, n = A >> (s + 1);
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int i = 0; i < n; ++i) e[i] = exchange(e[i], e[i + n], up, o);
  }
#pragma unroll
  for (int i = 0; i < A8; ++i) {
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) e[i] += __shfl_xor(e[i], o, 64);
  }
}

// Host side. K names a kernel family: `template <int A8, bool LDSW> static auto kernel()` returns
// the __global__ function taking one Args by value. The LDS form's dynamic-LDS attribute is set
// once per instantiation.
template <typename K, int A8, typename Args>
void launch(bool lds, int B, size_t smem, hipStream_t s, const Args& p) {
  if (lds) {
    static const bool attr_ =
        (hipFuncSetAttribute((const void*)K::template kernel<A8, true>(),
                             hipFuncAttributeMaxDynamicSharedMemorySize, LDS_LIMIT), true);
    (void)attr_;
    hipLaunchKernelGGL((K::template kernel<A8, true>()), grid(B), dim3(NT), smem, s, p);
  } else {
    hipLaunchKernelGGL((K::template kernel<A8, false>()), grid(B), dim3(NT), smem, s, p);
  }
}
// A in 8 .. 64 step 8 (the caller's argument check); returns whether the LDS form ran
template <typename K, typename Args>
bool dispatch(int A, int H, int B, hipStream_t s, const Args& p) {
  const bool lds = fits_lds(A, H);
  const size_t smem = lds_bytes(A, H, lds);
  switch (A / 8) {
    case 1: launch<K, 1>(lds, B, smem, s, p); break;
    case 2: launch<K, 2>(lds, B, smem, s, p); break;
    case 3: launch<K, 3>(lds, B, smem, s, p); break;
    case 4: launch<K, 4>(lds, B, smem, s, p); break;
    case 5: launch<K, 5>(lds, B, smem, s, p); break;
    case 6: launch<K, 6>(lds, B, smem, s, p); break;
    case 7: launch<K, 7>(lds, B, smem, s, p); break;
    default: launch<K, 8>(lds, B, smem, s, p); break;
  }
  return lds;
}

}  // namespace dw
}  // namespace mmt
