// QK-norm (gfx950): flax.linen.LayerNorm(use_bias=False) over the head dimension of the projected
// queries and keys (SelfAttention.normalize_qk, the ViT-22B recipe; the reference's
// attention_blocks/compressed_attention.py:184-198), in place on the q and k thirds of the packed
// (rows, 3, H, Dh) QKV buffer. Semantics in include/mmt_api.h ("QK-norm").
//
// A head row is Dh contiguous elements; the 2 H head rows of q and k of one token are contiguous
// too (the first 2 H Dh elements of the token's row). LPR = Dh / 8 lanes share one head row, 8
// elements each, moved as 16-B vectors: one per lane in bf16 (lane j holds columns 8 j .. 8 j + 7),
// two in fp32 (columns 4 j .. 4 j + 3 and Dh / 2 + 4 j .. + 3, so each wave load stays contiguous
// over a lane group). A wave holds 64 / LPR head rows at once and two such groups per loop step;
// the row sums are __shfl_xor butterflies inside the lane group. Nothing is staged in LDS.
//
// Backward: the statistics are recomputed from the saved pre-norm rows. Each lane keeps the scale
// gradient of its 8 columns (q and k apart) over the rows it visits; the workgroup folds them in a
// fixed order (lane groups by butterfly, waves through LDS in ascending order) into one partial
// row of the workspace, and a second launch sums the partials of every column in a fixed order and
// adds the sum once to the gradient: one writer per element, no float atomics.
#include <algorithm>

#include "common.h"

using namespace mmt;

namespace {

constexpr int QKN_THREADS = 256;      // 4 waves per workgroup
constexpr int QKN_WAVES = QKN_THREADS / 64;
constexpr int QKN_EPL = 8;            // elements per lane
constexpr int QKN_UNROLL = 2;         // row groups a wave keeps in flight per loop step
constexpr int QKN_FWD_MAX_GRID = 2048;
constexpr int QKN_BWD_MAX_GRID = 1024;  // = the most partial rows of the workspace

// Column of element e (0 .. 7) of lane j of a lane group.
template <typename T, int DH> __device__ __forceinline__ int qkn_col(int j, int e) {
  if (sizeof(T) == 2) return 8 * j + e;
  return (e < 4 ? 0 : DH / 2) + 4 * j + (e & 3);
}

template <typename T> struct QknIO;
template <> struct QknIO<bf16_t> {
  // p: the head row's first element
  template <int DH> static __device__ __forceinline__ void load(const bf16_t* p, int j, float* v) {
    const uint4 w = *reinterpret_cast<const uint4*>(p + 8 * j);
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(u[i] << 16);
      v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  }
  template <int DH> static __device__ __forceinline__ void store(bf16_t* p, int j, const float* v) {
    uint32_t u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = (uint32_t)f2bf(v[2 * i]) | (uint32_t)f2bf(v[2 * i + 1]) << 16;
    *reinterpret_cast<uint4*>(p + 8 * j) = make_uint4(u[0], u[1], u[2], u[3]);
  }
};
template <> struct QknIO<float> {
  template <int DH> static __device__ __forceinline__ void load(const float* p, int j, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p + 4 * j);
    const float4 b = *reinterpret_cast<const float4*>(p + DH / 2 + 4 * j);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
  template <int DH> static __device__ __forceinline__ void store(float* p, int j, const float* v) {
    *reinterpret_cast<float4*>(p + 4 * j) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + DH / 2 + 4 * j) = make_float4(v[4], v[5], v[6], v[7]);
  }
};

// sum over the LPR lanes of a lane group (every lane of the group gets it)
template <int LPR> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A head row from the lane's 8 elements: x becomes x - mean(x), rs = 1 / sqrt(var + eps) with
// Flax's fast variance var = max(0, mean(x^2) - mean(x)^2). Both means are taken of d = x - c, c the
// row's first element: mean(d^2) - mean(d)^2 is the same number in exact arithmetic, and in fp32
// it no longer cancels the row's offset (a row of mean 8 and unit spread would lose 6 bits of
// var); x - mean(x) = d - mean(d). A constant row gives exactly 0 and var = 0.
template <int DH> __device__ __forceinline__ void row_stats(float* x, float eps, float& rs) {
  constexpr int LPR = DH / QKN_EPL;
  const int lane = threadIdx.x & 63;
  const float c = __shfl(x[0], lane - lane % LPR, 64);
  float s = 0.f, ss = 0.f;
#pragma unroll
  for (int e = 0; e < QKN_EPL; ++e) {
    x[e] -= c;
    s += x[e];
    ss += x[e] * x[e];
  }
  s = group_sum<LPR>(s);
  ss = group_sum<LPR>(ss);
  const float m = s * (1.f / DH);
  const float var = fmaxf(0.f, ss * (1.f / DH) - m * m);
  rs = rsqrtf(var + eps);
#pragma unroll
  for (int e = 0; e < QKN_EPL; ++e) x[e] -= m;
}

// The lane's 8 q-scale and 8 k-scale entries.
template <typename T, int DH>
__device__ __forceinline__ void load_scales(const float* qs, const float* ks, int j, float* sq,
                                            float* sk) {
#pragma unroll
  for (int e = 0; e < QKN_EPL; ++e) {
    sq[e] = qs[qkn_col<T, DH>(j, e)];
    sk[e] = ks[qkn_col<T, DH>(j, e)];
  }
}

// Head row r of the 2 H per token: element offset of its first element in qkv, and in qk_pre.
struct QknRow {
  int64_t off, off_pre;
  bool is_k, valid;
};
template <int DH>
__device__ __forceinline__ QknRow qkn_row(int64_t r, int64_t rows, int H, int64_t ld) {
  QknRow o;
  o.valid = r < rows;
  const int64_t rr = o.valid ? r : 0;
  const int64_t tok = rr / (2 * H);
  const int hh = (int)(rr - tok * (2 * H));
  o.is_k = hh >= H;
  o.off = tok * ld + (int64_t)hh * DH;
  o.off_pre = rr * DH;
  return o;
}

template <typename T, int DH>
__global__ __launch_bounds__(QKN_THREADS) void qk_norm_fwd_kernel(
    T* __restrict__ qkv, int64_t ld, int64_t rows, int H, const float* __restrict__ q_scale,
    const float* __restrict__ k_scale, float eps, T* __restrict__ qk_pre) {
  constexpr int LPR = DH / QKN_EPL, RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, j = lane % LPR, g = lane / LPR;
  const int64_t wave = (int64_t)blockIdx.x * QKN_WAVES + (threadIdx.x >> 6);
  const int64_t step = (int64_t)gridDim.x * QKN_WAVES * RPW * QKN_UNROLL;
  float sq[QKN_EPL], sk[QKN_EPL];
  load_scales<T, DH>(q_scale, k_scale, j, sq, sk);
  // r0: the wave's first row of this step (wave-uniform loop bound)
  for (int64_t r0 = wave * RPW * QKN_UNROLL; r0 < rows; r0 += step) {
    QknRow row[QKN_UNROLL];
    float x[QKN_UNROLL][QKN_EPL];
#pragma unroll
    for (int u = 0; u < QKN_UNROLL; ++u) {
      row[u] = qkn_row<DH>(r0 + u * RPW + g, rows, H, ld);
      if (row[u].valid) {
        QknIO<T>::template load<DH>(qkv + row[u].off, j, x[u]);
      } else {
#pragma unroll
        for (int e = 0; e < QKN_EPL; ++e) x[u][e] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < QKN_UNROLL; ++u) {
      // the pre-norm row as loaded (the fp32 round trip of a bf16 value is exact)
      if (qk_pre != nullptr && row[u].valid)
        QknIO<T>::template store<DH>(qk_pre + row[u].off_pre, j, x[u]);
      float rs;
      row_stats<DH>(x[u], eps, rs);
      float y[QKN_EPL];
#pragma unroll
      for (int e = 0; e < QKN_EPL; ++e) y[e] = x[u][e] * rs * (row[u].is_k ? sk[e] : sq[e]);
      if (row[u].valid) QknIO<T>::template store<DH>(qkv + row[u].off, j, y);
    }
  }
}

template <typename T, int DH>
__global__ __launch_bounds__(QKN_THREADS) void qk_norm_bwd_kernel(
    T* __restrict__ dqkv, int64_t ld, int64_t rows, int H, const T* __restrict__ qk_pre,
    const float* __restrict__ q_scale, const float* __restrict__ k_scale, float eps,
    float* __restrict__ partials) {
  constexpr int LPR = DH / QKN_EPL, RPW = 64 / LPR;
  __shared__ float red[QKN_WAVES][2 * DH];
  const int lane = threadIdx.x & 63, j = lane % LPR, g = lane / LPR, w = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * QKN_WAVES + w;
  const int64_t step = (int64_t)gridDim.x * QKN_WAVES * RPW * QKN_UNROLL;
  float sq[QKN_EPL], sk[QKN_EPL], aq[QKN_EPL], ak[QKN_EPL];
  load_scales<T, DH>(q_scale, k_scale, j, sq, sk);
#pragma unroll
  for (int e = 0; e < QKN_EPL; ++e) aq[e] = ak[e] = 0.f;
  for (int64_t r0 = wave * RPW * QKN_UNROLL; r0 < rows; r0 += step) {
    QknRow row[QKN_UNROLL];
    float x[QKN_UNROLL][QKN_EPL], dy[QKN_UNROLL][QKN_EPL];
#pragma unroll
    for (int u = 0; u < QKN_UNROLL; ++u) {
      row[u] = qkn_row<DH>(r0 + u * RPW + g, rows, H, ld);
      if (row[u].valid) {
        QknIO<T>::template load<DH>(qk_pre + row[u].off_pre, j, x[u]);
        QknIO<T>::template load<DH>(dqkv + row[u].off, j, dy[u]);
      } else {  // zeros: the row adds +0 to the scale gradients and is not stored
#pragma unroll
        for (int e = 0; e < QKN_EPL; ++e) x[u][e] = dy[u][e] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < QKN_UNROLL; ++u) {
      float rs;
      row_stats<DH>(x[u], eps, rs);
      if (!row[u].valid) rs = 0.f;  // eps = 0: no 0 * inf into the scale gradients
      float xh[QKN_EPL], gg[QKN_EPL], sg = 0.f, sgx = 0.f;
#pragma unroll
      for (int e = 0; e < QKN_EPL; ++e) {
        xh[e] = x[u][e] * rs;
        gg[e] = dy[u][e] * (row[u].is_k ? sk[e] : sq[e]);
        sg += gg[e];
        sgx += gg[e] * xh[e];
        const float c = dy[u][e] * xh[e];
        aq[e] += row[u].is_k ? 0.f : c;
        ak[e] += row[u].is_k ? c : 0.f;
      }
      const float mg = group_sum<LPR>(sg) * (1.f / DH), mgx = group_sum<LPR>(sgx) * (1.f / DH);
      float dx[QKN_EPL];
#pragma unroll
      for (int e = 0; e < QKN_EPL; ++e) dx[e] = rs * (gg[e] - mg - xh[e] * mgx);
      if (row[u].valid) QknIO<T>::template store<DH>(dqkv + row[u].off, j, dx);
    }
  }
  // the wave's column sums: butterfly over its lane groups, then lane group 0 writes them
#pragma unroll
  for (int e = 0; e < QKN_EPL; ++e) {
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {
      aq[e] += __shfl_xor(aq[e], o, 64);
      ak[e] += __shfl_xor(ak[e], o, 64);
    }
  }
  if (g == 0) {
#pragma unroll
    for (int e = 0; e < QKN_EPL; ++e) {
      red[w][qkn_col<T, DH>(j, e)] = aq[e];
      red[w][DH + qkn_col<T, DH>(j, e)] = ak[e];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * DH; c += QKN_THREADS) {
    float s = red[0][c];
#pragma unroll
    for (int i = 1; i < QKN_WAVES; ++i) s += red[i][c];
    partials[(int64_t)blockIdx.x * (2 * DH) + c] = s;
  }
}

// One wave per column c of the 2 Dh (q-scale columns, then k-scale): lane l sums the partial rows
// l, l + 64, ... in ascending order, the butterfly folds the 64 lane sums, lane 0 adds the total.
__global__ __launch_bounds__(64) void qk_norm_dscale_kernel(const float* __restrict__ partials,
                                                            int nparts, int Dh,
                                                            float* __restrict__ dq_scale,
                                                            float* __restrict__ dk_scale) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int p = lane; p < nparts; p += 64) s += partials[(int64_t)p * (2 * Dh) + c];
  s = wave_sum(s);
  if (lane == 0) {
    float* dst = c < Dh ? dq_scale + c : dk_scale + (c - Dh);
    *dst += s;
  }
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// workgroups for `rows` head rows: one unrolled step of every wave covers the rows, up to `cap`
inline int qkn_grid(int64_t rows, int Dh, int cap) {
  const int64_t per_wg = (int64_t)QKN_WAVES * (64 / (Dh / QKN_EPL)) * QKN_UNROLL;
  return (int)std::min<int64_t>(cap, std::max<int64_t>(1, ceil_div(rows, per_wg)));
}

inline bool qkn_width_ok(int Dh) { return Dh == 32 || Dh == 64 || Dh == 128 || Dh == 256; }

// the shared argument rules of the two entry points; 0 or MMT_ERR_INVALID with the message set
int qkn_check(const char* name, const void* buf, int dtype, int64_t ld, int64_t rows, int H, int Dh,
              const float* q_scale, const float* k_scale, float eps) {
  MMT_CHECK_ARG(buf && q_scale && k_scale, "%s: null pointer", name);
  MMT_CHECK_ARG(dtype == MMT_F32 || dtype == MMT_BF16, "%s: dtype %d is neither MMT_F32 nor MMT_BF16",
                name, dtype);
  MMT_CHECK_ARG(qkn_width_ok(Dh), "%s: Dh %d not in {32, 64, 128, 256}", name, Dh);
  MMT_CHECK_ARG(rows > 0 && H > 0 && H <= 4096 && rows <= INT64_MAX / (8 * (int64_t)H * Dh),
                "%s: rows and H must be > 0 (H <= 4096)", name);
  MMT_CHECK_ARG(ld >= 3 * (int64_t)H * Dh, "%s: ld %lld < 3 H Dh = %lld", name, (long long)ld,
                3LL * H * Dh);
  const int64_t esz = dtype == MMT_BF16 ? 2 : 4;
  MMT_CHECK_ARG(aligned_to(buf, 16) && (ld * esz) % 16 == 0,
                "%s: rows must be 16-B aligned (base pointer and ld)", name);
  MMT_CHECK_ARG(eps >= 0.f && eps == eps, "%s: eps must be >= 0", name);
  return MMT_OK;
}

template <typename T>
void launch_fwd(int Dh, int grid, hipStream_t s, T* qkv, int64_t ld, int64_t rows, int H,
                const float* qs, const float* ks, float eps, T* pre) {
#define QKN_FWD(DH)                                                                              \
  hipLaunchKernelGGL((qk_norm_fwd_kernel<T, DH>), dim3(grid), dim3(QKN_THREADS), 0, s, qkv, ld, \
                     rows, H, qs, ks, eps, pre)
  switch (Dh) {
    case 32: QKN_FWD(32); break;
    case 64: QKN_FWD(64); break;
    case 128: QKN_FWD(128); break;
    default: QKN_FWD(256); break;
  }
#undef QKN_FWD
}

template <typename T>
void launch_bwd(int Dh, int grid, hipStream_t s, T* dqkv, int64_t ld, int64_t rows, int H,
                const T* pre, const float* qs, const float* ks, float eps, float* partials) {
#define QKN_BWD(DH)                                                                               \
  hipLaunchKernelGGL((qk_norm_bwd_kernel<T, DH>), dim3(grid), dim3(QKN_THREADS), 0, s, dqkv, ld, \
                     rows, H, pre, qs, ks, eps, partials)
  switch (Dh) {
    case 32: QKN_BWD(32); break;
    case 64: QKN_BWD(64); break;
    case 128: QKN_BWD(128); break;
    default: QKN_BWD(256); break;
  }
#undef QKN_BWD
}

}  // namespace

extern "C" int mmt_qk_norm_fwd(void* qkv, int dtype, int64_t ld, int64_t n_tokens, int H, int Dh,
                               const float* q_scale, const float* k_scale, float eps, void* qk_pre,
                               mmt_stream_t stream) {
  const int rc = qkn_check("mmt_qk_norm_fwd", qkv, dtype, ld, n_tokens, H, Dh, q_scale, k_scale, eps);
  if (rc != MMT_OK) return rc;
  MMT_CHECK_ARG(qk_pre == nullptr || aligned_to(qk_pre, 16),
                "mmt_qk_norm_fwd: qk_pre must be 16-B aligned");
  const int64_t rows = n_tokens * 2 * H;
  const int grid = qkn_grid(rows, Dh, QKN_FWD_MAX_GRID);
  if (dtype == MMT_BF16)
    launch_fwd<bf16_t>(Dh, grid, as_stream(stream), (bf16_t*)qkv, ld, rows, H, q_scale, k_scale, eps,
                       (bf16_t*)qk_pre);
  else
    launch_fwd<float>(Dh, grid, as_stream(stream), (float*)qkv, ld, rows, H, q_scale, k_scale, eps,
                      (float*)qk_pre);
  MMT_CHECK_LAUNCH("mmt_qk_norm_fwd");
  return MMT_OK;
}

extern "C" int64_t mmt_qk_norm_bwd_workspace(int64_t n_tokens, int H, int Dh) {
  MMT_CHECK_ARG(n_tokens > 0 && H > 0 && qkn_width_ok(Dh),
                "mmt_qk_norm_bwd_workspace: n_tokens, H must be > 0, Dh in {32, 64, 128, 256}");
  return (int64_t)qkn_grid(n_tokens * 2 * H, Dh, QKN_BWD_MAX_GRID) * 2 * Dh * (int64_t)sizeof(float);
}

extern "C" int mmt_qk_norm_bwd(void* dqkv, int dtype, int64_t ld, int64_t n_tokens, int H, int Dh,
                               const void* qk_pre, const float* q_scale, const float* k_scale,
                               float eps, float* dq_scale, float* dk_scale, void* workspace,
                               int64_t workspace_bytes, mmt_stream_t stream) {
  const int rc = qkn_check("mmt_qk_norm_bwd", dqkv, dtype, ld, n_tokens, H, Dh, q_scale, k_scale, eps);
  if (rc != MMT_OK) return rc;
  MMT_CHECK_ARG(qk_pre && dq_scale && dk_scale && workspace, "mmt_qk_norm_bwd: null pointer");
  MMT_CHECK_ARG(aligned_to(qk_pre, 16) && aligned_to(workspace, 16),
                "mmt_qk_norm_bwd: qk_pre and workspace must be 16-B aligned");
  const int64_t rows = n_tokens * 2 * H;
  const int grid = qkn_grid(rows, Dh, QKN_BWD_MAX_GRID);
  MMT_CHECK_ARG(workspace_bytes >= (int64_t)grid * 2 * Dh * (int64_t)sizeof(float),
                "mmt_qk_norm_bwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)grid * 2 * Dh * (long long)sizeof(float));
  float* partials = (float*)workspace;
  if (dtype == MMT_BF16)
    launch_bwd<bf16_t>(Dh, grid, as_stream(stream), (bf16_t*)dqkv, ld, rows, H, (const bf16_t*)qk_pre,
                       q_scale, k_scale, eps, partials);
  else
    launch_bwd<float>(Dh, grid, as_stream(stream), (float*)dqkv, ld, rows, H, (const float*)qk_pre,
                      q_scale, k_scale, eps, partials);
  MMT_CHECK_LAUNCH("mmt_qk_norm_bwd");
  hipLaunchKernelGGL(qk_norm_dscale_kernel, dim3(2 * Dh), dim3(64), 0, as_stream(stream), partials,
                     grid, Dh, dq_scale, dk_scale);
  MMT_CHECK_LAUNCH("mmt_qk_norm_bwd");
  return MMT_OK;
}
