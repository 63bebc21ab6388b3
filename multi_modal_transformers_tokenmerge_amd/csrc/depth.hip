// Depth-image back-projection (gfx950): a depth frame (H, W), uint16 or fp32, with pinhole
// intrinsics becomes a point cloud of at most P points and its count, the input of
// mmt_pc_sample_group_counts. Semantics in include/mmt_api.h ("depth back-projection"); every
// arithmetic operation is individually rounded (the __f*_rn intrinsics, and the file is built
// without FMA contraction), so numpy float32 restates the points bit for bit.
//
// mmt_depth_unproject: one workgroup of 1024 per image, two passes over the depth image as 16-B
// vectors (8 uint16 or 4 fp32 pixels per lane).
//   count  V = the valid pixels of the image (wave shuffles, one LDS exchange).
//   place  chunks of 1024 vectors in raster order. The rank of a lane's first valid pixel among
//          the valid pixels of the image = the running base of the chunks before + the totals of
//          the waves before (LDS, double-buffered: ONE barrier per chunk) + the valid pixels of the
//          lanes before (one wave ballot per vector element). The next chunk's vector is loaded
//          before the scan of this one; the second pass reads what the first left in the caches.
//          A pixel of rank j owns slot j when V <= P, else slot floor(j P / V) iff
//          (j P mod V) < P, which is the slot q with ceil(q V / P) == j: every slot has exactly one
//          writer, whatever the schedule. The slots >= min(V, P) are zeroed by other threads.
// The selection costs one 32-bit division per lane and chunk (the lane's first rank), then adds:
// j P < 2^20 * 2^12 and q V < 2^12 * 2^20 fit 32 bits.
#include <math.h>

#include "common.h"

using namespace mmt;

namespace {

constexpr int DU_NT = 1024;         // threads per workgroup
constexpr int DU_NW = DU_NT / 64;   // waves
constexpr int DU_MAX_PIXELS = 1 << 20;

struct DuParams {
  int H, W, nvec;  // nvec: 16-B vectors per image
  int P, C;
  float scale, zmin, zmax;
};

// the depth of element e of a vector as a float (uint16 -> float is exact)
template <bool F32>
__device__ __forceinline__ float du_depth(const uint4& v, int e) {
  const int i = F32 ? e : e >> 1;  // selects, not an indexed array: the vector stays in registers
  const uint32_t w = i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
  if (F32) return __uint_as_float(w);
  return (float)((w >> (16 * (e & 1))) & 0xffffu);
}

// bit e set: element e is a valid pixel. uint16: d != 0; fp32: d > 0 and finite (a NaN fails
// d > 0); both: z_min <= z <= z_max with z = d * scale.
template <bool F32>
__device__ __forceinline__ unsigned du_valid(const uint4& v, const DuParams& p) {
  constexpr int EPV = F32 ? 4 : 8;
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < EPV; ++e) {
    const float d = du_depth<F32>(v, e);
    const float z = __fmul_rn(d, p.scale);
    const bool ok = d > 0.f && d < INFINITY && z >= p.zmin && z <= p.zmax;
    m |= ok ? 1u << e : 0u;
  }
  return m;
}

struct DuCamera {
  float fx, fy, cx, cy;
  float pose[12];
  bool has_pose;
};

__device__ __forceinline__ void du_write(const DuParams& p, const DuCamera& cam, float d, int pixel,
                                         const uint8_t* __restrict__ rgb, float* __restrict__ out,
                                         int slot) {
  const int v = pixel / p.W, u = pixel - v * p.W;
  const float z = __fmul_rn(d, p.scale);
  const float x = __fdiv_rn(__fmul_rn(__fsub_rn((float)u, cam.cx), z), cam.fx);
  const float y = __fdiv_rn(__fmul_rn(__fsub_rn((float)v, cam.cy), z), cam.fy);
  float* o = out + (int64_t)slot * p.C;
  o[0] = x, o[1] = y, o[2] = z;
  if (cam.has_pose) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float* r = cam.pose + 4 * i;
      o[i] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r[0], x), __fmul_rn(r[1], y)),
                                 __fmul_rn(r[2], z)), r[3]);
    }
  }
  if (rgb != nullptr) {
    const uint8_t* c = rgb + (int64_t)pixel * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) o[3 + i] = __fdiv_rn((float)c[i], 255.f);
  }
}

template <bool F32>
__global__ __launch_bounds__(DU_NT) void depth_unproject_kernel(
    DuParams p, const uint4* __restrict__ depth, const float* __restrict__ intrinsics,
    const float* __restrict__ pose, const uint8_t* __restrict__ rgb, float* __restrict__ points,
    int32_t* __restrict__ counts) {
  constexpr int EPV = F32 ? 4 : 8;
  __shared__ int vsum[DU_NW];
  __shared__ int wsum[2][DU_NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t img = blockIdx.x;
  const uint4* src = depth + img * p.nvec;
  float* out = points + img * (int64_t)p.P * p.C;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);  // four or eight invalid pixels

  // ---- count: four loads in flight per thread
  int cnt = 0;
  for (int i0 = 0; i0 < p.nvec; i0 += 4 * DU_NT) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * DU_NT + tid;
      v[u] = i < p.nvec ? src[i] : zero;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) cnt += __popc(du_valid<F32>(v[u], p));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) vsum[wave] = cnt;
  __syncthreads();
  int V = 0;
#pragma unroll
  for (int w = 0; w < DU_NW; ++w) V += vsum[w];
  const int kept = V < p.P ? V : p.P;
  if (tid == 0) counts[img] = kept;
  // the slots no pixel owns
  for (int e = kept * p.C + tid; e < p.P * p.C; e += DU_NT) out[e] = 0.f;
  if (V == 0) return;

  // ---- place
  DuCamera cam;
  cam.fx = intrinsics[img * 4 + 0], cam.fy = intrinsics[img * 4 + 1];
  cam.cx = intrinsics[img * 4 + 2], cam.cy = intrinsics[img * 4 + 3];
  cam.has_pose = pose != nullptr;
#pragma unroll
  for (int i = 0; i < 12; ++i) cam.pose[i] = cam.has_pose ? pose[img * 12 + i] : 0.f;
  const uint8_t* rgb_img = rgb ? rgb + img * (int64_t)p.H * p.W * 3 : nullptr;
  const bool stride_pick = V > p.P;
  const uint32_t uV = (uint32_t)V, uP = (uint32_t)p.P;
  const unsigned long long below = (1ull << lane) - 1ull;

  int base = 0;  // valid pixels of the chunks before (workgroup-uniform)
  uint4 cur = tid < p.nvec ? src[tid] : zero;
  for (int i0 = 0; i0 < p.nvec; i0 += DU_NT) {
    const int i = i0 + tid;
    const uint4 nxt = i + DU_NT < p.nvec ? src[i + DU_NT] : zero;
    const unsigned m = du_valid<F32>(cur, p);
    int before = 0, wtot = 0;
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      const unsigned long long bal = __ballot((m >> e) & 1u);
      before += __popcll(bal & below);
      wtot += __popcll(bal);
    }
    int* ws = wsum[(i0 / DU_NT) & 1];  // double-buffered: one barrier per chunk is enough
    if (lane == 0) ws[wave] = wtot;
    __syncthreads();
    int woff = 0, ctot = 0;
#pragma unroll
    for (int w = 0; w < DU_NW; ++w) {
      const int t = ws[w];
      woff += w < wave ? t : 0;
      ctot += t;
    }
    if (m != 0u) {
      uint32_t j = (uint32_t)(base + woff + before);  // the rank of the lane's first valid pixel
      uint32_t q = j, rem = 0;
      if (stride_pick) {
        const uint32_t jp = j * uP;  // j < 2^20, P <= 2^12
        q = jp / uV;
        rem = jp - q * uV;
      }
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        if ((m >> e) & 1u) {
          // q < P always: j <= V - 1 gives floor(j P / V) <= P - 1; the guard costs nothing
          if (rem < uP && q < uP)
            du_write(p, cam, du_depth<F32>(cur, e), i * EPV + e, rgb_img, out, (int)q);
          if (stride_pick) {
            rem += uP;
            if (rem >= uV) rem -= uV, ++q;
          } else {
            ++q;  // V <= P: slot = rank
          }
        }
      }
    }
    base += ctot;
    cur = nxt;
  }
}

}  // namespace

extern "C" int mmt_depth_unproject(const void* depth, int depth_is_f32, int B, int S, int H, int W,
                                   const float* intrinsics, const float* pose, const uint8_t* rgb,
                                   float depth_scale, float z_min, float z_max, int P,
                                   float* points, int32_t* counts, mmt_stream_t stream) {
  const char* fn = "mmt_depth_unproject";
  MMT_CHECK_ARG(depth && intrinsics && points && counts, "%s: null pointer", fn);
  MMT_CHECK_ARG(B > 0 && S > 0 && (int64_t)B * S <= (1 << 24), "%s: B, S must be > 0 (B * S <= 2^24)",
                fn);
  MMT_CHECK_ARG(P >= 1 && P <= MMT_PC_MAX_POINTS, "%s: P %d outside 1 .. %d", fn, P,
                MMT_PC_MAX_POINTS);
  MMT_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W <= DU_MAX_PIXELS, "%s: H, W must be > 0, H * W <= 2^20 "
                "(H %d, W %d)", fn, H, W);
  const int epv = depth_is_f32 ? 4 : 8;
  MMT_CHECK_ARG(aligned_to(depth, 16) && (H * W) % epv == 0,
                "%s: images are read as 16-B vectors (depth 16-B aligned, H * W a multiple of %d)", fn,
                epv);
  // !(x > 0) and !(a <= b) also refuse NaN
  MMT_CHECK_ARG(depth_scale > 0.f && z_min <= z_max, "%s: need depth_scale > 0 and z_min <= z_max", fn);
  DuParams p{H, W, H * W / epv, P, rgb ? 6 : 3, depth_scale, z_min, z_max};
  const dim3 grid(B * S);
  if (depth_is_f32)
    hipLaunchKernelGGL(depth_unproject_kernel<true>, grid, dim3(DU_NT), 0, as_stream(stream), p,
                       (const uint4*)depth, intrinsics, pose, rgb, points, counts);
  else
    hipLaunchKernelGGL(depth_unproject_kernel<false>, grid, dim3(DU_NT), 0, as_stream(stream), p,
                       (const uint4*)depth, intrinsics, pose, rgb, points, counts);
  MMT_CHECK_LAUNCH(fn);
  return MMT_OK;
}
