// On-device image augmentation (gfx950): random resized crop (bilinear, corner-aligned) plus
// brightness, contrast and saturation jitter of uint8 camera frames (B, I, H, W, 3), one draw per
// (global sample, camera). Semantics in include/mmt_api.h ("image augmentation"); every float
// operation is individually rounded (the __f*_rn intrinsics, and the file is built without FMA
// contraction) and the contrast mean is an integer sum, so numpy float32 restates the pixels bit
// for bit whatever the schedule.
//
// mmt_image_augment: two launches.
//   stats  grid (B I, AUG_SPLIT): workgroup (img, s) sums the three channels of the source box of
//          its image over every AUG_SPLIT-th 16-B piece of the box rows (aligned 16-B loads, the
//          bytes outside the row segment masked) and writes ITS partial sums to the workspace: one
//          writer per word, no atomics, nothing to zero. Workgroup (img of slot 0, 0) also writes
//          params_out.
//   apply  grid (B I, ceil(H W / 4096)): a workgroup owns 4096 consecutive pixels of one image =
//          12 KiB of output. Thread t takes the pixels t, t + 256, ...: neighbouring lanes gather
//          neighbouring source pixels (the four neighbours of each pixel as bytes; a wave's
//          load touches a few cache lines, and the second read of a row comes from the caches),
//          add the AUG_SPLIT integer partials (any order gives the same), apply the colour chain
//          and put their three bytes into the tile in LDS; the tile then leaves as 16-B stores,
//          lane after lane, where the image's bytes start 16-B aligned (H W a multiple of 16,
//          every usual frame size), as bytes else and at an image's end. The draws and crop
//          parameters are recomputed per thread from the counter stream: a pure function of
//          (seed, step, sample, camera), no hand-off.
//          (A first form, 16 consecutive pixels per thread packed in registers, stored the same
//          vectors but spread each of a wave's byte gathers over 3 KiB: the call took 138 us
//          instead of 83 at 256 frames of 256 x 256; DESIGN.md, "Image augmentation".)
// Every index that addresses memory is clamped into its image, so device-side parameters of any
// value (NaN included) read and write inside the tensors.
#include <math.h>

#include "common.h"

using namespace mmt;

namespace {

constexpr int AUG_NT = 256;          // threads per workgroup
constexpr int AUG_NW = AUG_NT / 64;  // waves
constexpr int AUG_SPLIT = MMT_AUGMENT_SPLIT;  // partial sums per image
constexpr int AUG_PPT = 16;          // pixels per thread of the apply kernel
constexpr int AUG_TILE = AUG_NT * AUG_PPT;  // pixels per workgroup: 12 KiB of output, in LDS
constexpr uint32_t AUG_LAYER = 0xFFF6u;

struct AugDraw {
  float w, h, x0, y0, d, fc, fs;
};

// lo + u (hi - lo), each operation rounded
__device__ __forceinline__ float aug_lerp(float lo, float hi, float u) {
  return __fadd_rn(lo, __fmul_rn(u, __fsub_rn(hi, lo)));
}

// the draw of (global sample g, camera c): u_j = uniform01(key, (8 g + j) mod 2^32)
__device__ __forceinline__ AugDraw aug_draw(const uint32_t* __restrict__ rng, int64_t g, int c,
                                            const float* __restrict__ cam) {
  const uint32_t key = stream_key(rng[0], rng[1], AUG_LAYER, (uint32_t)c);
  const uint32_t ctr = (uint32_t)((uint64_t)g * 8u);
  float u[7];
#pragma unroll
  for (int j = 0; j < 7; ++j)
    u[j] = __fmul_rn((float)(draw_u32(key, ctr + (uint32_t)j) >> 8), 1.f / 16777216.f);
  const float* p = cam + c * 9;
  const float area = aug_lerp(p[0], p[1], u[0]);
  const float rho = aug_lerp(p[2], p[3], u[1]);
  AugDraw a;
  // sqrtf, not __fsqrt_rn: the intrinsic is the native 1-ulp instruction in this toolchain, the
  // library function the correctly rounded square root numpy computes
  a.w = fminf(1.f, sqrtf(__fmul_rn(area, rho)));
  a.h = fminf(1.f, sqrtf(__fdiv_rn(area, rho)));
  a.x0 = __fmul_rn(u[2], __fsub_rn(1.f, a.w));
  a.y0 = __fmul_rn(u[3], __fsub_rn(1.f, a.h));
  a.d = __fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(2.f, u[4]), 1.f), p[4]), 255.f);
  a.fc = aug_lerp(p[5], p[6], u[5]);
  a.fs = aug_lerp(p[7], p[8], u[6]);
  return a;
}

// Sample position of output index r along an axis of n pixels: s = org + float(r) step with
// org = x0 (n - 1); i0 = min(floor(s), n - 1), i1 = min(i0 + 1, n - 1), t = s - float(i0).
// The clamp into [0, n - 1] is made in float, before the conversion (for s in that range
// floor(min(s, n - 1)) is min(floor(s), n - 1)): no valid draw gives s < 0, a NaN becomes 0
// (fmaxf returns its other operand), and no value outside int's range is ever converted.
__device__ __forceinline__ void aug_axis(float org, float step, int n, int r, int& i0, int& i1,
                                         float& t) {
  const float s = __fadd_rn(org, __fmul_rn((float)r, step));
  i0 = (int)floorf(fminf(fmaxf(s, 0.f), (float)(n - 1)));
  i1 = min(i0 + 1, n - 1);
  t = __fsub_rn(s, (float)i0);
}

// the integer source box the crop reads: rows y0 .. y1, columns x0 .. x1 (inclusive)
struct AugBox {
  int y0, y1, x0, x1;
};
__device__ __forceinline__ AugBox aug_box(const AugDraw& a, int H, int W) {
  AugBox b;
  int i0, i1;
  float t;
  aug_axis(__fmul_rn(a.y0, (float)(H - 1)), a.h, H, 0, b.y0, i1, t);
  aug_axis(__fmul_rn(a.y0, (float)(H - 1)), a.h, H, H - 1, i0, b.y1, t);
  aug_axis(__fmul_rn(a.x0, (float)(W - 1)), a.w, W, 0, b.x0, i1, t);
  aug_axis(__fmul_rn(a.x0, (float)(W - 1)), a.w, W, W - 1, i0, b.x1, t);
  b.y1 = max(b.y1, b.y0), b.x1 = max(b.x1, b.x0);  // holds for every valid draw
  return b;
}

struct AugShape {
  int B, I, H, W, n_cam;
};

__global__ __launch_bounds__(AUG_NT) void augment_stats_kernel(
    AugShape sh, const uint8_t* __restrict__ images, const uint32_t* __restrict__ rng,
    int64_t sample_offset, const int32_t* __restrict__ image_camera,
    const float* __restrict__ cam_params, uint32_t* __restrict__ partials,
    float* __restrict__ params_out, unsigned int* fault) {
  __shared__ uint32_t wsum[AUG_NW][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x, part = blockIdx.y;
  const int b = img / sh.I, slot = img - b * sh.I;
  const int64_t g = sample_offset + b;
  if (params_out != nullptr && slot == 0 && part == 0 && tid < sh.n_cam) {
    const AugDraw a = aug_draw(rng, g, tid, cam_params);
    float* o = params_out + ((int64_t)b * sh.n_cam + tid) * 8;
    o[0] = a.w, o[1] = a.h, o[2] = a.x0, o[3] = a.y0, o[4] = a.d, o[5] = a.fc, o[6] = a.fs;
    o[7] = 0.f;
  }
  const int cam = checked_index(image_camera[slot], sh.n_cam, fault, MMT_FAULT_ROW_INDEX);
  const AugDraw a = aug_draw(rng, g, cam, cam_params);
  const AugBox box = aug_box(a, sh.H, sh.W);
  // the row segment [x0, x1] as bytes of the image; pieces = aligned 16-B vectors that cover it.
  // The images' base is 16-B aligned, so `ab` + a byte offset in the image aligns as its address.
  // Offsets in the image fit 32 bits (H W 3 <= 3 * 2^22).
  const int64_t base = (int64_t)img * sh.H * sh.W * 3;
  const uint8_t* src = images + base;
  const int ab = (int)(base & 15);
  const int img_bytes = sh.H * sh.W * 3;
  const int seg = (box.x1 - box.x0 + 1) * 3;
  const int ppr = (seg + 15) / 16 + 1;  // pieces per row, at least enough for any alignment
  const int rows = box.y1 - box.y0 + 1;
  const int items = rows * ppr;
  uint32_t acc[3] = {0, 0, 0};  // per channel
  for (int it = part * AUG_NT + tid; it < items; it += AUG_SPLIT * AUG_NT) {
    const int row = it / ppr, j = it - row * ppr;
    const int lo = ((box.y0 + row) * sh.W + box.x0) * 3, hi = lo + seg;
    const int o = ((lo + ab) & ~15) - ab + 16 * j;  // may start up to 15 bytes before lo
    if (o >= hi) continue;
    uint32_t w[4] = {0, 0, 0, 0};
    // a whole vector only inside this image (hence inside the tensor); bytes at the two ends
    if (o >= 0 && o + 16 <= img_bytes) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + o);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (o + e >= lo && o + e < hi) w[e >> 2] |= (uint32_t)src[o + e] << (8 * (e & 3));
    }
    const bool inner = o >= lo && o + 16 <= hi;
    uint32_t s0 = 0, s1 = 0, s2 = 0;  // the bytes at 0, 1, 2 mod 3 in the piece
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
      if (!inner && (o + e < lo || o + e >= hi)) byte = 0;
      if (e % 3 == 0) s0 += byte;
      else if (e % 3 == 1) s1 += byte;
      else s2 += byte;
    }
    // the channel of byte o + e is (o + e) mod 3: the image starts on a pixel
    const int ph = (o + 48) % 3;
    acc[0] += ph == 0 ? s0 : ph == 1 ? s2 : s1;
    acc[1] += ph == 0 ? s1 : ph == 1 ? s0 : s2;
    acc[2] += ph == 0 ? s2 : ph == 1 ? s1 : s0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    if (lane == 0) wsum[wave][k] = acc[k];
  }
  __syncthreads();
  if (tid < 4) {
    uint32_t t = 0;
    if (tid < 3)
      for (int w = 0; w < AUG_NW; ++w) t += wsum[w][tid];
    partials[((int64_t)img * AUG_SPLIT + part) * 4 + tid] = t;
  }
}

__device__ __forceinline__ float aug_bilerp(float p00, float p01, float p10, float p11, float tx,
                                            float ty) {
  const float top = __fadd_rn(p00, __fmul_rn(__fsub_rn(p01, p00), tx));
  const float bot = __fadd_rn(p10, __fmul_rn(__fsub_rn(p11, p10), tx));
  return __fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), ty));
}

__global__ __launch_bounds__(AUG_NT) void augment_apply_kernel(
    AugShape sh, const uint8_t* __restrict__ images, const uint32_t* __restrict__ rng,
    int64_t sample_offset, const int32_t* __restrict__ image_camera,
    const float* __restrict__ cam_params, const uint32_t* __restrict__ partials,
    uint8_t* __restrict__ out) {
  // the workgroup's AUG_TILE output pixels as bytes, then stored as 16-B vectors
  __shared__ uint4 tile4[AUG_TILE * 3 / 16];
  uint8_t* tile = reinterpret_cast<uint8_t*>(tile4);
  const int tid = threadIdx.x;
  const int img = blockIdx.x;
  const int HW = sh.H * sh.W;
  const int t0 = blockIdx.y * AUG_TILE;      // the tile's first pixel, in the image
  const int npx = min(AUG_TILE, HW - t0);    // >= 1 by the grid
  const int b = img / sh.I, slot = img - b * sh.I;
  const int cam = checked_index(image_camera[slot], sh.n_cam, nullptr, 0);  // stats reported it
  const AugDraw a = aug_draw(rng, sample_offset + b, cam, cam_params);
  const AugBox box = aug_box(a, sh.H, sh.W);
  // contrast mean of the box per channel, with the brightness shift: mb = m + d
  float mb[3];
  {
    const uint32_t* ps = partials + (int64_t)img * AUG_SPLIT * 4;
    const float n = (float)((box.y1 - box.y0 + 1) * (box.x1 - box.x0 + 1));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      uint32_t s = 0;
#pragma unroll
      for (int q = 0; q < AUG_SPLIT; ++q) s += ps[q * 4 + k];
      mb[k] = __fadd_rn(__fdiv_rn((float)s, n), a.d);
    }
  }
  const uint8_t* src = images + (int64_t)img * HW * 3;
  const float yorg = __fmul_rn(a.y0, (float)(sh.H - 1)), xorg = __fmul_rn(a.x0, (float)(sh.W - 1));
  // pixel k AUG_NT + tid of the tile: neighbouring lanes take neighbouring pixels, so a wave's
  // gathers fall into a few cache lines. (row, column) advance by AUG_NT pixels per step.
  const int dq = AUG_NT / sh.W, dm = AUG_NT - dq * sh.W;
  int r = (t0 + tid) / sh.W, c = (t0 + tid) - r * sh.W;
  // No guard on q < npx: past the image's end the row index only grows, every sample index is
  // clamped into the image and q stays inside the tile, so those lanes read valid bytes and
  // write tile bytes that are never stored; the loop body is straight-line code whose gathers
  // the compiler can issue ahead.
#pragma unroll 4
  for (int k = 0; k < AUG_PPT; ++k) {
    const int q = k * AUG_NT + tid;
    int iy, iy1, ix, ix1;
    float ty, tx;
    aug_axis(yorg, a.h, sh.H, r, iy, iy1, ty);
    aug_axis(xorg, a.w, sh.W, c, ix, ix1, tx);
    const uint8_t* row0 = src + iy * sh.W * 3;
    const uint8_t* row1 = src + iy1 * sh.W * 3;
    float v2[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v = aug_bilerp((float)row0[ix * 3 + ch], (float)row0[ix1 * 3 + ch],
                                 (float)row1[ix * 3 + ch], (float)row1[ix1 * 3 + ch], tx, ty);
      const float v1 = __fadd_rn(v, a.d);
      v2[ch] = __fadd_rn(__fmul_rn(__fsub_rn(v1, mb[ch]), a.fc), mb[ch]);
    }
    const float gray = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, v2[0]), __fmul_rn(0.587f, v2[1])),
                                 __fmul_rn(0.114f, v2[2]));
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v3 = __fadd_rn(gray, __fmul_rn(__fsub_rn(v2[ch], gray), a.fs));
      // one clamp, then round half to even; a NaN (no valid draw gives one) becomes 0
      tile[q * 3 + ch] = (uint8_t)(int)rintf(fminf(fmaxf(v3, 0.f), 255.f));
    }
    r += dq, c += dm;
    if (c >= sh.W) c -= sh.W, ++r;
  }
  __syncthreads();
  // the tile's 3 npx bytes: 16-B vectors where the image's bytes start 16-B aligned (a tile's
  // offset in its image, AUG_TILE * 3 bytes a tile, is a multiple of 16), bytes else and at the end
  uint8_t* dst = out + ((int64_t)img * HW + t0) * 3;
  const int nb = npx * 3;
  const bool vec = ((uintptr_t)dst & 15) == 0;
#pragma unroll
  for (int j = 0; j < AUG_TILE * 3 / 16 / AUG_NT; ++j) {
    const int o = (j * AUG_NT + tid) * 16;
    if (vec && o + 16 <= nb) {
      *reinterpret_cast<uint4*>(dst + o) = tile4[j * AUG_NT + tid];
    } else {
      for (int e = o; e < min(o + 16, nb); ++e) dst[e] = tile[e];
    }
  }
}

}  // namespace

extern "C" int64_t mmt_image_augment_workspace(int B, int I) {
  if (B < 1 || I < 1 || I > MMT_AUGMENT_MAX_IMAGES || (int64_t)B * I > MMT_AUGMENT_MAX_FRAMES) {
    set_error("mmt_image_augment_workspace: need B >= 1, 1 <= I <= %d, B * I <= %d (B %d, I %d)",
              MMT_AUGMENT_MAX_IMAGES, MMT_AUGMENT_MAX_FRAMES, B, I);
    return MMT_ERR_INVALID;
  }
  return (int64_t)B * I * AUG_SPLIT * 4 * (int64_t)sizeof(uint32_t);
}

extern "C" int mmt_image_augment(const uint8_t* images, int B, int I, int H, int W,
                                 const uint32_t* rng, int64_t sample_offset,
                                 const int32_t* image_camera, const float* cam_params, int n_cam,
                                 uint8_t* out, float* params_out, void* workspace,
                                 int64_t workspace_bytes, mmt_stream_t stream) {
  const char* fn = "mmt_image_augment";
  MMT_CHECK_ARG(images && rng && image_camera && cam_params && out && workspace,
                "%s: null pointer", fn);
  MMT_CHECK_ARG(B >= 1 && I >= 1 && I <= MMT_AUGMENT_MAX_IMAGES &&
                (int64_t)B * I <= MMT_AUGMENT_MAX_FRAMES,
                "%s: need B >= 1, 1 <= I <= %d, B * I <= %d (B %d, I %d)", fn,
                MMT_AUGMENT_MAX_IMAGES, MMT_AUGMENT_MAX_FRAMES, B, I);
  MMT_CHECK_ARG(H >= 1 && W >= 1 && H <= MMT_AUGMENT_MAX_SIDE && W <= MMT_AUGMENT_MAX_SIDE,
                "%s: H, W must be in 1 .. %d (H %d, W %d)", fn, MMT_AUGMENT_MAX_SIDE, H, W);
  MMT_CHECK_ARG(n_cam >= 1 && n_cam <= MMT_AUGMENT_MAX_CAMERAS, "%s: n_cam %d outside 1 .. %d", fn,
                n_cam, MMT_AUGMENT_MAX_CAMERAS);
  MMT_CHECK_ARG(aligned_to(images, 16) && aligned_to(out, 16) && aligned_to(workspace, 16),
                "%s: images, out and workspace must be 16-B aligned", fn);
  MMT_CHECK_ARG(aligned_to(rng, 4) && aligned_to(image_camera, 4) && aligned_to(cam_params, 4) &&
                aligned_to(params_out, 4),
                "%s: rng, image_camera, cam_params and params_out must be 4-B aligned", fn);
  const int64_t nbytes = (int64_t)B * I * H * W * 3;
  const uintptr_t s = (uintptr_t)images, d = (uintptr_t)out;
  MMT_CHECK_ARG(s + (uintptr_t)nbytes <= d || d + (uintptr_t)nbytes <= s,
                "%s: out overlaps images (no in-place form: the crop gathers)", fn);
  MMT_CHECK_ARG(sample_offset >= 0, "%s: sample_offset must be >= 0", fn);
  const int64_t need = mmt_image_augment_workspace(B, I);
  MMT_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)need);
  const AugShape sh{B, I, H, W, n_cam};
  uint32_t* partials = static_cast<uint32_t*>(workspace);
  hipLaunchKernelGGL(augment_stats_kernel, dim3(B * I, AUG_SPLIT), dim3(AUG_NT), 0,
                     as_stream(stream), sh, images, rng, sample_offset, image_camera, cam_params,
                     partials, params_out, fault_word());
  MMT_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(augment_apply_kernel, dim3(B * I, (H * W + AUG_TILE - 1) / AUG_TILE),
                     dim3(AUG_NT), 0, as_stream(stream), sh, images, rng, sample_offset,
                     image_camera, cam_params, partials, out);
  MMT_CHECK_LAUNCH(fn);
  return MMT_OK;
}
