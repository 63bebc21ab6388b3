// Observation pad masks (gfx950): absent token sets and padded instruction tokens. A masked token
// (a token of a set flagged absent for its sample, or a padded token of the text set) is never a
// key with weight, its content is never read and it sends no gradient to a tokenizer. Semantics
// in include/mmt_api.h ("observation pad masks") and DESIGN.md.
//
// The attention kernels are not touched: the mask enters them as the key_bias of
// mmt_attn_fwd_keybias / mmt_attn_bwd_keybias, MMT_PAD_MASK_LOGIT on the masked keys.
//   pack      bool (B, n_sets) -> one word of present-bits per sample (Readout sets forced present)
//   pack_counts  the same, with the bit of a PointCloud set cleared where the sample's cloud has
//             fewer valid points than the set has tokens (counts are read on the device)
//   bias      the key_bias rows of one layer from the words, the layer's set table and the text mask
//   images    a copy of the camera images with the pixels of absent cameras zeroed (the stem's
//             GroupNorm runs over all patches of all cameras of a sample)
//   rows_fwd  x0[b, l] = pe[l] on the masked rows of the assembled sequence
//   rows_bwd  dx0[b, l] = 0 on them
// A layer's set table travels by value (at most 16 sets); the set of a row is found by a scan of
// it. The row kernels give one wave a row at a time and move it as 16-B vectors; rows of present
// tokens are neither read nor written.
#include "common.h"

using namespace mmt;

namespace {

struct PadSets {
  int n;
  int start[MMT_PAD_MASK_MAX_SETS];
  int len[MMT_PAD_MASK_MAX_SETS];
};

// Is row l of sample b masked? word: the sample's present-bits (all ones without a set mask);
// text: the sample's row of the text mask (NULL: none), one byte per token of set text_set.
__device__ __forceinline__ bool row_masked(const PadSets& s, int l, uint32_t word,
                                           const uint8_t* __restrict__ text, int text_set) {
  int si = 0;
#pragma unroll 1
  for (int k = 1; k < s.n; ++k)
    if (l >= s.start[k]) si = k;   // starts ascend; an empty set shares its start with the next
  if (!((word >> si) & 1u)) return true;
  return text != nullptr && si == text_set && text[l - s.start[si]] == 0;
}

__global__ void pad_mask_pack_kernel(const uint8_t* __restrict__ mask, int B, int n_sets,
                                     uint32_t readout_bits, uint32_t* __restrict__ words,
                                     unsigned int* fault) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint32_t w = 0;
  for (int s = 0; s < n_sets; ++s)
    if (mask[(int64_t)b * n_sets + s]) w |= 1u << s;
  if (~w & readout_bits) {  // a Readout set flagged absent: reported, treated as present
    record_fault(fault, MMT_FAULT_PAD_MASK);
    w |= readout_bits;
  }
  words[b] = w;
}

struct CountSets {
  int S;
  int set[MMT_PAD_MASK_MAX_SETS];
  int min_points[MMT_PAD_MASK_MAX_SETS];
};

// pack, then bit cs.set[s] cleared where counts[b, s] < cs.min_points[s]. mask NULL: all present.
__global__ void pad_mask_pack_counts_kernel(const uint8_t* __restrict__ mask, int B, int n_sets,
                                            uint32_t readout_bits, CountSets cs,
                                            const int32_t* __restrict__ counts,
                                            uint32_t* __restrict__ words, unsigned int* fault) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint32_t w = 0;
  if (mask == nullptr) {
    w = n_sets >= 32 ? 0xffffffffu : (1u << n_sets) - 1u;
  } else {
    for (int s = 0; s < n_sets; ++s)
      if (mask[(int64_t)b * n_sets + s]) w |= 1u << s;
    if (~w & readout_bits) {  // a Readout set flagged absent: reported, treated as present
      record_fault(fault, MMT_FAULT_PAD_MASK);
      w |= readout_bits;
    }
  }
#pragma unroll 1
  for (int s = 0; s < cs.S; ++s)
    if (counts[(int64_t)b * cs.S + s] < cs.min_points[s]) w &= ~(1u << cs.set[s]);
  words[b] = w;
}

__global__ void pad_mask_bias_kernel(PadSets s, int L, int lp, const uint32_t* __restrict__ words,
                                     const uint8_t* __restrict__ text, int text_set, int T,
                                     float* __restrict__ kb, int64_t kb_s_b, int accumulate) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // position in the row
  if (i >= lp) return;
  float* p = kb + (int64_t)b * kb_s_b + i;
  if (i >= L) {
    if (!accumulate) *p = 0.f;
    return;
  }
  const uint32_t word = words ? words[b] : 0xffffffffu;
  const bool m = row_masked(s, i, word, text ? text + (int64_t)b * T : nullptr, text_set);
  if (accumulate) {
    if (m) *p += MMT_PAD_MASK_LOGIT;
  } else {
    *p = m ? MMT_PAD_MASK_LOGIT : 0.f;
  }
}

constexpr int PM_WAVES = 4;   // waves per workgroup, one row each per pass
constexpr int PM_ROWS = 16;   // rows per workgroup

// FWD: x[b, l] = pe[l]; else x[b, l] = 0, on the masked rows. D % 4 == 0.
template <bool FWD>
__global__ __launch_bounds__(64 * PM_WAVES) void pad_mask_rows_kernel(
    PadSets s, int L, int D, const uint32_t* __restrict__ words, const uint8_t* __restrict__ text,
    int text_set, int T, const float* __restrict__ pe, float* __restrict__ x, int64_t xs_b,
    int64_t xs_t) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t word = words ? words[b] : 0xffffffffu;
  const uint8_t* tb = text ? text + (int64_t)b * T : nullptr;
  const int l0 = blockIdx.x * PM_ROWS;
  for (int l = l0 + wave; l < min(l0 + PM_ROWS, L); l += PM_WAVES) {
    if (!row_masked(s, l, word, tb, text_set)) continue;   // wave-uniform
    float* xr = x + (int64_t)b * xs_b + (int64_t)l * xs_t;
    for (int c = lane * 4; c < D; c += 256) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (FWD) v = *reinterpret_cast<const float4*>(pe + (int64_t)l * D + c);
      *reinterpret_cast<float4*>(xr + c) = v;
    }
  }
}

struct ImageSets {
  int set[MMT_PAD_MASK_MAX_SETS];
};
constexpr int PM_IMG_VECS = 4;  // 16-B vectors per thread

// dst[b, i] = src[b, i], or zero bytes when image i's set is absent for sample b. n16: 16-B
// vectors per image.
__global__ __launch_bounds__(256) void pad_mask_images_kernel(
    ImageSets is, int I, int64_t n16, const uint32_t* __restrict__ words,
    const uint4* __restrict__ src, uint4* __restrict__ dst) {
  const int bi = blockIdx.y, b = bi / I, i = bi - b * I;
  const bool present = (words[b] >> is.set[i]) & 1u;   // block-uniform
  const int64_t base = (int64_t)bi * n16;
  const int64_t v0 = ((int64_t)blockIdx.x * PM_IMG_VECS) * 256 + threadIdx.x;
  uint4 v[PM_IMG_VECS];
#pragma unroll
  for (int u = 0; u < PM_IMG_VECS; ++u) {
    v[u] = make_uint4(0u, 0u, 0u, 0u);
    if (present && v0 + u * 256 < n16) v[u] = src[base + v0 + u * 256];
  }
#pragma unroll
  for (int u = 0; u < PM_IMG_VECS; ++u)
    if (v0 + u * 256 < n16) dst[base + v0 + u * 256] = v[u];
}

// the checks every entry point with a set table shares
int check_sets(const char* fn, int B, int L, int n_sets, const int32_t* set_start,
               const int32_t* set_len, const void* words, const void* text_mask, int text_set,
               int T, PadSets* out) {
  MMT_CHECK_ARG(set_start && set_len, "%s: null set table", fn);
  MMT_CHECK_ARG(words || text_mask, "%s: neither the packed set mask nor a text mask", fn);
  MMT_CHECK_ARG(B > 0 && L > 0 && B <= 65535, "%s: B (1 .. 65535) and L must be > 0", fn);
  MMT_CHECK_ARG(n_sets >= 1 && n_sets <= MMT_PAD_MASK_MAX_SETS, "%s: n_sets %d outside 1 .. %d", fn,
                n_sets, MMT_PAD_MASK_MAX_SETS);
  int cur = 0;
  for (int k = 0; k < n_sets; ++k) {
    MMT_CHECK_ARG(set_start[k] == cur && set_len[k] >= 0 && set_len[k] <= L - cur,
                  "%s: the sets do not tile [0, %d) (set %d: start %d, len %d)", fn, L, k,
                  set_start[k], set_len[k]);
    cur += set_len[k];
  }
  MMT_CHECK_ARG(cur == L, "%s: the sets cover %d tokens, the sequence has %d", fn, cur, L);
  if (text_mask) {
    MMT_CHECK_ARG(text_set >= 0 && text_set < n_sets, "%s: text_set %d outside the %d sets", fn,
                  text_set, n_sets);
    MMT_CHECK_ARG(T == set_len[text_set], "%s: the text mask has %d tokens, its set %d has %d", fn,
                  T, text_set, set_len[text_set]);
  }
  out->n = n_sets;
  for (int k = 0; k < MMT_PAD_MASK_MAX_SETS; ++k) {
    out->start[k] = k < n_sets ? set_start[k] : L;
    out->len[k] = k < n_sets ? set_len[k] : 0;
  }
  return MMT_OK;
}

template <bool FWD>
int pad_mask_rows(const char* fn, const uint32_t* words, int B, int L, int D, int n_sets,
                  const int32_t* set_start, const int32_t* set_len, const uint8_t* text_mask,
                  int text_set, int T, const float* pe, float* x, int64_t xs_b, int64_t xs_t,
                  mmt_stream_t stream) {
  MMT_CHECK_ARG(x && (!FWD || pe), "%s: null pointer", fn);
  PadSets s;
  if (int rc = check_sets(fn, B, L, n_sets, set_start, set_len, words, text_mask, text_set, T, &s))
    return rc;
  MMT_CHECK_ARG(D > 0 && D % 4 == 0, "%s: D must be > 0 and a multiple of 4", fn);
  MMT_CHECK_ARG(aligned_to(x, 16) && (!FWD || aligned_to(pe, 16)),
                "%s: the sequence and pe must be 16-B aligned", fn);
  MMT_CHECK_ARG(xs_t >= D && xs_t % 4 == 0 && xs_b % 4 == 0 && xs_b >= (int64_t)(L - 1) * xs_t + D,
                "%s: strides (xs_t >= D, xs_b covering L rows, both multiples of 4)", fn);
  const dim3 grid((L + PM_ROWS - 1) / PM_ROWS, B);
  hipLaunchKernelGGL(pad_mask_rows_kernel<FWD>, grid, dim3(64 * PM_WAVES), 0, as_stream(stream), s,
                     L, D, words, text_mask, text_set, T, pe, x, xs_b, xs_t);
  MMT_CHECK_LAUNCH(fn);
  return MMT_OK;
}

}  // namespace

extern "C" int mmt_pad_mask_pack(const uint8_t* set_mask, int B, int n_sets, uint32_t readout_bits,
                                 uint32_t* words, mmt_stream_t stream) {
  MMT_CHECK_ARG(set_mask && words, "mmt_pad_mask_pack: null pointer");
  MMT_CHECK_ARG(B > 0, "mmt_pad_mask_pack: B must be > 0");
  MMT_CHECK_ARG(n_sets >= 1 && n_sets <= MMT_PAD_MASK_MAX_SETS,
                "mmt_pad_mask_pack: n_sets %d outside 1 .. %d", n_sets, MMT_PAD_MASK_MAX_SETS);
  MMT_CHECK_ARG((readout_bits >> n_sets) == 0,
                "mmt_pad_mask_pack: readout_bits 0x%x names a set past the %d sets", readout_bits,
                n_sets);
  hipLaunchKernelGGL(pad_mask_pack_kernel, dim3((B + 255) / 256), dim3(256), 0, as_stream(stream),
                     set_mask, B, n_sets, readout_bits, words, fault_word());
  MMT_CHECK_LAUNCH("mmt_pad_mask_pack");
  return MMT_OK;
}

extern "C" int mmt_pad_mask_pack_counts(const uint8_t* set_mask, int B, int n_sets,
                                        uint32_t readout_bits, const int32_t* counts, int S,
                                        const int32_t* pc_set, const int32_t* min_points,
                                        uint32_t* words, mmt_stream_t stream) {
  const char* fn = "mmt_pad_mask_pack_counts";
  MMT_CHECK_ARG(counts && pc_set && min_points && words, "%s: null pointer", fn);
  MMT_CHECK_ARG(B > 0, "%s: B must be > 0", fn);
  MMT_CHECK_ARG(n_sets >= 1 && n_sets <= MMT_PAD_MASK_MAX_SETS, "%s: n_sets %d outside 1 .. %d", fn,
                n_sets, MMT_PAD_MASK_MAX_SETS);
  MMT_CHECK_ARG((readout_bits >> n_sets) == 0, "%s: readout_bits 0x%x names a set past the %d sets",
                fn, readout_bits, n_sets);
  MMT_CHECK_ARG(S >= 1 && S <= n_sets, "%s: S %d outside 1 .. n_sets = %d", fn, S, n_sets);
  CountSets cs{};
  cs.S = S;
  for (int s = 0; s < S; ++s) {
    MMT_CHECK_ARG(pc_set[s] >= 0 && pc_set[s] < n_sets && !((readout_bits >> pc_set[s]) & 1u),
                  "%s: cloud %d belongs to set %d, outside the %d sets or a Readout set", fn, s,
                  pc_set[s], n_sets);
    MMT_CHECK_ARG(min_points[s] >= 0, "%s: min_points[%d] = %d is negative", fn, s, min_points[s]);
    cs.set[s] = pc_set[s];
    cs.min_points[s] = min_points[s];
  }
  hipLaunchKernelGGL(pad_mask_pack_counts_kernel, dim3((B + 255) / 256), dim3(256), 0,
                     as_stream(stream), set_mask, B, n_sets, readout_bits, cs, counts, words,
                     fault_word());
  MMT_CHECK_LAUNCH(fn);
  return MMT_OK;
}

extern "C" int mmt_pad_mask_images(const uint32_t* words, const int32_t* image_set, int n_sets,
                                   int B, int I, int64_t image_bytes, const void* src, void* dst,
                                   mmt_stream_t stream) {
  const char* fn = "mmt_pad_mask_images";
  MMT_CHECK_ARG(words && image_set && src && dst, "%s: null pointer", fn);
  MMT_CHECK_ARG(n_sets >= 1 && n_sets <= MMT_PAD_MASK_MAX_SETS, "%s: n_sets %d outside 1 .. %d", fn,
                n_sets, MMT_PAD_MASK_MAX_SETS);
  MMT_CHECK_ARG(B > 0 && I > 0 && I <= MMT_PAD_MASK_MAX_SETS && (int64_t)B * I <= 65535,
                "%s: B, I must be > 0, I <= %d, B * I <= 65535", fn, MMT_PAD_MASK_MAX_SETS);
  MMT_CHECK_ARG(image_bytes > 0 && image_bytes % 16 == 0 && aligned_to(src, 16) &&
                    aligned_to(dst, 16),
                "%s: images are moved as 16-B vectors (image_bytes a multiple of 16, src and dst "
                "16-B aligned)", fn);
  MMT_CHECK_ARG(src != dst, "%s: src and dst must differ (the caller's images are not changed)", fn);
  ImageSets is{};
  for (int i = 0; i < I; ++i) {
    MMT_CHECK_ARG(image_set[i] >= 0 && image_set[i] < n_sets,
                  "%s: image %d belongs to set %d, outside the %d sets", fn, i, image_set[i], n_sets);
    is.set[i] = image_set[i];
  }
  const int64_t n16 = image_bytes / 16, per_block = (int64_t)PM_IMG_VECS * 256;
  const int64_t gx = (n16 + per_block - 1) / per_block;
  MMT_CHECK_ARG(gx <= INT32_MAX, "%s: image too large", fn);
  hipLaunchKernelGGL(pad_mask_images_kernel, dim3((unsigned)gx, B * I), dim3(256), 0,
                     as_stream(stream), is, I, n16, words, (const uint4*)src, (uint4*)dst);
  MMT_CHECK_LAUNCH(fn);
  return MMT_OK;
}

extern "C" int mmt_pad_mask_bias(const uint32_t* words, int B, int L, int n_sets,
                                 const int32_t* set_start, const int32_t* set_len,
                                 const uint8_t* text_mask, int text_set, int T, float* kb,
                                 int64_t kb_s_b, int accumulate, mmt_stream_t stream) {
  const char* fn = "mmt_pad_mask_bias";
  MMT_CHECK_ARG(kb, "%s: null pointer", fn);
  PadSets s;
  if (int rc = check_sets(fn, B, L, n_sets, set_start, set_len, words, text_mask, text_set, T, &s))
    return rc;
  const int lp = (L + 63) & ~63;
  MMT_CHECK_ARG(kb_s_b % 4 == 0 && kb_s_b >= lp && aligned_to(kb, 16),
                "%s: kb needs 16-B aligned rows of >= roundup(L, 64) = %d floats, stride a multiple "
                "of 4", fn, lp);
  hipLaunchKernelGGL(pad_mask_bias_kernel, dim3(lp / 64, B), dim3(64), 0, as_stream(stream), s, L,
                     lp, words, text_mask, text_set, T, kb, kb_s_b, accumulate);
  MMT_CHECK_LAUNCH(fn);
  return MMT_OK;
}

extern "C" int mmt_pad_mask_rows_fwd(const uint32_t* words, int B, int L, int D, int n_sets,
                                     const int32_t* set_start, const int32_t* set_len,
                                     const uint8_t* text_mask, int text_set, int T, const float* pe,
                                     float* x0, int64_t xs_b, int64_t xs_t, mmt_stream_t stream) {
  return pad_mask_rows<true>("mmt_pad_mask_rows_fwd", words, B, L, D, n_sets, set_start, set_len,
                             text_mask, text_set, T, pe, x0, xs_b, xs_t, stream);
}

extern "C" int mmt_pad_mask_rows_bwd(const uint32_t* words, int B, int L, int D, int n_sets,
                                     const int32_t* set_start, const int32_t* set_len,
                                     const uint8_t* text_mask, int text_set, int T, float* dx0,
                                     int64_t xs_b, int64_t xs_t, mmt_stream_t stream) {
  return pad_mask_rows<false>("mmt_pad_mask_rows_bwd", words, B, L, D, n_sets, set_start, set_len,
                              text_mask, text_set, T, nullptr, dx0, xs_b, xs_t, stream);
}
