/* libmmt_hip — C ABI of the MI355X (gfx950) hot path of an OCTO-style multimodal transformer
 * training step with token merging (ToMe).
 *
 * The reference (maggieHao/multi_modal_transformers_TokenMerge, JAX/Flax) has no FFI: its
 * "interface" is the Flax module / function API. Each entry point below names the reference
 * function or Flax layer it replaces (paths relative to the reference's multi_modal_transformers/).
 *
 * Conventions
 *   - All tensor arguments are caller-owned DEVICE pointers; the library allocates nothing.
 *   - Strides are in ELEMENTS. Shapes are int, strides int64_t.
 *   - Every call is ordered on `stream` (a hipStream_t passed as void*), is graph-capturable
 *     (no host sync, no allocation) and returns MMT_OK (0) or a negative MMT_ERR_* code.
 *   - mmt_last_error() returns a thread-local description of the last failure.
 *   - dtype codes: MMT_F32 = 0, MMT_BF16 = 1.
 */
#ifndef MMT_API_H
#define MMT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mmt_stream_t;

enum { MMT_OK = 0, MMT_ERR_INVALID = -1, MMT_ERR_HIP = -2, MMT_ERR_UNSUPPORTED = -3 };
enum { MMT_F32 = 0, MMT_BF16 = 1 };
/* ToMe flags. CLASS/DISTILL: token_compression.py:57-64. PLAIN_SUM: the bare merge(x, "sum")
 * closure (no size weighting, no division). NO_SCATTER: merge(x, mode) with mode != "sum", which
 * in the reference leaves dst unchanged (:99-101). */
enum {
  MMT_TOME_CLASS_TOKEN = 1,
  MMT_TOME_DISTILL_TOKEN = 2,
  MMT_TOME_PLAIN_SUM = 4,
  MMT_TOME_NO_SCATTER = 8
};

const char* mmt_last_error(void);
/* ABI version of this header. 2: mmt_epilogue_t gained its trailing keep_bits field (a caller
 * built against version 1 passes a shorter struct: mmt_gemm would read past it). Callers check
 * mmt_version() == MMT_API_VERSION at load time and zero-initialise every mmt_epilogue_t
 * (memset / `= {0}`) before setting the fields they use, so fields added later read as unused. */
#define MMT_API_VERSION 2
int mmt_version(void);

/* Device-side index checks. The entry points that address memory through caller-supplied index
 * arrays (mmt_tome_merge_wavg_fwd / _bwd, mmt_tome_merge_seqnorm_fwd, mmt_ln_unmerge_dropout_bwd,
 * mmt_gather_rows, mmt_topk_scatter_bwd, mmt_tome_pos_map, mmt_tome_source_step / _groups,
 * mmt_tome_unmerge_fwd / _bwd, mmt_value_tokens_fwd / _bwd, mmt_pc_sample_group,
 * mmt_pc_sample_group_counts, mmt_pc_embed_fwd / _bwd, mmt_pad_mask_pack,
 * mmt_pad_mask_pack_counts) cannot see those device values at launch. mmt_depth_unproject takes
 * no index, but sizes its output from device data: every slot it writes is in [0, P). Their kernels
 * range-check every index they use; an invalid one is replaced by 0 (so no access leaves its
 * tensor and the context survives) and sets a bit of a library-wide device status word:
 *   MMT_FAULT_TOME_INDEX     unm / src not in [0, ceil(t/2)), dst not in [0, t/2)
 *   MMT_FAULT_TOME_PARTITION unm and src repeat an a-token (not a partition of the a half)
 *   MMT_FAULT_POS_MAP        pos_map entry not in [0, t - r)
 *   MMT_FAULT_ROW_INDEX      gathered / scattered row not in [0, L); a saved value token not in
 *                            [0, num_bins) (mmt_value_tokens_bwd: the entry is skipped); a cloud's
 *                            count not in [0, P] or an injected start not below the count
 *                            (mmt_pc_sample_group_counts: clamped / 0)
 *   MMT_FAULT_PAD_MASK       a Readout set flagged absent in a set pad mask (mmt_pad_mask_pack:
 *                            the set is treated as present)
 * mmt_device_status synchronises `stream`, returns MMT_OK if the word is clear, else clears it and
 * returns MMT_ERR_INVALID with the decoded bits in mmt_last_error(). Not graph-capturable (it
 * synchronises); call it after a step, a test or a bench. The reference's jnp gathers cannot fault
 * (XLA clamps), so this adds the check the C ABI needs to keep its "never abort" convention. */
enum {
  MMT_FAULT_TOME_INDEX = 1,
  MMT_FAULT_TOME_PARTITION = 2,
  MMT_FAULT_POS_MAP = 4,
  MMT_FAULT_ROW_INDEX = 8,
  MMT_FAULT_PAD_MASK = 16
};
int mmt_device_status(mmt_stream_t stream);

/* Deterministic mode (SURVEY §5 "deterministic-mode reruns"). The gradient accumulations that are
 * otherwise fp32 atomics (bias / LayerNorm / GroupNorm / embedding / Fourier gradients, the
 * attention's QKV bias sums) go, for addresses inside the registered fp32 gradient buffer
 * [grad, grad + n), to fx: a signed 64-bit fixed-point shadow of it (round(v * 2^36), integer
 * atomics: order-independent). mmt_det_flush then adds fx * 2^-36 into grad and clears fx, so a
 * step's gradients are bitwise reproducible. fx NULL turns the mode off. mmt_set_deterministic is
 * synchronous: call it outside stream capture; fx must be zero-initialised. Replaces nothing in
 * the reference (its XLA reductions are deterministic per backend); reproducibility only. */
int mmt_set_deterministic(float* grad, long long* fx, int64_t n);
int mmt_det_flush(float* grad, long long* fx, int64_t n, mmt_stream_t stream);

/* Bytes of caller-provided device workspace an entry point needs (the library
 * allocates nothing; scratch comes from the caller). op / dims:
 *   MMT_WS_TOME_MATCH  {n, t, c}  (mmt_tome_match)
 *   MMT_WS_GRAD_NORM   {n}        (mmt_optim_prepare)
 * Returns the byte count, or a negative MMT_ERR_* code. */
enum { MMT_WS_TOME_MATCH = 1, MMT_WS_GRAD_NORM = 2 };
int64_t mmt_workspace_size(int op, const int64_t* dims, int ndims);

/* ------------------------------------------------------------------ ToMe
 * mmt_tome_match replaces tokenizers/token_compression.py:54-112 (bipartite_soft_matching)
 * for an r that the caller has already clamped to min(r, (t - protected) // 2) > 0
 * (token_compression.py:66-70; the r <= 0 "do nothing" branch is the caller's).
 *
 * metric element (b, i, h, k) lives at metric[b*s_n + i*s_t + h*s_h + k]; the matching metric is
 * the fp32 sum over h = 0..heads-1 (heads = 1 for a plain (n, t, c) metric; heads = H gives the
 * ToMe key metric  sum_h K  of tome_attention.py:253).
 * Outputs (int32, per batch row contiguous): unm_idx[n][ta - r], src_idx[n][r], dst_idx[n][r],
 * where ta = ceil(t/2) (indices into the a = x[::2] / b = x[1::2] halves, exactly as the
 * reference's edge_idx / node_idx). node_max[n][ta] (fp32) is optional (may be NULL).
 * Arithmetic is canonical (see DESIGN.md "ToMe canonical arithmetic") so indices are bit-exact
 * with oracle/tome_ref.c. t <= 2048, c <= 512. workspace: >= mmt_workspace_size(
 * MMT_WS_TOME_MATCH, {n, t, c}) bytes, 16-B aligned (normalised metric halves, node_max/idx).
 */
int mmt_tome_match(const void* metric, int dtype, int n, int t, int heads, int c, int64_t s_n,
                   int64_t s_t, int64_t s_h, int r, int flags, int32_t* unm_idx, int32_t* src_idx,
                   int32_t* dst_idx, float* node_max, void* workspace, int64_t ws_bytes,
                   mmt_stream_t stream);
/* The kernel chain that the last mmt_tome_match call launched: MMT_TOME_ROUTE_NONE after a call
 * rejected before any launch, else the form in MMT_TOME_ROUTE_FORM_MASK —
 *   _FUSED       one launch (norm + score + rank in LDS): 16-B-vector metric, the MFMA path and
 *                both normalised halves within 160 KB of LDS (t <= 513 at c = 64);
 *   _BIG_AG1/2   norm, the b-resident score kernel with 1 / 2 a tiles per workgroup, rank8: the
 *                MFMA path, c % 4 == 0 and the b half within 160 KB (t <= 1153 at c = 64); two a
 *                tiles when n * ceil(ta / 32) > 256 and they still fit;
 *   _TILED_MFMA  norm, the tiled score kernel (MFMA: the MFMA path and even c), rank;
 *   _TILED_VALU  the same with the VALU fmaf chain —
 * with MMT_TOME_ROUTE_NORM_SCALAR when the norm was the scalar kernel (c % 8 != 0, or a base or
 * stride that is no multiple of 16 B), else MMT_TOME_ROUTE_LPR = the lanes per token row of the
 * vector norm / the fused kernel (the power of two >= c / 8); MMT_TOME_ROUTE_NBT = the b tiles per
 * LDS group of the tiled forms (1..4, 0 otherwise); MMT_TOME_ROUTE_IN_BF16 for a bf16 metric.
 * Process-wide, not thread-safe. */
enum {
  MMT_TOME_ROUTE_NONE = 0,
  MMT_TOME_ROUTE_FUSED = 1,
  MMT_TOME_ROUTE_BIG_AG1 = 2,
  MMT_TOME_ROUTE_BIG_AG2 = 3,
  MMT_TOME_ROUTE_TILED_MFMA = 4,
  MMT_TOME_ROUTE_TILED_VALU = 5,
  MMT_TOME_ROUTE_FORM_MASK = 0xff,
  MMT_TOME_ROUTE_NORM_SCALAR = 0x10000,
  MMT_TOME_ROUTE_IN_BF16 = 0x20000
};
#define MMT_TOME_ROUTE_LPR(route) (((route) >> 8) & 0xff)
#define MMT_TOME_ROUTE_NBT(route) (((route) >> 20) & 0xf)
int mmt_tome_last_route(void);

/* mmt_tome_merge_wavg_fwd replaces token_compression.py:114-129 (merge_wavg) applied with the
 * merge closure of :90-109 (mode "sum"), fused with the surrounding sequence copy:
 * x is a sequence (n, L, D) whose rows [set_start, set_start + t) are the merged token set; the
 * output sequence (n, L - r, D) holds rows [0, set_start) copied, then the t - r merged rows
 * (concat[unm, dst], or the distill interleave), then the remaining rows copied.
 * size_in (n, t) fp32 may be NULL (= ones). size_out (n, t - r) receives the merged sizes.
 * pos_map (n, t) int32 (optional) receives, for each set token, the merged row it went to.
 */
int mmt_tome_merge_wavg_fwd(const void* x, int dtype, int n, int L, int D, int64_t x_s_n,
                            int64_t x_s_t, int set_start, int t, int r, int flags,
                            const float* size_in, const int32_t* unm_idx, const int32_t* src_idx,
                            const int32_t* dst_idx, void* x_out, int64_t o_s_n, int64_t o_s_t,
                            float* size_out, int32_t* pos_map, mmt_stream_t stream);

/* Selects the score path of mmt_tome_match: 1 = f32 MFMA (v_mfma_f32_32x32x2_f32, default),
 * 0 = VALU fmaf chain. Both produce the same canonical fmaf chain; the switch exists so the
 * parity tests can check each against the oracle. */
void mmt_tome_set_match_path(int use_mfma);

/* Backward of mmt_tome_merge_wavg_fwd w.r.t. x (sizes carry no gradient; the metric carries
 * none either: argmax/argsort):  g_in[row] = g_out[pos(row)] * size_in[row] / size_out[pos(row)]
 * for set rows, plain copy for the others.  pos_map comes from the forward. size_in and size_out
 * may both be NULL: the bare merge(x, "sum") closure, whose Jacobian is a 0/1 gather. */
/* The backward of the same pair plus the attention-output dropout, fused: mmt_seqnorm_bwd over the
 * merged sequence (dy bf16, x and addend fp32, L2 = L - r rows), then mmt_tome_merge_wavg_bwd
 * (pos_map, size_in, size_out) into g_in (B, L, D) fp32, then mmt_dropout_bwd (layer, site,
 * keep_prob, row_offset; rng NULL = no dropout) of g_in into z bf16 with its column sums added
 * to bias_grad. The merged gradient stays in LDS. L <= 512, L2 * 256 B <= 96 KB. */
int mmt_ln_unmerge_dropout_bwd(const void* dy, int64_t ds_b, int64_t ds_t, const float* x,
                               int64_t xs_b, int64_t xs_t, int B, int L2, int D, const float* mean,
                               const float* rstd, const float* gamma, const float* addend,
                               int64_t as_b, int64_t as_t, float* dgamma, float* dbeta, int L,
                               int set_start, int t, int r, const float* size_in,
                               const float* size_out, const int32_t* pos_map, float* g_in,
                               int64_t gs_b, int64_t gs_t, const uint32_t* rng, uint32_t layer,
                               uint32_t site, float keep_prob, int64_t row_offset, void* z,
                               int64_t zs_b, int64_t zs_t, float* bias_grad, mmt_stream_t stream);
/* mmt_tome_merge_wavg_fwd fused with the sequence-axis LayerNorm forward that follows it in the
 * block (attention.py:66; mmt_seqnorm_fwd semantics): fp32 x, merged rows x_out (bit-identical to
 * the unfused merge), size_out / pos_map as there, y = LN(x_out) bf16 with mean / rstd (B, D)
 * (bit-identical to mmt_seqnorm_fwd on x_out). L - r <= 512, D % 8 == 0. Both fused entries
 * follow the operand rules of the sequence LayerNorm section below and report their kernel form
 * through mmt_norm_last_route(). */
int mmt_tome_merge_seqnorm_fwd(const float* x, int n, int L, int D, int64_t x_s_n, int64_t x_s_t,
                               int set_start, int t, int r, int flags, const float* size_in,
                               const int32_t* unm_idx, const int32_t* src_idx,
                               const int32_t* dst_idx, float* x_out, int64_t o_s_n, int64_t o_s_t,
                               float* size_out, int32_t* pos_map, const float* gamma,
                               const float* beta, float eps, void* y, int64_t y_s_n, int64_t y_s_t,
                               float* mean, float* rstd, mmt_stream_t stream);
int mmt_tome_merge_wavg_bwd(const void* g_out, int dtype, int n, int L, int D, int64_t go_s_n,
                            int64_t go_s_t, int set_start, int t, int r, const float* size_in,
                            const float* size_out, const int32_t* pos_map, void* g_in,
                            int64_t gi_s_n, int64_t gi_s_t, mmt_stream_t stream);

/* ---- merge source and unmerge. Replaces ToMe's merge_source (the patch -> merged token map the
 * reference's merge closure, token_compression.py:90-129, never exposes) and adds the unmerge it
 * implies. All five are graph-capturable and allocate nothing; index values are range-checked on
 * the device (see "Device-side index checks" above: clamped to 0 and reported, never followed).
 *
 * mmt_tome_pos_map: the (n, t) int32 pos_map that mmt_tome_merge_wavg_fwd writes for the same
 * unm / src / dst and flags (class / distill layouts included; token_compression.py:90-109's
 * concat[unm, dst] placement), without touching any x. Same limits on t and r as the merge. */
int mmt_tome_pos_map(const int32_t* unm_idx, const int32_t* src_idx, const int32_t* dst_idx, int n,
                     int t, int r, int flags, int32_t* pos_map, mmt_stream_t stream);
/* One layer of ToMe's merge_source, in place on source (n, t0) int32:
 * source[b, p] = pos_map[b, source[b, p]] for the layer's pos_map (n, t) -> [0, t - r).
 * first != 0 starts from the identity (source[b, p] = pos_map[b, p]; needs t0 == t).
 * source values outside [0, t): MMT_FAULT_ROW_INDEX; pos_map values outside [0, t - r):
 * MMT_FAULT_POS_MAP. t <= t0 <= 2048 (mmt_tome_match's limit). */
int mmt_tome_source_step(const int32_t* pos_map, int n, int t, int r, int32_t* source, int t0,
                         int first, mmt_stream_t stream);
/* The inverse of source (n, t0) -> [0, tf) in CSR form (ToMe's merge_source matrix, sparse):
 * group_start (n, tf + 1) int32, members (n, t0) int32; merged token j of sample b stands for the
 * patches members[b, group_start[b, j] .. group_start[b, j + 1]), listed in ascending patch
 * order whatever the scheduling. Empty groups are legal. source values outside [0, tf):
 * MMT_FAULT_ROW_INDEX. tf <= t0 <= 2048. */
int mmt_tome_source_groups(const int32_t* source, int n, int t0, int tf, int32_t* group_start,
                           int32_t* members, mmt_stream_t stream);
/* Unmerge: x (n, L, D) holds a merged set of tf rows at [set_start, set_start + tf); out
 * (n, L - tf + t0, D) holds rows [0, set_start) copied, then the t0 rows
 * out[b, set_start + p] = x[b, set_start + source[b, p]], then the remaining rows copied (the
 * sequence layout of mmt_tome_merge_wavg_fwd, read backwards). fp32 / bf16, D % 8 == 0, strides
 * and base pointers multiples of 16 bytes. source outside [0, tf): MMT_FAULT_ROW_INDEX. */
int mmt_tome_unmerge_fwd(const void* x, int dtype, int n, int L, int D, int64_t x_s_n,
                         int64_t x_s_t, int set_start, int tf, const int32_t* source, int t0,
                         void* out, int64_t o_s_n, int64_t o_s_t, mmt_stream_t stream);
/* Its adjoint: g (n, L - tf + t0, D) -> g_x (n, L, D); copied rows copied, set row j = the sum of
 * g[b, set_start + p] over p in members(j) (mmt_tome_source_groups), accumulated in fp32 in that
 * (ascending) order and rounded once at the store; an empty group gives zeros. No atomics: the
 * result is bitwise reproducible. members outside [0, t0) and group_start rows that are not
 * 0 <= start <= end <= t0: MMT_FAULT_ROW_INDEX. */
int mmt_tome_unmerge_bwd(const void* g, int dtype, int n, int L, int D, int64_t g_s_n,
                         int64_t g_s_t, int set_start, int tf, const int32_t* group_start,
                         const int32_t* members, int t0, void* g_x, int64_t gx_s_n,
                         int64_t gx_s_t, mmt_stream_t stream);

/* ------------------------------------------------------------------ top-k token pruning
 * mmt_topk_gather replaces tokenizers/token_compression.py:15-46 (compute_top_k_tokens, vmapped
 * over the batch, :168): for each token set s (host arrays set_start/set_len/set_k, <= 16 sets,
 * len <= 4096), the indices of jax.lax.top_k(scores[b, start:start+len], k) (descending, equal
 * scores keep the lower index first, float total order with NaN largest) + start, concatenated
 * over the sets in the given order -> idx_out (B, K = sum k) int32, and out[b, i] = x[b, idx].
 * x/out: (B, L, D) / (B, K, D) rows of fp32 or bf16 (dtype), 16-B aligned rows. */
int mmt_topk_gather(const void* x, int dtype, int B, int L, int D, int64_t xs_b, int64_t xs_t,
                    const float* scores, int64_t ss_b, int n_sets, const int32_t* set_start,
                    const int32_t* set_len, const int32_t* set_k, void* out, int64_t os_b,
                    int64_t os_t, int32_t* idx_out, mmt_stream_t stream);
/* out[b, i] = x[b, idx[b, i]] for i < K (rows of D fp32 / bf16 elements; idx (B, K) from
 * mmt_topk_gather): the residual stream of a pruned block follows its attention rows. */
int mmt_gather_rows(const void* x, int dtype, int B, int L, int D, int64_t xs_b, int64_t xs_t,
                    const int32_t* idx, int K, void* out, int64_t os_b, int64_t os_t,
                    mmt_stream_t stream);
/* Importance of compressed_attention.py:302-306 from mmt_attn_fwd's wsum: scores[b, q] =
 * (sum_h wsum[b, h, q] / L) / H (h ascending), the input of mmt_topk_gather. */
int mmt_prune_importance(const float* wsum, int B, int H, int L, float* scores, mmt_stream_t stream);
/* Backward of the gather: dx = 0, dx[b, idx[b, i]] = dout[b, i]. */
int mmt_topk_scatter_bwd(const void* dout, int dtype, int B, int K, int D, int64_t ds_b,
                         int64_t ds_t, const int32_t* idx, int L, void* dx, int64_t xs_b,
                         int64_t xs_t, mmt_stream_t stream);

/* ------------------------------------------------------------------ GEMM (MFMA bf16)
 * C = epilogue(op(A) . op(B)), fp32 accumulation, replacing every flax.linen.Dense /
 * DenseGeneral on the path (attention.py:32-37 MLPBlock; Flax SelfAttention q/k/v/out
 * projections configured in model_configs/attention_blocks/vanilla_decoder.yaml:19-31; the
 * image stem and output Dense, image_tokenizer.py:158-176; diffusion.py:41-65; T5 layers) and
 * their backward products (dX = dY.W, dW = dY^T.X).
 *   transA = 0: A is [M][K] (lda >= K);  transA = 1: A is stored [K][M] (lda >= M)
 *   transB = 0: B is [K][N] (ldb >= N);  transB = 1: B is stored [N][K] (ldb >= K)
 * A, B bf16; contiguous dims and strides multiples of 8 elements, base pointers 16-B aligned.
 * c_mode: MMT_OUT_BF16 (store), MMT_OUT_F32 (C = epi + beta*C), MMT_OUT_F32_ACCUM (C += alpha*acc,
 * the weight-gradient form; no other epilogue; with split_k > 1 the K range is split over
 * workgroups writing fp32 partial slabs into `workspace` (>= split_k*M*N floats, 16-B aligned)
 * which a second kernel sums into C — deterministic, no atomics).
 * Batched: entry z of `batch` reads A + z*sA, B + z*sB and writes C + z*sC (element strides; sB = 0
 * shares one weight). gate, residual and dropout are indexed by the row within an entry, so they
 * are shared by all entries (bias is per column, so shared as well). Split-K needs batch == 1.
 * N, ldc and sC must be multiples of 8 (8-column vector epilogue); A, B, C 16-B aligned.
 * Epilogue order: v = alpha*acc + bias[n]; act; v *= (gate[m][n] > 0 ? gate_scale : 0);
 * dropout (flax.linen.Dropout with a counter-based stream: element idx = (drop_row_offset + m)*N
 * + n keeps iff the 16-bit half (idx & 1) of mix32(key ^ (idx >> 1)) < floor(keep_prob * 65536),
 * key = stream_key(rng[0], rng[1], drop_layer, drop_site); kept values scaled by 1/keep_prob);
 * v += residual[m][n] (bf16 or fp32 per res_dtype).
 */
enum { MMT_ACT_NONE = 0, MMT_ACT_RELU = 1 };
#define MMT_SET_CAUSAL 0x80000000u
enum { MMT_OUT_BF16 = 0, MMT_OUT_F32 = 1, MMT_OUT_F32_ACCUM = 2 };

typedef struct {
  const float* bias;          /* [N] fp32 or NULL */
  int act;                    /* MMT_ACT_* */
  const uint32_t* rng;        /* device {seed, step} or NULL (no dropout) */
  uint32_t drop_layer, drop_site;
  float keep_prob;
  int64_t drop_row_offset;
  const void* gate;           /* bf16 [M][ld_gate] or NULL */
  int64_t ld_gate;
  float gate_scale;
  const void* residual;       /* [M][ld_res] bf16 or fp32 (res_dtype) or NULL */
  int64_t ld_res;
  float alpha, beta;
  int res_dtype;              /* MMT_BF16 / MMT_F32 */
  float* colsum;              /* [mmt_gemm_colsum_rows(...)][N] fp32 or NULL: row p = the column
                                 sums of C rows [256 p, 256 p + 256) as stored (bf16), written
                                 (not accumulated) — the bias gradient of the next Dense backward
                                 (layers.py:59 colsum) without re-reading C; only where
                                 mmt_gemm_colsum_rows is nonzero, else mmt_gemm fails */
  /* 1-bit form of the relu gate (the MLP hidden layer, attention.py:20-39 MLPBlock), both only
   * where mmt_gemm_colsum_rows is nonzero (the 256-wide bf16 NT path), else mmt_gemm fails:
   * relu_bits (out): [ceil(M/256)*256][N/32] words (16-B aligned), bit set iff the output is
   *   > 0 (the stored bf16 value has the same sign); output (m, n) is bit 8 c + e of the word
   *   at flat index (g * N/32 + w) * 4 + f, g = (m / 256) * 64 + ((m / 64) & 3) * 16 + (m & 15),
   *   f = (m / 16) & 3, n = 256 (w / 8) + 128 ((w / 4) & 1) + 8 (w & 3) + 32 c + e (c < 4,
   *   e < 8): one 16-B vector per lane of that path's epilogue (its 4 rows x 32 columns);
   * gate_bits (in): the same layout, used in place of gate (v *= bit ? gate_scale : 0), so a
   *   backward reads M*N/8 bytes instead of the bf16 gate's 2*M*N. NULL: unused.
   * keep_bits (in, relu_bits launches only, rng NULL): the dropout keep decisions in the same
   *   layout (mmt_gemm_dropout_keep_bits), applied as v = bit ? v / keep_prob : 0 in place of the
   *   counter-RNG draws — bit-identical outputs, the draws moved off the GEMM. NULL: unused. */
  uint32_t* relu_bits;
  const uint32_t* gate_bits;
  const uint32_t* keep_bits;
} mmt_epilogue_t;

/* Tuning knob (benchmarks): 0 = 128x128 register-staged, double-buffered LDS; 1 = same, single
 * LDS stage at 3 workgroups/CU; 2 = single stage with 128-deep K-steps; 3 = 256x192 tiles, 8
 * waves; 4 = direct-to-LDS (global_load_lds) 128x128 kernel for NT; -1 = automatic (default).
 * Process-wide, not thread-safe. */
void mmt_gemm_set_variant(int variant);
/* The kernel that the last mmt_gemm / mmt_gemm_fp8 / mmt_gemm_xs call launched, so that a test
 * can assert that it ran the kernel it is about: one value per kernel template that differs in
 * addressing, MMT_GEMM_ROUTE_NONE after a call rejected before any launch. For the narrow NT
 * kernel the tile width and the tile height of the call's last launch are encoded beside the
 * value (MMT_GEMM_ROUTE_NTW_BN / _MT). MMT_GEMM_ROUTE_COMBINE is set as well when the split-K
 * combine kernel ran after the main kernel. Process-wide, not thread-safe. */
enum {
  MMT_GEMM_ROUTE_NONE = 0,
  MMT_GEMM_ROUTE_GENERIC_P0 = 1,       /* 128x128 register-staged, double-buffered (variant 0) */
  MMT_GEMM_ROUTE_GENERIC_P1 = 2,       /* 128x128 single LDS stage, 64-deep K-steps (1) */
  MMT_GEMM_ROUTE_GENERIC_P1_BK128 = 3, /* 128x128 single LDS stage, 128-deep K-steps (2) */
  MMT_GEMM_ROUTE_BIG = 4,              /* 256x192 tiles (3) */
  MMT_GEMM_ROUTE_GLDS_NT = 5,          /* direct-to-LDS 128x128 NT kernel (4) */
  MMT_GEMM_ROUTE_NT256_256 = 6,        /* persistent 256 x BN NT kernel, BN 256 / 192 / 128 */
  MMT_GEMM_ROUTE_NT256_192 = 7,
  MMT_GEMM_ROUTE_NT256_128 = 8,
  MMT_GEMM_ROUTE_NTW = 9,              /* narrow-output NT kernel; | bn / 64 << 8 | mt / 64 << 12 */
  MMT_GEMM_ROUTE_NTWS = 10,            /* warp-specialised wide NT kernel */
  MMT_GEMM_ROUTE_XS = 11,              /* activation-stationary K = 384 kernel */
  MMT_GEMM_ROUTE_TN_DMA_256 = 12,      /* TN split-K slabs, two-stage, 32x32x16 MFMAs */
  MMT_GEMM_ROUTE_TN_DMA_384 = 13,
  MMT_GEMM_ROUTE_TN_DMA16_256 = 14,    /* TN split-K slabs, two-stage, 16x16x32 MFMAs */
  MMT_GEMM_ROUTE_TN_DMA16_384 = 15,
  MMT_GEMM_ROUTE_TN_R4_384 = 16,       /* TN split-K slabs, four-stage ring */
  MMT_GEMM_ROUTE_FP8_NT = 17,          /* mmt_gemm_fp8's own NT kernel */
  MMT_GEMM_ROUTE_XS_FP8 = 18,          /* activation-stationary kernel on e4m3 operands */
  MMT_GEMM_ROUTE_KERNEL_MASK = 0xff,
  MMT_GEMM_ROUTE_COMBINE = 0x10000
};
#define MMT_GEMM_ROUTE_NTW_BN(route) ((((route) >> 8) & 0xf) * 64)
#define MMT_GEMM_ROUTE_NTW_MT(route) ((((route) >> 12) & 0xf) * 64)
int mmt_gemm_last_route(void);
/* Rows of the epilogue's colsum slab for this launch shape (ceil(M / 256)), 0 when the kernel the
 * launch would use cannot write it (then take the column sums with mmt_colsum). */
int mmt_gemm_colsum_rows(int M, int N, int K, int transA, int transB, int c_mode, int split_k);
/* The keep_bits words of an (M, N) output's counter-RNG dropout (stream (rng, layer, site), rows
 * offset by row_offset: the draws mmt_gemm's epilogue would make with the same fields) into out
 * ([ceil(M/256)*256][N/32] words, 16-B aligned; N % 256 == 0). Replaces the per-element dropout
 * draws of the MLP hidden layer (attention.py:20-39 MLPBlock, nn.Dropout after the relu). */
int mmt_gemm_dropout_keep_bits(const uint32_t* rng, uint32_t layer, uint32_t site, int M, int N,
                               float keep_prob, int64_t row_offset, uint32_t* out, mmt_stream_t stream);
int mmt_gemm(int M, int N, int K, const void* A, int transA, int64_t lda, const void* B,
             int transB, int64_t ldb, void* C, int c_mode, int64_t ldc, int batch, int64_t sA,
             int64_t sB, int64_t sC, int split_k, const mmt_epilogue_t* epi, float* workspace,
             int64_t ws_elems, mmt_stream_t stream);

/* mmt_gemm_xs: C = X . W^T (+ bias[n]) in bf16 for the short-K products (K == 384: the
 * OCTO-small QKV projection), X [M][ldx], W [N][ldw] bf16, C [M][ldc] bf16, N % 64 == 0, 16-B
 * aligned rows; bias fp32 [N] or NULL. The activation-stationary kernel of csrc/gemm_xs.hip (a
 * 256-row panel of X held in registers while W streams through LDS); mmt_gemm routes its
 * K = 384 bf16 products with a bias / alpha / relu / dropout / relu_bits epilogue (M >= 32768;
 * relu_bits needs N % 256 == 0) and mmt_gemm_fp8 its K = 768 bf16-output products (no gate /
 * residual / relu_bits) there itself, with bit-identical outputs and bit images (reference
 * attention.py:20-37, 41-69 Dense layers). */
int mmt_gemm_xs(int M, int N, int K, const void* X, int64_t ldx, const void* W, int64_t ldw,
                void* C, int64_t ldc, const float* bias, mmt_stream_t stream);

/* FP8 weight path (BASELINE configs[4]; SURVEY §8c bar cosine >= 0.995): forward Dense products
 * in OCP e4m3 with one fp32 scale per activation row and per weight row (output channel).
 * mmt_quant_rows_fp8: scale[r] = amax|x[r,:]| / 448 (1 for a zero row), q[r,k] = e4m3(x[r,k] /
 * scale[r]) rounded to nearest even; x bf16 rows (stride ld), q uint8 rows (stride ldq), K % 8 == 0.
 * mmt_gemm_fp8: C = epilogue((A_q . B_q^T)[m][n] * sa[m] * sb[n]) with A_q [M][lda], B_q [N][ldb]
 * e4m3 (the NT form of mmt_gemm: B is the weight W[out][in]), on the block-scaled
 * v_mfma_scale_f32_32x32x64_f8f6f4 (unit block scales); same epilogue as mmt_gemm; c_mode
 * MMT_OUT_BF16 or MMT_OUT_F32. K % 64 == 0, N % 8 == 0, 16-B aligned rows. */
int mmt_quant_rows_fp8(const void* x, int64_t ld, int rows, int K, void* q, int64_t ldq,
                       float* scale, mmt_stream_t stream);
int mmt_gemm_fp8(int M, int N, int K, const void* A, int64_t lda, const float* sa, const void* B,
                 int64_t ldb, const float* sb, void* C, int c_mode, int64_t ldc,
                 const mmt_epilogue_t* epi, mmt_stream_t stream);

/* ------------------------------------------------------------------ attention
 * Blockwise-causal MHA replacing flax.linen.SelfAttention / dot_product_attention as the
 * reference configures it (vanilla_decoder.yaml:19-31, mask token_sequencer.py:313-321,
 * octo.py:66-68,119): softmax(where(mask, q.k * scale, finfo.min)) with attention dropout
 * sharing ONE (L, L) keep-mask across batch and heads (Flax broadcast_dropout) times v.
 * qkv: bf16 rows (b, t) at qkv + b*s_b + t*s_t holding [q(H,Dh) | k(H,Dh) | v(H,Dh)].
 * Mask = token-set table: n_sets (<= 16) contiguous sets tiling [0, L) (set_start/set_len HOST
 * arrays) and set_vis[s] = bitmask of key sets that query set s attends to; n_sets = 0: no mask.
 * Bit 31 of set_vis[s] (MMT_SET_CAUSAL) makes set s causal within itself: its query q sees its
 * own set's keys k <= q only (Text sets, token_sequencer.py:76-82, nn.make_causal_mask).
 * drop_bits: the query-word image of mmt_dropout_bits(.., L, L, ..) (its `out`), or NULL (no
 * dropout); kept probabilities are scaled by 1/keep_prob. bias: optional fp32 (H, L, L) added to the
 * scaled logits (T5 relative position bias; forward only). o: bf16 (b, t) rows of (H, Dh);
 * lse: fp32 (B, H, L) natural-log softmax normaliser. Dh in {64, 128, 256}.
 * wsum (optional, fp32 (B, H, L)): per query, the sum over keys of the attention weights AFTER
 * dropout (kept / keep_prob) — the per-head factor of the pruning importance score
 * (compressed_attention.py:302-306: mean over keys, then over heads; mmt_prune_importance).
 * Operand rules, the same for mmt_attn_fwd and mmt_attn_bwd (and their _keybias forms), checked
 * before anything is launched (MMT_ERR_INVALID): the kernels move every bf16 operand (qkv, o,
 * dout, dqkv) as 16-B vectors, so each base pointer is 16-B aligned and each row and batch
 * stride (s_*, o_s_*, d_s_*, dq_s_*) is a multiple of 8 elements; a row stride is at least the
 * row it carries (s_t, dq_s_t >= 3*H*Dh; o_s_t, d_s_t >= H*Dh); Dh is 64, 128 or 256;
 * 0 < L <= 4096. Nothing outside rows [0, L) x the row width of a sample is read or written;
 * lse and wsum are written at [0, B*H*L) and delta inside its documented size only.
 */
/* The kernel that the last mmt_attn_fwd / mmt_attn_bwd (or _keybias) call launched, forward or
 * backward, as mmt_gemm_last_route() reports the GEMM's: MMT_ATTN_ROUTE_NONE after a call
 * rejected before any launch. Beside the kernel (MMT_ATTN_ROUTE_KERNEL_MASK) the value carries
 * MMT_ATTN_ROUTE_PARAM — the tiled forward's query blocks per wave NQ (1 / 2), a resident kernel's
 * NTILE (2 * ceil(L / 64): 2 .. 10), the tiled backward's waves per workgroup (2: 128 threads,
 * 4: 256) — for the tiled kernels MMT_ATTN_ROUTE_DH, and MMT_ATTN_ROUTE_WORKLIST when the
 * concurrent-phase backward took its blocks from the work list (NTILE 8 outside deterministic
 * mode) instead of the static deal. Process-wide, not thread-safe. */
enum {
  MMT_ATTN_ROUTE_NONE = 0,
  MMT_ATTN_ROUTE_FWD_TILED_1W = 1,    /* attn_fwd_kernel, one-wave workgroups (L <= 32) */
  MMT_ATTN_ROUTE_FWD_TILED_4W = 2,    /* attn_fwd_kernel, four waves x NQ query blocks */
  MMT_ATTN_ROUTE_FWD_RES_ONEPASS = 3, /* attn_fwd_res_kernel, online softmax (the default) */
  MMT_ATTN_ROUTE_FWD_RES_TWOPASS = 4, /* attn_fwd_res_kernel, exact row max first */
  MMT_ATTN_ROUTE_BWD_TILED = 5,       /* attn_bwd_dq_kernel + attn_bwd_dkdv_kernel */
  MMT_ATTN_ROUTE_BWD_RES = 6,         /* attn_bwd_res_kernel: two-phase, 4 waves */
  MMT_ATTN_ROUTE_BWD_RES8 = 7,        /* attn_bwd_res8_kernel: concurrent phases, 8 waves */
  MMT_ATTN_ROUTE_KERNEL_MASK = 0xff,
  MMT_ATTN_ROUTE_WORKLIST = 0x10000
};
#define MMT_ATTN_ROUTE_PARAM(route) (((route) >> 8) & 0xf)
#define MMT_ATTN_ROUTE_DH(route) ((((route) >> 12) & 0xf) * 64)
int mmt_attn_last_route(void);
int mmt_attn_fwd(const void* qkv, int64_t s_b, int64_t s_t, int B, int L, int H, int Dh,
                 float scale, int n_sets, const int32_t* set_start, const int32_t* set_len,
                 const uint32_t* set_vis, const uint32_t* drop_bits, float keep_prob,
                 const float* bias, void* o, int64_t o_s_b, int64_t o_s_t, float* lse,
                 float* wsum, mmt_stream_t stream);
/* Backward: writes dq, dk, dv into dqkv (same row layout as qkv). delta: fp32 workspace of
 * B * H * 2 * roundup(L, 64) floats (rowsum(dO * O), and the row constants of the K/V-resident
 * kernel used for Dh 64 and 32 < L <= 320). drop_bits / drop_bits_t: the query-word and key-word images of
 * mmt_dropout_bits (`out` / `out_t`); both or neither. bias_grad (fp32 [3 H Dh], may be NULL) += the
 * column sums of dq | dk | dv over (B, L): the bias gradient of the fused QKV projection. */
int mmt_attn_bwd(const void* qkv, int64_t s_b, int64_t s_t, int B, int L, int H, int Dh,
                 float scale, int n_sets, const int32_t* set_start, const int32_t* set_len,
                 const uint32_t* set_vis, const uint32_t* drop_bits, const uint32_t* drop_bits_t,
                 float keep_prob, const void* o, int64_t o_s_b, int64_t o_s_t, const void* dout,
                 int64_t d_s_b, int64_t d_s_t, const float* lse, float* delta, void* dqkv,
                 int64_t dq_s_b, int64_t dq_s_t, float* bias_grad, mmt_stream_t stream);
/* The same two with a per-sample, per-key additive logit shared by all heads and queries. Two
 * users: ToMe proportional attention, key_bias[b, k] = log size[b, k] (a merged token votes as the
 * patches it stands for; mmt_tome_size_bias), and the observation pad masks, key_bias[b, k] =
 * MMT_PAD_MASK_LOGIT on the keys of absent token sets and padded text tokens (mmt_pad_mask_bias);
 * with both, the two biases add:  logits[b,h,q,k] = scale * q.k + key_bias[b,k], then mask, softmax and dropout as
 * above. key_bias == NULL is mmt_attn_fwd / mmt_attn_bwd (which forward here with NULL).
 * key_bias: fp32, row b at key_bias + b*kb_s_b; kb_s_b a multiple of 4 and >= roundup(L, 64); the
 * base 16-B aligned. Entries [0, L) are used and must be finite; entries [L, roundup(L, 64)) must
 * be readable and are ignored whatever they hold, NaN and Inf included (the kernels load aligned
 * float4s, so L needs no multiple of 4, and mask those keys before the exponent).
 * lse includes the bias and the backward recomputes P with it; no gradient with respect to
 * key_bias is produced (sizes come from the non-differentiable match, masks are data). Rejected
 * (MMT_ERR_INVALID, nothing launched): key_bias with wsum, and key_bias with the T5 `bias`.
 * With key_bias the Dh 64, 32 < L <= 320 backward always takes the two-phase resident kernel. */
int mmt_attn_fwd_keybias(const void* qkv, int64_t s_b, int64_t s_t, int B, int L, int H, int Dh,
                         float scale, int n_sets, const int32_t* set_start, const int32_t* set_len,
                         const uint32_t* set_vis, const uint32_t* drop_bits, float keep_prob,
                         const float* bias, void* o, int64_t o_s_b, int64_t o_s_t, float* lse,
                         float* wsum, const float* key_bias, int64_t kb_s_b, mmt_stream_t stream);
int mmt_attn_bwd_keybias(const void* qkv, int64_t s_b, int64_t s_t, int B, int L, int H, int Dh,
                         float scale, int n_sets, const int32_t* set_start, const int32_t* set_len,
                         const uint32_t* set_vis, const uint32_t* drop_bits,
                         const uint32_t* drop_bits_t, float keep_prob, const void* o, int64_t o_s_b,
                         int64_t o_s_t, const void* dout, int64_t d_s_b, int64_t d_s_t,
                         const float* lse, float* delta, void* dqkv, int64_t dq_s_b, int64_t dq_s_t,
                         float* bias_grad, const float* key_bias, int64_t kb_s_b,
                         mmt_stream_t stream);
/* The key_bias rows of a ToMe layer from its token sizes: kb[b, set_start + j] = logf(size[b, j])
 * for j < t (size: fp32 (B, t) contiguous, > 0; kb rows of kb_s_b floats, L <= kb_s_b). With
 * zero_rest != 0 it also writes 0 over the rest of [0, roundup(L, 64)) (tokens of unmerged sets,
 * and the padding), so one merged set is one launch with no memset; several merged sets are one
 * launch each, the first with zero_rest. */
int mmt_tome_size_bias(const float* size, int B, int t, int set_start, int L, float* kb,
                       int64_t kb_s_b, int zero_rest, mmt_stream_t stream);
/* ------------------------------------------------------------------ observation pad masks
 * Absent token sets (a dataset without a wrist camera, the history of an episode's first steps)
 * and padded instruction tokens. Upstream Octo's pad_mask_dict / timestep_pad_mask / language
 * attention mask; the reference has none. A masked token — a token of a set flagged absent for
 * its sample, or a padded token of the text set — is treated in three ways:
 *   1. it is never a key with weight: every block adds MMT_PAD_MASK_LOGIT to its key logit through
 *      the key_bias of mmt_attn_fwd_keybias / mmt_attn_bwd_keybias (mmt_pad_mask_bias);
 *   2. its content is never read: its row of the assembled sequence x0 is overwritten with
 *      pos_embedding[row] alone (mmt_pad_mask_rows_fwd, after every tokenizer has written x0);
 *      and because the image stem's GroupNorm runs over all patches of all cameras of a sample,
 *      the stem reads a copy of the images with the pixels of absent cameras zeroed
 *      (mmt_pad_mask_images), so no statistic carries them into a present camera's tokens;
 *   3. it sends no gradient to a tokenizer: its row of dx0 is zeroed (mmt_pad_mask_rows_bwd) after
 *      d(pos_embedding) has been taken from the full dx0 and before anything else reads dx0.
 * MMT_PAD_MASK_LOGIT = -1024: finite, as key_bias requires; exact in fp32, and so is its quotient
 * by a power-of-two scale (Dh 64 and 256; at Dh 128 the quotient is rounded once). Condition: a
 * masked key's weight exp(logit + M - rowmax) underflows to exactly 0 in fp32 whenever the spread
 * of the row's unmasked logits (max - min over the keys the query sees) is below about 900
 * (1024 - 900 = 124 > 104 = the fp32 denormal underflow point of exp); a larger spread leaves a
 * weight below 1e-38 times that ratio. A query whose visible keys are ALL masked (the
 * TaskDescriptionPrefix queries of an absent instruction, the queries of a set that sees only
 * itself and is absent) gets, by the shift invariance of softmax, the ordinary softmax over those
 * keys: finite, and read by no present token.
 * Left as it is: the LayerNorm runs over the sequence axis, so a masked row (its fixed content of
 * rule 2) still enters its sample's statistics — a sample with an absent set is not a model built
 * without that set; ToMe matches and merges inside an absent set as usual (sets are matched one by
 * one, so a set stays wholly present or wholly absent); the frozen T5 is not masked inside.
 *
 * Set tables (n_sets, set_start, set_len: HOST arrays, the mmt_attn_fwd convention) must tile
 * [0, L) with 1 <= n_sets <= MMT_PAD_MASK_MAX_SETS; they are those of the layer the call serves
 * (the starts follow the shrinking sequence under ToMe). words: uint32 [B] from mmt_pad_mask_pack,
 * bit s set = set s present (NULL: every set present). text_mask: bytes (B, T) contiguous,
 * nonzero = real token, for the tokens of set text_set, T == set_len[text_set] (NULL: none); at
 * least one of the two is given. Checked before any launch (MMT_ERR_INVALID): null pointers,
 * n_sets, the tiling, T, text_set, and per entry point the alignment and stride rules below. */
#define MMT_PAD_MASK_LOGIT (-1024.0f)
#define MMT_PAD_MASK_MAX_SETS 16
/* words[b] = the present-bits of set_mask (bytes (B, n_sets) contiguous, nonzero = present).
 * readout_bits: the bit mask of the Readout sets, which cannot be absent (they carry the
 * prediction): one flagged absent is reported through the device status word
 * (MMT_FAULT_PAD_MASK, mmt_device_status) and treated as present, so its bit is set. */
int mmt_pad_mask_pack(const uint8_t* set_mask, int B, int n_sets, uint32_t readout_bits,
                      uint32_t* words, mmt_stream_t stream);
/* Thin clouds become absent sets: words[b] = mmt_pad_mask_pack's result (set_mask NULL: every set
 * present, no Readout rule to apply) with bit pc_set[s] cleared where counts[b, s] <
 * min_points[s]. counts: int32 (B, S) on the DEVICE, the valid points of the S clouds of a sample
 * (mmt_depth_unproject's, or the caller's); pc_set, min_points: HOST arrays of S entries, the token
 * set of cloud s (in [0, n_sets), not a Readout set) and its token count n (a cloud with fewer
 * points than tokens is absent; min_points >= 0). 1 <= S <= n_sets. No host synchronisation: a
 * replayed graph follows new contents of counts. Counts say nothing about cameras:
 * mmt_pad_mask_images is for a caller's own set mask. */
int mmt_pad_mask_pack_counts(const uint8_t* set_mask, int B, int n_sets, uint32_t readout_bits,
                             const int32_t* counts, int S, const int32_t* pc_set,
                             const int32_t* min_points, uint32_t* words, mmt_stream_t stream);
/* dst = src (B, I, image_bytes: the camera images, any pixel type) with the image_bytes of
 * image (b, i) zeroed where set image_set[i] (HOST array of I set indices in [0, n_sets)) is
 * absent in words[b]. src is not changed; src != dst, both 16-B aligned, image_bytes a multiple of
 * 16 (16-B vector moves), I <= 16, B * I <= 65535. A zero byte is pixel 0 (uint8) or 0.0 (fp32). */
int mmt_pad_mask_images(const uint32_t* words, const int32_t* image_set, int n_sets, int B, int I,
                        int64_t image_bytes, const void* src, void* dst, mmt_stream_t stream);
/* The key_bias rows of one layer: kb fp32, row b at kb + b*kb_s_b, 16-B aligned, kb_s_b a multiple
 * of 4 and >= roundup(L, 64). accumulate == 0: kb[b, l] = MMT_PAD_MASK_LOGIT (masked) or 0 over
 * [0, L) and 0 over the padding [L, roundup(L, 64)). accumulate != 0: kb[b, l] +=
 * MMT_PAD_MASK_LOGIT on the masked entries and nothing else is touched — launched after
 * mmt_tome_size_bias has written the rows (proportional attention: the two biases add). */
int mmt_pad_mask_bias(const uint32_t* words, int B, int L, int n_sets, const int32_t* set_start,
                      const int32_t* set_len, const uint8_t* text_mask, int text_set, int T,
                      float* kb, int64_t kb_s_b, int accumulate, mmt_stream_t stream);
/* x0[b, l, :] = pe[l, :] on the masked rows of the fp32 (B, L, D) sequence (row (b, l) at
 * x0 + b*xs_b + l*xs_t; pe fp32 (L, D) contiguous); rows of present tokens are neither read nor
 * written. D % 4 == 0, x0 and pe 16-B aligned, xs_t >= D, xs_b >= (L-1)*xs_t + D, both strides
 * multiples of 4 (rows move as 16-B vectors). The set table is layer 0's. */
int mmt_pad_mask_rows_fwd(const uint32_t* words, int B, int L, int D, int n_sets,
                          const int32_t* set_start, const int32_t* set_len,
                          const uint8_t* text_mask, int text_set, int T, const float* pe,
                          float* x0, int64_t xs_b, int64_t xs_t, mmt_stream_t stream);
/* dx0[b, l, :] = 0 on the same rows, in place; the same rules. */
int mmt_pad_mask_rows_bwd(const uint32_t* words, int B, int L, int D, int n_sets,
                          const int32_t* set_start, const int32_t* set_len,
                          const uint8_t* text_mask, int text_set, int T, float* dx0, int64_t xs_b,
                          int64_t xs_t, mmt_stream_t stream);
/* Keep mask of a dropout stream (flax Dropout keep-mask, broadcast over batch and heads for
 * attention): keep(r, c) iff keep_elem(key(rng, layer, site), r*cols + c), i.e. the 16-bit half
 * (idx & 1) of mix32(key ^ (idx >> 1)) is below floor(keep_prob * 65536).
 * out_t == NULL: row-major words (rows, ceil(cols/32)), bit j of word (r, w) = keep(r, 32w + j).
 * out_t != NULL (attention, rows == cols == L): two word-major images of W = ceil(L/32) rows of
 * LP = roundup(L, 64) words, positions interleaved pos(8g + 4h + i) = 8g + 2i + h, zero past L:
 *   out   (query words): bit j of word (w, pos(k)) = keep(32w + j, k)
 *   out_t (key words):   bit j of word (w, pos(q)) = keep(q, 32w + j)
 * so that the 64-bit pair 16u + r of a 64-aligned tile's words is the wave lane mask of MFMA
 * accumulator register r of the tile's 32-wide half u (read into SGPRs by the attention kernels). */
int mmt_dropout_bits(const uint32_t* rng, uint32_t layer, uint32_t site, int rows, int cols,
                     float keep_prob, uint32_t* out, uint32_t* out_t, mmt_stream_t stream);

/* ------------------------------------------------------------------ sequence LayerNorm
 * flax.linen.LayerNorm(reduction_axes=[1], feature_axes=[-1], epsilon) as used in
 * attention.py:58,66 (vanilla_decoder.yaml:5-13): stats per (b, d) over the SEQUENCE axis L,
 * fast variance; x (B, L, D) strided, bf16 or fp32 (x_dtype; the training path keeps the residual
 * stream in fp32 because this normalisation subtracts a large per-feature sequence mean); y bf16;
 * mean/rstd fp32 (B, D) saved for the backward.
 * Operand rules, the same for the five entry points of the family (mmt_seqnorm_fwd,
 * mmt_seqnorm_bwd, mmt_seqnorm_dropout_bwd, mmt_ln_unmerge_dropout_bwd and
 * mmt_tome_merge_seqnorm_fwd), checked before anything is launched (MMT_ERR_INVALID): every
 * (B, L, D) operand (x, y, dy, addend, dx, z, g_in, x_out) is moved as 16-B vectors, so its base
 * pointer is 16-B aligned, its row and batch strides are multiples of 8 elements and its row
 * stride is at least D; B, L, D > 0 and D % 8 == 0. addend is optional (NULL: its strides are
 * ignored). mean, rstd (B, D), gamma, beta, dgamma, dbeta, colsum / bias_grad [D] are contiguous
 * fp32 read and written one element at a time. Nothing outside rows [0, L) x columns [0, D) of a
 * sample is read or written; dgamma, dbeta and the column sums are ACCUMULATED at [0, D). */
/* The kernel form that the last call of one of those five entry points launched:
 * MMT_NORM_ROUTE_NONE after a call rejected before any launch, else the entry point's code, the
 * rows per thread of the register-resident form MMT_NORM_ROUTE_RPT (4 / 6 / 8 / 10 for
 * L <= 128 / 192 / 256 / 320 rows — L2 of mmt_ln_unmerge_dropout_bwd, L - r of
 * mmt_tome_merge_seqnorm_fwd — taken only for fp32 x with bf16 dy; 0: the two-pass form, also
 * with MMT_SNB_RPT=0 in the environment), and MMT_NORM_ROUTE_X_BF16 / _DY_BF16 for the operand
 * types (dy: the backward entries). Process-wide, not thread-safe. */
enum {
  MMT_NORM_ROUTE_NONE = 0,
  MMT_NORM_ROUTE_SEQ_FWD = 1,         /* mmt_seqnorm_fwd: seqnorm_fwd_kernel */
  MMT_NORM_ROUTE_SEQ_BWD = 2,         /* mmt_seqnorm_bwd: seqnorm_bwd_kernel */
  MMT_NORM_ROUTE_SEQ_DROPOUT_BWD = 3, /* mmt_seqnorm_dropout_bwd: seqnorm_bwd_kernel<DZ> */
  MMT_NORM_ROUTE_LN_UNMERGE_BWD = 4,  /* mmt_ln_unmerge_dropout_bwd */
  MMT_NORM_ROUTE_MERGE_SEQ_FWD = 5,   /* mmt_tome_merge_seqnorm_fwd */
  MMT_NORM_ROUTE_ENTRY_MASK = 0xff,
  MMT_NORM_ROUTE_X_BF16 = 0x10000,
  MMT_NORM_ROUTE_DY_BF16 = 0x20000
};
#define MMT_NORM_ROUTE_RPT(route) (((route) >> 8) & 0xf)
int mmt_norm_last_route(void);
int mmt_seqnorm_fwd(const void* x, int x_dtype, int64_t xs_b, int64_t xs_t, int B, int L, int D,
                    const float* gamma, const float* beta, float eps, void* y, int64_t ys_b,
                    int64_t ys_t, float* mean, float* rstd, mmt_stream_t stream);
/* dx = LN backward (+ addend, which may alias dx); x, addend and dx have x_dtype, dy has
 * dy_dtype; dgamma/dbeta fp32 [D] are ACCUMULATED. */
int mmt_seqnorm_bwd(const void* dy, int dy_dtype, int64_t ds_b, int64_t ds_t, const void* x,
                    int x_dtype, int64_t xs_b, int64_t xs_t, int B, int L, int D,
                    const float* mean, const float* rstd,
                    const float* gamma, const void* addend, int64_t as_b, int64_t as_t, void* dx,
                    int64_t dxs_b, int64_t dxs_t, float* dgamma, float* dbeta,
                    mmt_stream_t stream);
/* mmt_seqnorm_bwd (bf16 dy, fp32 x / addend / dx) that also applies the dropout backward of the
 * PREVIOUS block's MLP output (layer, site, keep_prob, row_offset; rng NULL = a plain cast) to
 * the dx it writes: z (B, L, D) bf16 = keep ? dx / keep_prob : 0, colsum += its column sums (as
 * mmt_dropout_bwd), without reading dx back. */
int mmt_seqnorm_dropout_bwd(const void* dy, int64_t ds_b, int64_t ds_t, const float* x,
                            int64_t xs_b, int64_t xs_t, int B, int L, int D, const float* mean,
                            const float* rstd, const float* gamma, const float* addend,
                            int64_t as_b, int64_t as_t, float* dx, int64_t dxs_b, int64_t dxs_t,
                            float* dgamma, float* dbeta, const uint32_t* rng, uint32_t layer,
                            uint32_t site, float keep_prob, int64_t row_offset, void* z,
                            int64_t zs_b, int64_t zs_t, float* colsum, mmt_stream_t stream);

/* ------------------------------------------------------------------ reductions / dropout
 * out[n] += sum_m x[m][n] (bf16 x, fp32 out): Dense bias gradients. */
int mmt_colsum(const void* x, int dtype, int64_t ldx, int M, int N, float* out,
               mmt_stream_t stream);
/* Backward of a GEMM-epilogue dropout (flax.linen.Dropout, attention.py:34-37,60):
 * dz = dy * keep / keep_prob (bf16) with the same stream/counters as the forward (rng NULL:
 * keep everything — a cast); colsum (optional) += column sums of dz (the bias gradient of the
 * Dense before the dropout). dy: bf16 or fp32 (dtype). */
int mmt_dropout_bwd(const void* dy, int dtype, int64_t ldy, int M, int N, const uint32_t* rng,
                    uint32_t layer, uint32_t site, float keep_prob, int64_t row_offset, void* dz,
                    int64_t ldz, float* colsum, mmt_stream_t stream);

/* ------------------------------------------------------------------ image tokenizer stem
 * Operand rules of the stem entry points (csrc/stem.hip), checked before anything is launched
 * (MMT_ERR_INVALID, the message names the entry point). Every tensor is contiguous. A pointer
 * that its kernels move as vectors or dwords must be aligned to that width, whichever kernel
 * form the shape selects; every other pointer is read and written one element at a time:
 *   mmt_patch_im2col        out 16 B (16-B and 8-B stores); img 4 B (dword reads of uint8
 *                           pixels, fp32 pixels); B, I, Himg, C, P, KH, KW, S > 0, Himg % P == 0,
 *                           KH, KW <= P, KH*KW*C % 8 == 0, in_dtype 0 or 2
 *   mmt_stem_conv_pool      img 4 B (dword reads); B, I > 0, Himg >= 16, Himg % 16 == 0
 *   mmt_stem_conv_wgrad     img 4 B; the same shape rules; slab_elems >= slabs * 64 * 432
 *   mmt_maxpool_patch       npatch, win, C > 0, win <= 255 (the slot is stored in a byte)
 *   mmt_maxpool_patch_bwd   dpooled 16 B, argmax 8 B, G 16 B; npatch, win, C > 0, win <= 255,
 *                           C % 8 == 0
 *   mmt_maxpool2d, _bwd     npatch, C, KP > 0, KP*KP <= 255, OH, OW >= KP
 *   mmt_im2col_same         x 16 B, cols 16 B; npatch, H, W, C > 0, C % 8 == 0, KS > 0 and odd
 *   mmt_col2im_same         npatch, H, W, C > 0, KS > 0 and odd
 *   mmt_groupnorm_gelu_fwd  x 16 B, y 8 B; B, R, C, G > 0, C divides 256, G divides C
 *   mmt_groupnorm_gelu_bwd  dy, x, dx 16 B; the same shape rules
 *   mmt_patch_positions     B, I, P > 0, Himg % P == 0, Q > 1; rng needed in train mode
 * Nothing outside the stated extents is read or written.
 *
 * The kernel form that the last call of a stem entry point launched: MMT_STEM_ROUTE_NONE after a
 * call rejected before any launch, else the entry point's code, the form MMT_STEM_ROUTE_FORM
 * (mmt_patch_im2col: MMT_STEM_IM2COL_GENERIC / _ROWS / _LDS; mmt_groupnorm_gelu_fwd / _bwd: 0 for
 * the general kernel, else the NV = 4 / 8 / 16 / 32 float4 per thread of the register-resident
 * kernel, taken when R*C == NV*1024 with C a power of two in [4, 256]; 0 for every other entry)
 * and MMT_STEM_ROUTE_IN_U8 when mmt_patch_im2col read uint8 pixels. mmt_stem_conv_wgrad_slabs
 * launches nothing and leaves the value alone. Process-wide, not thread-safe. */
enum {
  MMT_STEM_ROUTE_NONE = 0,
  MMT_STEM_ROUTE_PATCH_IM2COL = 1,
  MMT_STEM_ROUTE_CONV_POOL = 2,
  MMT_STEM_ROUTE_CONV_WGRAD = 3,
  MMT_STEM_ROUTE_MAXPOOL_PATCH = 4,
  MMT_STEM_ROUTE_MAXPOOL_PATCH_BWD = 5,
  MMT_STEM_ROUTE_GN_GELU_FWD = 6,
  MMT_STEM_ROUTE_GN_GELU_BWD = 7,
  MMT_STEM_ROUTE_PATCH_POSITIONS = 8,
  MMT_STEM_ROUTE_MAXPOOL2D = 9,
  MMT_STEM_ROUTE_MAXPOOL2D_BWD = 10,
  MMT_STEM_ROUTE_IM2COL_SAME = 11,
  MMT_STEM_ROUTE_COL2IM_SAME = 12,
  MMT_STEM_ROUTE_ENTRY_MASK = 0xff,
  MMT_STEM_ROUTE_IN_U8 = 0x10000
};
enum { MMT_STEM_IM2COL_GENERIC = 0, MMT_STEM_IM2COL_ROWS = 1, MMT_STEM_IM2COL_LDS = 2 };
#define MMT_STEM_ROUTE_FORM(route) (((route) >> 8) & 0xff)
int mmt_stem_last_route(void);
/* tokenizers/images/image_tokenizer.py: image_to_patches (:35-71, raster "(h p1)(w p2) -> (h w)",
 * normalise 2*(x/255)-1) fused with the im2col of the input Conv (KHxKW stride S VALID, Flax HWIO
 * kernel order (ky, kx, c)), :158. img: (B, I, H, H, C) fp32 (in_dtype 0) or uint8 (in_dtype 2);
 * out: bf16 [B*I*NP*OH*OW][KH*KW*C]. H % P != 0 is rejected (the reference's resize branch,
 * :54-59, is broken). Forms: KW*C == 36 (the 12x12 RGB stem conv) takes the LDS-staged kernel for
 * uint8 pixels while 8 patches fit 64 KB of LDS as bf16 (P*C % 4 == 0, P*P*C*16 <= 65536), else
 * the row-segment kernel; every other shape the generic kernel. */
int mmt_patch_im2col(const void* img, int in_dtype, int B, int I, int Himg, int C, int P, int KH,
                     int KW, int S, int normalize, void* out, mmt_stream_t stream);
/* max_pool over the `win` conv outputs of each patch (3x3 s1 VALID on the 3x3 map, :159) with
 * first-max argmax for the backward (fp32 conv [npatch][win][C] -> fp32 pooled [npatch][C]);
 * the backward scatters fp32 dpooled into the bf16 conv-output gradient G [npatch][win][C]. */
/* The stem's input conv and pool fused (image_tokenizer.py:35-71,140-162 at its gato_resnet
 * configuration): for every 16x16 patch of uint8 RGB images (B, I, H, H, 3), normalised as
 * 2 * (x / 255) - 1, the 12x12 stride-2 VALID conv with w (64, 432) bf16 [out][(ky, kx, c)] plus
 * bias, then the max over its 3x3 map: pooled (B*I*NP, 64) fp32 and the first-maximum position
 * argmax (B*I*NP, 64) uint8 (as mmt_maxpool_patch), without the im2col matrix. */
int mmt_stem_conv_pool(const void* img, int B, int I, int Himg, const void* w, const float* bias,
                       float* pooled, uint8_t* argmax, mmt_stream_t stream);
/* Its weight gradient without im2col: dw (64, 432) += sum over patches and conv positions of
 * G^T A, G the max-pool backward of dpooled (B*I*NP, 64) fp32 at argmax (bf16-rounded, as
 * mmt_maxpool_patch_bwd), A the normalised patch pixels: each of mmt_stem_conv_wgrad_slabs(B, I,
 * Himg) workgroups writes its partial (64, 432) to slab row i (caller-owned fp32), which the
 * caller sums into dw (mmt_colsum). */
int mmt_stem_conv_wgrad_slabs(int B, int I, int Himg);
int mmt_stem_conv_wgrad(const void* img, int B, int I, int Himg, const float* dpooled,
                        const uint8_t* argmax, float* slab, int64_t slab_elems,
                        mmt_stream_t stream);
int mmt_maxpool_patch(const void* conv, int64_t npatch, int win, int C, void* pooled,
                      uint8_t* argmax, mmt_stream_t stream);
int mmt_maxpool_patch_bwd(const void* dpooled, const uint8_t* argmax, int64_t npatch, int win,
                          int C, void* G, mmt_stream_t stream);
/* General stem maps (pooled map larger than 1 x 1: the reference's patch 56, 23 x 23 conv map,
 * image_tokenizer.py:156-176 with gato_resnet.yaml:45-92):
 * max_pool KP x KP stride 1 VALID over (npatch, OH, OW, C) fp32 -> (npatch, OH-KP+1, OW-KP+1, C)
 * plus the first-maximum window slot; its backward writes the bf16 (npatch, OH, OW, C) operand of
 * the conv weight gradient (gather over the windows, deterministic). */
int mmt_maxpool2d(const void* x, int64_t npatch, int OH, int OW, int C, int KP, void* y,
                  uint8_t* argmax, mmt_stream_t stream);
int mmt_maxpool2d_bwd(const void* dy, const uint8_t* argmax, int64_t npatch, int OH, int OW, int C,
                      int KP, void* G, mmt_stream_t stream);
/* KS x KS stride-1 SAME convolution as im2col (bf16 (npatch, H, W, C) -> (npatch*H*W, KS*KS*C) in
 * Flax HWIO (ky, kx, c) order, zero padding) + GEMM; col2im sums the fp32 column gradient back. */
int mmt_im2col_same(const void* x, int64_t npatch, int H, int W, int C, int KS, void* cols,
                    mmt_stream_t stream);
int mmt_col2im_same(const float* dcols, int64_t npatch, int H, int W, int C, int KS, float* dx,
                    mmt_stream_t stream);
/* flax GroupNorm(num_groups=G, eps) over every non-batch axis + gelu(tanh approx)
 * (gato_resnet.yaml:77-86, image_tokenizer.py:165-167): x (B, R, C) fp32 -> y bf16 (the next
 * conv's GEMM operand); statistics in fp32. */
int mmt_groupnorm_gelu_fwd(const void* x, int B, int R, int C, int G, float eps,
                           const float* gamma, const float* beta, void* y, float* mean,
                           float* rstd, mmt_stream_t stream);
/* backward (dy, x, dx fp32); dx += result when accumulate != 0; dgamma/dbeta accumulated. */
int mmt_groupnorm_gelu_bwd(const void* dy, const void* x, int B, int R, int C, int G,
                           const float* gamma, const float* beta, const float* mean,
                           const float* rstd, void* dx, int accumulate, float* dgamma,
                           float* dbeta, mmt_stream_t stream);
/* encode_patch_position (:74-132) for every (b, image, patch): Q quantisation levels, row token
 * from interval p % PPD, col from p // PPD; train: randint[start, stop) on the counter stream keyed
 * by the global sample index (sample_offset + b); eval: (start + stop) // 2. */
int mmt_patch_positions(const uint32_t* rng, uint32_t site, int B, int I, int Himg, int P, int Q,
                        int train, int64_t sample_offset, int32_t* row_tok, int32_t* col_tok,
                        mmt_stream_t stream);

/* ------------------------------------------------------------------ sequence assembly
 * x0[b, l] = source(l) + pe[l] with source = text[b, j] | img[b, j] + row_emb[rtok] + col_emb[ctok]
 * | readout_pe[j]  (row_src[l] = kind << 24 | j, kind 0 text / 1 image / 2 readout; a row of
 * kind 3, a value token, or 4, a point-cloud token, is left untouched by both directions:
 * mmt_value_tokens_fwd / _bwd, mmt_pc_embed_fwd / _bwd):
 * TokenSequence.assemble_embeddings (token_sequencer.py:255-269), readout AddPositionEmbedding
 * on zeros (readout.py:18-33, octo.py:103-108), ImageTokenizer embeddings (:300-307) and the
 * encoder's learned position embedding (attention.py:71-85,97-100), fused. fp32 tables.
 * D > 0, D % 8 == 0; text, img and x0 are read / written as 16-B vectors: 16-B aligned bases. */
int mmt_seq_assemble_fwd(int B, int L, int D, const int32_t* row_src, const void* text, int T,
                         const void* img, int NI, const int32_t* rtok, const int32_t* ctok,
                         const float* row_emb, const float* col_emb, const float* readout_pe,
                         const float* pe, void* x0, mmt_stream_t stream);
/* backward: gathers d(text), d(img) (bf16) from the fp32 dx0, accumulates d(readout_pe) and the
 * (Q, D) row/col embedding gradients (LDS histograms per 64-column slice, then one global
 * atomic per table entry). img_rows[j] = sequence row of image token j. d(pe) is mmt_colsum
 * over the batch. dtext NULL: the text rows are skipped (frozen text encoder). D > 0,
 * D % 8 == 0; dx0, dtext and dimg are 16-B vectors: 16-B aligned bases. */
int mmt_seq_assemble_bwd(int B, int L, int D, const int32_t* row_src, const void* dx0,
                         void* dtext, int T, void* dimg, int NI, const int32_t* rtok,
                         const int32_t* ctok, const int32_t* img_rows, int Q, float* drow_emb,
                         float* dcol_emb, float* dreadout_pe, mmt_stream_t stream);
/* The image row / column position-embedding gradients alone (drow_emb = dcol_emb = NULL above):
 * d(row_emb)[t] += dx0[b, img_rows[j]] over the image tokens (b, j) whose row token (rtok, from
 * mmt_patch_positions) is t, likewise columns. A patch row's tokens lie in one window of the
 * table (patch_positions' q(ri P) .. q((ri + 1) P)), so a workgroup owns one window and keeps a
 * register accumulator per window token: no LDS atomics (the form above: 268 -> ~40 us per step
 * at OCTO-small B = 256). I images of Himg x Himg pixels, patch P, table Q rows per axis, dx0
 * fp32 (B, L, D), tables fp32 (Q, D) accumulated. */
int mmt_patch_embed_grad(int B, int L, int D, int I, int Himg, int P, int Q,
                         const int32_t* img_rows, const void* dx0, const int32_t* rtok,
                         const int32_t* ctok, float* drow_emb, float* dcol_emb,
                         mmt_stream_t stream);
/* AddPositionEmbedding standalone (tokenizers/readout/readout.py:18-33; also attention.py:71-85):
 * out (B, L, D) fp32 = x + pe[None] (x may alias out). Backward: dx = dout; d(pe) = mmt_colsum of
 * dout viewed as (B, L*D). The training step fuses this add into mmt_seq_assemble_fwd. */
int mmt_add_position_embedding(const float* x, const float* pe, float* out, int B, int L, int D,
                               mmt_stream_t stream);
/* readout gather + mean (octo.py:122-124, diffusion.py:102): out[b] = mean_i x[b, rows[i]]
 * (x fp32 with element strides xs_b, xs_t; out bf16, row stride ld_out; B, D, nrows > 0). */
int mmt_rows_mean_fwd(const void* x, int64_t xs_b, int64_t xs_t, int B, int D,
                      const int32_t* rows, int nrows, void* out, int64_t ld_out,
                      mmt_stream_t stream);
/* backward: writes the whole contiguous fp32 dx (B, L, D), no zeroing needed first: de[b] / nrows
 * in the rows with row_flag[l] >= 0, 0 in every other row (de bf16, row stride ld_de). */
int mmt_rows_mean_bwd(const void* de, int64_t ld_de, int B, int L, int D, const int32_t* row_flag,
                      int nrows, void* dx, mmt_stream_t stream);

/* ------------------------------------------------------------------ value tokens
 * Low-dimensional numbers (proprioception: joint angles, gripper opening, end-effector pose, the
 * previous action) as sequence rows (csrc/values.hip): the reference's Gato-style pieces,
 * tokenizers/numeric_values/value_tokenizer.py:18-34: mu_law_encoder companding (:33-34), uniform
 * bins, one nn.Embed table over the discrete ids (ActionTokenizer, :18-30). Values are expected
 * normalised to [-1, 1]. For a value v, N = num_bins, all in fp32:
 *   s = fminf(fmaxf(v, -1), 1)                       clamp; IEEE fmax / fmin send NaN to -1
 *   y = s                                            MMT_VALUE_UNIFORM
 *   y = copysign(log1pf(mu |s|) / log1pf(mu), s)     MMT_VALUE_MU_LAW
 *   token = min(N - 1, (int)floorf((y + 1) * 0.5f * N))
 * so -1, -inf and NaN give token 0, 0 gives N / 2, and 1, +inf and anything above 1 give N - 1.
 * The row of value j of sample b: x0[b, rows[j], :] = table[token(b, j), :] + pe[rows[j], :], one
 * fp32 add (bit-exact). table (N, D) fp32 is shared by every value; pe (the encoder's learned
 * position embedding, one row per sequence position) tells the slots apart.
 *
 * Forward. values fp32 (B, n) with row stride ld_v >= n; rows (n,) int32, the sequence row of each
 * value; x0 fp32 with element strides xs_b, xs_t. Writes tok (B, n) int32 (kept for the backward)
 * and the n rows of x0 per sample as 16-B vectors, no other row (mmt_seq_assemble_fwd skips the
 * rows of kind 3, which these are). Checked before the launch (MMT_ERR_INVALID): null pointers;
 * B, n <= 0; D <= 0 or D % 8 != 0; num_bins outside MMT_VALUE_MIN_BINS .. MMT_VALUE_MAX_BINS; an
 * unknown encoding; mu <= 0 or not finite (mu-law only); x0 or table not 16-B aligned; xs_t < D;
 * xs_b or xs_t not a multiple of 4. A row outside its sample (rows[j] < 0 or rows[j] * xs_t + D >
 * xs_b) is not written: MMT_FAULT_ROW_INDEX. */
enum { MMT_VALUE_UNIFORM = 0, MMT_VALUE_MU_LAW = 1 };
#define MMT_VALUE_MIN_BINS 2
#define MMT_VALUE_MAX_BINS 4096
int mmt_value_tokens_fwd(const float* values, int64_t ld_v, int B, int n, int encoding, float mu,
                         int num_bins, const float* table, const float* pe, const int32_t* rows,
                         int D, void* x0, int64_t xs_b, int64_t xs_t, int32_t* tok,
                         mmt_stream_t stream);
/* Backward: dtable[k, :] += sum of dx0[b, rows[j], :] over the tokens tok[b, j] == k. The sum is
 * formed in ONE fp32 accumulator per table entry in ascending (b, j) order and then added once to
 * dtable (which holds zero after zero_grad): each entry has one writer and a fixed order, so there
 * are no float atomics, the result is bitwise reproducible with and without the deterministic
 * mode, and it equals a sequential fp32 sum in that order bit for bit. d(pe) is mmt_colsum over
 * dx0, as for every other row; no gradient reaches the values. dx0 fp32, strides as above. The
 * same checks as the forward (dx0 and dtable 16-B aligned). A tok entry outside [0, num_bins) or a
 * row outside its sample is skipped: MMT_FAULT_ROW_INDEX. */
int mmt_value_tokens_bwd(const void* dx0, int64_t xs_b, int64_t xs_t, int B, int n,
                         const int32_t* tok, const int32_t* rows, int D, int num_bins,
                         float* dtable, mmt_stream_t stream);

/* ------------------------------------------------------------------ point-cloud tokens
 * A point cloud (P, C) fp32 (the first three features are xyz; C in 3 .. 8, the extras colour or
 * normals) as n sequence rows, one per sampled centroid with its neighbourhood (csrc/
 * pointcloud.hip): the reference's tokenizers/pointclouds/point_cloud_tokenizer.py (farthest-point
 * sampling :42-92, kNN grouping :106-116, SampleAndGroupModule :119-198), restated. All fp32.
 *   d(p, c) = (dx dx + dy dy) + dz dz, dx = p.x - c.x ..., every operation individually rounded
 *             (no FMA): numpy float32 reproduces it bit for bit
 *   sampling: dist = +inf, ids[0] = start; for i = 1 .. n-1: dist = min(dist, d(., ids[i-1])),
 *             ids[i] = argmax over the points not yet sampled, the lowest index on ties
 *   grouping: per centroid the k points of smallest d, ascending by (d, index)
 *   features: neighbour j of centroid c: [points[j] - points[c], points[j]] (2 C numbers)
 *   embedding: h1 = relu(feat W1 + b1), h2 = relu(h1 W2 + b2), g = max over the k neighbours of
 *             h2, row = (g W_out + b_out) + pe[row]; W1 (2C, F1), W2 (F1, F2), W_out (F2, D),
 *             F1, F2 in {32, 64, 128}
 * Limits (MMT_ERR_INVALID before a launch): max(n, k) <= P <= MMT_PC_MAX_POINTS, 1 <= n <=
 * MMT_PC_MAX_TOKENS, 1 <= k <= MMT_PC_MAX_NEIGHBOURS, MMT_PC_MIN_FEATURES <= C <=
 * MMT_PC_MAX_FEATURES. points: cloud (b, s) starts at points + b ld_b + s ld_s (elements) and is
 * contiguous (P, C). Non-finite coordinates are the caller's error: every index written is still
 * in [0, P), the result is otherwise unspecified.
 *
 * mmt_pc_sample_group: centroid_idx (B, S, n) and neighbour_idx (B, S, n, k) int32. The start of
 * cloud (b, s) is start[b S + s] if start is non-null (outside [0, P): 0 and
 * MMT_FAULT_ROW_INDEX), else, with rng (the two-word RNG state) non-null, the draw
 * (draw_u32(stream_key(seed, step, 0xFFF7, 1), (sample_offset + b) S + s) * P) >> 32, else 0. */
#define MMT_PC_MAX_POINTS 4096
#define MMT_PC_MAX_TOKENS 256
#define MMT_PC_MAX_NEIGHBOURS 32
#define MMT_PC_MIN_FEATURES 3
#define MMT_PC_MAX_FEATURES 8
#define MMT_PC_MAX_WIDTH 4096
int mmt_pc_sample_group(const float* points, int64_t ld_b, int64_t ld_s, int B, int S, int P, int C,
                        int n, int k, const int32_t* start, const uint32_t* rng,
                        int64_t sample_offset, int32_t* centroid_idx, int32_t* neighbour_idx,
                        mmt_stream_t stream);
/* Ragged clouds: counts int32 (B S) on the device, c = counts[b S + s] = the number of leading
 * rows of cloud (b, s) that are points; NULL = mmt_pc_sample_group (every cloud has P points, the
 * same kernel instantiation, launches and bits). P stays the row stride and the limit above.
 *   count    outside [0, P]: clamped into it, MMT_FAULT_ROW_INDEX
 *   rows >= c are never read: their contents (NaN and Inf included) influence no output
 *   start    injected: start >= c gives 0 and MMT_FAULT_ROW_INDEX (any start when c == 0); drawn:
 *            (draw_u32(...) * c) >> 32, 0 when c == 0; else 0
 *   sampling the rule above over the rows < c for i < min(n, c); for i >= c >= 1 ids[i] =
 *            ids[i - c] (periodic repeat); c == 0: every index 0
 *   grouping the min(k, c) nearest among the rows < c, ascending by (d, index); the slots r >= c
 *            repeat slot 0, the nearest point (the centroid itself or its lowest-index duplicate,
 *            d = 0): the PointNet++ "pad with the first" convention; c == 0: every index 0
 * Every index written is in [0, max(c, 1)). mmt_pc_embed_fwd / _bwd take these indices unchanged:
 * the max over the neighbours records the FIRST slot that attains it, so a repeated slot changes
 * neither the pooled value nor the arg-max and receives no gradient. A cloud with c < n gives
 * repeated tokens; Octo treats it as an absent set (mmt_pad_mask_pack_counts). */
int mmt_pc_sample_group_counts(const float* points, int64_t ld_b, int64_t ld_s, int B, int S, int P,
                               int C, int n, int k, const int32_t* start, const uint32_t* rng,
                               int64_t sample_offset, const int32_t* counts, int32_t* centroid_idx,
                               int32_t* neighbour_idx, mmt_stream_t stream);
/* Forward of the embedding: writes x0[b, rows[s n + m], :] for token m of cloud (b, s) and no
 * other row (mmt_seq_assemble_fwd skips the rows of kind 4, which these are), and argmax
 * (B, S, n, F2) uint8, the first neighbour slot that attains each maximum. rows (S n,) int32; pe
 * (L, D) fp32 contiguous; x0 fp32 with element strides xs_b, xs_t; D a multiple of 4, at most
 * MMT_PC_MAX_WIDTH. An index of centroid_idx / neighbour_idx outside [0, P) is read as 0, a row
 * outside its sample is not written: MMT_FAULT_ROW_INDEX. */
int mmt_pc_embed_fwd(const float* points, int64_t ld_b, int64_t ld_s, int B, int S, int P, int C,
                     int n, int k, const int32_t* centroid_idx, const int32_t* neighbour_idx, int F1,
                     int F2, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w_out, const float* b_out, const float* pe, const int32_t* rows,
                     int D, void* x0, int64_t xs_b, int64_t xs_t, uint8_t* argmax,
                     mmt_stream_t stream);
/* Backward: the gradients of the six parameter tensors from the rows of dx0 (none reaches the
 * points; d(pe) is mmt_colsum over dx0). The hidden activations are recomputed. The max routes
 * its gradient to the saved arg-max slot; relu'(0) = 0. Token chunks of a size that depends on
 * B S n alone write partial gradients with one owner per element to the workspace; each gradient
 * element is then the sum of its partials in ascending chunk order, added ONCE to the gradient
 * buffer: no float atomics, bitwise reproducible with and without the deterministic mode.
 * workspace: >= mmt_pc_embed_bwd_workspace(...) bytes, 16-B aligned. An argmax entry >= k is read
 * as 0: MMT_FAULT_ROW_INDEX. */
int64_t mmt_pc_embed_bwd_workspace(int B, int S, int n, int C, int F1, int F2, int D);
int mmt_pc_embed_bwd(const void* dx0, int64_t xs_b, int64_t xs_t, const int32_t* rows, int D,
                     const float* points, int64_t ld_b, int64_t ld_s, int B, int S, int P, int C,
                     int n, int k, const int32_t* centroid_idx, const int32_t* neighbour_idx,
                     const uint8_t* argmax, int F1, int F2, const float* w1, const float* b1,
                     const float* w2, const float* b2, const float* w_out, float* dw1, float* db1,
                     float* dw2, float* db2, float* dw_out, float* db_out, void* workspace,
                     int64_t workspace_bytes, mmt_stream_t stream);

/* ------------------------------------------------------------------ depth back-projection
 * A depth image (H, W) with pinhole intrinsics as a point cloud of at most P points and its count
 * (csrc/depth.hip), the input of mmt_pc_sample_group_counts. depth: (B, S, H, W) contiguous, uint16
 * (depth_is_f32 == 0; millimetres with depth_scale 0.001) or fp32; intrinsics fp32 (B, S, 4) =
 * fx fy cx cy; pose fp32 (B, S, 3, 4) = [R | t] camera -> base, row-major, NULL: the camera frame;
 * rgb uint8 (B, S, H, W, 3) or NULL; points fp32 (B, S, P, C) contiguous, C = 6 with rgb, else 3;
 * counts int32 (B, S). Every operation is individually rounded (numpy float32 restates the bits):
 *   z      = fmul(float(d), depth_scale)
 *   valid  uint16: d != 0; fp32: d > 0 and finite (a NaN is invalid); both: z_min <= z <= z_max
 *   x      = fdiv(fmul(fsub(float(u), cx), z), fx), y likewise from the row v, cy, fy
 *   pose   p'_i = fadd(fadd(fadd(fmul(R_i0, x), fmul(R_i1, y)), fmul(R_i2, z)), t_i)
 *   colour features 3 .. 5 = fdiv(float(channel), 255.f)
 *   selection: the V valid pixels are ranked in raster order, j = 0 .. V-1. V <= P: slot j holds
 *          rank j. Else slot q holds the pixel of rank ceil(q V / P) (in 64-bit integers): an evenly
 *          strided subsample, exactly P slots, strictly increasing ranks, slot 0 = rank 0.
 *   counts = min(V, P); the slots >= counts are written as zeros in all C features.
 * One writer per slot; the result does not depend on scheduling. MMT_ERR_INVALID before a launch:
 * P outside 1 .. MMT_PC_MAX_POINTS, H W > 2^20, depth not 16-B aligned or H W no multiple of 8
 * (uint16) / 4 (fp32) (images are read as 16-B vectors), depth_scale <= 0, z_min > z_max, a NaN
 * among the three. fx and fy are device data and cannot be checked at launch: with a zero or
 * non-finite one the coordinates are unspecified (Inf / NaN), every write still inside points and
 * counts, the selection and counts unaffected. */
int mmt_depth_unproject(const void* depth, int depth_is_f32, int B, int S, int H, int W,
                        const float* intrinsics, const float* pose, const uint8_t* rgb,
                        float depth_scale, float z_min, float z_max, int P, float* points,
                        int32_t* counts, mmt_stream_t stream);

/* ------------------------------------------------------------------ image augmentation
 * Random resized crop plus brightness, contrast and saturation jitter of uint8 camera frames on
 * the device (csrc/augment.hip): the Octo training recipe (primary camera: crop + colour; wrist
 * camera: colour alone), keyed like every other random stream by (seed, step, global sample).
 * images, out: uint8 (B, I, H, W, 3) contiguous, 16-B aligned, not overlapping; rng: the two-word
 * RNG state {seed, step}; image_camera: int32 (I,) on the device, the camera of each image slot;
 * cam_params: fp32 (n_cam, 9) on the device = scale_lo, scale_hi, ratio_lo, ratio_hi, brightness,
 * contrast_lo, contrast_hi, sat_lo, sat_hi per camera; params_out (optional): fp32 (B, n_cam, 8) =
 * w, h, x0, y0, d, fc, fs, 0 of every (sample, camera), for callers that move other labels with
 * the crop. Every float operation below is individually rounded to fp32 (no FMA), so numpy
 * float32 restates the pixels bit for bit.
 *   draws    one set per (global sample g = sample_offset + b, camera c), shared by every image
 *            slot of the sample with that camera (a history window is cropped and tinted alike):
 *            key = stream_key(seed, step, 0xFFF6, c), u_j = (draw_u32(key, (8 g + j) mod 2^32)
 *            >> 8) / 2^24 for j = 0 .. 6. Layer word 0xFFF6 is this entry's alone: 0xFFF7 is the
 *            point-cloud start's, 0xFFF8 the categorical decode's, 0xFFF9 .. 0xFFFF are taken
 *            (see mmt_diffusion_loss_multi).
 *   params   area = scale_lo + u0 (scale_hi - scale_lo), rho = ratio_lo + u1 (ratio_hi - ratio_lo)
 *            (uniform, not log-uniform), w = min(1, sqrt(area rho)), h = min(1, sqrt(area / rho)),
 *            x0 = u2 (1 - w), y0 = u3 (1 - h), d = ((2 u4 - 1) brightness) 255,
 *            fc = contrast_lo + u5 (contrast_hi - contrast_lo), fs = sat_lo + u6 (sat_hi - sat_lo)
 *   resample bilinear, corner-aligned (crop_and_resize): output row r samples sy = y0 (H - 1) +
 *            float(r) h, iy = min(floor(sy), H - 1), iy1 = min(iy + 1, H - 1), ty = sy - float(iy);
 *            columns likewise with x0, w, W. Per channel top = p00 + (p01 - p00) tx, bot = p10 +
 *            (p11 - p10) tx, v = top + (bot - top) ty.
 *   mean     per channel over the integer source box the crop reads, rows iy(0) .. iy1(H - 1),
 *            columns ix(0) .. ix1(W - 1): m = float(sum) / float(n), sum the exact integer sum of
 *            the bytes, n the box area, both conversions to nearest. No float enters the sum: no
 *            summation order can show in the result.
 *   colour   v1 = v + d, mb = m + d, v2 = (v1 - mb) fc + mb, gray = (0.299 r2 + 0.587 g2) +
 *            0.114 b2, v3 = gray + (v2 - gray) fs, out = uint8(rint(min(max(v3, 0), 255))), rint to
 *            even. One clamp, at the end.
 * workspace: >= mmt_image_augment_workspace(B, I) bytes, 16-B aligned (the integer partial sums,
 * MMT_AUGMENT_SPLIT per image; every word read is written by the call first). Two launches,
 * stream-ordered, graph-capturable, no allocation, no atomics. MMT_ERR_INVALID before a launch: a
 * null pointer (params_out may be), images / out / workspace not 16-B aligned or another pointer
 * not 4-B aligned, B, I, H or W < 1, H or W > MMT_AUGMENT_MAX_SIDE, I > MMT_AUGMENT_MAX_IMAGES,
 * B I > MMT_AUGMENT_MAX_FRAMES, n_cam outside 1 .. MMT_AUGMENT_MAX_CAMERAS, sample_offset < 0,
 * out overlapping images, a workspace too small. image_camera and cam_params are device data: an
 * entry of image_camera outside [0, n_cam) is read as 0 (MMT_FAULT_ROW_INDEX), and with ranges
 * that are not ordered, positive and finite the pixels are unspecified, every read and write
 * still inside the tensors (every sample index is clamped into its image). */
#define MMT_AUGMENT_MAX_SIDE 2048
#define MMT_AUGMENT_MAX_IMAGES 64
#define MMT_AUGMENT_MAX_CAMERAS 16
#define MMT_AUGMENT_MAX_FRAMES (1 << 24)
#define MMT_AUGMENT_SPLIT 8
int64_t mmt_image_augment_workspace(int B, int I);
int mmt_image_augment(const uint8_t* images, int B, int I, int H, int W, const uint32_t* rng,
                      int64_t sample_offset, const int32_t* image_camera, const float* cam_params,
                      int n_cam, uint8_t* out, float* params_out, void* workspace,
                      int64_t workspace_bytes, mmt_stream_t stream);

/* ------------------------------------------------------------------ QK-norm
 * flax.linen.SelfAttention(normalize_qk=True): LayerNorm(use_bias=False) over the head dimension of
 * the projected queries and keys before the dot product (`query_ln`, `key_ln`; the reference's
 * attention_blocks/compressed_attention.py:184-198), csrc/qknorm.hip. qkv: n_tokens rows of the
 * packed (3, H, Dh) projection, dtype MMT_F32 or MMT_BF16, row stride ld >= 3 H Dh elements, every
 * row 16-B aligned. For every token and head, for q and k separately, in fp32 over the Dh elements
 * x of the head row:
 *   mu = mean(x), var = max(0, mean(x^2) - mu^2)       Flax's fast variance
 *   y  = (x - mu) * rsqrt(var + eps) * scale           scale = q_scale (Dh) for q, k_scale for k
 * The two means are accumulated on x - x[0], which leaves var and x - mu as they are in exact
 * arithmetic and keeps the row's offset out of the fp32 cancellation; a constant row gives y = 0.
 * Forward: y overwrites q and k in place; the V third and the columns past 3 H Dh are neither read
 * nor written. qk_pre (n_tokens, 2 H Dh) contiguous, the dtype of qkv, or NULL (evaluation): the
 * pre-norm q and k, bit for bit, for the backward.
 * Checked before a launch (MMT_ERR_INVALID): null pointers; a dtype that is neither code; Dh not in
 * {32, 64, 128, 256}; n_tokens or H <= 0; ld < 3 H Dh; qkv (or qk_pre, workspace) not 16-B aligned
 * or ld not a whole number of 16-B vectors; eps < 0 or NaN. */
int mmt_qk_norm_fwd(void* qkv, int dtype, int64_t ld, int64_t n_tokens, int H, int Dh,
                    const float* q_scale, const float* k_scale, float eps, void* qk_pre,
                    mmt_stream_t stream);
/* Backward, in place on the q and k thirds of dqkv (the attention backward's output, the layout
 * and dtype rules of qkv; the V third keeps its bits): with the statistics recomputed from qk_pre,
 * xhat = (x - mu) rs, g = dy * scale,
 *   dx = rs * (g - mean(g) - xhat * mean(g * xhat))
 * and dq_scale[j] += sum over (token, head) of dy[j] * xhat[j] (dk_scale likewise), fp32 (Dh). The
 * sums are ordered: every workgroup of a grid that depends on (n_tokens, H, Dh) alone writes one
 * partial row per column to the workspace, and one wave per column adds the partial rows in a
 * fixed order and then adds the total ONCE to the gradient: one writer per element, no float
 * atomics, bitwise reproducible with and without the deterministic mode.
 * workspace: >= mmt_qk_norm_bwd_workspace(n_tokens, H, Dh) bytes (at most 2 MiB), 16-B aligned. */
int64_t mmt_qk_norm_bwd_workspace(int64_t n_tokens, int H, int Dh);
int mmt_qk_norm_bwd(void* dqkv, int dtype, int64_t ld, int64_t n_tokens, int H, int Dh,
                    const void* qk_pre, const float* q_scale, const float* k_scale, float eps,
                    float* dq_scale, float* dk_scale, void* workspace, int64_t workspace_bytes,
                    mmt_stream_t stream);

/* ------------------------------------------------------------------ attention pooling
 * MultiHeadAttentionPooling (attention_blocks/attention.py:122-150) of the readout tokens, the
 * pieces around its GEMMs (csrc/pool.hip). None of them accumulates across workgroups (no
 * atomics): batch reductions are per-sample arrays for mmt_colsum.
 *
 * Readout gather: r (B, n, D) bf16 contiguous = x[b, rows[i], :] (x fp32, element strides xs_b,
 * xs_t multiples of 4, 16-B aligned; D % 8 == 0). rows outside [0, L): MMT_FAULT_ROW_INDEX. */
int mmt_rows_gather_bf16(const void* x, int64_t xs_b, int64_t xs_t, int B, int L, int D,
                         const int32_t* rows, int n, void* r, mmt_stream_t stream);
/* backward, mmt_rows_mean_bwd's contract: writes the whole contiguous fp32 dx (B, L, D):
 * dr[b, row_flag[l], :] (dr bf16 (B, n, D) contiguous) where row_flag[l] >= 0, 0 in every other
 * row. row_flag[l] >= n: MMT_FAULT_ROW_INDEX. */
int mmt_rows_scatter_bwd(const void* dr, int B, int L, int D, const int32_t* row_flag, int n,
                         void* dx, mmt_stream_t stream);
/* Single-query multi-head attention core. q (H * Dh) fp32: the projected, scaled query, shared by
 * the batch; k, v bf16, row (b, j) at (b * n + j) * ld_kv (both may be halves of one (B n, 2 D)
 * GEMM output); p (B, H, n) fp32 = softmax_j(q_h . k_bjh) (fp32 scores, max-subtracted), saved for
 * the backward; ctx (B, H * Dh) bf16, row stride ld_ctx, = sum_j p v accumulated in fp32.
 * 1 <= n <= 64, Dh % 8 == 0, Dh <= 512, strides multiples of 8, 16-B aligned bases. */
int mmt_attn_pool_fwd(const float* q, const void* k, const void* v, int64_t ld_kv, int B, int n,
                      int H, int Dh, void* ctx, int64_t ld_ctx, float* p, mmt_stream_t stream);
/* backward: dctx (B, H * Dh) bf16, row stride ld_dctx. dv[b,j,h,:] = p[b,h,j] dctx[b,h,:] and
 * dk[b,j,h,:] = ds[b,h,j] q[h,:] (bf16, row stride ld_dkv), ds = p (dp - sum_j p dp), dp[b,h,j] =
 * dctx[b,h,:] . v[b,j,h,:]; dqb (B, H * Dh) fp32 contiguous = sum_j ds[b,h,j] k[b,j,h,:], the
 * per-sample query gradient (d(q) = its column sum). */
int mmt_attn_pool_bwd(const void* dctx, int64_t ld_dctx, const float* p, const float* q,
                      const void* k, const void* v, int64_t ld_kv, int B, int n, int H, int Dh,
                      void* dk, void* dv, int64_t ld_dkv, float* dqb, mmt_stream_t stream);
/* flax.linen.LayerNorm over the FEATURE axis (reduction_axes [-1]) of (B, D) rows: fast variance
 * max(0, E[x^2] - E[x]^2), y = (x - mean) (rsqrt(var + eps) gamma) + beta. x fp32 or bf16
 * (x_dtype), row stride ldx; y bf16, row stride ldy; mean, rstd fp32 (B). D % 8 == 0. */
int mmt_layernorm_fwd(const void* x, int x_dtype, int64_t ldx, int B, int D, const float* gamma,
                      const float* beta, float eps, void* y, int64_t ldy, float* mean, float* rstd,
                      mmt_stream_t stream);
/* dx = LN backward (+ addend, which may alias dx); x, addend and dx have x_dtype, dy has dy_dtype
 * (as mmt_seqnorm_bwd). dyxhat (B, D) fp32 contiguous = dy xhat per row: d(scale) is its column
 * sum and d(bias) the column sum of dy (mmt_colsum). */
int mmt_layernorm_bwd(const void* dy, int dy_dtype, int64_t ld_dy, const void* x, int x_dtype,
                      int64_t ldx, int B, int D, const float* mean, const float* rstd,
                      const float* gamma, const void* addend, int64_t ld_add, void* dx,
                      int64_t ld_dx, float* dyxhat, mmt_stream_t stream);

/* ------------------------------------------------------------------ diffusion head
 * DiffusionActionHead.denoise_loss (diffusion.py:110-143) pieces: t ~ U{0..steps-1}, eps ~ N(0,1)
 * (or injected), noisy = sqrt(abar_t) a + sqrt(1-abar_t) eps written to cat[:, :A] (bf16),
 * FourierFeatures (:41-51) [cos 2 pi t W, sin 2 pi t W] (bf16 (B, 2F)). steps, A, F > 0,
 * ld_cat >= A. */
int mmt_diffusion_prep(const uint32_t* rng, int B, int A, int steps, int64_t sample_offset,
                       const float* actions, const float* alpha_hats, const float* fourier_w,
                       int F, const int32_t* t_in, const float* eps_in, int32_t* t_out,
                       float* eps_out, void* cat, int64_t ld_cat, void* feats,
                       mmt_stream_t stream);
int mmt_fourier_bwd(const void* dfeats, int B, int F, const int32_t* t, const float* fourier_w,
                    float* dw, mmt_stream_t stream);
/* optax.l2_loss summed over actions, mean over batch; dpred = (pred-eps)*grad_scale/B (bf16,
 * (B, A) contiguous). loss[0] is overwritten, not accumulated. ld_pred >= A, B * A fits int. */
int mmt_diffusion_loss(const float* pred, int64_t ld_pred, const float* eps, int B, int A,
                       float grad_scale, float* loss, void* dpred, mmt_stream_t stream);
/* DiffusionActionHead.predict_action (diffusion.py:146-209), SURVEY §8f row 2: all `steps`
 * DDPM steps (t = steps-1 .. 0) in one launch, one wave per sample. The first denoiser Dense is
 * pre-split by the caller: P (B, H) fp32 = readout_mean . W1[:, A+T:]^T, Q (steps, H) fp32 =
 * time_emb(t) . W1[:, A:A+T]^T + b1; w1 is the bf16 W1 (row stride ld_w1, its first A columns
 * are read), w2 the bf16 (A, H) output kernel, b2 (A,), coef (steps, 3) = [1/sqrt(a_t),
 * (1-a_t)/sqrt(1-abar_t), sqrt(b_t)]. z_in (B, A) injects the initial sample (else drawn from the
 * counter stream keyed by rng and the global sample index); the same z is the noise of every step
 * (the reference never splits its keys, :178). A must be 8 (:200). Writes actions (B, A) fp32
 * and, if z_out is non-NULL, z (B, A). */
int mmt_diffusion_sample(const uint32_t* rng, int B, int A, int steps, int64_t sample_offset,
                         const float* P, int64_t ld_p, const float* Q, int64_t ld_q,
                         const void* w1, int64_t ld_w1, const void* w2, const float* b2,
                         const float* coef, const float* z_in, int H, float* actions,
                         float* z_out, mmt_stream_t stream);
/* The step-table sampler: n_steps affine updates with a clip in one launch, for any action width,
 *   x <- clip(a_k x + b_k eps_hat(x, t_k) + c_k n_k, -clip, +clip),   k = 0 .. n_steps-1,
 *   eps_hat = W2 relu(W1x x + Q[t_k] + P[b]) + b2,
 * which covers DDPM with the reference's frozen noise, DDPM with fresh noise per step and DDIM
 * (eta = 0); the caller builds the table. P, Q (q_rows, H), w1, w2 (A, H) and b2 as for
 * mmt_diffusion_sample. step_t (n_steps) int32 and step_coef (n_steps, 3) = [a, b, c] fp32 live on
 * the device; row k uses Q[step_t[k]]. step_t follows "Device-side index checks": a value outside
 * [0, q_rows) is replaced by 0 and reported as MMT_FAULT_ROW_INDEX, never followed.
 * Noise: x_0 = z = z_in (B, A), or a draw. Without MMT_SAMPLE_FRESH_NOISE n_k = z (the
 * reference's quirk); with it n_k = noise_in[k] ((n_steps, B, A)), or a fresh draw. Draws are
 * Box-Muller on the counter streams: z from key stream_key(seed, step, 0xFFFE, 3), step k's
 * noise from stream_key(seed, step, 0xFFFE - k / 240, 16 + k % 240) (the key keeps 8 bits of
 * its site, so the layer word carries the rest of k: a stream of its own for every k up to 1023,
 * none of them z's or a training stream; for k < 240 this is site 16 + k of layer 0xFFFE), both
 * at counter g A + a with g = sample_offset + b, so a shifted batch reproduces its draws and, at
 * A = 8, z is mmt_diffusion_sample's. z_out (B, A) and noise_out (n_steps, B, A) are optional
 * and return what was used; noise_in / noise_out need the flag.
 * With MMT_SAMPLE_DRAWS_ONLY nothing is sampled: one small launch writes z_out and, with fresh
 * noise, noise_out exactly as the full call would (the per-step launch form of the head takes
 * its draws from it). At least one of the two outputs is needed; only rng, B, A, n_steps,
 * sample_offset, flags, z_in, noise_in and the two outputs are read or checked.
 * Supported: A % 8 == 0, 8 <= A <= 64; H % 8 == 0, H <= 1024; 1 <= n_steps <= 1024; q_rows >= 1;
 * clip > 0; rng or z_in (and, with the flag, rng or noise_in); ld_w1 % 8 == 0, w1 and w2 16-B
 * aligned. Anything else is MMT_ERR_INVALID before a launch. Graph-capturable, allocates nothing,
 * no atomics on the data path (one wave owns a sample): bitwise reproducible run to run.
 * Rounding model: fp32 operands throughout. The bf16 weights are widened exactly; x, the hidden
 * layer and all sums stay fp32 (the per-step launch form rounds x and the hidden layer to bf16).
 * Kernel forms, reported by mmt_sampler_last_route() (MMT_SAMPLER_ROUTE_NONE after a call of
 * either sampler entry rejected before its launch; process-wide, not thread-safe): one wave per
 * sample with W1x and W2 in LDS (_STEPS_LDS, while 4 H AP + 2048 ceil(H / 64) bytes <= 160 KB,
 * AP = A or A + 8 when A / 8 is even), else read from global memory each step (_STEPS_STREAM);
 * _LEGACY_WAVE is mmt_diffusion_sample's register-resident kernel, _STEPS_DRAWS the
 * MMT_SAMPLE_DRAWS_ONLY launch. */
enum { MMT_SAMPLE_FRESH_NOISE = 1, MMT_SAMPLE_DRAWS_ONLY = 2 };
enum {
  MMT_SAMPLER_ROUTE_NONE = 0,
  MMT_SAMPLER_ROUTE_LEGACY_WAVE = 1,
  MMT_SAMPLER_ROUTE_STEPS_LDS = 2,
  MMT_SAMPLER_ROUTE_STEPS_STREAM = 3,
  MMT_SAMPLER_ROUTE_STEPS_DRAWS = 4
};
int mmt_diffusion_sample_steps(const uint32_t* rng, int B, int A, int n_steps,
                               int64_t sample_offset, const float* P, int64_t ld_p, const float* Q,
                               int64_t ld_q, int q_rows, const void* w1, int64_t ld_w1,
                               const void* w2, const float* b2, const int32_t* step_t,
                               const float* step_coef, float clip, int flags, const float* z_in,
                               const float* noise_in, int H, float* actions, float* z_out,
                               float* noise_out, mmt_stream_t stream);
int mmt_sampler_last_route(void);

/* The multi-draw diffusion loss: denoise_loss (diffusion.py:110-143) with K independent (t, eps)
 * draws per sample against one P = readout . W1r^T, and a pad mask over the action components.
 * P, Q (steps, H), w1, w2 (A, H), b2 as for mmt_diffusion_sample_steps. Per sample b and draw k
 *   t = t_in[k, b] or U{0..steps-1};  eps = eps_in[k, b] or N(0, 1) (Box-Muller)
 *   noisy = sqrt(abar_t) a_b + sqrt(1 - abar_t) eps,  abar = alpha_hats (steps)
 *   pre = W1x noisy + Q[t] + P[b];  h = relu(pre);  pred = W2 h + b2;  d = pred - eps
 *   loss  = A / (K max(sum m, 1)) sum_{k,b,j} m[b,j] 0.5 d[k,b,j]^2
 *   dpred = grad_scale A / (K max(sum m, 1)) m d;  dh = (W2^T dpred) [pre > 0];  dP[b] = sum_k dh
 * m = pad_mask (B, A) uint8 (non-zero: the component counts), NULL = all ones, for which the loss
 * is the reference's mean_b sum_j 0.5 d^2 averaged over the draws. sum m is counted on the device
 * by a small launch of this entry; sum m == 0 gives loss 0 and zero gradients.
 * Outputs: loss[0] (overwritten), t_out (K, B) int32, eps_out (K, B, A) fp32 (optional), and the
 * five backward operands, bf16, rows k B + b: noisy (K B, A), h (K B, H), dh (K B, H), dpred
 * (K B, A), and dP (B, H). All five NULL: forward only (evaluation); otherwise all five are given.
 * scratch: B + 1 fp32 words of the caller (the mask count, then the per-sample loss partials).
 * An injected t outside [0, steps) follows "Device-side index checks": replaced by 0 (t_out holds
 * the 0) and reported as MMT_FAULT_ROW_INDEX, never followed.
 * Draws: draw 0 uses mmt_diffusion_prep's keys (t: stream_key(seed, step, 0xFFFE, 1) at counter
 * g = sample_offset + b; eps: site 2 at counter g A + j), so K = 1 reproduces its draws bit for
 * bit. Draw k >= 1 uses layer word 0xFFF9 (no other stream does: 0xFFFA .. 0xFFFE are the head's
 * and the sampler's, 0xFFFF the stem's), site 2 k for t and 2 k + 1 for eps, same counters.
 * The layer words taken, for whoever picks the next: 0xFFF6 mmt_image_augment, 0xFFF7 the
 * point-cloud start (mmt_pc_sample_group), 0xFFF8 mmt_head_categorical_decode, 0xFFF9 this entry,
 * 0xFFFA .. 0xFFFF as above; 0xFFF5 is the next free one.
 * Supported: A % 8 == 0, 8 <= A <= 64; H % 8 == 0, H <= 1024; 1 <= K <= 64; steps >= 1;
 * ld_w1 % 8 == 0, w1 and w2 16-B aligned; rng or both injections. Anything else is
 * MMT_ERR_INVALID before a launch. Graph-capturable, allocates nothing, no float atomics: a wave
 * owns a sample, the per-sample loss partials are added in ascending order by a last small
 * launch, and two calls on the same inputs agree bit for bit.
 * Rounding model: all forward arithmetic is fp32 on exactly widened bf16 weights (as the
 * sampler); the only bf16 roundings are the five backward outputs, dP being accumulated in fp32
 * from the unrounded dh and rounded once.
 * Kernel forms, reported by mmt_diffusion_loss_last_route() (_NONE after a call rejected before
 * its launch; process-wide, not thread-safe): W1x and W2 in LDS (_LDS, while
 * 4 H AP + 2048 ceil(H / 64) bytes <= 160 KB, AP = A or A + 8 when A / 8 is even), else read from
 * global memory each draw (_STREAM). */
enum {
  MMT_DIFFUSION_LOSS_ROUTE_NONE = 0,
  MMT_DIFFUSION_LOSS_ROUTE_LDS = 1,
  MMT_DIFFUSION_LOSS_ROUTE_STREAM = 2
};
int mmt_diffusion_loss_multi(const uint32_t* rng, int B, int A, int K, int steps, int H,
                             int64_t sample_offset, const float* actions, const uint8_t* pad_mask,
                             const float* alpha_hats, const float* P, int64_t ld_p, const float* Q,
                             int64_t ld_q, const void* w1, int64_t ld_w1, const void* w2,
                             const float* b2, const int32_t* t_in, const float* eps_in,
                             float grad_scale, float* scratch, float* loss, int32_t* t_out,
                             float* eps_out, void* noisy, void* h, void* dh, void* dpred, void* dP,
                             mmt_stream_t stream);
int mmt_diffusion_loss_last_route(void);
/* dQ (steps, H) fp32, row stride ld_dq: dQ[t] = sum of the rows r of dh (rows, H) bf16 (row stride
 * ld_dh) with t_rows[r] == t, added in ascending r (one workgroup per (t, 64 columns), no
 * atomics: bitwise reproducible); a t no row has gives a zero row. t_rows is mmt_diffusion_loss_multi's
 * t_out (rows = K B). */
int mmt_diffusion_loss_dq(const int32_t* t_rows, const void* dh, int64_t ld_dh, int rows, int steps,
                          int H, float* dQ, int64_t ld_dq, mmt_stream_t stream);

/* Transposed bf16 weight shadows (this build's layout, no reference twin): for each of n
 * matrices, desc[5i..5i+4] = {src_off, dst_off, rows, cols, first_tile} (elements / 64x64 tiles,
 * first_tile = running tile count), dst[dst_off + c*rows + r] = src[src_off + r*cols + c]. */
int mmt_transpose_bf16_batched(const void* src, void* dst, const int64_t* desc, int n,
                               int64_t total_tiles, mmt_stream_t stream);

/* ------------------------------------------------------------------ continuous / categorical heads
 * (SURVEY §8f row 4). Grouped readout means (categorical.py:32-37): out (B, G, D) bf16 = mean of
 * the rows with row_group[l] == g (counts[g] rows); backward writes the whole fp32 dx (B, L, D). */
int mmt_rows_group_mean_fwd(const void* x, int64_t xs_b, int64_t xs_t, int B, int L, int D,
                            const int32_t* row_group, int G, const int32_t* counts, void* out,
                            mmt_stream_t stream);
int mmt_rows_group_mean_bwd(const void* de, int B, int L, int D, const int32_t* row_group, int G,
                            const int32_t* counts, void* dx, mmt_stream_t stream);
/* kind 0: ContinuousActionHead tanh squash (continuous.py:26) + compute_l2_loss (octo.py:167-174);
 * kind 1: CategoricalActionHead logits + compute_ce_loss with assign_bins (octo.py:187-198,
 * categorical.py:12-22: digitize over `edges`, one_hot(bin, N) zero past the last class).
 * loss (+=, zero it first) = inv_count x sum of the per-row losses; dz bf16 (R, N). y NULL:
 * forward only (kind 0 writes pred). */
int mmt_action_head(int kind, const float* z, int64_t ldz, int R, int N, const float* y,
                    const float* edges, int n_edges, float max_action, float inv_count, float* pred,
                    float* loss, void* dz, mmt_stream_t stream);

/* ---- action chunks, pad mask and decoding (csrc/heads.hip). mmt_action_head above stays the path
 * of one action, no mask, squared error; these three entries take a chunk of h actions per sample,
 * a pad mask and (categorical) the way back from logits to an action. Common contract: one wave
 * per row, four rows per 256-thread workgroup; graph-capturable, allocate nothing, no host
 * synchronisation and no float atomics: every row writes an fp32 loss partial into `scratch`, a
 * first small launch counts the mask's ones with integer adds into scratch[0] (the element count
 * without a mask), and a last one-workgroup launch adds the partials in a fixed order: thread t of
 * 256 adds the partials t, t + 256, t + 512, ... in ascending order, then the 256 sums are folded
 * in halves (s[t] += s[t + 128], then 64, ... 1), and the normalisation is applied from the
 * device-side count. Two calls on the same inputs agree bit for bit. loss[0] is overwritten.
 * scratch: rows + 1 fp32 words of the caller. The normalisation is the diffusion head's masked
 * one (mmt_diffusion_loss_multi): width / max(sum m, 1) times the masked sum, so an all-ones mask
 * reproduces the unmasked mean and an all-zero mask gives loss 0 and zero gradients.
 *
 * mmt_head_continuous: ContinuousActionHead (continuous.py:19-26, the axis `seq` of :24 at its
 * general value h) + compute_l2_loss (octo.py:167-174) with the train step's mean (:262). Rows
 * are the B samples, width W = h A (step-major, component a of step s at s A + a), 1 <= W <= 4096;
 * z fp32 with row stride ldz >= W. p = tanh(z / max_action) max_action, written to pred (B, W)
 * fp32 if non-NULL. With targets y (B, W) fp32 and the optional mask m (B, W) uint8 (non-zero:
 * the component counts; NULL: all ones): e = (p - y)^2 (loss_kind MMT_HEAD_LOSS_MSE) or |p - y|
 * (MMT_HEAD_LOSS_L1, upstream Octo's default regression loss);
 *   loss = A / max(sum m, 1) sum m e   (no mask: the mean over (b, step) of sum_a e)
 *   dz   = A / max(sum m, 1) m e'(p - y) (1 - tanh^2)   bf16 (B, W), e' = 2 d or sign(d), sign(0) = 0
 * y NULL: forward only (pred is required; m, loss, dz, scratch must be NULL or are ignored, a mask
 * without targets is MMT_ERR_INVALID). */
enum { MMT_HEAD_LOSS_MSE = 0, MMT_HEAD_LOSS_L1 = 1 };
int mmt_head_continuous(const float* z, int64_t ldz, int B, int h, int A, const float* y,
                        const uint8_t* mask, int loss_kind, float max_action, float* pred,
                        float* scratch, float* loss, void* dz, mmt_stream_t stream);
/* mmt_head_categorical: CategoricalActionHead logits (categorical.py:25-40, the axis `action` of
 * :32-36 at h A groups) + compute_ce_loss (octo.py:187-198) with the train step's mean (:302).
 * Rows are the R = B h A (sample, step, component) groups, width N = num_bins, 2 <= N <= 1024; z
 * fp32 (R, N) with row stride ldz >= N; y (R,) fp32; the optional row mask m (R,) uint8. Labels as
 * kind 1 of mmt_action_head: bin = #edges <= y (edges (n_edges,) fp32, n_edges = N + 1 of
 * assign_bins, categorical.py:12-22), one_hot(bin, N) all zero for bin >= N (the reference's
 * off-by-one kept: such a row adds 0 to the loss and still counts in the denominator);
 *   loss = sum m ce / max(sum m, 1);   dz = m (has softmax(z) - label) / max(sum m, 1)   bf16 (R, N)
 * cls (R,) int32, optional: the argmax class of every row, the first index on ties (jnp.argmax).
 * y is required (a mask without targets is MMT_ERR_INVALID): the forward alone is the Dense. */
int mmt_head_categorical(const float* z, int64_t ldz, int R, int N, const float* y,
                         const uint8_t* mask, const float* edges, int n_edges, float* scratch,
                         float* loss, void* dz, int32_t* cls, mmt_stream_t stream);
/* mmt_head_categorical_decode: logits back to actions, the inverse of assign_bins that the
 * reference stops short of (octo.py:178-185 ends at the logits). z (R, N) fp32 (row stride ldz),
 * 2 <= N <= 1024; values (N,) fp32, the action each class stands for (action_heads/categorical.py
 * bin_values). Writes cls (R,) int32 and actions (R,) fp32 = values[cls].
 * mode MMT_DECODE_ARGMAX: the largest logit, the first index on ties.
 * mode MMT_DECODE_SAMPLE: one draw per row from softmax(z / temperature), temperature > 0, by
 * inverse CDF: key stream_key(seed, step, 0xFFF8, 1) of rng = {seed, step} (layer word 0xFFF8 is
 * this entry's alone: 0xFFF6, 0xFFF7 and 0xFFF9 .. 0xFFFF are taken, see
 * mmt_diffusion_loss_multi), counter
 * (sample_offset + b) G + g for row r = b G + g (G = h A groups per sample, R % G == 0);
 * u = ((draw_u32 >> 8) + 0.5) / 2^24 in fp32 (the sum is exact below 2^23 and rounds to even
 * above, so u lies in (0, 1]; oracle/rng.py restates the draw bit for bit); the class is the
 * smallest c with CDF(c) > u, N - 1 if there is none. The prefix sum stays in the wave: lane l
 * holds the contiguous classes [l n, (l + 1) n), n = ceil(N / 64), adds their exp((z - max) /
 * temperature) in ascending order, an exclusive scan over the lanes gives each run's start, and
 * CDF(c) > u is tested as prefix(c) > u total (no division). rng may be NULL in argmax mode. */
enum { MMT_DECODE_ARGMAX = 0, MMT_DECODE_SAMPLE = 1 };
int mmt_head_categorical_decode(const float* z, int64_t ldz, int R, int N, int G,
                                const float* values, int mode, float temperature,
                                const uint32_t* rng, int64_t sample_offset, int32_t* cls,
                                float* actions, mmt_stream_t stream);

/* ------------------------------------------------------------------ T5 encoder pieces
 * (tokenizers/text/t5_base.py:8-15, frozen FlaxT5 encoder): T5LayerNorm and the shared
 * embedding lookup. bf16 rows of D elements, D > 0, D % 8 == 0, moved as 16-B vectors: x, w, y
 * (table, out) have 16-B aligned bases. The gather clamps ids to [0, vocab - 1] (id < 0 reads
 * row 0, id >= vocab reads row vocab - 1), as jnp.take does in the reference. */
int mmt_rmsnorm_fwd(const void* x, int64_t rows, int D, const void* w, float eps, void* y,
                    mmt_stream_t stream);
int mmt_embedding_gather(const int32_t* ids, int64_t n, int D, const void* table, int vocab,
                         void* out, mmt_stream_t stream);

/* ------------------------------------------------------------------ optimizer / state
 * Fused AdamW over the flat fp32 parameter buffer (the reference takes an optax tx from the
 * caller, octo.py:228,341; this is optax.adamw semantics), writing the bf16 shadow copy.
 * state = device {seed, step}: step+1 is the bias-correction count; mmt_step_advance
 * increments it (keys every random stream of the next step). Hyper-parameters in double (the
 * caller's Python floats): 1 - beta and the bias corrections are formed in double. */
int mmt_adamw(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n,
              const int32_t* state, double lr, double b1, double b2, double eps, double wd,
              float grad_scale, mmt_stream_t stream);
int mmt_cast_f32_bf16(const float* a, void* b, int64_t n, mmt_stream_t stream);
int mmt_step_advance(int32_t* state, mmt_stream_t stream);

/* Device-resident optimizer control: the learning rate of a schedule, the global gradient norm
 * and the clip factor are computed on the device and read by AdamW from device memory, so one
 * captured graph serves a whole run (optax.chain(clip_by_global_norm(max_norm),
 * adamw(schedule)); the reference takes any optax tx from its caller, octo.py:341,377).
 *
 * Schedules of s = state[1] (the count BEFORE this step's advance, as optax scale_by_schedule),
 * W = warmup_steps, T = decay_steps, evaluated in double and rounded to fp32 once:
 *   CONSTANT       peak_value
 *   WARMUP_COSINE  optax.warmup_cosine_decay_schedule: s < W: init + (peak - init) s / W; else
 *                  c = min(s - W, T - W), a = end / peak:
 *                  peak ((1 - a) (1 + cos(pi c / (T - W))) / 2 + a)
 *   WARMUP_RSQRT   the same warm-up; s >= W: peak sqrt(timescale / (s - W + timescale))
 *
 * opt: 8 caller-owned fp32 words on the device, written by mmt_optim_prepare:
 *   0 grad_norm  grad_scale * sqrt(sum g^2): the norm of the averaged gradient before clipping
 *   1 clip       max_norm > 0: 1 if grad_norm < max_norm else max_norm / grad_norm
 *                (optax.clip_by_global_norm, no epsilon); max_norm <= 0: always 1
 *   2 gmul       grad_scale * clip, formed in double, rounded once: the only factor the update
 *                applies to g[i]
 *   3 lr         schedule(state[1])
 *   4 nonfinite  1 if sum g^2 is not finite, else 0
 *   5 skipped    running count of skipped steps (accumulated; every other word is overwritten)
 *   6 skip       nonfinite && skip_nonfinite
 *   7 0
 *
 * mmt_optim_prepare is two launches, no atomics, no host sync, graph-capturable:
 *   1. MMT_GRAD_NORM_GRID workgroups of 256 lanes (a constant: not a function of the device);
 *      workgroup b owns the 16-B vectors [b * per, (b + 1) * per) of g, per = ceil((n / 4) /
 *      MMT_GRAD_NORM_GRID), clipped to n / 4; the n % 4 tail elements go to the last workgroup.
 *      Every workgroup stores one fp32 partial (0 for an empty chunk) into workspace, which
 *      need not be zeroed.
 *   2. one workgroup adds the partials in double in a fixed order and writes opt.
 * The partition and both trees are fixed, so opt is bitwise reproducible from run to run.
 * Longest chain of fp32 roundings on any path to sum g^2 (each g^2 enters by one fused
 * multiply-add): ceil(per / 1024) + 1 (tail) + 4 (a lane's 16 accumulators) + 6 (wave64
 * tree) + 2 (4 waves) = ceil(per / 1024) + 13; 24 at 90 M elements.
 * g: 16-B aligned. workspace: >= mmt_workspace_size(MMT_WS_GRAD_NORM, {n}) bytes. sched is read
 * on the host at launch.
 *
 * mmt_adamw_dev is mmt_adamw with lr = opt[3] and grad_scale = opt[2] (the same update
 * function: bit-identical to mmt_adamw given the same fp32 values); when opt[6] != 0 it
 * returns at once and p, m, v and the shadow are not touched. */
enum { MMT_SCHED_CONSTANT = 0, MMT_SCHED_WARMUP_COSINE = 1, MMT_SCHED_WARMUP_RSQRT = 2 };
typedef struct {            /* zero-initialise, then set; read on the host at launch */
  int kind;
  double init_value, peak_value, end_value;   /* CONSTANT uses peak_value */
  int64_t warmup_steps, decay_steps;          /* decay_steps: COSINE only (total, warm-up included) */
  double timescale;                           /* RSQRT only */
} mmt_lr_schedule_t;
#define MMT_GRAD_NORM_GRID 2048

int mmt_optim_prepare(const float* g, int64_t n, float grad_scale, double max_norm,
                      int skip_nonfinite, const mmt_lr_schedule_t* sched, const int32_t* state,
                      float* opt, void* workspace, int64_t ws_bytes, mmt_stream_t stream);
int mmt_adamw_dev(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n,
                  const int32_t* state, const float* opt, double b1, double b2, double eps,
                  double wd, mmt_stream_t stream);

/* Parameter groups: optax.multi_transform({"trainable": optax.chain(clip_by_global_norm,
 * adamw(schedule, mask = decay_mask)), "frozen": set_to_zero()}) over the same flat buffer.
 *
 * chunk_flags: one byte per MMT_GROUP_CHUNK = 64 consecutive elements of the flat buffer,
 * ceil(n / 64) bytes on the device, bit 0 (MMT_GROUP_NO_DECAY) = the chunk takes no weight
 * decay, bit 1 (MMT_GROUP_FROZEN) = the chunk is never updated; the other bits are ignored.
 * The caller aligns every parameter to 64 elements, so a chunk never straddles two parameters
 * and a 16-B vector never straddles two chunks. `chunk` must be MMT_GROUP_CHUNK and chunk_flags
 * non-null: anything else returns MMT_ERR_INVALID before a launch.
 *
 * mmt_adamw_groups covers both forms above: opt == NULL takes lr and grad_scale from the host
 * arguments (mmt_adamw); opt != NULL reads lr = opt[3], the gradient factor opt[2] and the skip
 * flag opt[6] (mmt_adamw_dev; lr and grad_scale are ignored, opt[6] != 0 returns at once and
 * nothing is touched). It has the geometry of the plain kernels (a wave covers one chunk per
 * iteration) and calls the same per-element update function, so
 *   - a chunk with no bit set is bit-identical to mmt_adamw / mmt_adamw_dev on the same values;
 *   - a NO_DECAY chunk is bit-identical to the plain kernel called with wd = 0;
 *   - a FROZEN chunk issues no load or store of p, g, m, v or the shadow: those bytes stay as
 *     they are whatever g holds there (NaN and Inf included).
 *
 * mmt_optim_prepare_groups is mmt_optim_prepare over the trainable chunks: the same two
 * launches, the same partition (workgroup b owns the same 16-B vectors of g), the same
 * accumulators and trees. A vector of a FROZEN chunk is not loaded and enters as zeros, so it
 * contributes nothing to sum g^2 (opt[0] is the norm of the trainable gradient) nor to the
 * non-finite flag; every workgroup still stores its partial, 0 for an empty or all-frozen
 * range. With no FROZEN bit set the eight opt words are bit-identical to mmt_optim_prepare's.
 * Skipped vectors only shorten a chain, so the bound ceil(per / 1024) + 13 holds, and the
 * result is bitwise reproducible. All chunks frozen: sum g^2 = 0, grad_norm 0, clip 1,
 * gmul = grad_scale (no division takes place). NO_DECAY does not matter here. */
#define MMT_GROUP_CHUNK 64
#define MMT_GROUP_CHUNK_SHIFT 6
#define MMT_GROUP_NO_DECAY 1
#define MMT_GROUP_FROZEN 2
int mmt_adamw_groups(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n,
                     const int32_t* state, const float* opt, double lr, double b1, double b2,
                     double eps, double wd, float grad_scale, const uint8_t* chunk_flags,
                     int chunk, mmt_stream_t stream);
int mmt_optim_prepare_groups(const float* g, int64_t n, float grad_scale, double max_norm,
                             int skip_nonfinite, const mmt_lr_schedule_t* sched,
                             const int32_t* state, float* opt, void* workspace,
                             int64_t ws_bytes, const uint8_t* chunk_flags, int chunk,
                             mmt_stream_t stream);

/* Parameter EMA: the exponential moving average of the weights that diffusion recipes evaluate
 * (DDPM, Diffusion Policy, diffusers EMAModel; optax.ema(decay, debias = False) over the
 * parameters), kept in a second flat fp32 buffer `ema` of n elements and updated inside the AdamW
 * launch, where the new parameter is in a register:
 *   ema[i] = d_f * ema[i] + omd_f * p_new[i]
 * (one product, one fused multiply-add: two fp32 roundings).
 *
 * Decay of s = state[1] (the count BEFORE this step's advance, as the schedules above):
 *   MMT_EMA_CONSTANT  d = value
 *   MMT_EMA_WARMUP    the diffusers / Diffusion-Policy EMAModel rule:
 *                     k = max(0, s - update_after_step - 1); d = 0 if k == 0, else
 *                     min(max_value, max(min_value, 1 - (1 + k / inv_gamma)^(-power)))
 * d and 1 - d are formed in double on the device and each rounded once to fp32 (d_f, omd_f), as
 * the betas are: one captured graph serves the whole warm-up. d = 0 makes ema a copy of p_new.
 *
 * mmt_adamw_ema covers the three AdamW forms and takes every argument of theirs:
 *   opt == NULL, chunk_flags == NULL   mmt_adamw (lr, grad_scale from the host arguments)
 *   opt != NULL, chunk_flags == NULL   mmt_adamw_dev (lr, grad_scale ignored)
 *   chunk_flags != NULL                mmt_adamw_groups (either opt form; chunk must be
 *                                      MMT_GROUP_CHUNK)
 * It has the launch geometry of the kernel it replaces and calls the same per-element update
 * function, so p, m, v and the shadow are bit-identical to that kernel's on the same inputs. A
 * FROZEN chunk issues no load or store of ema either (a caller that initialises ema as a copy of
 * p keeps ema == p there). opt[6] != 0 (a skipped step) returns at once: ema is not touched, so
 * a skipped step does not enter the average, though it advances s. The opt words are only read.
 *
 * mmt_ema_swap exchanges p[i] and ema[i] and writes shadow[i] = bf16(new p[i]) in one pass
 * (shadow_bf16 may be NULL), for evaluating with the averaged weights in place: no buffer moves,
 * so captured graphs stay valid. chunk_flags may be NULL; FROZEN chunks are not touched. Applied
 * twice it is the identity, bit for bit.
 *
 * MMT_ERR_INVALID before any launch: a null p, g, m, v, state, ema or decay; n <= 0; chunk_flags
 * given with chunk != MMT_GROUP_CHUNK; an unknown kind; value, max_value or min_value outside
 * [0, 1]; for MMT_EMA_WARMUP also min_value > max_value, inv_gamma <= 0, power < 0,
 * update_after_step < 0. */
enum { MMT_EMA_CONSTANT = 0, MMT_EMA_WARMUP = 1 };
typedef struct {            /* zero-initialise, then set; read on the host at launch */
  int kind;
  double value;                               /* CONSTANT only */
  double max_value, min_value;                /* WARMUP only, as the fields below */
  double inv_gamma, power;
  int64_t update_after_step;
} mmt_ema_decay_t;
int mmt_adamw_ema(float* p, const float* g, float* m, float* v, void* shadow_bf16, float* ema,
                  int64_t n, const int32_t* state, const float* opt, double lr, double b1,
                  double b2, double eps, double wd, float grad_scale, const uint8_t* chunk_flags,
                  int chunk, const mmt_ema_decay_t* decay, mmt_stream_t stream);
int mmt_ema_swap(float* p, float* ema, void* shadow_bf16, int64_t n, const uint8_t* chunk_flags,
                 int chunk, mmt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMT_API_H */
