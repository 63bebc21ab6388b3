"""ctypes binding of libmmt_hip.so (the C ABI declared in include/mmt_api.h).

There is deliberately no CPU or PyTorch fallback: if the library is missing every op raises.
Build it with ``python -m multi_modal_transformers_tokenmerge_amd.csrc.build`` (or
``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
from pathlib import Path

_LIB_PATH = Path(__file__).resolve().parent / "libmmt_hip.so"
_lib = None

P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
U32, U64, Z = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
D = ctypes.c_double

class Epilogue(ctypes.Structure):
    """mmt_epilogue_t (include/mmt_api.h)."""
    _fields_ = [("bias", P), ("act", I), ("rng", P), ("drop_layer", U32), ("drop_site", U32),
                ("keep_prob", F), ("drop_row_offset", L), ("gate", P), ("ld_gate", L),
                ("gate_scale", F), ("residual", P), ("ld_res", L), ("alpha", F), ("beta", F),
                ("res_dtype", I), ("colsum", P), ("relu_bits", P), ("gate_bits", P),
                ("keep_bits", P)]


# name -> argtypes (every entry point returns int status unless listed in _VOID)
SIGNATURES: dict[str, list] = {
    "mmt_version": [],
    "mmt_device_status": [P],
    "mmt_tome_set_match_path": [I],
    "mmt_workspace_size": [I, P, I],
    "mmt_tome_match": [P, I, I, I, I, I, L, L, L, I, I, P, P, P, P, P, L, P],
    "mmt_tome_merge_wavg_fwd": [P, I, I, I, I, L, L, I, I, I, I, P, P, P, P, P, L, L, P, P, P],
    "mmt_tome_merge_wavg_bwd": [P, I, I, I, I, L, L, I, I, I, P, P, P, P, L, L, P],
    "mmt_seqnorm_dropout_bwd": [P, L, L, P, L, L, I, I, I, P, P, P, P, L, L, P, L, L, P, P, P, U32,
                                U32, F, L, P, L, L, P, P],
    "mmt_ln_unmerge_dropout_bwd": [P, L, L, P, L, L, I, I, I, P, P, P, P, L, L, P, P, I, I, I, I, P,
                                   P, P, P, L, L, P, U32, U32, F, L, P, L, L, P, P],
    "mmt_tome_merge_seqnorm_fwd": [P, I, I, I, L, L, I, I, I, I, P, P, P, P, P, L, L, P, P, P, P, F,
                                   P, L, L, P, P, P],
    "mmt_topk_gather": [P, I, I, I, I, L, L, P, L, I, P, P, P, P, L, L, P, P],
    "mmt_topk_scatter_bwd": [P, I, I, I, I, L, L, P, I, P, L, L, P],
    "mmt_gemm_set_variant": [I],
    "mmt_gemm_last_route": [],
    "mmt_attn_last_route": [],
    "mmt_norm_last_route": [],
    "mmt_stem_last_route": [],
    "mmt_tome_last_route": [],
    "mmt_set_deterministic": [P, P, L],
    "mmt_det_flush": [P, P, L, P],
    "mmt_gemm_colsum_rows": [I, I, I, I, I, I, I],
    "mmt_gemm_dropout_keep_bits": [P, U32, U32, I, I, F, L, P, P],
    "mmt_gemm": [I, I, I, P, I, L, P, I, L, P, I, L, I, L, L, L, I, P, P, L, P],
    "mmt_quant_rows_fp8": [P, L, I, I, P, L, P, P],
    "mmt_gemm_fp8": [I, I, I, P, L, P, P, L, P, P, I, L, P, P],
    "mmt_gemm_xs": [I, I, I, P, L, P, L, P, L, P, P],
    "mmt_attn_fwd": [P, L, L, I, I, I, I, F, I, P, P, P, P, F, P, P, L, L, P, P, P],
    "mmt_prune_importance": [P, I, I, I, P, P],
    "mmt_gather_rows": [P, I, I, I, I, L, L, P, I, P, L, L, P],
    "mmt_maxpool2d": [P, L, I, I, I, I, P, P, P],
    "mmt_maxpool2d_bwd": [P, P, L, I, I, I, I, P, P],
    "mmt_im2col_same": [P, L, I, I, I, I, P, P],
    "mmt_col2im_same": [P, L, I, I, I, I, P, P],
    "mmt_attn_bwd": [P, L, L, I, I, I, I, F, I, P, P, P, P, P, F, P, L, L, P, L, L, P, P, P, L, L, P, P],
    "mmt_attn_fwd_keybias": [P, L, L, I, I, I, I, F, I, P, P, P, P, F, P, P, L, L, P, P, P, L, P],
    "mmt_attn_bwd_keybias": [P, L, L, I, I, I, I, F, I, P, P, P, P, P, F, P, L, L, P, L, L, P, P, P,
                             L, L, P, P, L, P],
    "mmt_tome_size_bias": [P, I, I, I, I, P, L, I, P],
    "mmt_pad_mask_pack": [P, I, I, U32, P, P],
    "mmt_pad_mask_pack_counts": [P, I, I, U32, P, I, P, P, P, P],
    "mmt_pad_mask_images": [P, P, I, I, I, L, P, P, P],
    "mmt_pad_mask_bias": [P, I, I, I, P, P, P, I, I, P, L, I, P],
    "mmt_pad_mask_rows_fwd": [P, I, I, I, I, P, P, P, I, I, P, P, L, L, P],
    "mmt_pad_mask_rows_bwd": [P, I, I, I, I, P, P, P, I, I, P, L, L, P],
    "mmt_tome_pos_map": [P, P, P, I, I, I, I, P, P],
    "mmt_tome_source_step": [P, I, I, I, P, I, I, P],
    "mmt_tome_source_groups": [P, I, I, I, P, P, P],
    "mmt_tome_unmerge_fwd": [P, I, I, I, I, L, L, I, I, P, I, P, L, L, P],
    "mmt_tome_unmerge_bwd": [P, I, I, I, I, L, L, I, I, P, P, I, P, L, L, P],
    "mmt_dropout_bits": [P, U32, U32, I, I, F, P, P, P],
    "mmt_seqnorm_fwd": [P, I, L, L, I, I, I, P, P, F, P, L, L, P, P, P],
    "mmt_seqnorm_bwd": [P, I, L, L, P, I, L, L, I, I, I, P, P, P, P, L, L, P, L, L, P, P, P],
    "mmt_colsum": [P, I, L, I, I, P, P],
    "mmt_dropout_bwd": [P, I, L, I, I, P, U32, U32, F, L, P, L, P, P],
    "mmt_patch_im2col": [P, I, I, I, I, I, I, I, I, I, I, P, P],
    "mmt_maxpool_patch": [P, L, I, I, P, P, P],
    "mmt_maxpool_patch_bwd": [P, P, L, I, I, P, P],
    "mmt_groupnorm_gelu_fwd": [P, I, I, I, I, F, P, P, P, P, P, P],
    "mmt_groupnorm_gelu_bwd": [P, P, I, I, I, I, P, P, P, P, P, I, P, P, P],
    "mmt_patch_positions": [P, U32, I, I, I, I, I, I, L, P, P, P],
    "mmt_seq_assemble_fwd": [I, I, I, P, P, I, P, I, P, P, P, P, P, P, P, P],
    "mmt_seq_assemble_bwd": [I, I, I, P, P, P, I, P, I, P, P, P, I, P, P, P, P],
    "mmt_value_tokens_fwd": [P, L, I, I, I, F, I, P, P, P, I, P, L, L, P, P],
    "mmt_value_tokens_bwd": [P, L, L, I, I, P, P, I, I, P, P],
    "mmt_pc_sample_group": [P, L, L, I, I, I, I, I, I, P, P, L, P, P, P],
    "mmt_pc_sample_group_counts": [P, L, L, I, I, I, I, I, I, P, P, L, P, P, P, P],
    "mmt_depth_unproject": [P, I, I, I, I, I, P, P, P, F, F, F, I, P, P, P],
    "mmt_image_augment_workspace": [I, I],
    "mmt_image_augment": [P, I, I, I, I, P, L, P, P, I, P, P, P, L, P],
    "mmt_pc_embed_fwd": [P, L, L, I, I, I, I, I, I, P, P, I, I, P, P, P, P, P, P, P, P, I, P, L, L, P,
                         P],
    "mmt_pc_embed_bwd_workspace": [I, I, I, I, I, I, I],
    "mmt_pc_embed_bwd": [P, L, L, P, I, P, L, L, I, I, I, I, I, I, P, P, P, I, I, P, P, P, P, P, P, P,
                         P, P, P, P, P, L, P],
    "mmt_qk_norm_fwd": [P, I, L, L, I, I, P, P, F, P, P],
    "mmt_qk_norm_bwd_workspace": [L, I, I],
    "mmt_qk_norm_bwd": [P, I, L, L, I, I, P, P, P, F, P, P, P, L, P],
    "mmt_patch_embed_grad": [I, I, I, I, I, I, I, P, P, P, P, P, P, P],
    "mmt_stem_conv_pool": [P, I, I, I, P, P, P, P, P],
    "mmt_stem_conv_wgrad_slabs": [I, I, I],
    "mmt_stem_conv_wgrad": [P, I, I, I, P, P, P, L, P],
    "mmt_add_position_embedding": [P, P, P, I, I, I, P],
    "mmt_rows_mean_fwd": [P, L, L, I, I, P, I, P, L, P],
    "mmt_rows_mean_bwd": [P, L, I, I, I, P, I, P, P],
    "mmt_rows_gather_bf16": [P, L, L, I, I, I, P, I, P, P],
    "mmt_rows_scatter_bwd": [P, I, I, I, P, I, P, P],
    "mmt_attn_pool_fwd": [P, P, P, L, I, I, I, I, P, L, P, P],
    "mmt_attn_pool_bwd": [P, L, P, P, P, P, L, I, I, I, I, P, P, L, P, P],
    "mmt_layernorm_fwd": [P, I, L, I, I, P, P, F, P, L, P, P, P],
    "mmt_layernorm_bwd": [P, I, L, P, I, L, I, I, P, P, P, P, L, P, L, P, P],
    "mmt_diffusion_prep": [P, I, I, I, L, P, P, P, I, P, P, P, P, P, L, P, P],
    "mmt_fourier_bwd": [P, I, I, P, P, P, P],
    "mmt_diffusion_loss": [P, L, P, I, I, F, P, P, P],
    "mmt_diffusion_sample": [P, I, I, I, L, P, L, P, L, P, L, P, P, P, P, I, P, P, P],
    "mmt_diffusion_sample_steps": [P, I, I, I, L, P, L, P, L, I, P, L, P, P, P, P, F, I, P, P, I, P,
                                   P, P, P],
    "mmt_sampler_last_route": [],
    "mmt_diffusion_loss_multi": [P, I, I, I, I, I, L, P, P, P, P, L, P, L, P, L, P, P, P, P, F, P, P,
                                 P, P, P, P, P, P, P, P],
    "mmt_diffusion_loss_last_route": [],
    "mmt_diffusion_loss_dq": [P, P, L, I, I, I, P, L, P],
    "mmt_rows_group_mean_fwd": [P, L, L, I, I, I, P, I, P, P, P],
    "mmt_rows_group_mean_bwd": [P, I, I, I, P, I, P, P, P],
    "mmt_action_head": [I, P, L, I, I, P, P, I, F, F, P, P, P, P],
    "mmt_head_continuous": [P, L, I, I, I, P, P, I, F, P, P, P, P, P],
    "mmt_head_categorical": [P, L, I, I, P, P, P, I, P, P, P, P, P],
    "mmt_head_categorical_decode": [P, L, I, I, I, P, I, F, P, L, P, P, P],
    "mmt_rmsnorm_fwd": [P, L, I, P, F, P, P],
    "mmt_embedding_gather": [P, L, I, P, I, P, P],
    "mmt_adamw": [P, P, P, P, P, L, P, D, D, D, D, D, F, P],
    "mmt_cast_f32_bf16": [P, P, L, P],
    "mmt_transpose_bf16_batched": [P, P, P, I, L, P],
    "mmt_step_advance": [P, P],
    "mmt_optim_prepare": [P, L, F, D, I, P, P, P, P, L, P],
    "mmt_adamw_dev": [P, P, P, P, P, L, P, P, D, D, D, D, P],
    "mmt_adamw_groups": [P, P, P, P, P, L, P, P, D, D, D, D, D, F, P, I, P],
    "mmt_optim_prepare_groups": [P, L, F, D, I, P, P, P, P, L, P, I, P],
    "mmt_adamw_ema": [P, P, P, P, P, P, L, P, P, D, D, D, D, D, F, P, I, P, P],
    "mmt_ema_swap": [P, P, P, L, P, I, P],
}
_VOID = {"mmt_tome_set_match_path", "mmt_gemm_set_variant"}
_RESTYPE = {"mmt_workspace_size": L,      # returns a byte count (negative: error)
            "mmt_pc_embed_bwd_workspace": L,  # returns a byte count (negative: error)
            "mmt_qk_norm_bwd_workspace": L,   # returns a byte count (negative: error)
            "mmt_image_augment_workspace": L,  # returns a byte count (negative: error)
            "mmt_gemm_colsum_rows": I,    # returns a row count
            "mmt_gemm_last_route": I,     # returns a ROUTE_* value
            "mmt_attn_last_route": I,     # returns an ATTN_ROUTE_* value
            "mmt_norm_last_route": I,     # returns a NORM_ROUTE_* value
            "mmt_stem_last_route": I,     # returns a STEM_ROUTE_* value
            "mmt_tome_last_route": I,     # returns a TOME_ROUTE_* value
            "mmt_sampler_last_route": I,  # returns a SAMPLER_ROUTE_* value
            "mmt_diffusion_loss_last_route": I,  # returns a DIFFUSION_LOSS_ROUTE_* value
            "mmt_stem_conv_wgrad_slabs": I}


API_VERSION = 2  # include/mmt_api.h MMT_API_VERSION


class MMTError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise ImportError(f"{_LIB_PATH} is missing: build it with "
                              "`python -m multi_modal_transformers_tokenmerge_amd.csrc.build` "
                              "(no CPU fallback exists by design)")
        import os
        import sys
        path = str(_LIB_PATH)
        ab = os.environ.get("MMT_LIB_AB")
        if ab:  # benchmarking knob: A/B a second build of the same C ABI from inside the build tree
            p = Path(ab).resolve()
            root = _LIB_PATH.resolve().parent.parent
            if root not in p.parents or p.suffix != ".so":
                raise ImportError(f"MMT_LIB_AB={ab!r}: only a .so inside {root} may replace "
                                  f"{_LIB_PATH.name}")
            print(f"[mmt] MMT_LIB_AB: loading {p} instead of {_LIB_PATH}", file=sys.stderr)
            path = str(p)
        h = ctypes.CDLL(path)
        h.mmt_last_error.restype = ctypes.c_char_p
        h.mmt_last_error.argtypes = []
        for name, args in SIGNATURES.items():
            fn = getattr(h, name)
            fn.argtypes = args
            fn.restype = None if name in _VOID else _RESTYPE.get(name, I)
        if h.mmt_version() != API_VERSION:  # the Epilogue layout above is version 2's
            raise ImportError(f"{path}: C ABI version {h.mmt_version()}, this binding needs "
                              f"{API_VERSION} (include/mmt_api.h MMT_API_VERSION): rebuild it")
        _lib = h
        if os.environ.get("MMT_GEMM_VARIANT"):  # benchmarking knob (include/mmt_api.h)
            h.mmt_gemm_set_variant(int(os.environ["MMT_GEMM_VARIANT"]))
    return _lib


def call(name: str, *args) -> int:
    rc = getattr(lib(), name)(*args)
    if name in _VOID:
        return 0
    if name in _RESTYPE:
        if rc < 0:
            raise MMTError(f"{name} failed ({rc}): {lib().mmt_last_error().decode(errors='replace')}")
        return rc
    if rc != 0:
        msg = lib().mmt_last_error().decode(errors="replace")
        raise MMTError(f"{name} failed ({rc}): {msg}")
    return rc


def exported_symbols() -> list[str]:
    return ["mmt_last_error", *SIGNATURES.keys()]


WS_TOME_MATCH, WS_GRAD_NORM = 1, 2  # mmt_workspace_size op codes (include/mmt_api.h)
# MMT_GRAD_NORM_GRID: workgroups of mmt_optim_prepare's partial-sum launch (GRAD_NORM_GRID * 256
# lanes * 4 elements = one full 16-B pass of the grid); OPT_WORDS: the fp32 words of `opt`
GRAD_NORM_GRID = 2048
OPT_WORDS = 8
OPT_GRAD_NORM, OPT_CLIP, OPT_GMUL, OPT_LR, OPT_NONFINITE, OPT_SKIPPED, OPT_SKIP = range(7)


# MMT_GEMM_ROUTE_* (include/mmt_api.h): what mmt_gemm_last_route() reports
(ROUTE_NONE, ROUTE_GENERIC_P0, ROUTE_GENERIC_P1, ROUTE_GENERIC_P1_BK128, ROUTE_BIG, ROUTE_GLDS_NT,
 ROUTE_NT256_256, ROUTE_NT256_192, ROUTE_NT256_128, ROUTE_NTW, ROUTE_NTWS, ROUTE_XS,
 ROUTE_TN_DMA_256, ROUTE_TN_DMA_384, ROUTE_TN_DMA16_256, ROUTE_TN_DMA16_384, ROUTE_TN_R4_384,
 ROUTE_FP8_NT, ROUTE_XS_FP8) = range(19)
ROUTE_KERNEL_MASK, ROUTE_COMBINE = 0xff, 0x10000


def route_ntw(bn: int, mt: int) -> int:
    """The route of gemm_ntw_kernel with bn-wide tiles whose last launch used mt-row tiles."""
    return ROUTE_NTW | (bn // 64) << 8 | (mt // 64) << 12


def last_route() -> int:
    return call("mmt_gemm_last_route")


# MMT_ATTN_ROUTE_* (include/mmt_api.h): what mmt_attn_last_route() reports
(ATTN_ROUTE_NONE, ATTN_ROUTE_FWD_TILED_1W, ATTN_ROUTE_FWD_TILED_4W, ATTN_ROUTE_FWD_RES_ONEPASS,
 ATTN_ROUTE_FWD_RES_TWOPASS, ATTN_ROUTE_BWD_TILED, ATTN_ROUTE_BWD_RES, ATTN_ROUTE_BWD_RES8) = range(8)
ATTN_ROUTE_KERNEL_MASK, ATTN_ROUTE_WORKLIST = 0xff, 0x10000


def attn_route(kernel: int, param: int, dh: int = 0, worklist: bool = False) -> int:
    """The route of `kernel` with MMT_ATTN_ROUTE_PARAM `param` (the tiled forward's NQ, a resident
    kernel's NTILE, the tiled backward's waves per workgroup) and, for the tiled kernels, Dh."""
    return kernel | param << 8 | (dh // 64) << 12 | (ATTN_ROUTE_WORKLIST if worklist else 0)


def attn_last_route() -> int:
    return call("mmt_attn_last_route")


# MMT_NORM_ROUTE_* (include/mmt_api.h): what mmt_norm_last_route() reports
(NORM_ROUTE_NONE, NORM_ROUTE_SEQ_FWD, NORM_ROUTE_SEQ_BWD, NORM_ROUTE_SEQ_DROPOUT_BWD,
 NORM_ROUTE_LN_UNMERGE_BWD, NORM_ROUTE_MERGE_SEQ_FWD) = range(6)
NORM_ROUTE_ENTRY_MASK, NORM_ROUTE_X_BF16, NORM_ROUTE_DY_BF16 = 0xff, 0x10000, 0x20000


def norm_route(entry: int, rpt: int, x_bf16: bool = False, dy_bf16: bool = False) -> int:
    """The route of `entry` in the form with `rpt` rows per thread (MMT_NORM_ROUTE_RPT; 0: the
    two-pass form) and the operand types."""
    return (entry | rpt << 8 | (NORM_ROUTE_X_BF16 if x_bf16 else 0)
            | (NORM_ROUTE_DY_BF16 if dy_bf16 else 0))


def norm_last_route() -> int:
    return call("mmt_norm_last_route")


# MMT_STEM_ROUTE_* (include/mmt_api.h): what mmt_stem_last_route() reports
(STEM_ROUTE_NONE, STEM_ROUTE_PATCH_IM2COL, STEM_ROUTE_CONV_POOL, STEM_ROUTE_CONV_WGRAD,
 STEM_ROUTE_MAXPOOL_PATCH, STEM_ROUTE_MAXPOOL_PATCH_BWD, STEM_ROUTE_GN_GELU_FWD,
 STEM_ROUTE_GN_GELU_BWD, STEM_ROUTE_PATCH_POSITIONS, STEM_ROUTE_MAXPOOL2D, STEM_ROUTE_MAXPOOL2D_BWD,
 STEM_ROUTE_IM2COL_SAME, STEM_ROUTE_COL2IM_SAME) = range(13)
STEM_ROUTE_ENTRY_MASK, STEM_ROUTE_IN_U8 = 0xff, 0x10000
STEM_IM2COL_GENERIC, STEM_IM2COL_ROWS, STEM_IM2COL_LDS = range(3)   # forms of mmt_patch_im2col


def stem_route(entry: int, form: int = 0, in_u8: bool = False) -> int:
    """The route of `entry` in `form` (MMT_STEM_ROUTE_FORM: a STEM_IM2COL_* value for
    mmt_patch_im2col, the register kernel's NV or 0 for the GroupNorm entries) and, for
    mmt_patch_im2col, whether the pixels were uint8."""
    return entry | form << 8 | (STEM_ROUTE_IN_U8 if in_u8 else 0)


def stem_last_route() -> int:
    return call("mmt_stem_last_route")


# MMT_TOME_ROUTE_* (include/mmt_api.h): what mmt_tome_last_route() reports
(TOME_ROUTE_NONE, TOME_ROUTE_FUSED, TOME_ROUTE_BIG_AG1, TOME_ROUTE_BIG_AG2, TOME_ROUTE_TILED_MFMA,
 TOME_ROUTE_TILED_VALU) = range(6)
TOME_ROUTE_FORM_MASK, TOME_ROUTE_NORM_SCALAR, TOME_ROUTE_IN_BF16 = 0xff, 0x10000, 0x20000


def tome_route(form: int, lpr: int = 0, nbt: int = 0, in_bf16: bool = False) -> int:
    """The route of the mmt_tome_match chain `form` with `lpr` lanes per token row in the vector
    norm / fused kernel (MMT_TOME_ROUTE_LPR; 0: the scalar norm), `nbt` b tiles per LDS group of
    the tiled forms (MMT_TOME_ROUTE_NBT; 0 otherwise) and the metric's type."""
    return (form | lpr << 8 | nbt << 20 | (0 if lpr else TOME_ROUTE_NORM_SCALAR)
            | (TOME_ROUTE_IN_BF16 if in_bf16 else 0))


def tome_last_route() -> int:
    return call("mmt_tome_last_route")


# MMT_SAMPLER_ROUTE_* (include/mmt_api.h): what mmt_sampler_last_route() reports
(SAMPLER_ROUTE_NONE, SAMPLER_ROUTE_LEGACY_WAVE, SAMPLER_ROUTE_STEPS_LDS,
 SAMPLER_ROUTE_STEPS_STREAM, SAMPLER_ROUTE_STEPS_DRAWS) = range(5)
SAMPLE_FRESH_NOISE, SAMPLE_DRAWS_ONLY = 1, 2   # MMT_SAMPLE_* flags


def sampler_steps_route(A: int, H: int) -> int:
    """The form mmt_diffusion_sample_steps takes at action width A and hidden width H: the
    LDS-resident one while the padded bf16 W1x and W2 rows fit beside the per-wave P + Q rows."""
    ap = A if (A // 8) % 2 else A + 8
    fits = 4 * H * ap + 2048 * ((H + 63) // 64) <= 160 * 1024
    return SAMPLER_ROUTE_STEPS_LDS if fits else SAMPLER_ROUTE_STEPS_STREAM


def sampler_last_route() -> int:
    return call("mmt_sampler_last_route")


# MMT_DIFFUSION_LOSS_ROUTE_* (include/mmt_api.h): what mmt_diffusion_loss_last_route() reports
DIFFUSION_LOSS_ROUTE_NONE, DIFFUSION_LOSS_ROUTE_LDS, DIFFUSION_LOSS_ROUTE_STREAM = range(3)


def diffusion_loss_route(A: int, H: int) -> int:
    """The form mmt_diffusion_loss_multi takes at action width A and hidden width H (the
    sampler's LDS budget)."""
    lds = sampler_steps_route(A, H) == SAMPLER_ROUTE_STEPS_LDS
    return DIFFUSION_LOSS_ROUTE_LDS if lds else DIFFUSION_LOSS_ROUTE_STREAM


def diffusion_loss_last_route() -> int:
    return call("mmt_diffusion_loss_last_route")


# observation pad masks (include/mmt_api.h): the key logit of a masked token, the set limit, the
# device status bit of a Readout set flagged absent
PAD_MASK_LOGIT, PAD_MASK_MAX_SETS, FAULT_PAD_MASK = -1024.0, 16, 16
VALUE_UNIFORM, VALUE_MU_LAW = 0, 1   # MMT_VALUE_* (mmt_value_tokens_fwd encoding)
VALUE_MIN_BINS, VALUE_MAX_BINS = 2, 4096
# MMT_PC_* limits of the point-cloud tokenizer (mmt_pc_sample_group, mmt_pc_embed_fwd / _bwd)
PC_MAX_POINTS, PC_MAX_TOKENS, PC_MAX_NEIGHBOURS = 4096, 256, 32
PC_MIN_FEATURES, PC_MAX_FEATURES, PC_MAX_WIDTH = 3, 8, 4096
PC_HIDDEN_WIDTHS = (32, 64, 128)
DEPTH_MAX_PIXELS = 1 << 20           # mmt_depth_unproject: H * W at most
# MMT_AUGMENT_* limits of mmt_image_augment: the side of a frame, the image slots of a sample, the
# cameras, B * I
AUGMENT_MAX_SIDE, AUGMENT_MAX_IMAGES, AUGMENT_MAX_CAMERAS, AUGMENT_MAX_FRAMES = 2048, 64, 16, 1 << 24
QK_NORM_WIDTHS = (32, 64, 128, 256)   # head widths of mmt_qk_norm_fwd / _bwd
HEAD_LOSS_MSE, HEAD_LOSS_L1 = 0, 1   # MMT_HEAD_LOSS_* (mmt_head_continuous loss_kind)
DECODE_ARGMAX, DECODE_SAMPLE = 0, 1  # MMT_DECODE_* (mmt_head_categorical_decode mode)


def workspace_size(op: int, *dims: int) -> int:
    arr = (ctypes.c_int64 * len(dims))(*dims)
    return call("mmt_workspace_size", op, arr, len(dims))


def ptr(t) -> int | None:
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
