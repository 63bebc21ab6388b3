"""OCTO model and diffusion training step, mirroring the reference's
``multi_modal_transformers/models/octo/octo.py`` (Octo :55-198, generate_readouts :91-126,
compute_diffusion_denoise_loss :139-145, diffusion_train_step :204-240, OCTOTrainState :326-332,
create_octo_train_state :334-386).

MI355X design of the step (SURVEY §3.1 call stack):
  tokenizers  : frozen T5 (bf16 GEMM/attention kernels) -> Dense(768->D) [build addition for D!=768];
                image stem kernels; device-drawn patch positions; value tokens (proprioception:
                mu-law bins -> a shared embedding table, tokenizers/numeric_values); point-cloud
                tokens (farthest-point sampling + kNN grouping -> a shared two-layer embedding
                with a max over the neighbours, tokenizers/pointclouds)
  sequence    : ONE fused kernel writes the token sequence (text | image + row/col emb | readout
                embedding) + the learned position embedding; the blockwise mask is a token-set
                table evaluated inside the attention kernel, never an (B, H, L, L) tensor
  backbone    : StackedEncoder1DBlock with ToMe, explicit fwd/bwd (attention_blocks/attention.py)
  head        : diffusion denoise loss (action_heads/diffusion.py)
  optimizer   : one fused AdamW launch over the flat parameter buffer; device step counter;
                optionally a learning-rate schedule, global-norm clipping and non-finite-step
                skipping evaluated on the device (AdamW, OCTOTrainState.opt); optionally
                parameter groups (a weight-decay mask, frozen parameters: a flag byte per 64
                elements read by the kernels), and then a backward that stops at the lowest
                block still trained (Octo.set_param_groups); optionally an EMA of the
                parameters updated in the same launch (AdamW.ema_decay, ema_weights())
Everything after the input upload is stream-ordered device work with no host sync, so the whole
step is captured into a HIP graph and replayed (see OCTOTrainState.graphed_step).
"""
from __future__ import annotations

import ctypes
import os

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Union

import numpy as np
import torch

from ... import _C, _kernels as K
from ...tracing import phase
from ...action_heads.categorical import CategoricalActionHead
from ...action_heads.continuous import ContinuousActionHead, chunk_flat
from ...action_heads.diffusion import DiffusionActionHead
from ...attention_blocks.attention import (LayerCtx, MultiHeadAttentionPooling,
                                           StackedEncoder1DBlock, check_pad_masks)
from ...layers import Dense, wgrad_overlap
from ...params import GROUP_CHUNK, ParamStore, he_normal, normal
from ...schedules import (Constant, ConstantEmaDecay, EmaDecay, Schedule, WarmupCosine,
                          WarmupRsqrt)
from ...tokenizers.images.image_tokenizer import ImageTokenizer
from ...tokenizers.readout.readout import AddPositionEmbedding
from ...tokenizers.text.t5_base import T5Tokenizer
from ...tokenizers.token_compression import MergeSource
from ...tokenizers.numeric_values.value_tokenizer import ValueTokenizer
from ...tokenizers.pointclouds.point_cloud_tokenizer import PointCloudTokenizer
from ...tokenizers.token_sequencer import Image, PointCloud, Readout, Text, TokenSequence, Value
from .config import OctoConfig, get_config

KIND_TEXT, KIND_IMAGE, KIND_READOUT, KIND_VALUE, KIND_POINT = 0, 1, 2, 3, 4


class Octo:
    """Reference octo.py:55-198. ``Octo(config, device)`` declares, initialises (seeded, Flax
    initialisers) and uploads every parameter. ``config``: a preset / model_configs name, an
    OctoConfig, or a composed reference-schema dict (``config_loader.compose("octo_base")``,
    the DictConfig the reference's Octo(config) takes)."""

    def __init__(self, config: OctoConfig | str = "octo-small", device="cuda", seed: int = 0):
        if isinstance(config, dict):   # a composed reference-schema config (config_loader.compose)
            from ...config_loader import octo_config_from_yaml
            config = octo_config_from_yaml(config)
        self.cfg = cfg = get_config(config) if isinstance(config, str) else config
        self.device = torch.device(device)
        D = cfg.token_embedding_dim
        self.D = D
        self.seq = TokenSequence(cfg.input_sequence, cfg.token_compression_sequence)
        sets0 = self.seq.token_sequence
        # observation pad masks: set_pad_mask's second dimension, the Readout sets (never
        # absent), the set text_pad_mask speaks of (-1: none)
        self.n_sets, self.readout_set_bits, self.text_set = self.seq.pad_mask_layout()
        self.image_sets = [i for i, ts in enumerate(sets0) if isinstance(ts, Image)]
        self.L0 = sum(ts.num_tokens for ts in sets0)
        self.n_images = sum(isinstance(ts, Image) for ts in sets0)
        self.n_text = sum(ts.num_tokens for ts in sets0 if isinstance(ts, Text))
        self.n_readout = sum(ts.num_tokens for ts in sets0 if isinstance(ts, Readout))
        self.n_value_sets = sum(isinstance(ts, Value) for ts in sets0)
        self.n_values = sum(ts.num_tokens for ts in sets0 if isinstance(ts, Value))
        for ts in sets0:
            if isinstance(ts, Value) and ts.tokens_compressed_per_layer:
                raise ValueError("Value sets are never compressed: token_compression_sequence must "
                                 f"give them {{0}}, got {{{ts.tokens_compressed_per_layer}}}")
        pc_sets = [ts for ts in sets0 if isinstance(ts, PointCloud)]
        self.n_pc_sets = len(pc_sets)
        self.pc_set_ids = [i for i, ts in enumerate(sets0) if isinstance(ts, PointCloud)]
        self.pc_tokens = pc_sets[0].num_tokens if pc_sets else 0   # tokens per cloud
        for ts in pc_sets:
            if ts.tokens_compressed_per_layer:
                raise ValueError("PointCloud sets are never compressed: token_compression_sequence "
                                 f"must give them {{0}}, got {{{ts.tokens_compressed_per_layer}}}")
            if ts.num_tokens != self.pc_tokens:
                raise ValueError("every PointCloud set must hold the same number of tokens, got "
                                 f"{[t.num_tokens for t in pc_sets]}")
        # image augmentation of the training losses (OctoConfig.image_augmentation): no parameter
        self.augmentation = None
        self.last_augmentation = None   # (augmented images, params) of the last augmented forward
        if cfg.image_augmentation is not None:
            from ...tokenizers.images.augment import ImageAugmentation
            cams = cfg.image_camera()
            if len(cams) != self.n_images:
                raise ValueError(f"image_augmentation maps {len(cams)} image sets, the sequence "
                                 f"has {self.n_images}")
            self.augmentation = ImageAugmentation(cfg.image_augmentation["cameras"], cams)
        self.has_text = self.n_text > 0
        if self.has_text and cfg.text_tokens != self.n_text:
            raise ValueError("text_tokens must equal the text set sizes of input_sequence")
        store = self.store = ParamStore()
        # ---- tokenizers
        self.image_tokenizer = ImageTokenizer(cfg.image_size, cfg.patch_size, True,
                                              cfg.position_interval, "patch_encoding", D,
                                              resnet=cfg.stem).bind(store, "ImageTokenizer_0")
        NP = self.image_tokenizer.num_patches
        for ts in sets0:
            if isinstance(ts, Image) and ts.num_tokens != NP:
                raise ValueError(f"Image set of {ts.num_tokens} tokens != {NP} patches")
        self.text_proj = None
        if self.has_text and cfg.t5.d_model != D:
            self.text_proj = Dense(store, "TextProjection_0", cfg.t5.d_model, D)
        # readouts = AddPositionEmbedding(zeros) (octo.py:103-108); the add itself is fused into
        # the sequence assembly kernel, the module owns the parameter
        self.readout_encoder = AddPositionEmbedding().bind(store, "AddPositionEmbedding_0",
                                                           self.n_readout, D)
        self.readout_pe = self.readout_encoder.pe
        # ---- backbone (posembed_input of StackedEncoder1DBlock, attention.py:97-100)
        self.pos_embed = store.add("StackedEncoder1DBlock_0/posembed_input/pos_embedding",
                                   (self.L0, D), normal(0.02))
        self.stack = StackedEncoder1DBlock.create(store, "StackedEncoder1DBlock_0", cfg.num_blocks,
                                                  D, cfg.num_heads, cfg.mlp_dim, cfg.layer_norm_eps,
                                                  cfg.dropout_rate, cfg.attention_dropout_rate,
                                                  fp8=cfg.fp8, fp8_residual=cfg.fp8_residual,
                                                  normalize_qk=cfg.normalize_qk)
        # ---- head
        self.head = DiffusionActionHead.create(store, "diffusion_action_head", D,
                                               cfg.action_space_dim * cfg.action_horizon,
                                               cfg.diffusion_steps,
                                               num_blocks=cfg.denoise_blocks, sampler=cfg.sampler,
                                               n_diffusion_samples=cfg.n_diffusion_samples)
        self.continuous_head = self.categorical_head = None
        if "continuous" in cfg.action_heads:
            self.continuous_head = ContinuousActionHead(store, "continuous_action_head", D,
                                                        cfg.action_space_dim, cfg.max_action,
                                                        horizon=cfg.pred_horizon,
                                                        loss=cfg.continuous_loss)
        if "categorical" in cfg.action_heads:
            self.categorical_head = CategoricalActionHead(store, "categorical_action_head", D,
                                                          cfg.action_space_dim, cfg.num_bins,
                                                          cfg.max_action, horizon=cfg.pred_horizon)
        # readout pooling by attention (OctoConfig.readout_pooling): declared after every head, so
        # the offsets of all the parameters above are those of the "mean" configuration
        self.pooling = None
        if cfg.readout_pooling == "attention":
            self.pooling = MultiHeadAttentionPooling.create(
                store, "diffusion_action_head/MultiHeadAttentionPooling_0", D,
                cfg.pooling_heads or cfg.num_heads, cfg.pooling_mlp_dim or D, cfg.layer_norm_eps,
                cfg.pooling_norm_axes)
            self.head.attach_pooling(self.pooling)
        # value tokens: declared last of all and only with Value sets in the sequence, so every
        # configuration without them keeps its parameter offsets and seeded initial values
        self.value_tokenizer = None
        if self.n_values:
            self.value_tokenizer = ValueTokenizer(**(cfg.value_tokenizer or {})).bind(
                store, "ValueTokenizer_0", D)
        elif cfg.value_tokenizer is not None:
            raise ValueError("value_tokenizer is set but input_sequence has no Value set")
        # point-cloud tokens: declared after the value tokenizer and only with PointCloud sets
        self.point_cloud_tokenizer = None
        self.pc_points = self.pc_features = 0
        if self.n_pc_sets:
            if cfg.point_cloud_tokenizer is None:
                raise ValueError("input_sequence has PointCloud sets: set point_cloud_tokenizer "
                                 "(num_points at least)")
            pc = dict(cfg.point_cloud_tokenizer)
            self.pc_points = int(pc.pop("num_points"))
            self.point_cloud_tokenizer = PointCloudTokenizer(**pc).bind(
                store, "PointCloudTokenizer_0", D)
            self.pc_features = self.point_cloud_tokenizer.C
        elif cfg.point_cloud_tokenizer is not None:
            raise ValueError("point_cloud_tokenizer is set but input_sequence has no PointCloud set")
        store.materialize(self.device, seed)
        # MMT_DETERMINISTIC=1: bitwise-reproducible gradients (ParamStore.set_deterministic)
        if os.environ.get("MMT_DETERMINISTIC", "0") == "1" and torch.device(self.device).type == "cuda":
            store.set_deterministic(True)
        self.t5 = T5Tokenizer(cfg.t5).materialize(self.device, seed + 1) if self.has_text else None
        self._merge_sources = None  # the last tracked forward's source buffers (merge_source)
        self._cut = (0, False)      # where the backward stops (set_param_groups)
        self._build_tables()

    # ------------------------------------------------------------------ static tables
    def _build_tables(self):
        cfg = self.cfg
        NP = self.image_tokenizer.num_patches
        row_src = []
        ti = ii = ri = vi = pi = 0
        for ts in self.seq.token_sequence:
            for j in range(ts.num_tokens):
                if isinstance(ts, Text):
                    row_src.append((KIND_TEXT << 24) | (ti + j))
                elif isinstance(ts, Image):
                    row_src.append((KIND_IMAGE << 24) | (ii * NP + j))
                elif isinstance(ts, Value):   # rows the sequence assembly leaves to the tokenizer
                    row_src.append((KIND_VALUE << 24) | (vi + j))
                elif isinstance(ts, PointCloud):   # likewise
                    row_src.append((KIND_POINT << 24) | (pi + j))
                else:
                    row_src.append((KIND_READOUT << 24) | (ri + j))
            if isinstance(ts, Text):
                ti += ts.num_tokens
            elif isinstance(ts, Image):
                ii += 1
            elif isinstance(ts, Value):
                vi += ts.num_tokens
            elif isinstance(ts, PointCloud):
                pi += ts.num_tokens
            else:
                ri += ts.num_tokens
        self.row_src = torch.tensor(row_src, dtype=torch.int32, device=self.device)
        # value (set-major, slot) -> sequence row
        self.value_rows = torch.tensor([row for row, v in enumerate(row_src)
                                        if v >> 24 == KIND_VALUE], dtype=torch.int32,
                                       device=self.device)
        # point-cloud token (set-major, centroid) -> sequence row
        self.pc_rows = torch.tensor([row for row, v in enumerate(row_src)
                                     if v >> 24 == KIND_POINT], dtype=torch.int32,
                                    device=self.device)
        img_rows = np.zeros(ii * NP, np.int32)                 # image token -> sequence row
        for row, v in enumerate(row_src):
            if v >> 24 == KIND_IMAGE:
                img_rows[v & 0xFFFFFF] = row
        self.img_rows = torch.from_numpy(img_rows).to(self.device)
        # per-layer token-set tables (square masks) + ToMe set / r
        self.layer_sets = []
        if cfg.compression not in ("tome", "prune"):
            raise ValueError(f"compression must be 'tome' or 'prune', got {cfg.compression!r}")
        for layer in range(cfg.num_blocks):
            sets = self.seq.set_table(layer)
            merged = [i for i, ts in enumerate(self.seq._parse(layer) if cfg.token_compression_sequence
                                                else self.seq.token_sequence)
                      if ts.tokens_compressed_per_layer > 0]
            if cfg.compression == "prune":
                # top-k per token set, uncompressed sets keep all their tokens (k = n)
                prune = None
                if merged:
                    nxt = self.seq.set_table(layer + 1)
                    if min(nxt.lens) < 0:
                        raise ValueError(f"layer {layer}: pruning empties a token set")
                    prune = (tuple(zip(sets.starts, sets.lens)), tuple(nxt.lens))
                self.layer_sets.append((sets, K.SetTable(sets.starts, sets.lens, sets.vis, sets.causal),
                                        -1, 0, prune, ()))
                continue
            # ToMe per compressed token set (token_sequencer.py:222-238 gives every set its own
            # per-layer count): one bipartite match + merge per set, sizes carried per set
            parsed = self.seq._parse(layer)
            plan = []
            for si in merged:
                r = parsed[si].tokens_compressed_per_layer
                t = sets.lens[si]
                if r > t // 2:
                    raise ValueError(f"layer {layer}: ToMe r={r} exceeds t//2={t // 2} in set {si}")
                plan.append((si, r))
            tome_set = plan[0][0] if len(plan) == 1 else (-2 if plan else -1)
            self.layer_sets.append((sets, K.SetTable(sets.starts, sets.lens, sets.vis, sets.causal),
                                    tome_set, sum(r for _, r in plan), None, tuple(plan)))
        final = self.seq.set_table(cfg.num_blocks) if cfg.token_compression_sequence else self.seq.set_table(0)
        self.L_final = final.L
        rows = [s + j for s, n, m in zip(final.starts, final.lens, final.modalities) if m == "readouts"
                for j in range(n)]
        self.readout_rows = torch.tensor(rows, dtype=torch.int32, device=self.device)
        flag = np.full(self.L_final, -1, np.int32)
        flag[rows] = np.arange(len(rows))
        self.readout_flag = torch.from_numpy(flag).to(self.device)
        # categorical head: readout i belongs to group i // (n / G) ("batch (action timestep)
        # embeddings", categorical.py:32-36), G = pred_horizon * action_space_dim groups,
        # step-major (group g = step * A + a)
        G = self.n_groups = cfg.pred_horizon * cfg.action_space_dim
        self.readout_group = self.readout_group_counts = None
        if len(rows) % G == 0:
            per = len(rows) // G
            grp = np.full(self.L_final, -1, np.int32)
            grp[rows] = np.arange(len(rows)) // per
            self.readout_group = torch.from_numpy(grp).to(self.device)
            self.readout_group_counts = torch.full((G,), per, dtype=torch.int32, device=self.device)

    def layer_ctxs(self, train: bool, rng, sample_offset: int, pad=None) -> List[LayerCtx]:
        """pad: (packed set words, text token mask) of the observation pad masks, or None."""
        prop = bool(self.cfg.proportional_attention)
        track = bool(self.cfg.track_merge_source)
        words, text_mask = pad if pad is not None else (None, None)
        ctxs, carried = [], -1  # carried: the set whose sizes the last single-set merge handed on
        for i, (s, t, ts, r, pr, plan) in enumerate(self.layer_sets):
            ctxs.append(LayerCtx(layer=i, sets=s, table=t, tome_set=ts, r=r, prune=pr, train=train,
                                 rng=rng, sample_offset=sample_offset, tome_plan=plan,
                                 prop_attn=prop, size_set=carried, track_source=track,
                                 pad_words=words, text_mask=text_mask, text_set=self.text_set))
            if len(plan) == 1:
                carried = plan[0][0]
        return ctxs

    # ------------------------------------------------------------------ forward / backward
    def _check_values(self, values, B: int):
        """The `values` argument as the (B, n_values) fp32 matrix the tokenizer reads, None for a
        model without Value sets. ValueError: values missing from a model with Value sets, given
        to one without, not an fp32 tensor on the model's device, or of a shape other than
        (B, n_sets, n) / (B, n_sets * n)."""
        if not self.n_values:
            if values is not None:
                raise ValueError("values given, but input_sequence has no Value set")
            return None
        if values is None:
            raise ValueError(f"input_sequence has Value sets: pass values, fp32 "
                             f"(B, {self.n_value_sets}, n) or (B, {self.n_values})")
        if not torch.is_tensor(values) or values.dtype != torch.float32:
            raise ValueError("values must be an fp32 tensor")
        if values.device.type != self.device.type:
            raise ValueError(f"values must live on the model's device ({self.device.type})")
        flat = values.dim() == 2 and tuple(values.shape) == (B, self.n_values)
        sets = values.dim() == 3 and values.shape[:2] == (B, self.n_value_sets) and \
            values.shape[1] * values.shape[2] == self.n_values
        if not (flat or sets):
            raise ValueError(f"values {tuple(values.shape)}: expected ({B}, {self.n_value_sets}, "
                             f"n) or ({B}, {self.n_values})")
        return values.reshape(B, self.n_values)

    def _check_point_clouds(self, point_clouds, B: int, fps_start=None):
        """The `point_clouds` argument checked, None for a model without PointCloud sets.
        ValueError: point_clouds missing from a model with PointCloud sets, given to one without,
        not an fp32 tensor on the model's device, or of a shape other than (B, n_sets, P, C);
        fps_start not an int32 (B, n_sets) tensor on that device."""
        if not self.n_pc_sets:
            if point_clouds is not None or fps_start is not None:
                raise ValueError("point_clouds given, but input_sequence has no PointCloud set")
            return None
        shape = (B, self.n_pc_sets, self.pc_points, self.pc_features)
        if point_clouds is None:
            raise ValueError(f"input_sequence has PointCloud sets: pass point_clouds, fp32 {shape}")
        if not torch.is_tensor(point_clouds) or point_clouds.dtype != torch.float32:
            raise ValueError("point_clouds must be an fp32 tensor")
        if point_clouds.device.type != self.device.type:
            raise ValueError(f"point_clouds must live on the model's device ({self.device.type})")
        if tuple(point_clouds.shape) != shape:
            raise ValueError(f"point_clouds {tuple(point_clouds.shape)}: expected {shape}")
        if fps_start is not None and (
                not torch.is_tensor(fps_start) or fps_start.dtype != torch.int32
                or tuple(fps_start.shape) != shape[:2]
                or fps_start.device.type != self.device.type):
            raise ValueError(f"fps_start must be an int32 {shape[:2]} tensor on the model's device")
        return point_clouds

    def _check_point_cloud_counts(self, counts, point_clouds, B: int):
        """The `point_cloud_counts` argument checked before any launch. ValueError: given without
        point_clouds or to a model without PointCloud sets, not an int32 (B, n_pc_sets) tensor on
        the model's device, or compression == "prune" (a thin cloud is an absent set, and the
        pad masks cannot be combined with prune)."""
        if counts is None:
            return None
        if not self.n_pc_sets:
            raise ValueError("point_cloud_counts given, but input_sequence has no PointCloud set")
        if point_clouds is None:
            raise ValueError("point_cloud_counts given without point_clouds")
        if self.cfg.compression == "prune":
            raise ValueError('point_cloud_counts cannot be combined with compression == "prune": '
                             "a thin cloud is an absent token set, and the attention's key_bias "
                             "cannot be combined with wsum")
        shape = (B, self.n_pc_sets)
        if not torch.is_tensor(counts) or counts.dtype != torch.int32 or \
                tuple(counts.shape) != shape or counts.device.type != self.device.type:
            raise ValueError(f"point_cloud_counts must be an int32 {shape} tensor on the model's "
                             f"device ({self.device.type})")
        return counts.contiguous()

    def _check_augment(self, images, rng):
        """An augmented forward's inputs checked before any launch. ValueError: images not a
        uint8 (B, n_images, H, W, 3) tensor on the model's device (fp32 frames are refused: the
        augmentation is defined on uint8, and the stem keeps its fused uint8 route), rng
        missing."""
        if not torch.is_tensor(images) or images.dtype != torch.uint8:
            raise ValueError("image_augmentation is configured: the training losses take uint8 "
                             f"images, got {getattr(images, 'dtype', type(images))}")
        if images.dim() != 5 or images.shape[1] != self.n_images or images.shape[-1] != 3:
            raise ValueError(f"images {tuple(images.shape)}: expected (B, {self.n_images}, H, W, "
                             "3) for the augmentation")
        if images.device.type != self.device.type:
            raise ValueError(f"images must live on the model's device ({self.device.type})")
        if rng is None:
            raise ValueError("image_augmentation is configured: the training losses need rng "
                             "(the {seed, step} words the draws are keyed by)")

    def _check_pad_masks(self, set_pad_mask, text_pad_mask, B: int, images=None) -> bool:
        """The observation pad masks checked before any launch; returns whether one is given.
        ValueError: not a bool tensor on the model's device, set_pad_mask not (B, the set count
        of input_sequence after the repeat expansion), text_pad_mask not (B, the tokens of the
        first text set), text_pad_mask without a text set or with a compressed one, either
        mask with compression == "prune" (key_bias cannot be combined with wsum), and, with
        set_pad_mask and `images` (the (B, I, H, W, C) batch whose absent cameras
        mmt_pad_mask_images zeroes in a copy), more than 65,535 images or an image whose bytes
        are no multiple of 16."""
        if set_pad_mask is None and text_pad_mask is None:
            return False
        if self.cfg.compression == "prune":
            raise ValueError('pad masks cannot be combined with compression == "prune": the '
                             "attention's key_bias cannot be combined with wsum")
        T = -1
        if self.text_set >= 0:
            ts = self.seq.token_sequence[self.text_set]
            T = ts.num_tokens
            if text_pad_mask is not None and ts.tokens_compressed_per_layer:
                raise ValueError("text_pad_mask: the text set is compressed (per-token masks of "
                                 "compressed sets are not supported)")
        check_pad_masks(set_pad_mask, text_pad_mask, B, self.n_sets, T, self.device)
        if set_pad_mask is not None and images is not None and self.image_sets:
            I = len(self.image_sets)
            nbytes = images[0, 0].numel() * images.element_size()
            if B * I > 65535 or nbytes % 16:
                raise ValueError(f"set_pad_mask: the images of absent cameras are zeroed in a copy "
                                 f"moved as 16-B vectors, one grid row per image: B * I = {B * I} "
                                 f"must be <= 65535 and the bytes of an image ({nbytes}) a "
                                 "multiple of 16")
        return True

    def generate_readouts(self, text_tokens, images, train=True, rng=None, sample_offset=0,
                          positions=None, tome=None, t5_out=None, values=None, point_clouds=None,
                          fps_start=None, set_pad_mask=None, text_pad_mask=None,
                          point_cloud_counts=None, augment: bool = False):
        """Reference :91-126. Returns the final sequence (B, L_final, D) and the saved state.
        augment: with OctoConfig.image_augmentation set, the tokenizers read an augmented copy of
        the uint8 images (tokenizers/images/augment.py: one draw per (seed, step, sample_offset +
        b, camera) from rng, which is then required), made before the absent cameras are zeroed;
        `images` itself is not changed, point_clouds are not moved with the crop, and the copy
        and its parameters stay in the saved state ("aug_images", "aug_params" (B, n_cam, 8)) and
        on the model (last_augmentation). fp32 images are refused then. The compute_*_loss methods
        pass their `train` flag; the predict_* methods never augment. Without
        image_augmentation the flag does nothing.
        t5_out: the frozen T5 encoder's output for text_tokens, computed ahead (DDPStep's
        cross-step T5 pipeline); None runs the encoder here. values: the numbers behind the
        Value sets, fp32 (B, n_sets, n) or (B, n_sets * n), expected in [-1, 1]
        (tokenizers/numeric_values/value_tokenizer.py); required with Value sets in
        input_sequence, refused without. point_clouds: the clouds behind the PointCloud sets,
        fp32 (B, n_sets, P, C) (tokenizers/pointclouds/point_cloud_tokenizer.py), required and
        refused likewise; fps_start (tests): int32 (B, n_sets), the first sampled point of every
        cloud instead of the step's own (train: drawn, eval: point 0).
        set_pad_mask, text_pad_mask (the observation pad masks, both optional, bool, True = real):
        set_pad_mask (B, n_sets) flags the token sets of input_sequence, in sequence order after
        the repeat expansion, that a sample has (a dataset without a wrist camera; a history step
        is absent when all its sets are); text_pad_mask (B, T) flags the real tokens of the first
        text set (an instruction's attention_mask). A masked token gets no attention weight as a
        key in any block, its row of the assembled sequence holds pos_embedding alone whatever
        the caller passed for it, and no gradient reaches a tokenizer through it (DESIGN.md,
        "Observation pad masks"). Readout sets cannot be absent (reported by K.device_status()).
        point_cloud_counts: int32 (B, n_pc_sets) on the device, the leading rows of every cloud of
        point_clouds that are points (tokenizers/pointclouds/depth.py gives both); the other rows
        are never read. A cloud with fewer points than its set has tokens is an absent set for
        its sample, as if set_pad_mask flagged it; the counts are read on the device, so a
        replayed step follows new contents of the buffer. Refused without point_clouds, without
        PointCloud sets and with compression == "prune" ("Ragged clouds and depth
        back-projection")."""
        B = images.shape[0]
        D = self.D
        values = self._check_values(values, B)
        counts = self._check_point_cloud_counts(point_cloud_counts, point_clouds, B)
        point_clouds = self._check_point_clouds(point_clouds, B, fps_start)
        padded = self._check_pad_masks(set_pad_mask, text_pad_mask, B, images)
        padded = padded or counts is not None
        augment = bool(augment) and self.augmentation is not None
        if augment:
            self._check_augment(images, rng)
        st: Dict = dict(B=B, train=train, rng=rng, sample_offset=sample_offset)
        if augment:
            # before the pad masks: an absent camera's augmented frame is zeroed like any other
            params = torch.empty((B, self.augmentation.n_cam, 8), dtype=torch.float32,
                                 device=images.device)
            with phase("fwd/augment"):
                images = self.augmentation(images.contiguous(), rng, sample_offset,
                                           params_out=params)
            st["aug_images"], st["aug_params"] = images, params
            self.last_augmentation = (images, params)
        txt, T = None, max(self.n_text, 1)
        if self.has_text:
            if t5_out is None:
                with phase("fwd/t5"):
                    t5_out = self.t5(text_tokens)                           # stop_gradient
            st["t5_out"] = t5_out
            if self.text_proj is not None:
                txt = self.text_proj.fwd(t5_out.view(B * self.n_text, -1)).view(B, self.n_text, D)
            else:
                txt = t5_out
        pad = None
        if padded:
            if counts is not None:
                # a cloud with fewer points than tokens is an absent set of its sample: a bit of
                # the packed words, from the counts on the device (no host synchronisation)
                words = K.pad_mask_pack_counts(set_pad_mask, self.n_sets, self.readout_set_bits,
                                               counts, self.pc_set_ids,
                                               [self.pc_tokens] * self.n_pc_sets)
            else:
                words = (None if set_pad_mask is None
                         else K.pad_mask_pack(set_pad_mask, self.readout_set_bits))
            pad = st["pad"] = (words, text_pad_mask)
            if set_pad_mask is not None and self.image_sets:   # counts make no camera absent
                # the stem's GroupNorm runs over all patches of all cameras of a sample: it reads
                # a copy of the images with the absent cameras' pixels zeroed, so they reach no
                # present camera's tokens through its statistics
                images = K.pad_mask_images(images.contiguous(), words, self.image_sets,
                                           self.n_sets)
        with phase("fwd/stem"):
            img_tok, (rt, ct), isv = self.image_tokenizer.forward(images, train, rng, sample_offset,
                                                                  positions)
        st.update(img_sv=isv, rt=rt, ct=ct, img_tok=img_tok, txt=txt)
        x0 = torch.empty((B, self.L0, D), dtype=torch.float32, device=images.device)  # fp32 residual
        NI = img_tok.shape[1]
        _C.call("mmt_seq_assemble_fwd", B, self.L0, D, _C.ptr(self.row_src), _C.ptr(txt), T,
                _C.ptr(img_tok), NI, _C.ptr(rt), _C.ptr(ct), _C.ptr(self.image_tokenizer.row_emb.data),
                _C.ptr(self.image_tokenizer.col_emb.data), _C.ptr(self.readout_pe.data),
                _C.ptr(self.pos_embed.data), _C.ptr(x0), _C.stream_ptr())
        if values is not None:  # the rows of kind 3, which the assembly skipped
            st["val_tok"] = self.value_tokenizer.forward(values, self.value_rows,
                                                         self.pos_embed.data, x0)
        if point_clouds is not None:  # the rows of kind 4
            st["pc_sv"] = self.point_cloud_tokenizer.forward(
                point_clouds, self.pc_tokens, self.pc_rows, self.pos_embed.data, x0, train, rng,
                sample_offset, fps_start, counts)
        if padded:
            # after every tokenizer has written x0: the masked rows hold pos_embedding alone
            K.pad_mask_rows_fwd(x0, self.pos_embed.data, self.layer_sets[0][1], words,
                                text_pad_mask, self.text_set)
        ctxs = self.layer_ctxs(train, rng, sample_offset, pad)
        if tome is not None:  # injected ToMe index triples (tests: the golden step fixtures)
            for c, idx in zip(ctxs, tome):
                c.tome_forced = idx
        with phase("fwd/blocks"):
            xL, ssv = self.stack.forward(x0, ctxs)
        if self.cfg.track_merge_source:
            # the model keeps the forward's source buffers: a captured step drops its saved state,
            # and every replay rewrites these same buffers
            self._merge_sources = ssv[-1].get("merge_source") if ssv else {}
        st.update(ctxs=ctxs, stack_sv=ssv, NI=NI, T=T)
        return xL, st

    def merge_source(self, st: Optional[Dict] = None, *, _maps=None) -> Dict[int, MergeSource]:
        """{set index: MergeSource} of the forward that produced the saved state ``st``: for every
        merged token set, which of its final rows each original token (image patch) ended up in.
        ``st`` None: the model's last forward (a captured step holds its own buffers, which every
        replay rewrites: DDPStep.merge_source). The maps are copies: a later forward or replay does
        not change them. Needs OctoConfig.track_merge_source."""
        if not self.cfg.track_merge_source:
            raise RuntimeError("merge_source: this model was built with track_merge_source off "
                               "(OctoConfig.track_merge_source / YAML track_merge_source: true)")
        if _maps is not None:
            maps = _maps
        elif st is None:
            maps = self._merge_sources
        else:
            maps = st["stack_sv"][-1].get("merge_source") if st.get("stack_sv") else None
        if maps is None:
            raise RuntimeError("merge_source: no tracked forward has run yet")
        return {si: MergeSource(buf.clone(), t) for si, (buf, t) in sorted(maps.items())}

    def compute_diffusion_denoise_loss(self, text_tokens, images, actions, train=True, rng=None,
                                       sample_offset=0, inject: Optional[dict] = None, t5_out=None,
                                       action_pad_mask=None, values=None, point_clouds=None,
                                       set_pad_mask=None, text_pad_mask=None,
                                       point_cloud_counts=None):
        """Reference :139-145. Returns (loss (1,) fp32 device tensor, saved state). inject (tests):
        positions (rt, ct), t, eps, tome (per block an (unm, src, dst) triple of int32 device
        tensors or None) replace the step's own draws / matching. t5_out: the frozen encoder's
        output for text_tokens computed ahead (generate_readouts).
        action_pad_mask: bool (B, action_horizon, action_space_dim) or (B, h a), True where an
        action component is real: padded chunk steps / action dimensions do not enter the loss,
        which is normalised by the number of real components. With it, or with
        OctoConfig.n_diffusion_samples = K > 1 (K independent (t, eps) draws per sample; inject
        t (K, B) / eps (K, B, h a)), the head runs its fused multi-draw loss on the pooled readout
        (DiffusionActionHead.loss_forward_multi). values, point_clouds: generate_readouts'
        (inject fps_start: its fps_start), and so are set_pad_mask and text_pad_mask."""
        inject = inject or {}
        actions = self._chunk_flat(actions)
        multi = self.cfg.n_diffusion_samples > 1 or action_pad_mask is not None
        if action_pad_mask is not None:
            if action_pad_mask.dtype != torch.bool:
                raise ValueError("action_pad_mask must be a bool tensor")
            action_pad_mask = self._chunk_flat(action_pad_mask)
            if action_pad_mask.shape[0] != actions.shape[0]:
                raise ValueError("action_pad_mask and actions differ in batch size")
        xL, st = self.generate_readouts(text_tokens, images, train, rng, sample_offset,
                                        inject.get("positions"), inject.get("tome"), t5_out,
                                        values=values, point_clouds=point_clouds,
                                        set_pad_mask=set_pad_mask, text_pad_mask=text_pad_mask,
                                        point_cloud_counts=point_cloud_counts,
                                        fps_start=inject.get("fps_start"), augment=train)
        B = xL.shape[0]
        if multi:   # the pooled readout in a tensor of its own: the split first Dense reads it
            cat = None
            pooled = torch.empty((B, self.D), dtype=torch.bfloat16, device=xL.device)
        else:
            cat = self.head.new_cat(B, xL.device)
            pooled = self.head.readout_slot(cat)
        if self.pooling is not None:
            with phase("fwd/pool"):
                _, st["pool_sv"] = self.pooling.forward(xL, self.readout_rows, out=pooled)
        else:
            _C.call("mmt_rows_mean_fwd", _C.ptr(xL), xL.stride(0), xL.stride(1), B, self.D,
                    _C.ptr(self.readout_rows), self.readout_rows.numel(),
                    _C.ptr(pooled), pooled.stride(0), _C.stream_ptr())
        with phase("fwd/head"):
            if multi:
                loss, hsv = self.head.loss_forward_multi(
                    pooled, actions.float().contiguous(), rng, sample_offset,
                    self.cfg.n_diffusion_samples, action_pad_mask, inject.get("t"),
                    inject.get("eps"))
            else:
                loss, hsv = self.head.loss_forward(cat, actions, rng, sample_offset,
                                                   inject.get("t"), inject.get("eps"))
        st.update(head_sv=hsv, xL_shape=tuple(xL.shape), xL=xL)
        return loss, st

    def _chunk_flat(self, actions, horizon: Optional[int] = None):
        """A head's view of an action chunk: (B, h, action_space_dim) or the already flat
        (B, h * action_space_dim), as (B, h a); h = `horizon`, None: the diffusion head's
        action_horizon. A flat tensor is returned as it is."""
        h = self.cfg.action_horizon if horizon is None else horizon
        return chunk_flat(actions, h, self.cfg.action_space_dim)

    def predict_diffusion_denoise_term(self, text_tokens, images, time, noisy_actions, rng=None,
                                       sample_offset=0, train=True, values=None,
                                       point_clouds=None,
                                       set_pad_mask=None, text_pad_mask=None,
                                       point_cloud_counts=None):
        """Reference :130-137: readouts -> pooled readouts (their mean, or the attention
        pooling) -> OctoDenoise (diffusion.py:88-107)."""
        xL, _ = self.generate_readouts(text_tokens, images, train, rng, sample_offset,
                                       values=values, point_clouds=point_clouds,
                                       set_pad_mask=set_pad_mask, text_pad_mask=text_pad_mask,
                                       point_cloud_counts=point_cloud_counts)
        return self.head.predict_denoise_term_mean(self._readout_pooled(xL), time, noisy_actions)

    def predict_diffusion_action(self, text_tokens, images, rng, sample_offset=0, train=True,
                                 z: Optional[torch.Tensor] = None, return_noise=False,
                                 positions=None, sampler=None, values=None, point_clouds=None,
                                 set_pad_mask=None, text_pad_mask=None, point_cloud_counts=None,
                                 fps_start=None):
        """Reference :147-154: readouts (the reference's backbone always runs with
        train=True, :120, and its image encoder samples positions by default) -> readout mean ->
        the sampler (action_heads/diffusion.py:146-209): `sampler` (a SamplerSpec or a dict of its
        fields), else OctoConfig.sampler, else the reference's 32-step DDPM loop. Returns fp32
        (B, action_space_dim), or (B, action_horizon, action_space_dim) with a horizon > 1 (z
        and the returned noise stay flat, (B, h a))."""
        xL, _ = self.generate_readouts(text_tokens, images, train, rng, sample_offset, positions,
                                       values=values, point_clouds=point_clouds,
                                       set_pad_mask=set_pad_mask, text_pad_mask=text_pad_mask,
                                       point_cloud_counts=point_cloud_counts,
                                       fps_start=fps_start)
        if self.pooling is not None:
            e = self._readout_pooled(xL)
        else:
            B = xL.shape[0]
            e = torch.empty((B, self.D), dtype=torch.bfloat16, device=xL.device)
            _C.call("mmt_rows_mean_fwd", _C.ptr(xL), xL.stride(0), xL.stride(1), B, self.D,
                    _C.ptr(self.readout_rows), self.readout_rows.numel(), _C.ptr(e), e.stride(0),
                    _C.stream_ptr())
        out = self.head.predict_action_mean(e, rng, sample_offset, z, return_noise, sampler=sampler)
        h = self.cfg.action_horizon
        if h == 1:
            return out
        chunk = lambda a: a.view(a.shape[0], h, self.cfg.action_space_dim)
        return (chunk(out[0]), *out[1:]) if return_noise else chunk(out)

    def _readout_pooled(self, xL):
        """The diffusion head's conditioning vector (B, D) bf16: the readout mean, or the
        attention pooling of the readout rows (OctoConfig.readout_pooling)."""
        if self.pooling is None:
            return self._readout_mean(xL)
        return self.pooling.forward(xL, self.readout_rows)[0]

    # ------------------------------------------------------------------ other action heads
    def _readout_mean(self, xL):
        B = xL.shape[0]
        e = torch.empty((B, self.D), dtype=torch.bfloat16, device=xL.device)
        _C.call("mmt_rows_mean_fwd", _C.ptr(xL), xL.stride(0), xL.stride(1), B, self.D,
                _C.ptr(self.readout_rows), self.readout_rows.numel(), _C.ptr(e), e.stride(0),
                _C.stream_ptr())
        return e

    def _readout_group_means(self, xL):
        if self.readout_group is None:
            raise ValueError(f"the readout count {self.readout_rows.numel()} must be a multiple "
                             f"of pred_horizon * action_space_dim = {self.n_groups} "
                             "(categorical.py:32-36)")
        B, G = xL.shape[0], self.n_groups
        g = torch.empty((B, G, self.D), dtype=torch.bfloat16, device=xL.device)
        _C.call("mmt_rows_group_mean_fwd", _C.ptr(xL), xL.stride(0), xL.stride(1), B, self.L_final,
                self.D, _C.ptr(self.readout_group), G, _C.ptr(self.readout_group_counts), _C.ptr(g),
                _C.stream_ptr())
        return g

    def _need(self, head, name):
        if head is None:
            raise ValueError(f"{name} head not built: add it to OctoConfig.action_heads")
        return head

    def predict_continuous_action(self, text_tokens, images, rng=None, sample_offset=0, train=True,
                                  values=None, point_clouds=None,
                                  set_pad_mask=None, text_pad_mask=None, point_cloud_counts=None):
        """Reference :158-165 -> (B, pred_horizon, A) fp32 ((B, 1, A) as the reference)."""
        h = self._need(self.continuous_head, "continuous")
        xL, _ = self.generate_readouts(text_tokens, images, train, rng, sample_offset,
                                       values=values, point_clouds=point_clouds,
                                       set_pad_mask=set_pad_mask, text_pad_mask=text_pad_mask,
                                       point_cloud_counts=point_cloud_counts)
        return h.forward(self._readout_mean(xL))

    @staticmethod
    def _check_pad_mask(action_pad_mask):
        if action_pad_mask is not None and action_pad_mask.dtype != torch.bool:
            raise ValueError("action_pad_mask must be a bool tensor")

    def compute_l2_loss(self, text_tokens, images, actions, train=True, rng=None, sample_offset=0,
                        action_pad_mask=None, values=None, point_clouds=None,
                        set_pad_mask=None, text_pad_mask=None, point_cloud_counts=None):
        """Reference :167-174, batch-averaged as continuous_train_step (:262). (loss, saved).
        actions (B, pred_horizon, A) or flat; OctoConfig.continuous_loss picks the squared error
        or L1. action_pad_mask: bool, the actions' shape, True where a component is real: padded
        chunk steps / action dimensions do not enter the loss, which is normalised by the number
        of real components (as compute_diffusion_denoise_loss)."""
        h = self._need(self.continuous_head, "continuous")
        self._check_pad_mask(action_pad_mask)
        xL, st = self.generate_readouts(text_tokens, images, train, rng, sample_offset,
                                        values=values, point_clouds=point_clouds,
                                        set_pad_mask=set_pad_mask, text_pad_mask=text_pad_mask,
                                        point_cloud_counts=point_cloud_counts, augment=train)
        loss, hsv = h.loss_forward(self._readout_mean(xL), actions, action_pad_mask)
        st.update(head_kind="continuous", head_sv=hsv, xL_shape=tuple(xL.shape))
        return loss, st

    def predict_action_logits(self, text_tokens, images, rng=None, sample_offset=0, train=True,
                              values=None, point_clouds=None,
                              set_pad_mask=None, text_pad_mask=None, point_cloud_counts=None):
        """Reference :178-185 -> (B, A, num_bins) fp32, (B, pred_horizon, A, num_bins) with a
        pred_horizon > 1."""
        h = self._need(self.categorical_head, "categorical")
        xL, _ = self.generate_readouts(text_tokens, images, train, rng, sample_offset,
                                       values=values, point_clouds=point_clouds,
                                       set_pad_mask=set_pad_mask, text_pad_mask=text_pad_mask,
                                       point_cloud_counts=point_cloud_counts)
        return h.forward(self._readout_group_means(xL))

    def predict_categorical_action(self, text_tokens, images, rng=None, sample_offset=0, train=True,
                                   mode="argmax", temperature=1.0, values=None,
                                   point_clouds=None,
                                   set_pad_mask=None, text_pad_mask=None, point_cloud_counts=None):
        """The categorical head rolled out: logits (predict_action_logits) decoded to actions
        (B, pred_horizon, A) fp32 through bin_values, by argmax or (mode "sample") one draw per
        component from softmax(logits / temperature) keyed by rng and sample_offset
        (CategoricalActionHead.decode)."""
        h = self._need(self.categorical_head, "categorical")
        logits = self.predict_action_logits(text_tokens, images, rng, sample_offset, train,
                                            values=values, point_clouds=point_clouds,
                                            set_pad_mask=set_pad_mask, text_pad_mask=text_pad_mask,
                                            point_cloud_counts=point_cloud_counts)
        return h.decode(logits, rng, sample_offset, mode, temperature)[0]

    def compute_ce_loss(self, text_tokens, images, actions, train=True, rng=None, sample_offset=0,
                        action_pad_mask=None, values=None, point_clouds=None,
                        set_pad_mask=None, text_pad_mask=None, point_cloud_counts=None):
        """Reference :187-198, averaged as categorical_train_step (:302). (loss, saved).
        actions (B, pred_horizon, A) or flat. action_pad_mask: compute_l2_loss's; the loss is the
        mean of the cross entropy over the real components."""
        h = self._need(self.categorical_head, "categorical")
        self._check_pad_mask(action_pad_mask)
        xL, st = self.generate_readouts(text_tokens, images, train, rng, sample_offset,
                                        values=values, point_clouds=point_clouds,
                                        set_pad_mask=set_pad_mask, text_pad_mask=text_pad_mask,
                                        point_cloud_counts=point_cloud_counts, augment=train)
        loss, hsv = h.loss_forward(self._readout_group_means(xL), actions, action_pad_mask)
        st.update(head_kind="categorical", head_sv=hsv, xL_shape=tuple(xL.shape))
        return loss, st

    # ------------------------------------------------------------------ optimizer groups
    GROUP_PRESETS = {"kernels": ("*/kernel",)}

    def head_prefixes(self) -> List[str]:
        """Name prefixes of the parameters that belong to an action head, from the head objects
        (the pooling module is declared under the diffusion head)."""
        heads = [self.head._name]
        heads += [h.name for h in (self.continuous_head, self.categorical_head) if h is not None]
        if self.pooling is not None:
            heads.append(self.pooling._name)
        return heads

    def _group_selector(self, value, what: str):
        """An AdamW group field as ParamStore.set_groups takes it: None, a tuple of patterns (a
        preset name resolved, a single string one pattern) or, for "head_only", a predicate."""
        if value is None:
            return None
        if isinstance(value, str):
            if value == "head_only" and what == "frozen_keys":
                pre = tuple(p + "/" for p in self.head_prefixes())
                return lambda name: not name.startswith(pre)
            return self.GROUP_PRESETS.get(value, (value,))
        if isinstance(value, (list, tuple)) and all(isinstance(v, str) for v in value):
            return tuple(value)
        raise ValueError(f"{what}: {value!r} is neither None, a preset / pattern string nor a "
                         "sequence of pattern strings")

    def set_param_groups(self, weight_decay_mask=None, frozen_keys=None):
        """Resolve AdamW.weight_decay_mask / frozen_keys against this model's parameter names
        (ParamStore.set_groups: flags per parameter and the device chunk table; ValueError for a
        pattern that matches nothing or a request that freezes everything) and place the
        backward's cut. Both None: no groups, the whole backward."""
        self.store.set_groups(self._group_selector(weight_decay_mask, "weight_decay_mask"),
                              self._group_selector(frozen_keys, "frozen_keys"))
        self._cut = self._backward_cut()
        return self

    def _backward_cut(self):
        """(j, tokens_frozen). The store declares the tokenizers, the stem, TextProjection_0,
        AddPositionEmbedding_0 and posembed_input first, then blocks 0 .. nb-1, then the heads.
        tokens_frozen: everything declared before block 0 is frozen. j: the lowest block the
        backward has to reach: the lowest block holding a trainable parameter (nb if none does),
        or 0 while a parameter before the blocks is trained, whose gradient comes through all of
        them. The backward runs blocks [j, nb) and the token / stem part only for j == 0 and not
        tokens_frozen; with j == nb the heads do not produce the sequence gradient at all. The
        value tokenizer's embedding is a token-level parameter like those before block 0, though
        it is declared after the heads (Octo.__init__); so are the point-cloud tokenizer's
        parameters."""
        nb = self.cfg.num_blocks
        off0 = self._block_offset(0)
        pre = "StackedEncoder1DBlock_0/Block_"
        vpre = ("ValueTokenizer_0/", "PointCloudTokenizer_0/")
        tokens_frozen, j = True, nb
        for p in self.store.params:
            if p.frozen:
                continue
            if p.offset < off0 or p.name.startswith(vpre):
                tokens_frozen = False
            elif p.name.startswith(pre):
                j = min(j, int(p.name[len(pre):].split("/", 1)[0]))
        return (j if tokens_frozen else 0), tokens_frozen

    def stage_active(self, stage: int, stages) -> bool:
        """Does backward_stage(st, stage, stages) launch anything? Stage 0 always (the heads); a
        later stage only if it reaches above the cut (with the cut at 0 every stage does; the
        token / stem backward belongs to the last one)."""
        return stage == 0 or self.stage_bounds(stages)[stage] > self._cut[0]

    # ------------------------------------------------------------------ staged backward
    def _block_offset(self, j: int) -> int:
        """Flat index of block j's first parameter (store.n for j = num_blocks)."""
        if j >= self.cfg.num_blocks:
            return self.store.n
        return self.store.by_name[f"StackedEncoder1DBlock_0/Block_{j}/LayerNorm_0/scale"].offset

    def stage_bounds(self, stages) -> List[int]:
        """Block boundaries nb = b[0] > b[1] > ... > b[S] = 0 of a backward split into S stages
        (stage i runs blocks [b[i+1], b[i]); stage 0 also the heads, the last stage the tokens).
        `stages`: an int S (blocks split evenly), an explicit list, or "auto[:MB]": gradient
        regions of ~MB megabytes (default 24) from the top, and a last stage of block 0 alone, so
        the region all-reduced after the backward ends (block 0 and everything declared before
        it: the tokenizers, the stem) is the smallest possible."""
        nb = self.cfg.num_blocks
        if isinstance(stages, (list, tuple)):
            return self._check_bounds(list(stages))
        if isinstance(stages, str):
            mb = float(stages.split(":", 1)[1]) if ":" in stages else 24.0
            target = mb * (1 << 20)
            bounds, acc = [nb], 0.0
            for j in range(nb - 1, 0, -1):
                acc += 4.0 * (self._block_offset(j + 1) - self._block_offset(j))
                if acc >= target:
                    bounds.append(j)
                    acc = 0.0
            if nb > 1 and bounds[-1] != 1:
                bounds.append(1)
            bounds.append(0)
            return self._check_bounds(bounds)
        n = max(1, min(int(stages), nb))
        return self._check_bounds([nb * (n - i) // n for i in range(n + 1)])  # nb .. 0

    def _check_bounds(self, b: List[int]) -> List[int]:
        """A stage plan must cover blocks nb .. 0 once: b[0] == nb, b[-1] == 0, strictly
        decreasing — otherwise gradient regions would be missing or overlap, parts of the
        gradient never (or twice) all-reduced, and the ranks would drift apart silently."""
        nb = self.cfg.num_blocks
        if (len(b) < 2 or b[0] != nb or b[-1] != 0 or any(int(x) != x for x in b)
                or any(b[i] <= b[i + 1] for i in range(len(b) - 1))):
            raise ValueError(f"stage bounds {b}: need {nb} = b[0] > b[1] > ... > b[-1] = 0")
        return [int(x) for x in b]

    def _stage_bounds(self, n_stages) -> List[int]:
        return self.stage_bounds(n_stages)

    def grad_regions(self, stages) -> List[tuple]:
        """Flat-gradient index ranges that are final after each backward stage (stage 0: the
        heads and the last blocks, declared last in the store; the last stage: the first blocks
        and everything declared before them). `stages` as in stage_bounds. With Value or
        PointCloud sets and more than one stage, stage 0's region ends where tail_region()
        starts."""
        b = self.stage_bounds(stages)
        n_stages = len(b) - 1
        off = [self._block_offset(j) for j in b]
        tail = self.tail_region()
        top = tail[0] if tail is not None and n_stages > 1 else self.store.n
        regions = []
        for i in range(n_stages):
            hi = top if i == 0 else off[i]
            lo = 0 if i == n_stages - 1 else off[i + 1]
            regions.append((lo, hi))
        return regions

    def tail_region(self) -> Optional[tuple]:
        """The flat-gradient range of the value tokenizer's embedding and the point-cloud
        tokenizer's parameters (the tail tokenizers), None without Value and PointCloud sets:
        declared after the heads, but written by the token backward, so it is final only after
        the LAST stage (DDPStep all-reduces it there, beside that stage's own region)."""
        if self.value_tokenizer is not None:
            return self.value_tokenizer.embedding.offset, self.store.n
        if self.point_cloud_tokenizer is not None:
            return self.point_cloud_tokenizer.first_offset, self.store.n
        return None

    def backward_stage(self, st: Dict, stage: int, stages):
        """Stage `stage` of a backward split as stage_bounds(stages) (the heads run in stage 0,
        the stem / embeddings in the last): backward(st) == all stages in order.
        With frozen parameters (set_param_groups) the backward stops at the cut (_backward_cut):
        a stage that contains it clamps its lower block, a stage wholly below it launches
        nothing, and the gradients of everything below stay the zeros zero_grad wrote."""
        b = self.stage_bounds(stages)
        n_stages = len(b) - 1
        cut, tokens_frozen = self._cut
        if not self.stage_active(stage, b):
            if stage == n_stages - 1:
                st.pop("_dx", None)
                st.pop("_dz", None)
            return
        lo, hi = max(b[stage + 1], cut), b[stage]
        with wgrad_overlap(self.device):  # dW products beside the critical path; joined here
            if stage == 0:
                with phase("bwd/head"):
                    st["_dx"] = self._backward_head(st, need_dx=cut < self.cfg.num_blocks)
            dx = st["_dx"]
            if lo < hi:
                # floor: the stage's lowest block hands the dropout backward of the block below
                # to the next stage (st["_dz"]), so the stages launch what one backward launches
                # and give the same bits in deterministic mode
                with phase(f"bwd/blocks[{lo},{hi})"):
                    dx, st["_dz"] = self.stack.backward(dx, st["stack_sv"], st["ctxs"], lo=lo,
                                                        hi=hi, dz=st.pop("_dz", None), floor=cut)
            if stage == n_stages - 1:
                if cut == 0 and not tokens_frozen:
                    with phase("bwd/tokens+stem"):
                        self._backward_tokens(st, dx)
                st.pop("_dx", None)
                st.pop("_dz", None)
            else:
                st["_dx"] = dx
        if self.store.det_fx is not None:  # deterministic mode: this stage's final region
            self.store.det_flush(*self.grad_regions(stages)[stage])

    def backward(self, st: Dict):
        """Reverse schedule of compute_diffusion_denoise_loss / compute_l2_loss / compute_ce_loss;
        writes every parameter gradient into the flat gradient buffer (which must be zeroed
        before the forward); with frozen parameters, every gradient above the cut
        (backward_stage)."""
        self.backward_stage(st, 0, 1)

    def _backward_head(self, st: Dict, need_dx: bool = True):
        """The heads' parameter gradients; returns the gradient of the final sequence, or None
        with need_dx False (no block is trained: nothing reads it)."""
        B = st["B"]
        D = self.D
        kind = st.get("head_kind", "diffusion")
        if kind == "categorical":
            dg = self.categorical_head.loss_backward(st["head_sv"])
            if not need_dx:
                return None
            dxL = torch.empty(st["xL_shape"], dtype=torch.float32, device=dg.device)
            _C.call("mmt_rows_group_mean_bwd", _C.ptr(dg), B, self.L_final, D,
                    _C.ptr(self.readout_group), self.n_groups,
                    _C.ptr(self.readout_group_counts), _C.ptr(dxL), _C.stream_ptr())
        else:
            head = self.continuous_head if kind == "continuous" else self.head
            de = head.loss_backward(st["head_sv"])
            if kind == "diffusion" and self.pooling is not None:
                # readout_flag holds each readout row's slot index: the scatter writes all of dxL
                with phase("bwd/pool"):
                    if need_dx:
                        return self.pooling.backward(de, st["pool_sv"], self.readout_flag)
                    return self.pooling.backward(de, st["pool_sv"], self.readout_flag,
                                                 need_dx=False)
            if not need_dx:
                return None
            dxL = torch.empty(st["xL_shape"], dtype=torch.float32, device=de.device)
            _C.call("mmt_rows_mean_bwd", _C.ptr(de), de.stride(0), B, self.L_final, D,
                    _C.ptr(self.readout_flag), self.readout_rows.numel(), _C.ptr(dxL),
                    _C.stream_ptr())
        return dxL

    def _backward_tokens(self, st: Dict, dx0):
        B = st["B"]
        D = self.D
        NI, T = st["NI"], st["T"]
        dimg = torch.empty((B, NI, D), dtype=torch.bfloat16, device=dx0.device)
        dtxt = torch.empty((B, T, D), dtype=torch.bfloat16, device=dx0.device) if self.text_proj else None
        it = self.image_tokenizer
        pad = st.get("pad")
        if pad is not None:
            # pad masks: d(pos_embedding) from the full dx0 first (the position embedding IS used
            # in the masked rows), then those rows are zeroed, and only then does anything else
            # read dx0: no gradient reaches a tokenizer through a masked token
            K.colsum(dx0.view(B, self.L0 * D), self.pos_embed.grad.view(-1))
            K.pad_mask_rows_bwd(dx0, self.layer_sets[0][1], pad[0], pad[1], self.text_set)
        # token gradients (and the readout embedding's); the image row / column position
        # embedding gradients by token window (mmt_patch_embed_grad)
        _C.call("mmt_seq_assemble_bwd", B, self.L0, D, _C.ptr(self.row_src), _C.ptr(dx0),
                _C.ptr(dtxt), T, _C.ptr(dimg), NI, _C.ptr(st["rt"]), _C.ptr(st["ct"]),
                _C.ptr(self.img_rows), it.Q, None, None, _C.ptr(self.readout_pe.grad),
                _C.stream_ptr())
        if NI:
            _C.call("mmt_patch_embed_grad", B, self.L0, D, self.n_images, self.cfg.image_size[0],
                    self.cfg.patch_size, it.Q, _C.ptr(self.img_rows), _C.ptr(dx0),
                    _C.ptr(st["rt"]), _C.ptr(st["ct"]), _C.ptr(it.row_emb.grad),
                    _C.ptr(it.col_emb.grad), _C.stream_ptr())
        if pad is None:
            K.colsum(dx0.view(B, self.L0 * D), self.pos_embed.grad.view(-1))
        if self.value_tokenizer is not None:
            self.value_tokenizer.backward(dx0, st["val_tok"], self.value_rows)
        if self.point_cloud_tokenizer is not None:
            self.point_cloud_tokenizer.backward(dx0, st["pc_sv"], self.pc_rows)
        it.backward(dimg, st["img_sv"])
        if self.text_proj is not None:
            self.text_proj.bwd(dtxt.view(B * T, D), st["t5_out"].view(B * T, -1), need_dx=False)

    def num_params(self) -> int:
        return self.store.num_params()


# ---------------------------------------------------------------------- train state / step
@dataclass
class AdamW:
    """The reference takes an optax tx from its caller (octo.py:341); this is optax.adamw with
    these defaults (decoupled weight decay applied to every parameter, as optax without a mask,
    unless weight_decay_mask says otherwise).

    learning_rate: a float, or a schedule (schedules.Constant / WarmupCosine / WarmupRsqrt)
    evaluated on the device from the step counter. max_grad_norm: optax.clip_by_global_norm
    chained in front (None: off). skip_nonfinite: a step whose gradient has a non-finite norm
    leaves the parameters and both moments untouched. With a float learning rate and neither
    option the step is the plain mmt_adamw launch; otherwise the learning rate, the gradient norm
    and the clip factor live in device memory (OCTOTrainState.opt), so one captured graph serves
    the whole schedule.

    Parameter groups, optax.multi_transform({"trainable": optax.chain(clip_by_global_norm,
    adamw(schedule, mask=decay_mask)), "frozen": set_to_zero()}); both default to None, the
    behaviour above, launch for launch:
    weight_decay_mask: the parameters that ARE decayed, as fnmatch.fnmatchcase patterns against
    the full parameter name (one string or a sequence; a name itself is a pattern); the preset
    "kernels" = ("*/kernel",) is the Octo pre-training recipe (no decay on biases, norm scales,
    embeddings, fourier_kernel, learnt_q_input).
    frozen_keys: the parameters that are never updated (same pattern forms): their master, both
    shadows and both moments keep their bits, they do not enter the gradient norm, and the
    backward stops below the lowest block it still has to reach (Octo._backward_cut). The preset
    "head_only" freezes everything outside the action heads.
    The patterns are resolved in create_octo_train_state, where the model is known: one that
    matches no parameter, or freezing everything, is a ValueError.

    ema_decay: keep an exponential moving average of the parameters (ParamStore.ema), updated
    inside the AdamW launch (mmt_adamw_ema in place of whichever launch the options above select;
    the parameters, moments and shadows keep their bits). None (the default): off, the launches
    above. A float in [0, 1): a constant decay (optax.ema(decay, debias=False) over the
    parameters). A schedules.EmaDecay: the diffusers / Diffusion-Policy EMAModel warm-up, evaluated
    on the device from the step counter. A skipped step (skip_nonfinite) leaves the average as it
    is; frozen parameters' average stays equal to them. OCTOTrainState.ema_weights() evaluates
    with it."""
    learning_rate: Union[float, Constant, WarmupCosine, WarmupRsqrt] = 3e-4
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    weight_decay: float = 1e-4
    max_grad_norm: Optional[float] = None
    skip_nonfinite: bool = False
    weight_decay_mask: Union[None, str, tuple, list] = None
    frozen_keys: Union[None, str, tuple, list] = None
    ema_decay: Union[None, float, EmaDecay] = None

    def __post_init__(self):
        d = self.ema_decay
        if isinstance(d, bool) or not (d is None or isinstance(d, (int, float, EmaDecay))):
            raise TypeError(f"AdamW: ema_decay {d!r} is neither None, a float in [0, 1) nor a "
                            "schedules.EmaDecay")
        if isinstance(d, (int, float)) and not 0.0 <= d < 1.0:
            raise ValueError(f"AdamW: ema_decay {d} outside [0, 1)")
        for what in ("weight_decay_mask", "frozen_keys"):
            v = getattr(self, what)
            if not (v is None or isinstance(v, str) or (isinstance(v, (list, tuple))
                                                        and all(isinstance(x, str) for x in v))):
                raise ValueError(f"AdamW: {what} {v!r} is neither None, a preset / pattern string "
                                 "nor a sequence of pattern strings")
        if not isinstance(self.learning_rate, (int, float) + Schedule):
            raise TypeError(f"AdamW: learning_rate {self.learning_rate!r} is neither a number nor "
                            "a schedules.Constant / WarmupCosine / WarmupRsqrt")
        if self.max_grad_norm is not None and not self.max_grad_norm > 0:
            raise ValueError(f"AdamW: max_grad_norm {self.max_grad_norm} must be > 0 (None: off)")

    @property
    def device_control(self) -> bool:
        """The optimizer's scalars are computed on the device (mmt_optim_prepare)."""
        return (not isinstance(self.learning_rate, (int, float))
                or self.max_grad_norm is not None or self.skip_nonfinite)

    @property
    def grouped(self) -> bool:
        return self.weight_decay_mask is not None or self.frozen_keys is not None

    @property
    def schedule(self):
        lr = self.learning_rate
        return Constant(float(lr)) if isinstance(lr, (int, float)) else lr

    @property
    def ema_schedule(self):
        """None, or the decay as a schedules.ConstantEmaDecay / EmaDecay."""
        d = self.ema_decay
        return ConstantEmaDecay(float(d)) if isinstance(d, (int, float)) else d


class OCTOMetrics:
    """Reference octo.py:322-324 (``clu.metrics.Average.from_output("loss")``): running sum and
    count kept on the device, merged without a host sync (the reference's wandb.log forces one
    every step, :231-233). ``compute()`` is the average (a host read)."""

    def __init__(self, device):
        self.total = torch.zeros(1, dtype=torch.float64, device=device)
        self.count = torch.zeros(1, dtype=torch.float64, device=device)

    def merge(self, loss: torch.Tensor) -> "OCTOMetrics":
        """single_from_model_output(loss=loss) merged in place (Average.merge: sums add)."""
        self.total.add_(loss.detach().reshape(-1)[:1].double())
        self.count.add_(1.0)
        return self

    def compute(self) -> float:
        c = float(self.count.item())
        return float(self.total.item()) / c if c else float("nan")

    def reset(self):
        self.total.zero_()
        self.count.zero_()


@dataclass
class OCTOTrainState:
    """Reference octo.py:326-332: params (flat store), optimizer, rngs (device {seed, step}),
    step, metrics (running loss average, clu.metrics.Average equivalent)."""
    model: Octo
    tx: AdamW
    rng: torch.Tensor
    allreduce: Optional[Callable] = None        # DDP gradient all-reduce (distributed.py)
    sample_offset: int = 0
    metrics: Optional[OCTOMetrics] = None
    last_loss: Optional[torch.Tensor] = None    # loss of the latest step (device)
    # device-resident optimizer control (tx.device_control): the 8 fp32 words mmt_optim_prepare
    # writes (include/mmt_api.h: grad_norm, clip, gmul, lr, nonfinite, skipped, skip, 0) for
    # loggers that must not synchronise, and its workspace; None for the plain optimizer
    opt: Optional[torch.Tensor] = None
    opt_workspace: Optional[torch.Tensor] = None

    def __post_init__(self):
        if self.tx.device_control and self.opt is None:
            dev, n = self.model.device, self.model.store.flat.numel()
            self.opt = torch.zeros(_C.OPT_WORDS, dtype=torch.float32, device=dev)
            self.opt_workspace = torch.empty(_C.workspace_size(_C.WS_GRAD_NORM, n),
                                             dtype=torch.uint8, device=dev)
        self._sched_c = self.tx.schedule.to_c() if self.tx.device_control else None
        # parameter EMA (tx.ema_decay): the mmt_ema_decay_t the AdamW launch reads; the buffer
        # lives on the store (ParamStore.ema), so the latest state of a model decides it
        self._ema_c = self.tx.ema_schedule.to_c() if self.tx.ema_decay is not None else None
        self._ema_swapped = False  # inside ema_weights(): the master holds the EMA

    @property
    def params(self):
        return self.model.store.state_dict()

    def _ema_buffer(self) -> torch.Tensor:
        ema = self.model.store.ema if self._ema_c is not None else None
        if ema is None:
            raise AttributeError("the train state keeps no parameter EMA (AdamW.ema_decay is None, "
                                 "or a later state of this model dropped it)")
        return ema

    @property
    def ema_params(self) -> Dict[str, torch.Tensor]:
        """name -> fp32 view into the EMA buffer (the averaged weights; inside ema_weights() the
        buffer holds the raw iterate instead)."""
        self._ema_buffer()
        return self.model.store.ema_state_dict()

    @property
    def last_ema_decay(self) -> float:
        """The decay the latest step applied: the host restatement (schedules.EmaDecay.__call__)
        at the count before that step's advance. A host read of the step counter."""
        self._ema_buffer()
        return self.tx.ema_schedule(max(self.step - 1, 0))

    def ema_weights(self):
        """``with state.ema_weights(): ...`` evaluates with the averaged weights: mmt_ema_swap
        exchanges the master and the EMA in place and rewrites the bf16 shadow, then the
        transposed and e4m3 shadows are re-derived; the same again on exit. No buffer moves, so
        captured graphs stay valid, and every reader of the store (predict_diffusion_action, the
        losses with train=False, to_flax_params) sees the EMA inside the block. Frozen chunks
        are not touched (their EMA equals them). apply_gradients inside the block and a nested
        entry raise RuntimeError; a state without EMA raises AttributeError."""
        import contextlib
        self._ema_buffer()

        @contextlib.contextmanager
        def _cm():
            if self._ema_swapped:
                raise RuntimeError("ema_weights(): already inside the block")
            self._ema_swap()
            self._ema_swapped = True
            try:
                yield self
            finally:
                self._ema_swapped = False
                self._ema_swap()
        return _cm()

    def _ema_swap(self):
        s = self.model.store
        _C.call("mmt_ema_swap", _C.ptr(s.flat), _C.ptr(self._ema_buffer()), _C.ptr(s.flat_bf16),
                s.flat.numel(), _C.ptr(s.chunk_flags), GROUP_CHUNK, _C.stream_ptr())
        s.refresh_transposed()
        s.refresh_fp8()

    @property
    def step(self) -> int:
        return int(self.rng[1].item())

    @property
    def param_groups(self) -> Dict[str, Dict[str, bool]]:
        """name -> {"decay", "frozen"} as the optimizer applies them (AdamW.weight_decay_mask /
        frozen_keys resolved against the model)."""
        return self.model.store.param_groups()

    def _opt_word(self, i: int) -> float:
        if self.opt is None:
            raise AttributeError("the optimizer keeps no device-side state (plain AdamW: float "
                                 "learning rate, no clipping, no skip)")
        return float(self.opt[i].item())

    # host reads of `opt` (each synchronises with the device): the latest step's values
    @property
    def last_grad_norm(self) -> float:
        """Global norm of the averaged gradient before clipping, over the trainable parameters
        (frozen ones do not enter it: optax.multi_transform clips inside the trainable group)."""
        return self._opt_word(_C.OPT_GRAD_NORM)

    @property
    def last_lr(self) -> float:
        return self._opt_word(_C.OPT_LR)

    @property
    def last_clip(self) -> float:
        return self._opt_word(_C.OPT_CLIP)

    @property
    def skipped_steps(self) -> int:
        return int(self._opt_word(_C.OPT_SKIPPED))

    def apply_gradients(self):
        with phase("optimizer"):
            self._apply_gradients()

    def _apply_gradients(self):
        if self._ema_swapped:
            raise RuntimeError("apply_gradients inside ema_weights(): the master buffer holds "
                               "the EMA, not the iterate")
        s = self.model.store
        tx = self.tx
        grad_scale = getattr(self.allreduce, "grad_scale", 1.0)
        # parameter EMA: mmt_adamw_ema takes the place of whichever AdamW launch is chosen below
        ema = s.ema if self._ema_c is not None else None
        if s.chunk_flags is not None:
            # parameter groups: the grouped entry points, only when the store holds a flag table
            n = s.flat.numel()
            if self.opt is not None:
                _C.call("mmt_optim_prepare_groups", _C.ptr(s.flat_grad), n, grad_scale,
                        float(tx.max_grad_norm or 0.0), int(tx.skip_nonfinite),
                        ctypes.addressof(self._sched_c), _C.ptr(self.rng), _C.ptr(self.opt),
                        _C.ptr(self.opt_workspace), self.opt_workspace.numel(),
                        _C.ptr(s.chunk_flags), GROUP_CHUNK, _C.stream_ptr())
            lr = tx.learning_rate if self.opt is None else 0.0
            if ema is None:
                _C.call("mmt_adamw_groups", _C.ptr(s.flat), _C.ptr(s.flat_grad), _C.ptr(s.m),
                        _C.ptr(s.v), _C.ptr(s.flat_bf16), n, _C.ptr(self.rng), _C.ptr(self.opt),
                        lr, tx.b1, tx.b2, tx.eps, tx.weight_decay, grad_scale,
                        _C.ptr(s.chunk_flags), GROUP_CHUNK, _C.stream_ptr())
        elif self.opt is None:
            if ema is None:
                _C.call("mmt_adamw", _C.ptr(s.flat), _C.ptr(s.flat_grad), _C.ptr(s.m),
                        _C.ptr(s.v), _C.ptr(s.flat_bf16), s.flat.numel(), _C.ptr(self.rng),
                        tx.learning_rate, tx.b1, tx.b2, tx.eps, tx.weight_decay, grad_scale,
                        _C.stream_ptr())
        else:
            # after the all-reduce, so every rank reduces the same summed gradient to the same
            # bits. A skipped step (skip_nonfinite) still refreshes the shadows (a no-op on
            # unchanged weights) and advances the counter, which keys the random streams: unlike
            # optax.apply_if_finite, the bias-correction count includes skipped steps.
            n = s.flat.numel()
            _C.call("mmt_optim_prepare", _C.ptr(s.flat_grad), n, grad_scale,
                    float(tx.max_grad_norm or 0.0), int(tx.skip_nonfinite),
                    ctypes.addressof(self._sched_c), _C.ptr(self.rng), _C.ptr(self.opt),
                    _C.ptr(self.opt_workspace), self.opt_workspace.numel(), _C.stream_ptr())
            if ema is None:
                _C.call("mmt_adamw_dev", _C.ptr(s.flat), _C.ptr(s.flat_grad), _C.ptr(s.m),
                        _C.ptr(s.v), _C.ptr(s.flat_bf16), n, _C.ptr(self.rng), _C.ptr(self.opt),
                        tx.b1, tx.b2, tx.eps, tx.weight_decay, _C.stream_ptr())
        if ema is not None:
            lr = tx.learning_rate if self.opt is None else 0.0
            _C.call("mmt_adamw_ema", _C.ptr(s.flat), _C.ptr(s.flat_grad), _C.ptr(s.m), _C.ptr(s.v),
                    _C.ptr(s.flat_bf16), _C.ptr(ema), s.flat.numel(), _C.ptr(self.rng),
                    _C.ptr(self.opt), lr, tx.b1, tx.b2, tx.eps, tx.weight_decay, grad_scale,
                    _C.ptr(s.chunk_flags), GROUP_CHUNK, ctypes.addressof(self._ema_c),
                    _C.stream_ptr())
        s.refresh_transposed()
        s.refresh_fp8()
        _C.call("mmt_step_advance", _C.ptr(self.rng), _C.stream_ptr())


def create_octo_train_state(model: Octo, tx: AdamW | None = None, seed: int = 1234,
                            allreduce=None, sample_offset: int = 0) -> OCTOTrainState:
    """Reference octo.py:334-386 (parameters were initialised by Octo(...)). The optimizer's
    parameter groups are resolved here (Octo.set_param_groups: ValueError for a pattern that
    matches no parameter or a request that freezes everything); they live on the model's store,
    so the latest state created for a model decides them. The same holds for the parameter EMA
    (AdamW.ema_decay): allocated here as a copy of the master, dropped when tx has none."""
    tx = tx or AdamW()
    model.set_param_groups(tx.weight_decay_mask, tx.frozen_keys)
    model.store.set_ema(tx.ema_decay is not None)  # a copy of the master, or dropped
    rng = torch.tensor([seed, 0], dtype=torch.int32, device=model.device)
    return OCTOTrainState(model, tx, rng, allreduce, sample_offset,
                          metrics=OCTOMetrics(model.device))


def grads_tree(model: Octo) -> Dict[str, torch.Tensor]:
    """The step's gradients by parameter name (views into the flat fp32 gradient buffer, valid
    until the next step zeroes it) — the ``grads`` the reference's train steps return. With frozen
    parameters (AdamW.frozen_keys) the backward stops at the cut (Octo._backward_cut): gradients
    below it are exactly zero, zero_grad's value; a frozen parameter above the cut still shows its
    gradient, which the optimizer ignores."""
    return {p.name: p.grad for p in model.store.params}


def _train_step(loss_fn, model: Octo, train_state: OCTOTrainState, text_tokens, images, actions,
                **kw):
    """value_and_grad -> apply_gradients -> metrics merge (octo.py:216-239); returns
    (train_state, grads). The step's loss stays on the device: train_state.last_loss."""
    model.store.zero_grad()
    loss, st = loss_fn(text_tokens, images, actions, True, train_state.rng,
                       train_state.sample_offset, **kw)
    model.backward(st)
    if train_state.allreduce is not None:
        train_state.allreduce(model.store.flat_grad)
    train_state.apply_gradients()
    train_state.last_loss = loss
    if train_state.metrics is not None:
        train_state.metrics.merge(loss)
    return train_state, grads_tree(model)


def _step_kw(action_pad_mask, values, point_clouds=None, set_pad_mask=None,
             text_pad_mask=None, point_cloud_counts=None) -> dict:
    """The optional keywords of a loss, passed only when given."""
    kw = {} if action_pad_mask is None else {"action_pad_mask": action_pad_mask}
    if values is not None:
        kw["values"] = values
    if point_clouds is not None:
        kw["point_clouds"] = point_clouds
    if set_pad_mask is not None:
        kw["set_pad_mask"] = set_pad_mask
    if text_pad_mask is not None:
        kw["text_pad_mask"] = text_pad_mask
    if point_cloud_counts is not None:
        kw["point_cloud_counts"] = point_cloud_counts
    return kw


def continuous_train_step(model: Octo, train_state: OCTOTrainState, text_tokens, images, actions,
                          action_pad_mask=None, values=None, point_clouds=None,
                          set_pad_mask=None, text_pad_mask=None, point_cloud_counts=None):
    """Reference octo.py:242-280: value_and_grad of mean(compute_l2_loss), apply_gradients,
    metrics merge. Returns (train_state, grads). action_pad_mask, values: compute_l2_loss's;
    set_pad_mask, text_pad_mask, point_cloud_counts: generate_readouts'."""
    kw = _step_kw(action_pad_mask, values, point_clouds, set_pad_mask, text_pad_mask,
                  point_cloud_counts)
    return _train_step(model.compute_l2_loss, model, train_state, text_tokens, images, actions,
                       **kw)


def categorical_train_step(model: Octo, train_state: OCTOTrainState, text_tokens, images, actions,
                           action_pad_mask=None, values=None, point_clouds=None,
                           set_pad_mask=None, text_pad_mask=None, point_cloud_counts=None):
    """Reference octo.py:282-320: value_and_grad of mean(compute_ce_loss), apply_gradients,
    metrics merge. Returns (train_state, grads). action_pad_mask, values: compute_ce_loss's;
    set_pad_mask, text_pad_mask, point_cloud_counts: generate_readouts'."""
    kw = _step_kw(action_pad_mask, values, point_clouds, set_pad_mask, text_pad_mask,
                  point_cloud_counts)
    return _train_step(model.compute_ce_loss, model, train_state, text_tokens, images, actions,
                       **kw)


def diffusion_train_step(model: Octo, train_state: OCTOTrainState, text_tokens, images, actions,
                         inject: Optional[dict] = None, action_pad_mask=None, values=None,
                         point_clouds=None, set_pad_mask=None, text_pad_mask=None,
                         point_cloud_counts=None):
    """Reference octo.py:204-240: value_and_grad of the denoise loss, apply_gradients, metrics
    merge. Returns (train_state, grads) like the reference; grads are views of the flat gradient
    buffer by parameter name, the loss is train_state.last_loss (device) and the running average
    train_state.metrics. action_pad_mask, values: compute_diffusion_denoise_loss's;
    set_pad_mask, text_pad_mask, point_cloud_counts: generate_readouts'."""
    kw = _step_kw(action_pad_mask, values, point_clouds, set_pad_mask, text_pad_mask,
                  point_cloud_counts)
    return _train_step(model.compute_diffusion_denoise_loss, model, train_state, text_tokens,
                       images, actions, inject=inject, **kw)
