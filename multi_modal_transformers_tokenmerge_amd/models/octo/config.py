"""OCTO configurations.

The reference pins only ``model_configs/octo_base.yaml`` (D 768, 3 heads, 1 block, 280^2 images,
patch 56) and reads keys its YAMLs do not define. BASELINE names OCTO-tiny/small/base,
which the reference does not define; the sizes below are SURVEY §8.0's (upstream Octo ViT-t/s/b
widths with the reference architecture and quirks).
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Optional

from ...tokenizers.text.t5_base import T5Config


def _default_image_camera(input_sequence: str) -> list:
    """Per Image set of the sequence after the repeat expansion, as the sequencer parses it
    (TokenSequence, the parser the model itself uses): its ordinal among the Image sets of its
    observation block (the sets of one timestep)."""
    from ...tokenizers.token_sequencer import Image, TokenSequence
    out, seen = [], {}
    for ts in TokenSequence(input_sequence).token_sequence:
        if isinstance(ts, Image):
            out.append(seen.get(ts.timestep, 0))
            seen[ts.timestep] = out[-1] + 1
    return out


@dataclass
class OctoConfig:
    name: str = "octo-small"
    token_embedding_dim: int = 384
    num_heads: int = 6
    mlp_dim: int = 1536
    num_blocks: int = 12
    image_size: tuple = (256, 256, 3)
    patch_size: int = 16
    position_interval: int = 128
    input_sequence: str = "[TaskDescriptionPrefix{32}] [Image{256};Readout{4}]"
    token_compression_sequence: Optional[str] = None
    tokens_per_readout: int = 4
    num_observation_blocks: int = 1
    action_space_dim: int = 8
    diffusion_steps: int = 32
    # OctoDenoise num_blocks (diffusion.py:62-63): MLPBlocks applied in sequence, the first on
    # concatenate([noisy, time_emb, readout]), the others on the previous block's output
    denoise_blocks: int = 1
    # action heads built (octo.py:83-87 config.action_heads.heads); the bench path is diffusion only
    action_heads: tuple = ("diffusion",)
    num_bins: int = 256
    max_action: float = 5.0
    dropout_rate: float = 0.1
    attention_dropout_rate: float = 0.1
    layer_norm_eps: float = 1e-6
    t5: T5Config = field(default_factory=T5Config)
    text_tokens: int = 32
    # ResNetV2Block hyper-parameters (gato_resnet.yaml:41-104); None = the build defaults
    stem: Optional[dict] = None
    # fp8 weight path (BASELINE configs[4]): the encoder blocks' Dense forward products in e4m3 —
    # the QKV projection and MLP Dense_0 (activation-stationary fp8 kernel, 1.8x its bf16 twin);
    # fp8_residual also puts the residual-stream products (out-projection, MLP Dense_1, fp32
    # residual epilogue) in e4m3, measured slower than their bf16 kernels — off
    fp8: bool = False
    fp8_residual: bool = False
    # how token_compression_sequence's per-layer counts are realised: "tome" (bipartite soft
    # matching + merge_wavg, token_compression.py:54-129, per compressed set) or "prune"
    # (per-set top-k on the attention importance, compressed_attention.py:302-308 +
    # token_compression.py:15-46, every set); YAML key token_compression_method
    compression: str = "tome"
    # ToMe proportional attention (YAML key proportional_attention): from the second block on,
    # softmax(q.k * scale + log size[k]) with the token sizes the merges carry, so a merged token
    # votes as the patches it stands for (a per-key bias inside the attention kernels). Needs
    # compression == "tome" (pruning carries no sizes); a no-op without token_compression_sequence
    proportional_attention: bool = False
    # ToMe merge source (YAML key track_merge_source): every merge also composes its pos_map into
    # a per-set patch -> merged token map (one small launch per merged set and block, captured
    # with the step), read back with Octo.merge_source. Needs compression == "tome"; a no-op
    # without token_compression_sequence
    track_merge_source: bool = False
    # QK-norm (YAML key ...encoder_1d_block.self_attention.normalize_qk, flax.linen.SelfAttention's
    # own attribute): LayerNorm(use_bias=False) over the head dimension of the projected queries
    # and keys before the dot product, two (Dh,) scales per block (query_ln / key_ln); everything
    # that reads the keys (attention, the ToMe metric, the pruning importance) sees them
    # normalised. Head widths 32 / 64 / 128 / 256
    normalize_qk: bool = False
    # how the diffusion head turns the readout tokens into its conditioning vector (YAML key
    # readout_pooling): "mean" (the reference's live code path, diffusion.py:102) or "attention"
    # (MultiHeadAttentionPooling, attention.py:122-150, the call the reference left commented out,
    # diffusion.py:99): a learnt query attends to the readouts. pooling_heads: its head count
    # (None: num_heads); pooling_mlp_dim: its MLPBlock's hidden width (None: token_embedding_dim,
    # as in the reference's diffusion.yaml); pooling_norm_axes: its LayerNorm's reduction_axes,
    # [-1] (the features) or [1] (the reference YAML's value: on the length-1 pooled sequence the
    # norm then outputs its bias). The continuous and categorical heads keep their means.
    readout_pooling: str = "mean"
    pooling_heads: Optional[int] = None
    pooling_mlp_dim: Optional[int] = None
    pooling_norm_axes: tuple = (-1,)
    # action chunking (Octo / Diffusion Policy): the diffusion head denoises action_horizon
    # consecutive actions at once, so its width is action_space_dim * action_horizon (YAML key
    # action_heads.action_horizon). The continuous and categorical heads have a chunk length of
    # their own, pred_horizon (YAML key action_heads.pred_horizon, default 1: one action, the
    # reference's `seq=1` of continuous.py:24): the continuous Dense is D -> pred_horizon *
    # action_space_dim and the categorical head forms pred_horizon * action_space_dim readout
    # groups, step-major. With action_horizon > 1 beside one of these heads the two must agree
    # (one dataset chunk feeds every head); action_horizon = 1 with pred_horizon > 1 is allowed.
    action_horizon: int = 1
    pred_horizon: int = 1
    # the continuous head's regression loss (YAML key action_heads.continuous_loss): "mse" (the
    # reference's compute_l2_loss) or "l1" (upstream Octo's default)
    continuous_loss: str = "mse"
    # the diffusion head's default sampler: the fields of action_heads.diffusion.SamplerSpec as a
    # dict (YAML key action_heads.sampler), None = the reference's 32-step loop
    sampler: Optional[dict] = None
    # independent (t, eps) draws per sample in the diffusion loss, against one backbone forward
    # (upstream Octo's n_diffusion_samples; YAML key action_heads.n_diffusion_samples), 1 .. 64.
    # Above 1 the loss runs the fused multi-draw kernel (DiffusionActionHead.loss_forward_multi)
    n_diffusion_samples: int = 1
    # the value tokenizer behind the Value{n} sets of input_sequence (proprioception;
    # tokenizers/numeric_values/value_tokenizer.py; YAML key tokenizers.values.encoder): a dict
    # with any of num_bins (2 .. 4096, default 256), mu (> 0, default 255.0, the reference's) and
    # encoding ("mu_law", the default, or "uniform"). None with Value sets present: the defaults
    value_tokenizer: Optional[dict] = None
    # the point-cloud tokenizer behind the PointCloud{n} sets of input_sequence
    # (tokenizers/pointclouds/point_cloud_tokenizer.py; YAML key tokenizers.pointclouds.encoder):
    # a dict with num_points (P, the points of every cloud, n .. 4096; required) and any of
    # num_neighbours_knn (1 .. 32, default 16), point_features (C, 3 .. 8, default 3) and hidden
    # (the two LBR widths, each 32 / 64 / 128, default (64, 64)). Required with PointCloud sets
    point_cloud_tokenizer: Optional[dict] = None
    # image augmentation of the training losses (tokenizers/images/augment.py; YAML key
    # tokenizers.images.augmentation): a dict with `cameras`, a list of dicts with any of scale,
    # ratio, brightness, contrast, saturation (CameraAugmentation's fields), one per camera, and
    # optionally `image_camera`, the camera index of every Image set of input_sequence after the
    # repeat expansion (default: the Image sets of one observation block are cameras 0, 1, ...,
    # repeated across blocks, so a history window shares its camera's draw). uint8 images only;
    # applied by the compute_*_loss methods with train=True (hence the train steps and DDPStep),
    # never by the predict_* methods. None: off, no launch added
    image_augmentation: Optional[dict] = None

    def image_camera(self) -> list:
        """The camera index of every Image set of input_sequence after the repeat expansion:
        image_augmentation's `image_camera` if given, else 0, 1, ... within each observation
        block."""
        aug = self.image_augmentation or {}
        if aug.get("image_camera") is not None:
            return [int(c) for c in aug["image_camera"]]
        return _default_image_camera(self.input_sequence)

    def __post_init__(self):
        if self.image_augmentation is not None:
            from ...tokenizers.images.augment import ImageAugmentation
            aug = self.image_augmentation
            if not isinstance(aug, dict) or set(aug) - {"cameras", "image_camera"} or \
                    not isinstance(aug.get("cameras"), (list, tuple)) or not aug["cameras"]:
                raise ValueError("image_augmentation must be a dict with `cameras` (a non-empty "
                                 f"list) and optionally `image_camera`, got {aug!r}")
            explicit = aug.get("image_camera") is not None
            slots = _default_image_camera(self.input_sequence)
            if not slots:
                raise ValueError("image_augmentation is set but input_sequence has no Image set")
            if explicit:
                cams = list(aug["image_camera"])
                if len(cams) != len(slots):
                    raise ValueError(f"image_augmentation.image_camera names {len(cams)} image "
                                     f"sets, input_sequence has {len(slots)}")
            elif len(aug["cameras"]) != max(slots) + 1:
                raise ValueError(f"image_augmentation.cameras holds {len(aug['cameras'])} "
                                 f"cameras, an observation block of input_sequence has "
                                 f"{max(slots) + 1} Image sets (give image_camera to map them "
                                 "otherwise)")
            ia = ImageAugmentation(aug["cameras"], aug["image_camera"] if explicit else slots)
            if explicit and set(ia.image_camera) != set(range(ia.n_cam)):
                raise ValueError(f"image_augmentation.cameras holds {ia.n_cam} cameras, "
                                 f"image_camera uses {sorted(set(ia.image_camera))}")
        if self.point_cloud_tokenizer is not None:
            import re
            from ...tokenizers.pointclouds.point_cloud_tokenizer import (
                CONFIG_KEYS, check_point_cloud_config)
            pc = self.point_cloud_tokenizer
            if not isinstance(pc, dict) or set(pc) - set(CONFIG_KEYS) or "num_points" not in pc:
                raise ValueError("point_cloud_tokenizer must be a dict with num_points and keys "
                                 f"among {CONFIG_KEYS}, got {pc!r}")
            sizes = [int(v) for v in re.findall(r"PointCloud\s*\{(\d+)\}", self.input_sequence)]
            for n in sizes or [1]:
                check_point_cloud_config(pc["num_points"], n, pc.get("num_neighbours_knn", 16),
                                         pc.get("point_features", 3), pc.get("hidden", (64, 64)))
        if self.value_tokenizer is not None:
            from ...tokenizers.numeric_values.value_tokenizer import check_value_config
            vt = self.value_tokenizer
            if not isinstance(vt, dict) or set(vt) - {"num_bins", "mu", "encoding"}:
                raise ValueError("value_tokenizer must be a dict with keys among num_bins, mu, "
                                 f"encoding, got {vt!r}")
            check_value_config(vt.get("num_bins", 256), vt.get("mu", 255.0),
                               vt.get("encoding", "mu_law"))
        n = self.n_diffusion_samples
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 64:
            raise ValueError(f"n_diffusion_samples must be an integer in 1 .. 64, got {n!r}")
        if self.action_horizon < 1:
            raise ValueError(f"action_horizon must be >= 1, got {self.action_horizon}")
        ph = self.pred_horizon
        if isinstance(ph, bool) or not isinstance(ph, int) or ph < 1:
            raise ValueError(f"pred_horizon must be an integer >= 1, got {ph!r}")
        if self.continuous_loss not in ("mse", "l1"):
            raise ValueError(f"continuous_loss must be 'mse' or 'l1', got {self.continuous_loss!r}")
        if self.action_horizon > 1 and set(self.action_heads) - {"diffusion"} \
                and ph != self.action_horizon:
            raise ValueError("action_horizon > 1 is the diffusion head's: the continuous and "
                             "categorical heads predict pred_horizon actions, which must equal "
                             f"action_horizon {self.action_horizon} beside them, got pred_horizon "
                             f"{ph} with heads {self.action_heads}")
        if self.sampler is not None:
            from ...action_heads.diffusion import SamplerSpec
            SamplerSpec.of(self.sampler)     # ValueError on a bad spec
        if self.readout_pooling not in ("mean", "attention"):
            raise ValueError(f"readout_pooling must be 'mean' or 'attention', got "
                             f"{self.readout_pooling!r}")
        ph = self.pooling_heads if self.pooling_heads is not None else self.num_heads
        if (self.readout_pooling == "attention" or self.pooling_heads is not None) and \
                (ph < 1 or self.token_embedding_dim % ph):
            raise ValueError(f"pooling_heads {ph} must divide token_embedding_dim "
                             f"{self.token_embedding_dim}")
        if self.proportional_attention and self.compression != "tome":
            raise ValueError(f"proportional_attention needs compression='tome' (token sizes), got "
                             f"{self.compression!r}")
        if self.track_merge_source and self.compression != "tome":
            raise ValueError(f"track_merge_source needs compression='tome' (merge maps), got "
                             f"{self.compression!r}")

    @property
    def tome_r(self) -> int:
        if not self.token_compression_sequence or self.compression != "tome":
            return 0
        import re
        return max(int(x) for x in re.findall(r"\{(\d+)\}", self.token_compression_sequence))


TOME16 = "[TaskDescriptionPrefix{0}] [Image{16};Readout{0}]"

PRESETS = {
    # configs[0]: CPU plumbing case (no text, 64^2, 1 step)
    "octo-tiny": OctoConfig(name="octo-tiny", token_embedding_dim=192, num_heads=3, mlp_dim=768,
                            image_size=(64, 64, 3), input_sequence="[Image{16};Readout{4}]",
                            text_tokens=0),
    # configs[1]: small, ToMe off
    "octo-small": OctoConfig(),
    # configs[2]: small, ToMe r=16 per block (BASELINE metric config)
    "octo-small-tome16": OctoConfig(name="octo-small-tome16", token_compression_sequence=TOME16),
    # configs[2] with proportional attention (log token size on the keys from block 1 on)
    "octo-small-tome16-prop": OctoConfig(name="octo-small-tome16-prop",
                                         token_compression_sequence=TOME16,
                                         proportional_attention=True),
    # configs[2] with QK-norm (per-head LayerNorm of q and k, the ViT-22B recipe)
    "octo-small-tome16-qknorm": OctoConfig(name="octo-small-tome16-qknorm",
                                           token_compression_sequence=TOME16, normalize_qk=True),
    # configs[3]: base, 2 cameras, 2-step history
    "octo-base-2cam": OctoConfig(
        name="octo-base-2cam", token_embedding_dim=768, num_heads=12, mlp_dim=3072,
        input_sequence="[TaskDescriptionPrefix{32}] [Image{256};Image{256};Readout{4}]*2",
        num_observation_blocks=2),
    # configs[3] with ToMe on every image set: two cameras x two steps, r = 16 per set and block
    # (one bipartite match + merge per set, token_sequencer.py:222-238 per-set counts)
    "octo-base-2cam-tome16": OctoConfig(
        name="octo-base-2cam-tome16", token_embedding_dim=768, num_heads=12, mlp_dim=3072,
        input_sequence="[TaskDescriptionPrefix{32}] [Image{256};Image{256};Readout{4}]*2",
        token_compression_sequence="[TaskDescriptionPrefix{0}] [Image{16};Image{16};Readout{0}]*2",
        num_observation_blocks=2),
    # configs[4]: base hi-res 512^2, ToMe r=32, fp8 weight path
    "octo-base-hires-tome32": OctoConfig(
        name="octo-base-hires-tome32", token_embedding_dim=768, num_heads=12, mlp_dim=3072,
        image_size=(512, 512, 3), input_sequence="[TaskDescriptionPrefix{32}] [Image{1024};Readout{4}]",
        token_compression_sequence="[TaskDescriptionPrefix{0}] [Image{32};Readout{0}]", fp8=True),
    # configs[2] with the readouts pooled by attention (6 heads, feature-axis LayerNorm)
    "octo-small-tome16-map": OctoConfig(name="octo-small-tome16-map",
                                        token_compression_sequence=TOME16,
                                        readout_pooling="attention", pooling_heads=6),
    # top-k pruning on the small geometry: 16 image tokens per block
    "octo-small-prune16": OctoConfig(name="octo-small-prune16", token_compression_sequence=TOME16,
                                     compression="prune"),
    # configs[2] trained with Octo's primary-camera augmentation on its one camera: random resized
    # crop (area 0.8 .. 1, aspect 0.9 .. 1.1), brightness 0.1, contrast and saturation 0.9 .. 1.1
    "octo-small-tome16-aug": OctoConfig(
        name="octo-small-tome16-aug", token_compression_sequence=TOME16,
        image_augmentation=dict(cameras=[dict(scale=(0.8, 1.0), ratio=(0.9, 1.1), brightness=0.1,
                                              contrast=(0.9, 1.1), saturation=(0.9, 1.1))])),
    # configs[2] with 8 proprioception values per observation (Value tokens, never compressed)
    "octo-small-tome16-proprio8": OctoConfig(
        name="octo-small-tome16-proprio8",
        input_sequence="[TaskDescriptionPrefix{32}] [Image{256};Value{8};Readout{4}]",
        token_compression_sequence="[TaskDescriptionPrefix{0}] [Image{16};Value{0};Readout{0}]",
        value_tokenizer=dict(num_bins=256, mu=255.0, encoding="mu_law")),
    # configs[2] with one depth-camera cloud of 1024 points per observation as 64 point-cloud
    # tokens (farthest-point sampling + 16-NN grouping, never compressed)
    "octo-small-tome16-pc64": OctoConfig(
        name="octo-small-tome16-pc64",
        input_sequence="[TaskDescriptionPrefix{32}] [Image{256};PointCloud{64};Readout{4}]",
        token_compression_sequence="[TaskDescriptionPrefix{0}] [Image{16};PointCloud{0};Readout{0}]",
        point_cloud_tokenizer=dict(num_points=1024, num_neighbours_knn=16, point_features=3,
                                   hidden=(64, 64))),
}


def get_config(name: str, **overrides) -> OctoConfig:
    """A preset by name ("octo-small-tome16"), or a YAML config of the reference schema from
    model_configs/ ("octo_small_tome16", "ref_octo_base", or a path ending in .yaml)."""
    if name not in PRESETS:
        from ...config_loader import CONFIG_DIR, load_octo_config
        from pathlib import Path
        p = Path(name)
        if name.endswith(".yaml") and p.exists():
            return replace(load_octo_config(p.name, p.parent), **overrides)
        if (CONFIG_DIR / f"{name}.yaml").exists():
            return replace(load_octo_config(name), **overrides)
        raise KeyError(f"unknown config {name!r}; known: {sorted(PRESETS)} or "
                       f"model_configs/*.yaml")
    return replace(PRESETS[name], **overrides)
