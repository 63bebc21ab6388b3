"""DDPM action head, mirroring the reference's ``multi_modal_transformers/action_heads/diffusion.py``:
``cosine_beta_schedule`` (:17-27), ``FourierFeatures`` (:30-51), ``OctoDenoise`` (:53-65) and
``DiffusionActionHead`` (:68-209: ``denoise_loss`` :110-143, ``predict_denoise_term`` :88-107,
``predict_action`` :146-209).

Training path on MI355X: one fused kernel draws (t, eps), noises the actions and emits the Fourier
features straight into the denoiser's concatenated input buffer; the time-encoder MLP writes its
output into that same buffer (GEMM with a column-offset output), the readout mean is written into
its last columns, so ``concatenate([noisy, time_emb, readout])`` (:61) never materialises
separately. MLPBlocks here run with dropout disabled, as in the reference (they are called without
``train``, attention.py:29 default False).

With ``n_diffusion_samples`` > 1 or a pad mask the loss takes another route (``loss_forward_multi``):
the first Dense is split along its input as in the sampler, the time encoder runs once per
diffusion step and the readout product once per sample, and one fused kernel
(``mmt_diffusion_loss_multi``) handles all K draws of a sample; the backward is the split Dense's
(``_loss_backward_multi``).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from .. import _C, _kernels as K
from ..layers import Dense, split_k_for
from ..module_api import Bindable, init_from_spec, sget, spec
from ..params import ParamStore

K_ = K   # the kernels module where a method's K is the number of diffusion draws
_REF = "multi_modal_transformers."
_REF_MLP = _REF + "attention_blocks.attention.MLPBlock"
_REF_DENOISE = _REF + "action_heads.diffusion.OctoDenoise"
_REF_FOURIER = _REF + "action_heads.diffusion.FourierFeatures"


def cosine_beta_schedule(timesteps: int, s: float = 0.008) -> np.ndarray:
    """Reference :17-27 (float32 like jnp)."""
    steps = timesteps + 1
    t = (np.linspace(0, timesteps, steps, dtype=np.float32) / np.float32(timesteps)).astype(np.float32)
    ac = np.cos((t + np.float32(s)) / np.float32(1 + s) * np.float32(np.pi) * np.float32(0.5)) ** 2
    ac = (ac / ac[0]).astype(np.float32)
    betas = (1 - (ac[1:] / ac[:-1])).astype(np.float32)
    return np.clip(betas, 0, 0.999).astype(np.float32)


def _pooling_module(node):
    """The attention_pooling config node (a raw ``_target_`` dict, its LayerSpec, or a built
    module) as a MultiHeadAttentionPooling."""
    from ..attention_blocks.attention import MultiHeadAttentionPooling
    node = spec(node)
    if isinstance(node, MultiHeadAttentionPooling):
        return node
    kw = node.kwargs if hasattr(node, "kwargs") else {k: v for k, v in dict(node).items()
                                                       if not k.startswith("_")}
    return MultiHeadAttentionPooling(**kw)


def alpha_hats_of(betas: np.ndarray) -> np.ndarray:
    """Reference :84-86: prod(alphas[:i+1]) for each i (float32)."""
    alphas = (1 - betas).astype(np.float32)
    return np.array([np.prod(alphas[: i + 1], dtype=np.float32) for i in range(len(betas))],
                    dtype=np.float32)


@dataclasses.dataclass(frozen=True)
class SamplerSpec:
    """How predict_action turns noise into actions. Every kind is a table of affine updates
    x <- clip(a_k x + b_k eps_hat(x, t_k) + c_k n_k, -clip, clip) (DiffusionActionHead.sampler_table):
    kind "ddpm": the S ancestral steps t = S-1 .. 0; "ddim": `steps` deterministic (eta = 0) steps
    spread evenly over S-1 .. 0. noise "frozen": every step reuses the initial sample z as its
    noise (the reference's scan never splits its keys, diffusion.py:178); "fresh": a new draw per
    step. final_noise: whether the t = 0 row adds noise (default: True for frozen, as the
    reference does, False for fresh). The default spec is the reference's sampler."""
    kind: str = "ddpm"
    steps: int | None = None
    noise: str = "frozen"
    clip: float = 5.0
    final_noise: bool | None = None

    def __post_init__(self):
        if self.kind not in ("ddpm", "ddim"):
            raise ValueError(f"sampler kind must be 'ddpm' or 'ddim', got {self.kind!r}")
        if self.noise not in ("frozen", "fresh"):
            raise ValueError(f"sampler noise must be 'frozen' or 'fresh', got {self.noise!r}")
        if self.steps is not None and (isinstance(self.steps, bool) or int(self.steps) != self.steps
                                       or self.steps < 1):
            raise ValueError(f"sampler steps must be a positive integer, got {self.steps!r}")
        if not (isinstance(self.clip, (int, float)) and self.clip > 0):   # NaN fails too
            raise ValueError(f"sampler clip must be positive, got {self.clip!r}")
        if self.kind == "ddim" and (self.noise == "fresh" or self.final_noise):
            raise ValueError("the DDIM sampler is deterministic (eta = 0): it takes no step noise")

    @property
    def fresh(self) -> bool:
        return self.noise == "fresh"

    @property
    def adds_final_noise(self) -> bool:
        return (not self.fresh) if self.final_noise is None else bool(self.final_noise)

    def is_reference(self, diffusion_steps: int) -> bool:
        """The reference's own sampler: what mmt_diffusion_sample runs."""
        return (self.kind == "ddpm" and self.steps in (None, diffusion_steps) and not self.fresh
                and float(self.clip) == 5.0 and self.adds_final_noise)

    @classmethod
    def of(cls, node) -> "SamplerSpec":
        """A SamplerSpec from None (the default), a spec or a mapping of its fields."""
        if node is None:
            return cls()
        if isinstance(node, cls):
            return node
        try:
            return cls(**dict(node))
        except TypeError as e:
            raise ValueError(f"bad sampler spec {node!r}: {e}") from None


class DiffusionActionHead(Bindable):
    """Reference :68-209: ``DiffusionActionHead(diffusion_steps, attention_pooling,
    denoising_model, rng_collection="diffusion")`` with the model_configs/action_heads/diffusion.yaml
    nodes: ``denoising_model`` = OctoDenoise(time_encoder = FourierFeatures(output_dim, kernel_init,
    mlp_block), num_blocks, mlp_block) (:30-65). ``readout_pooling="mean"`` (the default):
    ``attention_pooling`` is accepted and unused, as in the reference (the pooling call is
    commented out, :99-102: the readouts are averaged). ``readout_pooling="attention"`` builds the
    MultiHeadAttentionPooling module (attention_blocks/attention.py) from that node and pools the
    readouts through it, the call the reference left commented out (:99); its parameters are
    declared after the denoiser's, and its backward is the module's own ``backward`` (the model
    calls it with what ``loss_backward`` returns).
    ``denoise_loss(readouts, actions)``, ``predict_denoise_term(readouts, time, noisy_actions)`` and
    ``predict_action(readouts)`` take the readout tokens (B, n, D) like the reference; the Octo
    training path feeds the readout MEAN straight from the backbone's fused rows-mean kernel
    (``loss_forward`` / ``*_mean``)."""

    def __init__(self, diffusion_steps: int = 32, attention_pooling=None, denoising_model=None,
                 rng_collection: str = "diffusion", *, readout_pooling: str = "mean",
                 sampler=None, n_diffusion_samples: int = 1):
        self.steps = int(diffusion_steps)
        if isinstance(n_diffusion_samples, bool) or int(n_diffusion_samples) != n_diffusion_samples \
                or not 1 <= n_diffusion_samples <= 64:
            raise ValueError("n_diffusion_samples must be an integer in 1 .. 64, got "
                             f"{n_diffusion_samples!r}")
        self.n_diffusion_samples = int(n_diffusion_samples)   # (t, eps) draws per sample in the loss
        self.sampler = SamplerSpec.of(sampler)   # predict_action's default (a spec or a dict)
        self.rng_collection = rng_collection
        self.attention_pooling = attention_pooling
        if readout_pooling not in ("mean", "attention"):
            raise ValueError(f"readout_pooling must be 'mean' or 'attention', got {readout_pooling!r}")
        self.readout_pooling = readout_pooling
        self.pooling = None
        if readout_pooling == "attention":
            if attention_pooling is None:
                raise ValueError("readout_pooling='attention' needs the attention_pooling node")
            self.pooling = _pooling_module(attention_pooling)
        dm = spec(denoising_model)
        te = spec(sget(dm, "time_encoder"))
        self.num_blocks = int(sget(dm, "num_blocks", 1))
        if self.num_blocks < 1:
            raise ValueError("OctoDenoise num_blocks must be >= 1")
        mlp = spec(sget(dm, "mlp_block"))
        self.time_dim_cfg = sget(te, "output_dim")
        self.fourier_init = sget(te, "kernel_init")
        tm = spec(sget(te, "mlp_block"))
        self.time_mlp_cfg = (sget(getattr(tm, "dense_spec", None), "features"),
                             sget(getattr(tm, "dense_out_spec", None), "features"))
        self.hidden_cfg = sget(getattr(mlp, "dense_spec", None), "features")
        self.A = int(sget(getattr(mlp, "dense_out_spec", None), "features", 8))
        betas = cosine_beta_schedule(self.steps)
        self.betas_np = betas
        self.alpha_hats_np = alpha_hats_of(betas)
        self._dev_consts = {}

    @classmethod
    def create(cls, store: ParamStore, name: str, embedding_dim: int, action_dim: int = 8,
               diffusion_steps: int = 32, time_dim: int | None = None,
               hidden: int | None = None, num_blocks: int = 1,
               sampler=None, n_diffusion_samples: int = 1) -> "DiffusionActionHead":
        """The head from its dimensions, declared in ``store`` (the Octo model's path)."""
        D = embedding_dim
        T = time_dim or D

        def mlp(h, o):
            return {"_target_": _REF_MLP, "dense": {"_target_": "flax.linen.Dense", "features": h},
                    "dense_out": {"_target_": "flax.linen.Dense", "features": o}}
        dm = {"_target_": _REF_DENOISE, "num_blocks": num_blocks,
              "time_encoder": {"_target_": _REF_FOURIER, "output_dim": T, "mlp_block": mlp(T, T)},
              "mlp_block": mlp(hidden or D, action_dim)}
        return cls(diffusion_steps, None, dm, sampler=sampler,
                   n_diffusion_samples=n_diffusion_samples).bind(store, name, D)

    def _declare(self, store: ParamStore, name: str, embedding_dim: int):
        D = embedding_dim
        self.D = D
        T0 = int(self.time_dim_cfg or D)
        self.F = T0 // 2
        T = 2 * self.F
        t_h, t_o = self.time_mlp_cfg
        if (t_h is not None and int(t_h) != T) or (t_o is not None and int(t_o) != T):
            raise NotImplementedError("FourierFeatures' MLPBlock must keep the output_dim width")
        self.time_dim = T
        self.hidden = int(self.hidden_cfg or D)
        p = f"{name}/OctoDenoise_0"
        self.fourier = store.add(f"{p}/FourierFeatures_0/fourier_kernel", (self.F, 1),
                                 init_from_spec(self.fourier_init, (self.F, 1)))
        self.t1 = Dense(store, f"{p}/FourierFeatures_0/MLPBlock_0/Dense_0", T, T)
        self.t2 = Dense(store, f"{p}/FourierFeatures_0/MLPBlock_0/Dense_1", T, T)
        self.cat_dim = self.A + T + D
        self.d1 = Dense(store, f"{p}/MLPBlock_0/Dense_0", self.cat_dim, self.hidden)
        self.d2 = Dense(store, f"{p}/MLPBlock_0/Dense_1", self.hidden, self.A)
        if self.cat_dim % 8:
            raise ValueError("action_dim + time_dim + D must be a multiple of 8 (16-B rows)")
        # OctoDenoise blocks 1.. (diffusion.py:62-63: a fresh MLPBlock per iteration, Flax names
        # MLPBlock_{i}) on the previous block's (B, A) output
        self.extra = [(Dense(store, f"{p}/MLPBlock_{i}/Dense_0", self.A, self.hidden),
                       Dense(store, f"{p}/MLPBlock_{i}/Dense_1", self.hidden, self.A))
                      for i in range(1, self.num_blocks)]
        if self.extra and self.A % 8:
            raise ValueError("OctoDenoise num_blocks > 1 needs action_dim % 8 == 0 (16-B rows)")
        if self.n_diffusion_samples > 1:
            self._check_multi(self.n_diffusion_samples)
        if self.pooling is not None and not self.pooling.bound:
            # after the denoiser: the offsets of everything above do not depend on the option (the
            # Octo model binds its module itself, after every head: attach_pooling)
            self.pooling.bind(store, f"{name}/MultiHeadAttentionPooling_0", D)

    def attach_pooling(self, module) -> "DiffusionActionHead":
        """Pool the readouts through ``module``, a MultiHeadAttentionPooling already bound to the
        head's store (the Octo model declares it after its last head, so the parameter offsets of
        a default configuration do not depend on the option)."""
        if not module.bound or module.D != self.D:
            raise ValueError(f"attach_pooling: the module must be bound at width {self.D}")
        self.pooling, self.readout_pooling = module, "attention"
        return self

    # ------------------------------------------------------------- reference-signature methods
    def _mean_into(self, readouts: torch.Tensor, out: torch.Tensor):
        """The readouts (B, n, D) pooled into a (B, D) bf16 view: their mean over the readout axis
        (:102), or with readout_pooling="attention" the pooling module's output (:99)."""
        if readouts.dim() != 3 or readouts.stride(2) != 1:
            raise ValueError(f"readouts must be (batch, tokens, {self.D}) with unit inner stride")
        B, n, D = readouts.shape
        x = readouts if readouts.dtype == torch.float32 else readouts.float()
        rows = torch.arange(n, dtype=torch.int32, device=readouts.device)
        if self.pooling is not None:
            return self.pooling.forward(x, rows, out=out)[0]
        _C.call("mmt_rows_mean_fwd", _C.ptr(x), x.stride(0), x.stride(1), B, D, _C.ptr(rows), n,
                _C.ptr(out), out.stride(0), _C.stream_ptr())
        return out

    def denoise_loss(self, readouts: torch.Tensor, actions: torch.Tensor, train: bool = True, *,
                     rng=None, sample_offset: int = 0, pad_mask=None) -> torch.Tensor:
        """Reference :110-143: t ~ U{0..steps-1}, eps ~ N(0, 1) from the 'diffusion' counter
        stream (rng, keyed by the global sample index), noisy = sqrt(abar) a + sqrt(1 - abar) eps,
        loss = mean_b sum_a 0.5 (pred - eps)^2. Returns the loss (1,) fp32 on the device.
        With n_diffusion_samples > 1 the loss averages that many independent (t, eps) draws per
        sample, and with pad_mask (B, A) bool only its components enter it, normalised by their
        number (loss_forward_multi); without either, the single-draw launches run unchanged."""
        self._ensure(readouts.device, int(readouts.shape[-1]))
        if rng is None:
            raise ValueError("denoise_loss needs the diffusion rng (rng=)")
        B = readouts.shape[0]
        if tuple(actions.shape) != (B, self.A):
            raise ValueError(f"actions must be ({B}, {self.A})")
        if self.n_diffusion_samples > 1 or pad_mask is not None:
            self._check_multi(self.n_diffusion_samples)
            e = torch.empty((B, self.D), dtype=torch.bfloat16, device=readouts.device)
            return self.loss_forward_multi(self._mean_into(readouts, e), actions.float().contiguous(),
                                           rng, sample_offset, self.n_diffusion_samples, pad_mask,
                                           backward=False)[0]
        cat = self.new_cat(B, readouts.device)
        self._mean_into(readouts, self.readout_slot(cat))
        loss, _ = self.loss_forward(cat, actions.float().contiguous(), rng, sample_offset)
        return loss

    def predict_denoise_term(self, readouts: torch.Tensor, time: torch.Tensor,
                             noisy_actions: torch.Tensor, train: bool = True) -> torch.Tensor:
        """Reference :88-107: OctoDenoise(noisy, time, mean(readouts)) -> (B, A) fp32."""
        self._ensure(readouts.device, int(readouts.shape[-1]))
        e = torch.empty((readouts.shape[0], self.D), dtype=torch.bfloat16, device=readouts.device)
        return self.predict_denoise_term_mean(self._mean_into(readouts, e), time,
                                              noisy_actions.float().contiguous())

    def predict_action(self, readouts: torch.Tensor, train: bool = True, *, rng=None,
                       sample_offset: int = 0, z: torch.Tensor | None = None,
                       return_noise: bool = False, sampler=None,
                       noise: torch.Tensor | None = None):
        """Reference :146-209: the sampler from the readouts (B, n, D); by default the reference's
        32-step DDPM loop, else what `sampler` / `noise` ask for (predict_action_mean)."""
        self._ensure(readouts.device, int(readouts.shape[-1]))
        e = torch.empty((readouts.shape[0], self.D), dtype=torch.bfloat16, device=readouts.device)
        return self.predict_action_mean(self._mean_into(readouts, e), rng, sample_offset, z,
                                        return_noise, sampler=sampler, noise=noise)

    def consts(self, device):
        if device not in self._dev_consts:
            self._dev_consts[device] = torch.from_numpy(self.alpha_hats_np).to(device)
        return self._dev_consts[device]

    def new_cat(self, B, device):
        return torch.empty((B, self.cat_dim), dtype=torch.bfloat16, device=device)

    def readout_slot(self, cat: torch.Tensor) -> torch.Tensor:
        return cat[:, self.A + self.time_dim:]

    # ------------------------------------------------------------------------- denoise_loss
    def loss_forward(self, cat: torch.Tensor, actions: torch.Tensor, rng, sample_offset: int = 0,
                     t_in=None, eps_in=None):
        """cat: (B, A+T+D) bf16 whose readout slot is already filled. Returns (loss (1,) fp32,
        saved). Mirrors denoise_loss (:110-143)."""
        B = cat.shape[0]
        dev = cat.device
        t = torch.empty(B, dtype=torch.int32, device=dev)
        eps = torch.empty((B, self.A), dtype=torch.float32, device=dev)
        feats = torch.empty((B, self.time_dim), dtype=torch.bfloat16, device=dev)
        _C.call("mmt_diffusion_prep", _C.ptr(rng), B, self.A, self.steps, sample_offset,
                _C.ptr(actions), _C.ptr(self.consts(dev)), _C.ptr(self.fourier.data), self.F,
                _C.ptr(t_in), _C.ptr(eps_in), _C.ptr(t), _C.ptr(eps), _C.ptr(cat), cat.stride(0),
                _C.ptr(feats), _C.stream_ptr())
        ht = self.t1.fwd(feats, act=K.ACT_RELU)
        self.t2.fwd(ht, out=cat[:, self.A:self.A + self.time_dim])
        hd = self.d1.fwd(cat, act=K.ACT_RELU)
        pred = self.d2.fwd(hd, out_mode=K.OUT_F32)
        pred, chain = self._extra_fwd(pred)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dpred = torch.empty((B, self.A), dtype=torch.bfloat16, device=dev)
        _C.call("mmt_diffusion_loss", _C.ptr(pred), pred.stride(0), _C.ptr(eps), B, self.A, 1.0,
                _C.ptr(loss), _C.ptr(dpred), _C.stream_ptr())
        return loss, dict(cat=cat, feats=feats, ht=ht, hd=hd, dpred=dpred, t=t, eps=eps, pred=pred,
                          chain=chain)

    def _extra_fwd(self, pred):
        """OctoDenoise blocks 1.. on the block-0 output pred (B, A) fp32: each input cast to bf16
        (the GEMM operand), Dense -> relu -> Dense. Returns (final pred, [(x, h) per block])."""
        chain = []
        for d1, d2 in self.extra:
            x = K.cast_f32_bf16(pred, torch.empty(pred.shape, dtype=torch.bfloat16, device=pred.device))
            h = d1.fwd(x, act=K.ACT_RELU)
            pred = d2.fwd(h, out_mode=K.OUT_F32)
            chain.append((x, h))
        return pred, chain

    # ------------------------------------------------------- multi-draw / masked denoise_loss
    def _check_multi(self, K: int = 1):
        """The fused loss (mmt_diffusion_loss_multi) holds one MLPBlock at the fused sampler's
        widths."""
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= 64:
            raise ValueError(f"n_diffusion_samples must be an integer in 1 .. 64, got {K!r}")
        if self.extra:
            raise ValueError("n_diffusion_samples > 1 and pad_mask need OctoDenoise num_blocks == 1 "
                             "(the fused loss holds one MLPBlock, as the fused sampler does)")
        self._check_fused_widths("fused loss")

    def _check_fused_widths(self, what: str, action: bool = True, hidden: bool = True):
        """The widths of the fused kernels (csrc/denoiser_wave.h): A in 8, 16 .. 64 (`action`;
        the loop sampler's draws need that too) and H a multiple of 8 up to 1024 (`hidden`)."""
        if action and (self.A % 8 or not 8 <= self.A <= 64):
            raise ValueError(f"the {what} needs an action width in 8, 16 .. 64, got {self.A}")
        if hidden and (self.hidden % 8 or self.hidden > 1024):
            raise ValueError(f"the {what} needs a hidden width that is a multiple of 8, at "
                             f"most 1024, got {self.hidden}")

    def _check_pooled(self, e: torch.Tensor, name: str):
        """The pooled readout of the fused loss and the samplers."""
        if e.dim() != 2 or e.shape[1] != self.D or e.dtype != torch.bfloat16 or e.stride(1) != 1:
            raise ValueError(f"{name} must be bf16 (B, {self.D}) with unit inner stride")

    def loss_forward_multi(self, e: torch.Tensor, actions: torch.Tensor, rng, sample_offset: int = 0,
                           K: int = 1, pad_mask=None, t_in=None, eps_in=None, backward: bool = True):
        """denoise_loss (:110-143) with K independent (t, eps) draws per sample against one pooled
        readout e (B, D) bf16, and a pad mask (B, A) (bool / uint8: components that count). The
        first Dense is split as in the sampler (_split_first_dense): the time encoder runs once
        per diffusion step and the readout product once per sample whatever K is; one fused kernel
        (mmt_diffusion_loss_multi) draws, noises, runs the MLPBlock in fp32 and emits the loss and
        the backward's bf16 operands. t_in (K, B) int32 / eps_in (K, B, A) fp32 inject the draws.
        backward=False: forward only (evaluation). Returns (loss (1,) fp32, saved)."""
        self._check_multi(K)
        B, A, H, S, dev = e.shape[0], self.A, self.hidden, self.steps, e.device
        self._check_pooled(e, "the pooled readout")
        if tuple(actions.shape) != (B, A) or actions.dtype != torch.float32 \
                or not actions.is_contiguous():
            raise ValueError(f"actions must be contiguous fp32 ({B}, {A})")
        if pad_mask is not None:
            if tuple(pad_mask.shape) != (B, A) or pad_mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"pad_mask must be bool or uint8 ({B}, {A})")
            pad_mask = pad_mask.to(torch.uint8).contiguous()
        if (t_in is None) != (eps_in is None):
            raise ValueError("inject t and eps together")
        if t_in is not None:
            if tuple(t_in.shape) != (K, B) or t_in.dtype != torch.int32 or not t_in.is_contiguous():
                raise ValueError(f"injected t must be contiguous int32 ({K}, {B})")
            if tuple(eps_in.shape) != (K, B, A) or eps_in.dtype != torch.float32 \
                    or not eps_in.is_contiguous():
                raise ValueError(f"injected eps must be contiguous fp32 ({K}, {B}, {A})")
        elif rng is None:
            raise ValueError("need the diffusion rng (or injected t and eps)")
        saved = self._time_embeddings_saved(dev)
        temb, feats, ht, t_all = saved
        P, Q = self._split_first_dense(e, saved)
        w1 = self.d1.w.bf16
        bf = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=dev) if backward else None
        t = torch.empty((K, B), dtype=torch.int32, device=dev)
        eps = torch.empty((K, B, A), dtype=torch.float32, device=dev)
        noisy, h, dh, dpred, dP = bf(K * B, A), bf(K * B, H), bf(K * B, H), bf(K * B, A), bf(B, H)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        scratch = torch.empty(B + 1, dtype=torch.float32, device=dev)
        _C.call("mmt_diffusion_loss_multi", _C.ptr(rng), B, A, K, S, H, sample_offset,
                _C.ptr(actions), _C.ptr(pad_mask), _C.ptr(self.consts(dev)), _C.ptr(P), P.stride(0),
                _C.ptr(Q), Q.stride(0), _C.ptr(w1), w1.stride(0), _C.ptr(self.d2.w.bf16),
                _C.ptr(self.d2.b.data), _C.ptr(t_in), _C.ptr(eps_in), 1.0, _C.ptr(scratch),
                _C.ptr(loss), _C.ptr(t), _C.ptr(eps), _C.ptr(noisy), _C.ptr(h), _C.ptr(dh),
                _C.ptr(dpred), _C.ptr(dP), _C.stream_ptr())
        return loss, dict(multi=True, e=e, temb=temb, feats=feats, ht=ht, t_all=t_all, t=t, eps=eps,
                          noisy=noisy, h=h, dh=dh, dpred=dpred, dP=dP, pad_mask=pad_mask)

    def _loss_backward_multi(self, sv: dict) -> torch.Tensor:
        """The split-Dense backward of loss_forward_multi, on the GEMM and column-sum paths into
        the flat gradient buffer. Returns d(pooled readout) (B, D) bf16."""
        if sv["dP"] is None:
            raise ValueError("loss_forward_multi ran forward-only (backward=False)")
        A, T, H, S = self.A, self.time_dim, self.hidden, self.steps
        dev = sv["dP"].device
        dh, dP = sv["dh"], sv["dP"]
        self.d2.bwd(sv["dpred"], sv["h"], need_dx=False)      # dW2 += dpred^T h, db2 += colsum
        w1g, w1t = self.d1.w.grad, self.d1.w.bf16_t           # (H, A+T+D) fp32, (A+T+D, H) bf16
        def wgrad(dy, x, cols):   # dW1[:, cols] += dy^T x, as Dense.bwd's weight gradient
            K_.gemm(dy, x, trans_a=True, out=w1g[:, cols], out_mode=K_.OUT_F32_ACCUM,
                    split_k=split_k_for(H, x.shape[1], dy.shape[0]))
        wgrad(dh, sv["noisy"], slice(0, A))                   # dW1[:, :A] += dh^T noisy
        wgrad(dP, sv["e"], slice(A + T, None))                # dW1[:, A+T:] += dP^T e
        de = K_.gemm(dP, w1t[A + T:], trans_b=True)           # dP . W1[:, A+T:]
        dQ = torch.empty((S, H), dtype=torch.float32, device=dev)
        _C.call("mmt_diffusion_loss_dq", _C.ptr(sv["t"]), _C.ptr(dh), dh.stride(0), dh.shape[0], S,
                H, _C.ptr(dQ), dQ.stride(0), _C.stream_ptr())
        K_.colsum(dQ, self.d1.b.grad)                         # db1 += colsum(dQ)
        dQb = K_.cast_f32_bf16(dQ, torch.empty((S, H), dtype=torch.bfloat16, device=dev))
        wgrad(dQb, sv["temb"], slice(A, A + T))               # dW1[:, A:A+T] += dQ^T temb
        dtemb = K_.gemm(dQb, w1t[A:A + T], trans_b=True)      # (steps, T)
        dzt = self.t2.bwd(dtemb, sv["ht"], gate=sv["ht"], gate_scale=1.0)
        dfeats = self.t1.bwd(dzt, sv["feats"])
        _C.call("mmt_fourier_bwd", _C.ptr(dfeats), S, self.F, _C.ptr(sv["t_all"]),
                _C.ptr(self.fourier.data), _C.ptr(self.fourier.grad), _C.stream_ptr())
        return de

    def loss_backward(self, sv: dict) -> torch.Tensor:
        """Returns d(readout mean) (B, D) bf16 view."""
        if sv.get("multi"):
            return self._loss_backward_multi(sv)
        B = sv["cat"].shape[0]
        dpred = sv["dpred"]
        for (d1, d2), (x, h) in reversed(list(zip(self.extra, sv.get("chain") or []))):
            dz = d2.bwd(dpred, h, gate=h, gate_scale=1.0)     # relu backward in the dX epilogue
            dpred = d1.bwd(dz, x)                              # bf16 (B, A): the previous output's
        dzd = self.d2.bwd(dpred, sv["hd"], gate=sv["hd"], gate_scale=1.0)
        dcat = self.d1.bwd(dzd, sv["cat"])
        dtemb = dcat[:, self.A:self.A + self.time_dim]
        dzt = self.t2.bwd(dtemb, sv["ht"], gate=sv["ht"], gate_scale=1.0)
        dfeats = self.t1.bwd(dzt, sv["feats"])
        _C.call("mmt_fourier_bwd", _C.ptr(dfeats), B, self.F, _C.ptr(sv["t"]),
                _C.ptr(self.fourier.data), _C.ptr(self.fourier.grad), _C.stream_ptr())
        return dcat[:, self.A + self.time_dim:]

    # ------------------------------------------------------------------ predict_denoise_term
    def predict_denoise_term_mean(self, readout_mean: torch.Tensor, time: torch.Tensor,
                                  noisy_actions: torch.Tensor) -> torch.Tensor:
        """Reference :88-107 (``OctoDenoise(noisy, time, mean(readouts))``) for given integer
        times (B,) or (B, 1) and noisy actions (B, A) fp32. Returns eps_hat (B, A) fp32."""
        B = readout_mean.shape[0]
        dev = readout_mean.device
        t = time.reshape(-1).to(torch.int32).contiguous()
        if t.numel() != B or tuple(noisy_actions.shape) != (B, self.A):
            raise ValueError("time must hold one step per sample and noisy_actions be (B, A)")
        if readout_mean.shape[1] != self.D or readout_mean.dtype != torch.bfloat16:
            raise ValueError(f"readout_mean must be bf16 (B, {self.D})")
        cat = self.new_cat(B, dev)
        feats = self._fourier_features(t, cat)
        cat[:, :self.A].copy_(noisy_actions)           # the given noisy sample (bf16 operand)
        self.readout_slot(cat).copy_(readout_mean)
        ht = self.t1.fwd(feats, act=K.ACT_RELU)
        self.t2.fwd(ht, out=cat[:, self.A:self.A + self.time_dim])
        hd = self.d1.fwd(cat, act=K.ACT_RELU)
        return self._extra_fwd(self.d2.fwd(hd, out_mode=K.OUT_F32))[0]

    # ------------------------------------------------------------------------- predict_action
    def sampler_coef(self, device) -> torch.Tensor:
        """(steps, 3) fp32 [1/sqrt(a_t), (1-a_t)/sqrt(1-abar_t), sqrt(b_t)] (:182-184)."""
        key = ("coef", device)
        if key not in self._dev_consts:
            b = self.betas_np.astype(np.float32)
            a = (np.float32(1) - b).astype(np.float32)
            c = np.stack([np.float32(1) / np.sqrt(a),
                          (np.float32(1) - a) / np.sqrt(np.float32(1) - self.alpha_hats_np),
                          np.sqrt(b)], axis=1).astype(np.float32)
            self._dev_consts[key] = torch.from_numpy(np.ascontiguousarray(c)).to(device)
        return self._dev_consts[key]

    def time_embeddings(self, device) -> torch.Tensor:
        """FourierFeatures (:41-51) + its MLPBlock for every t = 0..steps-1 -> (steps, T) bf16,
        through the training path's kernels (prep kernel with injected t, two GEMMs)."""
        return self._time_embeddings_saved(device)[0]

    def _time_embeddings_saved(self, device):
        """time_embeddings with what its backward needs: (temb (steps, T) bf16, the Fourier
        features (steps, T) bf16, the time MLP's hidden layer (steps, T) bf16, t = arange(steps))."""
        t_in = torch.arange(self.steps, dtype=torch.int32, device=device)
        feats = self._fourier_features(t_in, self.new_cat(self.steps, device))
        ht = self.t1.fwd(feats, act=K.ACT_RELU)
        return self.t2.fwd(ht), feats, ht, t_in

    def _fourier_features(self, t: torch.Tensor, cat: torch.Tensor) -> torch.Tensor:
        """The Fourier features (n, T) bf16 of the given steps t (n,) int32 from the training
        path's prep kernel, run with zero actions and injected (t, eps = 0); it also writes cat's
        action columns (n, A+T+D) bf16 (zeros)."""
        n, dev = t.shape[0], t.device
        zeros = torch.zeros((n, self.A), dtype=torch.float32, device=dev)
        feats = torch.empty((n, self.time_dim), dtype=torch.bfloat16, device=dev)
        t_out = torch.empty(n, dtype=torch.int32, device=dev)
        eps_out = torch.empty((n, self.A), dtype=torch.float32, device=dev)
        _C.call("mmt_diffusion_prep", None, n, self.A, self.steps, 0, _C.ptr(zeros),
                _C.ptr(self.consts(dev)), _C.ptr(self.fourier.data), self.F, _C.ptr(t),
                _C.ptr(zeros), _C.ptr(t_out), _C.ptr(eps_out), _C.ptr(cat), cat.stride(0),
                _C.ptr(feats), _C.stream_ptr())
        return feats

    def sampler_table(self, spec=None):
        """The update table of `spec` (default: the head's): (t int32 (K,), coef fp32 (K, 3)) numpy
        arrays with x <- clip(a x + b eps_hat(x, t) + c n) per row, built in float64 from the
        schedule. DDPM: t = S-1 .. 0, a = 1/sqrt(alpha_t), b = -a (1 - alpha_t)/sqrt(1 - abar_t),
        c = sqrt(beta_t) (0 on the t = 0 row without final noise). DDIM (eta = 0), K steps:
        t_k = round((S-1)(K-1-k)/(K-1)), a = sqrt(abar_prev/abar_t),
        b = sqrt(1 - abar_prev) - sqrt(abar_prev (1 - abar_t)/abar_t), c = 0, with abar_prev the
        next row's abar and 1 after the last."""
        spec = self.sampler if spec is None else SamplerSpec.of(spec)
        S = self.steps
        beta = self.betas_np.astype(np.float64)
        abar = self.alpha_hats_np.astype(np.float64)
        if spec.kind == "ddpm":
            if spec.steps not in (None, S):
                raise ValueError(f"the DDPM sampler walks all {S} diffusion steps, got steps="
                                 f"{spec.steps}")
            t = np.arange(S - 1, -1, -1)
            alpha = 1.0 - beta[t]
            a = 1.0 / np.sqrt(alpha)
            b = -a * (1.0 - alpha) / np.sqrt(1.0 - abar[t])
            c = np.sqrt(beta[t])
            if not spec.adds_final_noise:
                c[t == 0] = 0.0
        else:
            n = S if spec.steps is None else int(spec.steps)
            if not 1 <= n <= S:
                raise ValueError(f"the DDIM sampler needs 1 <= steps <= {S}, got {n}")
            k = np.arange(n)
            t = ((S - 1) * (n - 1 - k) + (n - 1) // 2) // (n - 1) if n > 1 else np.array([S - 1])
            prev = np.concatenate([abar[t[1:]], [1.0]])
            a = np.sqrt(prev / abar[t])
            b = np.sqrt(1.0 - prev) - np.sqrt(prev * (1.0 - abar[t]) / abar[t])
            c = np.zeros(n)
        return t.astype(np.int32), np.stack([a, b, c], axis=1).astype(np.float32)

    def _table_dev(self, spec: SamplerSpec, device):
        key = ("table", spec, device)
        if key not in self._dev_consts:
            t, coef = self.sampler_table(spec)
            self._dev_consts[key] = (torch.from_numpy(t).to(device),
                                     torch.from_numpy(np.ascontiguousarray(coef)).to(device), t)
        return self._dev_consts[key]

    def _split_first_dense(self, readout_mean, saved=None):
        """concatenate([noisy, time_emb, readout]) . W1^T (OctoDenoise :61) split along the input:
        P (B, H) = readout part, Q (steps, H) = time-embedding part + b1, both fp32. saved: the
        _time_embeddings_saved tuple of a caller that keeps it for its backward."""
        A, T = self.A, self.time_dim
        temb = (saved or self._time_embeddings_saved(readout_mean.device))[0]
        w1 = self.d1.w.bf16
        Q = K.gemm(temb, w1[:, A:A + T], trans_b=True, bias=self.d1.b.data, out_mode=K.OUT_F32)
        P = K.gemm(readout_mean, w1[:, A + T:], trans_b=True, out_mode=K.OUT_F32)
        return P, Q

    def _sample_steps(self, readout_mean, rng, sample_offset, z, noise, spec, want_z=False,
                      want_noise=False):
        """mmt_diffusion_sample_steps on spec's table. Returns (actions, z_out or None,
        noise_out or None)."""
        B, A, dev = readout_mean.shape[0], self.A, readout_mean.device
        t_dev, coef_dev, t_np = self._table_dev(spec, dev)
        n = len(t_np)
        P, Q = self._split_first_dense(readout_mean)
        w1 = self.d1.w.bf16
        actions = torch.empty((B, A), dtype=torch.float32, device=dev)
        z_out = torch.empty((B, A), dtype=torch.float32, device=dev) if want_z else None
        n_out = (torch.empty((n, B, A), dtype=torch.float32, device=dev)
                 if want_noise and spec.fresh else None)
        _C.call("mmt_diffusion_sample_steps", _C.ptr(rng), B, A, n, sample_offset, _C.ptr(P),
                P.stride(0), _C.ptr(Q), Q.stride(0), Q.shape[0], _C.ptr(w1), w1.stride(0),
                _C.ptr(self.d2.w.bf16), _C.ptr(self.d2.b.data), _C.ptr(t_dev), _C.ptr(coef_dev),
                float(spec.clip), _C.SAMPLE_FRESH_NOISE if spec.fresh else 0, _C.ptr(z),
                _C.ptr(noise), self.hidden, _C.ptr(actions), _C.ptr(z_out), _C.ptr(n_out),
                _C.stream_ptr())
        return actions, z_out, n_out

    def _sample_draws(self, B, device, rng, sample_offset, n_steps, fresh, want_z):
        """The initial sample z (B, A) (want_z) and, with fresh noise, the step noise
        (n_steps, B, A) that mmt_diffusion_sample_steps would draw, from its draws-only launch."""
        A = self.A
        z_out = torch.empty((B, A), dtype=torch.float32, device=device) if want_z else None
        n_out = torch.empty((n_steps, B, A), dtype=torch.float32, device=device) if fresh else None
        _C.call("mmt_diffusion_sample_steps", _C.ptr(rng), B, A, n_steps, sample_offset, None, 0,
                None, 0, 0, None, 0, None, None, None, None, 0.0,
                (_C.SAMPLE_FRESH_NOISE if fresh else 0) | _C.SAMPLE_DRAWS_ONLY, None, None,
                self.hidden, None, _C.ptr(z_out), _C.ptr(n_out), _C.stream_ptr())
        return z_out, n_out

    def predict_action_mean(self, readout_mean: torch.Tensor, rng=None, sample_offset: int = 0,
                            z: torch.Tensor | None = None, return_noise: bool = False, *,
                            sampler=None, noise: torch.Tensor | None = None):
        """Reference :146-209 (the DDPM loop of jax.lax.scan) on the device, and its variants.
        readout_mean: (B, D) bf16 = mean of the readout tokens (:102). `sampler` (a SamplerSpec or
        a dict of its fields; default: the head's) picks the update table; `noise` injects the
        step noise as fp32 (K, B, A), which implies fresh noise. The initial sample z and the
        step noise are drawn from the counter streams (rng = the (seed, step) device tensor, keyed
        by the global sample index sample_offset + b) unless injected. Returns actions (B, A) fp32;
        with return_noise also z and, when the noise is fresh, the step noise (K, B, A).
        One launch either way for num_blocks == 1: the reference's sampler at A == 8 runs
        mmt_diffusion_sample, everything else mmt_diffusion_sample_steps; num_blocks > 1 takes
        the per-step launch loop."""
        self._check_pooled(readout_mean, "readout_mean")
        spec = self.sampler if sampler is None else SamplerSpec.of(sampler)
        if noise is not None and not spec.fresh:
            spec = dataclasses.replace(spec, noise="fresh")   # ValueError for DDIM
        B, A = readout_mean.shape[0], self.A
        K_steps = len(self.sampler_table(spec)[0]) if noise is not None else 0
        if z is not None and (tuple(z.shape) != (B, A) or z.dtype != torch.float32
                              or not z.is_contiguous()):
            raise ValueError(f"z must be contiguous fp32 ({B}, {A})")
        if noise is not None and (tuple(noise.shape) != (K_steps, B, A)
                                  or noise.dtype != torch.float32 or not noise.is_contiguous()):
            raise ValueError(f"noise must be contiguous fp32 ({K_steps}, {B}, {A})")
        if rng is None and (z is None or (spec.fresh and noise is None)):
            raise ValueError("need rng (or an injected initial sample z and step noise)")
        self._check_fused_widths("sampler", hidden=False)   # the loop form's draws need A too
        if self.extra:
            return self._predict_action_loop(readout_mean, rng, sample_offset, z, return_noise,
                                             spec=spec, noise=noise)
        self._check_fused_widths("fused sampler", action=False)
        if not (spec.is_reference(self.steps) and A == 8 and noise is None):
            actions, z_out, n_out = self._sample_steps(readout_mean, rng, sample_offset, z, noise,
                                                       spec, want_z=return_noise,
                                                       want_noise=return_noise)
            if not return_noise:
                return actions
            return (actions, z_out, n_out) if spec.fresh else (actions, z_out)
        dev = readout_mean.device
        P, Q = self._split_first_dense(readout_mean)
        w1 = self.d1.w.bf16
        actions = torch.empty((B, A), dtype=torch.float32, device=dev)
        z_out = torch.empty((B, A), dtype=torch.float32, device=dev) if return_noise else None
        _C.call("mmt_diffusion_sample", _C.ptr(rng), B, A, self.steps, sample_offset, _C.ptr(P),
                P.stride(0), _C.ptr(Q), Q.stride(0), _C.ptr(w1), w1.stride(0),
                _C.ptr(self.d2.w.bf16), _C.ptr(self.d2.b.data), _C.ptr(self.sampler_coef(dev)),
                _C.ptr(z), self.hidden, _C.ptr(actions), _C.ptr(z_out), _C.stream_ptr())
        return (actions, z_out) if return_noise else actions

    def _predict_action_loop(self, readout_mean, rng, sample_offset, z, return_noise, *,
                             spec: SamplerSpec | None = None, noise=None):
        """predict_action for OctoDenoise num_blocks > 1 (the fused one-launch samplers hold one
        MLPBlock): the rows of spec's table (default: the head's sampler) as a loop of
        predict_denoise_term_mean launches and the clipped update on the device. What is not
        injected of the initial sample z and the step noise comes from the fused entry's own
        counter-stream draws (its draws-only launch), so both forms consume identical draws. The
        noisy sample enters the denoiser as its bf16 GEMM operand (the fused kernels keep it
        fp32)."""
        spec = self.sampler if spec is None else spec
        t_dev, coef, t_np = self._table_dev(spec, readout_mean.device)
        need_noise = spec.fresh and noise is None
        if z is None or need_noise:
            z_d, n_d = self._sample_draws(readout_mean.shape[0], readout_mean.device, rng,
                                          sample_offset, len(t_np), need_noise, z is None)
            z = z_d if z is None else z
            noise = n_d if need_noise else noise
        x = z.clone()
        for k, t in enumerate(t_np):
            tt = torch.full((x.shape[0],), int(t), dtype=torch.int32, device=x.device)
            eps = self.predict_denoise_term_mean(readout_mean, tt, x)
            n = noise[k] if spec.fresh else z
            x = torch.clamp(coef[k, 0] * x + coef[k, 1] * eps + coef[k, 2] * n,
                            -float(spec.clip), float(spec.clip))
        if not return_noise:
            return x
        return (x, z, noise) if spec.fresh else (x, z)
