"""AdamW parameter groups on a host-built model (no GPU): AdamW.weight_decay_mask / frozen_keys
resolved against the parameter names, the per-chunk flag table of the store, the backward's cut,
the errors, and the two optimizer YAMLs."""
import fnmatch

import pytest
import torch

from multi_modal_transformers_tokenmerge_amd import config_loader as CL
from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
from multi_modal_transformers_tokenmerge_amd.params import (ALIGN, GROUP_CHUNK, GROUP_FROZEN,
                                                            GROUP_NO_DECAY)
from multi_modal_transformers_tokenmerge_amd.schedules import WarmupCosine, WarmupRsqrt

_MODELS = {}


def _model(name="octo-tiny"):
    if name not in _MODELS:
        _MODELS[name] = O.Octo(get_config(name), torch.device("cpu"), seed=0)
    return _MODELS[name]


def _names(m):
    return [p.name for p in m.store.params]


def _before_blocks(m):
    """The names declared before block 0, in declaration order."""
    out = []
    for n in _names(m):
        if n.startswith("StackedEncoder1DBlock_0/Block_"):
            break
        out.append(n)
    return out


@pytest.mark.parametrize("config,count", [("octo-tiny", 56), ("octo-small", 57)])
def test_kernels_preset_is_the_names_ending_in_kernel(config, count):
    m = _model(config)
    state = O.create_octo_train_state(m, O.AdamW(weight_decay_mask="kernels"))
    groups = state.param_groups
    want = {n for n in _names(m) if n.split("/")[-1] == "kernel"}
    assert len(want) == count
    assert {n for n, g in groups.items() if g["decay"]} == want
    assert not any(g["frozen"] for g in groups.values())
    # what the recipe leaves alone
    leaf = lambda n: n.split("/")[-1]  # noqa: E731
    undecayed = {leaf(n) for n, g in groups.items() if not g["decay"]}
    assert undecayed == {"bias", "scale", "embedding", "pos_embedding", "fourier_kernel"}
    assert m._cut == (0, False)
    assert m.store.trainable_numel == m.store.num_params()


def test_kernels_preset_excludes_the_pooling_probe():
    m = O.Octo(get_config("octo-tiny", readout_pooling="attention"), torch.device("cpu"), seed=0)
    state = O.create_octo_train_state(m, O.AdamW(weight_decay_mask="kernels"))
    probe = [n for n in _names(m) if n.endswith("/learnt_q_input")]
    assert len(probe) == 1 and state.param_groups[probe[0]] == {"decay": False, "frozen": False}


def test_head_only_freezes_every_non_head_name():
    m = _model()
    nb = m.cfg.num_blocks
    state = O.create_octo_train_state(m, O.AdamW(frozen_keys="head_only"))
    groups = state.param_groups
    for n in _names(m):
        assert groups[n]["frozen"] == (not n.startswith("diffusion_action_head/")), n
        assert groups[n]["decay"] is True
    assert m._cut == (nb, True)
    head = sum(p.numel for p in m.store.params if p.name.startswith("diffusion_action_head/"))
    assert m.store.trainable_numel == head and 0 < head < m.store.num_params()
    # every stage of a split backward below the heads is idle
    assert [m.stage_active(k, 3) for k in range(3)] == [True, False, False]


def test_head_only_takes_the_prefixes_from_the_head_objects():
    cfg = get_config("octo-tiny", action_heads=("diffusion", "continuous", "categorical"),
                     readout_pooling="attention")
    m = O.Octo(cfg, torch.device("cpu"), seed=0)
    pre = m.head_prefixes()
    assert set(pre) == {"diffusion_action_head", "continuous_action_head",
                        "categorical_action_head",
                        "diffusion_action_head/MultiHeadAttentionPooling_0"}
    state = O.create_octo_train_state(m, O.AdamW(frozen_keys="head_only"))
    for n, g in state.param_groups.items():
        assert g["frozen"] == (n.split("/")[0] not in {"diffusion_action_head",
                                                       "continuous_action_head",
                                                       "categorical_action_head"}), n
    assert m._cut == (cfg.num_blocks, True)


def test_cut_follows_the_lowest_trainable_block():
    m = _model()
    nb = m.cfg.num_blocks
    pre = _before_blocks(m)
    assert len(pre) == 16 and pre[-1] == "StackedEncoder1DBlock_0/posembed_input/pos_embedding"
    O.create_octo_train_state(m, O.AdamW(frozen_keys=["*/Block_[0-5]/*", *pre]))
    assert m._cut == (6, True)
    frozen = {p.name for p in m.store.params if p.frozen}
    want = set(pre) | {n for n in _names(m)
                       if any(n.startswith(f"StackedEncoder1DBlock_0/Block_{j}/") for j in range(6))}
    assert frozen == want
    assert not any(n.split("/")[1] in ("Block_10", "Block_11") for n in frozen)
    # stage plan nb > 8 > 4 > 0: the stage holding the cut runs, the one below it does not
    assert m.stage_bounds(3) == [nb, 8, 4, 0]
    assert [m.stage_active(k, 3) for k in range(3)] == [True, True, False]

    O.create_octo_train_state(m, O.AdamW(frozen_keys="*/Block_3/*"))
    assert m._cut == (0, False)
    assert {p.name.split("/")[1] for p in m.store.params if p.frozen} == {"Block_3"}
    assert [m.stage_active(k, 3) for k in range(3)] == [True, True, True]

    # blocks frozen but a token parameter trained: its gradient comes through every block
    O.create_octo_train_state(m, O.AdamW(frozen_keys="*/Block_[0-5]/*"))
    assert m._cut == (0, False)

    # tokens frozen, every block trained: the blocks run, the token / stem backward does not
    O.create_octo_train_state(m, O.AdamW(frozen_keys=pre))
    assert m._cut == (0, True)
    assert [m.stage_active(k, 3) for k in range(3)] == [True, True, True]


def test_chunk_table_carries_every_parameters_flags():
    m = _model()
    st = m.store
    pre = _before_blocks(m)
    O.create_octo_train_state(m, O.AdamW(weight_decay_mask="kernels",
                                         frozen_keys=["*/Block_[0-5]/*", *pre]))
    table = st.chunk_flags
    assert table.dtype == torch.uint8 and ALIGN == GROUP_CHUNK == 64
    assert table.numel() == -(-st.n // 64) == -(-st.flat.numel() // 64)
    ends = [p.offset for p in st.params[1:]] + [st.n]
    covered = 0
    for p, end in zip(st.params, ends):
        assert p.offset % 64 == 0 and end % 64 == 0
        want = (0 if p.decay else GROUP_NO_DECAY) | (GROUP_FROZEN if p.frozen else 0)
        chunks = table[p.offset // 64:end // 64]          # the padding chunks included
        assert chunks.numel() == -(-p.numel // 64) and bool((chunks == want).all()), p.name
        covered += chunks.numel()
    assert covered == table.numel()
    seen = set(table.tolist())
    assert seen == {0, GROUP_NO_DECAY, GROUP_FROZEN, GROUP_NO_DECAY | GROUP_FROZEN}


def test_defaults_keep_no_table_and_a_new_state_resets_the_groups():
    m = _model()
    O.create_octo_train_state(m, O.AdamW(frozen_keys="head_only"))
    assert m.store.chunk_flags is not None and m._cut[0] == m.cfg.num_blocks
    state = O.create_octo_train_state(m, O.AdamW())
    assert m.store.chunk_flags is None and m._cut == (0, False)
    assert all(g == {"decay": True, "frozen": False} for g in state.param_groups.values())
    # an explicitly empty request keeps a table with no bit set
    O.create_octo_train_state(m, O.AdamW(weight_decay_mask="*", frozen_keys=()))
    assert m.store.chunk_flags is not None and int(m.store.chunk_flags.max()) == 0
    assert m._cut == (0, False)


def test_bad_requests_raise():
    m = _model()
    with pytest.raises(ValueError, match="Block_99"):
        O.create_octo_train_state(m, O.AdamW(frozen_keys=["*/Block_3/*", "*/Block_99/*"]))
    with pytest.raises(ValueError, match="kernal"):
        O.create_octo_train_state(m, O.AdamW(weight_decay_mask="*/kernal"))
    with pytest.raises(ValueError, match="every parameter"):
        O.create_octo_train_state(m, O.AdamW(frozen_keys="*"))
    for bad in (5, ("*/kernel", 3), {"a": 1}, True):
        with pytest.raises(ValueError):
            O.AdamW(frozen_keys=bad)
        with pytest.raises(ValueError):
            O.AdamW(weight_decay_mask=bad)
    # "head_only" is a preset of frozen_keys alone: as a decay mask it is a pattern, matching nothing
    with pytest.raises(ValueError, match="head_only"):
        O.create_octo_train_state(m, O.AdamW(weight_decay_mask="head_only"))
    # a refused request leaves the groups as they were
    O.create_octo_train_state(m, O.AdamW())
    with pytest.raises(ValueError):
        O.create_octo_train_state(m, O.AdamW(frozen_keys="nothing/like/this"))
    assert m.store.chunk_flags is None and not any(p.frozen for p in m.store.params)


def test_patterns_are_case_sensitive_fnmatch():
    m = _model()
    name = "StackedEncoder1DBlock_0/Block_3/MLPBlock_0/Dense_0/kernel"
    assert name in _names(m)
    state = O.create_octo_train_state(m, O.AdamW(weight_decay_mask=[name]))
    assert [n for n, g in state.param_groups.items() if g["decay"]] == [name]
    with pytest.raises(ValueError):
        O.create_octo_train_state(m, O.AdamW(weight_decay_mask=[name.lower()]))
    pats = ("*/Dense_?/kernel", "*/LayerNorm_[01]/scale")
    state = O.create_octo_train_state(m, O.AdamW(weight_decay_mask=pats))
    for n, g in state.param_groups.items():
        assert g["decay"] == any(fnmatch.fnmatchcase(n, p) for p in pats), n


def test_yamls_instantiate():
    tx = CL.instantiate(CL.compose("optimizers/adamw_octo_pretrain")["optimizer"])
    assert isinstance(tx, O.AdamW) and isinstance(tx.learning_rate, WarmupRsqrt)
    assert tx.max_grad_norm == 1.0 and tx.weight_decay == 0.1
    assert tx.weight_decay_mask == "kernels" and tx.frozen_keys is None and tx.grouped
    tx = CL.instantiate(CL.compose("optimizers/adamw_finetune_head_only")["optimizer"])
    assert isinstance(tx, O.AdamW) and isinstance(tx.learning_rate, WarmupCosine)
    assert tx.max_grad_norm == 1.0 and tx.frozen_keys == "head_only"
    assert tx.weight_decay_mask is None and tx.device_control
    m = _model()
    state = O.create_octo_train_state(m, tx)
    assert m._cut == (m.cfg.num_blocks, True) and sum(
        g["frozen"] for g in state.param_groups.values()) == 160
    assert not O.AdamW().grouped


def test_ddp_step_skips_idle_stages_and_frozen_regions():
    """distributed.DDPStep's plan over a 3-stage backward (blocks [8, 12) + heads, [4, 8), [0, 4) +
    tokens), built on the host (nothing is launched)."""
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep, GradAllReducer
    m = _model()
    red = GradAllReducer(2)

    def plan(tx):
        state = O.create_octo_train_state(m, tx, allreduce=red)
        return DDPStep(m, state, None, None, None, red, stages=3, use_graph=False)
    regions = m.grad_regions(3)
    size = [4 * (hi - lo) for lo, hi in regions]
    d = plan(O.AdamW())
    assert d.active == [True] * 3 and d.reduced == [True] * 3 and d.exposed_bytes == size[2]
    d = plan(O.AdamW(frozen_keys=["*/Block_[0-5]/*", *_before_blocks(m)]))
    assert d.active == [True, True, False] and d.reduced == [True, True, False]
    assert d.exposed_bytes == size[1]
    d = plan(O.AdamW(frozen_keys="head_only"))
    assert d.active == [True, False, False] and d.reduced == [True, False, False]
    assert d.exposed_bytes == size[0]
    d = plan(O.AdamW(frozen_keys="*/Block_[0-3]/*"))   # tokens trained: everything runs,
    assert d.active == [True] * 3 and d.reduced == [True] * 3  # the last region holds them
    d = plan(O.AdamW(frozen_keys=["*/Block_[4-7]/*"]))  # an all-frozen region in the middle
    assert d.active == [True] * 3 and d.reduced == [True, False, True]
    assert d.exposed_bytes == size[2]
    O.create_octo_train_state(m, O.AdamW())
