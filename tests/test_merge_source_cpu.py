"""CPU: the configuration surface, the C-ABI binding and the argument checks of the merge source
and unmerge entry points (csrc/tome.hip; include/mmt_api.h). Every call below is rejected by the
host wrapper before any HIP call: the return value is -1 (MMT_ERR_INVALID), mmt_last_error() names
the entry point and nothing is launched, so any aligned non-null pointer value serves."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["mmt_tome_pos_map", "mmt_tome_source_step", "mmt_tome_source_groups",
         "mmt_tome_unmerge_fwd", "mmt_tome_unmerge_bwd"]
PTR = 1 << 20          # non-null, 16-B aligned
F32, BF16 = 0, 1


# ------------------------------------------------------------------------------- config surface
def test_flag_defaults_to_off_and_reaches_the_config():
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import OctoConfig, get_config
    assert OctoConfig().track_merge_source is False
    assert get_config("octo-small-tome16").track_merge_source is False
    assert get_config("octo_small_tome16").track_merge_source is False          # YAML, key absent
    yaml_cfg = get_config("octo_small_tome16_source")                           # the new YAML file
    assert yaml_cfg.track_merge_source is True
    # the override path of bench.py --set track_merge_source=1
    preset = get_config("octo-small-tome16", track_merge_source=True)
    assert preset.track_merge_source is True
    assert get_config("octo_small_tome16", track_merge_source=True).track_merge_source is True
    base = get_config("octo_small_tome16")
    for f in ("token_embedding_dim", "num_heads", "mlp_dim", "num_blocks", "input_sequence",
              "token_compression_sequence", "compression", "proportional_attention", "image_size",
              "patch_size", "text_tokens"):
        assert getattr(yaml_cfg, f) == getattr(base, f) == getattr(preset, f), f


def test_yaml_differs_from_tome16_only_in_the_flag():
    d = ROOT / "multi_modal_transformers_tokenmerge_amd" / "model_configs"

    def body(name):
        return [ln for ln in (d / name).read_text().splitlines() if not ln.startswith("#")]
    a, b = body("octo_small_tome16.yaml"), body("octo_small_tome16_source.yaml")
    assert [ln for ln in b if ln not in a] == ["track_merge_source: true"]
    assert [ln for ln in a if ln not in b] == []


def test_flag_needs_tome():
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import OctoConfig, get_config
    with pytest.raises(ValueError):
        OctoConfig(token_compression_sequence="[Image{16};Readout{0}]", compression="prune",
                   track_merge_source=True)
    with pytest.raises(ValueError):
        get_config("octo-small-prune16", track_merge_source=True)
    # without a compression sequence the flag is a no-op, not an error
    assert get_config("octo-small", track_merge_source=True).tome_r == 0


def test_layer_ctx_carries_the_flag():
    from multi_modal_transformers_tokenmerge_amd.attention_blocks.attention import LayerCtx
    assert LayerCtx(layer=0, sets=None, table=None).track_source is False
    assert LayerCtx(layer=0, sets=None, table=None, track_source=True).track_source is True


def test_public_names():
    from multi_modal_transformers_tokenmerge_amd.tokenizers import token_compression as tc
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    for name in ("MergeSource", "merge_source", "unmerge"):
        assert hasattr(tc, name), name
    for name in ("tome_pos_map", "tome_source_step", "tome_source_groups", "tome_unmerge_fwd",
                 "tome_unmerge_bwd"):
        assert callable(getattr(K, name)), name


# -------------------------------------------------------------------------------------- binding
def _header_arg_count(name):
    text = (ROOT / "include" / "mmt_api.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/mmt_api.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NAMES)
def test_binding_lists_the_new_entry_points(name):
    from multi_modal_transformers_tokenmerge_amd import _C
    assert name in _C.SIGNATURES and name in _C.exported_symbols()
    assert len(_C.SIGNATURES[name]) == _header_arg_count(name)
    assert _C.SIGNATURES[name][-1] == _C.P          # the stream, last
    assert _C.API_VERSION == 2
    assert hasattr(_C.lib(), name)  # exported by the built library


# ------------------------------------------------------------------------- argument rejections
def _pos(lib, unm=PTR, src=PTR, dst=PTR, n=2, t=16, r=4, flags=0, pm=PTR):
    return lib.mmt_tome_pos_map(unm, src, dst, n, t, r, flags, pm, None)


def _step(lib, pm=PTR, n=2, t=16, r=4, source=PTR, t0=32, first=0):
    return lib.mmt_tome_source_step(pm, n, t, r, source, t0, first, None)


def _groups(lib, source=PTR, n=2, t0=32, tf=8, gs=PTR, members=PTR):
    return lib.mmt_tome_source_groups(source, n, t0, tf, gs, members, None)


def _ufwd(lib, x=PTR, dtype=F32, n=2, L=20, D=8, xs_n=160, xs_t=8, set_start=4, tf=8, source=PTR,
          t0=32, out=PTR, os_n=352, os_t=8):
    return lib.mmt_tome_unmerge_fwd(x, dtype, n, L, D, xs_n, xs_t, set_start, tf, source, t0, out,
                                    os_n, os_t, None)


def _ubwd(lib, g=PTR, dtype=F32, n=2, L=20, D=8, gs_n=352, gs_t=8, set_start=4, tf=8, gstart=PTR,
          members=PTR, t0=32, gx=PTR, xs_n=160, xs_t=8):
    return lib.mmt_tome_unmerge_bwd(g, dtype, n, L, D, gs_n, gs_t, set_start, tf, gstart, members,
                                    t0, gx, xs_n, xs_t, None)


REJECTED = [
    ("pos-null-unm", "mmt_tome_pos_map", lambda l: _pos(l, unm=None)),
    ("pos-null-src", "mmt_tome_pos_map", lambda l: _pos(l, src=None)),
    ("pos-null-dst", "mmt_tome_pos_map", lambda l: _pos(l, dst=None)),
    ("pos-null-pos_map", "mmt_tome_pos_map", lambda l: _pos(l, pm=None)),
    ("pos-n-0", "mmt_tome_pos_map", lambda l: _pos(l, n=0)),
    ("pos-n-neg", "mmt_tome_pos_map", lambda l: _pos(l, n=-1)),
    ("pos-t-1", "mmt_tome_pos_map", lambda l: _pos(l, t=1, r=1)),
    ("pos-r-0", "mmt_tome_pos_map", lambda l: _pos(l, r=0)),
    ("pos-r-neg", "mmt_tome_pos_map", lambda l: _pos(l, r=-2)),
    ("pos-r-gt-half", "mmt_tome_pos_map", lambda l: _pos(l, t=16, r=9)),
    ("pos-r-gt-512", "mmt_tome_pos_map", lambda l: _pos(l, t=2048, r=513)),
    ("pos-unm-gt-1024", "mmt_tome_pos_map", lambda l: _pos(l, t=2100, r=8)),
    ("pos-distill-no-unm", "mmt_tome_pos_map", lambda l: _pos(l, t=16, r=8, flags=2)),
    ("step-null-pos_map", "mmt_tome_source_step", lambda l: _step(l, pm=None)),
    ("step-null-source", "mmt_tome_source_step", lambda l: _step(l, source=None)),
    ("step-n-0", "mmt_tome_source_step", lambda l: _step(l, n=0)),
    ("step-t-1", "mmt_tome_source_step", lambda l: _step(l, t=1, r=1)),
    ("step-t0-gt-2048", "mmt_tome_source_step", lambda l: _step(l, t0=2049)),
    ("step-t0-lt-t", "mmt_tome_source_step", lambda l: _step(l, t=16, t0=15)),
    ("step-r-0", "mmt_tome_source_step", lambda l: _step(l, r=0)),
    ("step-r-gt-half", "mmt_tome_source_step", lambda l: _step(l, t=16, r=9)),
    ("step-first-t0-ne-t", "mmt_tome_source_step", lambda l: _step(l, t=16, t0=32, first=1)),
    ("groups-null-source", "mmt_tome_source_groups", lambda l: _groups(l, source=None)),
    ("groups-null-group_start", "mmt_tome_source_groups", lambda l: _groups(l, gs=None)),
    ("groups-null-members", "mmt_tome_source_groups", lambda l: _groups(l, members=None)),
    ("groups-n-0", "mmt_tome_source_groups", lambda l: _groups(l, n=0)),
    ("groups-tf-0", "mmt_tome_source_groups", lambda l: _groups(l, tf=0)),
    ("groups-tf-gt-t0", "mmt_tome_source_groups", lambda l: _groups(l, t0=8, tf=9)),
    ("groups-t0-gt-2048", "mmt_tome_source_groups", lambda l: _groups(l, t0=2049)),
    ("groups-t0-neg", "mmt_tome_source_groups", lambda l: _groups(l, t0=-4, tf=-8)),
    ("ufwd-null-x", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, x=None)),
    ("ufwd-null-source", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, source=None)),
    ("ufwd-null-out", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, out=None)),
    ("ufwd-n-0", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, n=0)),
    ("ufwd-L-0", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, L=0)),
    ("ufwd-D-0", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, D=0)),
    ("ufwd-D-neg", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, D=-8)),
    ("ufwd-D-12-f32", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, D=12, xs_t=12, os_t=12)),
    ("ufwd-D-12-bf16", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, dtype=BF16, D=12)),
    ("ufwd-dtype", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, dtype=2)),
    ("ufwd-tf-0", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, tf=0)),
    ("ufwd-tf-gt-t0", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, tf=8, t0=7)),
    ("ufwd-t0-gt-2048", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, t0=2049)),
    ("ufwd-set_start-neg", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, set_start=-1)),
    ("ufwd-set-leaves", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, L=20, set_start=13, tf=8)),
    ("ufwd-stride-2-bf16", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, dtype=BF16, xs_t=12)),
    ("ufwd-x-unaligned", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, x=PTR + 8)),
    ("ufwd-out-unaligned", "mmt_tome_unmerge_fwd", lambda l: _ufwd(l, out=PTR + 4)),
    ("ubwd-null-g", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, g=None)),
    ("ubwd-null-group_start", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, gstart=None)),
    ("ubwd-null-members", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, members=None)),
    ("ubwd-null-g_x", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, gx=None)),
    ("ubwd-n-0", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, n=0)),
    ("ubwd-L-neg", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, L=-3)),
    ("ubwd-D-0", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, D=0)),
    ("ubwd-D-12", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, D=12, gs_t=12, xs_t=12)),
    ("ubwd-dtype", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, dtype=-1)),
    ("ubwd-tf-0", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, tf=0)),
    ("ubwd-tf-gt-t0", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, tf=8, t0=4)),
    ("ubwd-t0-gt-2048", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, t0=4096)),
    ("ubwd-set_start-neg", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, set_start=-4)),
    ("ubwd-set-leaves", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, L=10, set_start=4, tf=8)),
    ("ubwd-stride-6", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, gs_n=358)),
    ("ubwd-g-unaligned", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, g=PTR + 2)),
    ("ubwd-g_x-unaligned", "mmt_tome_unmerge_bwd", lambda l: _ubwd(l, gx=PTR + 8)),
]


@pytest.mark.parametrize("name,call", [c[1:] for c in REJECTED], ids=[c[0] for c in REJECTED])
def test_entry_points_reject_bad_arguments_without_gpu(name, call):
    from multi_modal_transformers_tokenmerge_amd import _C
    lib = _C.lib()
    # leave another entry point's message behind first, so a stale one cannot satisfy the check
    assert lib.mmt_step_advance(None, None) == -1 and b"mmt_step_advance" in lib.mmt_last_error()
    assert call(lib) == -1                       # MMT_ERR_INVALID
    msg = lib.mmt_last_error()
    assert msg and name.encode() in msg, msg
