"""CPU: the configuration surface and the C-ABI binding of proportional attention."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_yaml_key_and_preset_reach_the_config():
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    assert get_config("octo-small-tome16").proportional_attention is False
    assert get_config("octo_small_tome16").proportional_attention is False
    preset = get_config("octo-small-tome16-prop")
    yaml_cfg = get_config("octo_small_tome16_prop")
    assert preset.proportional_attention is True and yaml_cfg.proportional_attention is True
    base = get_config("octo-small-tome16")
    for f in ("token_embedding_dim", "num_heads", "mlp_dim", "num_blocks", "input_sequence",
              "token_compression_sequence", "compression"):
        assert getattr(preset, f) == getattr(base, f) == getattr(yaml_cfg, f), f
    # the override path of bench.py --set proportional_attention=1
    assert get_config("octo-small-tome16", proportional_attention=True).proportional_attention


def test_flag_needs_tome():
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import OctoConfig, get_config
    with pytest.raises(ValueError):
        OctoConfig(token_compression_sequence="[Image{16};Readout{0}]", compression="prune",
                   proportional_attention=True)
    with pytest.raises(ValueError):
        get_config("octo-small-prune16", proportional_attention=True)
    # without a compression sequence the flag is a no-op, not an error
    assert get_config("octo-small", proportional_attention=True).tome_r == 0


def _header_arg_count(name):
    text = (ROOT / "include" / "mmt_api.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/mmt_api.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,extra_over", [("mmt_attn_fwd_keybias", "mmt_attn_fwd"),
                                             ("mmt_attn_bwd_keybias", "mmt_attn_bwd"),
                                             ("mmt_tome_size_bias", None)])
def test_binding_lists_the_new_entry_points(name, extra_over):
    from multi_modal_transformers_tokenmerge_amd import _C
    assert name in _C.SIGNATURES and name in _C.exported_symbols()
    assert len(_C.SIGNATURES[name]) == _header_arg_count(name)
    if extra_over:  # the existing argument list plus (key_bias, kb_s_b), the stream still last
        old, new = _C.SIGNATURES[extra_over], _C.SIGNATURES[name]
        assert new == old[:-1] + [_C.P, _C.L] + old[-1:]
        assert len(old) == _header_arg_count(extra_over)
    assert _C.API_VERSION == 2
    assert hasattr(_C.lib(), name)  # exported by the built library
