"""LoRA configuration and adapter layout (engine/lora.py), host side: field
validation, target resolution, scaling, rank padding and the round trip between
peft's state-dict names and the padded / transposed flat layout.  No GPU."""
import math
import types

import pytest
import torch

import swh_trl_amd
from swh_trl_amd.engine import lora, tiny_llama, tiny_qwen2
from swh_trl_amd.engine.lora import LoraConfig


def test_exported_and_defaults_are_pefts():
    assert swh_trl_amd.LoraConfig is LoraConfig
    c = LoraConfig()
    assert (c.r, c.lora_alpha, c.target_modules, c.lora_dropout, c.bias) == (8, 8, None, 0.0, "none")
    assert (c.use_rslora, c.use_dora, c.modules_to_save, c.task_type, c.init_lora_weights) == \
        (False, False, None, None, True)
    assert not c.rank_pattern and not c.alpha_pattern and not c.layers_to_transform


@pytest.mark.parametrize("field,value", [
    ("lora_dropout", 0.1), ("bias", "all"), ("bias", "lora_only"), ("use_dora", True),
    ("modules_to_save", ["lm_head"]), ("rank_pattern", {"q_proj": 4}), ("alpha_pattern", {"q_proj": 4}),
    ("layers_to_transform", [0]), ("init_lora_weights", False), ("init_lora_weights", "gaussian"),
    ("task_type", "SEQ_CLS"), ("r", 0), ("r", 65), ("r", 2.5), ("lora_alpha", 0),
    ("target_modules", ["lm_head"]), ("target_modules", []), ("target_modules", ".*proj"),
])
def test_refused_fields_raise_and_name_themselves(field, value):
    with pytest.raises(ValueError, match=field):
        lora.resolve(LoraConfig(**{field: value}))


@pytest.mark.parametrize("field,value", [
    ("lora_dropout", 0.0), ("lora_dropout", 0), ("bias", "none"), ("use_dora", False), ("modules_to_save", None),
    ("modules_to_save", []), ("rank_pattern", {}), ("alpha_pattern", {}), ("layers_to_transform", None),
    ("init_lora_weights", True), ("task_type", None), ("task_type", "CAUSAL_LM"), ("r", 1), ("r", 64),
    ("use_rslora", True),
])
def test_no_op_values_pass(field, value):
    spec = lora.resolve(LoraConfig(**{field: value}))
    assert spec.targets == ("q_proj", "v_proj")


def test_task_type_enum_like_and_gpt2_refused():
    enum_like = types.SimpleNamespace(value="CAUSAL_LM")
    assert lora.resolve(LoraConfig(task_type=enum_like)).task_type == "CAUSAL_LM"
    with pytest.raises(ValueError, match="gpt2"):
        lora.resolve(LoraConfig(), model_type="gpt2")


def test_target_resolution():
    assert lora.resolve(LoraConfig(target_modules=None)).targets == ("q_proj", "v_proj")
    assert lora.resolve(LoraConfig(target_modules=None), "llama").targets == ("q_proj", "v_proj")
    assert lora.resolve(LoraConfig(target_modules="all-linear")).targets == lora.TARGET_MODULES
    assert len(lora.TARGET_MODULES) == 7
    # an explicit list, in any order (and peft's set), comes out in canonical order
    assert lora.resolve(LoraConfig(target_modules=["down_proj", "k_proj"])).targets == ("k_proj", "down_proj")
    assert lora.resolve(LoraConfig(target_modules={"up_proj", "o_proj"})).targets == ("o_proj", "up_proj")


def test_scaling_with_and_without_rslora():
    assert lora.resolve(LoraConfig(r=16, lora_alpha=32)).scale == 2.0
    assert lora.resolve(LoraConfig(r=8, lora_alpha=8)).scale == 1.0
    assert lora.resolve(LoraConfig(r=16, lora_alpha=32, use_rslora=True)).scale == 8.0
    assert lora.resolve(LoraConfig(r=5, lora_alpha=3, use_rslora=True)).scale == pytest.approx(3 / math.sqrt(5))
    assert lora.scaling(4, 1) == 0.25


def test_rank_padding():
    assert [lora.rank_pad(r) for r in (1, 4, 8, 15, 16, 17, 32, 33, 48, 49, 64)] == \
        [16, 16, 16, 16, 16, 32, 32, 48, 48, 64, 64]
    from swh_trl_amd import nn_ops
    assert all(nn_ops.lora_rank_pad(r) == lora.rank_pad(r) for r in range(1, 65))


def test_duck_typed_config_is_accepted():
    ns = types.SimpleNamespace(r=4, lora_alpha=16, target_modules=["q_proj", "o_proj"], lora_dropout=0.0,
                               bias="none")
    spec = lora.resolve(ns)
    assert (spec.r, spec.scale, spec.targets, spec.use_rslora) == (4, 4.0, ("q_proj", "o_proj"), False)
    with pytest.raises(ValueError, match="use_dora"):
        lora.resolve(types.SimpleNamespace(r=4, lora_alpha=16, use_dora=True))


@pytest.mark.parametrize("cfg", [tiny_qwen2(1024, 2), tiny_llama(2048, 2)], ids=["qwen2", "llama"])
@pytest.mark.parametrize("targets,r", [("all-linear", 8), (None, 4), (["k_proj", "up_proj", "down_proj"], 20)])
def test_layout_and_peft_round_trip(cfg, targets, r):
    spec = lora.resolve(LoraConfig(r=r, lora_alpha=2 * r, target_modules=targets), cfg.model_type)
    layout, numel = lora.adapter_layout(cfg, spec)
    Rp = spec.rank_pad
    # stacked A per pack, one Bt per module, 64-element aligned, nothing overlaps
    spans = sorted((o, o + math.prod(s)) for o, s in layout.values())
    assert all(o % 64 == 0 for o, _ in spans) and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][1] <= numel
    n_qkv = sum(m in spec.targets for m in ("q_proj", "k_proj", "v_proj"))
    if n_qkv:
        assert layout["l0.qkv.A"][1] == (n_qkv * Rp, cfg.hidden_size)
    for m in spec.targets:
        assert layout[f"l1.{m}.Bt"][1] == (Rp, lora.module_dims(cfg, m)[1])
    # random peft state dict -> flat -> peft state dict
    g = torch.Generator().manual_seed(0)
    sd = {}
    for i in range(cfg.num_hidden_layers):
        for m in spec.targets:
            kin, nout = lora.module_dims(cfg, m)
            sd[lora.peft_key(i, m, "A")] = torch.randn(r, kin, generator=g)
            sd[lora.peft_key(i, m, "B")] = torch.randn(nout, r, generator=g)
    assert "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight" in sd or "q_proj" not in spec.targets
    flat = torch.full((numel,), 7.0)
    lora.pack_adapter(sd, flat, cfg, spec)
    back = lora.unpack_adapter(flat, cfg, spec)
    assert set(back) == set(sd)
    for k in sd:
        assert back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
    # B is stored transposed, pad rows (and the alignment gaps) are zero
    views = lora._views(flat, layout)
    m0 = spec.targets[0]
    assert torch.equal(views[f"l0.{m0}.Bt"][:r], sd[lora.peft_key(0, m0, "B")].t())
    for name, t in views.items():
        for r0 in range(0, t.shape[0], Rp):
            assert not t[r0 + r:r0 + Rp].any(), name
    assert flat.count_nonzero() == sum(t.count_nonzero() for t in sd.values())
    # peft's adapter-name infix is accepted; a wrong key set or shape is not
    named = {k.replace(".weight", ".default.weight"): t for k, t in sd.items()}
    flat2 = torch.zeros(numel)
    lora.pack_adapter(named, flat2, cfg, spec)
    assert torch.equal(flat2, flat)
    short = dict(sd)
    short.pop(next(iter(short)))
    with pytest.raises(ValueError, match="missing"):
        lora.pack_adapter(short, flat2, cfg, spec)
    k0 = lora.peft_key(0, m0, "A")
    with pytest.raises(ValueError, match="expected A"):
        lora.pack_adapter({**sd, k0: sd[k0][:, :-1]}, flat2, cfg, spec)


def test_adapter_config_dict_fields():
    spec = lora.resolve(LoraConfig(r=16, lora_alpha=32, target_modules="all-linear"))
    d = lora.adapter_config_dict(spec, "Qwen/Qwen2.5-0.5B")
    assert d["peft_type"] == "LORA" and d["r"] == 16 and d["lora_alpha"] == 32
    assert d["target_modules"] == list(lora.TARGET_MODULES)
    assert d["lora_dropout"] == 0.0 and d["bias"] == "none" and d["task_type"] == "CAUSAL_LM"
    assert d["base_model_name_or_path"] == "Qwen/Qwen2.5-0.5B"
    import json
    assert json.loads(json.dumps(d)) == d
