"""CPU: the ViT tower's host side (vlp_amd/vit.py) and its test reference.

  * tests/vit_ref.py (the fp64 restatement the GPU tests use) against
    transformers.ViTModel built locally from a ViTConfig;
  * ViTTower's timm key set, parameter count and constructor contract;
  * ImageEncoder / VisionLanguageModule construct with vit_base_patch16_224;
  * the new experiment YAML composes.
No compute call reaches the device here.
"""
import functools

import pytest
import torch

from tests.vit_ref import ViTRef, deterministic_weights


def test_vit_ref_matches_transformers_vit():
    tr = pytest.importorskip("transformers")
    D, depth, S = 64, 2, 32
    cfg = tr.ViTConfig(hidden_size=D, num_hidden_layers=depth, num_attention_heads=1, intermediate_size=4 * D,
                       image_size=S, patch_size=16, layer_norm_eps=1e-6, hidden_dropout_prob=0.0,
                       attention_probs_dropout_prob=0.0, hidden_act="gelu", qkv_bias=True)
    hf = tr.ViTModel(cfg, add_pooling_layer=False).double().eval()
    ref = ViTRef(D, depth, 1, 4 * D, S, "token").double()
    w = deterministic_weights([(k, tuple(p.shape)) for k, p in ref.named_timm_parameters()])
    ref.load_timm_state_dict(w)
    sd = {"embeddings.cls_token": w["cls_token"], "embeddings.position_embeddings": w["pos_embed"],
          "embeddings.patch_embeddings.projection.weight": w["patch_embed.proj.weight"],
          "embeddings.patch_embeddings.projection.bias": w["patch_embed.proj.bias"],
          "layernorm.weight": w["norm.weight"], "layernorm.bias": w["norm.bias"]}
    for i in range(depth):
        q, h = f"blocks.{i}.", f"layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):      # split the fused qkv Linear
            sd[h + f"attention.{n}.weight"] = w[q + "attn.qkv.weight"][j * D:(j + 1) * D]
            sd[h + f"attention.{n}.bias"] = w[q + "attn.qkv.bias"][j * D:(j + 1) * D]
        for a, b in (("attention.o_proj", "attn.proj"), ("layernorm_before", "norm1"), ("layernorm_after", "norm2"),
                     ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
            sd[h + a + ".weight"], sd[h + a + ".bias"] = w[q + b + ".weight"], w[q + b + ".bias"]
    assert set(sd) == set(hf.state_dict())
    hf.load_state_dict(sd)
    x = torch.randn(3, 3, S, S, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        want = hf(pixel_values=x).last_hidden_state
        got = ref.normed_tokens(x)
    assert got.shape == want.shape == (3, 5, D)
    assert (got - want).abs().max().item() < 1e-10


@pytest.mark.parametrize("pool", ["token", "avg"])
def test_state_dict_keys_are_timms(pool):
    from vlp_amd.vit import ViTTower
    t = ViTTower("vit_base_patch16_224", img_size=32, compute_dtype="fp32", device="cpu", depth=2, global_pool=pool)
    ref = ViTRef(768, 2, 12, 3072, 32, pool)
    ours = {k: tuple(v.shape) for k, v in t.state_dict().items()}
    want = {k: tuple(p.shape) for k, p in ref.named_timm_parameters()}
    assert list(ours) == list(want)          # timm's registration order too
    assert ours == want
    fn = "fc_norm" if pool == "avg" else "norm"
    assert (fn + ".weight" in ours) and (("norm.weight" if pool == "avg" else "fc_norm.weight") not in ours)
    assert t.seq == 5 and t.num_features == 768
    # parameters are views of the flat arena; timm's init: LayerNorm 1 / 0, zero Linear biases, tiny cls token
    assert t.cls_token.data_ptr() == t.arena.view("cls_token").data_ptr()
    assert torch.all(t.blocks[1].norm2.weight == 1) and torch.all(t.blocks[0].attn.qkv.bias == 0)
    assert t.cls_token.abs().max() < 1e-4 and 0.015 < t.pos_embed.std() < 0.025
    assert t.patch_embed.proj.bias.abs().max() <= 1 / 768 ** 0.5


@pytest.mark.parametrize("pool", ["token", "avg"])
def test_parameter_count_vit_base(pool):
    from vlp_amd.vit import ViTTower
    t = ViTTower("vit_base_patch16_224", compute_dtype="fp32", device="cpu", global_pool=pool)
    assert sum(p.numel() for p in t.parameters()) == 85_798_656
    assert t.seq == 197


def test_constructor_contract():
    from vlp_amd.vit import VIT_CFGS, ViTClassifier, ViTTower
    assert VIT_CFGS["vit_large_patch16_224"] == dict(dim=1024, depth=24, heads=16, mlp=4096)
    with pytest.raises(ValueError):
        ViTTower(img_size=40, device="cpu", depth=1)
    with pytest.raises(ValueError):
        ViTTower(img_size=32, device="cpu", depth=1, global_pool="max")
    t = ViTTower(img_size=32, device="cpu", depth=1, compute_dtype="fp32")
    with pytest.raises(ValueError, match="32x32"):
        t.run_forward(torch.zeros(1, 3, 48, 48), False)
    c = ViTClassifier(1, img_size=32, device="cpu", depth=1)
    assert c.global_pool == "token" and "norm.weight" in c.state_dict() and c.head.weight.shape == (1, 768)
    assert c.forward_head(torch.zeros(2, 768, 1, 1)).shape == (2, 1)


def _vlm(**kw):
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    args = dict(image_model="vit_base_patch16_224", text_encoder_model="tinybert",
                optimizer=functools.partial(torch.optim.AdamW, lr=5e-5), deduplicate=False, masked_loss=False,
                image_embedding_dim=768, text_embedding_dim=312, embedding_dim=128, device="cpu", image_size=32)
    args.update(kw)
    return VisionLanguageModule(**args)


def test_vision_language_module_constructs_with_vit():
    from vlp_amd.vit import ViTTower
    m = _vlm()
    t = m.image_encoder.model
    assert isinstance(t, ViTTower) and t.global_pool == "avg" and t.img_size == 32 and t.depth == 12
    keys = m.state_dict().keys()
    assert "image_encoder.model.fc_norm.weight" in keys and "image_encoder.model.blocks.11.mlp.fc2.bias" in keys
    assert "image_encoder.model.norm.weight" not in keys
    assert m.image_projection.shape == (768, 128)
    opt = m.configure_optimizers()["optimizer"]
    img = [g for g in opt.param_groups if g.get("name") == "image_encoder"][0]
    assert len(img["params"]) == 4 + 12 * 12 + 2


def test_vision_language_module_dimension_mismatch():
    with pytest.raises(ValueError, match="768"):
        _vlm(image_embedding_dim=512)


def test_image_encoder_names_the_supported_models():
    from src.models.pretrain.VisionLanguageModule import ImageEncoder
    with pytest.raises(ValueError, match="vit_base_patch16_224.*vit_large_patch16_224"):
        ImageEncoder("resnet50", device="cpu")


def test_vit_experiment_composes():
    from src.utils.config import compose
    c = compose("train", ["experiment=pretrain/pretrain_vit_base_16_tinybert_mi355x"])
    m = c["model"]
    assert m["image_model"] == "vit_base_patch16_224" and m["image_embedding_dim"] == 768
    assert m["image_size"] == 224 and c["data"]["image_size"] == 224
    assert m["text_encoder_model"] == "tinybert" and m["text_embedding_dim"] == 312
    assert m["compute_dtype"] == "bf16"
