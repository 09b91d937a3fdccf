"""The distilbert experiment through src/train.py's config boundary, on the CPU
(no kernel runs): composition, instantiation, HF key / parameter-count parity of
the DistilBERT tower, and the TinyBERT arena layout the new tower must not move."""
import hashlib
import json

import pytest
import torch

from src.utils.config import compose, instantiate


def test_compose_distilbert_experiments():
    c = compose("train", ["experiment=pretrain/pretrain_resnet34_distilbert"])
    assert c["data"]["_target_"] == "src.data.PretrainDataModule.PretrainDataModule"
    assert c["data"]["tokenizer"] == "distilbert" and c["data"]["batch_size"] == 128
    mc = c["model"]
    assert mc["_target_"] == "src.models.pretrain.VisionLanguageModule.VisionLanguageModule"
    assert (mc["image_model"], mc["text_encoder_model"]) == ("resnet34", "distilbert")
    assert (mc["image_embedding_dim"], mc["text_embedding_dim"], mc["embedding_dim"]) == (512, 768, 128)
    assert mc["deduplicate"] is False and mc["masked_loss"] is False
    assert mc["optimizer"]["lr"] == 5e-5 and c["trainer"]["max_epochs"] == 300
    assert mc["downstream_datamodule"]["_target_"] == "src.data.DownstreamDataModule.DownstreamDataModule"
    assert c["logger"]["wandb"]["name"] == "resnet34_distilbert"
    assert "precision" not in c["trainer"]
    c = compose("train", ["experiment=pretrain/pretrain_resnet34_distilbert_mi355x"])
    assert (c["data"]["batch_size"], c["data"]["image_size"], c["model"]["compute_dtype"]) == (256, 512, "bf16")
    assert (c["model"]["text_encoder_model"], c["model"]["text_embedding_dim"]) == ("distilbert", 768)
    assert c["data"]["tokenizer"] == "distilbert" and c["model"]["downstream_datamodule"] is None


def test_instantiate_distilbert_on_cpu():
    import src.train as T
    from vlp_amd.distilbert import DistilBertTower
    c = compose("train", ["experiment=pretrain/pretrain_resnet34_distilbert"])
    mc = T.model_config(c, (1.0, 1.0))
    assert mc["compute_dtype"] == "fp32"
    mc["downstream_datamodule"] = None
    m = instantiate(mc, device="cpu")
    tower = m.text_encoder.model
    assert isinstance(tower, DistilBertTower) and tower.compute_dtype == "fp32"
    cfg = tower.cfg
    assert (cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.vocab_size, cfg.max_pos) == (768, 6, 12, 3072, 30522, 512)
    assert (cfg.ln_eps, cfg.hidden_dropout, cfg.attention_dropout) == (1e-12, 0.1, 0.1)
    assert m.text_projection.shape == (768, 128)
    # HF DistilBertModel's key list, in its order, and its parameter count
    from transformers import DistilBertConfig, DistilBertModel
    hf = DistilBertModel(DistilBertConfig())
    keys = [k[len("text_encoder.model."):] for k in m.state_dict() if k.startswith("text_encoder.model.")]
    assert keys == list(hf.state_dict().keys())
    assert sum(p.numel() for p in tower.parameters()) == 66362880 == sum(p.numel() for p in hf.parameters())
    assert not any("token_type" in k or "pooler" in k for k in keys)
    # q/k/v weights, then q/k/v biases, contiguous: one [2304, 768] GEMM operand
    for i in (0, 5):
        o, n = tower.arena.span([f"transformer.layer.{i}.attention.{q}_lin.weight" for q in "qkv"])
        assert n == 3 * 768 * 768 and tower._qkv(tower.arena.data, i).shape == (2304, 768)
        ob, nb = tower.arena.span([f"transformer.layer.{i}.attention.{q}_lin.bias" for q in "qkv"])
        assert nb == 3 * 768 and ob == o + n
    # HF init: N(0, 0.02) weights and embeddings, zero biases, LayerNorm 1 / 0
    sd = tower.state_dict()
    assert abs(sd["transformer.layer.3.ffn.lin1.weight"].std().item() - 0.02) < 1e-3
    assert abs(sd["embeddings.word_embeddings.weight"].std().item() - 0.02) < 1e-3
    assert sd["transformer.layer.3.ffn.lin1.bias"].abs().max() == 0
    assert (sd["transformer.layer.2.sa_layer_norm.weight"] == 1).all()
    assert sd["transformer.layer.2.output_layer_norm.bias"].abs().max() == 0
    # a `distilbert.`-prefixed or a bare HF state dict loads; parameters stay arena views
    for prefix in ("distilbert.", ""):
        res = tower.load_hf_state_dict({prefix + k: v for k, v in hf.state_dict().items()})
        assert not res.missing_keys and not res.unexpected_keys
    w = tower.transformer.layer[1].attention.out_lin.weight
    assert torch.equal(w, hf.transformer.layer[1].attention.out_lin.weight)
    assert w.data_ptr() == tower.arena.view("transformer.layer.1.attention.out_lin.weight").data_ptr()
    # optimizer groups: the text tower is one group with its own learning rate
    m.hparams["text_encoder_lr"] = 1e-5
    groups = {g["name"]: g for g in m._configure_optimizer_parameters()}
    assert groups["text_encoder"]["lr"] == 1e-5 and len(groups["text_encoder"]["params"]) == 100


def test_small_config_and_dim_checks():
    from vlp_amd.distilbert import DistilBertConfig, DistilBertTower
    t = DistilBertTower(DistilBertConfig(0.0, 0.0, hidden=64, layers=1, heads=2, ffn=128, vocab_size=50, max_pos=16),
                        compute_dtype="fp32", device="cpu")
    assert sum(p.numel() for p in t.parameters()) == 50 * 64 + 16 * 64 + 2 * 64 + 4 * (64 * 64 + 64) \
        + 2 * 64 * 128 + 128 + 64 + 4 * 64
    with pytest.raises(ValueError):
        DistilBertConfig(hidden=100, heads=12)
    import functools
    from src.models.pretrain.VisionLanguageModule import TextEncoder, VisionLanguageModule
    opt = functools.partial(torch.optim.AdamW, lr=5e-5)
    with pytest.raises(ValueError, match="distilbert \\(768\\)"):
        VisionLanguageModule("resnet34", "distilbert", opt, False, False, text_embedding_dim=312, device="cpu")
    with pytest.raises(ValueError, match="tinybert \\(312\\)"):
        VisionLanguageModule("resnet34", "tinybert", opt, False, False, text_embedding_dim=768, device="cpu")
    with pytest.raises(ValueError, match="Supported models are: distilbert, tinybert"):
        TextEncoder("roberta", device="cpu")


def test_tinybert_arena_layout_unchanged():
    """TinyBertTower's state-dict keys and arena offsets are what they were before the
    drivers learnt DistilBERT's names (recorded from the parent revision)."""
    from vlp_amd.tinybert import TinyBertTower
    tb = TinyBertTower(device="cpu")
    lay = json.dumps([(k,) + tuple(v[:2]) for k, v in tb.arena.layout.items()])
    assert tb.arena.numel == 14350248
    assert hashlib.sha256(lay.encode()).hexdigest() == \
        "c4aa91865d306285f1ba32112ab96524f21bd72bc87306066d008811f6bc38f5"
    keys = list(tb.state_dict().keys())
    assert len(keys) == 71 and keys[2] == "embeddings.token_type_embeddings.weight"
    assert keys[5] == "encoder.layer.0.attention.self.query.weight" and keys[-1] == "pooler.dense.bias"
    assert tb.arena.layout["encoder.layer.0.attention.self.query.weight"][0] == (30522 + 512 + 2 + 2) * 312
