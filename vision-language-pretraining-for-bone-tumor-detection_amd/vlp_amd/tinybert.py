"""TinyBERT-4L-312D text tower on the HIP kernels (drop-in for
`AutoModel.from_pretrained("huawei-noah/TinyBERT_General_4L_312D")` wrapped by
TextEncoder, src/models/pretrain/VisionLanguageModule.py:38-60; the CLS hidden
state (token 0) is the sentence embedding, :52 / :60).

The encoder, its arena and its drivers are PostLNTextTower's (text_tower.py); this
module declares what is BERT's.  Parameter names are HF BertModel's (embeddings.*,
encoder.layer.{i}.*, pooler.dense.*), so `load_hf_state_dict` accepts a TinyBERT
checkpoint as is.  The pooler exists (it is in the reference's optimizer) but, as
in the reference, receives no gradient.  Query/key/value weights are laid out
contiguously in the arena so one [936, 312] GEMM computes all three.
"""
from __future__ import annotations

from .text_tower import PostLNTextTower, TextTowerFn  # noqa: F401  (TextTowerFn: imported from here)


class TinyBertConfig:
    vocab_size = 30522
    hidden = 312
    layers = 4
    heads = 12
    ffn = 1200
    max_pos = 512
    type_vocab = 2
    ln_eps = 1e-12

    def __init__(self, hidden_dropout=0.1, attention_dropout=0.1):
        self.hidden_dropout = float(hidden_dropout)
        self.attention_dropout = float(attention_dropout)


class TinyBertTower(PostLNTextTower):
    _LAYER = "encoder.layer.{}."
    _N = {"q": "attention.self.query", "k": "attention.self.key", "v": "attention.self.value",
          "ao": "attention.output.dense", "ln1": "attention.output.LayerNorm",
          "fc1": "intermediate.dense", "fc2": "output.dense", "ln2": "output.LayerNorm"}
    _TYPE_EMB = "embeddings.token_type_embeddings.weight"
    _DROP_AFTER_ATTN_OUT = True    # BertSelfOutput: dropout(dense(ctx)) + residual
    _HF_PREFIX = "bert."

    def __init__(self, config: TinyBertConfig = None, compute_dtype: str = "bf16", device=None):
        super().__init__(config or TinyBertConfig(), compute_dtype, device)

    def _tail_specs(self):
        D = self.cfg.hidden
        return [("pooler.dense.weight", (D, D)), ("pooler.dense.bias", (D,))]

    def grads_for_autograd(self, existing=None):
        out = super().grads_for_autograd()
        # pooler receives no gradient (only the CLS hidden state is used, :52/:60)
        for j, (owner, attr, full) in enumerate(self._param_slots):
            if full.startswith("pooler."):
                out[j] = None
        return out
