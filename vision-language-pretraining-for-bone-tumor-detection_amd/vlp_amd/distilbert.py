"""DistilBERT text tower on the HIP kernels (drop-in for
`DistilBertModel.from_pretrained("distilbert-base-uncased")` wrapped by
TextEncoder, src/models/pretrain/VisionLanguageModule.py:43, :57-60: the
reference's default text encoder; the CLS hidden state is the sentence embedding).

The encoder block is the post-LN BERT block PostLNTextTower drives (text_tower.py),
so this module only declares what is DistilBERT's (transformers modeling_distilbert):
  * parameter names and their order are HF DistilBertModel's (embeddings.*,
    transformer.layer.{i}.{attention.{q,k,v,out}_lin, sa_layer_norm,
    ffn.{lin1,lin2}, output_layer_norm}); no token-type table, no pooler;
  * dropout sits after the embedding LayerNorm, on the attention
    probabilities and after ffn.lin2, and NOT after attention.out_lin;
  * hidden 768, 12 heads of 64, FFN 3072, 6 layers.
Query/key/value weights are contiguous in the arena (then their biases), so one
[2304, 768] GEMM computes all three.
"""
from __future__ import annotations

from .text_tower import PostLNTextTower


class DistilBertConfig:
    """HF DistilBertConfig() defaults; every size can be overridden (tests use
    fewer layers)."""

    def __init__(self, dropout=0.1, attention_dropout=0.1, vocab_size=30522, hidden=768, layers=6, heads=12,
                 ffn=3072, max_pos=512, ln_eps=1e-12):
        if hidden % heads:
            raise ValueError(f"DistilBertConfig: hidden {hidden} is not a multiple of heads {heads}")
        self.vocab_size, self.hidden, self.layers, self.heads = int(vocab_size), int(hidden), int(layers), int(heads)
        self.ffn, self.max_pos, self.ln_eps = int(ffn), int(max_pos), float(ln_eps)
        self.type_vocab = 0
        self.hidden_dropout = float(dropout)            # DistilBertConfig.dropout
        self.attention_dropout = float(attention_dropout)


class DistilBertTower(PostLNTextTower):
    _LAYER = "transformer.layer.{}."
    _N = {"q": "attention.q_lin", "k": "attention.k_lin", "v": "attention.v_lin",
          "ao": "attention.out_lin", "ln1": "sa_layer_norm",
          "fc1": "ffn.lin1", "fc2": "ffn.lin2", "ln2": "output_layer_norm"}
    _TYPE_EMB = None
    _DROP_AFTER_ATTN_OUT = False   # TransformerBlock: sa_layer_norm(out_lin(ctx) + x), no dropout
    _HF_PREFIX = "distilbert."

    def __init__(self, config: DistilBertConfig = None, compute_dtype: str = "bf16", device=None):
        super().__init__(config or DistilBertConfig(), compute_dtype, device)
