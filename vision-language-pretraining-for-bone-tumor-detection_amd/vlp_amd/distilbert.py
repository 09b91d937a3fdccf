"""DistilBERT text tower on the HIP kernels (drop-in for
`DistilBertModel.from_pretrained("distilbert-base-uncased")` wrapped by
TextEncoder, src/models/pretrain/VisionLanguageModule.py:43, :57-60: the
reference's default text encoder; the CLS hidden state is the sentence embedding).

The encoder block is the post-LN BERT block TinyBertTower drives, so this
tower reuses its forward / backward drivers and only maps names.  What differs
(transformers modeling_distilbert):
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

import torch
import torch.nn as nn

from .tinybert import TinyBertTower, _Holder


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


class DistilBertTower(TinyBertTower):
    _LAYER = "transformer.layer.{}."
    _N = {"q": "attention.q_lin", "k": "attention.k_lin", "v": "attention.v_lin",
          "ao": "attention.out_lin", "ln1": "sa_layer_norm",
          "fc1": "ffn.lin1", "fc2": "ffn.lin2", "ln2": "output_layer_norm"}
    _TYPE_EMB = None
    _DROP_AFTER_ATTN_OUT = False   # TransformerBlock: sa_layer_norm(out_lin(ctx) + x), no dropout
    _HF_PREFIX = "distilbert."

    def __init__(self, config: DistilBertConfig = None, compute_dtype: str = "bf16", device=None):
        nn.Module.__init__(self)
        cfg = config or DistilBertConfig()
        self.cfg = cfg
        self.compute_dtype = compute_dtype
        D, F, N = cfg.hidden, cfg.ffn, self._N
        specs = [("embeddings.word_embeddings.weight", (cfg.vocab_size, D)),
                 ("embeddings.position_embeddings.weight", (cfg.max_pos, D)),
                 ("embeddings.LayerNorm.weight", (D,)), ("embeddings.LayerNorm.bias", (D,))]
        order = []   # HF registration order (q, k, v, out interleave weight / bias), not the arena's
        for i in range(cfg.layers):
            p = self._LAYER.format(i)
            # q/k/v weights then q/k/v biases: contiguous for the fused QKV GEMM
            specs += [(p + N[n] + ".weight", (D, D)) for n in ("q", "k", "v")]
            specs += [(p + N[n] + ".bias", (D,)) for n in ("q", "k", "v")]
            specs += [(p + N["ao"] + ".weight", (D, D)), (p + N["ao"] + ".bias", (D,)),
                      (p + N["ln1"] + ".weight", (D,)), (p + N["ln1"] + ".bias", (D,)),
                      (p + N["fc1"] + ".weight", (F, D)), (p + N["fc1"] + ".bias", (F,)),
                      (p + N["fc2"] + ".weight", (D, F)), (p + N["fc2"] + ".bias", (D,)),
                      (p + N["ln2"] + ".weight", (D,)), (p + N["ln2"] + ".bias", (D,))]
            order += [p + N[n] + s for n in ("q", "k", "v", "ao", "ln1", "fc1", "fc2", "ln2")
                      for s in (".weight", ".bias")]
        self._init_arena_packed(specs, device)
        for name, _ in specs[:4]:
            self._register_path(name)
        for name in order:
            self._register_path(name)
        self.reset_parameters()
        self._seed = 0x5EED
        self._ws = {}

    def _register_path(self, full):
        """Register arena view `full` as a parameter at its dotted path, creating
        the holder modules on the way (a numbered child makes its parent a
        ModuleList, as in HF's `transformer.layer`)."""
        parts = full.split(".")
        owner = self
        for j, part in enumerate(parts[:-1]):
            nxt = owner._modules.get(part)
            if nxt is None:
                nxt = nn.ModuleList() if parts[j + 1].isdigit() else _Holder()
                owner.add_module(part, nxt)
            owner = nxt
        self._register(owner, parts[-1], full)

    @torch.no_grad()
    def reset_parameters(self):
        """HF DistilBertPreTrainedModel._init_weights: N(0, 0.02) weights/embeddings,
        zero biases, LayerNorm 1/0 (the 1-D weights are the LayerNorm gains)."""
        for name, (o, n, shape) in self.arena.layout.items():
            v = self.arena.view(name)
            if name.endswith("bias"):
                v.zero_()
            elif len(shape) == 1:
                v.fill_(1.0)
            else:
                v.normal_(0.0, 0.02)

    def grads_for_autograd(self, existing=None):
        return super(TinyBertTower, self).grads_for_autograd()   # no pooler to leave out
