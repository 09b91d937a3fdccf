"""The post-LN BERT encoder both text towers are (TinyBertTower, DistilBertTower), on the HIP
kernels: the packed parameter arena, one encoder-layer forward, one encoder-layer backward and
the drivers around them.  A tower declares its HF parameter names and what differs (token-type
table, dropout after the attention output, a tail such as BERT's pooler); see tinybert.py and
distilbert.py.

One layer (`_layer_forward`, mirrored by `_layer_backward`) is nine launches:
  QKV GEMM, attention                                            on all M = B*T token rows,
  attention-output GEMM (+residual, dropout), LayerNorm,
  FFN GEMM (GELU), FFN GEMM (+residual, dropout), LayerNorm      on the layer's row set.
The row set (`_Rows`) is every token row, or, for the last layer under cls_only, the B CLS rows
(row b*T of every [B*T, .] tensor), read in place through the GEMMs' leading dimension T*D: the
caller (VisionLanguageModule TextEncoder, :57-60) reads token 0 only, and only the last layer's
keys and values need every token.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch
import torch.nn as nn

from . import ops
from .arena import ArenaModule, ParamArena

# one linear or LayerNorm of a layer: the operand weight (compute dtype for a GEMM, fp32 for a
# LayerNorm gain), the fp32 bias (forward only), and their gradient-arena views (backward only)
_Lin = namedtuple("_Lin", "w b gw gb")
# one encoder layer's _Lin per role; qkv is the fused [3D, D] operand
_Layer = namedtuple("_Layer", "qkv ao ln1 fc1 fc2 ln2")
# the rows a layer works on after attention: n of them, ld apart (None: dense, the default)
_Rows = namedtuple("_Rows", "n ld")


class _Holder(nn.Module):
    pass


class PostLNTextTower(ArenaModule):
    # what a tower declares: arena (= HF) names of one encoder layer, by role
    _LAYER = None                  # "encoder.layer.{}."
    _N = None                      # {"q", "k", "v", "ao", "ln1", "fc1", "fc2", "ln2"} -> name under _LAYER
    _TYPE_EMB = None               # the token-type table's name; None: no such table
    _DROP_AFTER_ATTN_OUT = False   # dropout(dense(ctx)) + residual, or no dropout there
    _HF_PREFIX = ""                # stripped from checkpoint keys

    def __init__(self, cfg, compute_dtype: str = "bf16", device=None):
        super().__init__()
        self.cfg = cfg
        self.compute_dtype = compute_dtype
        D, F, N = cfg.hidden, cfg.ffn, self._N
        specs = [("embeddings.word_embeddings.weight", (cfg.vocab_size, D)),
                 ("embeddings.position_embeddings.weight", (cfg.max_pos, D))]
        if self._TYPE_EMB:
            specs.append((self._TYPE_EMB, (cfg.type_vocab, D)))
        specs += [("embeddings.LayerNorm.weight", (D,)), ("embeddings.LayerNorm.bias", (D,))]
        order = [name for name, _ in specs]   # HF registration order: interleaves q/k/v weight and bias
        rest = {"ao": (D, D), "ln1": (D,), "fc1": (F, D), "fc2": (D, F), "ln2": (D,)}
        for i in range(cfg.layers):
            p = self._LAYER.format(i)
            # q/k/v weights then q/k/v biases: contiguous for the fused QKV GEMM
            specs += [(p + N[n] + ".weight", (D, D)) for n in ("q", "k", "v")]
            specs += [(p + N[n] + ".bias", (D,)) for n in ("q", "k", "v")]
            for n, shape in rest.items():
                specs += [(p + N[n] + ".weight", shape), (p + N[n] + ".bias", shape[:1])]
            order += [p + N[n] + s for n in ("q", "k", "v", *rest) for s in (".weight", ".bias")]
        tail = self._tail_specs()
        specs += tail
        order += [name for name, _ in tail]
        # no alignment padding: the q/k/v groups must be contiguous
        self.arena = ParamArena(specs, device=device, align=1)
        self._param_slots = []
        for name in order:
            self._register_path(name)
        self.reset_parameters()
        self._seed = 0x5EED
        self._ws = {}

    def _tail_specs(self):
        """Parameters after the encoder (arena specs, in HF order)."""
        return []

    def _register_path(self, full):
        """Register arena view `full` as a parameter at its dotted path, creating
        the holder modules on the way (a numbered child makes its parent a
        ModuleList, as in HF's `encoder.layer` / `transformer.layer`)."""
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
        """HF (Distil)BertPreTrainedModel._init_weights: N(0, 0.02) weights/embeddings,
        zero biases, LayerNorm 1/0 (the 1-D weights are the LayerNorm gains)."""
        for name, (o, n, shape) in self.arena.layout.items():
            v = self.arena.view(name)
            if name.endswith("bias"):
                v.zero_()
            elif len(shape) == 1:
                v.fill_(1.0)
            else:
                v.normal_(0.0, 0.02)

    def _after_apply(self):
        self._ws = {}

    @property
    def tdtype(self):
        return torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32

    def load_hf_state_dict(self, sd):
        """Load the HF model's state dict, bare or under the task models' prefix."""
        pre = self._HF_PREFIX
        sd = {k[len(pre):] if k.startswith(pre) else k: v for k, v in sd.items()}
        return self.load_state_dict({k: v for k, v in sd.items() if k in self.state_dict()}, strict=False)

    def _wcopy(self):
        """Compute-dtype copy of the whole arena (one cast launch; same offsets)."""
        if self.compute_dtype == "fp32":
            return self.arena.data
        key = ("wT", str(self.arena.data.device))
        buf = self._ws.get(key)
        if buf is None:
            buf = torch.empty(self.arena.numel, dtype=self.tdtype, device=self.arena.data.device)
            self._ws[key] = buf
        ops.cast(self.arena.data, buf)
        return buf

    def _qkv(self, wT, i, bias=False, grad=False):
        p = self._LAYER.format(i)
        names = [p + self._N[n] + (".bias" if bias else ".weight") for n in ("q", "k", "v")]
        o, n = self.arena.span(names)
        D = self.cfg.hidden
        buf = self.arena.grad if grad else wT
        t = buf[o:o + n]
        return t if bias else t.view(3 * D, D)

    def _layer(self, i, wT, grad=False):
        """Layer i's views: operand weights from wT and fp32 biases, or with `grad` operand
        weights and the gradient views."""
        A, p = self.arena, self._LAYER.format(i)

        def lin(n, src):
            w, b = p + self._N[n] + ".weight", p + self._N[n] + ".bias"
            if grad:
                return _Lin(A.view(w, src), None, A.gview(w), A.gview(b))
            return _Lin(A.view(w, src), A.view(b), None, None)
        if grad:
            qkv = _Lin(self._qkv(wT, i), None, self._qkv(None, i, grad=True), self._qkv(None, i, bias=True, grad=True))
        else:
            qkv = _Lin(self._qkv(wT, i), self._qkv(A.data, i, bias=True), None, None)
        return _Layer(qkv, lin("ao", wT), lin("ln1", None), lin("fc1", wT), lin("fc2", wT), lin("ln2", None))

    def _rows(self, sv, i):
        """Layer i's row set: the CLS rows for the last layer under cls_only, else every row."""
        if sv["cls_only"] and i == self.cfg.layers - 1:
            return _Rows(sv["B"], sv["Tn"] * self.cfg.hidden)
        return _Rows(sv["B"] * sv["Tn"], None)

    # ---------------- forward ----------------
    def run_forward(self, input_ids, attention_mask=None, token_type_ids=None, training=True, cls_only=False):
        """Returns (h, saved).  h = the last hidden state [B*T, D], or with
        cls_only the CLS rows only, [B, D]: the last encoder layer then runs its
        attention-output, LayerNorm and FFN work on the B CLS rows (its keys and
        values still cover every token)."""
        cfg = self.cfg
        D = cfg.hidden
        dev = self.arena.data.device
        T = self.tdtype
        B, Tn = input_ids.shape
        M = B * Tn
        ids = input_ids.contiguous().to(device=dev, dtype=torch.long)
        tt = None if token_type_ids is None or not self._TYPE_EMB else token_type_ids.contiguous().to(device=dev, dtype=torch.long)
        am = None if attention_mask is None else attention_mask.contiguous().to(device=dev, dtype=torch.long)
        wT = self._wcopy()
        p_h = cfg.hidden_dropout if training else 0.0
        p_a = cfg.attention_dropout if training else 0.0
        p_o = p_h if self._DROP_AFTER_ATTN_OUT else 0.0
        self._seed = (self._seed * 6364136223846793005 + 1442695040888963407) % (2 ** 63)
        seed = self._seed
        sv = {"B": B, "Tn": Tn, "ids": ids, "tt": tt, "seed": seed, "p_h": p_h, "p_a": p_a, "p_o": p_o,
              "wT": wT, "cls_only": cls_only}
        e = torch.empty(M, D, dtype=T, device=dev)
        ops.embed_fwd(ids, tt, self.arena.view("embeddings.word_embeddings.weight"),
                      self.arena.view("embeddings.position_embeddings.weight"),
                      self.arena.view(self._TYPE_EMB) if self._TYPE_EMB else None, e, M, Tn, D)
        h = torch.empty(M, D, dtype=T, device=dev)
        mu = torch.empty(M, device=dev)
        rs = torch.empty(M, device=dev)
        ops.layernorm_fwd(e, self.arena.view("embeddings.LayerNorm.weight"),
                          self.arena.view("embeddings.LayerNorm.bias"), cfg.ln_eps, h, mu, rs, M, D,
                          p=p_h, seed=seed + 1)
        sv["emb"] = (e, mu, rs)
        sv["layers"] = []
        for i in range(cfg.layers):
            sv["layers"].append(self._layer_forward(i, h, am, sv, self._rows(sv, i)))
            h = sv["layers"][-1]["h2"]
        sv["h_last"] = h
        return h, sv

    def _layer_forward(self, i, h, am, sv, rows):
        """Encoder layer i on the layer input h [B*T, D]; returns what its backward reads, with
        the layer output [rows.n, D] as "h2"."""
        cfg = self.cfg
        D, Fd, H = cfg.hidden, cfg.ffn, cfg.heads
        dh = D // H
        T, dev = self.tdtype, self.arena.data.device
        B, Tn = sv["B"], sv["Tn"]
        M = B * Tn
        R, ld = rows
        W = self._layer(i, sv["wT"])
        s_i = sv["seed"] + 100 * (i + 1)
        qkv = torch.empty(M, 3 * D, dtype=T, device=dev)
        ops.linear_fwd(h, W.qkv.w, W.qkv.b, qkv, M, 3 * D, D)
        ctx = torch.empty(M, D, dtype=T, device=dev)
        P = torch.empty(B, H, Tn, Tn, device=dev)
        ops.attn_fwd(qkv, am, ctx, P, B, Tn, H, dh, 1.0 / math.sqrt(dh), p=sv["p_a"], seed=s_i + 1)
        # from here on the row set: ctx and the residual h are read ld apart
        s1 = torch.empty(R, D, dtype=T, device=dev)
        ops.linear_fwd(ctx, W.ao.w, W.ao.b, s1, R, D, D, ldx=ld, mode=2, res=h, ldr=ld, p=sv["p_o"], seed=s_i + 2)
        h1 = torch.empty(R, D, dtype=T, device=dev)
        mu1 = torch.empty(R, device=dev)
        rs1 = torch.empty(R, device=dev)
        ops.layernorm_fwd(s1, W.ln1.w, W.ln1.b, cfg.ln_eps, h1, mu1, rs1, R, D)
        u = torch.empty(R, Fd, dtype=T, device=dev)
        f = torch.empty(R, Fd, dtype=T, device=dev)
        ops.linear_fwd(h1, W.fc1.w, W.fc1.b, f, R, Fd, D, mode=1, aux=u)
        s2 = torch.empty(R, D, dtype=T, device=dev)
        ops.linear_fwd(f, W.fc2.w, W.fc2.b, s2, R, D, Fd, mode=2, res=h1, p=sv["p_h"], seed=s_i + 3)
        h2 = torch.empty(R, D, dtype=T, device=dev)
        mu2 = torch.empty(R, device=dev)
        rs2 = torch.empty(R, device=dev)
        ops.layernorm_fwd(s2, W.ln2.w, W.ln2.b, cfg.ln_eps, h2, mu2, rs2, R, D)
        return {"h": h, "qkv": qkv, "ctx": ctx, "P": P, "s1": s1, "mu1": mu1, "rs1": rs1, "h1": h1, "u": u,
                "f": f, "s2": s2, "mu2": mu2, "rs2": rs2, "h2": h2, "seed": s_i}

    # ---------------- backward ----------------
    def run_backward(self, sv, dcls):
        """dcls: [B, D] gradient of the CLS hidden states (any dtype).  Zeroes and
        fills the grad arena (a tail such as the pooler keeps a zero gradient: unused)."""
        cfg = self.cfg
        D = cfg.hidden
        dev = self.arena.data.device
        T = self.tdtype
        B, Tn = sv["B"], sv["Tn"]
        M = B * Tn
        G = self.arena
        G.grad.zero_()
        if sv["cls_only"]:
            dy = dcls.to(T).contiguous()
        else:
            dy = torch.zeros(M, D, dtype=T, device=dev)
            ops.scatter_rows(dcls.to(T).contiguous(), dy, B, D, D, Tn * D)
        for i in range(cfg.layers - 1, -1, -1):
            dy = self._layer_backward(i, sv["layers"][i], dy, sv, self._rows(sv, i))
        e, mu, rs = sv["emb"]
        de = torch.empty(M, D, dtype=T, device=dev)
        ops.layernorm_bwd(dy, e, mu, rs, self.arena.view("embeddings.LayerNorm.weight"), de, None,
                          G.gview("embeddings.LayerNorm.weight"), G.gview("embeddings.LayerNorm.bias"),
                          M, D, p_out=sv["p_h"], seed_out=sv["seed"] + 1)
        ops.embed_bwd(sv["ids"], sv["tt"], de, G.gview("embeddings.word_embeddings.weight"),
                      G.gview("embeddings.position_embeddings.weight"),
                      G.gview(self._TYPE_EMB) if self._TYPE_EMB else None, M, Tn, D)

    def _layer_backward(self, i, Ls, dy, sv, rows):
        """Backward of _layer_forward: dy [rows.n, D] is the gradient of the layer output;
        returns the gradient of the layer input [B*T, D]."""
        cfg = self.cfg
        D, Fd, H = cfg.hidden, cfg.ffn, cfg.heads
        dh = D // H
        T, dev = self.tdtype, self.arena.data.device
        B, Tn = sv["B"], sv["Tn"]
        M = B * Tn
        R, ld = rows
        W = self._layer(i, sv["wT"], grad=True)
        s_i = Ls["seed"]
        # output LayerNorm: ds2 (residual) and dz = ds2 * dropout mask
        ds2 = torch.empty(R, D, dtype=T, device=dev)
        dz = torch.empty(R, D, dtype=T, device=dev)
        ops.layernorm_bwd(dy, Ls["s2"], Ls["mu2"], Ls["rs2"], W.ln2.w, ds2, dz, W.ln2.gw, W.ln2.gb,
                          R, D, p_in=sv["p_h"], seed_in=s_i + 3)
        ops.colsum(dz, W.fc2.gb, R, D)
        ops.linear_wgrad(dz, Ls["f"], W.fc2.gw, R, D, Fd)
        du = torch.empty(R, Fd, dtype=T, device=dev)
        ops.linear_dgrad(dz, W.fc2.w, du, R, Fd, D, mode=1, aux=Ls["u"])
        ops.colsum(du, W.fc1.gb, R, Fd)
        ops.linear_wgrad(du, Ls["h1"], W.fc1.gw, R, Fd, D)
        dh1 = torch.empty(R, D, dtype=T, device=dev)
        ops.linear_dgrad(du, W.fc1.w, dh1, R, D, Fd, addend=ds2)
        # attention output LayerNorm
        ds1 = torch.empty(R, D, dtype=T, device=dev)
        da = torch.empty(R, D, dtype=T, device=dev)
        ops.layernorm_bwd(dh1, Ls["s1"], Ls["mu1"], Ls["rs1"], W.ln1.w, ds1, da, W.ln1.gw, W.ln1.gb,
                          R, D, p_in=sv["p_o"], seed_in=s_i + 2)
        ops.colsum(da, W.ao.gb, R, D)
        ops.linear_wgrad(da, Ls["ctx"], W.ao.gw, R, D, D, ldx=ld)
        # back to all M rows.  On the CLS rows only the CLS queries receive a context
        # gradient: dctx starts as zeros and is written ld apart
        dctx = (torch.zeros if ld else torch.empty)(M, D, dtype=T, device=dev)
        ops.linear_dgrad(da, W.ao.w, dctx, R, D, D, lddx=ld)
        dqkv = torch.empty(M, 3 * D, dtype=T, device=dev)
        ops.attn_bwd(Ls["qkv"], Ls["P"], dctx, dqkv, B, Tn, H, dh, 1.0 / math.sqrt(dh), p=sv["p_a"], seed=s_i + 1)
        ops.colsum(dqkv, W.qkv.gb, M, 3 * D)
        ops.linear_wgrad(dqkv, Ls["h"], W.qkv.gw, M, 3 * D, D)
        if ld:
            # the residual gradient ds1 reaches the CLS rows of the layer input
            ds1_rows, ds1 = ds1, torch.zeros(M, D, dtype=T, device=dev)
            ops.scatter_rows(ds1_rows, ds1, R, D, D, ld)
        dx = torch.empty(M, D, dtype=T, device=dev)
        ops.linear_dgrad(dqkv, W.qkv.w, dx, M, D, 3 * D, addend=ds1)
        return dx

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, **kw):
        """API forward: returns the last hidden state [B, T, D] (fp32) like
        (Distil)BertModel(...).last_hidden_state."""
        return TextTowerFn.apply(self, input_ids, attention_mask, token_type_ids,
                                 *self.params_in_arena_order())


class TextTowerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tower, input_ids, attention_mask, token_type_ids, *params):
        h, sv = tower.run_forward(input_ids, attention_mask, token_type_ids, tower.training)
        ctx.tower, ctx.sv = tower, sv
        B, Tn = input_ids.shape
        return h.view(B, Tn, -1).float()

    @staticmethod
    def backward(ctx, dh):
        tower = ctx.tower
        # the API path gives a full [B,T,D] gradient; only CLS rows are non-zero in
        # the VLP model, but support the general case by scattering all rows
        dcls_rows = dh[:, 0, :].contiguous()
        if dh[:, 1:, :].abs().sum().item() != 0:  # pragma: no cover - generic last_hidden_state use
            raise NotImplementedError(f"{type(tower).__name__} backward supports gradients on the CLS token only")
        tower.begin_backward()
        tower.run_backward(ctx.sv, dcls_rows)
        ctx.sv = None
        return (None, None, None, None, *tower.grads_for_autograd())
