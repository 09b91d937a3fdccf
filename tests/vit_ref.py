"""Plain-torch restatement of timm's VisionTransformer (patch 16, qkv_bias, pre-norm
blocks, erf GELU, LayerNorm eps 1e-6, no layer-scale / DropPath / dropout) with
timm's parameter names: the reference the ViT tests hold vlp_amd.vit.ViTTower to
(run in fp64).  tests/test_vit_cpu.py holds this restatement itself to
transformers.ViTModel.

`act` / `wq` are the precision hooks of the tolerance measurement: act(t) rounds
every activation the HIP tower stores, wq(w) every GEMM weight operand (identity
by default; bf16 round trips for the bf16 budget).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def _id(t):
    return t


class ViTRef(nn.Module):
    def __init__(self, dim=768, depth=12, heads=12, mlp=3072, img_size=224, global_pool="token", patch=16):
        super().__init__()
        assert global_pool in ("token", "avg")
        self.dim, self.depth, self.heads, self.patch, self.global_pool = dim, depth, heads, patch, global_pool
        self.seq = (img_size // patch) ** 2 + 1
        P = {"cls_token": (1, 1, dim), "pos_embed": (1, self.seq, dim),
             "patch_embed.proj.weight": (dim, 3, patch, patch), "patch_embed.proj.bias": (dim,)}
        for i in range(depth):
            q = f"blocks.{i}."
            P.update({q + "norm1.weight": (dim,), q + "norm1.bias": (dim,),
                      q + "attn.qkv.weight": (3 * dim, dim), q + "attn.qkv.bias": (3 * dim,),
                      q + "attn.proj.weight": (dim, dim), q + "attn.proj.bias": (dim,),
                      q + "norm2.weight": (dim,), q + "norm2.bias": (dim,),
                      q + "mlp.fc1.weight": (mlp, dim), q + "mlp.fc1.bias": (mlp,),
                      q + "mlp.fc2.weight": (dim, mlp), q + "mlp.fc2.bias": (dim,)})
        fn = "fc_norm" if global_pool == "avg" else "norm"
        P.update({fn + ".weight": (dim,), fn + ".bias": (dim,)})
        self.final_norm = fn
        self.names = list(P)
        # flat registration under mangled names; state_dict() / load_state_dict() speak timm's
        self.p = nn.ParameterDict({k.replace(".", "/"): nn.Parameter(torch.zeros(s)) for k, s in P.items()})

    def timm_state_dict(self):
        return {k: self.p[k.replace(".", "/")].detach().clone() for k in self.names}

    def load_timm_state_dict(self, sd):
        assert set(sd) == set(self.names), set(sd) ^ set(self.names)
        with torch.no_grad():
            for k in self.names:
                self.p[k.replace(".", "/")].copy_(sd[k])

    def named_timm_parameters(self):
        return [(k, self.p[k.replace(".", "/")]) for k in self.names]

    def g(self, k):
        return self.p[k.replace(".", "/")]

    def tokens(self, x, act=_id, wq=_id):
        """[B,3,S,S] -> the last block's output tokens [B, N, dim] (before the final norm)."""
        g, D, H = self.g, self.dim, self.heads
        B = x.shape[0]
        pe = act(F.conv2d(act(x), wq(g("patch_embed.proj.weight")), g("patch_embed.proj.bias"), stride=self.patch))
        pe = pe.flatten(2).transpose(1, 2)                                   # [B, P, D]
        h = act(torch.cat([g("cls_token").expand(B, -1, -1), pe], 1) + g("pos_embed"))
        N = h.shape[1]
        for i in range(self.depth):
            q = f"blocks.{i}."
            y = act(F.layer_norm(h, (D,), g(q + "norm1.weight"), g(q + "norm1.bias"), 1e-6))
            qkv = act(F.linear(y, wq(g(q + "attn.qkv.weight")), g(q + "attn.qkv.bias")))
            qh, kh, vh = qkv.view(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)   # [B, H, N, dh]
            p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(D // H), -1)
            o = act((p @ vh).transpose(1, 2).reshape(B, N, D))
            h = act(h + F.linear(o, wq(g(q + "attn.proj.weight")), g(q + "attn.proj.bias")))
            y = act(F.layer_norm(h, (D,), g(q + "norm2.weight"), g(q + "norm2.bias"), 1e-6))
            a = act(F.gelu(act(F.linear(y, wq(g(q + "mlp.fc1.weight")), g(q + "mlp.fc1.bias")))))
            h = act(h + F.linear(a, wq(g(q + "mlp.fc2.weight")), g(q + "mlp.fc2.bias")))
        return h

    def normed_tokens(self, x):
        """timm forward_features with global_pool="token": the final norm over every token."""
        fn = self.final_norm
        return F.layer_norm(self.tokens(x), (self.dim,), self.g(fn + ".weight"), self.g(fn + ".bias"), 1e-6)

    def forward(self, x, act=_id, wq=_id):
        """[B,3,S,S] -> pooled features [B, dim] (timm forward_head(pre_logits=True))."""
        h = self.tokens(x, act, wq)
        fn = self.final_norm
        pooled = act(h[:, 0] if self.global_pool == "token" else h[:, 1:].mean(1))
        return act(F.layer_norm(pooled, (self.dim,), self.g(fn + ".weight"), self.g(fn + ".bias"), 1e-6))


def bf16_round(t):
    """Round to bf16 and back, keeping the dtype and the autograd graph (straight-through)."""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


def deterministic_weights(names_shapes, seed=0):
    """Name-keyed deterministic weights: each tensor from a generator seeded by its name,
    scaled so activations stay O(1) (LayerNorm weights near 1, the rest small)."""
    import zlib
    out = {}
    for k, shape in names_shapes:
        g = torch.Generator().manual_seed(zlib.crc32(k.encode()) + seed)
        t = torch.randn(shape, generator=g, dtype=torch.float64)
        if "norm" in k and k.endswith("weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith("bias"):
            t = 0.05 * t
        elif k in ("cls_token", "pos_embed"):
            t = 0.2 * t
        else:
            fan_in = math.prod(shape[1:])
            t = t / math.sqrt(fan_in)
        out[k] = t
    return out
