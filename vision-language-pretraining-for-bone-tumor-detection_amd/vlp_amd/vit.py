"""ViT-B/16 and ViT-L/16 image towers on the HIP kernels (drop-in for
`timm.create_model("vit_base_patch16_224", pretrained=False, num_classes=0,
global_pool="avg", ...)` behind ImageEncoder,
src/models/pretrain/VisionLanguageModule.py:27-35, and for the
`num_classes=1` classifier of src/models/baseline/OnlyImagingModule.py:73).

timm is not installed: the published architecture is restated (parity with
timm itself is unpinned, as for ResNet34 and NesT; tests/vit_ref.py is the
plain-torch restatement the tests hold this tower to, itself held to
transformers.ViTModel).  Parameter names are timm's, so a timm checkpoint loads
key for key.
  tokens   = [cls_token ; patch-embed GEMM of the 16x16/16 im2col (+ bias)] + pos_embed
  block    = x + proj(attn(qkv(LN1(x))));  x + fc2(GELU_erf(fc1(LN2(x))))
             (qkv_bias, LayerNorm eps 1e-6, no layer-scale, no DropPath / dropout)
  head     global_pool="token" (timm's default; what num_classes=1 uses):
             `norm` over the tokens, features = the class row;
           global_pool="avg" (the pretraining ImageEncoder's): mean over the
             patch tokens, then `fc_norm` (timm keys the final LayerNorm
             `fc_norm.*` instead of `norm.*` in this mode).
Attention runs the flash-attention kernels of csrc/nest_ops.hip at head dim 64
(vlp_vit_attn_*, scores never stored); its head-major output is timm's own
order, so the proj weight is used as stored.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops
from .arena import ArenaModule

VIT_CFGS = {
    "vit_base_patch16_224": dict(dim=768, depth=12, heads=12, mlp=3072),
    "vit_large_patch16_224": dict(dim=1024, depth=24, heads=16, mlp=4096),
}
LN_EPS = 1e-6
PATCH = 16
KP = 3 * PATCH * PATCH          # im2col width: (c, ky, kx)


class _Holder(nn.Module):
    pass


class ViTTower(ArenaModule):
    def __init__(self, variant="vit_base_patch16_224", img_size=224, drop_rate=0.0, compute_dtype="bf16",
                 device=None, depth=None, global_pool="avg"):
        super().__init__()
        cfg = VIT_CFGS[variant]
        self.variant = variant
        self.img_size = int(img_size)
        if self.img_size < PATCH or self.img_size % PATCH:
            raise ValueError(f"ViTTower: img_size {img_size} must be a multiple of {PATCH}")
        if global_pool not in ("token", "avg"):
            raise ValueError(f"ViTTower: global_pool {global_pool!r} (token or avg)")
        self.dim, self.heads, self.mlp = cfg["dim"], cfg["heads"], cfg["mlp"]
        self.depth = int(depth) if depth is not None else cfg["depth"]
        if self.dim // self.heads != 64:
            raise ValueError("ViTTower: 64-channel heads (vlp_vit_attn_*)")
        self.global_pool = global_pool
        self.final_norm = "fc_norm" if global_pool == "avg" else "norm"
        self.num_features = self.dim
        self.drop_rate = float(drop_rate)
        self.compute_dtype = compute_dtype
        self.num_patches = (self.img_size // PATCH) ** 2
        self.seq = self.num_patches + 1
        D, F = self.dim, self.mlp
        specs = [("cls_token", (1, 1, D)), ("pos_embed", (1, self.seq, D)),
                 ("patch_embed.proj.weight", (D, 3, PATCH, PATCH)), ("patch_embed.proj.bias", (D,))]
        for i in range(self.depth):
            q = f"blocks.{i}."
            specs += [(q + "norm1.weight", (D,)), (q + "norm1.bias", (D,)),
                      (q + "attn.qkv.weight", (3 * D, D)), (q + "attn.qkv.bias", (3 * D,)),
                      (q + "attn.proj.weight", (D, D)), (q + "attn.proj.bias", (D,)),
                      (q + "norm2.weight", (D,)), (q + "norm2.bias", (D,)),
                      (q + "mlp.fc1.weight", (F, D)), (q + "mlp.fc1.bias", (F,)),
                      (q + "mlp.fc2.weight", (D, F)), (q + "mlp.fc2.bias", (D,))]
        specs += [(self.final_norm + ".weight", (D,)), (self.final_norm + ".bias", (D,))]
        self._init_arena(specs, device=device)
        # module tree with timm's names (registration order = timm state_dict order)
        for name, _ in specs:
            parts = name.split(".")
            owner = self
            for k, part in enumerate(parts[:-1]):
                if part.isdigit():
                    while len(owner) <= int(part):
                        owner.append(_Holder())
                    owner = owner[int(part)]
                    continue
                if part not in owner._modules:
                    setattr(owner, part, nn.ModuleList() if parts[k + 1].isdigit() else _Holder())
                owner = owner._modules[part]
            self._register(owner, parts[-1], name)
        self.reset_parameters()
        self._ws = {}
        self.u8_norm = (127.5, 73.9)

    @torch.no_grad()
    def reset_parameters(self):
        """timm VisionTransformer.init_weights(""): Linear weights and pos_embed
        trunc_normal(std .02), biases 0, cls_token normal(std 1e-6), LayerNorm
        1 / 0; the patch projection keeps PyTorch's Conv2d default."""
        for name, (o, n, shape) in self.arena.layout.items():
            v = self.arena.view(name)
            if name == "cls_token":
                nn.init.normal_(v, std=1e-6)
            elif name == "patch_embed.proj.weight":
                nn.init.kaiming_uniform_(v, a=math.sqrt(5))
            elif name == "patch_embed.proj.bias":
                bound = 1.0 / math.sqrt(KP)
                nn.init.uniform_(v, -bound, bound)
            elif name == "pos_embed" or (name.endswith("weight") and len(shape) > 1):
                nn.init.trunc_normal_(v, std=0.02, a=-2, b=2)
            elif "norm" in name and name.endswith("weight"):
                v.fill_(1.0)
            else:
                v.zero_()

    def _after_apply(self):
        self._ws = {}

    @property
    def tdtype(self):
        return torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32

    def _weights(self):
        """Compute-dtype copy of the arena (one cast per step; fp32: the arena itself)."""
        if self.compute_dtype == "fp32":
            return self.arena.data
        wT = self._ws.get("wT")
        if wT is None:
            wT = torch.empty(self.arena.numel, dtype=self.tdtype, device=self.arena.data.device)
            self._ws["wT"] = wT
        ops.cast(self.arena.data, wT)
        return wT

    def _w(self, wT, name):
        return self.arena.view(name, wT)

    # ---------------- forward ----------------
    def run_forward(self, x, training, x_u8=None, u8_norm=None):
        """x: [B,3,H,W] fp32 (reference batch["x-ray"]) or x_u8 [B,1,H,W] uint8.
        Returns (features [B, dim] in the compute dtype, saved state)."""
        T, dev = self.tdtype, self.arena.data.device
        src = x if x is not None else x_u8
        B, S = src.shape[0], self.img_size
        if src.shape[-2] != S or src.shape[-1] != S:
            raise ValueError(f"ViTTower: built for {S}x{S} inputs (timm img_size), got {tuple(src.shape[-2:])}")
        A = self.arena
        wT = self._weights()
        D, F, H, N, P = self.dim, self.mlp, self.heads, self.seq, self.num_patches
        M = B * N
        pm = torch.empty(B * P, KP, dtype=T, device=dev)
        if x is not None:
            ops.vit_patch_prep(pm, B, S, S, x=x.contiguous().float())
        else:
            mean, std = u8_norm if u8_norm is not None else self.u8_norm
            ops.vit_patch_prep(pm, B, S, S, x_u8=x_u8.contiguous(), mean=mean, std=std)
        pe = torch.empty(B * P, D, dtype=T, device=dev)
        ops.linear_fwd(pm, self._w(wT, "patch_embed.proj.weight").view(D, KP), A.view("patch_embed.proj.bias"), pe,
                       B * P, D, KP)
        h = torch.empty(M, D, dtype=T, device=dev)
        ops.vit_assemble(pe, A.view("cls_token"), A.view("pos_embed"), h, B, N, D)
        sv = {"B": B, "wT": wT, "pm": pm, "layers": []}
        scale = 64 ** -0.5
        for i in range(self.depth):
            q = f"blocks.{i}."
            y1 = torch.empty(M, D, dtype=T, device=dev)
            mu1, rs1 = torch.empty(M, device=dev), torch.empty(M, device=dev)
            ops.layernorm_fwd(h, A.view(q + "norm1.weight"), A.view(q + "norm1.bias"), LN_EPS, y1, mu1, rs1, M, D)
            qkv = torch.empty(M, 3 * D, dtype=T, device=dev)
            ops.linear_fwd(y1, self._w(wT, q + "attn.qkv.weight"), A.view(q + "attn.qkv.bias"), qkv, M, 3 * D, D)
            o = torch.empty(M, D, dtype=T, device=dev)
            lse = torch.empty(B * H * N, device=dev)
            ops.vit_attn_fwd(qkv, o, lse, B, H, N, scale)
            x2 = torch.empty(M, D, dtype=T, device=dev)
            ops.linear_fwd(o, self._w(wT, q + "attn.proj.weight"), A.view(q + "attn.proj.bias"), x2, M, D, D,
                           mode=2, res=h)
            y2 = torch.empty(M, D, dtype=T, device=dev)
            mu2, rs2 = torch.empty(M, device=dev), torch.empty(M, device=dev)
            ops.layernorm_fwd(x2, A.view(q + "norm2.weight"), A.view(q + "norm2.bias"), LN_EPS, y2, mu2, rs2, M, D)
            pre = torch.empty(M, F, dtype=T, device=dev)
            act = torch.empty(M, F, dtype=T, device=dev)
            ops.linear_fwd(y2, self._w(wT, q + "mlp.fc1.weight"), A.view(q + "mlp.fc1.bias"), act, M, F, D, mode=1,
                           aux=pre)
            x3 = torch.empty(M, D, dtype=T, device=dev)
            ops.linear_fwd(act, self._w(wT, q + "mlp.fc2.weight"), A.view(q + "mlp.fc2.bias"), x3, M, D, F, mode=2,
                           res=x2)
            sv["layers"].append(dict(x=h, y1=y1, mu1=mu1, rs1=rs1, qkv=qkv, o=o, lse=lse, x2=x2, y2=y2, mu2=mu2,
                                     rs2=rs2, pre=pre, act=act))
            h = x3
        # head: one row per image (the class row, or the mean of the patch rows) through the final LayerNorm
        pooled = torch.empty(B, D, dtype=T, device=dev)
        if self.global_pool == "token":
            ops.scatter_rows(h, pooled, B, D, N * D, D)
        else:
            ops.avgpool_fwd(h.view(B, N, D)[:, 1:].contiguous().view(B, P, 1, D), pooled)
        feat = torch.empty(B, D, dtype=T, device=dev)
        muf, rsf = torch.empty(B, device=dev), torch.empty(B, device=dev)
        fn = self.final_norm
        ops.layernorm_fwd(pooled, A.view(fn + ".weight"), A.view(fn + ".bias"), LN_EPS, feat, muf, rsf, B, D)
        sv["final"] = (pooled, muf, rsf)
        return feat, sv

    # ---------------- backward ----------------
    def run_backward(self, sv, dfeat, on_stage_done=None):
        """dfeat: [B, dim] gradient of the features.  Overwrites the grad arena."""
        T, dev = self.tdtype, self.arena.data.device
        A, G = self.arena, self.arena
        G.grad.zero_()
        wT, B = sv["wT"], sv["B"]
        D, F, H, N, P = self.dim, self.mlp, self.heads, self.seq, self.num_patches
        M = B * N
        pooled, muf, rsf = sv["final"]
        fn = self.final_norm
        dpool = torch.empty(B, D, dtype=T, device=dev)
        ops.layernorm_bwd(dfeat.to(T).contiguous(), pooled, muf, rsf, A.view(fn + ".weight"), dpool, None,
                          G.gview(fn + ".weight"), G.gview(fn + ".bias"), B, D)
        if self.global_pool == "token":
            dh = torch.zeros(M, D, dtype=T, device=dev)
            ops.scatter_rows(dpool, dh, B, D, D, N * D)
        else:
            dpat = torch.empty(B * P, D, dtype=T, device=dev)
            ops.nest_bcast(dpool.float(), dpat, B, P, D, 1.0 / P)
            dh = torch.empty(M, D, dtype=T, device=dev)
            dh3 = dh.view(B, N, D)
            dh3[:, :1].zero_()
            dh3[:, 1:].copy_(dpat.view(B, P, D))
        scale = 64 ** -0.5
        for i in range(self.depth - 1, -1, -1):
            q = f"blocks.{i}."
            L = sv["layers"][i]
            # MLP branch
            ops.colsum(dh, G.gview(q + "mlp.fc2.bias"), M, D)
            ops.linear_wgrad(dh, L["act"], G.gview(q + "mlp.fc2.weight"), M, D, F)
            dpre = torch.empty(M, F, dtype=T, device=dev)
            ops.linear_dgrad(dh, self._w(wT, q + "mlp.fc2.weight"), dpre, M, F, D, mode=1, aux=L["pre"])
            ops.colsum(dpre, G.gview(q + "mlp.fc1.bias"), M, F)
            ops.linear_wgrad(dpre, L["y2"], G.gview(q + "mlp.fc1.weight"), M, F, D)
            dy2 = torch.empty(M, D, dtype=T, device=dev)
            ops.linear_dgrad(dpre, self._w(wT, q + "mlp.fc1.weight"), dy2, M, D, F)
            dx2 = torch.empty(M, D, dtype=T, device=dev)
            ops.layernorm_bwd_add(dy2, L["x2"], L["mu2"], L["rs2"], A.view(q + "norm2.weight"), dh, dx2,
                                  G.gview(q + "norm2.weight"), G.gview(q + "norm2.bias"), M, D)
            # attention branch
            ops.colsum(dx2, G.gview(q + "attn.proj.bias"), M, D)
            ops.linear_wgrad(dx2, L["o"], G.gview(q + "attn.proj.weight"), M, D, D)
            do = torch.empty(M, D, dtype=T, device=dev)
            ops.linear_dgrad(dx2, self._w(wT, q + "attn.proj.weight"), do, M, D, D)
            dqkv = torch.empty(M, 3 * D, dtype=T, device=dev)
            delta = torch.empty(B * H * N, device=dev)
            ops.vit_attn_bwd(L["qkv"], L["o"], do, L["lse"], delta, dqkv, B, H, N, scale)
            ops.colsum(dqkv, G.gview(q + "attn.qkv.bias"), M, 3 * D)
            ops.linear_wgrad(dqkv, L["y1"], G.gview(q + "attn.qkv.weight"), M, 3 * D, D)
            dy1 = torch.empty(M, D, dtype=T, device=dev)
            ops.linear_dgrad(dqkv, self._w(wT, q + "attn.qkv.weight"), dy1, M, D, 3 * D)
            dx = torch.empty(M, D, dtype=T, device=dev)
            ops.layernorm_bwd_add(dy1, L["x"], L["mu1"], L["rs1"], A.view(q + "norm1.weight"), dx2, dx,
                                  G.gview(q + "norm1.weight"), G.gview(q + "norm1.bias"), M, D)
            dh = dx
        # token assembly: dpos = sum over the batch, dcls = its class row; the patch rows feed the patch GEMM
        gpos = G.gview("pos_embed").view(N, D)
        ops.nest_pos_grad(dh, gpos, B, N, D)
        G.gview("cls_token").view(D).copy_(gpos[0])
        dpe = dh.view(B, N, D)[:, 1:].contiguous().view(B * P, D)
        ops.colsum(dpe, G.gview("patch_embed.proj.bias"), B * P, D)
        ops.linear_wgrad(dpe, sv["pm"], G.gview("patch_embed.proj.weight").view(D, KP), B * P, D, KP)
        if on_stage_done is not None:
            on_stage_done(0, self.arena.numel)

    def stage_span(self, stage):
        return 0, self.arena.numel

    # ---------------- autograd entry ----------------
    def forward(self, x):
        """API forward: [B,3,H,W] float (or [B,1,H,W] uint8) -> [B, dim] fp32 features."""
        feat = ViTTowerFn.apply(self, x, *self.params_in_arena_order())
        if self.drop_rate > 0.0 and self.training:
            feat = nn.functional.dropout(feat, self.drop_rate, True)
        return feat


class ViTTowerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tower: ViTTower, x, *params):
        if x.dtype == torch.uint8:
            feat, saved = tower.run_forward(None, tower.training, x_u8=x, u8_norm=tower.u8_norm)
        else:
            feat, saved = tower.run_forward(x, tower.training)
        ctx.tower, ctx.saved = tower, saved
        return feat.float()

    @staticmethod
    def backward(ctx, dfeat):
        tower = ctx.tower
        tower.begin_backward()
        tower.run_backward(ctx.saved, dfeat.contiguous())
        ctx.saved = None
        return (None, None, *tower.grads_for_autograd())


class ViTClassifier(ViTTower):
    """timm vit_*_patch16_224(num_classes) on the HIP tower (global_pool="token", timm's
    default): forward_features / forward_head / forward, as NestClassifier."""

    def __init__(self, num_classes: int = 1, variant: str = "vit_base_patch16_224", img_size: int = 224,
                 compute_dtype: str = "fp32", device=None, depth=None, global_pool: str = "token"):
        super().__init__(variant, img_size=img_size, compute_dtype=compute_dtype, device=device, depth=depth,
                         global_pool=global_pool)
        self.head = nn.Linear(self.dim, num_classes, device=device)
        nn.init.trunc_normal_(self.head.weight, std=0.02, a=-2, b=2)
        nn.init.zeros_(self.head.bias)

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.head._apply(fn)
        return self

    def forward_features(self, x):
        return ViTTower.forward(self, x)[:, :, None, None]

    def forward_head(self, x):
        return self.head(x.mean((2, 3)) if x.dim() == 4 else x)

    def forward(self, x):
        return self.forward_head(self.forward_features(x))


def vit_flops_per_image(variant="vit_base_patch16_224", img_size=224, depth=None):
    """Forward + backward FLOPs of one image (GEMMs and attention; backward = 2x forward)."""
    cfg = VIT_CFGS[variant]
    D, F = cfg["dim"], cfg["mlp"]
    P = (img_size // PATCH) ** 2
    N = P + 1
    f = 2.0 * P * D * KP
    f += (depth if depth is not None else cfg["depth"]) * (2.0 * N * (4 * D * D + 2 * D * F) + 4.0 * N * N * D)
    return 3.0 * f
