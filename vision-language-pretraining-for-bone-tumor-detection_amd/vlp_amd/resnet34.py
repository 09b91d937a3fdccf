"""ResNet34 image tower on the HIP kernels (drop-in for the timm model created
at src/models/pretrain/VisionLanguageModule.py:30-32 with num_classes=0,
global_pool="avg").

State-dict keys are timm's (conv1, bn1, layerX.Y.{conv1,bn1,conv2,bn2,
downsample.0,downsample.1}, BN running_mean/var/num_batches_tracked), so
checkpoints load into timm `resnet34` and the reference's finetuning modules
(OnlyImagingModule.py:76-80, FusionModule.py:92-96) unchanged.

Execution (train mode, per BasicBlock):
  y1 = conv1(x)                       [+ BN1 batch stats in the epilogue]
  y2 = conv2(relu(bn1(y1)))           [BN1+ReLU applied on load; + BN2 stats]
  yd = downsample.0(x)                [+ BNd stats]            (first block of layers 2-4)
  out = relu(bn2(y2) + (x | bnd(yd)))  one streaming pass
Backward (explicit, no autograd inside the tower):
  R   : sum(g), sum(g*xhat2) [, sum(g*xhatd)] with g = dout*(out>0)
  E   : dy2 = BN2'(g), dyd = BNd'(g) | g passed on as identity gradient
  conv2 dgrad -> g1 = (.)*(bn1(y1)>0) + BN1 backward sums in the epilogue
  conv2 wgrad on relu(bn1(y1)) recomputed on load
  E1  : dy1 = BN1'(g1);  conv1 dgrad (+ identity / downsample gradient) -> dout of the previous block
Which of the fused variants of these kernels a block's backward runs is decided
in one place, ResNet34Tower._bwd_route, before anything is launched; _block_bwd
then launches the steps above on that route.
Stem: conv 7x7/2 on a padded NHWC4 image, BN+ReLU+maxpool in one pass that
records the argmax tap; backward routes through the argmax, applies the ReLU
mask and accumulates BN sums in one pass.
"""
from __future__ import annotations

from collections import namedtuple
from typing import NamedTuple, Optional

import contextlib
import os

import torch
import torch.nn as nn

from . import ops
from .arena import ArenaModule

LAYERS = (3, 4, 6, 3)
WIDTHS = (64, 128, 256, 512)
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
# weight gradients on a side stream: they are off the data-gradient chain, so
# the MFMA-bound wgrad GEMMs overlap the HBM-bound BN / elementwise passes and
# the data-gradient epilogue bursts (r2 driver: +2.4 % pairs/s).  Each side-
# stream launch shares the CUs, so bench.py times the roofline kernel in a
# separate serial pass (this attribute set False).  Each stream has its own
# split-K workspace (ops.wgrad_ws), so the main-stream stem weight gradient
# never shares slabs with the side stream's.
_USE_WG_STREAM = True
_WG_STREAMS = {}
STAT_REP = 64   # replicas of per-channel fp64 sums (see vlp_stat_reduce)
# single-channel stem for the uint8 upload (VLP_STEM1=0: always the 3-channel NHWC4 path)
_USE_STEM1 = os.environ.get("VLP_STEM1", "1") != "0"
# bf16: stem conv + BN sums + max-pool fused (stem_ops.hip); False keeps the
# conv -> y0 -> max-pool kernels (tests compare the two)
_USE_STEM_FUSED = True
# layer-1 data gradients form their input dy = k*g + b*y + c in the rows kernel's
# ring (vlp_conv_dgrad_bn_act / vlp_conv_dgrad_relu_act) instead of a separate
# bn_bwd_apply pass (tests/test_gpu_streams.py holds on vs off)
_USE_BWD_ACT = os.environ.get("VLP_BWD_ACT", "1") != "0"
# bf16 stride-2 block entries: the downsample's data gradient folded into conv1's
# parity class (0, 0) (vlp_conv_dgrad_relu_ds) instead of its own launch + an addend
_USE_DS_FOLD = os.environ.get("VLP_DS_FOLD", "1") != "0"
# bf16: the second block of layers 2-4 takes its predecessor's bn2 + downsample-BN
# backward sums in its conv1 data-gradient epilogue (vlp_conv_dgrad_relu2)
_USE_RELU2 = os.environ.get("VLP_RELU2", "1") != "0"
# bf16 layer 1: bn1 + ReLU applied in conv2's input ring (vlp_conv_fwd_act), a1
# written by that kernel; False keeps the separate bn_add_relu pass
_USE_ACT_FUSED = True


def _side_stream(dev):
    s = _WG_STREAMS.get(dev)
    if s is None:
        s = _WG_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return s


STAGES = ("stem", "layer1", "layer2", "layer3", "layer4")


def _stage_of(key: str) -> str:
    return key.split(".", 1)[0] if key.startswith("layer") else "stem"


class _Holder(nn.Module):
    """Parameter/buffer container mirroring one timm submodule (no forward)."""


class _Conv:
    def __init__(self, key, Co, C, KH, KW, S, P):
        self.key, self.Co, self.C, self.KH, self.KW, self.S, self.P = key, Co, C, KH, KW, S, P
        self.numel = Co * C * KH * KW


class _BN:
    def __init__(self, key, C, holder):
        self.key, self.C, self.holder = key, C, holder


class _BNView(namedtuple("_BNView", "scale shift mean istd fsum fsumsq sum_g sum_gx sum_gxd tot_g tot_gx tot_gxd")):
    """One BatchNorm's slices of a workspace's "coef", "fstat" and "bstat" tables, built once
    per workspace: the fp32 coefficients [C]; the forward fp64 sum and sum of squares; the
    backward fp64 sums of g, g*xhat and g*xhat of the downsample BN.  The fp64 sums are
    [STAT_REP][C] replicas; the kernel that folds them leaves the total in replica 0,
    which tot_g, tot_gx, tot_gxd name (the first C entries of sum_*)."""
    __slots__ = ()

    @property
    def coefs(self):
        """(scale, shift, mean, istd): the `bn` operand of the data-gradient kernels."""
        return self[:4]


class _BwdRoute(NamedTuple):
    """What one BasicBlock's backward runs (ResNet34Tower._bwd_route)."""
    # conv1's data-gradient epilogue: the gradient reaching the block below passes that
    # block's output ReLU and feeds its BN backward sums, taken here where a kernel does so
    #   "stem"      mask + the stem BN's sums at each max-pool window's argmax
    #   "prev_bn2"  mask + the bn2 sums of a previous block without a downsample
    #   "relu2"     mask + the bn2 and downsample-BN sums of a previous block with one
    #   "plain"     none: the block below masks and reduces in a pass of its own
    epilogue: str
    fuse_in: bool     # both BN backward applies formed in the rows kernels' rings ("stem" / "prev_bn2" only)
    ds_fold: bool     # the downsample's data gradient folded into conv1's ("prev_bn2" only)
    relu_bits: bool   # the epilogue's ReLU operand: the input's sign-bit mask, else the input itself


def _tower_specs():
    convs, bns = [], []
    convs.append(_Conv("conv1", 64, 3, 7, 7, 2, 3))
    bns.append(("bn1", 64))
    inpl = 64
    for li, (n, planes) in enumerate(zip(LAYERS, WIDTHS)):
        for b in range(n):
            s = (1 if li == 0 else 2) if b == 0 else 1
            pre = f"layer{li + 1}.{b}"
            convs.append(_Conv(pre + ".conv1", planes, inpl, 3, 3, s, 1))
            bns.append((pre + ".bn1", planes))
            convs.append(_Conv(pre + ".conv2", planes, planes, 3, 3, 1, 1))
            bns.append((pre + ".bn2", planes))
            if b == 0 and (s != 1 or inpl != planes):
                convs.append(_Conv(pre + ".downsample.0", planes, inpl, 1, 1, s, 0))
                bns.append((pre + ".downsample.1", planes))
            inpl = planes
    return convs, bns


class ResNet34Tower(ArenaModule):
    num_features = 512

    def __init__(self, drop_rate: float = 0.0, compute_dtype: str = "bf16", device=None):
        super().__init__()
        self.drop_rate = float(drop_rate)
        self.compute_dtype = compute_dtype
        convs, bns = _tower_specs()
        self._convs = {c.key: c for c in convs}
        # arena order (internal; the state dict keeps timm's order): one contiguous
        # range per stage, stem first, so each stage's gradients form one bucket of
        # the data-parallel all-reduce, launched as soon as the backward leaves it
        specs = []
        self._stage_names = {}
        for st in STAGES:
            names = []
            for c in convs:
                if _stage_of(c.key) == st:
                    specs.append((c.key + ".weight", (c.Co, c.C, c.KH, c.KW)))
                    names.append(c.key + ".weight")
            for key, C in bns:
                if _stage_of(key) == st:
                    specs += [(key + ".weight", (C,)), (key + ".bias", (C,))]
                    names += [key + ".weight", key + ".bias"]
            self._stage_names[st] = names
        self._init_arena(specs, device=device)
        self._build_modules(dict(bns), device)
        self._blocks = []
        for li, n in enumerate(LAYERS):
            for b in range(n):
                pre = f"layer{li + 1}.{b}"
                self._blocks.append((pre, (pre + ".downsample.0") in self._convs))
        self.reset_parameters()
        self._ws = {}  # per-device workspaces (packed weights, wgrad buffers, BN coefficients)
        self._dbg = None   # dict: block -> (gradient of its output, masked) during backward
        self._sw = None    # the weight-gradient side stream, inside _wgrad_stream()
        self.u8_norm = (127.5, 73.9)   # (mean, std) of the uint8 upload; set per batch by the module

    def _build_modules(self, bn_c, device):
        """The module tree with timm's names (registration order = timm state_dict order)."""
        self._bns = {}

        def mk_conv(parent, attr, key):
            h = _Holder()
            setattr(parent, attr, h)
            self._register(h, "weight", key + ".weight")

        def mk_bn(parent, attr, key):
            h = _Holder()
            setattr(parent, attr, h)
            self._register(h, "weight", key + ".weight")
            self._register(h, "bias", key + ".bias")
            C = bn_c[key]
            h.register_buffer("running_mean", torch.zeros(C, device=device))
            h.register_buffer("running_var", torch.ones(C, device=device))
            h.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long, device=device))
            self._bns[key] = _BN(key, C, h)

        mk_conv(self, "conv1", "conv1")
        mk_bn(self, "bn1", "bn1")
        inpl = 64
        for li, (n, planes) in enumerate(zip(LAYERS, WIDTHS)):
            layer = nn.Sequential()
            for b in range(n):
                s = (1 if li == 0 else 2) if b == 0 else 1
                pre = f"layer{li + 1}.{b}"
                blk = _Holder()
                mk_conv(blk, "conv1", pre + ".conv1")
                mk_bn(blk, "bn1", pre + ".bn1")
                mk_conv(blk, "conv2", pre + ".conv2")
                mk_bn(blk, "bn2", pre + ".bn2")
                if b == 0 and (s != 1 or inpl != planes):
                    ds = nn.Sequential()
                    mk_conv(ds, "0", pre + ".downsample.0")
                    mk_bn(ds, "1", pre + ".downsample.1")
                    blk.downsample = ds
                layer.add_module(str(b), blk)
                inpl = planes
            setattr(self, f"layer{li + 1}", layer)

    # ---------------- init (timm ResNet.init_weights) ----------------
    @torch.no_grad()
    def reset_parameters(self, zero_init_last: bool = True):
        for c in self._convs.values():
            nn.init.kaiming_normal_(self.arena.view(c.key + ".weight"), mode="fan_out",
                                    nonlinearity="relu")
        for key in self._bns:
            self.arena.view(key + ".weight").fill_(1.0)
            self.arena.view(key + ".bias").zero_()
        if zero_init_last:
            for pre, _ in self._blocks:
                self.arena.view(pre + ".bn2.weight").zero_()

    def _after_apply(self):
        self._ws = {}

    @property
    def tdtype(self):
        return torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32

    # ---------------- workspaces ----------------
    def _workspace(self):
        dev = self.arena.data.device
        key = (str(dev), self.compute_dtype)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        T = self.tdtype
        ws = {}
        for c in self._convs.values():
            if c.key == "conv1":
                ws["conv1.wp"] = torch.empty(64, 256, dtype=T, device=dev)
            else:
                ws[c.key + ".wp"] = torch.empty(c.Co, c.KH, c.KW, c.C, dtype=T, device=dev)
                if c.key.endswith(".downsample.0"):
                    continue
                cd = self._convs.get(c.key[:-len("conv1")] + "downsample.0") if c.key.endswith(".conv1") else None
                if cd is not None:
                    # a stage's first conv1 and its downsample: transposed weights in one
                    # allocation, downsample second (vlp_conv_dgrad_relu_ds reads both)
                    n1 = c.C * c.KH * c.KW * c.Co
                    buf = torch.empty(n1 + cd.C * cd.Co, dtype=T, device=dev)
                    ws[c.key + ".wt"] = buf[:n1].view(c.C, c.KH, c.KW, c.Co)
                    ws[cd.key + ".wt"] = buf[n1:].view(cd.C, 1, 1, cd.Co)
                else:
                    ws[c.key + ".wt"] = torch.empty(c.C, c.KH, c.KW, c.Co, dtype=T, device=dev)
        # per-BN coefficient and statistic slices
        nb = len(self._bns)
        Cmax = 512
        ws["coef"] = torch.zeros(nb, 4, Cmax, dtype=torch.float32, device=dev)   # scale, shift, mean, istd
        # [R][C] replicated fp64 sums; replica 0 holds the total after vlp_stat_reduce
        ws["fstat"] = torch.zeros(nb, 2, STAT_REP * Cmax, dtype=torch.float64, device=dev)  # sum, sumsq
        ws["bstat"] = torch.zeros(nb, 3, STAT_REP * Cmax, dtype=torch.float64, device=dev)  # sum_g, sum_gx, sum_gx(ds)
        ws["bwd_coef"] = torch.empty(2, 3 * 64, dtype=torch.float32, device=dev)   # bn_bwd_coef's (k, b, c) of bn2, bn1
        ws["bn"] = {}
        for i, (k, bn) in enumerate(self._bns.items()):
            c, f, b, C, n = ws["coef"][i], ws["fstat"][i], ws["bstat"][i], bn.C, STAT_REP * bn.C
            ws["bn"][k] = _BNView(c[0, :C], c[1, :C], c[2, :C], c[3, :C], f[0, :n], f[1, :n],
                                  b[0, :n], b[1, :n], b[2, :n], b[0, :C], b[1, :C], b[2, :C])
        self._ws[key] = ws
        return ws

    def pack_weights(self):
        """fp32 master (timm layout) -> GEMM operand layouts in the compute dtype."""
        ws = self._workspace()
        key = ("pack_desc", self.arena.data.data_ptr())
        desc = ws.get(key)
        if desc is None:   # one launch for every 3x3 / 1x1 conv (pointers are stable per arena)
            entries = [(self.arena.view(c.key + ".weight"), ws[c.key + ".wp"], ws[c.key + ".wt"])
                       for c in self._convs.values() if c.key != "conv1"]
            desc = ops.pack_conv_batch(entries[0][1], entries)
            ws[key] = desc
        ops.pack_conv_batch_run(desc)
        ops.pack_stem(self.arena.view("conv1.weight"), ws["conv1.wp"])
        return ws

    # ---------------- BN helpers ----------------
    def _bn_finalize(self, ws, key, count, training):
        gamma, beta = self.arena.view(key + ".weight"), self.arena.view(key + ".bias")
        v = ws["bn"][key]
        h = self._bns[key].holder
        if training:
            ops.bn_finalize_rep(STAT_REP, count, v.fsum, v.fsumsq, gamma, beta, BN_EPS, BN_MOMENTUM, h.running_mean,
                                h.running_var, v.scale, v.shift, v.mean, v.istd)
            h.num_batches_tracked.add_(1)
        else:
            ops.bn_eval_coeffs(gamma, beta, h.running_mean, h.running_var, BN_EPS, v.scale, v.shift)
        return v.scale, v.shift

    # ---------------- forward ----------------
    def run_forward(self, x: Optional[torch.Tensor], training: bool, x_u8: Optional[torch.Tensor] = None,
                    u8_norm=(127.5, 73.9)):
        """x: [N,3,H,W] fp32 NCHW (reference batch["x-ray"]) or x_u8: [N,1,H,W] uint8.
        Returns (features [N,512] in the compute dtype, saved-state dict)."""
        ws = self.pack_weights()
        ws["fstat"].zero_()
        p, pm, saved = self._stem_forward(ws, x, x_u8, u8_norm, training)
        return self._run_blocks(ws, self.tdtype, self.arena.data.device, p.shape[0], p, pm, saved, training)

    def _stem1_input(self, ws, x_u8, u8_norm, N, H, W, Hp, Wp1):
        """The single-channel uint8 upload as the stem's 4 shifted copies xs (cached per
        shape) and the channel-summed weights ws["conv1.wp1"]."""
        T, dev = self.tdtype, self.arena.data.device
        key = ("xs", N, H, W)
        xs = ws.get(key)
        if xs is None:
            xs = ws[key] = torch.empty(4, N, Hp, Wp1, dtype=T, device=dev)   # fully written by the prep
        ops.stem1_prep_u8(x_u8.contiguous(), xs, u8_norm[0], u8_norm[1])
        if "conv1.wp1" not in ws:
            ws["conv1.wp1"] = torch.empty(64, 64, dtype=T, device=dev)
        ops.pack_stem1(self.arena.view("conv1.weight"), ws["conv1.wp1"])
        return xs

    def _stem3_input(self, ws, x, x_u8, u8_norm, N, H, W, Hp, Wp):
        """The fp32 NCHW image, or the uint8 upload replicated, as the padded NHWC4 image xp (cached per shape)."""
        key = ("xp", N, H, W)
        xp = ws.get(key)
        if xp is None:   # zeros once: the padding stays zero
            xp = ws[key] = torch.zeros(N, Hp, Wp, 4, dtype=self.tdtype, device=self.arena.data.device)
        if x is not None:
            ops.stem_prep(x.contiguous(), xp)
        else:
            ops.stem_prep_u8(x_u8.contiguous(), xp, u8_norm[0], u8_norm[1])
        return xp

    def _stem_forward(self, ws, x, x_u8, u8_norm, training):
        """conv1 -> bn1 -> ReLU -> max-pool -> (p, ReLU sign bits of p | None, saved-state dict)."""
        T, dev = self.tdtype, self.arena.data.device
        src = x if x is not None else x_u8
        N, H, W = src.shape[0], src.shape[-2], src.shape[-1]
        # the 1-channel uint8 upload carries ONE grayscale channel (the reference
        # replicates it 3x, PretrainDataModule.py:167-171): the stem then runs as a
        # K = 64 single-channel conv with channel-summed weights (vlp_stem1_*)
        g1 = ops.stem1_geom(H, W) if (x is None and _USE_STEM1) else None
        fused = g1 is not None and T == torch.bfloat16 and _USE_STEM_FUSED and ops.stem1_fused_ok(H, W)
        saved = {"N": N, "H": H, "W": W, "training": training, "stem_fused": fused}
        if g1 is not None:
            Ho, Wo, Hp, Wp1 = g1
            xin = saved["xs"] = self._stem1_input(ws, x_u8, u8_norm, N, H, W, Hp, Wp1)
        else:
            Ho, Wo, Hp, Wp = ops.stem_geom(H, W)
            xin = saved["xp"] = self._stem3_input(ws, x, x_u8, u8_norm, N, H, W, Hp, Wp)
        Hq, Wq = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
        p = torch.empty(N, Hq, Wq, 64, dtype=T, device=dev)
        idx = torch.empty(N, Hq, Wq, 64, dtype=torch.uint8, device=dev)
        # y0 at each window's argmax: the fused kernel's output; else kept for the backward only
        yarg = torch.empty_like(p) if (fused or training) else None
        bits = training and T == torch.bfloat16              # ReLU sign bits of each block input
        pm = torch.empty(p.numel() // 8, dtype=torch.uint8, device=dev) if bits else None
        bn, y0 = ws["bn"]["bn1"], None
        if fused:
            # conv + BN sums + max-pool in one pass (vlp_stem1_pool_fwd): the
            # full-resolution conv output is never written; the pooled window
            # extreme (sign of gamma) of y0 and its tap are
            s, ss = (bn.fsum, bn.fsumsq) if training else (None, None)
            ops.stem1_pool_fwd(xin, ws["conv1.wp1"], self.arena.view("bn1.weight"), yarg, idx, N, H, W, s, ss,
                               STAT_REP)
            sc0, sh0 = self._bn_finalize(ws, "bn1", N * Ho * Wo, training)
            ops.bn_add_relu(yarg, sc0, sh0, None, None, None, p, relu_mask=pm)
        else:
            y0 = torch.empty(N, Ho, Wo, 64, dtype=T, device=dev)
            if g1 is not None:
                ops.stem1_fwd(xin, ws["conv1.wp1"], N, H, W, y0, bn.fsum, bn.fsumsq, STAT_REP)
            else:
                ops.stem_fwd(xin, ws["conv1.wp"], N, H, W, y0, bn.fsum, bn.fsumsq, STAT_REP)
            sc0, sh0 = self._bn_finalize(ws, "bn1", N * Ho * Wo, training)
            ops.maxpool_fwd(y0, sc0, sh0, p, idx, yarg, relu_mask=pm)
        saved.update(y0=y0, idx=idx, yarg=yarg if training else None)
        return p, pm, saved

    def _run_blocks(self, ws, T, dev, N, p, pm, saved, training):
        bits = training and T == torch.bfloat16
        xmask = pm
        xcur = p
        blocks = []
        for pre, has_ds in self._blocks:
            blk, xcur, xmask = self._block_fwd(ws, T, dev, pre, has_ds, xcur, xmask, training, bits)
            blocks.append(blk)
        feat = torch.empty(N, 512, dtype=T, device=dev)
        ops.avgpool_fwd(xcur, feat)
        saved["blocks"] = blocks
        return feat, saved

    def _block_fwd(self, ws, T, dev, pre, has_ds, xcur, xmask, training, bits):
        """One BasicBlock forward on the current stream -> (saved dict, out, ReLU bits)."""
        c1, c2 = self._convs[pre + ".conv1"], self._convs[pre + ".conv2"]
        b1, b2 = ws["bn"][pre + ".bn1"], ws["bn"][pre + ".bn2"]
        y1 = ops.conv_fwd(xcur, ws[c1.key + ".wp"], c1.Co, 3, 3, c1.S, 1, stat_sum=b1.fsum, stat_sumsq=b1.fsumsq,
                          stat_rep=STAT_REP)
        Mb = y1.numel() // y1.shape[-1]
        sc1, sh1 = self._bn_finalize(ws, pre + ".bn1", Mb, training)
        a1 = torch.empty_like(y1)    # relu(bn1(y1)), materialised once: conv2 fwd + wgrad stream it
        if _USE_ACT_FUSED and ops.conv_fwd_act_ok(y1, c2.Co, 3, 3, 1, 1):
            # layer 1: conv2 applies bn1 + ReLU to each input row once in its ring and writes a1
            y2 = ops.conv_fwd_act(y1, ws[c2.key + ".wp"], c2.Co, 3, 3, 1, 1, sc1, sh1, a1, b2.fsum, b2.fsumsq,
                                  stat_rep=STAT_REP)
        else:
            ops.bn_add_relu(y1, sc1, sh1, None, None, None, a1)
            y2 = ops.conv_fwd(a1, ws[c2.key + ".wp"], c2.Co, 3, 3, 1, 1, stat_sum=b2.fsum, stat_sumsq=b2.fsumsq,
                              stat_rep=STAT_REP)
        sc2, sh2 = self._bn_finalize(ws, pre + ".bn2", Mb, training)
        yd = scd = shd = None
        if has_ds:
            cd = self._convs[pre + ".downsample.0"]
            bd = ws["bn"][pre + ".downsample.1"]
            yd = ops.conv_fwd(xcur, ws[cd.key + ".wp"], cd.Co, 1, 1, cd.S, 0, stat_sum=bd.fsum,
                              stat_sumsq=bd.fsumsq, stat_rep=STAT_REP)
            scd, shd = self._bn_finalize(ws, pre + ".downsample.1", Mb, training)
        out = torch.empty_like(y2)
        om = torch.empty(out.numel() // 8, dtype=torch.uint8, device=dev) if bits else None
        ops.bn_add_relu(y2, sc2, sh2, yd if has_ds else xcur, scd, shd, out, relu_mask=om)
        blk = {"x": xcur, "xmask": xmask, "y1": y1, "a1": a1, "y2": y2, "yd": yd, "out": out}
        return blk, out, om

    # ---------------- backward ----------------
    def stage_span(self, stage):
        """(offset, length) of one stage's parameters in the arena."""
        return self.arena.span(self._stage_names[stage])

    def run_backward(self, saved, dfeat: torch.Tensor, on_stage_done=None):
        """dfeat: [N,512] fp32 gradient of the pooled features.  Writes every
        parameter gradient into the grad arena (overwriting).  on_stage_done(off,
        n) is called (in backward order: layer4, layer3, layer2, layer1 + stem)
        once the arena range [off, off+n) holds its final gradients, with every
        kernel writing it already queued on the current stream -- the data-
        parallel all-reduce of that bucket is launched there."""
        dev = self.arena.data.device
        with self._wgrad_stream(dev):
            self._run_backward(saved, dfeat, self._workspace(), self.tdtype, dev, on_stage_done)

    @contextlib.contextmanager
    def _wgrad_stream(self, dev):
        """Fork: inside, _wgrad queues the weight gradients on the side stream self._sw
        (None: on the current stream).  Join on exit: every weight gradient is in the arena."""
        self._sw = _side_stream(dev) if (_USE_WG_STREAM and dev.type == "cuda") else None
        try:
            yield
        finally:
            if self._sw is not None:
                torch.cuda.current_stream(dev).wait_stream(self._sw)
            self._sw = None

    def _stage_done(self, stages, cb, dev):
        """Hand a finished stage's arena range to `cb` (the bucket all-reduce).
        With the weight-gradient side stream the collective is launched FROM that
        stream: the side stream waits for main (the stage's BN-parameter
        gradients, written there) and the collective is ordered after the
        stage's weight gradients queued on it.  The main stream never waits, so
        the data-gradient chain runs on into the next stage (VERDICT r5 item 1a:
        main.wait_stream(side) here stalled it at every stage boundary)."""
        if cb is None:
            return
        spans = [self.stage_span(s) for s in stages]
        lo = min(o for o, _ in spans)
        hi = max(o + n for o, n in spans)
        if self._sw is not None:
            self._sw.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(self._sw):
                cb(lo, hi - lo)
            return
        cb(lo, hi - lo)

    # ---------------- block ranges (tests/test_gpu_blocks.py) ----------------
    def run_block_range_forward(self, x: torch.Tensor, lo: int, hi: int, training: bool = True):
        """Forward of BasicBlocks [lo, hi) on a given NHWC input in the compute
        dtype (the output of a ReLU, as every block input is).  The same kernels
        and fusions the whole tower picks at these shapes run; returns (out,
        saved) for run_block_range_backward."""
        ws = self.pack_weights()
        T = self.tdtype
        dev = self.arena.data.device
        if x.dtype != T or x.dim() != 4 or x.shape[-1] != self._convs[self._blocks[lo][0] + ".conv1"].C:
            raise ValueError(f"block range input must be NHWC {T} with the block's channel count, got "
                             f"{tuple(x.shape)} {x.dtype}")
        ws["fstat"].zero_()
        bits = training and T == torch.bfloat16
        xmask = None
        if bits:   # sign bits of the block input, as maxpool_fwd / bn_add_relu write them
            xmask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=dev)
            C = x.shape[-1]
            one = torch.ones(C, dtype=torch.float32, device=dev)
            xr = torch.empty_like(x)
            ops.bn_add_relu(x, one, torch.zeros_like(one), None, None, None, xr, relu_mask=xmask)
        blocks = [None] * lo
        xcur = x
        for pre, has_ds in self._blocks[lo:hi]:
            blk, xcur, xmask = self._block_fwd(ws, T, dev, pre, has_ds, xcur, xmask, training, bits)
            blocks.append(blk)
        return xcur, {"blocks": blocks, "range": (lo, hi), "training": training}

    def run_block_range_backward(self, saved, dout: torch.Tensor):
        """Backward of run_block_range_forward for the gradient `dout` of the
        range's output.  Returns the gradient of its input; the parameter
        gradients of blocks [lo, hi) are written into the grad arena."""
        dev = self.arena.data.device
        lo, hi = saved["range"]
        with self._wgrad_stream(dev):
            return self._run_backward(saved, None, self._workspace(), self.tdtype, dev, None, lo=lo, hi=hi,
                                      dout0=dout.to(self.tdtype).contiguous())

    def _run_backward(self, saved, dfeat, ws, T, dev, on_stage_done=None, lo=0, hi=None, dout0=None):
        ws["bstat"].zero_()
        dfeat = dfeat.float().contiguous() if dfeat is not None else None
        blocks = saved["blocks"]
        hi = len(self._blocks) if hi is None else hi
        dout = dout0
        dout_masked = False   # dout already = g (ReLU-masked) with bn2 sums accumulated by the dgrad epilogue
        for bi in range(hi - 1, lo - 1, -1):
            route = self._bwd_route(bi, lo, T, saved, blocks, dout, dout_masked)
            dout, dout_masked = self._block_bwd(ws, dev, saved, blocks, bi, route, dout, dfeat, dout_masked)
            pre = self._blocks[bi][0]
            stage = pre.split(".", 1)[0]
            if pre.endswith(".0") and stage != "layer1":
                # first block of a stage: every gradient of that stage is final
                # (its bn2 sums came from the block above, already folded)
                self._stage_done([stage], on_stage_done, dev)
        if dout0 is not None:   # a block range (run_block_range_backward): the input gradient
            return dout
        self._stem_backward(saved, dout, ws, dev, on_stage_done)

    def _bwd_route(self, bi, lo, T, saved, blocks, dout, dout_masked) -> _BwdRoute:
        """Everything the backward of block bi chooses, decided before anything is launched.
        dout is the gradient of its output (None: the pooled features' gradient)."""
        pre, has_ds = self._blocks[bi]
        B = blocks[bi]
        x, y1, yd, xmask = B["x"], B["y1"], B["yd"], B.get("xmask")
        c1 = self._convs[pre + ".conv1"]
        Cin = x.shape[-1]
        bf16 = T == torch.bfloat16
        prev = self._blocks[bi - 1] if bi > lo else None
        if bi == 0 and lo == 0 and saved.get("yarg") is not None:
            # block 0's input is the maxpool output p = relu(bn1(y0)) at each window's
            # argmax: its mask and the stem BN's backward sums (xhat of y0 at the
            # argmax) are taken per pooled output, replacing a full-resolution pass
            epilogue = "stem"
        elif prev is not None and not prev[1]:
            epilogue = "prev_bn2"
        elif (_USE_RELU2 and prev is not None and prev[1] and bf16 and c1.S == 1
              and xmask is not None and Cin >= 128 and Cin % 64 == 0):
            # the previous block (a stage's first) has a downsample: its bn2 and downsample-BN
            # sums come out of this epilogue too, so its backward needs no reduce pass
            epilogue = "relu2"
        else:
            epilogue = "plain"
        # layer 1: both BN backward applies move into the rows kernels' rings -- only where
        # conv1's data gradient then runs a fused-input epilogue; otherwise dy1 is applied in a pass
        fuse_in = (epilogue in ("stem", "prev_bn2") and _USE_BWD_ACT and bf16 and dout_masked and not has_ds
                   and c1.S == 1 and ops.conv_dgrad_act_ok(dout, B["out"].shape[-1], 3, 3, 1, 1))
        # (dy1 | dyd) is one 32-bit buffer resource in vlp_conv_dgrad_relu_ds: 2 bf16 tensors < 4 GiB
        ds_fold = (epilogue == "prev_bn2" and _USE_DS_FOLD and has_ds and bf16 and c1.S == 2
                   and tuple(y1.shape) == tuple(yd.shape) and 4 * y1.numel() < 2 ** 32)
        # sign bits for stride 1; the stride-2 parity-class epilogue reads the
        # activation faster than single mask bytes (measured 840 vs 884 us)
        relu_bits = epilogue != "plain" and xmask is not None and c1.S == 1
        return _BwdRoute(epilogue, fuse_in, ds_fold, relu_bits)

    def _bn2_sums(self, ws, pre, has_ds, B, dout, dbc, dout_masked):
        """R: the bn2 (and downsample-BN) backward sums of g = dout * (out > 0), unless the
        data-gradient epilogue of the block above took them, and those BNs' parameter gradients."""
        out, k2, kd = B["out"], pre + ".bn2", pre + ".downsample.1"
        N, Hh, Ww, C = out.shape
        b2, bd = ws["bn"][k2], ws["bn"].get(kd)
        mud, isd, sgxd = (bd.mean, bd.istd, b2.sum_gxd) if has_ds else (None, None, None)
        if not dout_masked:
            ops.bn_bwd_reduce(N * Hh * Ww, C, dout, dbc, Hh * Ww, out, B["y2"], b2.mean, b2.istd, B["yd"], mud, isd,
                              b2.sum_g, b2.sum_gx, sgxd, out, stat_rep=STAT_REP)
        dgd = (self.arena.gview(kd + ".weight"), self.arena.gview(kd + ".bias")) if has_ds else (None, None)
        ops.bn_grad_rep(STAT_REP, C, b2.sum_g, b2.sum_gx, self.arena.gview(k2 + ".weight"),
                        self.arena.gview(k2 + ".bias"), sgxd, *dgd)

    def _block_bwd(self, ws, dev, saved, blocks, bi, r, dout, dfeat, dout_masked):
        """Backward of BasicBlock bi on route r -> (the gradient of its input, whether that is
        already masked by the ReLU below with that block's bn2 sums taken)."""
        pre, has_ds = self._blocks[bi]
        B = blocks[bi]
        x, y1, y2, yd, out = B["x"], B["y1"], B["y2"], B["yd"], B["out"]
        N, Hh, Ww, C = out.shape
        M = N * Hh * Ww
        c1, c2 = self._convs[pre + ".conv1"], self._convs[pre + ".conv2"]
        k1, k2, kd = pre + ".bn1", pre + ".bn2", pre + ".downsample.1"
        b1, b2, bd, coef = ws["bn"][k1], ws["bn"][k2], ws["bn"].get(kd), ws["bwd_coef"]
        dbc = dfeat if dout is None else None
        if self._dbg is not None and dout is not None:   # diagnostics (tools/diag_blocks.py)
            self._dbg[pre] = (dout.detach().clone(), dout_masked)
        self._bn2_sums(ws, pre, has_ds, B, dout, dbc, dout_masked)
        # E: dy2 = BN2'(g), dyd = BNd'(g) | g as the identity gradient; conv2's data gradient
        # through relu(bn1(y1)) with the BN1 backward sums -- fused: dy2 formed in its ring.
        # ds_fold: dy1 and dyd in one allocation (dyd second), one GEMM reads both
        dy2 = torch.empty_like(y2)
        dy_pair = torch.empty((2,) + tuple(y1.shape), dtype=y1.dtype, device=dev) if r.ds_fold else None
        dyd = g_id = None
        if has_ds:
            dyd = dy_pair[1] if r.ds_fold else torch.empty_like(yd)
        else:
            g_id = dout if dout_masked else torch.empty_like(out)   # masked: the identity gradient is g itself
        if r.fuse_in:
            ops.bn_bwd_coef(M, self.arena.view(k2 + ".weight"), b2.istd, b2.mean, b2.tot_g, b2.tot_gx, coef[0])
            g1 = ops.conv_dgrad_bn_act(dout, y2, coef[0], dy2, ws[c2.key + ".wt"], Hh, Ww, C, 3, 3, 1, 1,
                                       y1, b1.coefs, b1.sum_g, b1.sum_gx, stat_rep=STAT_REP)
        else:
            A = (y2, b2.mean, b2.istd, self.arena.view(k2 + ".weight"), b2.tot_g, b2.tot_gx, dy2)
            Bside = None
            if has_ds:
                Bside = (yd, bd.mean, bd.istd, self.arena.view(kd + ".weight"), b2.tot_g, b2.tot_gxd, dyd)
            ops.bn_bwd_apply(M, C, dout, dbc, Hh * Ww, None if dout_masked else out, A, Bside,
                             None if dout_masked else g_id, out)
            g1 = ops.conv_dgrad(dy2, ws[c2.key + ".wt"], Hh, Ww, C, 3, 3, 1, 1, y_bn=y1, bn=b1.coefs,
                                stat1=b1.sum_g, stat2=b1.sum_gx, stat_rep=STAT_REP)
        ops.bn_grad_rep(STAT_REP, C, b1.sum_g, b1.sum_gx, self.arena.gview(k1 + ".weight"),
                        self.arena.gview(k1 + ".bias"))
        self._wgrad(c2, dy2, B["a1"])   # on relu(bn1(y1))
        # E1: dy1 = BN1'(g1), or its coefficients for conv1's fused-input data gradient
        dy1 = dy_pair[0] if r.ds_fold else torch.empty_like(y1)
        if r.fuse_in:
            ops.bn_bwd_coef(M, self.arena.view(k1 + ".weight"), b1.istd, b1.mean, b1.tot_g, b1.tot_gx, coef[1])
        else:
            ops.bn_bwd_apply(M, C, g1, None, 1, None,
                             (y1, b1.mean, b1.istd, self.arena.view(k1 + ".weight"), b1.tot_g, b1.tot_gx, dy1),
                             None, None, y1)
        addend = g_id
        if has_ds:
            cd = self._convs[pre + ".downsample.0"]
            if not r.ds_fold:
                addend = ops.conv_dgrad(dyd, ws[cd.key + ".wt"], x.shape[1], x.shape[2], x.shape[3], 1, 1, cd.S, 0)
            self._wgrad(cd, dyd, x)
        dx = self._conv1_dgrad(ws, saved, blocks, bi, r, g1, dy1, dyd, coef, addend)
        self._wgrad(c1, dy1, x)
        if self._dbg is not None:
            for k, t in (("/dy2", dy2), ("/g1", g1), ("/dy1", dy1)) + ((("/dyd", dyd),) if has_ds else ()):
                self._dbg[pre + k] = (t.detach().clone(), False)
        return dx, r.epilogue != "plain"

    def _conv1_dgrad(self, ws, saved, blocks, bi, r, g1, dy1, dyd, coef, addend):
        """conv1's data gradient (+ addend: the identity / downsample gradient) by the kernel the
        route selects -> the gradient of the block's input.  Every epilogue but "plain" masks it
        by the input's ReLU and takes the BN backward sums of what that input feeds below."""
        pre = self._blocks[bi][0]
        c1, B = self._convs[pre + ".conv1"], blocks[bi]
        x, wt = B["x"], ws[pre + ".conv1.wt"]
        geom = (x.shape[1], x.shape[2], x.shape[3], 3, 3, c1.S, 1)
        if r.epilogue == "plain":
            return ops.conv_dgrad(dy1, wt, *geom, addend=addend)
        relu = B["xmask"] if r.relu_bits else x
        if r.epilogue == "stem":
            y, bn = saved["yarg"], ws["bn"]["bn1"]
        else:
            pp, P = self._blocks[bi - 1][0], blocks[bi - 1]
            y, bn = P["y2"], ws["bn"][pp + ".bn2"]
        if r.epilogue == "relu2":
            bnd = ws["bn"][pp + ".downsample.1"]
            return ops.conv_dgrad_relu2(dy1, wt, *geom, relu, y, bn.mean, bn.istd, P["yd"], bnd.mean, bnd.istd,
                                        bn.sum_g, bn.sum_gx, bn.sum_gxd, addend=addend, stat_rep=STAT_REP)
        sums = (y, bn.mean, bn.istd, bn.sum_g, bn.sum_gx)
        if r.fuse_in:   # dy1 = k*g1 + b*y1 + c formed in the kernel's ring and written out
            return ops.conv_dgrad_relu_act(g1, B["y1"], coef[1], dy1, wt, *geom, relu, *sums, addend=addend,
                                           stat_rep=STAT_REP)
        if r.ds_fold:
            return ops.conv_dgrad_relu_ds(dy1, dyd, wt, ws[pre + ".downsample.0.wt"], *geom, relu, *sums,
                                          stat_rep=STAT_REP)
        return ops.conv_dgrad_relu(dy1, wt, *geom, relu, *sums, addend=addend, stat_rep=STAT_REP)

    def _stem_backward(self, saved, dout, ws, dev, on_stage_done):
        """stem: maxpool -> relu -> bn1 -> conv1.  dout: the gradient of the max-pool output, ReLU-masked,
        with the stem BN's backward sums taken by block 0's data-gradient epilogue (the "stem" route)."""
        y0, idx, bn = saved["y0"], saved["idx"], ws["bn"]["bn1"]
        N, H, W = saved["N"], saved["H"], saved["W"]
        gamma, dw = self.arena.view("bn1.weight"), self.arena.gview("conv1.weight")
        ops.bn_grad_rep(STAT_REP, 64, bn.sum_g, bn.sum_gx, self.arena.gview("bn1.weight"), self.arena.gview("bn1.bias"))
        if saved["stem_fused"]:
            # the pooled gradient routed to each window's tap, through the BN backward
            # (y0 recomputed) and into the weight gradient in one pass (vlp_stem1_bwd_fused)
            ops.stem1_bwd_fused_into(saved["xs"], ws["conv1.wp1"], dout, idx, bn.mean, bn.istd, gamma,
                                     bn.tot_g, bn.tot_gx, N, H, W, dw)
        else:
            dy0 = torch.empty_like(y0)
            ops.maxpool_bwd_apply(dout, idx, y0, bn.scale, bn.shift, bn.mean, bn.istd, gamma, bn.tot_g, bn.tot_gx, dy0)
            if "xs" in saved:
                ops.stem1_wgrad_into(dy0, saved["xs"], N, H, W, dw)
            else:
                ops.stem_wgrad_into(dy0, saved["xp"], N, H, W, dw)
        self._stage_done(["layer1", "stem"], on_stage_done, dev)

    def _wgrad(self, c, dy, x):
        sw = self._sw
        if sw is not None:
            # fork onto the weight-gradient stream; the allocator must not
            # recycle dy / x before that stream has read them
            sw.wait_stream(torch.cuda.current_stream(dy.device))
            with torch.cuda.stream(sw):
                ops.conv_wgrad_into(dy, x, c.KH, c.KW, c.S, c.P, self.arena.gview(c.key + ".weight"))
            dy.record_stream(sw)
            x.record_stream(sw)
            return
        ops.conv_wgrad_into(dy, x, c.KH, c.KW, c.S, c.P, self.arena.gview(c.key + ".weight"))

    # ---------------- autograd entry ----------------
    def forward(self, x):
        """API forward: [N,3,H,W] float -> [N,512] fp32 features (timm semantics)."""
        feat = ImageTowerFn.apply(self, x, *self.params_in_arena_order())
        if self.drop_rate > 0.0 and self.training:
            feat = DropoutFn.apply(feat, self.drop_rate)
        return feat


class ImageTowerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tower: ResNet34Tower, x, *params):
        if x.dtype == torch.uint8:   # collated 1-channel upload (src/data/PretrainDataModule.py)
            feat, saved = tower.run_forward(None, tower.training, x_u8=x, u8_norm=tower.u8_norm)
        else:
            feat, saved = tower.run_forward(x, tower.training)
        ctx.tower = tower
        # under no_grad apply() records no node, so ctx (and saved) is dropped with it
        ctx.saved = saved
        return feat.float()

    @staticmethod
    def backward(ctx, dfeat):
        tower = ctx.tower
        tower.begin_backward()
        tower.run_backward(ctx.saved, dfeat)
        ctx.saved = None
        return (None, None, *tower.grads_for_autograd())


class DropoutFn(torch.autograd.Function):
    """Dropout of the pooled [N,512] features (timm's drop_rate): forward draws a keep
    mask with torch.rand_like, scaled by 1 / (1 - p), and multiplies; backward
    multiplies the gradient by the same mask."""

    @staticmethod
    def forward(ctx, x, p):
        keep = (torch.rand_like(x) >= p).to(x.dtype) / (1.0 - p)
        ctx.save_for_backward(keep)
        return x * keep

    @staticmethod
    def backward(ctx, g):
        (keep,) = ctx.saved_tensors
        return g * keep, None
