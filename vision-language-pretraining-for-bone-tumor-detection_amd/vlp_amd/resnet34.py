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
Stem: conv 7x7/2 on a padded NHWC4 image, BN+ReLU+maxpool in one pass that
records the argmax tap; backward routes through the argmax, applies the ReLU
mask and accumulates BN sums in one pass.
"""
from __future__ import annotations

from typing import List, Optional

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
        # module tree with timm names (registration order = timm state_dict order)
        self._bns = {}
        bn_c = dict(bns)

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
        self._blocks = []
        for li, n in enumerate(LAYERS):
            for b in range(n):
                pre = f"layer{li + 1}.{b}"
                self._blocks.append((pre, (pre + ".downsample.0") in self._convs))
        self.reset_parameters()
        self._ws = {}  # per-device workspaces (packed weights, wgrad buffers, BN coefficients)
        self._dbg = None   # dict: block -> (gradient of its output, masked) during backward
        self.u8_norm = (127.5, 73.9)   # (mean, std) of the uint8 upload; set per batch by the module

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
        self._bn_idx = {k: i for i, k in enumerate(self._bns)}
        self._ws[key] = ws
        return ws

    def _coef(self, ws, key):
        i, C = self._bn_idx[key], self._bns[key].C
        c = ws["coef"][i]
        return c[0, :C], c[1, :C], c[2, :C], c[3, :C]

    def _fstat(self, ws, key, full=False):
        i, C = self._bn_idx[key], self._bns[key].C
        n = STAT_REP * C if full else C
        return ws["fstat"][i, 0, :n], ws["fstat"][i, 1, :n]

    def _bstat(self, ws, key, full=False):
        i, C = self._bn_idx[key], self._bns[key].C
        n = STAT_REP * C if full else C
        return ws["bstat"][i, 0, :n], ws["bstat"][i, 1, :n]

    def _bstat_ds(self, ws, key, full=False):
        i, C = self._bn_idx[key], self._bns[key].C
        return ws["bstat"][i, 2, :(STAT_REP * C if full else C)]

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
        bn = self._bns[key]
        gamma, beta = self.arena.view(key + ".weight"), self.arena.view(key + ".bias")
        sc, sh, mu, ist = self._coef(ws, key)
        h = bn.holder
        if training:
            s, ss = self._fstat(ws, key, full=True)
            ops.bn_finalize_rep(STAT_REP, count, s, ss, gamma, beta, BN_EPS, BN_MOMENTUM, h.running_mean,
                                h.running_var, sc, sh, mu, ist)
            h.num_batches_tracked.add_(1)
        else:
            ops.bn_eval_coeffs(gamma, beta, h.running_mean, h.running_var, BN_EPS, sc, sh)
        return sc, sh

    # ---------------- forward ----------------
    def run_forward(self, x: Optional[torch.Tensor], training: bool, x_u8: Optional[torch.Tensor] = None,
                    u8_norm=(127.5, 73.9)):
        """x: [N,3,H,W] fp32 NCHW (reference batch["x-ray"]) or x_u8: [N,1,H,W] uint8.
        Returns (features [N,512] in the compute dtype, saved-state dict)."""
        ws = self.pack_weights()
        T = self.tdtype
        dev = self.arena.data.device
        src = x if x is not None else x_u8
        N, H, W = src.shape[0], src.shape[-2], src.shape[-1]
        ws["fstat"].zero_()
        # the 1-channel uint8 upload carries ONE grayscale channel (the reference
        # replicates it 3x, PretrainDataModule.py:167-171): the stem then runs as a
        # K = 64 single-channel conv with channel-summed weights (vlp_stem1_*)
        g1 = ops.stem1_geom(H, W) if (x is None and _USE_STEM1) else None
        fused = g1 is not None and T == torch.bfloat16 and _USE_STEM_FUSED and ops.stem1_fused_ok(H, W)
        if fused:
            # conv + BN sums + max-pool in one pass (vlp_stem1_pool_fwd): the
            # full-resolution conv output is never written; the pooled window
            # extreme (sign of gamma) of y0 and its tap are
            Ho, Wo, Hp, Wp1 = g1
            key = ("xs", N, H, W)
            xs = ws.get(key)
            if xs is None:
                xs = torch.empty(4, N, Hp, Wp1, dtype=T, device=dev)
                ws[key] = xs
            ops.stem1_prep_u8(x_u8.contiguous(), xs, u8_norm[0], u8_norm[1])
            if "conv1.wp1" not in ws:
                ws["conv1.wp1"] = torch.empty(64, 64, dtype=T, device=dev)
            ops.pack_stem1(self.arena.view("conv1.weight"), ws["conv1.wp1"])
            Hq, Wq = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
            yarg = torch.empty(N, Hq, Wq, 64, dtype=T, device=dev)
            idx = torch.empty(N, Hq, Wq, 64, dtype=torch.uint8, device=dev)
            s, ss = self._fstat(ws, "bn1", full=True) if training else (None, None)
            ops.stem1_pool_fwd(xs, ws["conv1.wp1"], self.arena.view("bn1.weight"), yarg, idx, N, H, W, s, ss,
                               STAT_REP)
            sc0, sh0 = self._bn_finalize(ws, "bn1", N * Ho * Wo, training)
            p = torch.empty(N, Hq, Wq, 64, dtype=T, device=dev)
            pm = torch.empty(p.numel() // 8, dtype=torch.uint8, device=dev) if training else None
            ops.bn_add_relu(yarg, sc0, sh0, None, None, None, p, relu_mask=pm)
            saved = {"N": N, "H": H, "W": W, "xs": xs, "training": training, "stem_fused": True,
                     "y0": None, "idx": idx, "yarg": yarg if training else None}
            return self._run_blocks(ws, T, dev, N, p, pm, saved, training)
        if g1 is not None:
            Ho, Wo, Hp, Wp1 = g1
            key = ("xs", N, H, W)
            xs = ws.get(key)
            if xs is None:
                xs = torch.empty(4, N, Hp, Wp1, dtype=T, device=dev)   # fully written by the prep
                ws[key] = xs
            ops.stem1_prep_u8(x_u8.contiguous(), xs, u8_norm[0], u8_norm[1])
            if "conv1.wp1" not in ws:
                ws["conv1.wp1"] = torch.empty(64, 64, dtype=T, device=dev)
            ops.pack_stem1(self.arena.view("conv1.weight"), ws["conv1.wp1"])
            saved = {"N": N, "H": H, "W": W, "xs": xs, "training": training}
            y0 = torch.empty(N, Ho, Wo, 64, dtype=T, device=dev)
            s, ss = self._fstat(ws, "bn1", full=True)
            ops.stem1_fwd(xs, ws["conv1.wp1"], N, H, W, y0, s, ss, STAT_REP)
        else:
            Ho, Wo, Hp, Wp = ops.stem_geom(H, W)
            xp_key = ("xp", N, H, W)
            xp = ws.get(xp_key)
            if xp is None:
                xp = torch.zeros(N, Hp, Wp, 4, dtype=T, device=dev)  # padding stays zero
                ws[xp_key] = xp
            if x is not None:
                ops.stem_prep(x.contiguous(), xp)
            else:
                ops.stem_prep_u8(x_u8.contiguous(), xp, u8_norm[0], u8_norm[1])
            saved = {"N": N, "H": H, "W": W, "xp": xp, "training": training}
            y0 = torch.empty(N, Ho, Wo, 64, dtype=T, device=dev)
            s, ss = self._fstat(ws, "bn1", full=True)
            ops.stem_fwd(xp, ws["conv1.wp"], N, H, W, y0, s, ss, STAT_REP)
        sc0, sh0 = self._bn_finalize(ws, "bn1", N * Ho * Wo, training)
        Hq, Wq = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
        p = torch.empty(N, Hq, Wq, 64, dtype=T, device=dev)
        idx = torch.empty(N, Hq, Wq, 64, dtype=torch.uint8, device=dev)
        yarg = torch.empty_like(p) if training else None   # y0 at each window's argmax
        bits = training and T == torch.bfloat16              # ReLU sign bits of each block input
        pm = torch.empty(p.numel() // 8, dtype=torch.uint8, device=dev) if bits else None
        ops.maxpool_fwd(y0, sc0, sh0, p, idx, yarg, relu_mask=pm)
        saved["y0"], saved["idx"], saved["yarg"] = y0, idx, yarg
        return self._run_blocks(ws, T, dev, N, p, pm, saved, training)

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
        s, ss = self._fstat(ws, pre + ".bn1", full=True)
        y1 = ops.conv_fwd(xcur, ws[c1.key + ".wp"], c1.Co, 3, 3, c1.S, 1, stat_sum=s, stat_sumsq=ss,
                          stat_rep=STAT_REP)
        Mb = y1.numel() // y1.shape[-1]
        sc1, sh1 = self._bn_finalize(ws, pre + ".bn1", Mb, training)
        a1 = torch.empty_like(y1)    # relu(bn1(y1)), materialised once: conv2 fwd + wgrad stream it
        s, ss = self._fstat(ws, pre + ".bn2", full=True)
        if _USE_ACT_FUSED and ops.conv_fwd_act_ok(y1, c2.Co, 3, 3, 1, 1):
            # layer 1: conv2 applies bn1 + ReLU to each input row once in its ring and writes a1
            y2 = ops.conv_fwd_act(y1, ws[c2.key + ".wp"], c2.Co, 3, 3, 1, 1, sc1, sh1, a1, s, ss,
                                  stat_rep=STAT_REP)
        else:
            ops.bn_add_relu(y1, sc1, sh1, None, None, None, a1)
            y2 = ops.conv_fwd(a1, ws[c2.key + ".wp"], c2.Co, 3, 3, 1, 1, stat_sum=s, stat_sumsq=ss,
                              stat_rep=STAT_REP)
        sc2, sh2 = self._bn_finalize(ws, pre + ".bn2", Mb, training)
        yd = scd = shd = None
        if has_ds:
            cd = self._convs[pre + ".downsample.0"]
            s, ss = self._fstat(ws, pre + ".downsample.1", full=True)
            yd = ops.conv_fwd(xcur, ws[cd.key + ".wp"], cd.Co, 1, 1, cd.S, 0, stat_sum=s,
                              stat_sumsq=ss, stat_rep=STAT_REP)
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
        ws = self._workspace()
        T = self.tdtype
        dev = self.arena.data.device
        self._sw = _side_stream(dev) if (_USE_WG_STREAM and dev.type == "cuda") else None
        try:
            self._run_backward(saved, dfeat, ws, T, dev, on_stage_done)
        finally:
            if self._sw is not None:   # join: every weight gradient is in the arena
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
        ws = self._workspace()
        dev = self.arena.data.device
        self._sw = _side_stream(dev) if (_USE_WG_STREAM and dev.type == "cuda") else None
        try:
            lo, hi = saved["range"]
            return self._run_backward(saved, None, ws, self.tdtype, dev, None, lo=lo, hi=hi,
                                      dout0=dout.to(self.tdtype).contiguous())
        finally:
            if self._sw is not None:
                torch.cuda.current_stream(dev).wait_stream(self._sw)
            self._sw = None

    def _run_backward(self, saved, dfeat, ws, T, dev, on_stage_done=None, lo=0, hi=None, dout0=None):
        ws["bstat"].zero_()
        dfeat = dfeat.float().contiguous() if dfeat is not None else None
        blocks = saved["blocks"]
        hi = len(self._blocks) if hi is None else hi
        dout = dout0
        dout_masked = False   # dout already = g (ReLU-masked) with bn2 sums accumulated by the dgrad epilogue
        for bi in range(hi - 1, lo - 1, -1):
            pre, has_ds = self._blocks[bi]
            B = blocks[bi]
            x, y1, y2, yd, out = B["x"], B["y1"], B["y2"], B["yd"], B["out"]
            N, Hh, Ww, C = out.shape
            Cin = x.shape[-1]
            M = N * Hh * Ww
            last = dout is None
            dbc = dfeat if last else None
            if self._dbg is not None and dout is not None:   # diagnostics (tools/diag_blocks.py)
                self._dbg[pre] = (dout.detach().clone(), dout_masked)
            HW = Hh * Ww
            c1, c2 = self._convs[pre + ".conv1"], self._convs[pre + ".conv2"]
            k1, k2 = pre + ".bn1", pre + ".bn2"
            _, _, mu2, is2 = self._coef(ws, k2)
            sg2f, sgx2f = self._bstat(ws, k2, full=True)
            mud = isd = sgxdf = None
            if has_ds:
                kd = pre + ".downsample.1"
                _, _, mud, isd = self._coef(ws, kd)
                sgxdf = self._bstat_ds(ws, k2, full=True)
            if not dout_masked:
                ops.bn_bwd_reduce(M, C, dout, dbc, HW, out, y2, mu2, is2, yd, mud, isd, sg2f, sgx2f, sgxdf,
                                  out, stat_rep=STAT_REP)
            kd = pre + ".downsample.1"
            ops.bn_grad_rep(STAT_REP, C, sg2f, sgx2f, self.arena.gview(k2 + ".weight"),
                            self.arena.gview(k2 + ".bias"), sgxdf,
                            self.arena.gview(kd + ".weight") if has_ds else None,
                            self.arena.gview(kd + ".bias") if has_ds else None)
            sg2, sgx2 = sg2f[:C], sgx2f[:C]
            sgxd = sgxdf[:C] if has_ds else None
            dy2 = torch.empty_like(y2)
            A = (y2, mu2, is2, self.arena.view(k2 + ".weight"), sg2, sgx2, dy2)
            Bside, g_id = None, None
            prev = self._blocks[bi - 1] if bi > lo else None
            # (dy1 | dyd) is one 32-bit buffer resource in vlp_conv_dgrad_relu_ds: 2 bf16 tensors < 4 GiB
            ds_fold = (_USE_DS_FOLD and has_ds and T == torch.bfloat16 and c1.S == 2 and prev is not None
                       and not prev[1] and tuple(y1.shape) == tuple(yd.shape) and 4 * y1.numel() < 2 ** 32)
            dy_pair = None
            if has_ds:
                if ds_fold:   # dy1 and dyd in one allocation (dyd second): one GEMM reads both
                    dy_pair = torch.empty((2,) + tuple(y1.shape), dtype=y1.dtype, device=dev)
                    dyd = dy_pair[1]
                else:
                    dyd = torch.empty_like(yd)
                Bside = (yd, mud, isd, self.arena.view(kd + ".weight"), sg2, sgxd, dyd)
            elif dout_masked:
                g_id = dout          # the identity branch's gradient is g itself
            else:
                g_id = torch.empty_like(out)
            # layer 1: both BN backward applies move into the rows kernels' rings -- only where
            # conv1's data gradient then runs a fused-input epilogue (the stem-sums or the
            # previous-block branch below); otherwise the plain path applies dy1 itself
            stem_sums = bi == 0 and lo == 0 and saved.get("yarg") is not None
            fuse_in = (_USE_BWD_ACT and T == torch.bfloat16 and dout_masked and not has_ds
                       and c1.S == 1 and (stem_sums or (prev is not None and not prev[1]))
                       and ops.conv_dgrad_act_ok(dout, C, 3, 3, 1, 1))
            sc1, sh1, mu1, is1 = self._coef(ws, k1)
            sg1f, sgx1f = self._bstat(ws, k1, full=True)
            if fuse_in:
                coef = ws.get("bwd_coef")
                if coef is None:
                    coef = ws["bwd_coef"] = torch.empty(2, 3 * 64, dtype=torch.float32, device=dev)
                ops.bn_bwd_coef(M, self.arena.view(k2 + ".weight"), is2, mu2, sg2, sgx2, coef[0])
                # conv2: dgrad of dy2 = BN2'(dout) through relu(bn1(y1)) with BN1 backward sums
                g1 = ops.conv_dgrad_bn_act(dout, y2, coef[0], dy2, ws[c2.key + ".wt"], Hh, Ww, C, 3, 3, 1, 1,
                                           y1, (sc1, sh1, mu1, is1), sg1f, sgx1f, stat_rep=STAT_REP)
            else:
                ops.bn_bwd_apply(M, C, dout, dbc, HW, None if dout_masked else out, A, Bside,
                                 None if dout_masked else g_id, out)
                # conv2: dgrad through relu(bn1(y1)) with BN1 backward sums; wgrad on relu(bn1(y1))
                g1 = ops.conv_dgrad(dy2, ws[c2.key + ".wt"], Hh, Ww, C, 3, 3, 1, 1, y_bn=y1,
                                    bn=(sc1, sh1, mu1, is1), stat1=sg1f, stat2=sgx1f, stat_rep=STAT_REP)
            ops.bn_grad_rep(STAT_REP, C, sg1f, sgx1f, self.arena.gview(k1 + ".weight"),
                            self.arena.gview(k1 + ".bias"))
            sg1, sgx1 = sg1f[:C], sgx1f[:C]
            self._wgrad(c2, dy2, B["a1"])
            dy1 = dy_pair[0] if dy_pair is not None else torch.empty_like(y1)
            if fuse_in:
                ops.bn_bwd_coef(M, self.arena.view(k1 + ".weight"), is1, mu1, sg1, sgx1, coef[1])
            else:
                ops.bn_bwd_apply(M, C, g1, None, 1, None,
                                 (y1, mu1, is1, self.arena.view(k1 + ".weight"), sg1, sgx1, dy1), None, None, y1)
            Hi, Wi = x.shape[1], x.shape[2]
            addend = g_id
            if has_ds:
                cd = self._convs[pre + ".downsample.0"]
                if not ds_fold:
                    addend = ops.conv_dgrad(dyd, ws[cd.key + ".wt"], Hi, Wi, Cin, 1, 1, cd.S, 0)
                self._wgrad(cd, dyd, x)
            # the gradient reaching block bi-1 passes its output ReLU and feeds its bn2:
            # when that block has no downsample branch, mask + reduce in this epilogue
            if stem_sums:
                # block 0's input is the maxpool output p = relu(bn1(y0)) at each window's
                # argmax: its mask and the stem BN's backward sums (xhat of y0 at the
                # argmax) are taken per pooled output here, replacing a full-resolution pass
                _, _, mu0, is0 = self._coef(ws, "bn1")
                sg0f, sgx0f = self._bstat(ws, "bn1", full=True)
                rmask = B["xmask"] if B.get("xmask") is not None else x
                if fuse_in:
                    dx = ops.conv_dgrad_relu_act(g1, y1, coef[1], dy1, ws[c1.key + ".wt"], Hi, Wi, Cin, 3, 3, 1, 1,
                                                 rmask, saved["yarg"], mu0, is0, sg0f, sgx0f, addend=addend,
                                                 stat_rep=STAT_REP)
                else:
                    dx = ops.conv_dgrad_relu(dy1, ws[c1.key + ".wt"], Hi, Wi, Cin, 3, 3, c1.S, 1, rmask,
                                             saved["yarg"], mu0, is0, sg0f, sgx0f, addend=addend, stat_rep=STAT_REP)
                dout_masked = True
            elif prev is not None and not prev[1]:
                kp = prev[0] + ".bn2"
                _, _, mup, isp = self._coef(ws, kp)
                sgpf, sgxpf = self._bstat(ws, kp, full=True)
                # sign bits for stride 1; the stride-2 parity-class epilogue reads the
                # activation faster than single mask bytes (measured 840 vs 884 us)
                rmask = B["xmask"] if (B.get("xmask") is not None and c1.S == 1) else x
                if fuse_in:
                    dx = ops.conv_dgrad_relu_act(g1, y1, coef[1], dy1, ws[c1.key + ".wt"], Hi, Wi, Cin, 3, 3, 1, 1,
                                                 rmask, blocks[bi - 1]["y2"], mup, isp, sgpf, sgxpf,
                                                 addend=addend, stat_rep=STAT_REP)
                elif ds_fold:
                    dx = ops.conv_dgrad_relu_ds(dy1, dyd, ws[c1.key + ".wt"], ws[cd.key + ".wt"], Hi, Wi, Cin, 3, 3,
                                                c1.S, 1, rmask, blocks[bi - 1]["y2"], mup, isp, sgpf, sgxpf,
                                                stat_rep=STAT_REP)
                else:
                    dx = ops.conv_dgrad_relu(dy1, ws[c1.key + ".wt"], Hi, Wi, Cin, 3, 3, c1.S, 1, rmask,
                                             blocks[bi - 1]["y2"], mup, isp, sgpf, sgxpf, addend=addend,
                                             stat_rep=STAT_REP)
                dout_masked = True
            elif (_USE_RELU2 and prev is not None and prev[1] and T == torch.bfloat16 and c1.S == 1
                  and B.get("xmask") is not None and Cin >= 128 and Cin % 64 == 0):
                # the previous block (a stage's first) has a downsample: its bn2 and downsample-BN
                # sums come out of this epilogue too, so its backward needs no reduce pass
                kp, kdp = prev[0] + ".bn2", prev[0] + ".downsample.1"
                _, _, mup, isp = self._coef(ws, kp)
                _, _, mudp, isdp = self._coef(ws, kdp)
                sgpf, sgxpf = self._bstat(ws, kp, full=True)
                sgxdpf = self._bstat_ds(ws, kp, full=True)
                dx = ops.conv_dgrad_relu2(dy1, ws[c1.key + ".wt"], Hi, Wi, Cin, 3, 3, 1, 1, B["xmask"],
                                          blocks[bi - 1]["y2"], mup, isp, blocks[bi - 1]["yd"], mudp, isdp,
                                          sgpf, sgxpf, sgxdpf, addend=addend, stat_rep=STAT_REP)
                dout_masked = True
            else:
                if fuse_in:   # dy1 was never applied: the branches above are the only consumers of coef
                    raise RuntimeError(f"{pre}: fused BN-backward input without a fused data-gradient epilogue")
                dx = ops.conv_dgrad(dy1, ws[c1.key + ".wt"], Hi, Wi, Cin, 3, 3, c1.S, 1, addend=addend)
                dout_masked = False
            self._wgrad(c1, dy1, x)
            if self._dbg is not None:
                self._dbg[pre + "/dy2"] = (dy2.detach().clone(), False)
                self._dbg[pre + "/g1"] = (g1.detach().clone(), False)
                self._dbg[pre + "/dy1"] = (dy1.detach().clone(), False)
                if has_ds:
                    self._dbg[pre + "/dyd"] = (dyd.detach().clone(), False)
            dout = dx
            stage = pre.split(".", 1)[0]
            if pre.endswith(".0") and stage != "layer1":
                # first block of a stage: every gradient of that stage is final
                # (its bn2 sums came from the block above, already folded)
                self._stage_done([stage], on_stage_done, dev)
        if dout0 is not None:   # a block range (run_block_range_backward): the input gradient
            return dout
        self._stem_backward(saved, dout, ws, dev, on_stage_done)

    def _stem_backward(self, saved, dout, ws, dev, on_stage_done):
        """stem: maxpool -> relu -> bn1 -> conv1 (dout: the gradient of the max-pool output)."""
        y0, idx = saved["y0"], saved["idx"]
        sc0, sh0, mu0, is0 = self._coef(ws, "bn1")
        sg0f, sgx0f = self._bstat(ws, "bn1", full=True)
        if saved.get("stem_fused"):
            # the pooled gradient routed to each window's tap, through the BN backward
            # (y0 recomputed) and into the weight gradient in one pass (vlp_stem1_bwd_fused)
            ops.bn_grad_rep(STAT_REP, 64, sg0f, sgx0f, self.arena.gview("bn1.weight"),
                            self.arena.gview("bn1.bias"))
            N, H, W = saved["N"], saved["H"], saved["W"]
            ops.stem1_bwd_fused_into(saved["xs"], ws["conv1.wp1"], dout, idx, mu0, is0, self.arena.view("bn1.weight"),
                                     sg0f[:64], sgx0f[:64], N, H, W, self.arena.gview("conv1.weight"))
            self._stage_done(["layer1", "stem"], on_stage_done, dev)
            return
        if saved.get("yarg") is None:
            ops.maxpool_bwd(dout, idx, y0, sc0, sh0, mu0, is0, sg0f, sgx0f, stat_rep=STAT_REP)
        ops.bn_grad_rep(STAT_REP, 64, sg0f, sgx0f, self.arena.gview("bn1.weight"), self.arena.gview("bn1.bias"))
        sg0, sgx0 = sg0f[:64], sgx0f[:64]
        dy0 = torch.empty_like(y0)
        ops.maxpool_bwd_apply(dout, idx, y0, sc0, sh0, mu0, is0, self.arena.view("bn1.weight"), sg0, sgx0, dy0)
        if "xs" in saved:
            ops.stem1_wgrad_into(dy0, saved["xs"], saved["N"], saved["H"], saved["W"],
                                 self.arena.gview("conv1.weight"))
        else:
            ops.stem_wgrad_into(dy0, saved["xp"], saved["N"], saved["H"], saved["W"],
                                self.arena.gview("conv1.weight"))
        self._stage_done(["layer1", "stem"], on_stage_done, dev)

    def _wgrad(self, c, dy, x):
        sw = getattr(self, "_sw", None)
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
    """Feature dropout of timm's head (drop_rate); mask from the HIP hash RNG is
    not needed here: this runs on a [N,512] tensor, via the linear-fwd dropout
    epilogue would be overkill, so it uses a precomputed keep-mask."""

    @staticmethod
    def forward(ctx, x, p):
        keep = (torch.rand_like(x) >= p).to(x.dtype) / (1.0 - p)
        ctx.save_for_backward(keep)
        return x * keep

    @staticmethod
    def backward(ctx, g):
        (keep,) = ctx.saved_tensors
        return g * keep, None
