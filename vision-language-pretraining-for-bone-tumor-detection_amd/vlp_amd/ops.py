"""Tensor-level wrappers over the C ABI (libvlp_hip.so).

PyTorch provides only device memory (caching allocator), the current stream,
and zero-fills; every arithmetic operation below is a hand-written HIP kernel.
All functions enqueue on torch's current stream and never synchronise.
"""
from __future__ import annotations

import ctypes

import torch

from . import ktimer
from ._lib import BF16, F32, lib, ptr, stream_of


def dcode(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported storage dtype {t.dtype}")


def _s():
    return stream_of()


def conv_out_hw(H, W, KH, KW, S, P):
    return (H + 2 * P - KH) // S + 1, (W + 2 * P - KW) // S + 1


# kernel-family keys mirror the tile dispatch in csrc (one key = one kernel name)
def _tile_auto(n):
    return "/narrow" if n <= 64 else "/wide"


def _tile_wgrad(m):
    return "/short" if m <= 64 else "/wide"


def _tile_lin(m, n):
    return "/narrow" if n <= 64 else ("/64x256" if m <= 1024 else "/wide")


# ---------------- convolutions ----------------
def conv_fwd(x, wp, Co, KH, KW, S, P, in_scale=None, in_shift=None, stat_sum=None, stat_sumsq=None,
             out=None, stat_rep=1):
    N, H, W, C = x.shape
    Ho, Wo = conv_out_hw(H, W, KH, KW, S, P)
    y = out if out is not None else torch.empty((N, Ho, Wo, Co), dtype=x.dtype, device=x.device)
    if stat_sum is None:
        stat_sum = torch.zeros(Co, dtype=torch.float64, device=x.device)
        stat_sumsq = torch.zeros(Co, dtype=torch.float64, device=x.device)
    tk = ktimer.begin(f"conv_fwd[{'xf' if in_scale is not None else 'raw'}]{_tile_auto(Co)}",
                      2.0 * N * Ho * Wo * Co * C * KH * KW)
    lib().vlp_conv_fwd(dcode(x), ptr(x), ptr(wp), ptr(y), N, H, W, C, Co, KH, KW, S, P,
                       ptr(in_scale), ptr(in_shift), ptr(stat_sum), ptr(stat_sumsq), int(stat_rep), _s())
    ktimer.end(tk)
    return y


def conv_fwd_act_ok(x, Co, KH, KW, S, P):
    N, H, W, C = x.shape
    return bool(lib()._dll.vlp_conv_fwd_act_ok(dcode(x), N, H, W, C, Co, KH, KW, S, P))


def conv_fwd_act(x, wp, Co, KH, KW, S, P, in_scale, in_shift, x_act, stat_sum, stat_sumsq, stat_rep=1, out=None):
    """conv(relu(in_scale*x + in_shift)) with that activation also written to x_act
    (vlp_conv_fwd_act: BN-apply + ReLU fused into the layer-1 rows kernel's ring)."""
    N, H, W, C = x.shape
    Ho, Wo = conv_out_hw(H, W, KH, KW, S, P)
    y = out if out is not None else torch.empty((N, Ho, Wo, Co), dtype=x.dtype, device=x.device)
    tk = ktimer.begin("conv_fwd[act]/" + ("narrow" if C == 64 else "wide"), 2.0 * N * Ho * Wo * Co * C * KH * KW)
    lib().vlp_conv_fwd_act(dcode(x), ptr(x), ptr(wp), ptr(y), ptr(x_act), N, H, W, C, Co, KH, KW, S, P,
                           ptr(in_scale), ptr(in_shift), ptr(stat_sum), ptr(stat_sumsq), int(stat_rep), _s())
    ktimer.end(tk)
    return y


def _conv_dgrad(entry, label, pre, geom, post, stat_rep, out, relu=None, post2=(), taps=None):
    """The shared body of the conv_dgrad* wrappers:
    vlp_<entry>(dtype, *pre, out, N, H, W, C, Co, KH, KW, S, P, *post, [relu_out, relu_mask,] *post2, stat_rep, stream)
    timed under `label`.  pre[0] is the [N][Ho][Wo][Co] gradient; `relu` is the ReLU
    activation or its uint8 sign-bit mask and fills the one pointer of the pair it is."""
    dy = pre[0]
    H, W, C, KH, KW, S, P = geom
    N, Ho, Wo, Co = dy.shape
    if out is None:
        out = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    if relu is not None:
        bits = relu.dtype == torch.uint8
        post = (*post, None if bits else relu, relu if bits else None)
    tk = ktimer.begin(label, 2.0 * N * Ho * Wo * Co * C * (taps or KH * KW))
    getattr(lib(), "vlp_" + entry)(dcode(dy), *map(ptr, pre), ptr(out), N, H, W, C, Co, KH, KW, S, P,
                                   *map(ptr, post), *map(ptr, post2), int(stat_rep), _s())
    ktimer.end(tk)
    return out


def conv_dgrad(dy, wt, H, W, C, KH, KW, S, P, addend=None, y_bn=None, bn=None, stat1=None,
               stat2=None, out=None, stat_rep=1):
    """bn = (scale, shift, mean, invstd) of the BN+ReLU producing the conv input."""
    bn = bn if y_bn is not None else (None,) * 4
    return _conv_dgrad("conv_dgrad", f"conv_dgrad[{'bn' if y_bn is not None else 'add'}]{_tile_auto(C)}",
                       (dy, wt), (H, W, C, KH, KW, S, P), (addend, y_bn, *bn, stat1, stat2), stat_rep, out)


def conv_dgrad_relu(dy, wt, H, W, C, KH, KW, S, P, relu_out, y, mean, invstd, stat1, stat2,
                    addend=None, stat_rep=1, out=None):
    """g = (dgrad(dy) + addend) * (relu_out > 0), plus the BN backward sums of g
    against y (the next block's bn2 input).  relu_out may be the activation or
    its uint8 sign-bit mask (bn_add_relu / maxpool_fwd relu_mask)."""
    return _conv_dgrad("conv_dgrad_relu", f"conv_dgrad[relu]{_tile_auto(C)}", (dy, wt), (H, W, C, KH, KW, S, P),
                       (addend,), stat_rep, out, relu_out, (y, mean, invstd, stat1, stat2))


def conv_dgrad_act_ok(dy, C, KH, KW, S, P):
    N, H, W, Co = dy.shape
    return bool(lib()._dll.vlp_conv_dgrad_act_ok(dcode(dy), N, H, W, C, Co, KH, KW, S, P))


def bn_bwd_coef(M, gamma, istd, mean, sum_g, sum_gx, coef):
    """coef[3][C] = (k, b, c) of the folded BN backward dy = k*g + b*y + c."""
    lib().vlp_bn_bwd_coef(int(M), gamma.numel(), ptr(gamma), ptr(istd), ptr(mean), ptr(sum_g), ptr(sum_gx),
                          ptr(coef), _s())


def conv_dgrad_bn_act(g_in, y_in, in_coef, dy_out, wt, H, W, C, KH, KW, S, P, y_bn, bn, stat1, stat2,
                      stat_rep=1, out=None):
    """conv_dgrad(dy, y_bn=..., bn=...) with dy = k*g_in + b*y_in + c formed in the
    layer-1 rows kernel's ring from in_coef (bn_bwd_coef) and written to dy_out
    (vlp_conv_dgrad_bn_act: the bn_bwd_apply pass fused)."""
    return _conv_dgrad("conv_dgrad_bn_act", "conv_dgrad[bn,act]/narrow", (g_in, y_in, in_coef, dy_out, wt),
                       (H, W, C, KH, KW, S, P), (y_bn, *bn, stat1, stat2), stat_rep, out)


def conv_dgrad_relu_act(g_in, y_in, in_coef, dy_out, wt, H, W, C, KH, KW, S, P, relu_out, y, mean, invstd,
                        stat1, stat2, addend=None, stat_rep=1, out=None):
    """conv_dgrad_relu with its input dy = k*g_in + b*y_in + c formed in the rows
    kernel's ring and written to dy_out (vlp_conv_dgrad_relu_act)."""
    return _conv_dgrad("conv_dgrad_relu_act", "conv_dgrad[relu,act]/narrow", (g_in, y_in, in_coef, dy_out, wt),
                       (H, W, C, KH, KW, S, P), (addend,), stat_rep, out, relu_out, (y, mean, invstd, stat1, stat2))


def conv_dgrad_relu_ds(dy, dyd, wt, wtd, H, W, C, KH, KW, S, P, relu_out, y, mean, invstd, stat1, stat2,
                       stat_rep=1, out=None):
    """conv_dgrad_relu of a stride-2 conv with the 1x1/2 downsample's data gradient
    (dyd against wtd) folded into parity class (0, 0) in the same GEMMs
    (vlp_conv_dgrad_relu_ds).  dyd must follow dy and wtd follow wt in memory."""
    return _conv_dgrad("conv_dgrad_relu_ds", f"conv_dgrad[relu,ds]{_tile_auto(C)}", (dy, dyd, wt, wtd),
                       (H, W, C, KH, KW, S, P), (), stat_rep, out, relu_out, (y, mean, invstd, stat1, stat2),
                       taps=KH * KW + 1)


def conv_dgrad_relu2(dy, wt, H, W, C, KH, KW, S, P, relu_mask, y, mean, invstd, yd, meand, invstdd,
                     stat1, stat2, stat3, addend=None, stat_rep=1, out=None):
    """g = (dgrad(dy) + addend) * relu bits, with the three BN backward sums of a
    block whose output feeds its bn2 (y, mean, invstd) and its downsample BN (yd,
    meand, invstdd): sum g, sum g*xhat, sum g*xhatd (vlp_conv_dgrad_relu2)."""
    return _conv_dgrad("conv_dgrad_relu2", f"conv_dgrad[relu2]{_tile_auto(C)}", (dy, wt), (H, W, C, KH, KW, S, P),
                       (addend, relu_mask, y, mean, invstd, yd, meand, invstdd, stat1, stat2, stat3), stat_rep, out)


def conv_wgrad(dy, x, KH, KW, S, P, dw_ws, in_scale=None, in_shift=None):
    N, H, W, C = x.shape
    Co = dy.shape[-1]
    Ho, Wo = dy.shape[1], dy.shape[2]
    tk = ktimer.begin(f"conv_wgrad[{'xf' if in_scale is not None else 'raw'}]{_tile_wgrad(Co)}",
                      2.0 * N * Ho * Wo * Co * C * KH * KW)
    lib().vlp_conv_wgrad(dcode(dy), ptr(dy), ptr(x), ptr(dw_ws), N, H, W, C, Co, KH, KW, S, P,
                         ptr(in_scale), ptr(in_shift), _s())
    ktimer.end(tk)
    return dw_ws


WGRAD_WS_FLOATS = 32 << 20   # 128 MB of split-K slabs (the largest conv needs ~17M floats at bs=256)
# Split-K slab workspaces, one per (device, stream).  A workspace is only ever
# written and folded by launches on ONE stream, so the stream order is its
# only synchronisation: the text tower's backward (its own stream), the image
# tower's weight-gradient side stream and the main stream each get their own
# buffer.  Allocated while that stream is current, so the caching allocator
# also ties the block (and a replaced, smaller block) to that stream.
_WS_CACHE = {}


def _stream_ws(kind, device, elems):
    import torch as _t
    st = _t.cuda.current_stream(device) if device.type == "cuda" else None
    key = (kind, str(device), st.cuda_stream if st is not None else 0)
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < elems:
        buf = torch.empty(elems, dtype=torch.float32, device=device)
        _WS_CACHE[key] = buf
    return buf


def wgrad_ws(device):
    return _stream_ws("wgrad", device, WGRAD_WS_FLOATS)


def _wgrad_into(entry, label, flops, dy, x, geom, fold_geom, grad):
    """The shared body of the *_wgrad_into wrappers:
    vlp_<entry>_wgrad_ws(dtype, dy, x, ws, ws floats, &nsplit, *geom, stream) timed under `label`,
    its K-splits stored as fp32 slabs of the stream's cached workspace, then
    vlp_<entry>_wgrad_fold(*fold_geom, nsplit, ws, grad, stream) with the split count the
    first call returned."""
    ws = wgrad_ws(dy.device)
    ns = ctypes.c_int(0)
    tk = ktimer.begin(label, flops)
    getattr(lib(), f"vlp_{entry}_wgrad_ws")(dcode(dy), ptr(dy), ptr(x), ptr(ws), ws.numel(), ctypes.addressof(ns),
                                            *geom, _s())
    ktimer.end(tk)
    getattr(lib(), f"vlp_{entry}_wgrad_fold")(*fold_geom, ns.value, ptr(ws), ptr(grad), _s())
    return grad


def conv_wgrad_into(dy, x, KH, KW, S, P, grad):
    """grad[Co][C][KH][KW] = sum over pixels dy x_patch, overwriting grad (the
    parameter's own gradient layout).  The GEMM's K-splits write fp32 slabs of
    a cached workspace; one fold pass sums and transposes them."""
    N, H, W, C = x.shape
    Co, Ho, Wo = dy.shape[-1], dy.shape[1], dy.shape[2]
    return _wgrad_into("conv", f"conv_wgrad[raw]{_tile_wgrad(Co)}", 2.0 * N * Ho * Wo * Co * C * KH * KW, dy, x,
                       (N, H, W, C, Co, KH, KW, S, P), (Co, C, KH, KW), grad)


def stem_wgrad_into(dy, xp, N, H, W, grad):
    """grad[64][3][7][7] = stem weight gradient (overwrites), via per-split
    fp32 slabs of the shared weight-gradient workspace and one fold pass."""
    return _wgrad_into("stem", "stem_wgrad", 2.0 * dy.numel() * 147, dy, xp, (N, H, W), (), grad)


def stem_geom(H, W):
    a, b, c, d = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int())
    lib()._dll.vlp_stem_geom(H, W, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                             ctypes.byref(d))
    return a.value, b.value, c.value, d.value


def stem1_geom(H, W):
    """(Ho, Wo, Hp, Wp1) of the single-channel stem, or None when it does not apply
    (Wo % 4 != 0: the caller takes the 3-channel path)."""
    a, b, c, d = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int())
    r = lib()._dll.vlp_stem1_geom(H, W, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d))
    return None if r else (a.value, b.value, c.value, d.value)


def stem1_prep_u8(x_u8, xs, mean, std):
    N, H, W = x_u8.shape[0], x_u8.shape[-2], x_u8.shape[-1]
    lib().vlp_stem1_prep_u8(dcode(xs), ptr(x_u8), ptr(xs), N, H, W, float(mean), float(std), _s())


def pack_stem1(w, wp1):
    lib().vlp_pack_stem1(dcode(wp1), ptr(w), ptr(wp1), _s())


def stem1_fwd(xs, wp1, N, H, W, y, stat_sum, stat_sumsq, stat_rep=1):
    tk = ktimer.begin("stem_fwd", 2.0 * y.numel() * 147)
    lib().vlp_stem1_fwd(dcode(xs), ptr(xs), ptr(wp1), ptr(y), N, H, W, ptr(stat_sum), ptr(stat_sumsq),
                        int(stat_rep), _s())
    ktimer.end(tk)


def stem1_wgrad_into(dy, xs, N, H, W, grad):
    """grad[64][3][7][7] = stem weight gradient of the single-channel path (overwrites)."""
    return _wgrad_into("stem1", "stem_wgrad", 2.0 * dy.numel() * 147, dy, xs, (N, H, W), (), grad)


def stem1_fused_ok(H, W):
    return bool(lib()._dll.vlp_stem1_fused_ok(int(H), int(W)))


def stem1_pool_fwd(xs, wp1, gamma, yarg, idx, N, H, W, stat_sum=None, stat_sumsq=None, stat_rep=1):
    """Fused stem conv + BN sums + 3x3/2 max-pool of sign(gamma)*y0 (bf16); y0 is never stored."""
    tk = ktimer.begin("stem_fwd", 2.0 * N * (H // 2) * (W // 2) * 64 * 147)
    lib().vlp_stem1_pool_fwd(ptr(xs), ptr(wp1), ptr(gamma), ptr(yarg), ptr(idx), N, H, W, ptr(stat_sum),
                             ptr(stat_sumsq), int(stat_rep), _s())
    ktimer.end(tk)


def stem1_route_bwd(xs, wp1, dp, idx, sc, sh, mean, istd, gamma, sum_g, sum_gx, dy, N, H, W):
    lib().vlp_stem1_route_bwd(ptr(xs), ptr(wp1), ptr(dp), ptr(idx), ptr(sc), ptr(sh), ptr(mean), ptr(istd),
                              ptr(gamma), ptr(sum_g), ptr(sum_gx), ptr(dy), N, H, W, _s())


def stem1_bwd_fused_into(xs, wp1, dp, idx, mean, istd, gamma, sum_g, sum_gx, N, H, W, grad):
    """grad[64][3][7][7] = the stem weight gradient from the pooled gradient dp
    (ReLU-masked): routing, BN backward and the weight gradient in one pass
    through the batch sums R = sum g P^T, G = sum P P^T, S = sum P (y0 and dy
    never formed); per-workgroup slabs folded in a fixed order."""
    n = ctypes.c_longlong(0)
    lib().vlp_stem1_bwd_fused_ws_floats(N, H, W, ctypes.byref(n))
    ws = _stream_ws("wgrad", dp.device, max(n.value, WGRAD_WS_FLOATS))
    tk = ktimer.begin("stem_bwd_fused", 6.0 * N * (H // 2) * (W // 2) * 64 * 64)
    lib().vlp_stem1_bwd_fused(ptr(xs), ptr(wp1), ptr(dp), ptr(idx), ptr(mean), ptr(istd), ptr(gamma), ptr(sum_g),
                              ptr(sum_gx), ptr(ws), ws.numel(), ptr(grad), N, H, W, _s())
    ktimer.end(tk)
    return grad


def stem_prep(x_nchw, xp):
    N, _, H, W = x_nchw.shape
    lib().vlp_stem_prep(dcode(xp), ptr(x_nchw), ptr(xp), N, H, W, _s())


def stem_prep_u8(x_u8, xp, mean, std):
    N, H, W = x_u8.shape[0], x_u8.shape[-2], x_u8.shape[-1]
    lib().vlp_stem_prep_u8(dcode(xp), ptr(x_u8), ptr(xp), N, H, W, float(mean), float(std), _s())


def stem_fwd(xp, wp, N, H, W, y, stat_sum, stat_sumsq, stat_rep=1):
    tk = ktimer.begin("stem_fwd", 2.0 * y.numel() * 147)
    lib().vlp_stem_fwd(dcode(xp), ptr(xp), ptr(wp), ptr(y), N, H, W, ptr(stat_sum),
                       ptr(stat_sumsq), int(stat_rep), _s())
    ktimer.end(tk)


def stem_wgrad(dy, xp, N, H, W, dw_ws):
    tk = ktimer.begin("stem_wgrad", 2.0 * dy.numel() * 147)
    lib().vlp_stem_wgrad(dcode(dy), ptr(dy), ptr(xp), ptr(dw_ws), N, H, W, _s())
    ktimer.end(tk)


# ---------------- BN / pooling ----------------
def stat_reduce(rep, C, a, b=None, c=None):
    lib().vlp_stat_reduce(int(rep), int(C), ptr(a), ptr(b), ptr(c), _s())


def bn_finalize_rep(rep, count, s, ss, gamma, beta, eps, momentum, running_mean, running_var, scale, shift,
                    mean, invstd):
    """Fold the [rep][C] replicated sums and finalize in one launch."""
    lib().vlp_bn_finalize_rep(int(rep), gamma.numel(), float(count), ptr(s), ptr(ss), ptr(gamma), ptr(beta),
                              float(eps), float(momentum), ptr(running_mean), ptr(running_var),
                              ptr(scale), ptr(shift), ptr(mean), ptr(invstd), _s())


def bn_grad_rep(rep, C, sum_g, sum_gx, dgamma, dbeta, sum_gxd=None, dgamma_d=None, dbeta_d=None):
    lib().vlp_bn_grad_rep(int(rep), int(C), ptr(sum_g), ptr(sum_gx), ptr(sum_gxd), ptr(dgamma), ptr(dbeta),
                          ptr(dgamma_d), ptr(dbeta_d), _s())


def bn_finalize(count, s, ss, gamma, beta, eps, momentum, running_mean, running_var, scale, shift,
                mean, invstd):
    lib().vlp_bn_finalize(gamma.numel(), float(count), ptr(s), ptr(ss), ptr(gamma), ptr(beta),
                          float(eps), float(momentum), ptr(running_mean), ptr(running_var),
                          ptr(scale), ptr(shift), ptr(mean), ptr(invstd), _s())


def bn_eval_coeffs(gamma, beta, rm, rv, eps, scale, shift):
    lib().vlp_bn_eval_coeffs(gamma.numel(), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), float(eps),
                             ptr(scale), ptr(shift), _s())


def bn_add_relu(y, sc, sh, idt, scd, shd, out, relu_mask=None):
    C = y.shape[-1]
    M = y.numel() // C
    lib().vlp_bn_add_relu(dcode(y), M, C, ptr(y), ptr(sc), ptr(sh), ptr(idt), ptr(scd), ptr(shd),
                          ptr(out), ptr(relu_mask), _s())


def bn_bwd_reduce(M, C, dout, dbc, HW, mask, ya, mean_a, istd_a, yb, mean_b, istd_b, sum_g, sum_ga,
                  sum_gb, dtype_ref, stat_rep=1):
    lib().vlp_bn_bwd_reduce(dcode(dtype_ref), M, C, ptr(dout), ptr(dbc), HW, ptr(mask), ptr(ya),
                            ptr(mean_a), ptr(istd_a), ptr(yb), ptr(mean_b), ptr(istd_b), ptr(sum_g),
                            ptr(sum_ga), ptr(sum_gb), int(stat_rep), _s())


def bn_bwd_apply(M, C, dout, dbc, HW, mask, A, B, g_out, dtype_ref):
    """A/B = (y, mean, istd, gamma, sum_g, sum_gx, dy_out) or None."""
    a = A if A is not None else (None,) * 7
    b = B if B is not None else (None,) * 7
    lib().vlp_bn_bwd_apply(dcode(dtype_ref), M, C, ptr(dout), ptr(dbc), HW, ptr(mask),
                           *[ptr(t) for t in a], *[ptr(t) for t in b], ptr(g_out), _s())


def bn_param_grad(sum_g, sum_gx, dgamma, dbeta):
    lib().vlp_bn_param_grad(dgamma.numel(), ptr(sum_g), ptr(sum_gx), ptr(dgamma), ptr(dbeta), _s())


def maxpool_fwd(y, sc, sh, out, idx, yarg=None, relu_mask=None):
    N, H, W, C = y.shape
    lib().vlp_maxpool_fwd(dcode(y), N, H, W, C, ptr(y), ptr(sc), ptr(sh), ptr(out), ptr(idx), ptr(yarg),
                          ptr(relu_mask), _s())


def maxpool_bwd(dp, idx, y, sc, sh, mean, istd, sum_g, sum_gx, stat_rep=1):
    """BN backward sums of the routed, ReLU-masked stem gradient (nothing stored)."""
    N, H, W, C = y.shape
    lib().vlp_maxpool_bwd(dcode(y), N, H, W, C, ptr(dp), ptr(idx), ptr(y), ptr(sc), ptr(sh),
                          ptr(mean), ptr(istd), ptr(sum_g), ptr(sum_gx), int(stat_rep), _s())


def maxpool_bwd_apply(dp, idx, y, sc, sh, mean, istd, gamma, sum_g, sum_gx, dy):
    """dy = BN1'(relu-masked routed gradient), recomputing the routing."""
    N, H, W, C = y.shape
    lib().vlp_maxpool_bwd_apply(dcode(y), N, H, W, C, ptr(dp), ptr(idx), ptr(y), ptr(sc), ptr(sh),
                                ptr(mean), ptr(istd), ptr(gamma), ptr(sum_g), ptr(sum_gx), ptr(dy), _s())


def avgpool_fwd(x, feat):
    N, H, W, C = x.shape
    lib().vlp_avgpool_fwd(dcode(x), N, H * W, C, ptr(x), ptr(feat), _s())


# ---------------- text tower ----------------
def linear_fwd(x, w, bias, y, M, N, K, ldx=None, ldy=None, mode=0, aux=None, res=None, ldr=None,
               p=0.0, seed=0):
    tk = ktimer.begin(f"linear_fwd{_tile_lin(M, N)}", 2.0 * M * N * K)
    lib().vlp_linear_fwd(dcode(x), M, N, K, ptr(x), ldx or K, ptr(w), ptr(bias), ptr(y), ldy or N,
                         mode, ptr(aux), ptr(res), ldr or N, float(p), int(seed), _s())
    ktimer.end(tk)


def linear_fwd_rs(x, w, bias, y, res, rscale, rps, M, N, K):
    """y = res + rscale[row // rps] * (x W^T + bias)  (residual branch under DropPath)."""
    tk = ktimer.begin(f"linear_fwd{_tile_lin(M, N)}", 2.0 * M * N * K)
    lib().vlp_linear_fwd_rs(dcode(x), M, N, K, ptr(x), K, ptr(w), ptr(bias), ptr(y), N, ptr(res), N, ptr(rscale),
                            int(rps), _s())
    ktimer.end(tk)


def linear_dgrad(dy, w, dx, M, Kin, Nout, lddy=None, lddx=None, mode=0, aux=None, ldaux=None,
                 addend=None, ldad=None):
    tk = ktimer.begin(f"linear_dgrad{_tile_lin(M, Kin)}", 2.0 * M * Kin * Nout)
    lib().vlp_linear_dgrad(dcode(dy), M, Kin, Nout, ptr(dy), lddy or Nout, ptr(w), ptr(dx),
                           lddx or Kin, mode, ptr(aux), ldaux or Kin, ptr(addend), ldad or Kin, _s())
    ktimer.end(tk)


def _linw_ws(device, elems):
    """Split-K slabs of the linear weight gradients: per (device, stream), so the
    text tower's backward on its own stream and NesT's on the main stream never
    share (or free under each other) a workspace."""
    return _stream_ws("linw", device, elems)


def linear_wgrad(dy, x, dw, M, Nout, Kin, lddy=None, ldx=None):
    """dw[Nout][Kin] += dy^T x.  bf16: split-K partial slabs in a cached fp32
    workspace folded by one reduction pass; fp32: atomic split-K."""
    tk = ktimer.begin("linear_wgrad/wide", 2.0 * M * Nout * Kin)
    if dy.dtype == torch.bfloat16 and Kin % 4 == 0:
        n =ctypes.c_longlong(0)
        lib().vlp_linear_wgrad_ws_floats(M, Nout, Kin, ctypes.byref(n))
        ws = _linw_ws(dy.device, max(n.value, 16 * Nout * Kin))
        lib().vlp_linear_wgrad_ws(dcode(dy), M, Nout, Kin, ptr(dy), lddy or Nout, ptr(x), ldx or Kin,
                                  ptr(dw), ptr(ws), ws.numel(), _s())
    else:
        lib().vlp_linear_wgrad(dcode(dy), M, Nout, Kin, ptr(dy), lddy or Nout, ptr(x), ldx or Kin,
                               ptr(dw), _s())
    ktimer.end(tk)


def colsum(x, out, M, N, ld=None):
    lib().vlp_colsum(dcode(x), M, N, ptr(x), ld or N, ptr(out), _s())


def layernorm_fwd(x, gamma, beta, eps, y, mean, rstd, M, D, p=0.0, seed=0):
    lib().vlp_layernorm_fwd(dcode(x), M, D, ptr(x), ptr(gamma), ptr(beta), float(eps), ptr(y),
                            ptr(mean), ptr(rstd), float(p), int(seed), _s())


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dxd, dgamma, dbeta, M, D, p_out=0.0, seed_out=0,
                  p_in=0.0, seed_in=0):
    lib().vlp_layernorm_bwd(dcode(dy), M, D, ptr(dy), float(p_out), int(seed_out), ptr(x),
                            ptr(mean), ptr(rstd), ptr(gamma), ptr(dx), ptr(dxd), float(p_in),
                            int(seed_in), ptr(dgamma), ptr(dbeta), _s())


def attn_fwd(qkv, amask, ctx, P, B, T, H, dh, scale, p=0.0, seed=0):
    lib().vlp_attn_fwd(dcode(qkv), B, T, H, dh, ptr(qkv), ptr(amask), ptr(ctx), ptr(P),
                       float(scale), float(p), int(seed), _s())


def attn_bwd(qkv, P, dctx, dqkv, B, T, H, dh, scale, p=0.0, seed=0):
    lib().vlp_attn_bwd(dcode(qkv), B, T, H, dh, ptr(qkv), ptr(P), ptr(dctx), ptr(dqkv),
                       float(scale), float(p), int(seed), _s())


def embed_fwd(ids, tt, wemb, pemb, temb, e_out, M, T, D):
    lib().vlp_embed_fwd(dcode(e_out), M, T, D, ptr(ids), ptr(tt), ptr(wemb), ptr(pemb), ptr(temb),
                        ptr(e_out), _s())


def embed_bwd(ids, tt, de, dwemb, dpemb, dtemb, M, T, D):
    lib().vlp_embed_bwd(dcode(de), M, T, D, ptr(ids), ptr(tt), ptr(de), ptr(dwemb), ptr(dpemb),
                        ptr(dtemb), _s())


def scatter_rows(src, dst, R, D, ldi, ldo):
    lib().vlp_scatter_rows(dcode(src), R, D, ptr(src), ldi, ptr(dst), ldo, _s())


# ---------------- head ----------------
def l2norm_fwd(x, y, norm):
    R, E = x.shape
    lib().vlp_l2norm_fwd(R, E, ptr(x), ptr(y), ptr(norm), _s())


def l2norm_bwd(y, norm, dy, dx=None, dx_t=None, gscale=None):
    R, E = y.shape
    code = dcode(dx_t) if dx_t is not None else F32
    lib().vlp_l2norm_bwd(code, R, E, ptr(y), ptr(norm), ptr(dy), ptr(gscale), ptr(dx), ptr(dx_t),
                         _s())


def scale(x, s, y, accumulate=False):
    lib().vlp_scale(x.numel(), ptr(x), ptr(s), ptr(y), int(accumulate), _s())


def clip_loss_finish(parts, N, out):
    lib().vlp_clip_loss_finish(ptr(parts), int(N), ptr(out), _s())


def clip_loss_fused(B, N, E, offset, img_all, txt_all, logit_scale, g_img_all, g_txt_all, d_ls,
                    loss_parts, lse_out=None, role_w=None):
    """Global-batch symmetric InfoNCE + gradients (three launches, split over key
    chunks; the scratch is a per-(device, stream) cached workspace)."""
    n = ctypes.c_longlong(0)
    lib().vlp_clip_loss_ws_floats(B, N, E, ctypes.addressof(n))
    ws = _stream_ws("clip", img_all.device, n.value)
    lib().vlp_clip_loss_fused(B, N, E, offset, ptr(img_all), ptr(txt_all), ptr(logit_scale),
                              ptr(g_img_all), ptr(g_txt_all), ptr(d_ls), ptr(loss_parts),
                              ptr(lse_out), ptr(role_w), ptr(ws), ws.numel(), _s())


def _check_cid(cid, n):
    if cid.dtype != torch.int32 or cid.numel() != n or not cid.is_contiguous():
        raise TypeError(f"caption ids must be a contiguous int32 tensor of {n} elements, got "
                        f"{cid.dtype} {tuple(cid.shape)}")


def clip_loss_fused_masked(B, N, E, offset, img_all, txt_all, logit_scale, cid_all, g_img_all, g_txt_all,
                           d_ls, loss_parts, lse_out=None, role_w=None):
    """clip_loss_fused without the duplicate-caption negatives: cid_all int32 [N], entries
    (i, j), i != j, with equal ids are left out of both softmaxes (same workspace)."""
    _check_cid(cid_all, N)
    n = ctypes.c_longlong(0)
    lib().vlp_clip_loss_ws_floats(B, N, E, ctypes.addressof(n))
    ws = _stream_ws("clip", img_all.device, n.value)
    lib().vlp_clip_loss_fused_masked(B, N, E, offset, ptr(img_all), ptr(txt_all), ptr(logit_scale),
                                     ptr(cid_all), ptr(g_img_all), ptr(g_txt_all), ptr(d_ls),
                                     ptr(loss_parts), ptr(lse_out), ptr(role_w), ptr(ws), ws.numel(), _s())


def ce_sym(logits, out, dlogits=None, role_w=None):
    lib().vlp_ce_sym(logits.shape[0], ptr(logits), ptr(out), ptr(dlogits), ptr(role_w), _s())


def ce_sym_masked(logits, cid, out, dlogits=None, role_w=None):
    _check_cid(cid, logits.shape[0])
    lib().vlp_ce_sym_masked(logits.shape[0], ptr(logits), ptr(cid), ptr(out), ptr(dlogits), ptr(role_w), _s())


def matmul(A, B, C, M, N, K, lda, a_kc, ldb, b_kc, ldc, alpha=1.0, accumulate=False, dtype_ref=None):
    ref = dtype_ref if dtype_ref is not None else A
    out_f32 = 1 if C.dtype == torch.float32 else 0
    lib().vlp_matmul(dcode(ref), M, N, K, ptr(A), lda, int(a_kc), ptr(B), ldb, int(b_kc), ptr(C),
                     ldc, out_f32, float(alpha), int(accumulate), _s())


def cast(x, y):
    lib().vlp_cast(dcode(y), x.numel(), ptr(x), ptr(y), _s())


# ---------------- optimizer / packing ----------------
def _step(entry, p, g, m, v, lr, beta1, beta2, eps, wd, step, clip=None, accum=None):
    """One optimizer-step entry point of the library: the bias corrections in fp64 here, then
    the arguments the entry point takes after them: clip = (coef, clip_value) -> mode (1: coef,
    2: clip_value, 0: neither), coef, clip_value;  accum = (acc, w) -> acc, w."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    tail = ()
    if clip is not None:
        coef, clip_value = clip
        tail = (1 if coef is not None else 2 if clip_value is not None else 0, ptr(coef), float(clip_value or 0.0))
    if accum is not None:
        tail += (ptr(accum[0]), float(accum[1]))
    getattr(lib(), entry)(p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), float(lr), float(beta1), float(beta2),
                          float(eps), float(wd), float(lr / bc1), float(bc2 ** 0.5), *tail, _s())


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    _step("vlp_adamw", p, g, m, v, lr, beta1, beta2, eps, wd, step)


def grad_sumsq_nparts(n):
    """Number of fp64 partials vlp_grad_sumsq writes for an n-element span."""
    k = ctypes.c_int(0)
    lib().vlp_grad_sumsq_nparts(int(n), ctypes.byref(k))
    return k.value


def grad_sumsq(g, partials, offset=0):
    """fp64 partial sums of g^2 into partials[offset:]; returns how many were written
    (replaces the per-tensor norms of torch.nn.utils.clip_grad_norm_)."""
    if g.dtype != torch.float32 or partials.dtype != torch.float64 or not g.is_contiguous():
        raise TypeError("grad_sumsq: contiguous fp32 gradients and fp64 partials")
    if offset < 0 or offset + grad_sumsq_nparts(g.numel()) > partials.numel():
        raise ValueError("grad_sumsq: partials buffer too small")
    k = ctypes.c_int(0)
    lib().vlp_grad_sumsq(g.numel(), ptr(g), ptr(partials[offset:]), ctypes.byref(k), _s())
    return k.value


def clip_coef(nparts, partials, max_norm, out):
    """out[0] = global gradient norm, out[1] = min(1, max_norm / (norm + 1e-6)) (fp32 [2])."""
    if nparts > partials.numel() or out.numel() < 2 or out.dtype != torch.float32 or partials.dtype != torch.float64:
        raise ValueError("clip_coef: nparts fp64 partials and an fp32 [2] output")
    lib().vlp_clip_coef(int(nparts), ptr(partials), float(max_norm), ptr(out), _s())


def adamw_clip(p, g, m, v, lr, beta1, beta2, eps, wd, step, coef=None, clip_value=None):
    """adamw on the clipped gradient (written back to g): g * coef[0] with coef a device
    fp32 tensor (norm clipping), else clamp(g, -clip_value, clip_value)."""
    if (coef is None) == (clip_value is None):
        raise ValueError("adamw_clip: exactly one of coef / clip_value")
    _step("vlp_adamw_clip", p, g, m, v, lr, beta1, beta2, eps, wd, step, clip=(coef, clip_value))


def _f32_flat(name, *ts):
    for t in ts:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError(f"{name}: contiguous fp32 tensors")
    if any(t.numel() != ts[0].numel() for t in ts):
        raise ValueError(f"{name}: operands of one length")


def grad_accum(acc, g, w=1.0, first=False):
    """acc = (0 if first else acc) + w * g; first=True never reads acc (gradient accumulation
    over the flat arenas, whose backward overwrites g)."""
    _f32_flat("grad_accum", acc, g)
    lib().vlp_grad_accum(g.numel(), ptr(acc), ptr(g), float(w), 1 if first else 0, _s())


def grad_accum_sumsq(acc, g, w, partials, offset=0):
    """grad_sumsq of acc + w * g (which is not stored) into partials[offset:]; returns how many
    partials were written."""
    _f32_flat("grad_accum_sumsq", acc, g)
    if partials.dtype != torch.float64:
        raise TypeError("grad_accum_sumsq: fp64 partials")
    if offset < 0 or offset + grad_sumsq_nparts(g.numel()) > partials.numel():
        raise ValueError("grad_accum_sumsq: partials buffer too small")
    k = ctypes.c_int(0)
    lib().vlp_grad_accum_sumsq(g.numel(), ptr(acc), ptr(g), float(w), ptr(partials[offset:]), ctypes.byref(k), _s())
    return k.value


def adamw_clip_accum(p, g, m, v, lr, beta1, beta2, eps, wd, step, acc, w=1.0, coef=None, clip_value=None):
    """adamw on acc + w * g, scaled by coef[0] (device fp32, norm clipping), clamped to
    +-clip_value, or as it is (neither given); g and acc are not written.  acc=None is
    adamw_clip(p, g, ...), which needs one of coef / clip_value."""
    if coef is not None and clip_value is not None:
        raise ValueError("adamw_clip_accum: at most one of coef / clip_value")
    if acc is None and coef is None and clip_value is None:
        raise ValueError("adamw_clip_accum: without an accumulator one of coef / clip_value (else adamw)")
    _f32_flat("adamw_clip_accum", p, g, m, v, *(() if acc is None else (acc,)))
    _step("vlp_adamw_clip_accum", p, g, m, v, lr, beta1, beta2, eps, wd, step, clip=(coef, clip_value), accum=(acc, w))


def adam_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, acc=None, w=1.0, coef=None, clip_value=None):
    """torch.optim.Adam's step (weight decay as an L2 term of the gradient, added after the
    clipping) on acc + w * g, or on g alone (acc=None), scaled by coef[0] (device fp32, norm
    clipping), clamped to +-clip_value, or as it is (neither given).  With acc, g and acc are
    not written; without, the clipped gradient is written back to g."""
    if coef is not None and clip_value is not None:
        raise ValueError("adam_step: at most one of coef / clip_value")
    _f32_flat("adam_step", p, g, m, v, *(() if acc is None else (acc,)))
    _step("vlp_adam_step", p, g, m, v, lr, beta1, beta2, eps, wd, step, clip=(coef, clip_value), accum=(acc, w))


def pack_conv(w, wp, wt):
    Co, C, KH, KW = w.shape
    ref = wp if wp is not None else wt
    lib().vlp_pack_conv(dcode(ref), Co, C, KH, KW, ptr(w), ptr(wp), ptr(wt), _s())


def pack_conv_batch(dtype_ref, entries):
    """entries: [(w fp32 [Co][C][KH][KW], wp, wt)] packed in one launch.
    Returns the ctypes descriptor table (reusable with pack_conv_batch_run)."""
    rows = []
    for w, wp, wt in entries:
        Co, C, KH, KW = w.shape
        rows += [w.data_ptr(), wp.data_ptr() if wp is not None else 0, wt.data_ptr() if wt is not None else 0,
                 Co, C, KH * KW]
    table = (ctypes.c_longlong * len(rows))(*rows)
    return (dcode(dtype_ref), len(entries), table)


def pack_conv_batch_run(desc):
    code, n, table = desc
    lib().vlp_pack_conv_batch(code, n, ctypes.addressof(table), _s())


def pack_stem(w, wp):
    lib().vlp_pack_stem(dcode(wp), ptr(w), ptr(wp), _s())


def unpack_conv_grad(ws, g):
    Co, C, KH, KW = g.shape
    lib().vlp_unpack_conv_grad(Co, C, KH, KW, ptr(ws), ptr(g), _s())


def unpack_stem_grad(ws, g):
    lib().vlp_unpack_stem_grad(ptr(ws), ptr(g), _s())


# ---------------- retrieval metrics ----------------
SIM_CHUNK_BYTES = 256 << 20


def sim_topk(q, keys, K):
    """Top-K (values, indices) of q @ keys^T per row, descending (ties to the
    lower index), without materialising the full similarity matrix: query
    chunks of <= 256 MB of fp32 similarities, each an fp32 GEMM
    (vlp_linear_fwd) reduced by vlp_row_topk.  q [Q, E], keys [N, E] fp32."""
    q = q.float().contiguous()
    keys = keys.float().contiguous()
    if q.shape[1] % 4:   # 16-B operand rows: zero columns leave every dot product unchanged
        pad = 4 - q.shape[1] % 4
        q = torch.nn.functional.pad(q, (0, pad))
        keys = torch.nn.functional.pad(keys, (0, pad))
    Q, E = q.shape
    N = keys.shape[0]
    Np = (N + 3) // 4 * 4   # 16-B rows for the GEMM epilogue
    vals = torch.empty(Q, K, device=q.device)
    idx = torch.empty(Q, K, dtype=torch.int32, device=q.device)
    rows = max(1, min(Q, SIM_CHUNK_BYTES // (4 * Np)))
    tile = torch.empty(rows, Np, device=q.device)
    for r0 in range(0, Q, rows):
        r = min(rows, Q - r0)
        linear_fwd(q[r0:r0 + r], keys, None, tile, r, N, E, ldy=Np)
        lib().vlp_row_topk(r, N, ptr(tile), Np, K, ptr(vals[r0:r0 + r]), ptr(idx[r0:r0 + r]), _s())
    return vals, idx.long()


# ---------------- post-fit silhouette scores ----------------
MAX_CLUSTERS = 8   # kMaxClusters of csrc/retrieval_ops.hip


def cluster_dist_sums(x, labels_i32, C, xq=None):
    """[Q, C] fp32: out[q, c] = sum over rows j of x with labels_i32[j] == c of
    ||xq[q] - x[j]||_2 (xq defaults to x), every distance from direct fp32
    differences (vlp_cluster_dist_sums: one launch, no Q x N matrix, bitwise
    reproducible).  x [N, D], xq [Q, D]; C <= 8 and every label in [0, C), else
    ValueError -- the label range is read back once, the only host sync here."""
    C = int(C)
    if not 1 <= C <= MAX_CLUSTERS:
        raise ValueError(f"cluster_dist_sums: C={C}, the kernel keeps 1 to {MAX_CLUSTERS} clusters")
    x = x.float().contiguous()
    xq = x if xq is None else xq.float().contiguous()
    labels_i32 = labels_i32.to(device=x.device, dtype=torch.int32).contiguous()
    N, D = x.shape
    Q = xq.shape[0]
    if xq.dim() != 2 or xq.shape[1] != D or labels_i32.shape != (N,):
        raise ValueError(f"cluster_dist_sums: x {tuple(x.shape)}, xq {tuple(xq.shape)}, "
                         f"labels {tuple(labels_i32.shape)} do not fit")
    if N and not (0 <= int(labels_i32.min()) and int(labels_i32.max()) < C):
        raise ValueError(f"cluster_dist_sums: labels must lie in [0, {C})")
    out = torch.empty(Q, C, dtype=torch.float32, device=x.device)
    lib().vlp_cluster_dist_sums(Q, N, D, ptr(xq), D, ptr(x), D, ptr(labels_i32), C, ptr(out), _s())
    return out


# ---------------- post-fit t-SNE ----------------
TSNE_MAX_N = 32768   # kTsneMaxN of csrc/tsne_ops.hip: P [N, N] fp32 stays within 4 GB
TSNE_PARTS = 7       # kParts: doubles per row of the all-pairs pass


def tsne_sqdist(x):
    """[N, N] fp32 squared Euclidean distances of the rows of x [N, D] (direct
    differences: zero diagonal, symmetric bit for bit)."""
    x = x.float().contiguous()
    N, D = x.shape
    d2 = torch.empty(N, N, dtype=torch.float32, device=x.device)
    lib().vlp_tsne_sqdist(N, D, ptr(x), D, ptr(d2), N, _s())
    return d2


def tsne_affinities(d2, perplexity, return_conditional=False):
    """sklearn's joint probabilities P [N, N] fp32 of the squared distances d2
    [N, N] fp32 (vlp_tsne_affinities); with return_conditional also the
    conditional matrix the bisection left, fp32."""
    d2 = d2.float().contiguous()
    N = d2.shape[0]
    if d2.shape != (N, N):
        raise ValueError(f"tsne_affinities: d2 must be square, got {tuple(d2.shape)}")
    cond = torch.empty(N, N, dtype=torch.float32, device=d2.device)
    P = torch.empty(N, N, dtype=torch.float32, device=d2.device)
    ws = torch.empty(N + 1, dtype=torch.float64, device=d2.device)
    lib().vlp_tsne_affinities(N, ptr(d2), N, float(perplexity), ptr(cond), ptr(ws), ptr(P), _s())
    return (P, cond) if return_conditional else P


def tsne_pairs(y, P, parts, check):
    """parts [N, 7] fp64 <- the per-row sums of one iteration over y [N, 2], P [N, N]."""
    N = y.shape[0]
    assert y.shape == (N, 2) and P.shape == (N, N) and parts.shape == (N, TSNE_PARTS)
    assert y.is_contiguous() and P.is_contiguous() and parts.is_contiguous()
    assert y.dtype == P.dtype == torch.float32 and parts.dtype == torch.float64
    lib().vlp_tsne_pairs(N, ptr(y), ptr(P), ptr(parts), int(bool(check)), _s())


def tsne_update(parts, y, update, gains, exag, momentum, lr, check, stats):
    """One gains + momentum step in place on y, update, gains [N, 2] fp32; when
    check, stats [2] fp64 <- (KL, norm of the gained gradient)."""
    N = y.shape[0]
    for t in (y, update, gains):
        assert t.shape == (N, 2) and t.dtype == torch.float32 and t.is_contiguous()
    assert parts.shape == (N, TSNE_PARTS) and parts.dtype == torch.float64 and parts.is_contiguous()
    assert stats.shape == (2,) and stats.dtype == torch.float64
    lib().vlp_tsne_update(N, ptr(parts), ptr(y), ptr(update), ptr(gains), float(exag), float(momentum), float(lr),
                          int(bool(check)), ptr(stats), _s())


# ---------------- the linear probe's logistic regression ----------------
LOGREG_ROWS = 32      # kLrRows of csrc/logreg_ops.hip: rows of X per workgroup (one partial each)
LOGREG_MAX_D = 2048   # kLrMaxD
LOGREG_STATE = 10     # doubles of device state; the host reads the first LOGREG_STATUS of them
LOGREG_STATUS = 5     # f, |g|_inf, g.d, f(trial), CG steps taken
LOGREG_GRAD, LOGREG_HVP, LOGREG_LOSS, LOGREG_SCORES = 0, 1, 2, 3


def logreg_nparts(N):
    return (int(N) + LOGREG_ROWS - 1) // LOGREG_ROWS


def logreg_pass(mode, x, y, u, s=None, parts=None, z=None, state=None):
    """One pass of vlp_logreg_pass over x [N, D] fp32 (any row stride >= D, unit column stride)
    at u [D + 1] fp64; y, s, z [N] fp64, parts [ceil(N / 32), D + 2] fp64, as the mode needs."""
    N, D = x.shape
    assert x.dtype == torch.float32 and x.stride(1) == 1 and u.dtype == torch.float64 and u.shape == (D + 1,)
    for t in (y, u, s, parts, z, state):
        assert t is None or (t.dtype == torch.float64 and t.is_contiguous())
    assert parts is None or parts.shape == (logreg_nparts(N), D + 2)
    assert all(t is None or t.shape == (N,) for t in (y, s, z))
    ldx = x.stride(0) if N > 1 else D
    lib().vlp_logreg_pass(int(mode), N, D, ptr(x), ldx, ptr(y), ptr(u), ptr(s), ptr(parts), ptr(z), ptr(state),
                          _s())


def _logreg_vec_ok(D, vec, state):
    assert vec.shape == (4, D + 1) and vec.dtype == torch.float64 and vec.is_contiguous()
    assert state.shape == (LOGREG_STATE,) and state.dtype == torch.float64


def logreg_newton_begin(N, D, C, parts, w, tol, vec, state):
    """vec [4, D + 1] = (g, 0, -g, -g) and the state from the GRAD partials at w [D + 1]."""
    _logreg_vec_ok(D, vec, state)
    assert parts.shape == (logreg_nparts(N), D + 2) and parts.dtype == w.dtype == torch.float64
    assert w.shape == (D + 1,) and parts.is_contiguous()
    lib().vlp_logreg_newton_begin(N, D, float(C), ptr(parts), ptr(w), float(tol), ptr(vec), ptr(state), _s())


def logreg_cg_step(N, D, C, parts, vec, state):
    """One conjugate-gradient update of vec (d, r, q) from the HVP partials at q."""
    _logreg_vec_ok(D, vec, state)
    assert parts.shape == (logreg_nparts(N), D + 2) and parts.dtype == torch.float64 and parts.is_contiguous()
    lib().vlp_logreg_cg_step(N, D, float(C), ptr(parts), ptr(vec), ptr(state), _s())


def logreg_trial(N, D, C, w, t, vec, wt, state):
    """wt [D + 1] = w + t d, and its penalty into the state."""
    _logreg_vec_ok(D, vec, state)
    assert w.shape == wt.shape == (D + 1,) and w.dtype == wt.dtype == torch.float64
    lib().vlp_logreg_trial(N, D, float(C), ptr(w), float(t), ptr(vec), ptr(wt), ptr(state), _s())


def logreg_trial_loss(N, D, parts, state):
    """state[3] = f(wt) from the LOSS partials at wt."""
    assert parts.shape == (logreg_nparts(N), D + 2) and parts.dtype == torch.float64 and parts.is_contiguous()
    assert state.shape == (LOGREG_STATE,) and state.dtype == torch.float64
    lib().vlp_logreg_trial_loss(N, D, ptr(parts), ptr(state), _s())


# ---------------- the baselines' binary classification metrics ----------------
BINMETRIC_TILE = 256         # kBmThreads = kBmTile of csrc/binmetric_ops.hip: the i tile and the j tile
BINMETRIC_MAX_N = 1 << 18    # kBmMaxN: the ceiling of the O(n^2) pair count
BINMETRIC_BLOCKS = 1024      # workgroups the pair count aims for (four per CU) when it splits the j range
_BINMETRIC_KIND = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}


def binmetric_append(prob, label, scores, labels, offset, counts):
    """scores[offset : offset + n] = prob, labels[offset : offset + n] = label as 0 / 1 (2 for any
    other value) and counts [4] int64 += the batch's tp, fp, fn, tn at prob >= 0.5
    (vlp_binmetric_append: one launch, nothing read back).  prob [n] fp32; label [n] int64, int32,
    uint8 or bool."""
    n = prob.numel()
    if label.dtype == torch.bool:
        label = label.view(torch.uint8)
    if label.dtype not in _BINMETRIC_KIND:
        raise TypeError(f"binmetric_append: labels must be int64, int32, uint8 or bool, got {label.dtype}")
    assert prob.dtype == torch.float32 and prob.is_contiguous() and label.is_contiguous() and label.numel() == n
    assert scores.dtype == torch.float32 and labels.dtype == torch.uint8 and scores.numel() == labels.numel()
    assert scores.is_contiguous() and labels.is_contiguous()
    assert counts.dtype == torch.int64 and counts.shape == (4,)
    if not 0 <= offset <= scores.numel() - n:
        raise ValueError(f"binmetric_append: rows [{offset}, {offset + n}) do not fit {scores.numel()} slots")
    lib().vlp_binmetric_append(n, ptr(prob), ptr(label), _BINMETRIC_KIND[label.dtype], ptr(scores), ptr(labels),
                               int(offset), scores.numel(), ptr(counts), _s())


def binmetric_grid(n):
    """(workgroups along i, splits of the j range) of the pair count over n rows: the j range is
    split until about BINMETRIC_BLOCKS workgroups run, one tile of j at the least per split."""
    bx = (int(n) + BINMETRIC_TILE - 1) // BINMETRIC_TILE
    return bx, max(1, min(bx, (BINMETRIC_BLOCKS + bx - 1) // bx))


def binmetric_counts(n, scores, labels, counts):
    """int64 [6] on the device: tp, fp, fn, tn (counts) and the pair counts wins, ties over the first
    n rows of scores / labels (vlp_binmetric_pairs + vlp_binmetric_fold).  n <= BINMETRIC_MAX_N."""
    if not 0 <= n <= min(BINMETRIC_MAX_N, scores.numel()):
        raise ValueError(f"binmetric_counts: n={n}; the pair count takes 0 to "
                         f"{min(BINMETRIC_MAX_N, scores.numel())} rows")
    assert scores.dtype == torch.float32 and labels.dtype == torch.uint8 and scores.numel() == labels.numel()
    assert counts.dtype == torch.int64 and counts.shape == (4,)
    out = torch.empty(6, dtype=torch.int64, device=scores.device)
    parts, nparts = None, 0
    if n:
        bx, splits = binmetric_grid(n)
        nparts = bx * splits
        parts = torch.empty(nparts, 2, dtype=torch.int64, device=scores.device)
        lib().vlp_binmetric_pairs(n, ptr(scores), ptr(labels), splits, ptr(parts), _s())
    lib().vlp_binmetric_fold(nparts, ptr(parts), ptr(counts), ptr(out), _s())
    return out


# ---------------- the test-set evaluation's per-subgroup counts ----------------
GROUPMETRIC_MAX_LEVELS = 8     # kGmMaxLevels of csrc/groupmetric_ops.hip: one byte per level in 64 bits
GROUPMETRIC_MAX_GROUPS = 255   # kGmMaxGroups: codes 0 .. 254
GROUPMETRIC_NO_GROUP = 255     # the code of a row that is in no group of a level


def groupmetric_check(scores, labels, codes, n_groups):
    """(n, L, cell_base) of a grouped count's arguments; ValueError on shapes or sizes the op does
    not take.  Nothing but the tensors' shapes is read: no library call, no device access."""
    n_groups = [int(g) for g in n_groups]
    L = len(n_groups)
    if not 1 <= L <= GROUPMETRIC_MAX_LEVELS:
        raise ValueError(f"groupmetric: {L} levels; 1 to {GROUPMETRIC_MAX_LEVELS} are supported")
    for l, g in enumerate(n_groups):
        if not 1 <= g <= GROUPMETRIC_MAX_GROUPS:
            raise ValueError(f"groupmetric: level {l} declares {g} groups; 1 to {GROUPMETRIC_MAX_GROUPS} are "
                             f"supported")
    if scores.dim() != 1 or labels.dim() != 1 or codes.dim() != 2:
        raise ValueError(f"groupmetric: scores [n], labels [n] and codes [L, n], got {tuple(scores.shape)}, "
                         f"{tuple(labels.shape)} and {tuple(codes.shape)}")
    n = scores.shape[0]
    if labels.shape[0] != n or codes.shape[1] != n or codes.shape[0] != L:
        raise ValueError(f"groupmetric: {n} scores, {labels.shape[0]} labels, codes {tuple(codes.shape)} and "
                         f"{L} group counts do not match")
    if not 1 <= n <= BINMETRIC_MAX_N:
        raise ValueError(f"groupmetric: n={n}; the pair count takes 1 to {BINMETRIC_MAX_N} rows")
    cell_base = [0]
    for g in n_groups:
        cell_base.append(cell_base[-1] + g)
    return n, L, cell_base


def groupmetric_ws_bytes(n, L, cells):
    b = ctypes.c_longlong(0)
    lib().vlp_groupmetric_ws_bytes(int(n), int(L), int(cells), ctypes.byref(b))
    return b.value


def groupmetric_counts(scores, labels, codes, n_groups):
    """int64 [cells, 6] on the device: tp, fp, fn, tn, wins, ties of every group of every level
    (vlp_groupmetric_counts: two launches, nothing read back).  scores [n] fp32; labels [n] uint8 (1,
    0, or 2 = counted nowhere); codes [L, n] uint8, row i's group per level or 255 for none;
    n_groups the levels' group counts.  Level l's group g is row sum(n_groups[:l]) + g."""
    n, L, cell_base = groupmetric_check(scores, labels, codes, n_groups)
    if scores.dtype != torch.float32 or labels.dtype != torch.uint8 or codes.dtype != torch.uint8:
        raise TypeError(f"groupmetric_counts: scores fp32, labels uint8 and codes uint8, got {scores.dtype}, "
                        f"{labels.dtype} and {codes.dtype}")
    assert scores.is_contiguous() and labels.is_contiguous() and codes.is_contiguous()
    assert labels.device == scores.device and codes.device == scores.device
    cells = cell_base[-1]
    out = torch.empty(cells, 6, dtype=torch.int64, device=scores.device)
    nbytes = groupmetric_ws_bytes(n, L, cells)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=scores.device)
    base = (ctypes.c_int * (L + 1))(*cell_base)
    lib().vlp_groupmetric_counts(n, ptr(scores), ptr(labels), L, ptr(codes), ctypes.cast(base, ctypes.c_void_p),
                                 ptr(out), ptr(ws), nbytes, _s())
    return out


# ---------------- the baselines' weighted BCE + CORAL loss ----------------
DOMAIN_LOSS_MAX_N = 1 << 18   # kDlMaxN of csrc/domain_loss_ops.hip
DOMAIN_LOSS_MAX_D = 2048      # kDlMaxD


def domain_loss_ws_bytes(N, D):
    n = ctypes.c_longlong(0)
    lib().vlp_domain_loss_ws_bytes(int(N), int(D), ctypes.byref(n))
    return n.value


def domain_loss(feat, logits, label, domain, w0, w1, coral_lambda, grad=True):
    """(out, g_feat, g_logits) of vlp_domain_loss: out [3] fp64 = total, cls, coral on the device,
    g_feat [N, D] fp32 = d coral / d feat and g_logits [N] fp32 = d cls / d logits (both None when
    grad is false: the gradient pass is skipped).  feat [N, D] fp32 (any row stride >= D, unit
    column stride); logits [N] fp32; label [N] int64, int32, uint8 or bool; domain [N] uint8 codes
    (0 source, 1 target, else neither).  Nothing is read back."""
    N, D = feat.shape
    if not (0 <= N <= DOMAIN_LOSS_MAX_N and 1 <= D <= DOMAIN_LOSS_MAX_D):
        raise ValueError(f"domain_loss: N={N}, D={D}; 0 to {DOMAIN_LOSS_MAX_N} rows and 1 to "
                         f"{DOMAIN_LOSS_MAX_D} columns")
    if label.dtype == torch.bool:
        label = label.view(torch.uint8)
    if label.dtype not in _BINMETRIC_KIND:
        raise TypeError(f"domain_loss: labels must be int64, int32, uint8 or bool, got {label.dtype}")
    assert feat.dtype == torch.float32 and feat.stride(1) == 1 and (N <= 1 or feat.stride(0) >= D)
    assert logits.dtype == torch.float32 and logits.shape == (N,) and logits.is_contiguous()
    assert label.shape == (N,) and label.is_contiguous()
    assert domain.dtype == torch.uint8 and domain.shape == (N,) and domain.is_contiguous()
    dev = feat.device
    out = torch.empty(3, dtype=torch.float64, device=dev)
    g_feat = torch.empty(N, D, dtype=torch.float32, device=dev) if grad else None
    g_logits = torch.empty(N, dtype=torch.float32, device=dev) if grad else None
    nbytes = domain_loss_ws_bytes(N, D)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    ldf = feat.stride(0) if N > 1 else D
    lib().vlp_domain_loss(N, D, ptr(feat), ldf, ptr(logits), ptr(label), _BINMETRIC_KIND[label.dtype], ptr(domain),
                          float(w0), float(w1), float(coral_lambda), ptr(out), ptr(g_feat), ptr(g_logits), ptr(ws),
                          nbytes, _s())
    return out, g_feat, g_logits


# ---------------- NesT image encoder ----------------
def nest_attn_fwd(qkv, out, lse, BT, H, N, scale):
    tk = ktimer.begin("nest_attn_fwd", 4.0 * BT * H * N * N * 32)
    lib().vlp_nest_attn_fwd(dcode(qkv), BT, H, N, 32, ptr(qkv), ptr(out), ptr(lse), float(scale), _s())
    ktimer.end(tk)


def nest_attn_bwd(qkv, out, dout, lse, delta, dqkv, BT, H, N, scale):
    tk = ktimer.begin("nest_attn_bwd", 10.0 * BT * H * N * N * 32)
    lib().vlp_nest_attn_bwd(dcode(qkv), BT, H, N, 32, ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(delta),
                            ptr(dqkv), float(scale), _s())
    ktimer.end(tk)


def nest_blockify(x, y, B, Hg, Wg, bs, C, pos=None, inverse=False):
    lib().vlp_nest_blockify(dcode(x), B, Hg, Wg, bs, C, ptr(x), ptr(pos), ptr(y), int(inverse), _s())


def nest_pos_grad(dy, dpos, B, TN, C):
    lib().vlp_nest_pos_grad(dcode(dy), B, TN, C, ptr(dy), ptr(dpos), _s())


def nest_maxpool_fwd(x, y, idx):
    B, H, W, C = x.shape
    lib().vlp_nest_maxpool_fwd(dcode(x), B, H, W, C, ptr(x), ptr(y), ptr(idx), _s())


def nest_maxpool_bwd(dy, idx, dx):
    B, H, W, C = dx.shape
    lib().vlp_nest_maxpool_bwd(dcode(dy), B, H, W, C, ptr(dy), ptr(idx), ptr(dx), _s())


def nest_patch_prep(out, B, H, W, bs, x=None, x_u8=None, mean=0.0, std=1.0):
    lib().vlp_nest_patch_prep(dcode(out), B, H, W, bs, ptr(x), ptr(x_u8), float(mean), float(std), ptr(out), _s())


def nest_add_bias(y, bias, M, N):
    lib().vlp_nest_add_bias(dcode(y), M, N, ptr(y), ptr(bias), _s())


def nest_permute_cols(src, dst, Nr, H, Dh):
    lib().vlp_nest_permute_cols(dcode(dst), Nr, H, Dh, ptr(src), ptr(dst), _s())


def nest_unpermute_cols(src, dst, Nr, H, Dh):
    lib().vlp_nest_unpermute_cols(Nr, H, Dh, ptr(src), ptr(dst), _s())


def nest_rowscale(x, y, s, M, N, rows, mode):
    lib().vlp_nest_rowscale(dcode(x), M, N, rows, ptr(s), ptr(x), ptr(y), int(mode), _s())


def nest_bcast(dfeat, dy, B, HW, C, inv):
    lib().vlp_nest_bcast(dcode(dy), B, HW, C, ptr(dfeat), float(inv), ptr(dy), _s())


def layernorm_bwd_add(dy, x, mean, rstd, gamma, addend, dx, dgamma, dbeta, M, D, dxs=None, rscale=None, rps=1):
    """dx = LN backward + addend; with rscale also dxs = rscale[row // rps] * dx."""
    if rscale is None:
        lib().vlp_layernorm_bwd_add(dcode(dy), M, D, ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma),
                                    ptr(addend), ptr(dx), ptr(dgamma), ptr(dbeta), _s())
    else:
        lib().vlp_layernorm_bwd_add_rs(dcode(dy), M, D, ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma),
                                       ptr(addend), ptr(dx), ptr(dxs), ptr(rscale), int(rps), ptr(dgamma),
                                       ptr(dbeta), _s())


# ---------------- ViT image encoder (csrc/vit_ops.hip; attention: csrc/nest_ops.hip at head dim 64) ----------------
def vit_attn_fwd(qkv, out, lse, B, H, N, scale):
    tk = ktimer.begin("vit_attn_fwd", 4.0 * B * H * N * N * 64)
    lib().vlp_vit_attn_fwd(dcode(qkv), B, H, N, 64, ptr(qkv), ptr(out), ptr(lse), float(scale), _s())
    ktimer.end(tk)


def vit_attn_bwd(qkv, out, dout, lse, delta, dqkv, B, H, N, scale):
    tk = ktimer.begin("vit_attn_bwd", 10.0 * B * H * N * N * 64)
    lib().vlp_vit_attn_bwd(dcode(qkv), B, H, N, 64, ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(delta),
                           ptr(dqkv), float(scale), _s())
    ktimer.end(tk)


def vit_patch_prep(out, B, H, W, x=None, x_u8=None, mean=0.0, std=1.0):
    lib().vlp_vit_patch_prep(dcode(out), B, H, W, ptr(x), ptr(x_u8), float(mean), float(std), ptr(out), _s())


def vit_assemble(patch, cls, pos, tok, B, N, D):
    lib().vlp_vit_assemble(dcode(tok), B, N, D, ptr(patch), ptr(cls), ptr(pos), ptr(tok), _s())


# ---------------- radiograph preprocessing / augmentation (csrc/prep_ops.hip) ----------------
PREP_WORK_BYTES_PER_IMAGE = (64 * 2 + 256 + 2) * 4


def prep_images(src, src_u8, off, hw, n, size, mean, std, channels, out, work):
    """src: packed pixels (device, uint8 or fp32); off [n] int64 / hw [n, 2] int32 (device)."""
    lib().vlp_prep_images(n, ptr(src), int(bool(src_u8)), ptr(off), ptr(hw), int(size), float(mean), float(std),
                          int(channels), ptr(out), ptr(work), _s())


def aug_warp(x, out, maps, noise_std, seed, mean=0.0, std=1.0):
    """x: fp32 [B, Cin, H, W] or uint8 [B, 1, H, W]; out fp32 [B, C, H, W]; maps [B, 6] fp32."""
    B, Cin, H, W = x.shape
    C = out.shape[1]
    lib().vlp_aug_warp(B, Cin, C, H, W, ptr(x), int(x.dtype == torch.uint8), float(mean), float(std), ptr(maps),
                       ptr(noise_std), int(seed) & ((1 << 64) - 1), ptr(out), _s())
