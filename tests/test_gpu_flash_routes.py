"""Every flash-attention route of csrc/nest_ops.hip (vlp_nest_attn_* at head dim 32,
vlp_vit_attn_* at head dim 64) per element against fp64, and the grid-capped NesT elementwise
kernels past their cap.

Method and helpers as tests/test_gpu_text_routes.py (u = 2^-24, r_T = 2^-8 for bf16, 0 for fp32):
inputs rounded to the storage dtype, fp64 reference on the same values, NaN-filled over-allocated
outputs, NaN rows after the inputs, one bound per element from the kernel's rounding points.

Routes and the case that reaches them (test_flash[dt-dh-BT-H-N-pattern])
    key tiles of 64, query blocks of 128 (forward, dQ) and 64 (dK/dV): N = 1, 15, 16, 17, 63, 64,
    65, 127, 128, 129, 192, 193 (three key tiles: two rescales), 197, 257, at (BT, H) = (2, 2).
    XCD block-id remap (attn_tile; compiled in through VLP_ATTN_XCD = 1, the default), grids
    forward / dQ = ceil(N / 128) H BT and dK/dV = ceil(N / 64) H BT:
        (1, 15, 1)   15 / 15       remap off (< 16)
        (1, 16, 1)   16 / 16       active, even
        (1, 24, 1)   24 / 24       active, even
        (1, 17, 1)   17 / 17       uneven, remainder 1
        (1, 23, 1)   23 / 23       uneven, remainder 7
        (3, 3, 129)  18 / 27       uneven, remainders 2 and 3
    Outputs are NaN-poisoned, so a tile computed twice and another never leaves NaN behind.
    Score patterns: "mod" moderate spread; "last" the maximum in the last (partial) key tile;
    "under" the maximum in the first tile and every key from 64 on more than 2^126 below it (its
    weight underflows to 0; the reference weight is below 2^-126 of the row's largest and the
    bound allows losing it entirely); "big" |logit| around 80 with both signs, no overflow.

Bounds.  sl2 = fp32(scale * log2 e) is a hyper-parameter: the reference uses the same fp32 value.
    raw score: e_raw = dh u sum_d |q k|; exponent x = fma(raw, sl2, -max): e_x = sl2 e_raw + u |x|
    weight 2^x by the hardware exp2, taken as 1 ulp (SUPPOSED: neither guide gives v_exp_f32's
    accuracy): rel_j = ln2 e_x + 2 u + r_T (the bf16 rounding of the MFMA operand P); the row sum
    comes out of the same MFMA with a ones operand, so numerator and denominator see the same
    rounded weights and the running-max rescale alpha multiplies both:
        e_out = sum_j P_j (rel_j + sum_k P_k rel_k) |v_j| + 2 (65 nt) u sum_j P_j |v_j| + 2 u |out|
                (nt key tiles: 64 additions and one rescale product each, for O and for l)
        e_lse = (sum_k P_k rel_k + 65 nt u) / ln2 + 2 u |lse - max| + u |lse|   (log2f 1 ulp, SUPPOSED)
    Backward (out and lse are given inputs; the reference uses the same values):
        delta = sum_d dO out: e_delta = dh u sum|dO out|
        P = 2^(fma(raw, sl2, -lse)): rel_P = ln2 (sl2 e_raw + u |x|) + 2 u
        dP = -delta + sum_d dO V: e_dp = e_delta + (dh + 1) u (|delta| + sum|dO V|)
        dS = P dP: e_dS = P (rel_P |dP| + e_dp) + (u + r_T) |dS|
        dq = scale sum_j dS K: scale (sum e_dS |K| + 64 nt u sum|dS K|) + u |dq|; dk likewise
        dv = sum_i P dO: sum (rel_P + r_T) P |dO| + 64 nt u sum P |dO|;  then the store.
    N = 1: out = v exactly, so the true dq and dk are 0 (the fp64 reference keeps only its own
    2^-52-level rounding, asserted) and the bound is what the two dot products dO.V and delta
    leave (the existing exact-zero argument of test_gpu_vit_ops.py).

Elementwise kernels behind ew() (grid capped at 16384 workgroups of 256): each runs once with
work items just past 16384 * 256 = 4 194 304 and a partial last workgroup, so the grid-stride
loop iterates; results are exact (copies, permutations, one fp32 operation rounded once):
    blockify / inverse   strides by 16-byte chunk: 2054 x 2046 pixels x 8 bf16 = 4 202 484 chunks
    pos_grad             by element: TN * C = 524 413 * 8
    maxpool fwd          by output element: 1449 x 1449 x 8 -> 725 x 725 x 8 = 4 205 000
    maxpool bwd          by input element: 725 x 725 x 8
    patch_prep           by element: 294 x 298 patches x 48 = 4 205 376
    add_bias / rowscale  by element: 174 800 x 24
    permute_cols / bcast by element: 43 702 x 96

`test_cpu_replay_flash` (no gpu marker) replays the arithmetic in fp32 torch (operands rounded to
the storage dtype where the kernel feeds an MFMA) at every attention shape against the same bounds.
Worst |err| / bound per tensor, CPU replay | MI355X:
    out 0.348 | 0.348    lse 0.291 | 0.295    dq 0.860 | 0.860    dk 0.980 | 0.980    dv 0.835 | 0.835
    maxpool bwd dx  - | 0.996   (bf16 figures approach 1 by construction: the half ulp of the store)
The whole file runs in 4.4 s on an MI355X (92 tests, the slowest 0.5 s).

Mutations tried on a scratch copy of csrc/nest_ops.hip, each caught by the named case:
    remap using q for every XCD                         test_flash[bf16-dh32-remap-BT1H17-N1]
    last partial key tile not masked (forward)          test_flash[bf16-dh32-BT2H2-N65-last]
    lse written in natural log                          test_flash[bf16-dh32-BT2H2-N16-mod]
    add_bias: ew() cap without the stride loop          test_ew_add_bias_and_rowscale
    forward: lsum not rescaled by alpha                 test_flash[bf16-dh32-BT2H2-N65-last]
    forward: o not rescaled by alpha                    test_flash[bf16-dh32-BT2H2-N65-last]
xcd < rr -> xcd <= rr is no mutation: at xcd == rr both branches give rr (q + 1) + idx.  Nor is
"the rescale skipped when the maximum does not move": alpha = exp2(mi - mn) is exactly 1 then,
so skipping the two products changes no bit; the two mutations above drop a rescale for good
(each also fails N128-big, N129-last, N193-last and remap-BT3H3-N129, in both dtypes).
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.routes_fp64 import BF16, F32, F64, U, check_into, dtid, gpu_ops, nan_out, nan_tail, r_t, rnd, store_bound, take

gpu = pytest.mark.gpu
WORST = {}          # worst |err| / bound per tensor family, this file's cases only
check = functools.partial(check_into, WORST)


@pytest.fixture(scope="module")
def ops():
    return gpu_ops()


LN2 = math.log(2.0)

N_PATTERN = [(1, "mod"), (15, "big"), (16, "mod"), (17, "last"), (63, "big"), (64, "mod"), (65, "last"),
             (127, "under"), (128, "big"), (129, "last"), (192, "under"), (193, "last"), (197, "under"),
             (257, "under")]
REMAP = [(1, 15, 1), (1, 16, 1), (1, 24, 1), (1, 17, 1), (1, 23, 1), (3, 3, 129)]


def flash_cases():
    cases = []
    for dt in (BF16, F32):
        for dh in (32, 64):
            for N, pat in N_PATTERN:
                cases.append(pytest.param(dt, dh, 2, 2, N, pat, id=f"{dtid(dt)}-dh{dh}-BT2H2-N{N}-{pat}"))
            for BT, H, N in REMAP:
                cases.append(pytest.param(dt, dh, BT, H, N, "mod", id=f"{dtid(dt)}-dh{dh}-remap-BT{BT}H{H}-N{N}"))
    return cases


FLASH_CASES = flash_cases()


def flash_inputs(dt, dh, BT, H, N, pat, seed):
    g = torch.Generator().manual_seed(seed)
    C = H * dh
    scale = float(torch.tensor(dh ** -0.5, dtype=F32))
    qkv = torch.randn(BT * N, 3, H, dh, generator=g, dtype=F64)
    if pat == "last":
        qkv[:, 0, :, 0] = 2.0
        qkv.view(BT, N, 3, H, dh)[:, N - 1, 1, :, 0] = 12.0
    elif pat in ("under", "big"):
        a = math.sqrt((50.0 if pat == "under" else 80.0) / scale)
        qkv[:, 0:2] *= 0.5
        qkv[:, 0, :, 0] = a
        k0 = qkv.view(BT, N, 3, H, dh)[:, :, 1, :, 0]
        if pat == "under":
            k0[:] = a
            k0[:, 64:] = -a
        else:
            k0[:] = a * (1 - 2 * torch.randint(0, 2, k0.shape, generator=g).double())
    inp = dict(dt=dt, dh=dh, BT=BT, H=H, N=N, scale=scale)
    inp["sl2"] = float(np.float32(scale) * np.float32(1.4426950408889634))
    inp["qkv"] = qkv.view(BT * N, 3 * C).to(dt)
    inp["dout"] = rnd((BT * N, C), g, dt)
    return inp


def hsplit(t, BT, N, H, dh):
    return t.view(BT, N, H, dh).permute(0, 2, 1, 3)           # [BT][H][N][dh]


def hjoin(t, BT, N, H, dh):
    return t.permute(0, 2, 1, 3).reshape(BT * N, H * dh)


def flash_ref(inp):
    dt, dh, BT, H, N, sc, sl2 = (inp[k] for k in ("dt", "dh", "BT", "H", "N", "scale", "sl2"))
    C, rT, nt = H * dh, r_t(dt), -(-N // 64)
    qkv = inp["qkv"].double()
    q, k, v = (hsplit(qkv[:, i * C:(i + 1) * C], BT, N, H, dh) for i in range(3))
    raw = q @ k.transpose(2, 3)
    e_raw = dh * U * (q.abs() @ k.abs().transpose(2, 3))
    z = raw * sl2
    mx = z.max(3, keepdim=True).values
    x = z - mx
    w = torch.exp2(x)
    l = w.sum(3, keepdim=True)
    P = w / l
    rel = LN2 * (sl2 * e_raw + U * x.abs()) + 2 * U + rT
    rel = torch.where(x < -125.0, torch.ones_like(rel), rel)     # flushed to 0 by the hardware exp2
    rbar = (P * rel).sum(3, keepdim=True)
    out = P @ v
    e_out = (P * (rel + rbar)) @ v.abs() + 2 * 65 * nt * U * (P @ v.abs()) + 2 * U * out.abs()
    lse = mx + torch.log2(l)
    e_lse = (rbar + 65 * nt * U) / LN2 + 2 * U * (lse - mx).abs() + U * lse.abs()
    o2 = hjoin(out, BT, N, H, dh)
    R = {"out": (o2, store_bound(hjoin(e_out, BT, N, H, dh), o2, dt)),
         "lse": (lse.reshape(-1), e_lse.reshape(-1))}
    # backward on the stored out / lse
    inp["out_in"] = o2.to(dt)
    inp["lse_in"] = lse.reshape(-1).to(F32)
    ob = hsplit(inp["out_in"].double(), BT, N, H, dh)
    lb = inp["lse_in"].double().view(BT, H, N, 1)
    dO = hsplit(inp["dout"].double(), BT, N, H, dh)
    delta = (dO * ob).sum(3, keepdim=True)
    e_delta = dh * U * (dO * ob).abs().sum(3, keepdim=True)
    xb = z - lb
    Pb = torch.exp2(xb)
    rel_P = LN2 * (sl2 * e_raw + U * xb.abs()) + 2 * U
    rel_P = torch.where(xb < -125.0, torch.ones_like(rel_P), rel_P)
    dOV = dO @ v.transpose(2, 3)
    dP = dOV - delta
    e_dp = e_delta + (dh + 1) * U * (delta.abs() + dO.abs() @ v.abs().transpose(2, 3))
    dS = Pb * dP
    e_dS = Pb * (rel_P * dP.abs() + e_dp) + (U + rT) * dS.abs()
    acc = 64 * nt * U
    dq = sc * (dS @ k)
    e_dq = sc * (e_dS @ k.abs() + acc * (dS.abs() @ k.abs())) + U * dq.abs()
    dk = sc * (dS.transpose(2, 3) @ q)
    e_dk = sc * (e_dS.transpose(2, 3) @ q.abs() + acc * (dS.abs().transpose(2, 3) @ q.abs())) + U * dk.abs()
    dv = Pb.transpose(2, 3) @ dO
    e_dv = (Pb * (rel_P + rT)).transpose(2, 3) @ dO.abs() + acc * (Pb.transpose(2, 3) @ dO.abs())
    for nme, val, err in (("dq", dq, e_dq), ("dk", dk, e_dk), ("dv", dv, e_dv)):
        v2 = hjoin(val, BT, N, H, dh)
        R[nme] = (v2, store_bound(hjoin(err, BT, N, H, dh), v2, dt))
    return R


def flash_replay(inp):
    dt, dh, BT, H, N, sc, sl2 = (inp[k] for k in ("dt", "dh", "BT", "H", "N", "scale", "sl2"))
    C = H * dh
    qkv = inp["qkv"].float()
    q, k, v = (hsplit(qkv[:, i * C:(i + 1) * C], BT, N, H, dh) for i in range(3))
    sl2f, scf = torch.tensor(sl2, dtype=F32), torch.tensor(sc, dtype=F32)
    raw = q @ k.transpose(2, 3)
    mx = (raw * sl2f).max(3, keepdim=True).values
    w = torch.exp2(raw * sl2f - mx).to(dt).float()
    l = w.sum(3, keepdim=True)
    out = {"out": hjoin((w @ v) * (1.0 / l), BT, N, H, dh).to(dt), "lse": (mx + torch.log2(l)).reshape(-1)}
    ob = hsplit(inp["out_in"].float(), BT, N, H, dh)
    dO = hsplit(inp["dout"].float(), BT, N, H, dh)
    delta = (dO * ob).sum(3, keepdim=True)
    P = torch.exp2(raw * sl2f - inp["lse_in"].view(BT, H, N, 1))
    dS = (P * (dO @ v.transpose(2, 3) - delta)).to(dt).float()
    out["dq"] = hjoin((dS @ k) * scf, BT, N, H, dh).to(dt)
    out["dk"] = hjoin((dS.transpose(2, 3) @ q) * scf, BT, N, H, dh).to(dt)
    out["dv"] = hjoin(P.to(dt).float().transpose(2, 3) @ dO, BT, N, H, dh).to(dt)
    return out


def flash_device(ops, inp, raw=False):
    dev, dt, dh, BT, H, N = "cuda", inp["dt"], inp["dh"], inp["BT"], inp["H"], inp["N"]
    C, R = H * dh, BT * N
    fwd, bwd = (ops.nest_attn_fwd, ops.nest_attn_bwd) if dh == 32 else (ops.vit_attn_fwd, ops.vit_attn_bwd)
    qkv, dout = nan_tail(inp["qkv"], dev), nan_tail(inp["dout"], dev)
    out = nan_out(R, C, dt, dev)
    lse = torch.full((BT * H * N + 64,), float("nan"), dtype=F32, device=dev)
    fwd(qkv, out, lse, BT, H, N, inp["scale"])
    dqkv = nan_out(R, 3 * C, dt, dev)
    delta = torch.full((BT * H * N + 64,), float("nan"), dtype=F32, device=dev)
    bwd(qkv, nan_tail(inp["out_in"], dev), dout, inp["lse_in"].to(dev), delta, dqkv, BT, H, N, inp["scale"])
    torch.cuda.synchronize()
    if raw:
        return out.cpu(), lse.cpu(), dqkv.cpu()
    d = take("dqkv", dqkv, R)
    assert bool(torch.isnan(delta[BT * H * N:]).all().item()), "delta: elements beyond the scratch written"
    return {"out": take("out", out, R), "lse": take("lse", lse, BT * H * N),
            "dq": d[:, :C], "dk": d[:, C:2 * C], "dv": d[:, 2 * C:]}


def flash_check(tag, R, out, side):
    for k in ("out", "lse", "dq", "dk", "dv"):
        check(f"{tag} {k}", f"{side} flash {k}", out[k], *R[k])


def seed_of(dh, BT, H, N):
    return 7 * N + dh + 13 * H + BT


@gpu
@pytest.mark.parametrize("dt,dh,BT,H,N,pat", FLASH_CASES)
def test_flash(ops, dt, dh, BT, H, N, pat):
    inp = flash_inputs(dt, dh, BT, H, N, pat, seed_of(dh, BT, H, N))
    R = flash_ref(inp)
    flash_check(f"flash {dtid(dt)} dh{dh} BT{BT} H{H} N{N} {pat}", R, flash_device(ops, inp), "dev")
    if N == 1:
        # the exact-zero argument: out = v, so the true dq and dk are 0; the fp64 reference itself
        # keeps only its own two dh-term dot products' rounding, 2 dh 2^-52 sum|dO v| |k or q| scale
        C = H * dh
        v, do = inp["qkv"][:, 2 * C:].double(), inp["dout"].double()
        lim = 2 * dh * 2.0 ** -52 * float((do.abs() * v.abs()).view(-1, H, dh).sum(2).max()) * \
            float(inp["qkv"][:, :2 * C].double().abs().max()) * inp["scale"]
        assert float(R["dq"][0].abs().max()) <= lim and float(R["dk"][0].abs().max()) <= lim


def test_cpu_replay_flash():
    for c in FLASH_CASES:
        dt, dh, BT, H, N, pat = c.values
        inp = flash_inputs(dt, dh, BT, H, N, pat, seed_of(dh, BT, H, N))
        flash_check(f"replay flash {c.id}", flash_ref(inp), flash_replay(inp), "cpu")


@gpu
@pytest.mark.parametrize("dh", [32, 64])
def test_flash_run_to_run_bits(ops, dh):
    inp = flash_inputs(BF16, dh, 3, 3, 129, "mod", 5)
    flash_ref(inp)
    a, b = flash_device(ops, inp, raw=True), flash_device(ops, inp, raw=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16 if x.dtype == BF16 else torch.int32),
                           y.view(torch.int16 if y.dtype == BF16 else torch.int32))


@gpu
def test_flash_refusals(ops):
    from vlp_amd._lib import HipError, lib, ptr
    L = lib()
    a = ptr(torch.zeros(4096, dtype=F32, device="cuda"))
    for fwd, bwd, dh in ((L.vlp_nest_attn_fwd, L.vlp_nest_attn_bwd, 32), (L.vlp_vit_attn_fwd, L.vlp_vit_attn_bwd, 64)):
        for k in range(3):
            args = [a] * 3
            args[k] = None
            with pytest.raises(HipError, match="hipError 1$"):
                fwd(0, 1, 1, 1, dh, args[0], args[1], args[2], 0.1, 0)
        for k in range(6):
            args = [a] * 6
            args[k] = None
            with pytest.raises(HipError, match="hipError 1$"):
                bwd(0, 1, 1, 1, dh, args[0], args[1], args[2], args[3], args[4], args[5], 0.1, 0)


# ================================================================ ew()-capped elementwise kernels
CAP = 16384 * 256


def guard1(n, dt, dev, fill=float("nan")):
    return torch.full((n + 256,), fill, dtype=dt, device=dev)


def guard_ok(buf, n, fill=None):
    tail = buf[n:]
    return bool((torch.isnan(tail) if fill is None else tail == fill).all().item())


def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


@gpu
def test_ew_blockify_and_inverse(ops):
    dev, B, Hg, Wg, bs, C = "cuda", 1, 1027, 1023, 2, 8
    npix = B * Hg * bs * Wg * bs
    assert npix * C // 8 > CAP and (npix * C // 8) % 256
    g = gen(dev, 1)
    x = torch.randn(npix * C, generator=g, device=dev).to(BF16)
    pos = torch.randn(Hg * Wg * bs * bs * C, generator=g, device=dev)
    y = guard1(npix * C, BF16, dev)
    ops.nest_blockify(x, y, B, Hg, Wg, bs, C, pos=pos)
    tok = x.view(B, Hg, bs, Wg, bs, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hg * Wg, bs * bs, C)
    ref = (tok.float() + pos.view(1, Hg * Wg, bs * bs, C)).to(BF16).reshape(-1)
    assert guard_ok(y, npix * C) and torch.equal(bits(y[:npix * C]), bits(ref)), "blockify + pos"
    back = guard1(npix * C, BF16, dev)
    ops.nest_blockify(ref, back, B, Hg, Wg, bs, C, inverse=True)
    inv = ref.view(B, Hg, Wg, bs, bs, C).permute(0, 1, 3, 2, 4, 5).reshape(-1)
    assert guard_ok(back, npix * C) and torch.equal(bits(back[:npix * C]), bits(inv)), "deblockify"


@gpu
def test_ew_pos_grad(ops):
    dev, B, TN, C = "cuda", 2, 524413, 8
    assert TN * C > CAP and (TN * C) % 256
    dy = torch.randn(B, TN * C, generator=gen(dev, 2), device=dev).to(BF16)
    dpos = guard1(TN * C, F32, dev)
    ops.nest_pos_grad(dy, dpos, B, TN, C)
    ref = dy[0].float() + dy[1].float()          # 0 + a is exact, then one fp32 addition
    assert guard_ok(dpos, TN * C) and torch.equal(dpos[:TN * C], ref)


def first_max_tap(x_nhwc):
    """values and first-maximum tap (row-major over the 3 x 3 / 2, pad 1 window) of x[1][H][W][C]"""
    _, H, W, C = x_nhwc.shape
    xp = F.pad(x_nhwc.float().permute(0, 3, 1, 2), (1, 1, 1, 1), value=-float("inf"))
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    best = torch.full((C, Ho, Wo), -float("inf"), device=x_nhwc.device)
    tap = torch.zeros((C, Ho, Wo), dtype=torch.uint8, device=x_nhwc.device)
    for kh in range(3):
        for kw in range(3):
            v = xp[0, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2][:, :Ho, :Wo]
            better = v > best
            best = torch.where(better, v, best)
            tap = torch.where(better, torch.full_like(tap, kh * 3 + kw), tap)
    return best.permute(1, 2, 0).contiguous(), tap.permute(1, 2, 0).contiguous()


@gpu
def test_ew_maxpool_fwd(ops):
    dev, H, W, C = "cuda", 1449, 1449, 8
    Ho = Wo = 725
    n = Ho * Wo * C
    assert n > CAP and n % 256
    x = torch.randn(1, H, W, C, generator=gen(dev, 3), device=dev).to(BF16)
    y = guard1(n, BF16, dev)
    idx = guard1(n, torch.uint8, dev, fill=255)
    ops.nest_maxpool_fwd(x, y, idx)
    best, tap = first_max_tap(x)
    assert guard_ok(y, n) and guard_ok(idx, n, 255)
    assert torch.equal(y[:n].float(), best.reshape(-1)) and torch.equal(idx[:n], tap.reshape(-1))


@gpu
def test_ew_maxpool_bwd(ops):
    """dx = the sum of at most four bf16 gradients in fp32 (exact to 3 u of their magnitudes),
    rounded once to bf16"""
    dev, H, W, C = "cuda", 725, 725, 8
    Ho = Wo = 363
    n = H * W * C
    assert n > CAP and n % 256
    g = gen(dev, 4)
    x = torch.randn(1, H, W, C, generator=g, device=dev).to(BF16)
    _, tap = first_max_tap(x)
    dy = torch.randn(1, Ho, Wo, C, generator=g, device=dev).to(BF16)
    dx = guard1(n, BF16, dev)
    ops.nest_maxpool_bwd(dy, tap.view(1, Ho, Wo, C), dx[:n].view(1, H, W, C))
    ho = torch.arange(Ho, device=dev).view(Ho, 1, 1)
    wo = torch.arange(Wo, device=dev).view(1, Wo, 1)
    t = tap.long()
    hi, wi = 2 * ho - 1 + t // 3, 2 * wo - 1 + t % 3
    flat = ((hi * W + wi) * C + torch.arange(C, device=dev).view(1, 1, C)).reshape(-1)
    ref = torch.zeros(n, dtype=F64, device=dev).index_add_(0, flat, dy.double().reshape(-1))
    mag = torch.zeros(n, dtype=F64, device=dev).index_add_(0, flat, dy.double().abs().reshape(-1))
    assert guard_ok(dx, n)
    check("maxpool bwd dx", "dev ew maxpool_bwd", dx[:n].cpu(), ref.cpu(), store_bound(3 * U * mag, ref, BF16).cpu())


@gpu
def test_ew_patch_prep(ops):
    dev, B, Hi, Wi, bs = "cuda", 1, 1176, 1192, 2
    Hp, Wp = Hi // 4, Wi // 4
    n = B * Hp * Wp * 48
    assert n > CAP and n % 256
    x = torch.randn(B, 3, Hi, Wi, generator=gen(dev, 5), device=dev)
    out = guard1(n, BF16, dev)
    ops.nest_patch_prep(out, B, Hi, Wi, bs, x=x)
    p = x.view(B, 3, Hp, 4, Wp, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, Hp // bs, bs, Wp // bs, bs, 48)
    ref = p.permute(0, 1, 3, 2, 4, 5).reshape(-1).to(BF16)
    assert guard_ok(out, n) and torch.equal(bits(out[:n]), bits(ref))


@gpu
def test_ew_add_bias_and_rowscale(ops):
    dev, M, N, rows = "cuda", 174800, 24, 1000
    n = M * N
    assert n > CAP and n % 256
    g = gen(dev, 6)
    y0 = torch.randn(n, generator=g, device=dev).to(BF16)
    bias = torch.randn(N, generator=g, device=dev)
    y = guard1(n, BF16, dev)
    y[:n] = y0
    ops.nest_add_bias(y, bias, M, N)
    ref = (y0.float().view(M, N) + bias).to(BF16).reshape(-1)
    assert guard_ok(y, n) and torch.equal(bits(y[:n]), bits(ref)), "add_bias"
    # DropPath scales 0 and 2 = 1 / (1 - 0.5): k * y is exact, so x + k y rounds once with or
    # without a fused multiply-add
    s = (torch.arange(-(-M // rows), device=dev) % 3 != 1).float() * 2.0
    x = guard1(n, BF16, dev)
    x0 = torch.randn(n, generator=g, device=dev).to(BF16)
    x[:n] = x0
    ops.nest_rowscale(x, y0, s, M, N, rows, 0)
    k = s[torch.arange(M, device=dev) // rows].view(M, 1)
    ref = (x0.float().view(M, N) + k * y0.float().view(M, N)).to(BF16).reshape(-1)
    assert guard_ok(x, n) and torch.equal(bits(x[:n]), bits(ref)), "rowscale mode 0"
    yb = guard1(n, BF16, dev)
    ops.nest_rowscale(x0, yb, s, M, N, rows, 1)
    ref = (k * x0.float().view(M, N)).to(BF16).reshape(-1)
    assert guard_ok(yb, n) and torch.equal(bits(yb[:n]), bits(ref)), "rowscale mode 1"


@gpu
def test_ew_permute_cols_and_bcast(ops):
    dev, Nr, H, Dh = "cuda", 43702, 3, 32
    C = H * Dh
    n = Nr * C
    assert n > CAP and n % 256
    g = gen(dev, 7)
    src = torch.randn(Nr, C, generator=g, device=dev)
    dst = guard1(n, BF16, dev)
    ops.nest_permute_cols(src, dst, Nr, H, Dh)
    ref = src.view(Nr, Dh, H).permute(0, 2, 1).reshape(-1).to(BF16)      # dst[n][h Dh + d] = src[n][d H + h]
    assert guard_ok(dst, n) and torch.equal(bits(dst[:n]), bits(ref)), "permute_cols"
    B, HW = 2, Nr // 2
    dfeat = torch.randn(B, C, generator=g, device=dev)
    inv = float(torch.tensor(1.0 / HW, dtype=F32))
    dy = guard1(n, BF16, dev)
    ops.nest_bcast(dfeat, dy, B, HW, C, inv)
    ref = (dfeat * torch.tensor(inv, device=dev)).to(BF16).view(B, 1, C).expand(B, HW, C).reshape(-1)
    assert guard_ok(dy, n) and torch.equal(bits(dy[:n]), bits(ref)), "bcast"


def test_zz_worst_ratios_flash():
    for k in sorted(WORST):
        print(f"WORST {k:24s} {WORST[k]:.3f}")
        assert WORST[k] <= 1.0
