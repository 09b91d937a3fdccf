"""Every route of the stem (conv 7x7/2 -> BN -> ReLU -> max-pool 3x3/2) per element against fp64.

Routes.  csrc/stem_ops.hip: stem1_pool_fwd_kernel<NA> (train and eval), stem1_route_bwd_kernel<NA>,
stem1_bwd_gram_kernel<64 | 128> + the part / tot / grad fold, each at NA = Wo / 64 = 1..4 (the Gram
column block is 128 when Wo % 128 == 0, else 64).  csrc/conv_ops.hip: stem_prep / stem_prep_u8, the
3-channel vlp_stem_fwd (gemm_narrow bf16, launch_gemm fp32), vlp_stem_wgrad (atomics),
vlp_stem_wgrad_ws + fold (launch_gemm_bk<64,128> split slabs bf16, atomics into slab 0 fp32), the
single-channel vlp_stem1_fwd (launch_gemm_bk<256,64> bf16, launch_gemm fp32), vlp_stem1_wgrad_ws + fold.
csrc/bn_ops.hip: maxpool_fwd_kernel with sc / sh applied on load.

Reference.  Plain fp64 torch on the CPU on the kernels' own operands: the image is
(u8 - mean) * f32(1 / std) rounded to the storage dtype (stem*_prep_u8_kernel), the single-channel
weights are (w0 + w1) + w2 in fp32, rounded (pack_stem1_kernel), the 3-channel weights are rounded
per channel (pack_stem_kernel).  S is the same expression on absolute values.  gamma, sc, sh, mean,
istd, sum_g and sum_gx carry a factor 1 + c / 64 and alternate in sign, so a channel group mapped
wrongly fails by orders of magnitude; gamma holds exact zeros (counted as >= 0), negatives and
positives.

Rounding points as the kernels have them, u = 2^-24, eps32 = 2 u.
  * conv accumulation: fp32 on MFMA (stem_mfma: two K = 32 steps; the GEMMs likewise), 49 (147)
    non-zero products of a K = 64 (256) layout whose other weights are exact zeros.  The worst case
    gamma_49 <= 64 u (gamma_147 <= 256 u) is affordable: noise = K u S = (K / 2) eps32 S, K = 64 and 256,
    in place of the suite's random-walk C_ACC.
  * fused forward: stem_store rounds the fp32 accumulator to bf16 into the LDS row; pooling compares
    those bf16 values (strict >, row-major tap order, padding taps never compared) and yarg is
    sign * best, exact.  So yarg is bf16(acc) at the chosen tap: 2 (2^-9 |ref| + 32 eps32 S).
    The BN sums are taken from the SAME bf16 row (unpack8 of the tile, `if (stats && rr >= 1)`): the
    reference sums are those of v = bf16(y0_64); an element may deviate by one ulp of v only where
    `staged` finds y0_64 within the noise of a rounding boundary.  Each thread sums in fp32, the 32
    threads of a chunk meet in LDS in fp32, then ONE fp64 atomic per channel and workgroup: T = the
    workgroup's owned conv rows x Wo = 2 kStemBand Wo pixels; + workgroups * 2^-52 * sum |terms|.
  * route backward: y0 recomputed, rounded to bf16 (stem_store), g summed over up to four windows in
    fp32 (`gsum`, not rounded), d = fmaf(k, gsum, fmaf(b, y, c)) rounded once to bf16.  k, b, c are
    formed in fp32 from fp32 / fp64 inputs: k one rounding; mg, mgx two each (1.f / count, the cast);
    b = -k * is * mgx five in all; c = -k * mg + k * is * mgx * mean seven on its absolute terms; the
    inner fmaf one; gsum three.  At most 8 u = 4 eps32 on Sdy = |k| sum |dp| + |b| |y| + |k mg| +
    |k is mgx mean|: C_DY = 4.  The reference is built from v = bf16(y0_64) and one ulp of v times |b|
    is allowed where `staged` finds a possible flip; the share of those elements is printed and must
    be <= 5 %.
  * Gram backward: the routed gradient tile is bf16(fp32 sum of <= 4 windows) (route(): Chunk::pack),
    R = Gt^T P, G = P^T P, S = 1^T P accumulate in fp32 on MFMA over the workgroup's pixels
    (2 kGramBand conv rows x CW columns <= 8192, in two k-parity halves), one fp32 slab per workgroup;
    stem1_gram_part_kernel sums <= ceil(ns / 32) slabs per group in fp32 (two accumulators), then fp64
    (stem1_gram_tot_kernel) and dW1 = k R + b (W1 G) + c S in fp64, cast to fp32.  The depth is the
    pixel count, so C_ACC = 64 as for every weight gradient of the suite: 64 eps32 * (|k| |g| (*) |P| +
    |b| |W1| (|P| (*) |P|) + |c| sum |P|), + |k| (flip of the routed gradient's bf16 rounding) (*) |P|
    where the fp64 window sum lies within 3 u sum |dp| of a rounding boundary.  y0 is not rounded here.
  * unfused forwards: EpiConvFwd rounds once on store, sums from the unrounded fp32 value, T = 256 rows.
    bf16: 2 (2^-9 |ref| + (K / 2) eps32 S); fp32: (K / 2) eps32 S.
  * unfused weight gradients: C_ACC eps32 (|dy| (*) |x|); the depth per fp32 slab is M / splits pixels
    (<= 8192 here), the fold adds <= 4 slabs in fp32.  fp32 accumulates every split into slab 0.
  * max-pool with BN on load: q = max(fmaf(y, sc, sh), 0) in fp32, compared in fp32, rounded on store:
    fp32 eps32 (|y sc| + |sh|), bf16 2 (2^-9 |ref| + eps32 (|y sc| + |sh|)); yarg is y at the tap, exact.

Gate.  Every case asserts the bound per element with zero violations, and the gate of the earlier
norm tests wherever it computes that figure (dy rel-L2 1e-2, Gram gradient rel-L2 2e-3, sums l1 / 512
and 1 / 256, first-maximum agreement > 0.999, tol(dt) for the unfused calls).  The chosen tap is a
non-padding tap; with v = sign(gamma) y0_64 no tap exceeds the chosen one by more than
bound(tap) + bound(chosen).  Exact ties (all-zero and constant images) pin the tap order itself.

Untouched memory.  yarg, idx (byte sentinel 0xEE > 8), dy, y, the statistics replicas, grad and the
workspaces are prefilled with a sentinel and have guard rows behind them.  xs comes from
vlp_stem1_prep_u8 (the fused kernels load the zero-weight kh = 7 row and kw = 7 column and rely on
them being finite); inputs are followed inside their allocation by large FINITE values.

`test_bound_holds_for_emulated_arithmetic` (CPU) replays each family in fp32 and shows every bound
holds, then perturbs the emulated result the way a real defect would; each perturbation violates the
per-element gate.  Worst |err| / bound, emulated on the CPU | measured on an MI355X (maximum over the
file's run):
    fused yarg (bf16)        0.994 | 0.991
    fused BN sums            0.009 | 0.006
    route backward dy (bf16) 0.996 | 0.995
    Gram gradient            0.004 | 0.002
    unfused y bf16           0.988 | 0.988
    unfused y fp32           0.056 | 0.073
    unfused sums             0.002 | 0.002
    weight gradient          0.023 | 0.025
    max-pool out             0.975 | 0.996
(the bf16 element figures approach 1 by construction: 2 * 2^-9 |ref| is exactly the half-ulp at the bottom
of a binade.  The sums and both gradient families sit far below 1 on the CPU and on the device alike: their
bounds are worst-case in the depth T, resp. carry the suite's C_ACC = 64, while random-sign errors grow with
the square root of the depth.  No bf16 family has a device figure far below its CPU figure.)
Staged shares of the route backward: 2.4 % .. 3.3 % of the elements (the fp64 reference alone; <= 5 % asserted).

Sensitivity (CPU, in the emulation test).  The edge column of conv row 16 taken from the band above, and one
window routed one tap to the right, both in the 3 x 132 x 512 case: 60 of 3.2e6 elements violate the gate by
factors above 1e5 while dy's rel-L2 stays at 2.8e-3 and 4.6e-3, inside the earlier 1e-2 gate, which would have
missed both.  The tail slab dropped from the fold at ns = 33 and a partial Gram band reading the row pair above:
2525 and 2880 of 3136 elements violate; their rel-L2 (3.5e-2, 2.5e-2) is beyond the earlier 2e-3 gate, which
would have caught them had any earlier case reached ns > 32 or a partial band; none did.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.routes_fp64 import BF16, EPS32, F32, dtid, emu_sum, staged, sum_bound

gpu = pytest.mark.gpu

MEAN, STD = 127.5, 73.9
C_ACC = 64.0          # weight gradients: random-walk figure at pixel-count depth (<= 8192 per slab here)
C_DY = 4.0            # route backward: 8 u on Sdy (derivation in the module docstring)
K1, K3 = 64, 256      # padded reduction depths; noise = K u S = (K / 2) eps32 S
GUARD = 64            # sentinel rows behind every output
SENT = -1024.0
IDX_SENT = 0xEE
TAIL = 4096           # large finite values behind every input
K_BAND, K_PAIRS, G_BAND, G_GROUPS = 8, 8, 32, 32   # kStemBand, kStemPairs, kGramBand, kGramGroups
G_SLAB = 64 * 64 * 2 + 64
WORST = {}
SHARES = {}


def tol(dt):
    return 2e-5 if dt == F32 else 1.5e-2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlp_amd import ops as o
    return o


# ---------------------------------------------------------------- gate and buffers
def check(name, fam, got, ref, bound, rel_gate=None):
    got = got.double()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    d = (got - ref).abs()
    nviol = int((~(d <= bound)).sum())          # NaN counts as a violation
    worst = float((d / (bound + 1e-300)).max()) if ref.numel() else 0.0
    r = float(torch.linalg.vector_norm(got - ref) / (torch.linalg.vector_norm(ref) + 1e-300))
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    print(f"{name}: rel-L2 {r:.3e}, worst |err|/bound {worst:.3f}, violations {nviol} of {ref.numel()}")
    assert nviol == 0, f"{name}: {nviol} of {ref.numel()} elements beyond the bound (worst ratio {worst:.2f})"
    if rel_gate is not None:
        assert r < rel_gate, f"{name}: rel-L2 {r:.3e} >= {rel_gate:.1e}"
    return r


def with_tail(t, dev):
    """t on dev inside an allocation followed by TAIL large finite elements"""
    fill = 200 if t.dtype == torch.uint8 else 100.0
    buf = torch.full((t.numel() + TAIL,), fill, dtype=t.dtype, device=dev)
    buf[:t.numel()].copy_(t.flatten())
    return buf[:t.numel()].view(t.shape)


def guarded(shape, dt, dev, fill=SENT):
    """A [.., C] output as the first rows of a sentinel-filled [M + GUARD][C] buffer"""
    C = shape[-1]
    M = 1
    for s in shape[:-1]:
        M *= s
    buf = torch.full((M + GUARD, C), fill, dtype=dt, device=dev)
    return buf, buf[:M].view(shape)


def guard_ok(name, buf, M, fill=SENT):
    assert bool((buf[M:] == fill).all()), f"{name}: rows beyond the output written"


def stat_buf(rep, dev):
    s = torch.zeros((rep + 1) * 64, dtype=torch.float64, device=dev)
    s[rep * 64:] = SENT
    return s


def stat_total(name, s, rep):
    assert bool((s[rep * 64:] == SENT).all()), f"{name}: statistics written beyond stat_rep replicas"
    return s[:rep * 64].view(rep, 64).sum(0).cpu()


def chan(g, scale, lo=0.5):
    """[64] per-channel vector: (lo + rand) * scale * (1 + c / 64), alternating in sign"""
    c = torch.arange(64, dtype=torch.float32)
    return (lo + torch.rand(64, generator=g)) * scale * (1 + c / 64) * torch.where(c % 2 == 0, 1.0, -1.0)


def make_gamma(g):
    gamma = chan(g, 1.0)
    gamma[[0, 9, 34]] = 0.0                     # exact zeros on even and odd channels: counted as >= 0
    gamma[[4, 5]] = gamma[[5, 4]].clone()       # two neighbours break the strict alternation
    return gamma


def image_f32(xu):
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(STD, dtype=F32)      # the host's 1.f / std
    return (xu.float() - MEAN) * inv


# ---------------------------------------------------------------- fused stem: reference
FUSED = [  # (N, H, W): NA 1..4, odd and even W, H in {4, 7, 36, 132}, N in {1, 3}
    (1, 4, 128), (3, 7, 127), (3, 36, 128), (1, 132, 127),
    (3, 4, 256), (1, 36, 255), (1, 132, 256),
    (1, 7, 384), (3, 36, 384),
    (1, 4, 511), (3, 36, 511), (1, 7, 512), (3, 132, 512),
]
_REF = {}


def sid(c):
    return "x".join(str(v) for v in c)


def windows(y0):
    """[N, C, Hq, Wq, 9] of y0 over the 3x3/2 pad-1 windows, taps row-major, NaN at padding taps"""
    N, C, Ho, Wo = y0.shape
    pad = F.pad(y0, (1, 1, 1, 1), value=float("nan"))
    return torch.stack([pad[:, :, dh:dh + Ho:2, dw:dw + Wo:2] for dh in range(3) for dw in range(3)], -1)


def first_max(key):
    """first maximum along the last axis (padding = -inf)"""
    eq = key == key.max(-1, keepdim=True).values
    return torch.where(eq, torch.arange(9), torch.tensor(9)).min(-1).values


def fused_ref(case, xu=None, tag=""):
    """Operands and fp64 forward of one fused case, computed once and shared."""
    key = (case, tag)
    if key in _REF:
        return _REF[key]
    N, H, W = case
    g = torch.Generator().manual_seed(1000 * H + W + N)
    if xu is None:
        xu = torch.randint(0, 256, (N, 1, H, W), generator=g, dtype=torch.uint8)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    gamma = make_gamma(g)
    x = image_f32(xu).to(BF16).double()
    w1 = ((w[:, 0] + w[:, 1]) + w[:, 2]).to(BF16).double().unsqueeze(1)
    y0 = F.conv2d(x, w1, stride=2, padding=3)
    S0 = F.conv2d(x.abs(), w1.abs(), stride=2, padding=3)
    Ho, Wo = y0.shape[2:]
    sg = torch.where(gamma < 0, -1.0, 1.0).double().view(1, 64, 1, 1)
    noise = (K1 / 2) * EPS32 * S0
    v, flip = staged(y0, noise)
    idx_ref = first_max(torch.nan_to_num(windows(v * sg), nan=-float("inf")))      # [N, C, Hq, Wq]
    R = dict(N=N, H=H, W=W, Ho=Ho, Wo=Wo, Hq=Ho // 2, Wq=Wo // 2, M=N * Ho * Wo, xu=xu, w=w, gamma=gamma, x=x,
             w1=w1, y0=y0, S0=S0, sg=sg, noise=noise, v=v, flip=flip, idx_ref=idx_ref)
    _REF[key] = R
    return R


def bwd_inputs(R):
    """Pooled gradient (bf16, a third of it zero), taps (the reference's first maxima) and BN vectors."""
    if "dp" in R:
        return R
    g = torch.Generator().manual_seed(77 + R["H"] + R["W"])
    N, Hq, Wq = R["N"], R["Hq"], R["Wq"]
    dp = torch.randn(N, Hq, Wq, 64, generator=g)
    dp = torch.where(torch.rand(N, Hq, Wq, 64, generator=g) < 0.33, torch.zeros(()), dp).to(BF16)
    idx = R["idx_ref"].permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    istd, mean = chan(g, 1.0), chan(g, 0.3)
    sc, sh = R["gamma"] * istd, chan(g, 0.2)
    sum_g, sum_gx = chan(g, 0.3).double() * R["M"], chan(g, 0.3).double() * R["M"]
    R.update(dp=dp, idx=idx, istd=istd, mean=mean, sc=sc, sh=sh, sum_g=sum_g, sum_gx=sum_gx)
    # routed gradient g[n, c, h, w] = sum of dp over the windows whose tap is (h, w), and sum |dp|
    t = idx.permute(0, 3, 1, 2).long()
    n, c, i, j = torch.meshgrid(torch.arange(N), torch.arange(64), torch.arange(Hq), torch.arange(Wq), indexing="ij")
    pos = (n.reshape(-1), c.reshape(-1), (2 * i + t // 3).reshape(-1), (2 * j + t % 3).reshape(-1))
    dpp = dp.permute(0, 3, 1, 2).double().reshape(-1)
    gr = torch.zeros(N, 64, R["Ho"] + 2, R["Wo"] + 2, dtype=torch.float64)
    ga = torch.zeros_like(gr)
    gr.index_put_(pos, dpp, accumulate=True)
    ga.index_put_(pos, dpp.abs(), accumulate=True)
    assert float(ga[:, :, 0].sum() + ga[:, :, -1].sum() + ga[:, :, :, 0].sum() + ga[:, :, :, -1].sum()) == 0.0
    R["g"], R["gabs"] = gr[:, :, 1:-1, 1:-1].contiguous(), ga[:, :, 1:-1, 1:-1].contiguous()
    v4 = lambda t_: t_.double().view(1, 64, 1, 1)              # noqa: E731
    k = v4(R["gamma"]) * v4(istd)
    mg, mgx = v4(sum_g / R["M"]), v4(sum_gx / R["M"])
    R["k"], R["b"], R["c"] = k, -k * v4(istd) * mgx, -k * mg + k * v4(istd) * mgx * v4(mean)
    R["cabs"] = (k * mg).abs() + (k * v4(istd) * mgx * v4(mean)).abs()
    return R


# ---------------------------------------------------------------- fused stem: gates
def gate_fwd(name, R, yarg, idx, s, ss, nwg):
    """yarg / idx [N, Hq, Wq, 64] (CPU), s / ss [64] fp64 totals or None (eval mode)."""
    y0, S0, sg = R["y0"], R["S0"], R["sg"]
    t = idx.permute(0, 3, 1, 2).long()
    assert int(t.max()) <= 8, f"{name}: tap {int(t.max())}"
    win, wS = windows(y0), windows(S0)
    chosen = torch.gather(win, -1, t.unsqueeze(-1)).squeeze(-1)
    assert not bool(torch.isnan(chosen).any()), f"{name}: a padding tap was chosen"
    bnd = 2.0 * (2.0 ** -9 * win.abs() + (K1 / 2) * EPS32 * wS)                  # per tap
    bc = torch.gather(bnd, -1, t.unsqueeze(-1)).squeeze(-1)
    check(name + " yarg", "fused yarg", yarg.permute(0, 3, 1, 2), chosen, bc)
    # no valid tap exceeds the chosen one by more than both bounds (covers the maximum and the earlier taps)
    sg5 = sg.unsqueeze(-1)
    over = torch.nan_to_num(win * sg5 - (chosen * sg).unsqueeze(-1) - bnd - bc.unsqueeze(-1), nan=-1.0)
    nover = int((over > 0).sum())
    print(f"{name} tap: {nover} windows hold a tap beyond the chosen one + both bounds")
    assert nover == 0
    first = R["idx_ref"]
    agree = float((first == t).double().mean())
    print(f"{name} tap: first-maximum agreement {agree:.5f}")
    assert agree > 0.999, agree
    if s is None:
        return
    v, flip = R["v"], R["flip"]
    T = 2 * K_BAND * R["Wo"]
    l1 = v.abs().sum((0, 2, 3))
    ref1, ref2 = v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))
    b1 = sum_bound(flip, v, T, (0, 2, 3)) + nwg * 2.0 ** -52 * l1
    b2 = sum_bound((2 * v.abs() + flip) * flip, v * v, T, (0, 2, 3)) + nwg * 2.0 ** -52 * ref2
    check(name + " sum", "fused BN sums", s, ref1, b1)
    check(name + " sumsq", "fused BN sums", ss, ref2, b2)
    assert bool(((s - y0.sum((0, 2, 3))).abs() <= y0.abs().sum((0, 2, 3)) / 512).all())       # the earlier gates
    assert torch.allclose(ss, (y0 * y0).sum((0, 2, 3)), rtol=1 / 256)


def gate_dy(name, R, dy):
    """dy [N, Ho, Wo, 64] (CPU) against k g + b bf16(y0_64) + c."""
    v, flip = R["v"], R["flip"]
    ref = R["k"] * R["g"] + R["b"] * v + R["c"]
    Sdy = R["k"].abs() * R["gabs"] + R["b"].abs() * v.abs() + R["cabs"]
    bound = 2.0 * (2.0 ** -9 * ref.abs() + C_DY * EPS32 * Sdy) + R["b"].abs() * flip
    share = float((flip > 0).double().mean())
    SHARES[name] = share
    print(f"{name}: staged share {100 * share:.2f} % of {ref.numel()} elements")
    assert share <= 0.05, f"{name}: staged share {share:.3f}"
    return check(name, "route backward dy", dy.permute(0, 3, 1, 2), ref, bound, rel_gate=1e-2)


def gram_ref(R):
    """fp64 dW1 [64][49] = k R + b W1 G + c S (y0 unrounded) and its bound."""
    if "gw_ref" in R:
        return R["gw_ref"], R["gw_bound"]
    N, Ho, Wo = R["N"], R["Ho"], R["Wo"]
    P = F.unfold(R["x"], 7, padding=3, stride=2).transpose(1, 2).reshape(-1, 49)        # [N Ho Wo][49]
    g64 = R["g"].permute(0, 2, 3, 1).reshape(-1, 64)
    gab = R["gabs"].permute(0, 2, 3, 1).reshape(-1, 64)
    gb, gflip = staged(g64, 3 * 2.0 ** -24 * gab)            # bf16 of the fp32 window sum
    Pa = P.abs()
    w1 = R["w1"].reshape(64, 49)
    k, b, c = (R[n_].reshape(64, 1) for n_ in ("k", "b", "c"))
    Rm, G, Sv = gb.t() @ P, P.t() @ P, P.sum(0, keepdim=True)
    ref = k * Rm + b * (w1 @ G) + c * Sv
    Sabs = k.abs() * (gb.abs().t() @ Pa) + b.abs() * (w1.abs() @ (Pa.t() @ Pa)) + R["cabs"].reshape(64, 1) * Pa.sum(0, keepdim=True)
    bound = C_ACC * EPS32 * Sabs + k.abs() * (gflip.t() @ Pa)
    R["P"], R["gb"] = P, gb
    R["gw_ref"], R["gw_bound"] = ref, bound
    return ref, bound


def gate_gram(name, R, grad):
    """grad [64, 3, 7, 7] (CPU fp32)."""
    ref, bound = gram_ref(R)
    assert bool(torch.isfinite(grad).all()), f"{name}: non-finite gradient"
    assert torch.equal(grad[:, 0], grad[:, 1]) and torch.equal(grad[:, 0], grad[:, 2]), f"{name}: channel copies differ"
    return check(name, "Gram gradient", grad[:, 0].reshape(64, 49), ref, bound, rel_gate=2e-3)


def gram_wgs(N, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    cw = 128 if Wo % 128 == 0 else 64
    return N * ((Ho // 2 + G_BAND - 1) // G_BAND) * (Wo // cw), cw


# ---------------------------------------------------------------- fused stem: device runs
def dev_operands(ops, R):
    """xs from vlp_stem1_prep_u8 (every element written) and wp1 from vlp_pack_stem1, both tailed."""
    if "xs" in R:
        return R["xs"], R["wp1"]
    N, H, W = R["N"], R["H"], R["W"]
    assert ops.stem1_fused_ok(H, W)
    Ho, Wo, Hp, Wp1 = ops.stem1_geom(H, W)
    assert (Ho, Wo) == (R["Ho"], R["Wo"])
    xs = with_tail(torch.zeros(4, N, Hp, Wp1, dtype=BF16), "cuda")
    xs.fill_(float("nan"))
    ops.stem1_prep_u8(with_tail(R["xu"], "cuda"), xs, MEAN, STD)
    wp1 = with_tail(torch.zeros(64, 64, dtype=BF16), "cuda")
    ops.pack_stem1(with_tail(R["w"], "cuda"), wp1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xs.float()).all())
    w1p = torch.zeros(64, 8, 8, dtype=torch.float64)
    w1p[:, :7, :7] = R["w1"].reshape(64, 7, 7)
    assert torch.equal(wp1.cpu().double().view(64, 8, 8), w1p), "vlp_pack_stem1 differs from (w0 + w1) + w2 rounded"
    R["xs"], R["wp1"] = xs, wp1
    return xs, wp1


def run_fwd(ops, R, training, rep):
    xs, wp1 = dev_operands(ops, R)
    N, Hq, Wq = R["N"], R["Hq"], R["Wq"]
    ybuf, yarg = guarded((N, Hq, Wq, 64), BF16, "cuda")
    ibuf, idx = guarded((N, Hq, Wq, 64), torch.uint8, "cuda", IDX_SENT)
    s, ss = stat_buf(rep, "cuda"), stat_buf(rep, "cuda")
    ops.stem1_pool_fwd(xs, wp1, with_tail(R["gamma"], "cuda"), yarg, idx, N, R["H"], R["W"],
                       s if training else None, ss if training else None, rep)
    torch.cuda.synchronize()
    name = f"fused fwd {sid((N, R['H'], R['W']))} {'train' if training else 'eval'}"
    guard_ok(name + " yarg", ybuf, N * Hq * Wq)
    guard_ok(name + " idx", ibuf, N * Hq * Wq, IDX_SENT)
    if training:
        return name, yarg.float().cpu(), idx.cpu(), stat_total(name, s, rep), stat_total(name, ss, rep)
    assert bool((s[:rep * 64] == 0).all()) and bool((ss[:rep * 64] == 0).all()), "eval mode wrote statistics"
    return name, yarg.float().cpu(), idx.cpu(), None, None


@gpu
@pytest.mark.parametrize("case", FUSED, ids=sid)
def test_fused_forward_train_and_eval(ops, case):
    R = fused_ref(case)
    nwg = R["N"] * ((R["Hq"] + K_BAND - 1) // K_BAND)
    name, ya, ia, s, ss = run_fwd(ops, R, True, 4 if FUSED.index(case) % 2 == 0 else 1)
    gate_fwd(name, R, ya, ia, s, ss, nwg)
    name, yb, ib, _, _ = run_fwd(ops, R, False, 1)
    assert torch.equal(ya, yb) and torch.equal(ia, ib), "eval-mode pooling differs from train mode"


def bwd_dev(R):
    return [with_tail(R[n_], "cuda") for n_ in ("dp", "idx", "sc", "sh", "mean", "istd", "gamma", "sum_g", "sum_gx")]


@gpu
@pytest.mark.parametrize("case", FUSED, ids=sid)
def test_fused_route_backward(ops, case):
    R = bwd_inputs(fused_ref(case))
    xs, wp1 = dev_operands(ops, R)
    N, Ho, Wo = R["N"], R["Ho"], R["Wo"]
    dbuf, dy = guarded((N, Ho, Wo, 64), BF16, "cuda")
    ops.stem1_route_bwd(xs, wp1, *bwd_dev(R), dy, N, R["H"], R["W"])
    torch.cuda.synchronize()
    name = f"route bwd {sid(case)}"
    guard_ok(name, dbuf, N * Ho * Wo)
    gate_dy(name, R, dy.float().cpu())


def run_gram(R, xs, wp1, short=0):
    """vlp_stem1_bwd_fused on a workspace of exactly the required length (minus `short`) + NaN tail."""
    from vlp_amd._lib import lib
    N, H, W = R["N"], R["H"], R["W"]
    n = ctypes.c_longlong(0)
    lib().vlp_stem1_bwd_fused_ws_floats(N, H, W, ctypes.byref(n))
    nwg, _ = gram_wgs(N, H, W)
    assert n.value == (nwg + G_GROUPS + 2) * G_SLAB
    ws = torch.full((n.value + 1024,), float("nan"), device="cuda")
    grad = torch.full((64 + 8, 3, 7, 7), float("nan"), device="cuda")
    grad[64:] = SENT
    dp, idx, _, _, mean, istd, gamma, sum_g, sum_gx = bwd_dev(R)
    args = [t.data_ptr() for t in (xs, wp1, dp, idx, mean, istd, gamma, sum_g, sum_gx)]
    st = torch.cuda.current_stream().cuda_stream
    lib().vlp_stem1_bwd_fused(*args, ws.data_ptr(), n.value - short, grad.data_ptr(), N, H, W, st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n.value:]).all()), "writes past the workspace"
    assert bool((grad[64:] == SENT).all()), "rows beyond the gradient written"
    return grad[:64].cpu()


@gpu
@pytest.mark.parametrize("case", FUSED, ids=sid)
def test_fused_gram_backward(ops, case):
    R = bwd_inputs(fused_ref(case))
    xs, wp1 = dev_operands(ops, R)
    g1 = run_gram(R, xs, wp1)
    gate_gram(f"gram bwd {sid(case)} CW{gram_wgs(*case)[1]}", R, g1)
    assert torch.equal(g1, run_gram(R, xs, wp1)), "two runs differ: the Gram path promises bit-equal results"


FOLD_NS = [1, 32, 33, 64, 65, 97]   # no pair loop, exactly the groups, one tail, one pair, pair + tail, two-deep


@gpu
@pytest.mark.parametrize("ns", FOLD_NS)
def test_gram_slab_fold(ops, ns):
    """H = 4, W = 128, N = ns: one workgroup per image, so stem1_gram_part_kernel folds ns slabs."""
    from vlp_amd._lib import HipError
    case = (ns, 4, 128)
    assert gram_wgs(*case)[0] == ns
    R = bwd_inputs(fused_ref(case))
    xs, wp1 = dev_operands(ops, R)
    g1 = run_gram(R, xs, wp1)
    gate_gram(f"gram fold ns={ns}", R, g1)
    assert torch.equal(g1, run_gram(R, xs, wp1))
    with pytest.raises(HipError):                 # one float short: refused on the host, nothing written
        run_gram(R, xs, wp1, short=1)
    torch.cuda.synchronize()


@gpu
def test_gram_short_workspace_leaves_grad(ops):
    from vlp_amd._lib import HipError, lib
    R = bwd_inputs(fused_ref((1, 4, 128)))
    xs, wp1 = dev_operands(ops, R)
    n = ctypes.c_longlong(0)
    lib().vlp_stem1_bwd_fused_ws_floats(1, 4, 128, ctypes.byref(n))
    ws = torch.full((n.value,), SENT, device="cuda")
    grad = torch.full((64, 3, 7, 7), SENT, device="cuda")
    dp, idx, _, _, mean, istd, gamma, sum_g, sum_gx = bwd_dev(R)
    with pytest.raises(HipError):
        lib().vlp_stem1_bwd_fused(*[t.data_ptr() for t in (xs, wp1, dp, idx, mean, istd, gamma, sum_g, sum_gx)],
                                  ws.data_ptr(), n.value - 1, grad.data_ptr(), 1, 4, 128,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((grad == SENT).all()) and bool((ws == SENT).all())


# ---------------------------------------------------------------- exact tap order
def first_valid_tap(Hq, Wq):
    t = torch.zeros(Hq, Wq, dtype=torch.uint8)
    t[0, :], t[:, 0], t[0, 0] = 3, 1, 4
    return t


@gpu
@pytest.mark.parametrize("case", [(3, 7, 127), (1, 36, 384)], ids=sid)
def test_all_zero_image_ties_every_tap(ops, case):
    """Every y0 is +-0 and every tap ties: idx is the first non-padding tap, yarg == 0, the sums are 0.
    The image value that normalises to exactly 0 does not exist in uint8, so the image is zeroed
    through the mean: mean = 0 and an all-zero uint8 image."""
    N, H, W = case
    R = fused_ref(case, xu=torch.zeros(N, 1, H, W, dtype=torch.uint8), tag="zero")
    assert ops.stem1_fused_ok(H, W)
    Ho, Wo, Hp, Wp1 = ops.stem1_geom(H, W)
    xs = with_tail(torch.zeros(4, N, Hp, Wp1, dtype=BF16), "cuda")
    ops.stem1_prep_u8(with_tail(R["xu"], "cuda"), xs, 0.0, STD)
    wp1 = with_tail(torch.zeros(64, 64, dtype=BF16), "cuda")
    ops.pack_stem1(with_tail(R["w"], "cuda"), wp1)
    Hq, Wq = Ho // 2, Wo // 2
    ybuf, yarg = guarded((N, Hq, Wq, 64), BF16, "cuda")
    ibuf, idx = guarded((N, Hq, Wq, 64), torch.uint8, "cuda", IDX_SENT)
    s, ss = stat_buf(4, "cuda"), stat_buf(4, "cuda")
    ops.stem1_pool_fwd(xs, wp1, with_tail(R["gamma"], "cuda"), yarg, idx, N, H, W, s, ss, 4)
    torch.cuda.synchronize()
    guard_ok("zero yarg", ybuf, N * Hq * Wq)
    guard_ok("zero idx", ibuf, N * Hq * Wq, IDX_SENT)
    assert bool((xs == 0).all())
    want = first_valid_tap(Hq, Wq).view(1, Hq, Wq, 1).expand(N, Hq, Wq, 64)
    assert torch.equal(idx.cpu(), want), "tap order: not the first non-padding tap on an exact tie"
    assert bool((yarg.float() == 0).all())
    assert bool((stat_total("zero", s, 4) == 0).all()) and bool((stat_total("zero", ss, 4) == 0).all())


@gpu
@pytest.mark.parametrize("case", [(3, 36, 128), (1, 36, 511)], ids=sid)
def test_constant_image_ties_interior_windows(ops, case):
    """A constant non-zero image: every conv pixel whose 7x7 patch lies inside the image has the same
    y0 (same products, same order), so a window of nine such pixels ties exactly: idx == 0, for both
    signs of gamma."""
    N, H, W = case
    R = fused_ref(case, xu=torch.full((N, 1, H, W), 201, dtype=torch.uint8), tag="const")
    _, _, ia, _, _ = run_fwd(ops, R, True, 1)
    Ho, Wo = R["Ho"], R["Wo"]
    h, w = torch.arange(Ho), torch.arange(Wo)
    inside = ((2 * h - 3 >= 0) & (2 * h + 3 <= H - 1)).view(Ho, 1) & ((2 * w - 3 >= 0) & (2 * w + 3 <= W - 1)).view(1, Wo)
    win_in = windows(inside.double().view(1, 1, Ho, Wo))[0, 0]           # NaN at padding taps
    full = (torch.nan_to_num(win_in, nan=0.0).sum(-1) == 9)              # [Hq, Wq]
    assert int(full.sum()) > 0
    t = ia.permute(0, 3, 1, 2)[:, :, full]
    assert bool((t == 0).all()), f"{int((t != 0).sum())} interior windows did not keep the first tap on a tie"
    assert bool((R["gamma"] < 0).any()) and bool((R["gamma"] > 0).any())


# ---------------------------------------------------------------- refusals
@gpu
@pytest.mark.parametrize("N,H,W", [(1, 4, 192), (1, 4, 640), (1, 10, 128), (0, 4, 128)],
                         ids=["Wo96", "Wo320", "Ho-odd", "N0"])
def test_fused_launchers_refuse(ops, N, H, W):
    """Host checks before any launch: an error through ops, outputs untouched."""
    if N > 0:
        assert not ops.stem1_fused_ok(H, W)
    Nb = max(N, 1)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp1 = 2 * Ho + 6, (2 * Wo + 8 + 7) // 8 * 8
    dev = "cuda"
    xs = torch.zeros(4, Nb, Hp, Wp1, dtype=BF16, device=dev)
    wp1 = torch.zeros(64, 64, dtype=BF16, device=dev)
    Hq, Wq = (Ho + 1) // 2, (Wo + 1) // 2
    yarg = torch.full((Nb, Hq, Wq, 64), SENT, dtype=BF16, device=dev)
    idx = torch.full((Nb, Hq, Wq, 64), IDX_SENT, dtype=torch.uint8, device=dev)
    dy = torch.full((Nb, Ho, Wo, 64), SENT, dtype=BF16, device=dev)
    grad = torch.full((64, 3, 7, 7), SENT, device=dev)
    s, ss = torch.full((64,), SENT, dtype=torch.float64, device=dev), torch.full((64,), SENT, dtype=torch.float64, device=dev)
    vec = torch.ones(64, device=dev)
    dvec = torch.ones(64, dtype=torch.float64, device=dev)
    dp = torch.zeros(Nb, Hq, Wq, 64, dtype=BF16, device=dev)
    tap = torch.full((Nb, Hq, Wq, 64), 4, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError):
        ops.stem1_pool_fwd(xs, wp1, vec, yarg, idx, N, H, W, s, ss, 1)
    with pytest.raises(RuntimeError):
        ops.stem1_route_bwd(xs, wp1, dp, tap, vec, vec, vec, vec, vec, dvec, dvec, dy, N, H, W)
    with pytest.raises(RuntimeError):
        ops.stem1_bwd_fused_into(xs, wp1, dp, tap, vec, vec, vec, dvec, dvec, N, H, W, grad)
    torch.cuda.synchronize()
    assert bool((yarg == SENT).all()) and bool((idx == IDX_SENT).all()) and bool((dy == SENT).all())
    assert bool((grad == SENT).all()) and bool((s == SENT).all()) and bool((ss == SENT).all())


# ---------------------------------------------------------------- unfused: prep
@gpu
@pytest.mark.parametrize("dt", [BF16, F32], ids=dtid)
@pytest.mark.parametrize("case", [(3, 7, 13), (2, 18, 30), (1, 36, 29)], ids=sid)
def test_stem_prep_bit_equal(ops, dt, case):
    """vlp_stem_prep (fp32 NCHW) and vlp_stem_prep_u8 into the padded NHWC4 image: bit-equal to the
    reference, channel 3 zero, the pre-zeroed padding still zero, the sentinel behind intact."""
    N, H, W = case
    g = torch.Generator().manual_seed(H * W + N)
    Ho, Wo, Hp, Wp = ops.stem_geom(H, W)
    xu = torch.randint(0, 256, (N, 1, H, W), generator=g, dtype=torch.uint8)
    x3 = torch.randn(N, 3, H, W, generator=g)
    for kind in ("f32", "u8"):
        buf = torch.zeros(N * Hp * Wp * 4 + TAIL, dtype=dt, device="cuda")
        buf[N * Hp * Wp * 4:] = SENT
        xp = buf[:N * Hp * Wp * 4].view(N, Hp, Wp, 4)
        ref = torch.zeros(N, Hp, Wp, 4, dtype=dt)
        if kind == "f32":
            ops.stem_prep(with_tail(x3, "cuda"), xp)
            ref[:, 3:3 + H, 3:3 + W, :3] = x3.permute(0, 2, 3, 1).to(dt)
        else:
            ops.stem_prep_u8(with_tail(xu, "cuda"), xp, MEAN, STD)
            ref[:, 3:3 + H, 3:3 + W, :3] = image_f32(xu)[:, 0].to(dt).unsqueeze(-1)
        torch.cuda.synchronize()
        assert torch.equal(xp.cpu(), ref), f"stem_prep {kind}: not bit-equal"
        assert bool((buf[N * Hp * Wp * 4:] == SENT).all()), f"stem_prep {kind}: wrote past the image"


# ---------------------------------------------------------------- unfused: forwards and weight gradients
STEM3 = [(1, 10, 14), (3, 18, 30), (2, 36, 58)]      # M = 35, 405 (Wo = 15), 1044 (Wo = 29: Wo % 4 != 0)
STEM1 = [(2, 6, 8), (9, 7, 16), (3, 36, 40)]         # M = 24, 288, 1080; Wo % 4 == 0
STEM3_SPLIT, STEM1_SPLIT = (4, 64, 126), (4, 64, 128)   # M = 8064 / 8192: up to 3 / 4 splits of >= 2048 pixels


def unfused_ref(ch, case, dt):
    """Operands of one unfused case: x [N, ch, H, W] and w [64, ch, 7, 7] as fp64 of the storage dtype."""
    key = ("u", ch, case, dt)
    if key in _REF:
        return _REF[key]
    N, H, W = case
    g = torch.Generator().manual_seed(31 * H + W + N + ch)
    xu = torch.randint(0, 256, (N, 1, H, W), generator=g, dtype=torch.uint8)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    x = image_f32(xu).to(dt).double()
    if ch == 3:
        x, wd = x.repeat(1, 3, 1, 1), w.to(dt).double()
    else:
        wd = ((w[:, 0] + w[:, 1]) + w[:, 2]).to(dt).double().unsqueeze(1)
    y = F.conv2d(x, wd, stride=2, padding=3)
    S = F.conv2d(x.abs(), wd.abs(), stride=2, padding=3)
    dy = torch.randn(y.shape, generator=g).to(dt)                       # NCHW
    gw = torch.nn.grad.conv2d_weight(x, wd.shape, dy.double(), stride=2, padding=3)
    gwa = torch.nn.grad.conv2d_weight(x.abs(), wd.shape, dy.double().abs(), stride=2, padding=3)
    R = dict(xu=xu, w=w, x=x, wd=wd, y=y, S=S, dy=dy, gw=gw, gwa=gwa)
    _REF[key] = R
    return R


def gate_unfused_fwd(name, R, ch, dt, y, s, ss):
    K = K3 if ch == 3 else K1
    ref, S = R["y"], R["S"]
    noise = (K / 2) * EPS32 * S
    bound = 2.0 * (2.0 ** -9 * ref.abs() + noise) if dt == BF16 else noise
    check(name, "unfused y " + dtid(dt), y.permute(0, 3, 1, 2), ref, bound, rel_gate=tol(dt))
    check(name + " sum", "unfused sums", s, ref.sum((0, 2, 3)), sum_bound(noise, ref, 256, (0, 2, 3)), rel_gate=tol(dt))
    check(name + " sumsq", "unfused sums", ss, (ref * ref).sum((0, 2, 3)),
          sum_bound(2 * ref.abs() * noise, ref * ref, 256, (0, 2, 3)), rel_gate=tol(dt))


def gate_wgrad(name, R, ch, dt, grad):
    """grad [64, 3, 7, 7] (CPU)."""
    assert bool(torch.isfinite(grad).all()), f"{name}: non-finite gradient"
    bound = C_ACC * EPS32 * R["gwa"]
    if ch == 1:
        assert torch.equal(grad[:, 0], grad[:, 1]) and torch.equal(grad[:, 0], grad[:, 2]), f"{name}: channel copies differ"
        grad = grad[:, :1]
    check(name, "weight gradient", grad, R["gw"], bound, rel_gate=tol(dt) / 2)


def unfused_operands(ops, R, ch, case, dt):
    N, H, W = case
    if ch == 3:
        Ho, Wo, Hp, Wp = ops.stem_geom(H, W)
        xp = with_tail(torch.zeros(N, Hp, Wp, 4, dtype=dt), "cuda")
        ops.stem_prep_u8(with_tail(R["xu"], "cuda"), xp, MEAN, STD)
        wp = with_tail(torch.zeros(64, 256, dtype=dt), "cuda")
        ops.pack_stem(with_tail(R["w"], "cuda"), wp)
    else:
        Ho, Wo, Hp, Wp = ops.stem1_geom(H, W)
        xp = with_tail(torch.zeros(4, N, Hp, Wp, dtype=dt), "cuda")
        ops.stem1_prep_u8(with_tail(R["xu"], "cuda"), xp, MEAN, STD)
        wp = with_tail(torch.zeros(64, 64, dtype=dt), "cuda")
        ops.pack_stem1(with_tail(R["w"], "cuda"), wp)
    return Ho, Wo, xp, wp


def ucases():
    return [(3, c) for c in STEM3] + [(1, c) for c in STEM1]


def uid(v):
    return f"stem{v[0]}-{sid(v[1])}"


@gpu
@pytest.mark.parametrize("dt", [BF16, F32], ids=dtid)
@pytest.mark.parametrize("chc", ucases(), ids=uid)
def test_unfused_forward(ops, chc, dt):
    ch, case = chc
    N, H, W = case
    R = unfused_ref(ch, case, dt)
    Ho, Wo, xp, wp = unfused_operands(ops, R, ch, case, dt)
    for rep in (1, 4):
        ybuf, y = guarded((N, Ho, Wo, 64), dt, "cuda")
        s, ss = stat_buf(rep, "cuda"), stat_buf(rep, "cuda")
        (ops.stem_fwd if ch == 3 else ops.stem1_fwd)(xp, wp, N, H, W, y, s, ss, rep)
        torch.cuda.synchronize()
        name = f"stem{ch}_fwd {sid(case)} {dtid(dt)} rep{rep}"
        guard_ok(name, ybuf, N * Ho * Wo)
        gate_unfused_fwd(name, R, ch, dt, y.float().cpu() if dt == BF16 else y.cpu(), stat_total(name, s, rep),
                         stat_total(name, ss, rep))


def run_wgrad_ws(R, ch, case, dt, xp, slabs):
    """vlp_stem*_wgrad_ws into `slabs` slabs + NaN tail, then the fold into a NaN-prefilled gradient."""
    from vlp_amd._lib import lib
    N, H, W = case
    slab = 64 * (256 if ch == 3 else 64)
    nws = slabs * slab
    ws = torch.full((nws + 1024,), float("nan"), device="cuda")
    grad = torch.full((64 + 8, 3, 7, 7), float("nan"), device="cuda")
    grad[64:] = SENT
    dy = with_tail(R["dy"].permute(0, 2, 3, 1).contiguous(), "cuda")
    ns = ctypes.c_int(0)
    st = torch.cuda.current_stream().cuda_stream
    pre = "vlp_stem_" if ch == 3 else "vlp_stem1_"
    getattr(lib(), pre + "wgrad_ws")(1 if dt == BF16 else 0, dy.data_ptr(), xp.data_ptr(), ws.data_ptr(), nws,
                                     ctypes.addressof(ns), N, H, W, st)
    assert 1 <= ns.value <= slabs
    getattr(lib(), pre + "wgrad_fold")(ns.value, ws.data_ptr(), grad.data_ptr(), st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nws:]).all()), "slab writes past the workspace"
    assert bool((grad[64:] == SENT).all()), "rows beyond the gradient written"
    return ns.value, grad[:64].cpu()


@gpu
@pytest.mark.parametrize("dt", [BF16, F32], ids=dtid)
@pytest.mark.parametrize("chc", ucases() + [(3, STEM3_SPLIT), (1, STEM1_SPLIT)], ids=uid)
def test_unfused_weight_gradient(ops, chc, dt):
    """Split slabs + fold (bf16), atomics into slab 0 (fp32), and vlp_stem_wgrad's atomics; the slab's
    kh = 7, kw = 7 and c = 3 columns must not reach the [64][3][7][7] gradient."""
    ch, case = chc
    N, H, W = case
    R = unfused_ref(ch, case, dt)
    Ho, Wo, xp, _ = unfused_operands(ops, R, ch, case, dt)
    M = N * Ho * Wo
    counts = []
    for slabs in (1, 2, 64):
        ns, grad = run_wgrad_ws(R, ch, case, dt, xp, slabs)
        counts.append(ns)
        gate_wgrad(f"stem{ch}_wgrad_ws {sid(case)} {dtid(dt)} {ns} of {slabs} slabs", R, ch, dt, grad)
        if dt == BF16:
            _, again = run_wgrad_ws(R, ch, case, dt, xp, slabs)
            assert torch.equal(grad, again), "the split-slab fold promises bit-equal runs"
    print(f"stem{ch} {sid(case)} {dtid(dt)}: M = {M}, splits {counts}")
    assert counts[0] == 1
    if dt == F32:
        assert counts == [1, 1, 1], "fp32 accumulates into slab 0"
    elif M >= 4096:
        assert counts[1] == 2 and counts[2] == M // 2048, "a split is >= 2048 pixels deep"
    if ch == 3:
        ws = torch.zeros(64 + 8, 256, device="cuda")
        ws[64:] = SENT
        ops.stem_wgrad(with_tail(R["dy"].permute(0, 2, 3, 1).contiguous(), "cuda"), xp, N, H, W, ws)
        torch.cuda.synchronize()
        assert bool((ws[64:] == SENT).all())
        g = ws[:64].cpu().view(64, 8, 8, 4)[:, :7, :7, :3].permute(0, 3, 1, 2)
        gate_wgrad(f"stem_wgrad atomics {sid(case)} {dtid(dt)}", R, ch, dt, g)


# ---------------------------------------------------------------- unfused: max-pool with BN + ReLU on load
def pool_inputs(N, H, W, dt, const):
    g = torch.Generator().manual_seed(5 * H + W)
    y = torch.full((N, H, W, 64), 0.75) if const else torch.randn(N, H, W, 64, generator=g)
    return y.to(dt), chan(g, 1.0), chan(g, 0.3)


def gate_pool(name, y, sc, sh, dt, out, idx, yarg):
    N, H, W, _ = y.shape
    yd = y.double().permute(0, 3, 1, 2)
    a, b = sc.double().view(1, 64, 1, 1), sh.double().view(1, 64, 1, 1)
    q, Sq = torch.relu(yd * a + b), (yd * a).abs() + b.abs()
    win, wS = windows2(q), windows2(Sq)
    t = idx.permute(0, 3, 1, 2).long()
    assert int(t.max()) <= 8
    chosen = torch.gather(win, -1, t.unsqueeze(-1)).squeeze(-1)
    assert not bool(torch.isnan(chosen).any()), f"{name}: a padding tap was chosen"
    e32 = EPS32 * wS
    ec = torch.gather(e32, -1, t.unsqueeze(-1)).squeeze(-1)
    bound = 2.0 * (2.0 ** -9 * chosen.abs() + ec) if dt == BF16 else ec
    best = torch.nan_to_num(win, nan=-float("inf")).max(-1).values
    check(name, "max-pool out", out.permute(0, 3, 1, 2), best, bound + (best - chosen), rel_gate=tol(dt))
    over = torch.nan_to_num(win - chosen.unsqueeze(-1) - e32 - ec.unsqueeze(-1), nan=-1.0)
    assert int((over > 0).sum()) == 0, f"{name}: the tap is no maximiser within the bound"
    ya = torch.gather(windows2(yd), -1, t.unsqueeze(-1)).squeeze(-1)
    assert torch.equal(yarg.double().permute(0, 3, 1, 2), ya), f"{name}: yarg is not y at the tap"


def windows2(y):
    """windows() for any H, W: [N, C, Ho, Wo, 9], Ho = (H - 1) // 2 + 1"""
    N, C, H, W = y.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = F.pad(y, (1, 2, 1, 2), value=float("nan"))
    return torch.stack([pad[:, :, dh:dh + 2 * Ho:2, dw:dw + 2 * Wo:2] for dh in range(3) for dw in range(3)], -1)


@gpu
@pytest.mark.parametrize("dt", [BF16, F32], ids=dtid)
@pytest.mark.parametrize("const", [False, True], ids=["random", "tie"])
@pytest.mark.parametrize("case", [(3, 18, 30), (2, 5, 7)], ids=sid)
def test_maxpool_fwd_bn_on_load(ops, case, const, dt):
    N, H, W = case
    y, sc, sh = pool_inputs(N, H, W, dt, const)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    obuf, out = guarded((N, Ho, Wo, 64), dt, "cuda")
    abuf, yarg = guarded((N, Ho, Wo, 64), dt, "cuda")
    ibuf, idx = guarded((N, Ho, Wo, 64), torch.uint8, "cuda", IDX_SENT)
    ops.maxpool_fwd(with_tail(y, "cuda"), with_tail(sc, "cuda"), with_tail(sh, "cuda"), out, idx, yarg)
    torch.cuda.synchronize()
    name = f"maxpool_fwd {sid((N, H, W))} {dtid(dt)} {'tie' if const else 'random'}"
    for nm, bf, fill in (("out", obuf, SENT), ("yarg", abuf, SENT), ("idx", ibuf, IDX_SENT)):
        guard_ok(f"{name} {nm}", bf, N * Ho * Wo, fill)
    gate_pool(name, y, sc, sh, dt, out.float().cpu(), idx.cpu(), yarg.float().cpu())
    if const:
        want = first_valid_tap(Ho, Wo).view(1, Ho, Wo, 1).expand(N, Ho, Wo, 64)
        assert torch.equal(idx.cpu(), want), "a constant input must give the first valid tap"


# ---------------------------------------------------------------- CPU: the bounds are satisfiable and sensitive
def emu_fwd(R):
    """fp32 conv, bf16 row, first maximum on the bf16 values, fp32 partial sums of T pixels, fp64 totals."""
    acc = F.conv2d(R["x"].float(), R["w1"].float(), stride=2, padding=3)
    vb = acc.to(BF16)
    key = torch.nan_to_num(windows(vb.double() * R["sg"]), nan=-float("inf"))
    t = first_max(key)
    yarg = torch.gather(windows(vb.double()), -1, t.unsqueeze(-1)).squeeze(-1)
    T = 2 * K_BAND * R["Wo"]
    rows = vb.float().permute(0, 2, 3, 1).reshape(-1, 64)
    return (yarg.permute(0, 2, 3, 1).float(), t.permute(0, 2, 3, 1).to(torch.uint8), emu_sum(rows, T),
            emu_sum(rows * rows, T), vb)


def emu_coefs(R):
    f = lambda t_: t_.float().view(1, 64, 1, 1)               # noqa: E731
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(R["M"]), dtype=F32)
    is_, k = f(R["istd"]), f(R["gamma"]) * f(R["istd"])
    mg = (R["sum_g"] * inv.double()).float().view(1, 64, 1, 1)
    mgx = (R["sum_gx"] * inv.double()).float().view(1, 64, 1, 1)
    return k, -k * is_ * mgx, -k * mg + k * is_ * mgx * f(R["mean"])


def route32(R, dp=None):
    """fp32 window sums of the routed gradient in the kernel's order: [N, 64, Ho, Wo]"""
    dp = R["dp"] if dp is None else dp
    N, Hq, Wq = R["N"], R["Hq"], R["Wq"]
    t = R["idx"].permute(0, 3, 1, 2).long()
    n, c, i, j = torch.meshgrid(torch.arange(N), torch.arange(64), torch.arange(Hq), torch.arange(Wq), indexing="ij")
    g = torch.zeros(N, 64, R["Ho"] + 2, R["Wo"] + 2)
    g.index_put_((n.reshape(-1), c.reshape(-1), (2 * i + t // 3).reshape(-1), (2 * j + t % 3).reshape(-1)),
                 dp.permute(0, 3, 1, 2).float().reshape(-1), accumulate=True)
    return g[:, :, 1:-1, 1:-1]


def emu_dy(R, vb, g32=None):
    k, b, c = emu_coefs(R)
    g32 = route32(R) if g32 is None else g32
    inner = (b.double() * vb.double() + c.double()).float()                       # fmaf: one rounding
    return (k.double() * g32.double() + inner.double()).float().to(BF16).float().permute(0, 2, 3, 1)


def emu_gram_slabs(R):
    """One fp32 slab [R | G | S] (49-column form) per workgroup, in blockIdx order (n, band, column block)."""
    N, Ho, Wo, Hq = R["N"], R["Ho"], R["Wo"], R["Hq"]
    _, cw = gram_wgs(N, R["H"], R["W"])
    P = F.unfold(R["x"], 7, padding=3, stride=2).transpose(1, 2).reshape(N, Ho, Wo, 49).float()
    gb = route32(R).to(BF16).float().permute(0, 2, 3, 1)                          # bf16 of the fp32 window sum
    slabs = []
    for n in range(N):
        for i0 in range(0, Hq, G_BAND):
            r0, r1 = 2 * i0, 2 * min(i0 + G_BAND, Hq)
            for c0 in range(0, Wo, cw):
                p = P[n, r0:r1, c0:c0 + cw].reshape(-1, 49)
                gg = gb[n, r0:r1, c0:c0 + cw].reshape(-1, 64)
                slabs.append(torch.cat([(gg.t() @ p).reshape(-1), (p.t() @ p).reshape(-1), p.sum(0)]))
    return torch.stack(slabs)


def emu_gram_fold(R, slabs, drop=None):
    """stem1_gram_part_kernel (two fp32 accumulators per group), then fp64."""
    ns = slabs.shape[0]
    acc = [torch.zeros(G_GROUPS, slabs.shape[1]), torch.zeros(G_GROUPS, slabs.shape[1])]
    for lvl in range((ns + G_GROUPS - 1) // G_GROUPS):
        for grp in range(min(G_GROUPS, ns - lvl * G_GROUPS)):
            s = lvl * G_GROUPS + grp
            if s != drop:
                acc[lvl % 2][grp] += slabs[s]
    tot = (acc[0] + acc[1]).double().sum(0)
    Rm, G, Sv = tot[:64 * 49].view(64, 49), tot[64 * 49:64 * 49 + 49 * 49].view(49, 49), tot[-49:].view(1, 49)
    k, b, c = (R[n_].reshape(64, 1) for n_ in ("k", "b", "c"))
    v = (k * Rm + b * (R["w1"].reshape(64, 49) @ G) + c * Sv).float()
    return v.view(64, 1, 7, 7).repeat(1, 3, 1, 1)


def emu_unfused(ch, case, dt):
    R = unfused_ref(ch, case, dt)
    acc = F.conv2d(R["x"].float(), R["wd"].float(), stride=2, padding=3)
    rows = acc.permute(0, 2, 3, 1).reshape(-1, 64)
    name = f"emulated stem{ch} {sid(case)} {dtid(dt)}"
    gate_unfused_fwd(name, R, ch, dt, acc.to(dt).float().permute(0, 2, 3, 1), emu_sum(rows, 256), emu_sum(rows * rows, 256))
    gw = torch.nn.grad.conv2d_weight(R["x"].float(), R["wd"].shape, R["dy"].float(), stride=2, padding=3)
    gate_wgrad(name + " wgrad", R, ch, dt, gw.repeat(1, 3, 1, 1) if ch == 1 else gw)


def violates(fn, *a):
    """the per-element gate must fail; returns the assertion text (which carries the figures)"""
    with pytest.raises(AssertionError) as e:
        fn(*a)
    return str(e.value)


def rel_l2(a, b):
    return float((a.double() - b).norm() / b.norm())




def test_bound_holds_for_emulated_arithmetic():
    """Each family's fp32 sequence replayed in torch on the suite's own inputs meets every bound with zero
    violations (the CPU column of the module docstring); then four defects are planted in the emulated
    results and the per-element gate catches each, while the earlier rel-L2 gate would have let the
    first two pass (the other two it never saw: no earlier case had a partial band or ns > 8)."""
    WORST.clear()
    for case in FUSED + [(ns, 4, 128) for ns in FOLD_NS[1:]]:
        R = bwd_inputs(fused_ref(case))
        name = f"emulated {sid(case)}"
        ya, ia, s, ss, vb = emu_fwd(R)
        gate_fwd(name + " fwd", R, ya, ia, s, ss, R["N"] * ((R["Hq"] + K_BAND - 1) // K_BAND))
        gate_dy(name + " dy", R, emu_dy(R, vb))
        gate_gram(name + " gram", R, emu_gram_fold(R, emu_gram_slabs(R)))
    for ch, case in ucases():
        for dt in (BF16, F32):
            emu_unfused(ch, case, dt)
    for dt in (BF16, F32):
        for const in (False, True):
            y, sc, sh = pool_inputs(2, 5, 7, dt, const)
            q = torch.relu(y.float() * sc + sh).permute(0, 3, 1, 2)               # fp32, then the store rounding
            t = first_max(torch.nan_to_num(windows2(q.double()), nan=-float("inf")))
            out = torch.gather(windows2(q.double()), -1, t.unsqueeze(-1)).squeeze(-1).to(dt).float()
            ya = torch.gather(windows2(y.double().permute(0, 3, 1, 2)), -1, t.unsqueeze(-1)).squeeze(-1).float()
            gate_pool(f"emulated maxpool {dtid(dt)}", y, sc, sh, dt, out.permute(0, 2, 3, 1),
                      t.permute(0, 2, 3, 1).to(torch.uint8), ya.permute(0, 2, 3, 1))
    print("worst emulated |err| / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    print("staged shares: " + ", ".join(f"{k} {100 * v:.2f} %" for k, v in sorted(SHARES.items())))
    assert all(v <= 1.0 for v in WORST.values())
    keep = dict(WORST)

    # ---- sensitivity: defects a kernel could have, planted in the emulated result
    R = bwd_inputs(fused_ref((3, 132, 512)))
    _, _, _, _, vb = emu_fwd(R)
    good = emu_dy(R, vb)
    ref_dy = (R["k"] * R["g"] + R["b"] * R["v"] + R["c"]).permute(0, 2, 3, 1)
    # (1) the route backward's second pair band (conv rows 16 ..) recomputes the edge column of row 16
    #     from the neighbouring band's patches (row 15), in one image: 64 of 3.2e6 elements
    bad = vb.clone()
    bad[0, :, 16, -1] = vb[0, :, 15, -1]
    d1 = emu_dy(R, bad)
    msg1 = violates(gate_dy, "defect: edge column of conv row 16 taken from the band above", R, d1)
    # (2) the last window of pooled row 8 routes one tap to the right (taps 0, 1, 3, 4, 6, 7: stays in range)
    idx2 = R["idx"].clone()
    row = idx2[0, 8, -1]
    idx2[0, 8, -1] = torch.where(row % 3 != 2, row + 1, row)
    d2 = emu_dy(R, vb, route32(dict(R, idx=idx2)))
    msg2 = violates(gate_dy, "defect: one window routed one tap to the right", R, d2)
    r1, r2 = rel_l2(d1, ref_dy), rel_l2(d2, ref_dy)
    print(f"sensitivity dy: clean rel-L2 {rel_l2(good, ref_dy):.2e}; wrong edge column {r1:.2e}; shifted tap {r2:.2e} "
          f"(earlier gate 1e-2)\n  {msg1}\n  {msg2}")
    assert r1 < 1e-2 and r2 < 1e-2, "both defects stay inside the earlier rel-L2 gate"
    # (3) the fold drops the tail slab at ns = 33, (4) the Gram kernel's partial band (pooled row 32 of
    #     H = 132) reads the patches of the row pair above
    R3 = bwd_inputs(fused_ref((33, 4, 128)))
    slabs = emu_gram_slabs(R3)
    g3 = emu_gram_fold(R3, slabs, drop=32)
    msg3 = violates(gate_gram, "defect: slab 32 of 33 dropped", R3, g3)
    r3 = rel_l2(g3[:, 0].reshape(64, 49), gram_ref(R3)[0])
    R4 = bwd_inputs(fused_ref((1, 132, 256)))
    slabs4 = emu_gram_slabs(R4)
    P = F.unfold(R4["x"], 7, padding=3, stride=2).transpose(1, 2).reshape(1, 66, 128, 49).float()
    gb = route32(R4).to(BF16).float().permute(0, 2, 3, 1)
    p_bad, gg = P[0, 62:64].reshape(-1, 49), gb[0, 64:66].reshape(-1, 64)
    slabs4[1] = torch.cat([(gg.t() @ p_bad).reshape(-1), (p_bad.t() @ p_bad).reshape(-1), p_bad.sum(0)])
    g4 = emu_gram_fold(R4, slabs4)
    msg4 = violates(gate_gram, "defect: the partial Gram band reads the row pair above", R4, g4)
    r4 = rel_l2(g4[:, 0].reshape(64, 49), gram_ref(R4)[0])
    print(f"sensitivity gram: dropped slab rel-L2 {r3:.2e}, partial band {r4:.2e} (earlier gate 2e-3)\n  {msg3}\n  {msg4}")
    WORST.clear()
    WORST.update(keep)
