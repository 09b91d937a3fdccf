"""Every route and fused epilogue of the convolution family against fp64.

csrc/conv_ops.hip sends vlp_conv_fwd / vlp_conv_dgrad* / vlp_conv_wgrad* to the
layer-1 rows kernels, the LDS-window kernel (W = 16 and 64 at the default
VLP_WIN_WIDTHS), the 256x256 ping-pong kernel, gemm_big<128,256> / <128,128> /
<256,64> / <64,192>, gemm_bk<256,64> / <64,128>, the register-staged launch_gemm
(C % 64 != 0, BN-on-load off the ping-pong path, all fp32) and two fold kernels.
The case ids name the kernel the bf16 call takes at GEMM variant 5.

Reference.  Inputs are rounded to the storage dtype first.  The reference is fp64
on the device: a sum over filter taps of shifted-slice matmuls on a zero-padded
NHWC tensor (`conv64`, `dgrad64`, `wgrad64`; stride by slicing), so it does not
depend on fp64 convolutions of the vendor library; test 1 proves the helpers
equal F.conv2d / conv2d_input / conv2d_weight in fp64 on the CPU.  The same
helpers on abs() operands give S = conv(|x|, |w|) (+ |addend|).

Rounding points, as the kernels have them (read from the code, not from the
epilogues' names).  EpiConvFwd rounds the fp32 accumulator once, on store, and its
sums are taken from the unrounded fp32 value.  The fp32 kernels and the
register-staged kernel (operator() form of every epilogue) add the addend in fp32,
mask, and round once.  But every bf16 data-gradient route -- the rows kernel, the
window kernel and the LDS-DMA GEMMs (ms_epilogue) -- runs the ROW-CHUNK form
(row8 / row8r / row8r3) of EpiDgradAdd / BN / Relu / Relu2: the accumulator is
first staged in LDS as v = bf16(acc), then addend, mask and the sums are applied
to v in fp32 and the result is rounded a second time on store.  The reference
follows that: g = mask * (bf16(acc64) + addend), the sums are those of this g
(unrounded at the second point).  The staged rounding can flip where fp32 and
fp64 accumulation land on different sides of a bf16 rounding boundary; `staged`
finds exactly those elements (acc64 within the accumulation-noise term of a
boundary) and allows one ulp of v there and nothing elsewhere, in the element
bound and, summed, in the sum bounds.  So "the addend is added after a bf16
rounding" is the bf16 kernels' documented behaviour (as EpiLinear's staging in the
linear suite), not something these tests can reject; an addend added after the
FINAL rounding, or a third rounding, would fail them.

Masks need no exclusion list.  fmaf(y, sc, sh) > 0 has the sign of the exact
value, and fp64 of bf16 x fp32 + fp32 reproduces that sign; relu_out > 0 and the
sign bits are exact.  Every masked case asserts out == 0 exactly where the
reference mask is 0, and the bound where it is 1.

Input transforms on load (ConvFwdA<T, true>, ConvFwdABn, rows XF = 1, rows
XF = 2) are formed as fp64 -> fp32 -> storage dtype (double-rounding mismatches
are of order 2^-29 per element; XF = 2 is fmaf(k, g, fmaf(b, y, c)) and the
reference rounds the inner fmaf to fp32 as well, because where k * g cancels it
that rounding exceeds a bf16 ulp of the result: 3 of 8.4e6 elements).  Where the kernel also writes the operand
(x_act, dy_out) it is gated against that at <= 1 ulp with the count of differing
elements printed, and the convolution reference is built from the DEVICE's
operand, so an operand flip and a convolution error are reported separately.
The shifts are > 0 on every second channel (every c of XF = 2 is non-zero), so a
transform leaking into the zero padding shows in the halo outputs.

Gate.  Each case asserts the suite's rel-L2 gate AND a per-element bound with
zero violations:
    bf16 outputs:      2 * (2^-9 |ref| + C_ACC * eps32 * S)
                       (+ one ulp of the staged v where `staged` finds a possible flip:
                       bf16 data gradients only)
    fp32 outputs:      C_F32 * K * eps32 * S
    weight gradients:  C_ACC * eps32 * (|dy| (*) |x|)
with the linear suite's constants and justification: 2^-9 |ref| is the one
rounding on store (half an ulp at the top of a binade, the leading 2 covers the
bottom and is the only margin); C_ACC = 64 (128 u, u = eps32 / 2) is the
random-walk figure sqrt(K) u at depth 16384, far below the worst case K u; the
deepest K here is 9 * 576 = 5184.  C_F32 = 1 is twice gamma_K = K u.  Weight
gradient depths per fp32 slab: the GEMM routes reduce all N * Ho * Wo pixels
of a case in at most one slab, <= 16384 here (largest: 16 * 32 * 32); the rows
kernel accumulates whole images per workgroup, N * H * 128 / slabs <= 1024 here.

BN sums, per channel (derived from the kernels' reduction, `sum_bound`):
    2 * ( sum_pixels noise * |f|  +  (T + 4) * eps32 * sum_pixels |g * f| )
  * noise is the element's accumulation term (C_ACC * eps32 * S for bf16,
    C_F32 * K * eps32 * S for fp32, zero where the mask is 0) carried linearly
    into the sum; f is 1 (stat1), |xhat| (stat2 / stat3), and for the forward sum
    of squares the term is 2 |v| noise.
  * every kernel sums its workgroup's rows in fp32 (lane partials, row16_sum, the
    per-wave partials) and then issues ONE fp64 atomic per column: a sum of T
    terms in fp32 is within T * u * sum |terms| for any order; eps32 = 2 u covers
    it, and the + 4 covers the fp32 evaluation of (y - mean) * invstd * g or v * v.
    T = rows per workgroup, read per kernel: 256 for the ping-pong, window,
    gemm_bk<256,64> and gemm_big<256,64> tiles (128 for the 128-row tiles and the
    register-staged kernel: 256 is used as the common upper figure), and
    ceil(N / min(CUs, N)) * H * 128 for the rows kernel, whose accumulators live
    across all images of a workgroup.
  * the leading 2 as in the element bound.
  Forward sums additionally keep the earlier 1e-4 relative gate, so the new gate
  is nowhere looser than it.  stat_rep 1 and 4 alternate over the cases.

Untouched memory.  Every output has 256 sentinel rows beyond M (the stride-2
remap scatters into a fully pre-filled output: an unwritten element keeps the
sentinel and fails the bound); statistic buffers have a sentinel replica beyond
stat_rep; workspaces have a NaN tail; inputs are followed by a 4096-element
guard of large values inside the same allocation.

`test_bound_holds_for_emulated_arithmetic` shows on the CPU that fp32
accumulation of the rounded inputs with one rounding on store, and fp32 partial
sums of T rows, meet every bound.  Worst ratios |err| / bound, emulated on the
CPU | measured on an MI355X:
    element bf16      0.988 | 0.989
    element fp32      0.023 | 0.025
    weight gradient   0.051 | 0.038
    sums              0.118 | 0.118
(the bf16 element figure approaches 1 by construction: 2 * 2^-9 |ref| is exactly the
half-ulp at the bottom of a binade).  The device column is the maximum over the
whole file's run.

Argument checks (last tests).  ConvFwdA::load / ConvDgradA::load / ConvWgradB
resolve the filter tap from the first element of a 16-byte chunk and the
epilogues store 4- or 8-column groups, so bf16 C = 100, bf16 Co = 100 and fp32
C = 6 let a chunk straddle a tap or a row; none is provably correct, and
vlp_conv_fwd / _dgrad / _dgrad_relu / _wgrad / _wgrad_ws now refuse a C or Co
that is no multiple of the chunk (8 bf16 / 4 fp32).  C = 96 (NesT) stays a case.
With C % 8 == 0 no bf16 shape has K % 4 != 0, so the atomics fallback of
conv_wgrad_ws_t is reached by fp32 only.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
EPS32 = 2.0 ** -23
C_ACC = 64.0
C_F32 = 1.0
GUARD = 256
SENT = -1024.0
TAIL = 4096
T_TILE = 256
WORST = {}


def tol(dt):
    return 2e-5 if dt == F32 else 1.5e-2


def dtid(dt):
    return "fp32" if dt == F32 else "bf16"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlp_amd import ops as o
    return o


def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count if dev != "cpu" else 256


# ---------------------------------------------------------------- reference
def out_hw(H, W, KH, S, P):
    return (H + 2 * P - KH) // S + 1, (W + 2 * P - KH) // S + 1


def conv64(x, w, S, P):
    """x [N][H][W][C], w [Co][KH][KW][C] -> [N][Ho][Wo][Co], in the operands' dtype."""
    N, H, W, C = x.shape
    Co, KH, KW, _ = w.shape
    Ho, Wo = out_hw(H, W, KH, S, P)
    xp = F.pad(x, (0, 0, P, P, P, P))
    y = torch.zeros(N, Ho, Wo, Co, dtype=x.dtype, device=x.device)
    for kh in range(KH):
        for kw in range(KW):
            xs = xp[:, kh:kh + S * (Ho - 1) + 1:S, kw:kw + S * (Wo - 1) + 1:S, :]
            y += xs @ w[:, kh, kw, :].t()
    return y


def dgrad64(dy, w, H, W, S, P):
    """dy [N][Ho][Wo][Co], w [Co][KH][KW][C] -> dx [N][H][W][C]."""
    N, Ho, Wo, Co = dy.shape
    _, KH, KW, C = w.shape
    dxp = torch.zeros(N, H + 2 * P, W + 2 * P, C, dtype=dy.dtype, device=dy.device)
    for kh in range(KH):
        for kw in range(KW):
            dxp[:, kh:kh + S * (Ho - 1) + 1:S, kw:kw + S * (Wo - 1) + 1:S, :] += dy @ w[:, kh, kw, :]
    return dxp[:, P:P + H, P:P + W, :].contiguous()


def wgrad64(dy, x, KH, S, P):
    """dy [N][Ho][Wo][Co], x [N][H][W][C] -> dw [Co][KH][KW][C]."""
    N, Ho, Wo, Co = dy.shape
    C = x.shape[-1]
    xp = F.pad(x, (0, 0, P, P, P, P))
    dw = torch.zeros(Co, KH, KH, C, dtype=dy.dtype, device=dy.device)
    d2 = dy.reshape(-1, Co).t()
    for kh in range(KH):
        for kw in range(KH):
            xs = xp[:, kh:kh + S * (Ho - 1) + 1:S, kw:kw + S * (Wo - 1) + 1:S, :]
            dw[:, kh, kw, :] = d2 @ xs.reshape(-1, C)
    return dw


def test_reference_helpers_match_torch_fp64():
    """conv64 / dgrad64 / wgrad64 against torch's fp64 convolution and its gradients:
    3x3/1, 3x3/2 and 1x1/2 at a small odd shape."""
    g = torch.Generator().manual_seed(1)
    for KH, S, P in ((3, 1, 1), (3, 2, 1), (1, 2, 0)):
        N, H, W, C, Co = 2, 7, 9, 5, 3
        x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
        w = torch.randn(Co, KH, KH, C, generator=g, dtype=torch.float64)
        xn, wn = x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
        y = F.conv2d(xn, wn, stride=S, padding=P)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        dyh = dy.permute(0, 2, 3, 1).contiguous()
        e1 = (conv64(x, w, S, P) - y.permute(0, 2, 3, 1)).abs().max().item()
        dx = torch.nn.grad.conv2d_input(xn.shape, wn, dy, stride=S, padding=P)
        e2 = (dgrad64(dyh, w, H, W, S, P) - dx.permute(0, 2, 3, 1)).abs().max().item()
        dw = torch.nn.grad.conv2d_weight(xn, wn.shape, dy, stride=S, padding=P)
        e3 = (wgrad64(dyh, x, KH, S, P) - dw.permute(0, 2, 3, 1)).abs().max().item()
        print(f"{KH}x{KH}/{S}: conv {e1:.1e}, dgrad {e2:.1e}, wgrad {e3:.1e}")
        assert max(e1, e2, e3) < 1e-12


# ---------------------------------------------------------------- gate
def noise_term(dt, S, K):
    return (C_ACC * EPS32) * S if dt == BF16 else (C_F32 * K * EPS32) * S


def elem_bound(dt, ref, S, K):
    if dt == BF16:
        return 2.0 * (2.0 ** -9 * ref.abs() + (C_ACC * EPS32) * S)
    return (C_F32 * K * EPS32) * S


def staged(acc64, noise):
    """The bf16 row-chunk epilogues' staged value bf16(acc) and, per element, what a flip of
    that rounding may move it by: one ulp where acc64 lies within the accumulation noise of
    a rounding boundary (where fp32 and fp64 accumulation can round apart), zero elsewhere."""
    v = acc64.to(BF16).double()
    m, e = torch.frexp(v.abs())
    ulp = torch.ldexp(torch.ones_like(v), e - 8) * (v != 0)
    d = (acc64 - v).abs()
    near = (ulp / 2 - d) <= noise
    near |= (m == 0.5) & ((ulp / 4 - d).abs() <= noise)   # below a power of two the spacing halves
    return v, torch.where(near, ulp, torch.zeros_like(ulp))


def sum_bound(noise_f, gf, T):
    """noise_f = noise * |f|, gf = g * f, both [pixels..., channels]."""
    dims = tuple(range(gf.dim() - 1))
    return 2.0 * (noise_f.sum(dims) + (T + 4) * EPS32 * gf.abs().sum(dims))


def _note(family, worst):
    WORST[family] = max(WORST.get(family, 0.0), worst)


def check(name, y, ref, bound, rel_tol, family):
    """rel-L2 and per-element gate; prints the figures before asserting."""
    y = y.double()
    d = (y - ref).abs()
    r = (torch.linalg.vector_norm(y - ref) / (torch.linalg.vector_norm(ref) + 1e-30)).item()
    nviol = int((~(d <= bound)).sum().item())   # NaN counts as a violation
    worst = (d / (bound + 1e-300)).max().item()
    _note(family, worst)
    print(f"{name}: rel-L2 {r:.3e} (gate {rel_tol:.1e}), per-element worst |err|/bound {worst:.3f}, "
          f"violations {nviol} of {ref.numel()}")
    assert r < rel_tol, f"{name}: rel-L2 {r:.3e} >= {rel_tol:.1e}"
    assert nviol == 0, f"{name}: {nviol} elements beyond the per-element bound (worst ratio {worst:.2f})"


def check_sum(name, got, ref, bound, rel_gate=None):
    d = (got - ref).abs()
    nviol = int((~(d <= bound)).sum().item())
    worst = (d / (bound + 1e-300)).max().item()
    r = (torch.linalg.vector_norm(got - ref) / (torch.linalg.vector_norm(ref) + 1e-30)).item()
    _note("sums", worst)
    print(f"{name}: rel-L2 {r:.3e}, per-channel worst |err|/bound {worst:.3f}, violations {nviol} of {ref.numel()}")
    assert nviol == 0, f"{name}: {nviol} channels beyond the sum bound (worst ratio {worst:.2f})"
    if rel_gate is not None:
        assert r < rel_gate, f"{name}: rel-L2 {r:.3e} >= {rel_gate:.1e}"


def gen_for(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def randn(shape, g, dev, scale=1.0):
    return torch.randn(shape, generator=g, device=dev) * scale


def with_tail(t):
    """t inside an allocation followed by TAIL large elements."""
    buf = torch.full((t.numel() + TAIL,), 100.0, dtype=t.dtype, device=t.device)
    buf[:t.numel()].copy_(t.flatten())
    return buf[:t.numel()].view(t.shape)


def guarded(shape, dt, dev):
    """A [.., Cc] output as the first rows of a sentinel-filled [M + GUARD][Cc] buffer."""
    Cc = shape[-1]
    M = math.prod(shape[:-1])
    buf = torch.full((M + GUARD, Cc), SENT, dtype=dt, device=dev)
    return buf, buf[:M].view(shape)


def assert_guard(name, buf, M):
    assert bool((buf[M:] == SENT).all().item()), f"{name}: rows beyond M written"


def stat_buf(rep, Cc, dev):
    s = torch.zeros((rep + 1) * Cc, dtype=torch.float64, device=dev)
    s[rep * Cc:] = SENT
    return s


def stat_total(name, s, rep, Cc):
    assert bool((s[rep * Cc:] == SENT).all().item()), f"{name}: statistics written beyond stat_rep replicas"
    return s[:rep * Cc].view(rep, Cc).sum(0)


def emu_sum(v32, T):
    """fp32 partial sums of T rows, then fp64: the kernels' reduction, emulated."""
    v = v32.reshape(-1, v32.shape[-1])
    pad = (-v.shape[0]) % T
    if pad:
        v = torch.cat([v, torch.zeros(pad, v.shape[1])])
    return v.view(-1, T, v.shape[1]).sum(1).double().sum(0)


def pack_bits(mask):
    """bit e & 7 of byte e >> 3 for element e."""
    m = mask.reshape(-1, 8).to(torch.int32)
    wgt = 2 ** torch.arange(8, device=mask.device, dtype=torch.int32)
    return (m * wgt).sum(1).to(torch.uint8)


def ulp_gate(name, got, ref, dt):
    """The operand a kernel writes against fp64 -> fp32 -> storage: at most 1 ulp."""
    a, b = got.double(), ref.double()
    d = (a - b).abs()
    ndiff = int((d > 0).sum().item())
    rel = 2.0 ** -7 if dt == BF16 else 2.0 ** -23
    nbad = int((~(d <= rel * torch.maximum(a.abs(), b.abs()))).sum().item())
    print(f"{name}: {ndiff} of {got.numel()} elements differ from the fp64 -> fp32 -> storage operand, "
          f"{nbad} by more than 1 ulp")
    assert nbad == 0


def xf_coeffs(C, g, dev):
    sc = (torch.rand(C, generator=g, device=dev) + 0.5) * torch.where(torch.arange(C, device=dev) % 5 == 0, -1.0, 1.0)
    sh = torch.where(torch.arange(C, device=dev) % 2 == 0, 0.3 + 0.3 * torch.rand(C, generator=g, device=dev),
                     -0.3 * torch.rand(C, generator=g, device=dev))
    return sc, sh


def resolve_n(N, dev):
    return cus(dev) - N if N < 0 else N


def rows_T(N, H, dev):
    grid = min(cus(dev), N)
    return ((N + grid - 1) // grid) * H * 128


# ---------------------------------------------------------------- forward
# (N, H, W, C, Co, KH, S, route); N < 0: CU count + |N| images
FWD_CASES = [
    (3, 5, 128, 64, 64, 3, 1, "rows_c64"),
    (2, 3, 128, 64, 64, 3, 1, "rows_c64-H3"),
    (-3, 4, 128, 64, 64, 3, 1, "rows_c64-images>CUs"),
    (2, 8, 64, 128, 128, 3, 1, "win64"),
    (2, 8, 64, 128, 256, 3, 1, "win64-2Ntiles"),
    (3, 4, 64, 256, 128, 3, 1, "win64-C256"),
    (2, 16, 16, 512, 512, 3, 1, "win16"),
    (2, 32, 16, 128, 128, 3, 1, "win16-2tiles-per-image"),
    (2, 12, 12, 256, 256, 3, 1, "pp256-partialM"),
    (4, 8, 8, 320, 256, 3, 1, "pp256-oddKsteps"),
    (2, 16, 32, 256, 256, 3, 1, "pp256-W32"),
    (1, 12, 12, 128, 256, 3, 1, "big128x256"),
    (2, 12, 12, 128, 128, 3, 1, "big128x128"),
    (2, 12, 12, 64, 64, 3, 1, "bk256x64"),
    (2, 12, 12, 64, 64, 1, 1, "bk256x64-1x1"),
    (2, 16, 16, 96, 192, 3, 1, "regstaged-C96"),
    (2, 13, 13, 64, 128, 3, 2, "big128x128-3x3s2"),
    (2, 13, 13, 64, 128, 1, 2, "big128x128-1x1s2"),
]
FWD_XF_CASES = [
    (2, 12, 12, 128, 256, 3, 1, "pp256-ConvFwdABn"),
    (2, 12, 12, 512, 256, 3, 1, "pp256-ConvFwdABn-C512"),
    (2, 12, 12, 128, 128, 3, 1, "reg-Co128"),
    (1, 12, 12, 128, 256, 3, 1, "reg-M<256"),
    (2, 12, 12, 576, 256, 3, 1, "reg-C576"),
    (2, 12, 12, 64, 64, 3, 1, "reg-narrow"),
]
FWD_F32_CASES = [
    (2, 12, 12, 64, 64, 3, 1, "launch_gemm-3x3"),
    (2, 13, 13, 64, 128, 3, 2, "launch_gemm-3x3s2"),
    (2, 13, 13, 64, 128, 1, 2, "launch_gemm-1x1s2"),
    (3, 5, 128, 64, 64, 3, 1, "launch_gemm-W128"),
]


def cid(c):
    return "x".join(str(v) for v in c[:-1]) + "-" + c[-1]


def run_fwd(ops, case, dt, dev, xf=False, rep=1, emulate=False, fused=False, seed=3):
    N, H, W, C, Co, KH, S, route = case
    N = resolve_n(N, dev)
    P = 1 if KH == 3 else 0
    K = KH * KH * C
    name = f"fwd {N}x{H}x{W}x{C}->{Co} {KH}x{KH}/{S} {route}{' xf' if xf else ''} {dtid(dt)}"
    g = gen_for(dev, seed)
    x = with_tail(randn((N, H, W, C), g, dev).to(dt))
    w = with_tail(randn((Co, KH, KH, C), g, dev, K ** -0.5).to(dt))
    sc = sh = None
    a = x
    if xf:
        sc, sh = xf_coeffs(C, g, dev)
        a = torch.relu(x.double() * sc.double() + sh.double()).float().to(dt)
    Ho, Wo = out_hw(H, W, KH, S, P)
    M = N * Ho * Wo
    ybuf, y = guarded((N, Ho, Wo, Co), dt, dev)
    s1, s2 = stat_buf(rep, Co, dev), stat_buf(rep, Co, dev)
    T = rows_T(N, H, dev) if route.startswith("rows") else T_TILE
    if emulate:
        v = conv64(a.float(), w.float(), S, P)
        y.copy_(v.to(dt))
        s1[:Co] = emu_sum(v, T)
        s2[:Co] = emu_sum(v * v, T)
    elif fused:
        abuf, a_dev = guarded((N, H, W, C), dt, dev)
        assert ops.conv_fwd_act_ok(x, Co, KH, KH, S, P)
        ops.conv_fwd_act(x, w, Co, KH, KH, S, P, sc, sh, a_dev, s1, s2, stat_rep=rep, out=y)
        torch.cuda.synchronize()
        assert_guard(name + " x_act", abuf, N * H * W)
        ulp_gate(name + " x_act", a_dev, a, dt)
        a = a_dev
    else:
        ops.conv_fwd(x, w, Co, KH, KH, S, P, sc, sh, s1, s2, out=y, stat_rep=rep)
        torch.cuda.synchronize()
    a64, w64 = a.double(), w.double()
    ref = conv64(a64, w64, S, P)
    Sabs = conv64(a64.abs(), w64.abs(), S, P)
    fam = "element " + dtid(dt)
    check(name, y, ref, elem_bound(dt, ref, Sabs, K), tol(dt), fam)
    assert_guard(name, ybuf, M)
    nz = noise_term(dt, Sabs, K)
    check_sum(name + " sum", stat_total(name, s1, rep, Co), ref.sum((0, 1, 2)), sum_bound(nz, ref, T), 1e-4)
    check_sum(name + " sumsq", stat_total(name, s2, rep, Co), (ref * ref).sum((0, 1, 2)),
              sum_bound(2.0 * ref.abs() * nz, ref * ref, T), 1e-4)


@gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=cid)
def test_conv_fwd_routes(ops, case):
    run_fwd(ops, case, BF16, "cuda", rep=4 if FWD_CASES.index(case) % 2 == 0 else 1)


@gpu
@pytest.mark.parametrize("case", FWD_XF_CASES, ids=cid)
def test_conv_fwd_bn_on_load_routes(ops, case):
    run_fwd(ops, case, BF16, "cuda", xf=True, rep=1 if FWD_XF_CASES.index(case) % 2 == 0 else 4)


@gpu
@pytest.mark.parametrize("xf", [False, True], ids=["raw", "xf"])
@pytest.mark.parametrize("case", FWD_F32_CASES, ids=cid)
def test_conv_fwd_fp32(ops, case, xf):
    run_fwd(ops, case, F32, "cuda", xf=xf, rep=4 if xf else 1)


ROWS_SHAPES = [(3, 5), (2, 3), (-3, 4)]


@gpu
@pytest.mark.parametrize("N,H", ROWS_SHAPES, ids=["N3-H5", "N2-H3", "images>CUs-H4"])
def test_conv_fwd_act_rows_xf1(ops, N, H):
    """vlp_conv_fwd_act (rows kernel, XF = 1) against fp64, not against the unfused path."""
    run_fwd(ops, (N, H, 128, 64, 64, 3, 1, "rows_c64-XF1"), BF16, "cuda", xf=True, rep=4, fused=True)


# ---------------------------------------------------------------- data gradient
# (N, H, W, C, Co, KH, S, route): dx [N][H][W][C] from dy [N][Ho][Wo][Co]
DGRAD_S1 = [
    (3, 5, 128, 64, 64, 3, 1, "rows_c64-flip"),
    (2, 32, 16, 128, 128, 3, 1, "win16-2tiles-per-image"),
    (2, 8, 64, 128, 128, 3, 1, "win64"),
    (2, 12, 12, 256, 256, 3, 1, "pp256"),
    (2, 12, 12, 128, 128, 3, 1, "big128x128"),
    (2, 12, 12, 64, 128, 3, 1, "bk256x64"),
]
DGRAD_S2 = [
    (2, 12, 12, 64, 128, 3, 2, "big256x64-H12"),
    (2, 13, 13, 64, 128, 3, 2, "big256x64-H13"),
    (2, 13, 13, 128, 256, 3, 2, "big128x128-H13"),
    (6, 13, 13, 256, 256, 3, 2, "pp256+big128x256-H13"),
    (2, 12, 14, 128, 128, 3, 2, "big128x128-H12xW14"),
    (2, 13, 13, 64, 128, 1, 2, "big256x64-1x1s2"),
]
EPIS = ["none", "add", "bn", "relu_act", "relu_bits", "relu_bits_add", "relu2"]


def dgrad_cases():
    out = []
    for c in DGRAD_S1:
        for e in EPIS:
            if e == "relu2" and c[3] < 128:
                continue
            out.append((c, e))
    for c in DGRAD_S2:
        for e in ("none", "add", "bn", "relu_act", "relu_bits_add"):
            out.append((c, e))
    return out


def run_dgrad(ops, case, epi, dt, dev, rep=1, emulate=False, fused=False, seed=5):
    N, H, W, C, Co, KH, S, route = case
    N = resolve_n(N, dev)
    P = 1 if KH == 3 else 0
    K = KH * KH * Co
    Ho, Wo = out_hw(H, W, KH, S, P)
    M = N * H * W
    name = f"dgrad {N}x{H}x{W}x{C}<-{Co} {KH}x{KH}/{S} {route} {epi}{' fused' if fused else ''} {dtid(dt)}"
    g = gen_for(dev, seed)
    w = randn((Co, KH, KH, C), g, dev, K ** -0.5).to(dt)          # [Co][KH][KW][C]
    wt = with_tail(w.permute(3, 1, 2, 0).contiguous())             # Wt [C][KH][KW][Co]
    dy = with_tail(randn((N, Ho, Wo, Co), g, dev).to(dt))
    T = rows_T(N, H, dev) if route.startswith("rows") else T_TILE
    has_add = epi in ("add", "relu_act", "relu_bits_add", "relu2", "ds")
    if epi == "ds":
        has_add = False
    addend = with_tail(randn((N, H, W, C), g, dev).to(dt)) if has_add else None
    yb = with_tail((randn((N, H, W, C), g, dev) * 1.5 + 0.2).to(dt))   # BN input the sums run against
    mu, ist = randn((C,), g, dev, 0.1), torch.rand(C, generator=g, device=dev) + 0.5
    mask = None
    kw = {}
    if epi == "bn":
        sc, sh = randn((C,), g, dev), randn((C,), g, dev, 0.3)
        mask = (yb.double() * sc.double() + sh.double()) > 0
    elif epi != "none" and epi != "add":
        act = with_tail(randn((N, H, W, C), g, dev).to(dt))
        mask = act > 0
    if epi == "relu2":
        yd = with_tail(randn((N, H, W, C), g, dev).to(dt))
        mud, isd = randn((C,), g, dev, 0.1), torch.rand(C, generator=g, device=dev) + 0.5
    if epi == "ds":
        wd = randn((Co, 1, 1, C), g, dev, Co ** -0.5).to(dt)
        both = torch.cat([wt.flatten(), wd.permute(3, 1, 2, 0).flatten()])
        wt, wtd = both[:wt.numel()].view(wt.shape), both[wt.numel():].view(C, 1, 1, Co)
        pair = with_tail(torch.stack([dy, randn((N, Ho, Wo, Co), g, dev).to(dt)]))
        dy, dyd = pair[0], pair[1]
    if fused:   # rows XF = 2: dy = k * g_in + (b * y_in + c), formed in the ring and written to dy_out
        g_in = dy
        y_in = with_tail((randn((N, H, W, Co), g, dev) * 2 + 0.3).to(dt))
        coef = torch.cat([randn((Co,), g, dev), randn((Co,), g, dev, 0.3), randn((Co,), g, dev, 0.5)])
        kc, bc, cc = (coef[i * Co:(i + 1) * Co].double() for i in range(3))
        # bn_bwd_dy is fmaf(k, g, fmaf(b, y, c)): the inner fmaf's fp32 rounding is followed, since
        # where k * g cancels it, that rounding exceeds a bf16 ulp of the (tiny) result
        dy = (kc * g_in.double() + (bc * y_in.double() + cc).float().double()).float().to(dt)
    obuf, out = guarded((N, H, W, C), dt, dev)
    s1, s2, s3 = (stat_buf(rep, C, dev) for _ in range(3))

    if emulate:
        v = dgrad64(dy.float(), w.float(), H, W, S, P)
        if epi == "ds":
            v = v + dgrad64(dyd.float(), wd.float(), H, W, 2, 0)
        if dt == BF16:
            v = v.to(BF16).float()
        if addend is not None:
            v = v + addend.float()
        if mask is not None:
            v = torch.where(mask, v, torch.zeros_like(v))
        out.copy_(v.to(dt))
        xh = (yb.float() - mu) * ist
        if mask is not None:
            s1[:C] = emu_sum(v, T)
            s2[:C] = emu_sum(v * xh, T)
        if epi == "relu2":
            s3[:C] = emu_sum(v * ((yd.float() - mud) * isd), T)
    else:
        a = (dy, wt, H, W, C, KH, KH, S, P)
        bits = pack_bits(mask) if epi in ("relu_bits", "relu_bits_add", "relu2") else None
        if fused:
            dbuf, dy_dev = guarded((N, Ho, Wo, Co), dt, dev)
            assert ops.conv_dgrad_act_ok(g_in, C, KH, KH, S, P)
            fa = (g_in, y_in, coef, dy_dev, wt, H, W, C, KH, KH, S, P)
            if epi == "bn":
                ops.conv_dgrad_bn_act(*fa, yb, (sc, sh, mu, ist), s1, s2, stat_rep=rep, out=out)
            else:
                ops.conv_dgrad_relu_act(*fa, bits if bits is not None else act, yb, mu, ist, s1, s2,
                                        addend=addend, stat_rep=rep, out=out)
            torch.cuda.synchronize()
            assert_guard(name + " dy_out", dbuf, N * Ho * Wo)
            ulp_gate(name + " dy_out", dy_dev, dy, dt)
            dy = dy_dev
        elif epi in ("none", "add"):
            ops.conv_dgrad(*a, addend=addend, out=out)
        elif epi == "bn":
            ops.conv_dgrad(*a, y_bn=yb, bn=(sc, sh, mu, ist), stat1=s1, stat2=s2, out=out, stat_rep=rep)
        elif epi == "relu2":
            ops.conv_dgrad_relu2(*a, bits, yb, mu, ist, yd, mud, isd, s1, s2, s3, addend=addend, stat_rep=rep, out=out)
        elif epi == "ds":
            ops.conv_dgrad_relu_ds(dy, dyd, wt, wtd, H, W, C, KH, KH, S, P, act, yb, mu, ist, s1, s2,
                                   stat_rep=rep, out=out)
        else:
            ops.conv_dgrad_relu(*a, bits if bits is not None else act, yb, mu, ist, s1, s2, addend=addend,
                                stat_rep=rep, out=out)
        torch.cuda.synchronize()

    dy64, w64 = dy.double(), w.double()
    g64 = dgrad64(dy64, w64, H, W, S, P)
    Sabs = dgrad64(dy64.abs(), w64.abs(), H, W, S, P)
    if epi == "ds":
        g64 = g64 + dgrad64(dyd.double(), wd.double(), H, W, 2, 0)
        Sabs = Sabs + dgrad64(dyd.double().abs(), wd.double().abs(), H, W, 2, 0)
        K = K + Co
    nz = noise_term(dt, Sabs, K)
    flip = torch.zeros_like(g64)
    if dt == BF16:   # every bf16 data-gradient route runs a row-chunk epilogue on bf16(acc)
        g64, flip = staged(g64, nz)
    if addend is not None:
        g64 = g64 + addend.double()
        Sabs = Sabs + addend.double().abs()
    if mask is not None:
        g64 = torch.where(mask, g64, torch.zeros_like(g64))
        leaked = int((out[~mask] != 0).sum().item())
        print(f"{name}: {leaked} non-zero outputs where the reference mask is 0 (of {int((~mask).sum().item())})")
        assert leaked == 0
    check(name, out, g64, elem_bound(dt, g64, Sabs, K) + flip, tol(dt), "element " + dtid(dt))
    assert_guard(name, obuf, M)
    if epi in ("none", "add"):
        for s in (s1, s2, s3):
            assert bool((s[:rep * C] == 0).all().item())
        return
    nz = (nz + flip) * mask.double()
    xh = (yb.double() - mu.double()) * ist.double()
    check_sum(name + " stat1", stat_total(name, s1, rep, C), g64.sum((0, 1, 2)), sum_bound(nz, g64, T))
    check_sum(name + " stat2", stat_total(name, s2, rep, C), (g64 * xh).sum((0, 1, 2)),
              sum_bound(nz * xh.abs(), g64 * xh, T))
    if epi == "relu2":
        xd = (yd.double() - mud.double()) * isd.double()
        check_sum(name + " stat3", stat_total(name, s3, rep, C), (g64 * xd).sum((0, 1, 2)),
                  sum_bound(nz * xd.abs(), g64 * xd, T))


DG = dgrad_cases()


@gpu
@pytest.mark.parametrize("case,epi", DG, ids=[cid(c) + "-" + e for c, e in DG])
def test_conv_dgrad_routes(ops, case, epi):
    run_dgrad(ops, case, epi, BF16, "cuda", rep=4 if DG.index((case, epi)) % 2 == 0 else 1)


@gpu
@pytest.mark.parametrize("case", [(2, 12, 12, 64, 128, 3, 2, "big256x64-fold"), (3, 13, 13, 128, 256, 3, 2, "big128x128-fold"),
                                  (6, 13, 13, 256, 256, 3, 2, "pp256-fold"), (2, 12, 14, 64, 128, 3, 2, "big256x64-fold-H12xW14")],
                         ids=cid)
def test_conv_dgrad_relu_ds_fold(ops, case):
    """vlp_conv_dgrad_relu_ds against the fp64 SUM of both data gradients (the fold adds
    them in fp32 inside one GEMM: one rounding on store, reduction depth K + Co)."""
    run_dgrad(ops, case, "ds", BF16, "cuda", rep=4)


@gpu
@pytest.mark.parametrize("epi", ["none", "add", "bn", "relu_act"])
@pytest.mark.parametrize("case", [(2, 12, 12, 64, 128, 3, 1, "launch_gemm"), (2, 13, 13, 64, 128, 3, 2, "launch_gemm-s2")],
                         ids=cid)
def test_conv_dgrad_fp32(ops, case, epi):
    run_dgrad(ops, case, epi, F32, "cuda", rep=1)


@gpu
@pytest.mark.parametrize("epi", ["bn", "relu_bits_add", "relu_act"])
@pytest.mark.parametrize("N,H", ROWS_SHAPES, ids=["N3-H5", "N2-H3", "images>CUs-H4"])
def test_conv_dgrad_act_rows_xf2(ops, N, H, epi):
    """vlp_conv_dgrad_bn_act / _relu_act (rows kernel, XF = 2) against fp64, not against
    the unfused HIP path; dy_out gated at 1 ulp, the convolution reference built from it."""
    run_dgrad(ops, (N, H, 128, 64, 64, 3, 1, "rows_c64-XF2"), epi, BF16, "cuda", rep=4, fused=True)


@gpu
@pytest.mark.parametrize("N,H,epi", [(2, 3, "bn"), (-3, 4, "relu_bits_add"), (-3, 4, "none")],
                         ids=["N2-H3-bn", "images>CUs-H4-relu_bits_add", "images>CUs-H4-none"])
def test_conv_dgrad_rows_more_shapes(ops, N, H, epi):
    """The plain rows data gradient at the minimum H and with several images per workgroup."""
    run_dgrad(ops, (N, H, 128, 64, 64, 3, 1, "rows_c64-flip"), epi, BF16, "cuda", rep=4)


# ---------------------------------------------------------------- weight gradient
# (N, H, W, C, Co, KH, S, route, slabs): slabs = workspace size in slabs
WGRAD_CASES = [
    (3, 5, 128, 64, 64, 3, 1, "rows", 64),
    (4, 1, 128, 64, 64, 3, 1, "rows-H1", 64),
    (5, 4, 128, 64, 64, 3, 1, "rows-3slabs-5images", 3),
    (2, 12, 12, 64, 64, 3, 1, "big64x192", 64),
    (2, 13, 13, 128, 64, 1, 2, "bk64x128-1x1s2", 64),
    (4, 8, 8, 128, 128, 3, 1, "pp128x384", 64),
    (4, 8, 8, 256, 256, 3, 1, "pp256-MNxMN", 64),
    (2, 13, 13, 64, 128, 3, 2, "big128x256-3x3s2", 64),
    (16, 32, 32, 128, 128, 3, 1, "pp128x384-tight3", 3),
    (2, 8, 8, 576, 128, 3, 1, "big128x256-fold-per-element-C576", 64),
]


def wgrad_inputs(case, dt, dev, seed=7):
    N, H, W, C, Co, KH, S = case[:7]
    P = 1 if KH == 3 else 0
    Ho, Wo = out_hw(H, W, KH, S, P)
    g = gen_for(dev, seed)
    x = with_tail(randn((N, H, W, C), g, dev).to(dt))
    dy = with_tail(randn((N, Ho, Wo, Co), g, dev).to(dt))
    return x, dy, P


def wgrad_gate(name, grad, dy, x, KH, S, P, dt):
    """grad [Co][C][KH][KW] (+ guard rows) against fp64."""
    Co = dy.shape[-1]
    ref = wgrad64(dy.double(), x.double(), KH, S, P).permute(0, 3, 1, 2)
    bound = (C_ACC * EPS32) * wgrad64(dy.double().abs(), x.double().abs(), KH, S, P).permute(0, 3, 1, 2)
    check(name, grad[:Co], ref, bound, tol(dt) / 4, "weight gradient")
    assert bool((grad[Co:] == SENT).all().item()), f"{name}: rows beyond Co written"


def grad_out(Co, C, KH, dev):
    g = torch.full((Co + 8, C, KH, KH), float("nan"), device=dev)
    g[Co:] = SENT
    return g


def run_wgrad_ws(case, dt, offset_fold=False):
    from vlp_amd._lib import lib
    N, H, W, C, Co, KH, S, route, slabs = case
    x, dy, P = wgrad_inputs(case, dt, "cuda")
    name = f"wgrad {N}x{H}x{W}x{C}->{Co} {KH}x{KH}/{S} {route} {dtid(dt)}"
    slab = Co * KH * KH * C
    nws = slabs * slab
    ws = torch.full((nws + 64,), float("nan"), device="cuda")
    grad = grad_out(Co, C, KH, "cuda")
    st = torch.cuda.current_stream().cuda_stream
    ns = ctypes.c_int(0)
    prev = ctypes.c_int(0)
    lib().vlp_set_wgrad_rows_min_images(1 if route.startswith("rows") else -1, ctypes.addressof(prev))
    try:
        lib().vlp_conv_wgrad_ws(1 if dt == BF16 else 0, dy.data_ptr(), x.data_ptr(), ws.data_ptr(), nws,
                                ctypes.addressof(ns), N, H, W, C, Co, KH, KH, S, P, st)
    finally:
        lib().vlp_set_wgrad_rows_min_images(prev.value, None)
    print(f"{name}: {ns.value} slabs of {slabs} allowed, {N * (dy.shape[1] * dy.shape[2])} pixels")
    assert 1 <= ns.value <= slabs
    if route.startswith("rows"):
        assert ns.value == min(N, slabs), "the rows kernel writes one slab per workgroup"
    src = ws
    if offset_fold:   # the same slabs at a pointer 4 bytes off 16-byte alignment: per-element fold
        shifted = torch.full((nws + 64,), float("nan"), device="cuda")
        shifted[1:1 + ns.value * slab].copy_(ws[:ns.value * slab])
        src = shifted[1:]
        assert src.data_ptr() % 16 == 4
    lib().vlp_conv_wgrad_fold(Co, C, KH, KH, ns.value, src.data_ptr(), grad.data_ptr(), st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nws:]).all().item()), f"{name}: slab writes past the workspace"
    wgrad_gate(name, grad, dy, x, KH, S, P, dt)
    return ns.value


@gpu
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: cid(c[:8]))
def test_conv_wgrad_ws_routes(ops, case):
    ns = run_wgrad_ws(case, BF16)
    if case[7].endswith("tight3"):
        full = run_wgrad_ws(case[:8] + (64,), BF16)
        assert full > 3, "the full split count is expected to need more than three slabs"
        assert ns <= 3


@gpu
def test_conv_wgrad_fold_unaligned_workspace(ops):
    """vlp_conv_wgrad_fold on a workspace pointer 4 bytes off: the per-element kernel."""
    run_wgrad_ws((4, 8, 8, 128, 128, 3, 1, "pp128x384-fold-unaligned", 64), BF16, offset_fold=True)


@gpu
@pytest.mark.parametrize("case", [(2, 12, 12, 64, 64, 3, 1, "atomics", 64), (2, 13, 13, 64, 128, 3, 2, "atomics-s2", 64),
                                  (2, 13, 13, 128, 64, 1, 2, "atomics-1x1s2", 64)], ids=lambda c: cid(c[:8]))
def test_conv_wgrad_ws_fp32_atomics(ops, case):
    """fp32 takes the atomics fallback of conv_wgrad_ws_t: one slab, zeroed by the call."""
    assert run_wgrad_ws(case, F32) == 1


@gpu
@pytest.mark.parametrize("dt", [F32, BF16], ids=dtid)
@pytest.mark.parametrize("case", [(2, 12, 12, 64, 128, 3, 1, "ConvWgradB-xf"), (2, 13, 13, 128, 64, 3, 2, "ConvWgradB-xf-s2")],
                         ids=cid)
def test_conv_wgrad_bn_on_load(ops, case, dt):
    """vlp_conv_wgrad with in_scale / in_shift (ConvWgradB<T, true>): atomics into
    dw_ws [Co][KH][KW][C]; the operand is relu(sc * x + sh) rounded to the storage dtype."""
    N, H, W, C, Co, KH, S, route = case
    x, dy, P = wgrad_inputs(case, dt, "cuda")
    sc, sh = xf_coeffs(C, gen_for("cuda", 9), "cuda")
    a = torch.relu(x.double() * sc.double() + sh.double()).float().to(dt)
    ws = torch.zeros(Co + 8, KH, KH, C, device="cuda")
    ws[Co:] = SENT
    ops.conv_wgrad(dy, x, KH, KH, S, P, ws, sc, sh)
    torch.cuda.synchronize()
    grad = ws.permute(0, 3, 1, 2)
    wgrad_gate(f"wgrad xf {cid(case)} {dtid(dt)}", grad, dy, a, KH, S, P, dt)


# ---------------------------------------------------------------- CPU: the bounds are satisfiable
def test_bound_holds_for_emulated_arithmetic():
    """fp32 accumulation of the rounded inputs, one rounding on store and fp32 partial
    sums of T rows meet every bound with zero violations, for each epilogue; the worst
    ratio per bound family is printed (the figures of the module docstring)."""
    WORST.clear()
    small = lambda c: c[0] * c[1] * c[2] * c[3] * c[4] <= 2 * 16 * 16 * 512 * 512 and c[0] > 0
    for c in [c for c in FWD_CASES if small(c)]:
        run_fwd(None, c, BF16, "cpu", emulate=True)
    for c in FWD_XF_CASES:
        run_fwd(None, c, BF16, "cpu", xf=True, emulate=True)
    for c in FWD_F32_CASES[:3]:
        run_fwd(None, c, F32, "cpu", emulate=True)
    for c, e in DG:
        if small(c) and c[2] != 128:
            run_dgrad(None, c, e, BF16, "cpu", emulate=True)
    for e in EPIS[:-1]:
        run_dgrad(None, DGRAD_S1[0], e, BF16, "cpu", emulate=True)
    run_dgrad(None, (2, 12, 12, 64, 128, 3, 2, "fold"), "ds", BF16, "cpu", emulate=True)
    for e in ("add", "bn", "relu_act"):
        run_dgrad(None, (2, 12, 12, 64, 128, 3, 1, "fp32"), e, F32, "cpu", emulate=True)
    for case in WGRAD_CASES:
        for dt in (BF16, F32):
            N, H, W, C, Co, KH, S = case[:7]
            x, dy, P = wgrad_inputs(case, dt, "cpu")
            grad = grad_out(Co, C, KH, "cpu")
            grad[:Co] = wgrad64(dy.float(), x.float(), KH, S, P).permute(0, 3, 1, 2)
            wgrad_gate(f"emulated wgrad {cid(case[:8])} {dtid(dt)}", grad, dy, x, KH, S, P, dt)
    print("worst emulated |err| / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())


# ---------------------------------------------------------------- argument checks
@gpu
@pytest.mark.parametrize("dt,C,Co", [(BF16, 100, 128), (BF16, 128, 100), (F32, 6, 64)],
                         ids=["bf16-C100", "bf16-Co100", "fp32-C6"])
def test_conv_rejects_partial_channel_chunk(ops, dt, C, Co):
    """A channel count that is no whole number of 16-byte chunks: the loaders resolve
    the filter tap from a chunk's first element (so the chunk would take the next
    pixel's channels) and the epilogues store 4- / 8-column groups.  Forward, data
    gradient (both entry points), and both weight-gradient entry points refuse the
    shape on the host; no output or workspace element is touched."""
    from vlp_amd._lib import lib
    N, H, W = 2, 12, 12
    dev = "cuda"
    g = gen_for(dev, 31)
    x = with_tail(randn((N, H, W, C), g, dev).to(dt))
    dy = with_tail(randn((N, H, W, Co), g, dev).to(dt))
    wp = with_tail(randn((Co, 3, 3, C), g, dev, 0.05).to(dt))
    wt = with_tail(randn((C, 3, 3, Co), g, dev, 0.05).to(dt))
    ybuf, y = guarded((N, H, W, Co), dt, dev)
    dbuf, dx = guarded((N, H, W, C), dt, dev)
    s1, s2 = stat_buf(1, max(C, Co), dev), stat_buf(1, max(C, Co), dev)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError):
        ops.conv_fwd(x, wp, Co, 3, 3, 1, 1, stat_sum=s1, stat_sumsq=s2, out=y)
    with pytest.raises(RuntimeError):
        ops.conv_dgrad(dy, wt, H, W, C, 3, 3, 1, 1, out=dx)
    with pytest.raises(RuntimeError):
        ops.conv_dgrad_relu(dy, wt, H, W, C, 3, 3, 1, 1, x, x, s1, s2, s1, s2, out=dx)
    ws = torch.full((4 * Co * 9 * C + 64,), SENT, device=dev)
    ns = ctypes.c_int(0)
    with pytest.raises(RuntimeError):
        lib().vlp_conv_wgrad_ws(1 if dt == BF16 else 0, dy.data_ptr(), x.data_ptr(), ws.data_ptr(), 4 * Co * 9 * C,
                                ctypes.addressof(ns), N, H, W, C, Co, 3, 3, 1, 1, st)
    with pytest.raises(RuntimeError):
        ops.conv_wgrad(dy, x, 3, 3, 1, 1, ws)
    torch.cuda.synchronize()
    assert bool((ybuf == SENT).all().item()) and bool((dbuf == SENT).all().item()) and bool((ws == SENT).all().item())
    assert bool((s1[:max(C, Co)] == 0).all().item()) and bool((s2[:max(C, Co)] == 0).all().item())
