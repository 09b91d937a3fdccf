"""Every route and fused epilogue of the linear GEMM family against fp64.

`gemm_lin` (csrc/bert_ops.hip) sends vlp_linear_fwd / _fwd_rs / _dgrad to one of six
kernels by M, N and K thresholds, and vlp_linear_wgrad_ws picks among three.  The
cases below name, in their ids, the kernel the bf16 call takes at GEMM variant 5;
fp32 always lands on launch_gemm<float, ...>.

Reference.  Inputs are rounded to the storage dtype first (w ~ K^-0.5, bias and
residual of order 1; large operands are generated on the device).  The reference is
torch fp64 on those rounded inputs.  For bf16 it follows the rounding points EpiLinear
documents: acc + bias is staged once as bf16, the epilogue then runs in fp32 and
rounds once on store, so v = bf16(acc64 + bias) and the epilogue is applied to v in
fp64.  The data gradient stages bf16(acc64) the same way.

Gate.  Each case asserts the suite's rel-L2 bound (tol/2 forward and data gradient,
tol/4 weight gradient) AND a per-element bound with zero violations allowed: at
M = 65600 a 128-row tile that is 10 % off moves rel-L2 by only 4e-3.

Per-element bound, bf16 (derived, not tuned; `elem_bound`):
    2 * ( 2^-9 |ref|  +  L * 2^-8 |v|  +  L * C_ACC * eps32 * S )
  * 2^-9 |ref|: the one bf16 rounding on store, a half-ulp (2^-9 relative at the top
    of a binade, 2^-8 at the bottom: the factor 2 in front covers the bottom).
  * L * 2^-8 |v|: fp32 accumulation noise can put acc + bias on the other side of a
    bf16 rounding boundary than acc64 + bias, so the staged v differs by one ulp
    (2^-8 .. 2^-7 relative, again covered by the factor 2), carried through the
    epilogue's Lipschitz constant L: 1 for mode 0 / addend, sup |gelu'| = 1.129 -> 1.13
    for the GELU modes (a constant, so the formula error of the device GELU at
    gelu' ~ 0 stays covered), |rscale[row]| / (1 - p) for mode 2.  The M <= 1024 kernel
    does not stage (one rounding of the fp32 value): its v is within a half-ulp of the
    reference v, inside the same term.
  * S = |x| @ |w|^T + |b|, C_ACC = 64: fp32 accumulation noise.  The worst case is
    K * u * S with u = eps32 / 2; a random-walk estimate is sqrt(K) * u * S.  64 * eps32
    = 128 u is the random-walk figure at K = 16384 (the deepest forward K here is
    1536: sqrt = 39) and far below the worst case (1536 u), so the term is a real
    constraint while still above what correct arithmetic produces.
  * the leading 2 is the only margin.
  fp32: C_F32 * K * eps32 * S * max(L, 1) with C_F32 = 1, twice the worst-case bound
  gamma_K = K u of an fp32 dot product of depth K (no rounding of v, no store rounding
  beyond eps32).
  Weight gradient (fp32 output in both storage modes): C_ACC * eps32 * (|dy|^T @ |x|).
  The reduction depth is M / splits <= 4096 rows per fp32 slab, then a short fold.
`test_bound_holds_for_emulated_arithmetic` shows on the CPU that correct arithmetic
(fp32 matmul of the bf16 inputs, rounding at the same two points) meets the bound for
every mode with zero violations; the bound is per element, so it does not depend on M.

Untouched memory.  Every output has 256 guard rows beyond M and, where ld > N, padding
columns; both hold a sentinel that must survive.

GELU (tests 5).  A&S 7.1.26 evaluated in fp32 numpy on the CPU against fp64
x Phi(x) and Phi(x) + x phi(x) over the test grid gives max |error| 3.30e-7 (forward)
and 2.92e-7 (gradient); these are recomputed by the test, and the device (1-ulp rcp and
exp against numpy's correctly rounded ones) is gated at twice them.  Device maxima
measured on an MI355X by `test_gelu_accuracy_isolated`: 3.30e-7 (forward, 3.302e-7
before rounding) and 2.39e-7 (gradient).  The kernel's comment quoted 3.3e-7; it now
says 3.4e-7.

Argument checks (tests 6).  KMat::load and the buffer-protocol loaders zero-fill at
16-byte-chunk granularity (a chunk is dropped only when its first element is outside
[M) x [K)), so K = 100 in bf16 with ld = K summed the next row's first four elements
into every output and returned success.  The entry points now refuse a K or a leading
dimension that is no multiple of the chunk (8 bf16 / 4 fp32); the tests pin "matches
fp64 or raises".
"""
import ctypes
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DT = [F32, BF16]
EPS32 = 2.0 ** -23
C_ACC = 64.0
C_F32 = 1.0
L_GELU = 1.13
GUARD = 256
SENT = -1024.0


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


# ---------------------------------------------------------------- reference and gate
def staged(acc64, dt):
    """acc (+ bias) as the kernel holds it before the epilogue."""
    return acc64.to(BF16).double() if dt == BF16 else acc64


def elem_bound(dt, ref, v, L, S, K):
    """Per-element bound of the module docstring.  L: scalar or broadcastable tensor."""
    if dt == BF16:
        return 2.0 * (2.0 ** -9 * ref.abs() + L * (2.0 ** -8) * v.abs() + L * (C_ACC * EPS32) * S)
    Lm = L.clamp(min=1.0) if torch.is_tensor(L) else max(L, 1.0)
    return (C_F32 * K * EPS32) * S * Lm


def gelu64(x):
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _as_tail32(x):
    """A&S 7.1.26 in fp32 numpy: (1 - erf(|x| / sqrt 2)) and exp(-x^2 / 2)."""
    f = np.float32
    ax = np.abs(x)
    t = f(1.0) / (f(0.3275911 / math.sqrt(2.0)) * ax + f(1.0))
    P = t * f(1.061405429) + f(-1.453152027)
    P = t * P + f(1.421413741)
    P = t * P + f(-0.284496736)
    P = t * P + f(0.254829592)
    P = P * t
    e = np.exp(f(-0.5) * x * x)
    return P * e, e


def gelu_as32(x):
    """GELU(erf) through A&S 7.1.26, all in fp32 (numpy array in, numpy array out)."""
    x = x.astype(np.float32)
    tail, _ = _as_tail32(x)
    q = np.float32(0.5) * x * tail
    return np.where(x >= 0, x - q, q).astype(np.float32)


def gelu_grad_as32(x):
    x = x.astype(np.float32)
    tail, e = _as_tail32(x)
    h = np.float32(0.5) * tail
    cdf = np.where(x >= 0, np.float32(1.0) - h, h)
    return (x * np.float32(0.3989422804014327) * e + cdf).astype(np.float32)


def check(name, y, ref, bound, rel_tol):
    """rel-L2 and per-element gate; prints the figures before asserting."""
    y = y.double()
    d = (y - ref).abs()
    r = (torch.linalg.vector_norm(y - ref) / (torch.linalg.vector_norm(ref) + 1e-30)).item()
    nviol = int((~(d <= bound)).sum().item())   # NaN counts as a violation
    worst = (d / (bound + 1e-300)).max().item()
    print(f"{name}: rel-L2 {r:.3e} (gate {rel_tol:.1e}), per-element worst |err|/bound {worst:.3f}, "
          f"violations {nviol} of {ref.numel()}")
    assert r < rel_tol, f"{name}: rel-L2 {r:.3e} >= {rel_tol:.1e}"
    assert nviol == 0, f"{name}: {nviol} elements beyond the per-element bound (worst ratio {worst:.2f})"


def guarded(M, N, ld, dt, dev):
    return torch.full((M + GUARD, ld), SENT, dtype=dt, device=dev)


def assert_guard(name, buf, M, N):
    assert bool((buf[M:] == SENT).all().item()), f"{name}: rows beyond M written"
    if buf.shape[1] > N:
        assert bool((buf[:M, N:] == SENT).all().item()), f"{name}: padding columns written"


def randn(shape, gen, dev, scale=1.0):
    return torch.randn(shape, generator=gen, device=dev) * scale


def gen_for(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


RS_CYCLE = [0.0, 2.0, 1.25, 1.0, 0.5, 1.0 / 0.9, 0.0, 1.5, 1.0, 2.0, 0.75]


def fwd_inputs(M, N, K, dt, dev, seed, ldx=None, ldr=None):
    """x [M, ldx] (logical [:, :K]), w [N, K], b [N], res [M, ldr] in storage dtype."""
    g = gen_for(dev, seed)
    x = randn((M, ldx or K), g, dev).to(dt)
    w = randn((N, K), g, dev, K ** -0.5).to(dt)
    b = randn((N,), g, dev)
    res = randn((M, ldr or N), g, dev).to(dt)
    return x, w, b, res


def fwd_reference(x, w, b, dt, K):
    x64, w64 = x[:, :K].double(), w.double()
    acc = x64 @ w64.t() + b.double()
    S = x64.abs() @ w64.abs().t() + b.double().abs()
    return staged(acc, dt), S


# (M, N, K, epilogue, route); epilogue: m0, m1, m2 (p = 0), m2p (p = 0.1), rs (linear_fwd_rs)
FWD_CASES = [
    (1536, 64, 312, "m0", "narrow-bk256x64"),
    (1536, 48, 312, "m0", "narrow-bk256x64-partialN"),
    (1100, 936, 312, "m0", "ring128"),
    (1100, 1200, 312, "m1", "ring128"),
    (1100, 312, 1200, "m2p", "ring128"),
    (1100, 1152, 384, "m0", "pp256-partialMN"),
    (1100, 1536, 384, "m1", "pp256"),
    (1100, 384, 1536, "m2", "pp256"),
    (1100, 384, 1536, "rs100", "pp256"),
    (65600, 96, 48, "m0", "big128-shortK"),
    (65600, 96, 96, "rs16400", "big128-Ktail"),
    (65600, 96, 384, "m2", "big128"),
    (65600, 192, 192, "m2", "big128-partialN"),
    (65600, 576, 192, "m0", "pp256-partialN"),
    (65600, 768, 192, "m1", "pp256"),
    (65600, 384, 96, "m1", "ring128-largeM"),
]


def run_fwd(ops, M, N, K, epi, dt, dev, seed=11, ldx=None, ldy=None, ldr=None, emulate=None):
    """One forward case on the device (or through `emulate` on the CPU): returns nothing,
    asserts the gate, the aux gate (mode 1), the dropout properties (m2p) and the guards."""
    name = f"fwd {M}x{N}x{K} {epi} {dtid(dt)}"
    x, w, b, res = fwd_inputs(M, N, K, dt, dev, seed, ldx, ldr)
    v, S = fwd_reference(x, w, b, dt, K)
    res64 = res[:, :N].double()
    y = guarded(M, N, ldy or N, dt, dev)
    aux = guarded(M, N, ldy or N, dt, dev) if epi == "m1" else None
    p, rs_row = 0.0, None
    if epi.startswith("rs"):
        rps = int(epi[2:])
        ng = (M + rps - 1) // rps
        rscale = torch.tensor([RS_CYCLE[i % len(RS_CYCLE)] for i in range(ng)], dtype=F32, device=dev)
        rs_row = rscale.double().repeat_interleave(rps)[:M, None]
    if epi == "m2p":
        p = 0.1

    if emulate is not None:
        emulate(x[:, :K], w, b, res[:, :N], y, aux, epi, p, rs_row)
    elif epi.startswith("rs"):
        assert ldx is None and ldy is None and ldr is None
        ops.linear_fwd_rs(x, w, b, y, res, rscale, rps, M, N, K)
    else:
        mode = {"m0": 0, "m1": 1, "m2": 2, "m2p": 2}[epi]
        ops.linear_fwd(x, w, b, y, M, N, K, ldx=ldx, ldy=ldy, mode=mode, aux=aux,
                       res=res if mode == 2 else None, ldr=ldr, p=p, seed=1234)
    if dev != "cpu":
        torch.cuda.synchronize()
    out = y[:M, :N]

    if epi == "m0":
        check(name, out, v, elem_bound(dt, v, v, 1.0, S, K), tol(dt) / 2)
    elif epi == "m1":
        # aux is the staged pre-activation itself: no second rounding, one possible ulp flip
        ab = 2.0 * ((2.0 ** -8) * v.abs() + C_ACC * EPS32 * S) if dt == BF16 else C_F32 * K * EPS32 * S
        check(name + " aux", aux[:M, :N], v, ab, tol(dt) / 2)
        ref = gelu64(v)
        check(name, out, ref, elem_bound(dt, ref, v, L_GELU, S, K), tol(dt) / 2)
    elif epi == "m2" or epi.startswith("rs"):
        L = rs_row.abs() if rs_row is not None else 1.0
        ref = res64 + (rs_row * v if rs_row is not None else v)
        check(name, out, ref, elem_bound(dt, ref, v, L, S, K), tol(dt) / 2)
    else:   # dropout: every element is res (dropped) or res + v / (1 - p) (kept); mask from the output
        L = 1.0 / (1.0 - p)
        kept_ref = res64 + v * L
        o = out.double()
        kept = (o - kept_ref).abs() < (o - res64).abs()
        ref = torch.where(kept, kept_ref, res64)
        bound = torch.where(kept, elem_bound(dt, kept_ref, v, L, S, K), elem_bound(dt, res64, v, 0.0, S, K))
        check(name, out, ref, bound, tol(dt) / 2)
        # kept fraction, counted where the two candidates are far enough apart to tell
        clear = (v.abs() * L) > 4.0 * elem_bound(dt, kept_ref, v, L, S, K)
        n = int(clear.sum().item())
        frac = (kept & clear).sum().item() / n
        sigma = math.sqrt(p * (1.0 - p) / n)
        print(f"{name}: kept fraction {frac:.5f} over {n} elements (1 - p = {1 - p}, sigma {sigma:.1e})")
        assert abs(frac - (1.0 - p)) < 4.0 * sigma
    assert_guard(name, y, M, N)
    if aux is not None:
        assert_guard(name + " aux", aux, M, N)


@gpu
@pytest.mark.parametrize("dt", DT, ids=dtid)
@pytest.mark.parametrize("M,N,K,epi,route", FWD_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}-{c[4]}" for c in FWD_CASES])
def test_linear_fwd_routes(ops, dt, M, N, K, epi, route):
    run_fwd(ops, M, N, K, epi, dt, "cuda")


@gpu
def test_linear_fwd_leading_dims(ops):
    """mode 2 with ldx = 2 K, ldy = N + 8, ldr = N + 16 (bf16, 128x128 ring)."""
    run_fwd(ops, 1100, 312, 1200, "m2", BF16, "cuda", ldx=2400, ldy=320, ldr=328)


@gpu
def test_dropout_mask_same_across_kernels(ops):
    """The mask depends on (seed, row * N + col) only: M = 1024 (64x256 kernel) and
    M = 1100 (ping-pong kernel) at N = 384, K = 1536 drop the same elements of the
    first 1024 rows."""
    N, K, p, dt = 384, 1536, 0.1, BF16
    x, w, b, res = fwd_inputs(1100, N, K, dt, "cuda", 23)
    v, S = fwd_reference(x, w, b, dt, K)
    kept_ref = res.double() + v / (1.0 - p)
    masks = []
    for M in (1024, 1100):
        y = guarded(M, N, N, dt, "cuda")
        ops.linear_fwd(x[:M].contiguous(), w, b, y, M, N, K, mode=2, res=res[:M].contiguous(), p=p, seed=99)
        torch.cuda.synchronize()
        assert_guard(f"dropout M={M}", y, M, N)
        o = y[:1024].double()
        masks.append((o - kept_ref[:1024]).abs() < (o - res[:1024].double()).abs())
    clear = ((v.abs() / (1.0 - p)) > 4.0 * elem_bound(dt, kept_ref, v, 1.0 / (1.0 - p), S, K))[:1024]
    differ = int(((masks[0] != masks[1]) & clear).sum().item())
    print(f"dropout masks: {differ} differing of {int(clear.sum().item())} decidable elements")
    assert differ == 0


# ---------------------------------------------------------------- data gradient
# (M, Kin, Nout, epilogue, route)
DGRAD_CASES = [
    (1100, 384, 1152, "m0", "pp256-KxMN"),
    (1100, 1536, 384, "m1", "pp256-KxMN"),
    (1100, 384, 1536, "add", "pp256-KxMN"),
    (1100, 312, 936, "add", "ring128"),
    (1100, 1200, 312, "m1", "ring128"),
    (65600, 96, 288, "m0", "ring128-largeM"),
    (65600, 192, 768, "m1", "ring128-largeM"),
]


def run_dgrad(ops, M, Kin, Nout, epi, dt, dev, seed=13, lddx=None, ldad=None, emulate=None):
    name = f"dgrad {M}x{Kin}x{Nout} {epi} {dtid(dt)}"
    g = gen_for(dev, seed)
    dy = randn((M, Nout), g, dev).to(dt)
    w = randn((Nout, Kin), g, dev, Nout ** -0.5).to(dt)
    side = randn((M, ldad or Kin), g, dev).to(dt)   # saved pre-activation (m1) or addend
    dy64, w64 = dy.double(), w.double()
    v = staged(dy64 @ w64, dt)
    S = dy64.abs() @ w64.abs()
    dx = guarded(M, Kin, lddx or Kin, dt, dev)
    if emulate is not None:
        emulate(dy, w, side[:, :Kin], dx, epi)
    elif epi == "m0":
        ops.linear_dgrad(dy, w, dx, M, Kin, Nout, lddx=lddx)
    elif epi == "m1":
        ops.linear_dgrad(dy, w, dx, M, Kin, Nout, lddx=lddx, mode=1, aux=side, ldaux=ldad)
    else:
        ops.linear_dgrad(dy, w, dx, M, Kin, Nout, lddx=lddx, addend=side, ldad=ldad)
    if dev != "cpu":
        torch.cuda.synchronize()
    s64 = side[:, :Kin].double()
    if epi == "m0":
        ref, L = v, 1.0
    elif epi == "m1":
        ref, L = v * gelu_grad64(s64), L_GELU
    else:
        ref, L = v + s64, 1.0
    check(name, dx[:M, :Kin], ref, elem_bound(dt, ref, v, L, S, Nout), tol(dt) / 2)
    assert_guard(name, dx, M, Kin)


@gpu
@pytest.mark.parametrize("dt", DT, ids=dtid)
@pytest.mark.parametrize("M,Kin,Nout,epi,route", DGRAD_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}-{c[4]}" for c in DGRAD_CASES])
def test_linear_dgrad_routes(ops, dt, M, Kin, Nout, epi, route):
    run_dgrad(ops, M, Kin, Nout, epi, dt, "cuda")


@gpu
@pytest.mark.parametrize("dt", DT, ids=dtid)
def test_linear_dgrad_leading_dims(ops, dt):
    """The CLS-only path's layout: lddx = 2 Kin, ldad = Kin + 8."""
    run_dgrad(ops, 1100, 312, 936, "add", dt, "cuda", lddx=624, ldad=320)


# ---------------------------------------------------------------- weight gradient
# (M, Nout, Kin, route)
WGRAD_CASES = [
    (65576, 96, 96, "big128"),
    (65576, 192, 768, "big128"),
    (65576, 288, 96, "big128"),
    (65576, 96, 48, "big128"),
    (16448, 384, 1152, "pp256"),
    (16424, 384, 1152, "ring128-depth16424"),
]


def wgrad_inputs(M, Nout, Kin, dt, dev, seed=17, lddy=None, ldx=None):
    g = gen_for(dev, seed)
    dy = randn((M, lddy or Nout), g, dev).to(dt)
    x = randn((M, ldx or Kin), g, dev).to(dt)
    dy64, x64 = dy[:, :Nout].double(), x[:, :Kin].double()
    ref = dy64.t() @ x64 + 0.5
    bound = (C_ACC * EPS32) * (dy64.abs().t() @ x64.abs())
    return dy, x, ref, bound


def wgrad_out(Nout, Kin, dev):
    dw = torch.full((Nout + 8, Kin), 0.5, device=dev)
    dw[Nout:] = SENT
    return dw


@gpu
@pytest.mark.parametrize("dt", DT, ids=dtid)
@pytest.mark.parametrize("M,Nout,Kin,route", WGRAD_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}" for c in WGRAD_CASES])
def test_linear_wgrad_routes(ops, dt, M, Nout, Kin, route):
    dy, x, ref, bound = wgrad_inputs(M, Nout, Kin, dt, "cuda")
    dw = wgrad_out(Nout, Kin, "cuda")
    ops.linear_wgrad(dy, x, dw, M, Nout, Kin)
    torch.cuda.synchronize()
    check(f"wgrad {M}x{Nout}x{Kin} {dtid(dt)}", dw[:Nout], ref, bound, tol(dt) / 4)
    assert bool((dw[Nout:] == SENT).all().item())


@gpu
@pytest.mark.parametrize("M,Nout,Kin,route", [(65576, 192, 768, "big128"), (16448, 384, 1152, "pp256")],
                         ids=["big128", "pp256"])
def test_linear_wgrad_tight_workspace(ops, M, Nout, Kin, route):
    """vlp_linear_wgrad_ws with room for only two slabs: the split count must shrink to
    fit and nothing may land past the workspace."""
    from vlp_amd._lib import lib
    dy, x, ref, bound = wgrad_inputs(M, Nout, Kin, BF16, "cuda")
    dw = wgrad_out(Nout, Kin, "cuda")
    n = ctypes.c_longlong(0)
    lib().vlp_linear_wgrad_ws_floats(M, Nout, Kin, ctypes.byref(n))
    nws = 2 * Nout * Kin
    assert n.value > nws, "the full split count is expected to need more than two slabs"
    ws = torch.full((nws + 64,), float("nan"), device="cuda")
    lib().vlp_linear_wgrad_ws(1, M, Nout, Kin, dy.data_ptr(), Nout, x.data_ptr(), Kin, dw.data_ptr(),
                              ws.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nws:]).all().item()), "slab writes past the workspace"
    check(f"wgrad tight {M}x{Nout}x{Kin}", dw[:Nout], ref, bound, tol(BF16) / 4)
    assert bool((dw[Nout:] == SENT).all().item())


@gpu
@pytest.mark.parametrize("dt", DT, ids=dtid)
def test_linear_wgrad_leading_dims(ops, dt):
    M, Nout, Kin = 65576, 96, 96
    dy, x, ref, bound = wgrad_inputs(M, Nout, Kin, dt, "cuda", lddy=Nout + 8, ldx=2 * Kin)
    dw = wgrad_out(Nout, Kin, "cuda")
    ops.linear_wgrad(dy, x, dw, M, Nout, Kin, lddy=Nout + 8, ldx=2 * Kin)
    torch.cuda.synchronize()
    check(f"wgrad strided {dtid(dt)}", dw[:Nout], ref, bound, tol(dt) / 4)
    assert bool((dw[Nout:] == SENT).all().item())


# ---------------------------------------------------------------- CPU: the bound is satisfiable
def _emu_fwd(x, w, b, res, y, aux, epi, p, rs_row):
    """The bf16 kernels' arithmetic in torch: fp32 matmul of the bf16 inputs, acc + bias
    staged as bf16, fp32 epilogue, one bf16 rounding on store."""
    M, N = res.shape
    v = (x.float() @ w.float().t() + b).to(BF16).float()
    if epi == "m0":
        o = v
    elif epi == "m1":
        aux[:M, :N] = v.to(BF16)
        o = torch.from_numpy(gelu_as32(v.numpy()))
    elif epi == "m2p":
        keep = torch.rand(M, N, generator=torch.Generator().manual_seed(3)) >= p
        o = v * keep.float() * (1.0 / (1.0 - p)) + res.float()
    else:
        o = (v * rs_row.float() if rs_row is not None else v) + res.float()
    y[:M, :N] = o.to(BF16)


def _emu_dgrad(dy, w, side, dx, epi):
    M, Kin = side.shape
    v = (dy.float() @ w.float()).to(BF16).float()
    if epi == "m1":
        o = v * torch.from_numpy(gelu_grad_as32(side.float().numpy()))
    elif epi == "add":
        o = v + side.float()
    else:
        o = v
    dx[:M, :Kin] = o.to(BF16)


def test_bound_holds_for_emulated_arithmetic():
    """Correct arithmetic alone meets the per-element bound: every forward and
    data-gradient case's (N, K, epilogue) at M = 2048 and every weight-gradient
    (Nout, Kin) at depth 2048, emulated on the CPU, with zero violations."""
    M = 2048
    for N, K, epi in sorted({(c[1], c[2], c[3]) for c in FWD_CASES}):
        if epi.startswith("rs"):
            epi = "rs512"
        run_fwd(None, M, N, K, epi, BF16, "cpu", emulate=_emu_fwd)
    for Kin, Nout, epi in sorted({(c[1], c[2], c[3]) for c in DGRAD_CASES}):
        run_dgrad(None, M, Kin, Nout, epi, BF16, "cpu", emulate=_emu_dgrad)
    for Nout, Kin in sorted({(c[1], c[2]) for c in WGRAD_CASES}):
        dy, x, ref, bound = wgrad_inputs(M, Nout, Kin, BF16, "cpu")
        dw = dy.float().t() @ x.float() + 0.5
        check(f"emulated wgrad {Nout}x{Kin}", dw, ref, bound, tol(BF16) / 4)


# ---------------------------------------------------------------- GELU, isolated from the GEMM
def gelu_grid():
    """[1024, 128] fp32: a grid over [-12, 12] and the special values."""
    tiny = float(np.finfo(np.float32).tiny)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-6, -1e-6, tiny, -tiny, 12.0, -12.0], dtype=F32)
    grid = torch.linspace(-12.0, 12.0, 1024 * 128 - special.numel(), dtype=torch.float64).float()
    return torch.cat([special, grid]).view(1024, 128), special.numel()


def gelu_cpu_figures(x):
    """max |error| of the fp32 A&S 7.1.26 evaluation against fp64, forward and gradient."""
    x64 = x.double()
    f = np.abs(gelu_as32(x.numpy()).astype(np.float64) - gelu64(x64).numpy()).max()
    g = np.abs(gelu_grad_as32(x.numpy()).astype(np.float64) - gelu_grad64(x64).numpy()).max()
    return float(f), float(g)


def test_gelu_formula_error_cpu():
    """The formula's own error in fp32 (the figures of the module docstring)."""
    x, _ = gelu_grid()
    f, g = gelu_cpu_figures(x.flatten())
    print(f"A&S 7.1.26 in fp32 on the CPU: forward max |err| {f:.3e}, gradient {g:.3e}")
    assert f < 5e-7 and g < 5e-7


@gpu
def test_gelu_accuracy_isolated(ops):
    """gelu_erf and gelu_erf_grad as the device computes them: fp32, W = I (N = K = 128),
    no bias, so every output has one non-zero product and aux == x exactly.

    CPU figures (fp32 numpy evaluation of the same polynomial vs fp64, recomputed here):
    forward 3.30e-7, gradient 2.92e-7; the device is gated at twice them.
    Device maxima measured on an MI355X: forward 3.302e-7, gradient 2.387e-7."""
    x, nspecial = gelu_grid()
    cf, cg = gelu_cpu_figures(x.flatten())
    M, N = x.shape
    xd = x.cuda()
    eye = torch.eye(N, device="cuda")
    out, aux = guarded(M, N, N, F32, "cuda"), guarded(M, N, N, F32, "cuda")
    ops.linear_fwd(xd, eye, None, out, M, N, N, mode=1, aux=aux)
    dx = guarded(M, N, N, F32, "cuda")
    ops.linear_dgrad(torch.ones(M, N, device="cuda"), eye, dx, M, N, N, mode=1, aux=xd)
    torch.cuda.synchronize()
    for nm, b in (("out", out), ("aux", aux), ("dx", dx)):
        assert_guard("gelu " + nm, b, M, N)
    assert torch.equal(aux[:M], xd), "aux must be x exactly"
    o, gr = out[:M].double().cpu(), dx[:M].double().cpu()
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(gr).all())
    x64 = x.double()
    ef = (o - gelu64(x64)).abs().max().item()
    eg = (gr - gelu_grad64(x64)).abs().max().item()
    print(f"gelu_erf on the device: max |err| {ef:.3e} (CPU formula {cf:.3e}); "
          f"gelu_erf_grad {eg:.3e} (CPU formula {cg:.3e})")
    assert ef <= 2.0 * cf
    assert eg <= 2.0 * cg
    flat = o.flatten()
    assert flat[0].item() == 0.0 and flat[1].item() == 0.0, "gelu(+-0) must be zero"
    neg = x64.flatten() <= -11.0
    assert bool((flat[neg].abs() <= 1e-30 + 2.0 * cf).all())


# ---------------------------------------------------------------- argument checks
def _or_raises(call, verify):
    """The call either raises (the entry point refuses the shape) or matches fp64."""
    try:
        call()
        torch.cuda.synchronize()
    except RuntimeError as e:
        print(f"refused: {e}")
        return
    verify()


@gpu
@pytest.mark.parametrize("dt,K,ldx", [(BF16, 100, 100), (BF16, 96, 100), (F32, 102, 102), (F32, 96, 98)],
                         ids=["bf16-K100", "bf16-ldxK+4", "fp32-K102", "fp32-ldxK+2"])
def test_linear_rejects_partial_k_chunk(ops, dt, K, ldx):
    """A reduction depth or leading dimension that is no multiple of the loaders' 16-byte
    chunk: forward, row-scaled forward and data gradient either match fp64 or raise.
    Every operand has slack behind it, so nothing is read or written out of bounds."""
    M, N, slack = 1100, 128, 4096
    g = gen_for("cuda", 29)

    def padded(rows, ld):
        buf = randn((rows * ld + slack,), g, "cuda").to(dt)
        return buf, buf[:rows * ld].view(rows, ld)

    xb, x = padded(M, ldx)
    wb, w = padded(N, K)
    rb, res = padded(M, N)
    b = randn((N,), g, "cuda")
    v, S = fwd_reference(x, w, b, dt, K)
    y = guarded(M, N, N, dt, "cuda")

    _or_raises(lambda: ops.linear_fwd(x, w, b, y, M, N, K, ldx=ldx),
               lambda: check("fwd odd K", y[:M], v, elem_bound(dt, v, v, 1.0, S, K), tol(dt) / 2))
    assert_guard("fwd odd K", y, M, N)

    from vlp_amd._lib import lib
    y2 = guarded(M, N, N, dt, "cuda")
    rs = torch.ones(11, device="cuda")
    ref = res.double() + v
    _or_raises(lambda: lib().vlp_linear_fwd_rs(ops.dcode(x), M, N, K, x.data_ptr(), ldx, w.data_ptr(), b.data_ptr(),
                                               y2.data_ptr(), N, res.data_ptr(), N, rs.data_ptr(), 100,
                                               torch.cuda.current_stream().cuda_stream),
               lambda: check("fwd_rs odd K", y2[:M], ref, elem_bound(dt, ref, v, 1.0, S, K), tol(dt) / 2))
    assert_guard("fwd_rs odd K", y2, M, N)

    # data gradient: dy [M, Nout = K] with lddy = ldx, W [Nout][Kin = N]
    w2b, w2 = padded(K, N)
    dx = guarded(M, N, N, dt, "cuda")
    v2 = staged(x[:, :K].double() @ w2.double(), dt)
    S2 = x[:, :K].double().abs() @ w2.double().abs()
    _or_raises(lambda: ops.linear_dgrad(x, w2, dx, M, N, K, lddy=ldx),
               lambda: check("dgrad odd Nout", dx[:M], v2, elem_bound(dt, v2, v2, 1.0, S2, K), tol(dt) / 2))
    assert_guard("dgrad odd Nout", dx, M, N)


@gpu
def test_linear_wgrad_ws_rejects_unaligned_rows(ops):
    """vlp_linear_wgrad_ws with ldx = Kin + 4 (token rows of x not 16-byte aligned):
    matches fp64 or raises."""
    from vlp_amd._lib import lib
    M, Nout, Kin = 2048, 128, 96
    dy, x, ref, bound = wgrad_inputs(M, Nout, Kin, BF16, "cuda", ldx=Kin + 4)
    x = torch.cat([x.flatten(), torch.zeros(4096, dtype=BF16, device="cuda")])[:M * (Kin + 4)].view(M, Kin + 4)
    dw = wgrad_out(Nout, Kin, "cuda")
    nws = 16 * Nout * Kin
    ws = torch.zeros(nws + 64, device="cuda")
    _or_raises(lambda: lib().vlp_linear_wgrad_ws(1, M, Nout, Kin, dy.data_ptr(), Nout, x.data_ptr(), Kin + 4,
                                                 dw.data_ptr(), ws.data_ptr(), nws,
                                                 torch.cuda.current_stream().cuda_stream),
               lambda: check("wgrad_ws ldx = Kin + 4", dw[:Nout], ref, bound, tol(BF16) / 4))
    assert bool((dw[Nout:] == SENT).all().item())
