"""Every BatchNorm / streaming-pass route of csrc/bn_ops.hip (and the head and optimizer
passes next to it) per element against fp64.

Routes, as vlp_bn_add_relu / vlp_bn_bwd_apply choose them (ew_form_add_relu,
ew_form_bwd_apply, blk_grid, ew_grid, ew_blocks); the case ids name the kernel taken:
    blk         bn_add_relu_blk_kernel / bn_bwd_apply_blk_kernel <.., NTL = false>: a workgroup
                owns segments of 256 * 4 = 1024 chunks (16 bytes each), blk_grid caps the grid at
                2048 workgroups, so nchunks > 2048 * 1024 makes the segment loop iterate.
                add-ReLU: bf16, no residual, tensor <= 100 MB.  bwd-apply: bf16, no dbc / mask /
                g_out, tensor < 256 MB.
    blk-ntl     the same kernels with non-temporal loads: add-ReLU without residual >= 512 MB,
                with residual >= 256 MB; bwd-apply >= 256 MB.
    strided     bn_add_relu_kernel / bn_bwd_apply_kernel, one chunk per thread per iteration,
                grid = min(ceil(nchunks / 256), 4096) workgroups (ew_grid), so nchunks > 2^20 runs the
                grid-stride loop.  bf16 add-ReLU takes the <U = 1, NT = true> form (non-temporal
                stores; ew_variant() = 4): residual < 256 MB, no residual between 100 and
                512 MB.  Every fp32 call, and every bwd-apply with dbc, mask or g_out.
    reduce      bn_bwd_reduce_kernel: rows_per_iter = 256 / cpr rows per workgroup iteration,
                grid = min(ceil(M / (16 rows_per_iter)), 2048), replica = workgroup % stat_rep.
cpr = C / (8 bf16 | 4 fp32) chunks per row; a thread keeps chunk (thread % cpr), which needs
256 % cpr == 0 -- now checked on the host (last tests).

Reference.  Inputs are rounded to the storage dtype first (hyper-parameters to fp32).  The
reference is plain fp64 torch of the defining formula, on the CPU for small cases and on the
device in row slices of at most 2^24 elements for the large ones.  Per-channel coefficients
carry a factor 1 + c / C and alternate in sign, so a chunk mapped to a wrong channel group
fails by orders of magnitude.  test 1 shows the formulas equal torch's own fp64 BatchNorm
backward, F.normalize autograd and torch.optim.AdamW.

Rounding points, read from the kernels (u = 2^-24, eps32 = 2 u):
    add-ReLU     b' = sh + shd (1), t = fma(idt, scd, b') (1), fma(y, sc, t) (1), max, store.
                 <= 3 u S, S = |y||sc| + |idt||scd| + |sh| + |shd|          -> C_EW = 2 (4 u)
    bwd coef     k = gamma istd (1); mg = f32(sum) * f32(1 / count) (3); t = (k istd) mgx
                 (1 + 1 + 3 + 1 = 6), b = -t; c = -(k mg) + t mean: terms 5 and 7, add 1.
                 k: 1, b: 6, c: 8 roundings of S_c = |k mg| + |t mean|
    bwd apply    fma(k, g, fma(b, y, c)): k g 1 + 1, b y 6 + 2, c 8 + 2 -> <= 10 u S,
                 S = |k g| + |b y| + |k mg| + |t mean|                        -> C_APPLY = 6 (12 u)
                 broadcast g = dbc * f32(1 / HW): 2 more on the k g term (4 <= 10); g_out is g
                 rounded once: exact without dbc, 2 roundings with it
    bwd reduce   per row gg * ((y - mean) * istd): 3 roundings (5 with dbc), summed in fp32 over
                 the T = rows_per_iter * ceil(M / (grid rows_per_iter)) rows of a workgroup
                 (thread partials, then the LDS fold), ONE fp64 atomic per workgroup
    finalize     fp64 mean / var; invstd f32 (1); scale = gamma invstd (2); shift = beta -
                 f32(mean) scale: product 4, subtraction 1 -> 5 of S = |beta| + |mean scale|;
                 running = (1 - mom) r + mom f32(x): 4 of S = |(1 - mom) r| + |mom x|.  The fp64
                 cancellation of var enters as (4 + 2 rep) 2^-52 (E x^2 + mean^2) / (var + eps)
    eval coeffs  rv + eps (1), sqrtf (2: one ulp), 1 / (2): invstd 5; scale 6; shift
                 = beta - (rm gamma) invstd: 7 + 1 = 8 of S = |beta| + |rm gamma invstd|
    l2norm       lane sum of L = ceil(E / 64) squares, 6 shuffle levels, sqrt, divide:
                 norm (L + 7) / 2 + 2, y two more.  Backward: dot (L + 7), y dot, subtraction,
                 divide (2), gscale -> (L + 12) of S = (|g| + |y| sum |y dy|) gscale / n
    adamw        m: 1 - b1, g - m, fma -> 3 of S_m = (1 - b1)(|g| + |m|) + |m|
                 v: v b2 (1), ((1 - b2) g) g (3), add (1) -> 5 of v (all terms >= 0)
                 p: p (1 - lr wd) 3; sqrt(v) 2.5 + 2, / bc2 2, bc2's own rounding 1, + eps 1 =
                 8.5 on the denominator, m / denom 2, step_size 1 + 1, m itself 3 -> 15.5 of
                 step S_m / denom; final subtraction 1 -> C_P = 17 of S_p = |p| + step S_m / denom

Gate.  Each case asserts the suite's rel-L2 figure (2e-5 fp32, 1.5e-2 bf16) AND a per-element
bound with zero violations:
    bf16 outputs     2 * (2^-9 |ref| + c eps32 S)     (2^-9 |ref|: the one rounding on store; the
                                                       leading 2 is the only margin)
    fp32 outputs     c eps32 S                         (c eps32 = 2 c u: the same factor 2)
    float results of the statistics kernels: n eps32 |ref| (or S) for n roundings as listed
    ReLU needs no exclusion list: max(., 0) is 1-Lipschitz, |ref| near 0 is inside the bound
    mask bits        equal to (device out > 0) bit for bit
    backward sums    the convolution suite's sum_bound 2 (T + 4) eps32 sum |g f| per replica and
                     for the total (+ workgroups * 2^-52 for the fp64 atomics)
    fp64 folds       rep * 2^-52 * sum |terms|
    vlp_cast         bit-equal to x.to(dtype)
The constants come from the counts above, not from a run.
`test_bound_holds_for_emulated_arithmetic` replays each kernel's fp32 sequence in torch (same
order, fma where the kernel has one, one rounding on store) on the suite's own small inputs.
Worst |err| / bound per family, emulated on the CPU | measured on an MI355X:
    add_relu bf16     0.996 | 0.996
    add_relu fp32     0.530 | 0.637
    bwd_apply bf16    0.996 | 0.996
    bwd_apply fp32    0.367 | 0.661
    bwd_reduce sums   0.037 | 0.032
    stats             0.484 | 0.497
    l2norm            0.995 | 0.995   (the bf16 dxT copy; fp32 outputs stay below 0.3)
    adamw             0.268 | 0.292
(bf16 figures approach 1 by construction: 2 * 2^-9 |ref| is the half ulp at the bottom of a
binade.  The CPU column covers the small cases only; the device column is the maximum over the
whole file's run, the >= 100 MB cases included.)

Untouched memory.  Outputs are pre-filled with a sentinel and have 256 sentinel rows beyond M,
statistic buffers one sentinel replica beyond stat_rep, the bit mask 64 sentinel bytes, float
vectors 256 sentinel elements; inputs are followed by 4096 large values in the same allocation.
A sentinel left inside an output fails the bound (|SENT| = 1024 is far beyond any value here).
"""
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
C_EW = 2.0
C_APPLY = 6.0
C_P = 17.0
GUARD = 256
SENT = -1024.0
TAIL = 4096
SLICE = 1 << 24
WORST = {}


def tol(dt):
    return 2e-5 if dt == F32 else 1.5e-2


def dtid(dt):
    return "fp32" if dt == F32 else "bf16"


def epc(dt):
    return 8 if dt == BF16 else 4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlp_amd import ops as o
    return o


# ---------------------------------------------------------------- helpers
def gen_for(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def chan(C, g, lo=0.5, hi=1.5, signed=True, dtype=F32):
    """[C] coefficients on the CPU: (lo..hi) * (1 + c / C), alternating sign."""
    c = torch.arange(C, dtype=F64)
    v = (lo + (hi - lo) * torch.rand(C, generator=g, dtype=F64)) * (1 + c / C)
    if signed:
        v = v * (1 - 2 * (c % 2))
    return v.to(dtype)


def with_tail(t, dev=None):
    dev = dev or t.device
    buf = torch.full((t.numel() + TAIL,), 100.0, dtype=t.dtype, device=dev)
    buf[:t.numel()].copy_(t.flatten())
    return buf[:t.numel()].view(t.shape)


def guarded(M, Cc, dt, dev):
    buf = torch.full((M + GUARD, Cc), SENT, dtype=dt, device=dev)
    return buf, buf[:M]


def gvec(n, dev, dt=F32):
    buf = torch.full((n + GUARD,), SENT, dtype=dt, device=dev)
    return buf, buf[:n]


def assert_guard(name, buf, M):
    assert bool((buf[M:] == SENT).all().item()), f"{name}: elements beyond the output written"


def stat_buf(rep, Cc, dev):
    s = torch.zeros((rep + 1) * Cc, dtype=F64, device=dev)
    s[rep * Cc:] = SENT
    return s


def pack_bits(mask):
    m = mask.reshape(-1, 8).to(torch.int32)
    wgt = 2 ** torch.arange(8, device=mask.device, dtype=torch.int32)
    return (m * wgt).sum(1).to(torch.uint8)


def row_slices(M, Cc):
    step = max(1, SLICE // Cc)
    for a in range(0, M, step):
        yield a, min(M, a + step)


def ref_dev(numel, dev):
    return "cpu" if numel <= (1 << 22) else dev


def fma32(a, b, c):
    """fp32 fma: the product of two fp32 is exact in fp64, one rounding back to fp32 (the
    double rounding differs from a true fma by at most 2^-29 relative, and rarely)."""
    return (a.double() * b.double() + c.double()).float()


def store(v32, dt):
    return v32.to(dt)


class Gate:
    """rel-L2 and per-element gate accumulated over row slices."""

    def __init__(self, name, family, rel_tol):
        self.name, self.family, self.rel_tol = name, family, rel_tol
        self.d2 = self.r2 = 0.0
        self.nviol = self.n = 0
        self.worst = 0.0

    def add(self, got, ref, bound):
        got = got.double().to(ref.device)
        d = (got - ref).abs()
        self.d2 += float((d * d).sum())
        self.r2 += float((ref * ref).sum())
        self.nviol += int((~(d <= bound)).sum())   # NaN counts as a violation
        self.n += ref.numel()
        if ref.numel():
            self.worst = max(self.worst, float((d / (bound + 1e-300)).max()))
        return self

    def finish(self):
        r = math.sqrt(self.d2) / (math.sqrt(self.r2) + 1e-30)
        WORST[self.family] = max(WORST.get(self.family, 0.0), self.worst)
        print(f"{self.name}: rel-L2 {r:.3e} (gate {self.rel_tol:.1e}), worst |err|/bound {self.worst:.3f}, "
              f"violations {self.nviol} of {self.n}")
        assert r < self.rel_tol, f"{self.name}: rel-L2 {r:.3e} >= {self.rel_tol:.1e}"
        assert self.nviol == 0, f"{self.name}: {self.nviol} elements beyond the bound (worst ratio {self.worst:.2f})"


def gate(name, family, rel_tol, got, ref, bound):
    Gate(name, family, rel_tol).add(got, ref, bound).finish()


def out_bound(dt, ref, noise):
    """noise = c eps32 S (already holding the factor 2 as c eps32 = 2 c u)."""
    return 2.0 * (2.0 ** -9 * ref.abs() + noise) if dt == BF16 else noise


# ---------------------------------------------------------------- add-ReLU
def add_relu_inputs(M, C, dt, variant, dev, seed):
    """variant: 'none' | 'idt' | 'ds' (idt transformed by scd / shd).  Large tensors are drawn on
    the device, small ones on the CPU (the emulation test reads the same ones)."""
    gd = ref_dev(M * C, dev)
    g = gen_for(gd, seed)
    gc = gen_for("cpu", seed + 1)
    d = {"y": torch.randn(M, C, generator=g, device=gd).to(dt), "idt": None, "scd": None, "shd": None,
         "sc": chan(C, gc), "sh": chan(C, gc, 0.1, 0.6)}
    if variant != "none":
        d["idt"] = torch.randn(M, C, generator=g, device=gd).to(dt)
    if variant == "ds":
        d["scd"], d["shd"] = chan(C, gc, 0.3, 1.0), chan(C, gc, 0.1, 0.4)
    return d


def add_relu_ref(d, a, b, where):
    """fp64 reference and S for rows [a, b) on device `where`."""
    f = lambda t: t.to(where).double()
    y, sc, sh = f(d["y"][a:b]), f(d["sc"]), f(d["sh"])
    r = y * sc + sh
    S = y.abs() * sc.abs() + sh.abs()
    if d["idt"] is not None:
        i = f(d["idt"][a:b])
        if d["scd"] is not None:
            r = r + i * f(d["scd"]) + f(d["shd"])
            S = S + i.abs() * f(d["scd"]).abs() + f(d["shd"]).abs()
        else:
            r = r + i
            S = S + i.abs()
    return torch.relu(r), S


def add_relu_emulate(d, dt):
    y, sc, sh = d["y"].float(), d["sc"], d["sh"]
    b = sh + d["shd"] if d["scd"] is not None else sh
    if d["idt"] is not None:
        c = d["scd"] if d["scd"] is not None else torch.ones_like(sc)
        u = fma32(y, sc.expand_as(y), fma32(d["idt"].float(), c.expand_as(y), b.expand_as(y)))
    else:
        u = fma32(y, sc.expand_as(y), b.expand_as(y))
    return store(torch.relu(u), dt)


def run_add_relu(ops, name, M, C, dt, variant, dev, seed, emulate=False):
    d = add_relu_inputs(M, C, dt, variant, dev, seed)
    fam = f"add_relu {dtid(dt)}"
    if emulate:
        out = add_relu_emulate(d, dt)
        ref, S = add_relu_ref(d, 0, M, "cpu")
        gate(f"emulated {name}", fam, tol(dt), out, ref, out_bound(dt, ref, C_EW * EPS32 * S))
        return
    dd = {k: (with_tail(v, dev) if v is not None else None) for k, v in d.items()}
    nb = M * C // 8
    outs = []
    for use_mask in ((True, False) if dt == BF16 else (False,)):
        obuf, out = guarded(M, C, dt, dev)
        rm = torch.full((nb + 64,), 0xA5, dtype=torch.uint8, device=dev) if use_mask else None
        ops.bn_add_relu(dd["y"], dd["sc"], dd["sh"], dd["idt"], dd["scd"], dd["shd"], out, rm)
        torch.cuda.synchronize()
        assert_guard(name, obuf, M)
        if use_mask:
            assert bool((rm[nb:] == 0xA5).all().item()), f"{name}: mask bytes beyond M * C / 8 written"
            assert torch.equal(rm[:nb], pack_bits(out > 0)), f"{name}: relu_mask differs from (out > 0)"
        outs.append(out)
    where = ref_dev(M * C, dev)
    G = Gate(name, fam, tol(dt))
    for a, b in row_slices(M, C):
        ref, S = add_relu_ref(d, a, b, where)
        G.add(outs[0][a:b], ref, out_bound(dt, ref, C_EW * EPS32 * S))
    G.finish()
    if len(outs) == 2:   # the call without relu_mask: the same kernel, the same bits
        assert torch.equal(outs[0], outs[1]), f"{name}: output differs between relu_mask and no relu_mask"


# (id, M, C): nchunks = M * C / 8.  C = 8 is cpr = 1 (any chunk count reachable): one partial
# segment, one short of / exactly / one past a 1024-chunk segment, three segments and a tail;
# then every cpr up to 256 (C = 2048) at a chunk count that is no multiple of 1024.
SMALL_BF16 = [("C8-n1", 1, 8), ("C8-n1023", 1023, 8), ("C8-n1024", 1024, 8), ("C8-n1025", 1025, 8),
              ("C8-n3077", 3 * 1024 + 5, 8), ("C64-n1048", 131, 64), ("C128-n1072", 67, 128),
              ("C256-n1184", 37, 256), ("C512-n1216", 19, 512), ("C2048-n1280", 5, 2048)]
VARIANTS = ("none", "idt", "ds")


def ar_route(variant):
    return "blk" if variant == "none" else "strided-nt"


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", SMALL_BF16, ids=[c[0] for c in SMALL_BF16])
def test_add_relu_bf16_small(ops, case, variant):
    """No residual: bn_add_relu_blk_kernel<false, false> (tensor <= 100 MB).  Residual, plain and
    transformed: bn_add_relu_kernel<bf16, true, 1, true> (tensor < 256 MB)."""
    _, M, C = case
    run_add_relu(ops, f"add_relu {ar_route(variant)} {case[0]} {variant}", M, C, BF16, variant, "cuda", 11)


# 32800 * 64 = 2099200 chunks > 2048 * 1024: the blocked kernel's segment loop iterates (no
# residual); with a residual it is the thread-strided kernel past the ew_grid cap (> 2^20 chunks).
# 106496 x 512 bf16 = 104 MB: thread-strided with non-temporal stores, grid-stride loop.
# 524288 x 512 = 512 MB (no residual) and 262144 x 512 = 256 MB (residual): blocked + NT loads.
BIG_AR = [("blk-cap-M32800", 32800, 512, "none"), ("strided-nt-cap-M32800", 32800, 512, "ds"),
          ("strided-nt-104MB", 106496, 512, "none"), ("blk-ntl-512MB", 524288, 512, "none"),
          ("blk-ntl-256MB-idt", 262144, 512, "idt"), ("blk-ntl-256MB-ds", 262144, 512, "ds")]


@gpu
@pytest.mark.parametrize("case", BIG_AR, ids=[c[0] for c in BIG_AR])
def test_add_relu_bf16_large(ops, case):
    name, M, C, variant = case
    run_add_relu(ops, f"add_relu {name}", M, C, BF16, variant, "cuda", 12)


# fp32: thread-strided only (bn_add_relu_kernel<float, HAS_IDT>); C = 4 is cpr = 1, C = 1024 is
# cpr = 256; 8200 * 128 = 1049600 chunks > 2^20 is past the ew_grid cap.
F32_AR = [("C4-n1", 1, 4), ("C4-n1025", 1025, 4), ("C64-n2096", 131, 64), ("C512-n2432", 19, 512),
          ("C1024-n1280", 5, 1024), ("cap-C512-M8200", 8200, 512)]


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", F32_AR, ids=[c[0] for c in F32_AR])
def test_add_relu_fp32(ops, case, variant):
    _, M, C = case
    run_add_relu(ops, f"add_relu strided fp32 {case[0]} {variant}", M, C, F32, variant, "cuda", 13)


@gpu
def test_add_relu_fp32_refuses_relu_mask(ops):
    dev = "cuda"
    y = torch.randn(16, 64, device=dev)
    sc = torch.ones(64, device=dev)
    obuf, out = guarded(16, 64, F32, dev)
    rm = torch.full((16 * 64 // 8 + 64,), 0xA5, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError):
        ops.bn_add_relu(y, sc, sc, None, None, None, out, rm)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all().item()) and bool((rm == 0xA5).all().item())


# ---------------------------------------------------------------- BN backward: coefficients, apply
def side_inputs(C, count, gc):
    """mean, istd, gamma (fp32) and folded sums (fp64) of one BN side, on the CPU."""
    return {"mean": chan(C, gc, 0.2, 0.8), "istd": chan(C, gc, 0.5, 2.0, signed=False), "gamma": chan(C, gc),
            "sg": chan(C, gc, 0.02, 0.2, dtype=F64) * count, "sgx": chan(C, gc, 0.02, 0.2, dtype=F64) * count}


def coef_ref(s, count, where="cpu"):
    f = lambda t: t.to(where).double()
    k = f(s["gamma"]) * f(s["istd"])
    mg, mgx = f(s["sg"]) / count, f(s["sgx"]) / count
    t = k * f(s["istd"]) * mgx
    return k, -t, -k * mg, t * f(s["mean"])   # k, b, c = c1 + c2


def coef_emulate(s, count):
    inv = torch.tensor(1.0 / count, dtype=F64).float()
    k = s["gamma"] * s["istd"]
    mg, mgx = s["sg"].float() * inv, s["sgx"].float() * inv
    t = (k * s["istd"]) * mgx
    return k, -t, (-(k * mg)) + t * s["mean"]


def apply_inputs(M, C, dt, two, opts, HW, dev, seed):
    """opts: subset of {'mask', 'gout', 'dbc'}."""
    gd = ref_dev(M * C, dev)
    g = gen_for(gd, seed)
    gc = gen_for("cpu", seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g, device=gd)
    d = {"dout": None, "dbc": None, "mask": None, "HW": HW if "dbc" in opts else 1, "A": side_inputs(C, M, gc),
         "B": side_inputs(C, M, gc) if two else None}
    if "dbc" in opts:
        d["dbc"] = rn(M // HW, C) * 7.0
    else:
        d["dout"] = rn(M, C).to(dt)
    if "mask" in opts:
        mk = rn(M, C)
        d["mask"] = torch.where(mk.abs() < 0.2, torch.zeros_like(mk), mk).to(dt)   # > 0, < 0 and == 0
    d["A"]["y"] = rn(M, C).to(dt)
    if two:
        d["B"]["y"] = rn(M, C).to(dt)
    return d


def apply_g(d, a, b, where, emulate=False):
    if d["dbc"] is not None:
        C = d["dbc"].shape[1]
        rows = torch.arange(a, b, device=d["dbc"].device) // d["HW"]
        if emulate:
            g = d["dbc"][rows] * torch.tensor(1.0 / d["HW"], dtype=F64).float()
        else:
            g = d["dbc"][rows].to(where).double() / d["HW"]
    else:
        g = d["dout"][a:b].float() if emulate else d["dout"][a:b].to(where).double()
    if d["mask"] is not None:
        mk = d["mask"][a:b].to(g.device)
        g = torch.where(mk > 0, g, torch.zeros_like(g))
    return g


def apply_ref(d, side, g, a, b, M, where):
    k, bb, c1, c2 = coef_ref(d[side], M, where)
    y = d[side]["y"][a:b].to(where).double()
    return k * g + bb * y + (c1 + c2), (k * g).abs() + (bb * y).abs() + c1.abs() + c2.abs()


def run_bwd_apply(ops, name, M, C, dt, two, opts, HW, dev, seed, emulate=False):
    d = apply_inputs(M, C, dt, two, opts, HW, dev, seed)
    fam = f"bwd_apply {dtid(dt)}"
    sides = ("A", "B") if two else ("A",)
    if emulate:
        g32 = apply_g(d, 0, M, "cpu", emulate=True)
        g64 = apply_g(d, 0, M, "cpu")
        for s in sides:
            k, bb, c = coef_emulate(d[s], M)
            y = d[s]["y"].float()
            dy = store(fma32(k.expand_as(y), g32, fma32(bb.expand_as(y), y, c.expand_as(y))), dt)
            ref, S = apply_ref(d, s, g64, 0, M, M, "cpu")
            gate(f"emulated {name} dy_{s}", fam, tol(dt), dy, ref, out_bound(dt, ref, C_APPLY * EPS32 * S))
        return
    mv = lambda t: with_tail(t, dev) if t is not None else None
    dout, dbc, mask = mv(d["dout"]), mv(d["dbc"]), mv(d["mask"])
    args, bufs = {}, {}
    for s in sides:
        bufs[s] = guarded(M, C, dt, dev)
        args[s] = [mv(d[s][q]) for q in ("y", "mean", "istd", "gamma", "sg", "sgx")] + [bufs[s][1]]
    gbuf, gout = guarded(M, C, dt, dev) if "gout" in opts else (None, None)
    ops.bn_bwd_apply(M, C, dout, dbc, d["HW"], mask, args["A"], args.get("B"), gout, bufs["A"][1])
    torch.cuda.synchronize()
    where = ref_dev(M * C, dev)
    gates = {s: Gate(f"{name} dy_{s}", fam, tol(dt)) for s in sides}
    Gg = Gate(f"{name} g_out", fam, tol(dt))
    for a, b in row_slices(M, C):
        g = apply_g(d, a, b, where)
        for s in sides:
            ref, S = apply_ref(d, s, g, a, b, M, where)
            gates[s].add(bufs[s][1][a:b], ref, out_bound(dt, ref, C_APPLY * EPS32 * S))
        if gout is not None:
            got = gout[a:b].double().to(where)
            assert bool((got[g == 0] == 0).all().item()), f"{name}: g_out not exactly 0 where the mask is 0"
            if d["dbc"] is None:
                assert torch.equal(got, g), f"{name}: g_out differs from the masked dout"
            else:
                Gg.add(got, g, out_bound(dt, g, EPS32 * g.abs()))   # dbc * f32(1 / HW): 2 roundings
    for s in sides:
        gates[s].finish()
        assert_guard(name, bufs[s][0], M)
    if gout is not None:
        assert_guard(name, gbuf, M)
        if d["dbc"] is not None:
            Gg.finish()


APPLY_BLK = SMALL_BF16 + [("cap-M32800", 32800, 512)]


@gpu
@pytest.mark.parametrize("two", (False, True), ids=["one-side", "two-sides"])
@pytest.mark.parametrize("case", APPLY_BLK, ids=[c[0] for c in APPLY_BLK])
def test_bwd_apply_bf16_plain(ops, case, two):
    """bn_bwd_apply_blk_kernel<HAS_B, false>: what every plain call of the training step runs."""
    _, M, C = case
    run_bwd_apply(ops, f"bwd_apply blk {case[0]} {'two' if two else 'one'}", M, C, BF16, two, (), 1, "cuda", 21)


@gpu
@pytest.mark.parametrize("two", (False, True), ids=["one-side", "two-sides"])
def test_bwd_apply_bf16_plain_256MB(ops, two):
    """bn_bwd_apply_blk_kernel<HAS_B, true> (non-temporal loads): 262144 x 512 bf16 = 256 MB."""
    run_bwd_apply(ops, f"bwd_apply blk-ntl 256MB {'two' if two else 'one'}", 262144, 512, BF16, two, (), 1,
                  "cuda", 22)


# thread-strided bn_bwd_apply_kernel: N = 5, HW = 49 (245 rows: 49 divides neither the 256 / cpr
# rows a workgroup covers per sweep nor M's chunk count); 16400 * 64 chunks > 2^20: past ew_grid.
APPLY_OPTS = [("mask",), ("gout",), ("mask", "gout"), ("dbc",), ("dbc", "mask", "gout")]
APPLY_STRIDED = [(M, C, o, two) for (M, C) in ((245, 8), (245, 64), (245, 512)) for o in APPLY_OPTS
                 for two in (False, True)] + [(16400, 512, ("mask", "gout"), True), (16400, 512, ("dbc", "mask"), False)]


def _aid(c):
    return f"M{c[0]}-C{c[1]}-{'+'.join(c[2]) or 'plain'}-{'two' if c[3] else 'one'}"


@gpu
@pytest.mark.parametrize("case", APPLY_STRIDED, ids=[_aid(c) for c in APPLY_STRIDED])
def test_bwd_apply_bf16_strided(ops, case):
    M, C, opts, two = case
    HW = 49 if M == 245 else 82
    run_bwd_apply(ops, f"bwd_apply strided bf16 {_aid(case)}", M, C, BF16, two, opts, HW, "cuda", 23)


APPLY_F32 = [(M, C, o, two) for (M, C) in ((245, 4), (245, 64), (245, 1024))
             for o in ((), ("mask",), ("dbc", "mask", "gout")) for two in (False, True)]


@gpu
@pytest.mark.parametrize("case", APPLY_F32, ids=[_aid(c) for c in APPLY_F32])
def test_bwd_apply_fp32(ops, case):
    """bn_bwd_apply_kernel<float, HAS_B>: fp32 never takes the blocked kernel."""
    M, C, opts, two = case
    run_bwd_apply(ops, f"bwd_apply strided fp32 {_aid(case)}", M, C, F32, two, opts, 49, "cuda", 24)


# ---------------------------------------------------------------- BN backward: reduce
def reduce_geom(M, C, dt):
    cpr = C // epc(dt)
    rpi = 256 // cpr
    blocks = max(1, min(2048, -(-M // (rpi * 16))))
    iters = -(-M // (blocks * rpi))
    return rpi, blocks, rpi * iters   # T: rows one workgroup sums in fp32


def reduce_inputs(M, C, dt, has_b, bcast, HW, dev, seed):
    gd = ref_dev(M * C, dev)
    g = gen_for(gd, seed)
    gc = gen_for("cpu", seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g, device=gd)
    d = {"dout": None, "dbc": None, "HW": HW if bcast else 1}
    if bcast:
        d["dbc"] = rn(M // HW, C) * 7.0
    else:
        d["dout"] = rn(M, C).to(dt)
    mk = rn(M, C)
    d["mask"] = torch.where(mk.abs() < 0.2, torch.zeros_like(mk), mk).to(dt)
    for s in ("a", "b") if has_b else ("a",):
        d["y" + s] = rn(M, C).to(dt)
        d["mean" + s], d["istd" + s] = chan(C, gc, 0.2, 0.8), chan(C, gc, 0.5, 2.0, signed=False)
    return d


def reduce_terms(d, a, b, where, has_b, emulate=False):
    """[g, g xhat_a, g xhat_b] for rows [a, b): fp64, or the kernel's fp32 sequence."""
    dd = {"dout": d["dout"], "dbc": d["dbc"], "mask": d["mask"], "HW": d["HW"]}
    g = apply_g(dd, a, b, where, emulate)
    out = [g]
    for s in ("a", "b") if has_b else ("a",):
        y, mu, is_ = d["y" + s][a:b].to(g.device), d["mean" + s].to(g.device), d["istd" + s].to(g.device)
        out.append(g * ((y.float() - mu) * is_) if emulate else g * ((y.double() - mu.double()) * is_.double()))
    return out


def run_bwd_reduce(ops, name, M, C, dt, has_b, bcast, rep, dev, seed, emulate=False):
    HW = 49
    d = reduce_inputs(M, C, dt, has_b, bcast, HW, dev, seed)
    rpi, blocks, T = reduce_geom(M, C, dt)
    nt = 3 if has_b else 2
    where = "cpu" if emulate else ref_dev(M * C, dev)
    ref = torch.zeros(nt, rep, C, dtype=F64, device=where)
    mag = torch.zeros(nt, rep, C, dtype=F64, device=where)
    emu = torch.zeros(nt, rep, C, dtype=F64)
    for a, b in row_slices(M, C):
        terms = reduce_terms(d, a, b, where, has_b)
        wg = (torch.arange(a, b, device=where) // rpi) % blocks        # the workgroup of each row
        onehot = F.one_hot(wg % rep, rep).double().t()                  # [rep][rows]: replica = workgroup % rep
        for q, t in enumerate(terms):
            ref[q] += onehot @ t
            mag[q] += onehot @ t.abs()
        if emulate:   # fp32 sum per workgroup, then fp64 per replica
            for q, t in enumerate(reduce_terms(d, a, b, "cpu", has_b, emulate=True)):
                part = torch.zeros(blocks, C).index_add_(0, wg, t)
                emu[q].index_add_(0, torch.arange(blocks) % rep, part.double())
    bound = 2.0 * (T + 4) * EPS32 * mag + blocks * EPS64 * mag
    tot_ref, tot_bound = ref.sum(1), bound.sum(1)
    if emulate:
        gate(f"emulated {name}", "bwd_reduce sums", 1e-4, emu, ref, bound)
        return
    mv = lambda t: with_tail(t, dev) if t is not None else None
    sums = [stat_buf(rep, C, dev) for _ in range(3)]
    ops.bn_bwd_reduce(M, C, mv(d["dout"]), mv(d["dbc"]), d["HW"], mv(d["mask"]), mv(d["ya"]), mv(d["meana"]),
                      mv(d["istda"]), mv(d.get("yb")), mv(d.get("meanb")), mv(d.get("istdb")), sums[0], sums[1],
                      sums[2], d["mask"].to(dev), stat_rep=rep)
    torch.cuda.synchronize()
    got = torch.stack([s[:rep * C].view(rep, C) for s in sums[:nt]]).to(where)
    for s in sums:
        assert bool((s[rep * C:] == SENT).all().item()), f"{name}: sums written beyond stat_rep replicas"
    if not has_b:
        assert bool((sums[2][:rep * C] == 0).all().item()), f"{name}: sum_gb written without yb"
    # replica r holds exactly the workgroups r mod rep; their sum is the total
    gate(f"{name} per replica (T = {T}, {blocks} workgroups)", "bwd_reduce sums", 1e-4, got, ref, bound)
    gate(f"{name} sum over replicas", "bwd_reduce sums", 1e-4, got.sum(1), tot_ref, tot_bound)
    ops.stat_reduce(rep, C, sums[0], sums[1], sums[2] if has_b else None)
    torch.cuda.synchronize()
    fold = torch.stack([s[:C] for s in sums[:nt]]).to(where)
    gate(f"{name} folded copy 0", "bwd_reduce sums", 1e-4, fold, tot_ref, tot_bound + rep * EPS64 * mag.sum(1))
    for s in sums:
        assert bool((s[rep * C:] == SENT).all().item()), f"{name}: stat_reduce wrote beyond stat_rep replicas"


# C at cpr 1, 8, 64, 256; M = 245 = 5 * 49 is no multiple of rows_per_iter 256, 32, 4.
REDUCE = [(dt, C, has_b, bcast, rep) for dt, Cs in ((BF16, (8, 64, 512, 2048)), (F32, (4, 32, 256, 1024)))
          for C in Cs for has_b in (False, True) for bcast in (False, True) for rep in (1, 4)]


def _rid(c):
    return f"{dtid(c[0])}-C{c[1]}-{'yb' if c[2] else 'noyb'}-{'dbc' if c[3] else 'dout'}-rep{c[4]}"


@gpu
@pytest.mark.parametrize("case", REDUCE, ids=[_rid(c) for c in REDUCE])
def test_bwd_reduce(ops, case):
    dt, C, has_b, bcast, rep = case
    run_bwd_reduce(ops, f"bwd_reduce {_rid(case)}", 245, C, dt, has_b, bcast, rep, "cuda", 31)


@gpu
@pytest.mark.parametrize("case", [(F32, 1024, 32768 + 3), (BF16, 512, 131072 + 5)], ids=["fp32-C1024", "bf16-C512"])
def test_bwd_reduce_past_workgroup_cap(ops, case):
    """ceil(M / (16 rows_per_iter)) = 2049 > 2048 workgroups: every thread accumulates 17 rows."""
    dt, C, M = case
    rpi, blocks, T = reduce_geom(M, C, dt)
    assert blocks == 2048 and T == 17 * rpi
    run_bwd_reduce(ops, f"bwd_reduce cap {dtid(dt)} C{C} M{M}", M, C, dt, True, False, 4, "cuda", 32)


# ---------------------------------------------------------------- fp64 statistics kernels
REPS = (1, 2, 3, 4, 5, 8, 31, 32, 33, 64)   # 4-wave and 8-wave splits, the 4x unrolled loop and its tail
CS = (1, 63, 64, 65, 100, 512)              # partial 64-channel groups
COUNTS = (256 * 128 * 128, 245, 2, 1)
BN_EPS = float(torch.tensor(1e-5, dtype=F32))
BN_MOM = float(torch.tensor(0.1, dtype=F32))


def finalize_ref(s, ss, count, gamma, beta, rm, rv):
    """fp64 BatchNorm statistics -> mean, invstd, scale, shift, running mean / var and bounds."""
    mean = s / count
    ex2 = ss / count
    var = (ex2 - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    g, b = gamma.double(), beta.double()
    unb = var * count / (count - 1) if count > 1 else var
    ref = {"mean": mean, "invstd": invstd, "scale": g * invstd, "shift": b - mean * g * invstd,
           "rm": (1 - BN_MOM) * rm.double() + BN_MOM * mean, "rv": (1 - BN_MOM) * rv.double() + BN_MOM * unb}
    return ref, var, ex2


def finalize_bounds(ref, var, ex2, count, gamma, beta, rm, rv, rep):
    dvar = (4 + 2 * rep) * EPS64 * (ex2 + ref["mean"] ** 2)          # fp64 cancellation of var
    rel = 0.5 * dvar / (var + BN_EPS)                                  # its share of invstd
    S_shift = beta.double().abs() + (ref["mean"] * ref["scale"]).abs()
    ub = count / (count - 1) if count > 1 else 1.0
    return {"mean": EPS32 * ref["mean"].abs(), "invstd": (EPS32 + rel) * ref["invstd"],
            "scale": (2 * EPS32 + rel) * ref["scale"].abs(), "shift": (5 * EPS32 + rel) * S_shift,
            "rm": 4 * EPS32 * ((1 - BN_MOM) * rm.double().abs() + BN_MOM * ref["mean"].abs()),
            "rv": 4 * EPS32 * ((1 - BN_MOM) * rv.double().abs() + BN_MOM * var * ub) + BN_MOM * dvar * ub}


def finalize_inputs(rep, C, count, seed):
    """Replicated sums whose every partial sum is exact in fp64 (multiples of 2^-16 below 2^30):
    any fold order gives the same bits, so bit-equality between the two fold kernels is owed.
    Channel 0 (and every 7th) holds equal values: var = 0 exactly, invstd = 1 / sqrt(eps)."""
    gc = gen_for("cpu", seed)
    q = lambda t: torch.round(t * 65536.0) / 65536.0
    mu = q(chan(C, gc, 0.2, 1.5, dtype=F64))
    sig2 = q(chan(C, gc, 0.3, 2.0, signed=False, dtype=F64))
    const = torch.arange(C) % 7 == 0
    mu = torch.where(const, torch.full_like(mu, 3.0), mu)
    sig2 = torch.where(const, torch.zeros_like(sig2), sig2)
    s, ss = mu * count, (sig2 + mu * mu) * count
    w = torch.randint(-512, 512, (rep, C), generator=gc).double() / 1024.0
    w[rep - 1] = 1.0 - w[:rep - 1].sum(0)                              # the replicas add up exactly
    s = q(s)
    ss = q(ss)
    S, SS = q(w * s), q(w * ss)
    S[rep - 1] = s - S[:rep - 1].sum(0)
    SS[rep - 1] = ss - SS[:rep - 1].sum(0)
    return {"S": S, "SS": SS, "s": s, "ss": ss, "gamma": chan(C, gc), "beta": chan(C, gc, 0.1, 0.6),
            "rm": chan(C, gc, 0.1, 0.5), "rv": chan(C, gc, 0.5, 1.5, signed=False)}


def finalize_emulate(s, ss, count, gamma, beta, rm, rv):
    mean = s / count
    var = (ss / count - mean * mean).clamp_min(0)
    invstd = (1.0 / torch.sqrt(var + BN_EPS)).float()
    sc = gamma * invstd
    unb = (var * count / (count - 1) if count > 1 else var).float()
    mom = torch.tensor(BN_MOM, dtype=F32)
    return {"mean": mean.float(), "invstd": invstd, "scale": sc, "shift": beta - mean.float() * sc,
            "rm": (1 - mom) * rm + mom * mean.float(), "rv": (1 - mom) * rv + mom * unb}


def test_reference_formulas_match_torch_fp64():
    """The fp64 formulas used as references against torch's own fp64 operators on the CPU: train-mode
    BatchNorm forward / running statistics / backward (folded k, b, c form), F.normalize and its
    autograd including an all-zero row, and torch.optim.AdamW."""
    g = gen_for("cpu", 1)
    N, C, H = 5, 6, 7
    x = torch.randn(N, C, H, H, generator=g, dtype=F64) * 2 + 0.5
    gamma, beta = chan(C, g, dtype=F64), chan(C, g, 0.1, 0.6, dtype=F64)
    rm, rv = chan(C, g, dtype=F64), chan(C, g, signed=False, dtype=F64)
    xr = x.clone().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C, eps=BN_EPS, momentum=BN_MOM).double()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    y = bn(xr)
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)
    xm = x.permute(0, 2, 3, 1).reshape(-1, C)
    count = xm.shape[0]
    ref, var, _ = finalize_ref(xm.sum(0), (xm * xm).sum(0), count, gamma, beta, rm, rv)
    assert (xm * ref["scale"] + ref["shift"] - y.detach().permute(0, 2, 3, 1).reshape(-1, C)).abs().max() < 1e-12
    assert (ref["rm"] - bn.running_mean).abs().max() < 1e-12 and (ref["rv"] - bn.running_var).abs().max() < 1e-12
    gm = dy.permute(0, 2, 3, 1).reshape(-1, C)
    xhat = (xm - ref["mean"]) * ref["invstd"]
    side = {"gamma": gamma, "istd": ref["invstd"], "mean": ref["mean"], "sg": gm.sum(0), "sgx": (gm * xhat).sum(0)}
    k, b, c1, c2 = coef_ref(side, count)
    dx = k * gm + b * xm + c1 + c2
    assert (dx - xr.grad.permute(0, 2, 3, 1).reshape(-1, C)).abs().max() < 1e-12
    assert (side["sgx"] - bn.weight.grad).abs().max() < 1e-12 and (side["sg"] - bn.bias.grad).abs().max() < 1e-12
    # l2norm
    x = torch.randn(5, 9, generator=g, dtype=F64)
    x[2] = 0
    xr = x.clone().requires_grad_(True)
    yn = F.normalize(xr, dim=1)
    dyn = torch.randn(5, 9, generator=g, dtype=F64)
    yn.backward(dyn)
    yy, nn = l2_fwd_ref(x)
    assert (yy - yn.detach()).abs().max() < 1e-15
    assert (l2_bwd_ref(yy, nn, dyn, 1.0)[0] - xr.grad).abs().max() < 1e-12 * xr.grad.abs().max()
    # AdamW
    for step, wd in ((1, 0.0), (2, 0.01), (1000, 0.01)):
        d = adamw_inputs(257, step, wd, 3)
        ref = adamw_ref(d)
        tp, tm, tv = adamw_torch(d)
        for q, b in (("p", tp), ("m", tm), ("v", tv)):   # 1e-6 of the fp32 bound: a few fp64 roundings of S
            assert ((ref[q] - b).abs() <= 1e-6 * ref["b" + q]).all(), f"fp64 AdamW formula differs from torch in {q}"


@gpu
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("rep", REPS)
def test_stat_reduce(ops, rep, C):
    """stat_reduce_kernel: (a, b, c), (a) and (a, -, c) with general fp64 values; copy 0 is the fold
    within rep * 2^-52 * sum |terms|, copies 1.. and the sentinel replica keep their values."""
    dev = "cuda"
    g = gen_for("cpu", 40 + rep)
    for present in ((1, 1, 1), (1, 0, 0), (1, 0, 1)):
        vals = [torch.randn(rep, C, generator=g, dtype=F64) * chan(C, g, dtype=F64) * 1e3 for _ in range(3)]
        bufs = []
        for v in vals:
            s = stat_buf(rep, C, dev)
            s[:rep * C] = v.flatten().to(dev)
            bufs.append(s)
        ops.stat_reduce(rep, C, *[b if p else None for b, p in zip(bufs, present)])
        torch.cuda.synchronize()
        for q, (v, s, p) in enumerate(zip(vals, bufs, present)):
            got = s.cpu()
            assert bool((got[rep * C:] == SENT).all()), "sentinel replica written"
            assert torch.equal(got[C:rep * C], v.flatten()[C:]), "replicas 1.. changed"
            if p:
                gate(f"stat_reduce rep {rep} C {C} array {q}", "stats", 1e-12, got[:C], v.sum(0),
                     rep * EPS64 * v.abs().sum(0))
            else:
                assert torch.equal(got[:C], v[0]), "an absent array was written"


@gpu
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("rep", REPS)
def test_bn_finalize(ops, rep, C):
    """vlp_bn_finalize (bn_finalize_kernel) against fp64 for every count, with and without the running
    statistics; vlp_bn_finalize_rep (fold_replicas + the same arithmetic) bit-equal to vlp_stat_reduce
    followed by vlp_bn_finalize in every float output, with the folded sums left in copy 0."""
    dev = "cuda"
    names = ("scale", "shift", "mean", "invstd")
    for ci, count in enumerate(COUNTS):
        d = finalize_inputs(rep, C, count, 50 + rep)
        ref, var, ex2 = finalize_ref(d["s"], d["ss"], count, d["gamma"], d["beta"], d["rm"], d["rv"])
        bnd = finalize_bounds(ref, var, ex2, count, d["gamma"], d["beta"], d["rm"], d["rv"], rep)
        const = torch.arange(C) % 7 == 0
        assert bool((var[const] == 0).all()) and torch.allclose(ref["invstd"][const], torch.tensor(BN_EPS, dtype=F64) ** -0.5)
        gm, bt = d["gamma"].to(dev), d["beta"].to(dev)
        res = []
        for fused in (False, True):
            for running in (True, False):
                s, ss = stat_buf(rep, C, dev), stat_buf(rep, C, dev)
                s[:rep * C], ss[:rep * C] = d["S"].flatten().to(dev), d["SS"].flatten().to(dev)
                outs = {n: gvec(C, dev) for n in names}
                rmb, rmv = gvec(C, dev)
                rvb, rvv = gvec(C, dev)
                rmv.copy_(d["rm"]), rvv.copy_(d["rv"])
                a = (gm, bt, BN_EPS, BN_MOM, rmv if running else None, rvv if running else None,
                     *[outs[n][1] for n in names])
                if fused:
                    ops.bn_finalize_rep(rep, count, s, ss, *a)
                else:
                    ops.stat_reduce(rep, C, s, ss)
                    ops.bn_finalize(count, s, ss, *a)
                torch.cuda.synchronize()
                tag = f"bn_finalize{'_rep' if fused else ''} rep {rep} C {C} count {count}"
                for buf in [outs[n][0] for n in names] + [rmb, rvb]:
                    assert_guard(tag, buf, C)
                for sb, tot in ((s, d["s"]), (ss, d["ss"])):
                    assert bool((sb[rep * C:] == SENT).all().item()), f"{tag}: sentinel replica written"
                    assert torch.equal(sb[:C].cpu(), tot), f"{tag}: copy 0 is not the (exact) fold"
                got = {n: outs[n][1].cpu() for n in names}
                got["rm"], got["rv"] = rmv.cpu(), rvv.cpu()
                if not running:
                    assert torch.equal(got["rm"], d["rm"]) and torch.equal(got["rv"], d["rv"]), f"{tag}: running written"
                for n in names + (("rm", "rv") if running else ()):
                    gate(f"{tag} {n}", "stats", 2e-5, got[n], ref[n], bnd[n])
                res.append(got)
        for n in res[0]:
            assert torch.equal(res[0][n], res[2][n]) and torch.equal(res[1][n], res[3][n]), \
                f"bn_finalize_rep differs from stat_reduce + bn_finalize in {n} (rep {rep}, C {C}, count {count})"


@gpu
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("rep", REPS)
def test_bn_grad_rep_and_param_grad(ops, rep, C):
    """bn_grad_rep_kernel with and without the downsample side, bn_param_grad_kernel on the folded sums:
    one fp32 rounding of the fp64 fold."""
    dev = "cuda"
    g = gen_for("cpu", 60 + rep)
    for ds in (False, True):
        vals = [torch.randn(rep, C, generator=g, dtype=F64) * chan(C, g, dtype=F64) * 50 for _ in range(3)]
        bufs = []
        for v in vals:
            s = stat_buf(rep, C, dev)
            s[:rep * C] = v.flatten().to(dev)
            bufs.append(s)
        o = [gvec(C, dev) for _ in range(6)]
        ops.bn_grad_rep(rep, C, bufs[0], bufs[1], o[0][1], o[1][1], bufs[2] if ds else None,
                        o[2][1] if ds else None, o[3][1] if ds else None)
        ops.bn_param_grad(bufs[0], bufs[1], o[4][1], o[5][1])
        torch.cuda.synchronize()
        tot = [v.sum(0) for v in vals]
        fb = [rep * EPS64 * v.abs().sum(0) for v in vals]
        tag = f"bn_grad_rep rep {rep} C {C} ds {ds}"
        for q in range(3):
            got = bufs[q].cpu()
            assert bool((got[rep * C:] == SENT).all()), f"{tag}: sentinel replica written"
            if q < 2 or ds:
                gate(f"{tag} fold {q}", "stats", 1e-12, got[:C], tot[q], fb[q])
            else:
                assert torch.equal(got[:rep * C], vals[2].flatten()), f"{tag}: absent sum_gxd written"
        for buf, _ in o:
            assert_guard(tag, buf, C)
        fl = lambda q: EPS32 * tot[q].abs() + fb[q]
        gate(f"{tag} dgamma", "stats", 2e-5, o[0][1].cpu(), tot[1], fl(1))
        gate(f"{tag} dbeta", "stats", 2e-5, o[1][1].cpu(), tot[0], fl(0))
        gate(f"bn_param_grad dgamma", "stats", 2e-5, o[4][1].cpu(), tot[1], fl(1))
        gate(f"bn_param_grad dbeta", "stats", 2e-5, o[5][1].cpu(), tot[0], fl(0))
        if ds:
            gate(f"{tag} dgamma_d", "stats", 2e-5, o[2][1].cpu(), tot[2], fl(2))
            gate(f"{tag} dbeta_d", "stats", 2e-5, o[3][1].cpu(), tot[0], fl(0))
        else:
            assert bool((o[2][0] == SENT).all().item()) and bool((o[3][0] == SENT).all().item())


@gpu
def test_bn_grad_rep_refuses_half_a_downsample_side(ops):
    dev = "cuda"
    s = [stat_buf(2, 64, dev) for _ in range(3)]
    o = [gvec(64, dev) for _ in range(4)]
    with pytest.raises(RuntimeError):
        ops.bn_grad_rep(2, 64, s[0], s[1], o[0][1], o[1][1], s[2], None, None)
    with pytest.raises(RuntimeError):
        ops.bn_grad_rep(2, 64, s[0], s[1], o[0][1], o[1][1], None, o[2][1], o[3][1])
    torch.cuda.synchronize()
    assert all(bool((b == SENT).all().item()) for b, _ in o)


def eval_ref(gamma, beta, rm, rv):
    invstd = 1.0 / torch.sqrt(rv.double() + BN_EPS)
    t = rm.double() * gamma.double() * invstd
    return {"scale": gamma.double() * invstd, "shift": beta.double() - t}, \
           {"scale": 6 * EPS32 * (gamma.double() * invstd).abs(), "shift": 8 * EPS32 * (beta.double().abs() + t.abs())}


def eval_inputs(C, seed):
    g = gen_for("cpu", seed)
    return chan(C, g), chan(C, g, 0.1, 0.6), chan(C, g, 0.1, 0.9), chan(C, g, 0.05, 2.0, signed=False)


@gpu
@pytest.mark.parametrize("C", CS)
def test_bn_eval_coeffs(ops, C):
    dev = "cuda"
    gamma, beta, rm, rv = eval_inputs(C, 70)
    ref, bnd = eval_ref(gamma, beta, rm, rv)
    (sb, sc), (hb, sh) = gvec(C, dev), gvec(C, dev)
    ops.bn_eval_coeffs(gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), BN_EPS, sc, sh)
    torch.cuda.synchronize()
    assert_guard("bn_eval_coeffs", sb, C), assert_guard("bn_eval_coeffs", hb, C)
    gate(f"bn_eval_coeffs C {C} scale", "stats", 2e-5, sc.cpu(), ref["scale"], bnd["scale"])
    gate(f"bn_eval_coeffs C {C} shift", "stats", 2e-5, sh.cpu(), ref["shift"], bnd["shift"])


def coef_bounds(s, count):
    k, b, c1, c2 = coef_ref(s, count)
    return (k, b, c1 + c2), (EPS32 * k.abs(), 6 * EPS32 * b.abs(), 8 * EPS32 * (c1.abs() + c2.abs()))


@gpu
@pytest.mark.parametrize("C", CS + (4,))
def test_bn_bwd_coef(ops, C):
    """bn_bwd_coef_kernel against fp64, and bit-equal to the coefficients vlp_bn_bwd_apply forms:
    on an fp32 tensor, g = 0, y = 0 returns c and g = 1, y = 0 returns k + c rounded once."""
    dev = "cuda"
    M = 245
    s = side_inputs(C, M, gen_for("cpu", 80))
    sd = {q: v.to(dev) for q, v in s.items()}
    cb, coef = gvec(3 * C, dev)
    ops.bn_bwd_coef(M, sd["gamma"], sd["istd"], sd["mean"], sd["sg"], sd["sgx"], coef)
    torch.cuda.synchronize()
    assert_guard("bn_bwd_coef", cb, 3 * C)
    got = coef.cpu().view(3, C)
    refs, bnds = coef_bounds(s, M)
    for q, n in enumerate("kbc"):
        gate(f"bn_bwd_coef C {C} {n}", "stats", 2e-5, got[q], refs[q], bnds[q])
    if C % 4 or 256 % (C // 4):
        return
    y = torch.zeros(M, C, device=dev)
    for gval in (0.0, 1.0):
        gin = torch.full((M, C), gval, device=dev)
        dbuf, dy = guarded(M, C, F32, dev)
        ops.bn_bwd_apply(M, C, gin, None, 1, None, (y, sd["mean"], sd["istd"], sd["gamma"], sd["sg"], sd["sgx"], dy),
                         None, None, y)
        torch.cuda.synchronize()
        want = got[2] if gval == 0.0 else got[0] + got[2]      # IEEE fp32 add = fma(k, 1, c)
        assert torch.equal(dy.cpu(), want.expand(M, C)), f"bn_bwd_apply's coefficients differ from bn_bwd_coef (g = {gval})"


# ---------------------------------------------------------------- head: l2norm, cast
L2_R = (1, 3, 4, 5, 257)
L2_E = (4, 63, 64, 65, 128, 512)
L2_TINY = float(torch.tensor(1e-12, dtype=F32))


def l2_rounds(E):
    return -(-E // 64) + 7


def l2_fwd_ref(x):
    n = x.double().norm(dim=1, keepdim=True)
    return x.double() / n.clamp_min(1e-12), n[:, 0]


def l2_bwd_ref(y, n, dy, gs):
    y, n, dy = y.double(), n.double()[:, None], dy.double()
    dotabs = (y * dy).abs().sum(1, keepdim=True)
    dot = (y * dy).sum(1, keepdim=True)
    live = n > L2_TINY
    nn = torch.where(live, n, torch.full_like(n, 1e-12))
    ref = gs * torch.where(live, (dy - y * dot) / nn, dy / nn)
    S = gs * (dy.abs() + torch.where(live, y.abs() * dotabs, torch.zeros_like(dy))) / nn
    return ref, S


def l2_inputs(R, E, seed):
    g = gen_for("cpu", seed)
    x = torch.randn(R, E, generator=g) * (1 + torch.arange(R)[:, None] % 5)
    if R >= 3:
        x[R // 2] = 0
    return x, torch.randn(R, E, generator=g)


def l2_fwd_emulate(x):
    E = x.shape[1]
    pad = (-E) % 64
    sq = F.pad(x * x, (0, pad)).view(x.shape[0], -1, 64)
    s = torch.zeros(x.shape[0], 64)
    for j in range(sq.shape[1]):
        s = s + sq[:, j]
    w = 32
    while w:   # butterfly
        s = s + s.view(-1, 64 // (2 * w), 2, w).flip(2).reshape(-1, 64)
        w //= 2
    n = torch.sqrt(s[:, :1])
    return x / n.clamp_min(L2_TINY), n[:, 0]


@gpu
@pytest.mark.parametrize("E", L2_E)
@pytest.mark.parametrize("R", L2_R)
def test_l2norm(ops, R, E):
    """l2norm_fwd_kernel / l2norm_bwd_kernel<T>: four rows per workgroup (R = 1, 3, 5, 257 leave a partial
    one), an all-zero row (n <= 1e-12 in both directions), gscale present / absent, dx only, dxT only
    (bf16 and fp32) and both.  The backward reference is the defining formula on the fp32 y and norm
    the kernel is given (test 1 shows it equal to F.normalize's autograd)."""
    dev = "cuda"
    x, dy = l2_inputs(R, E, 90)
    xd, dyd = with_tail(x, dev), with_tail(dy, dev)
    ybuf, y = guarded(R, E, F32, dev)
    nbuf, nrm = gvec(R, dev)
    ops.l2norm_fwd(xd, y, nrm)
    torch.cuda.synchronize()
    assert_guard("l2norm_fwd", ybuf, R), assert_guard("l2norm_fwd", nbuf, R)
    yr, nr = l2_fwd_ref(x)
    c = l2_rounds(E) / 2 + 2
    gate(f"l2norm_fwd R {R} E {E} norm", "l2norm", 2e-5, nrm.cpu(), nr, c * EPS32 * nr)
    gate(f"l2norm_fwd R {R} E {E} y", "l2norm", 2e-5, y.cpu(), yr, (c + 2) * EPS32 * yr.abs())
    if R >= 3:
        assert bool((y[R // 2] == 0).all().item()) and float(nrm[R // 2]) == 0.0
    gsv = torch.tensor([1.75], device=dev)
    for gs in (None, gsv):
        ref, S = l2_bwd_ref(y.cpu(), nrm.cpu(), dy, 1.0 if gs is None else 1.75)
        nb = (l2_rounds(E) + 5) * EPS32 * S
        for want_dx, tdt in ((True, None), (False, BF16), (False, F32), (True, BF16)):
            dxb, dx = guarded(R, E, F32, dev)
            tb, dxt = guarded(R, E, tdt, dev) if tdt is not None else (None, None)
            ops.l2norm_bwd(y, nrm, dyd, dx if want_dx else None, dxt, gs)
            torch.cuda.synchronize()
            tag = f"l2norm_bwd R {R} E {E} gs {gs is not None} dx {want_dx} dxT {tdt}"
            if want_dx:
                assert_guard(tag, dxb, R)
                gate(tag + " dx", "l2norm", 2e-5, dx.cpu(), ref, nb)
            else:
                assert bool((dxb == SENT).all().item()), f"{tag}: dx written though absent"
            if tdt is not None:
                assert_guard(tag, tb, R)
                gate(tag + " dxT", "l2norm", tol(tdt), dxt.cpu(), ref, out_bound(tdt, ref, nb))


CAST_N = (1, 255, 8192 * 256 + 259)


@gpu
@pytest.mark.parametrize("n", CAST_N)
@pytest.mark.parametrize("dt", (BF16, F32), ids=dtid)
def test_cast(ops, dt, n):
    """cast_kernel<T>: bit-equal to x.to(dtype) (round to nearest even) on bf16 ties (both parities),
    subnormals, +-0, and past the 8192-workgroup cap with an odd tail."""
    dev = "cuda"
    bits = torch.tensor([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x00000001,
                         0x00008000, 0x00018000, 0x807FFFFF, 0x00000000, 0x80000000, 0x7F7FFFFF, 0x7F7F7FFF,
                         0x00800000, 0x3F800000], dtype=torch.int64)
    special = ((bits & 0x7FFFFFFF) - (bits & 0x80000000)).to(torch.int32).view(F32)
    x = torch.randn(n, generator=gen_for("cpu", 95)) * 3
    k = min(n, special.numel())
    x[:k] = special[:k]
    x[n - 1] = special[n % special.numel()]
    xd = with_tail(x, dev)
    ybuf, y = gvec(n, dev, dt)
    ops.cast(xd, y)
    torch.cuda.synchronize()
    assert_guard("cast", ybuf, n)
    want = x.to(dt)
    iv = torch.int16 if dt == BF16 else torch.int32
    assert torch.equal(y.cpu().view(iv), want.view(iv)), f"vlp_cast {dtid(dt)} n {n}: not bit-equal to x.to(dtype)"


# ---------------------------------------------------------------- optimizer
ADAM_N = (1, 257, 8192 * 256 + 259)   # grid_for caps at 8192 workgroups of 256


def f32v(x):
    return float(torch.tensor(x, dtype=F32))


def adamw_inputs(n, step, wd, seed):
    """Hyper-parameters rounded to fp32 (the ABI passes floats); gradients over 1e-8 .. 1e3; the first
    elements have g = 0 and v = 0 (denominator eps)."""
    g = gen_for("cpu", seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=F64) * 11 - 8)
    grad = (mag * (1 - 2 * torch.randint(0, 2, (n,), generator=g))).float()
    p = torch.randn(n, generator=g)
    m = (torch.randn(n, generator=g, dtype=F64) * mag * 0.5).float()
    v = (torch.rand(n, generator=g, dtype=F64) * mag * mag).float()
    grad[:min(n, 3)] = 0
    v[:min(n, 3)] = 0
    if n > 1:
        m[1] = 0
    return {"p": p, "g": grad, "m": m, "v": v, "lr": f32v(5e-5), "b1": f32v(0.9), "b2": f32v(0.999),
            "eps": f32v(1e-8), "wd": f32v(wd), "step": step}


def adamw_hyper(d, rounded):
    """step_size and bc2_sqrt exactly as vlp_amd.ops.adamw computes them (fp64 on the host); the ABI
    passes them as floats: `rounded` is what the kernel sees, and the bound counts that rounding."""
    bc1 = 1.0 - d["b1"] ** d["step"]
    bc2 = 1.0 - d["b2"] ** d["step"]
    ss, bc2s = d["lr"] / bc1, bc2 ** 0.5
    return (f32v(ss), f32v(bc2s)) if rounded else (ss, bc2s)


def adamw_ref(d):
    """The formula of csrc/optim_ops.hip's header in fp64, and the S of each bound."""
    p, g, m, v = (d[q].double() for q in "pgmv")
    ss, bc2s = adamw_hyper(d, False)
    b1, b2 = d["b1"], d["b2"]
    pi = p * (1 - d["lr"] * d["wd"])
    mi = b1 * m + (1 - b1) * g
    vi = b2 * v + (1 - b2) * g * g
    den = vi.sqrt() / bc2s + d["eps"]
    S_m = (1 - b1) * (g.abs() + m.abs()) + m.abs()
    return {"p": pi - ss * mi / den, "m": mi, "v": vi, "bm": 3 * EPS32 * S_m, "bv": 5 * EPS32 * vi,
            "bp": C_P * EPS32 * (p.abs() + ss * S_m / den)}


def adamw_torch(d):
    p = torch.nn.Parameter(d["p"].double())
    opt = torch.optim.AdamW([p], lr=d["lr"], betas=(d["b1"], d["b2"]), eps=d["eps"], weight_decay=d["wd"])
    p.grad = d["g"].double()
    opt.state[p] = {"step": torch.tensor(float(d["step"] - 1)), "exp_avg": d["m"].double().clone(),
                    "exp_avg_sq": d["v"].double().clone()}
    opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


def adamw_emulate(d):
    p, g, m, v = d["p"], d["g"], d["m"], d["v"]
    t = lambda x: torch.tensor(x, dtype=F32)
    ss, bc2s = adamw_hyper(d, True)
    pi = p * (1 - t(d["lr"]) * t(d["wd"]))
    mi = fma32((1 - t(d["b1"])).expand_as(g), g - m, m)
    vi = v * t(d["b2"]) + (1 - t(d["b2"])) * g * g
    den = torch.sqrt(vi) / t(bc2s) + t(d["eps"])
    return pi - t(ss) * (mi / den), mi, vi


@gpu
@pytest.mark.parametrize("wd", (0.0, 0.01))
@pytest.mark.parametrize("step", (1, 2, 1000))
@pytest.mark.parametrize("n", ADAM_N)
def test_adamw(ops, n, step, wd):
    """vlp_adamw against the fp64 formula, and the formula against torch.optim.AdamW in fp64 on the
    CPU (n <= 257; test 1 covers it without a device as well)."""
    dev = "cuda"
    d = adamw_inputs(n, step, wd, 100 + step)
    ref = adamw_ref(d)
    if n <= 257:
        tp, tm, tv = adamw_torch(d)
        for q, b in (("p", tp), ("m", tm), ("v", tv)):   # 1e-6 of the fp32 bound: a few fp64 roundings of S
            assert ((ref[q] - b).abs() <= 1e-6 * ref["b" + q]).all(), f"fp64 AdamW formula differs from torch in {q}"
    bufs = {q: gvec(n, dev) for q in "pmv"}
    for q in "pmv":
        bufs[q][1].copy_(d[q])
    gd = with_tail(d["g"], dev)
    ops.adamw(bufs["p"][1], gd, bufs["m"][1], bufs["v"][1], d["lr"], d["b1"], d["b2"], d["eps"], d["wd"], step)
    torch.cuda.synchronize()
    tag = f"adamw n {n} step {step} wd {wd}"
    for q in "pmv":
        assert_guard(tag, bufs[q][0], n)
        gate(f"{tag} {q}", "adamw", 2e-5, bufs[q][1].cpu(), ref[q], ref["b" + q])
    assert torch.equal(gd.cpu(), d["g"])


@gpu
def test_adamw_n0_is_a_noop(ops):
    dev = "cuda"
    bufs = [torch.full((GUARD,), SENT, device=dev) for _ in range(4)]
    ops.adamw(bufs[0][:0], bufs[1][:0], bufs[2][:0], bufs[3][:0], 5e-5, 0.9, 0.999, 1e-8, 0.01, 1)
    torch.cuda.synchronize()
    assert all(bool((b == SENT).all().item()) for b in bufs)


@gpu
def test_adamw_rejects_null_and_misaligned_operands(ops):
    """vlp_adamw checks its operands as the other step entry points do: a NULL or not 4-B aligned
    pointer with n > 0 is hipErrorInvalidValue (1) and nothing is launched."""
    from vlp_amd._lib import lib, stream_of
    raw = lib()._fns["vlp_adamw"]
    t = [torch.ones(4, device="cuda") for _ in range(4)]
    ptrs = [x.data_ptr() for x in t]
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1e-2, 0.03, stream_of())
    for i in range(4):
        for bad in (None, ptrs[i] + 2):
            q = list(ptrs)
            q[i] = bad
            assert raw(4, *q, *tail) == 1, (i, bad)
    for n in (0, -5):
        assert raw(n, None, None, None, None, *tail) == 0
    torch.cuda.synchronize()
    assert all(bool((x == 1).all().item()) for x in t)


# ---------------------------------------------------------------- CPU: the bounds are satisfiable
def test_bound_holds_for_emulated_arithmetic():
    """Each kernel's fp32 sequence replayed in torch fp32 (same order, fma where the kernel has one, one
    rounding on store) meets every bound against the fp64 reference on the suite's own small inputs;
    the worst ratio per family is printed (the CPU column of the module docstring)."""
    WORST.clear()
    for _, M, C in SMALL_BF16:
        for variant in VARIANTS:
            run_add_relu(None, f"add_relu bf16 M{M} C{C} {variant}", M, C, BF16, variant, "cpu", 11, emulate=True)
    for _, M, C in F32_AR[:5]:
        for variant in VARIANTS:
            run_add_relu(None, f"add_relu fp32 M{M} C{C} {variant}", M, C, F32, variant, "cpu", 13, emulate=True)
    for _, M, C in SMALL_BF16:
        run_bwd_apply(None, f"bwd_apply bf16 M{M} C{C}", M, C, BF16, True, (), 1, "cpu", 21, emulate=True)
    for M, C, opts, two in APPLY_STRIDED[:30]:
        run_bwd_apply(None, f"bwd_apply bf16 {_aid((M, C, opts, two))}", M, C, BF16, two, opts, 49, "cpu", 23, emulate=True)
    for M, C, opts, two in APPLY_F32:
        run_bwd_apply(None, f"bwd_apply fp32 {_aid((M, C, opts, two))}", M, C, F32, two, opts, 49, "cpu", 24, emulate=True)
    for case in REDUCE:
        dt, C, has_b, bcast, rep = case
        run_bwd_reduce(None, f"bwd_reduce {_rid(case)}", 245, C, dt, has_b, bcast, rep, "cpu", 31, emulate=True)
    run_bwd_reduce(None, "bwd_reduce fp32 C256 M4099", 4099, 256, F32, True, False, 4, "cpu", 32, emulate=True)
    for rep in (1, 5, 64):
        for C in (65, 512):
            for count in COUNTS:
                d = finalize_inputs(rep, C, count, 50 + rep)
                ref, var, ex2 = finalize_ref(d["s"], d["ss"], count, d["gamma"], d["beta"], d["rm"], d["rv"])
                bnd = finalize_bounds(ref, var, ex2, count, d["gamma"], d["beta"], d["rm"], d["rv"], rep)
                emu = finalize_emulate(d["S"].sum(0), d["SS"].sum(0), count, d["gamma"], d["beta"], d["rm"], d["rv"])
                for n in ref:
                    gate(f"emulated bn_finalize rep {rep} C {C} count {count} {n}", "stats", 2e-5, emu[n], ref[n], bnd[n])
    for C in CS:
        gamma, beta, rm, rv = eval_inputs(C, 70)
        ref, bnd = eval_ref(gamma, beta, rm, rv)
        inv = 1.0 / torch.sqrt(rv + torch.tensor(BN_EPS, dtype=F32))
        gate(f"emulated bn_eval_coeffs C {C} scale", "stats", 2e-5, gamma * inv, ref["scale"], bnd["scale"])
        gate(f"emulated bn_eval_coeffs C {C} shift", "stats", 2e-5, beta - rm * gamma * inv, ref["shift"], bnd["shift"])
        s = side_inputs(C, 245, gen_for("cpu", 80))
        refs, bnds = coef_bounds(s, 245)
        for q, (got, n) in enumerate(zip(coef_emulate(s, 245), "kbc")):
            gate(f"emulated bn_bwd_coef C {C} {n}", "stats", 2e-5, got, refs[q], bnds[q])
    for R in L2_R:
        for E in L2_E:
            x, dy = l2_inputs(R, E, 90)
            y, nrm = l2_fwd_emulate(x)
            yr, nr = l2_fwd_ref(x)
            c = l2_rounds(E) / 2 + 2
            gate(f"emulated l2norm_fwd R {R} E {E} norm", "l2norm", 2e-5, nrm, nr, c * EPS32 * nr)
            gate(f"emulated l2norm_fwd R {R} E {E} y", "l2norm", 2e-5, y, yr, (c + 2) * EPS32 * yr.abs())
            ref, S = l2_bwd_ref(y, nrm, dy, 1.75)
            dot = (y * dy).sum(1, keepdim=True)
            live = nrm[:, None] > L2_TINY
            dx = torch.tensor(1.75) * torch.where(live, (dy - y * dot) / nrm[:, None], dy / torch.tensor(L2_TINY))
            nb = (l2_rounds(E) + 5) * EPS32 * S
            gate(f"emulated l2norm_bwd R {R} E {E} dx", "l2norm", 2e-5, dx, ref, nb)
            gate(f"emulated l2norm_bwd R {R} E {E} dxT", "l2norm", tol(BF16), dx.to(BF16), ref, out_bound(BF16, ref, nb))
    for n in ADAM_N[:2] + (4099,):
        for step in (1, 2, 1000):
            for wd in (0.0, 0.01):
                d = adamw_inputs(n, step, wd, 100 + step)
                ref = adamw_ref(d)
                for q, got in zip("pmv", adamw_emulate(d)):
                    gate(f"emulated adamw n {n} step {step} wd {wd} {q}", "adamw", 2e-5, got, ref[q], ref["b" + q])
    print("worst emulated |err| / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())


# ---------------------------------------------------------------- argument checks
BAD_SHAPES = [(BF16, 16, 4, "C<chunk"), (F32, 16, 2, "C<chunk"), (BF16, 16, 12, "C%chunk"), (F32, 16, 6, "C%chunk"),
              (BF16, 16, 24, "256%cpr"), (F32, 16, 2048, "256%cpr"), (BF16, 16, 4096, "cpr>256"), (BF16, 0, 64, "M<1")]


@gpu
@pytest.mark.parametrize("case", BAD_SHAPES, ids=[f"{dtid(c[0])}-M{c[1]}-C{c[2]}" for c in BAD_SHAPES])
def test_streaming_passes_refuse_bad_shapes(ops, case):
    """A thread keeps chunk (thread % cpr) of every row it visits: C below one chunk (cpr = 0, a host
    division by zero before this check), a partial chunk, or a cpr that does not divide 256 is refused
    by vlp_bn_add_relu, vlp_bn_bwd_apply, vlp_bn_bwd_reduce, vlp_maxpool_bwd and vlp_maxpool_bwd_apply
    before any launch; so is M < 1.  Nothing is written."""
    dt, M, C, _ = case
    dev = "cuda"
    R = max(M, 16)
    t = lambda: torch.ones(R, C, device=dev, dtype=dt)
    v = lambda: torch.ones(C, device=dev)
    y, idt, dout = t(), t(), t()
    obuf, out = guarded(R, C, dt, dev)
    o2buf, out2 = guarded(R, C, dt, dev)
    sums = [stat_buf(1, C, dev) for _ in range(3)]
    with pytest.raises(RuntimeError):
        ops.bn_add_relu(y[:M], v(), v(), None, None, None, out[:M])
    with pytest.raises(RuntimeError):
        ops.bn_add_relu(y[:M], v(), v(), idt[:M], v(), v(), out[:M])
    A = (y, v(), v(), v(), sums[0], sums[1], out)
    B = (idt, v(), v(), v(), sums[0], sums[1], out2)
    with pytest.raises(RuntimeError):
        ops.bn_bwd_apply(M, C, dout, None, 1, None, A, None, None, y)
    with pytest.raises(RuntimeError):
        ops.bn_bwd_apply(M, C, dout, None, 1, y, A, B, out2, y)
    with pytest.raises(RuntimeError):
        ops.bn_bwd_reduce(M, C, dout, None, 1, y, y, v(), v(), idt, v(), v(), sums[0], sums[1], sums[2], y)
    # the stem passes: the same thread-to-chunk rule over an N x H x W x C tensor
    N, H = (0 if M < 1 else 1), 4
    y4 = torch.ones(max(N, 1), H, H, C, device=dev, dtype=dt)[:N]
    dp = torch.ones(max(N, 1), 2, 2, C, device=dev, dtype=dt)[:N]
    idx = torch.zeros(max(N, 1), 2, 2, C, device=dev, dtype=torch.uint8)[:N]
    d4buf = torch.full((H * H + GUARD, C), SENT, device=dev, dtype=dt)
    with pytest.raises(RuntimeError):
        ops.maxpool_bwd(dp, idx, y4, v(), v(), v(), v(), sums[0], sums[1])
    with pytest.raises(RuntimeError):
        ops.maxpool_bwd_apply(dp, idx, y4, v(), v(), v(), v(), v(), sums[0], sums[1], d4buf[:N * H * H].view(N, H, H, C))
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all().item()) and bool((o2buf == SENT).all().item()) and bool((d4buf == SENT).all().item())
    assert all(bool((s[:C] == 0).all().item()) and bool((s[C:] == SENT).all().item()) for s in sums)


@gpu
@pytest.mark.parametrize("dt", (BF16, F32), ids=dtid)
def test_bn_bwd_rejects_missing_operands(ops, dt):
    """vlp_bn_bwd_reduce reads mask, ya, mean_a, istd_a and one of dout / dbc unconditionally (and divides by
    HW with dbc); vlp_bn_bwd_apply reads side A and, when dy_b selects side B, yb.  Each missing one is
    refused on the host; nothing is written."""
    dev = "cuda"
    M, C = 32, 64
    t = lambda: torch.ones(M, C, device=dev, dtype=dt)
    v = lambda: torch.ones(C, device=dev)
    y, dout = t(), t()
    dbc = torch.ones(M // 4, C, device=dev)
    sums = [stat_buf(1, C, dev) for _ in range(3)]
    good = dict(dout=dout, dbc=None, HW=1, mask=y, ya=y, mean_a=v(), istd_a=v())

    def reduce(**kw):
        a = {**good, **kw}
        ops.bn_bwd_reduce(M, C, a["dout"], a["dbc"], a["HW"], a["mask"], a["ya"], a["mean_a"], a["istd_a"], None, None,
                          None, sums[0], sums[1], sums[2], y)

    for bad in (dict(mask=None), dict(ya=None), dict(mean_a=None), dict(istd_a=None), dict(dout=None),
                dict(dout=None, dbc=dbc, HW=0), dict(dout=None, dbc=dbc, HW=-4)):
        with pytest.raises(RuntimeError):
            reduce(**bad)
    obuf, out = guarded(M, C, dt, dev)
    o2buf, out2 = guarded(M, C, dt, dev)
    A = [y, v(), v(), v(), sums[0], sums[1], out]
    with pytest.raises(RuntimeError):   # null side A
        ops.bn_bwd_apply(M, C, dout, None, 1, None, None, None, None, y)
    with pytest.raises(RuntimeError):   # side A without its input
        ops.bn_bwd_apply(M, C, dout, None, 1, None, [None] + A[1:], None, None, y)
    with pytest.raises(RuntimeError):   # dy_b without yb
        ops.bn_bwd_apply(M, C, dout, None, 1, None, A, [None, v(), v(), v(), sums[0], sums[1], out2], None, y)
    with pytest.raises(RuntimeError):   # neither dout nor dbc
        ops.bn_bwd_apply(M, C, None, None, 1, None, A, None, None, y)
    with pytest.raises(RuntimeError):   # dbc with HW < 1
        ops.bn_bwd_apply(M, C, None, dbc, 0, None, A, None, None, y)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all().item()) and bool((o2buf == SENT).all().item())
    assert all(bool((s[:C] == 0).all().item()) and bool((s[C:] == SENT).all().item()) for s in sums)
