"""Every LayerNorm, embedding, scatter and text-attention route of csrc/bert_ops.hip per element
against fp64.

Method as tests/test_gpu_bn_routes.py: inputs are rounded to the storage dtype first, the
reference is plain fp64 of the defining formula on those same values, every output is
over-allocated and NaN-filled (integer data: a sentinel), every owned element must be finite and
inside a bound derived from the kernel's rounding points, the guard region must be untouched, and
inputs carry NaN rows past the last row the kernel may read.  u = 2^-24, r_T = 2^-8 (the bf16 unit roundoff) for bf16
storage / MFMA operands and 0 for fp32.

Routes and the case that reaches them
    LayerNorm, LN_DISPATCH (NCH = 16-byte chunks per lane, 16 lanes per row), M = 37:
        bf16 D   8 -> 1 chunk (NCH 1, 15 idle lanes), 128 NCH 1 full, 136 NCH 2, 312 NCH 3,
                 512 NCH 4, 520 5 -> NCH 6, 768 NCH 6, 776 7 -> NCH 8, 1024 NCH 8
        fp32 D   4 / 64 NCH 1, 68 NCH 2, 192 NCH 3, 256 NCH 4, 312 5 -> 6, 388 7 -> 8, 512 NCH 8,
                 516 9 -> 12, 768 NCH 12, 772 13 -> 16, 1024 NCH 16           test_ln_widths[dt-D]
    LayerNorm backward launch (ln_bwd_t; test_ln_bwd_routes[dt-D-M]):
        8-wave block, 32 rows per pass, cap 160 (D = 312): M 1, 31, 32, 33, 5120 (160 blocks, one
        pass), 5128 (grid-stride loop entered, 8 rows in the second pass)
        4-wave "wide rows" block, 16 rows per pass, cap 160 (D = 768: 16 NCH E > 512): M 16, 17,
        2560, 2566
        M > 65536 (D = 8 bf16, D = 4 fp32): 65536 keeps the 8-wave block at cap 160; 65537 takes
        the 4-wave block at cap 4096 = 65536 rows per pass, so block 0 alone walks a second row.
        The 8-wave block exists through the compile-time switch VLP_LNB_TEXT_WAVES = 8 (default).
    LayerNorm backward variants (test_ln_bwd_variants): plain, dxd + p_in, p_out (forward run with
        the same p / seed and checked against the same host mask), addend, addend + rscale (rps 37,
        one rscale entry 0), dgamma / dbeta onto non-zero values -- each at D = 312, M = 5128 and
        D = 768, M = 2566 (both past the grid cap), both dtypes.
    Embeddings: D 8 / 312 / 768 x B 1 / 3 / 5 (the batch loop strides by 4), ids all equal /
        repeats with id 0 and the last row, token types all 0 / all 1 / mixed / None with a table /
        no table.  scatter_rows: ldi != ldo, both above D.
    Text attention (ATTN_DISPATCH: TB = 3 for T <= 48 else 4, DP = 32 for dh <= 32 else 64), each
        instantiation at its smallest and largest T in both dtypes (ATTN_CASES), every T edge
        1 15 16 17 33 47 48 49 63 64 and dh edge 7 26 32 33 48 64; masks None / ones / ragged
        prefix / 1 0 1 ... / one valid key / one fully masked sequence; dropout at dh 26 and 64,
        T 17 / 47 and 49 / 63, with and without a mask.

Bounds (first order in u; no constant beyond the counted roundings)
    LayerNorm forward.  n = NCH E + 4 additions per row sum (lane chain + 4 DPP steps).
        e_mean = (n + 1) u sum|x| / D
        rel(var + eps) = (n + 6) u + e_mean^2 / (var + eps)   (x - mean 1, square 2, sum n, / D 1,
                         + eps 1, the compiler's possible fma only removes roundings; a wrong mean
                         enters the centred sum of squares only in second order)
        rel(rstd) = rel(var + eps) / 2 + 2 u    (rsqrtf taken as 1 ulp = 2 u: SUPPOSED, the ISA
                         and micro-architecture guides give no accuracy figure for v_rsq_f32)
        e_y = |g| rstd (e_mean + u |x - mean|) + |y - beta| (rel(rstd) + 2 u) + u |y|, then the
              dropout scale: s e_y + u |s y|; bf16 store: e + r_T (|ref| + e)
    LayerNorm backward (mean / rstd are given fp32 inputs; the reference uses the same values).
        xh = (x - mu) rs 2 roundings, g = dy s_out 1, gg = g gamma 1
        e_a = (n + 4) u sum|gg| / D; e_b = (n + 8) u sum|gg xh| / D
        e_d = rs (e_a + |xh| e_b + 5 u (|gg| + |a| + |xh b|)) + u |d|
        + addend: u |dx|; dxd: one more u |dxd| (dropout or rscale product)
        dgamma / dbeta (atomics, order free): n_c u (|init| + sum|terms|), n_c = rows per thread
        + 2 shuffles + waves + blocks (one atomic each) + 4 roundings per term.  n_c is about
        176 at the 160-block cap, tight enough to see one dropped row; at M = 65537 (4096
        blocks) it is about 4100, and a row dropped there is seen through the NaN-poisoned dx,
        not through dgamma / dbeta.
    Embedding forward: exact (asserted ==).  Gradients: n u (|init| + sum|terms|) with n = the
        number of additions that can reach the address (rows naming the id + 1; ceil(B / 4) + 5
        for a position; ceil(B / 4) + 4 + T for a token type).
    Text attention.  e_s = scale (dh + 1) u sum_d |q k| per score.  The fast exp is modelled as
        hardware exp2 at 1 ulp (SUPPOSED, as above) plus the rounding of its scaled argument:
        relative (1 + |x|) 2^-23, x = s - max; the subtraction adds u |x|.
        rel_j = e_s + 2 u (1 + |x|) + u |x|;  e_P = P (rel_j + sum_k P_k rel_k + (4 TB + 4) u)
        ctx: sum_j (e_P s + (u + r_T) P') |V| + TK u sum|P' V|, TK = 48 or 64 (fp32 accumulation
        over the padded key extent), then the store.
        Backward (P is a given fp32 input): e_dp = dh u sum|dO V|;
        e_dot = sum_j P (m e_dp + u |dP|) + (4 TB + 3) u sum|P dP|
        e_dS = P (m e_dp + u |dP| + e_dot + u |dP - dot|) + u |dS| + r_T |dS|
        dq = scale sum_j dS K: scale (sum e_dS |K| + TK u sum|dS K|) + u |dq|; dk likewise over
        queries; dv = sum_i P' dO: (u + r_T) sum|P' dO| + TK u sum|P' dO|; then the store.
    Exact (==): masked-key probabilities, dk / dv rows of masked keys, untouched embedding
    rows, the padding row of dwemb, scatter copies, and the dropout zeros of LayerNorm's y and
    dxd.  The attention kernels never write P' (the dropped probabilities), so their dropout
    zeros cannot be seen directly: every attention dropout case holds ctx, dq, dk and dv to the
    fp64 result under the exact host mask, and test_attn_dropout_rowsums makes ctx the row sums
    of P' alone.

Dropout reference: hash_uniform (csrc/common.h) re-implemented in numpy uint64 / float32 below;
every dropout case uses the exact host mask.  Seeds: 20240229 and 2^40 + 12345; p = 0.1, whose
float32 value 13421773 * 2^-27 is no multiple of 2^-24 (so u >= p is decided between two grid
points of the 24-bit uniform), and p = 0.3, whose float32 value 5033165 * 2^-24 is one (u == p
can occur and is kept).

`test_cpu_replay_*` (no gpu marker) replay each kernel's fp32 arithmetic in torch (fp32 sums, one
rounding per listed point, storage rounding at the end) at every shape of this file and hold the
replay to the same bounds.  Worst |err| / bound per tensor:
                     CPU replay | MI355X
    ln y             0.996 | 0.996     (bf16 figures approach 1 by construction: r_T |ref| is the
    ln mean          0.272 | 0.272      half ulp at the bottom of a binade)
    ln rstd          0.370 | 0.315
    ln dx            0.996 | 0.996
    ln dxd           0.996 | 0.996
    ln dgamma        0.272 | 0.136
    ln dbeta         0.211 | 0.112
    emb dwemb        0.533 | 0.533
    emb dpemb        0.328 | 0.328
    emb dtemb        0.212 | 0.201
    attn P           0.100 | 0.143
    attn ctx         0.817 | 0.817
    attn dq          0.800 | 0.800
    attn dk          0.704 | 0.704
    attn dv          0.668 | 0.668
The whole file runs in 9 s on an MI355X (134 tests, the slowest GPU case 0.34 s).

Mutations tried on a scratch copy of csrc/bert_ops.hip, each caught by the named case:
    variance loop's c < nch guard dropped               test_ln[widths-bf16-D8]
    row16_allsum without its last step                  test_ln[widths-bf16-D128]
    forward dropout index NCH*16*E instead of D         test_ln[variants-p_out-bf16-D312-M5128]
    backward row stride one wave short                  test_ln[routes-bf16-D312-M5128]
    part[] fold skipping the last wave                  test_ln[routes-bf16-D312-M32]
    rscale[row / rps] -> rscale[row / rps / 2] (the in-bounds form of rscale[row])
                                                        test_ln[variants-rs-bf16-D312-M5128]
    key bias read at the query's index                  test_attn[bf16-T48-dh64-B2H12-alternate]
    dropout index transposed                            test_attn[fp32-T49-dh26-B3H5-alternate-p0.3]
    d < dh store mask dropped (ctx)                     test_attn[bf16-T15-dh26-B3H5-prefix]
    b += 4 -> b += 3                                    test_embed[bf16-D8-B5-repeats-no_table]
    id == 0 skip removed                                test_embed[fp32-D8-B1-repeats-ones]
    D + c -> c in dtemb                                 test_embed[bf16-D8-B3-repeats-mixed]
Not catchable by a value test, by reading the code: M <= 65536 flipped, Tn <= 48 -> < 48 and
dh > 32 -> >= 32 only move a shape to the other instantiation, which computes it correctly too
(T = 48 fits the TB = 4 tile, dh = 32 fits DP = 64); the cases on both sides of each threshold
hold both instantiations to the bound.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests.routes_fp64 import (BF16, F32, F64, GUARD, U, check_into, drop_scale, dtid, epc, gpu_ops, hash_u,
                               nan_out, nan_tail, r_t, rnd, store_bound, take)

gpu = pytest.mark.gpu
WORST = {}          # worst |err| / bound per tensor family, this file's cases only
check = functools.partial(check_into, WORST)
SEED_A, SEED_B = 20240229, (1 << 40) + 12345


@pytest.fixture(scope="module")
def ops():
    return gpu_ops()


# ================================================================ LayerNorm
LN_D = {BF16: [8, 128, 136, 312, 512, 520, 768, 776, 1024],
        F32: [4, 64, 68, 192, 256, 312, 388, 512, 516, 768, 772, 1024]}
EPS_CYCLE = [1e-12, 1e-6, 1e-5]


def ln_nch(dt, D):
    c = -(-(D // epc(dt)) // 16)
    table = [1, 2, 3, 4, 6, 8] if dt == BF16 else [1, 2, 3, 4, 6, 8, 12, 16]
    return next(t for t in table if t >= c)


def ln_bwd_launch(dt, D, M):
    """(waves per block, blocks) as ln_bwd_t chooses them"""
    wide = 16 * ln_nch(dt, D) * epc(dt) > 512
    if not wide and M <= 65536:
        return 8, min(-(-M // 32), 160)
    return 4, min(-(-M // 16), 160 if M <= 65536 else 4096)


def ln_inputs(dt, M, D, eps, variant, seed):
    g = torch.Generator().manual_seed(seed)
    inp = dict(dt=dt, M=M, D=D, eps=eps, variant=variant)
    inp["x"] = (torch.randn(M, D, generator=g, dtype=F64) * 1.3
                + (torch.rand(M, 1, generator=g, dtype=F64) * 4 - 2)).to(dt)
    c = torch.arange(D, dtype=F64)
    inp["gamma"] = ((0.5 + torch.rand(D, generator=g, dtype=F64)) * (1 - 2 * (c % 2))).to(F32)
    inp["beta"] = rnd((D,), g, F32, 0.5)
    inp["dy"] = rnd((M, D), g, dt)
    inp["p_fwd"], inp["seed_fwd"] = 0.0, 0
    inp["p_out"], inp["seed_out"], inp["p_in"], inp["seed_in"] = 0.0, 0, 0.0, 0
    inp["dxd"] = False
    inp["addend"] = inp["rscale"] = None
    inp["rps"] = 1
    inp["dg0"] = torch.zeros(D, dtype=F32)
    inp["db0"] = torch.zeros(D, dtype=F32)
    if variant == "dxd_pin":
        inp["dxd"], inp["p_in"], inp["seed_in"] = True, 0.3, SEED_B
    elif variant == "p_out":
        inp["p_fwd"] = inp["p_out"] = 0.1
        inp["seed_fwd"] = inp["seed_out"] = SEED_B + 7
    elif variant in ("addend", "rs"):
        inp["addend"] = rnd((M, D), g, dt)
        if variant == "rs":
            inp["rps"] = 37
            rs = (torch.rand(-(-M // 37), generator=g, dtype=F64) + 1.0).to(F32)
            rs[1 % rs.numel()] = 0.0
            inp["rscale"], inp["dxd"] = rs, True
    elif variant == "accum":
        inp["dg0"], inp["db0"] = rnd((D,), g, F32, 3.0), rnd((D,), g, F32, 3.0)
    return inp


def ln_ref(inp):
    """fp64 reference and bounds; also the fp32 mean / rstd handed to the backward"""
    dt, M, D, eps = inp["dt"], inp["M"], inp["D"], inp["eps"]
    E, nch = epc(dt), ln_nch(dt, D)
    n = nch * E + 4
    x, gm, bt = inp["x"].double(), inp["gamma"].double(), inp["beta"].double()
    R = {}
    mean = x.mean(1, keepdim=True)
    xm = x - mean
    var = (xm * xm).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    e_mean = (n + 1) * U * x.abs().sum(1, keepdim=True) / D
    rel_rstd = 0.5 * ((n + 6) * U + e_mean ** 2 / (var + eps)) + 2 * U
    y0 = xm * rstd * gm + bt
    e_y = gm.abs() * rstd * (e_mean + U * xm.abs()) + (y0 - bt).abs() * (rel_rstd + 2 * U) + U * y0.abs()
    s = drop_scale(inp["seed_fwd"], M * D, inp["p_fwd"]).view(M, D)
    y = y0 * s
    R["y"] = (y, store_bound(s * e_y + (U * y.abs() if inp["p_fwd"] > 0 else 0.0), y, dt))
    R["mean"] = (mean[:, 0], e_mean[:, 0])
    R["rstd"] = (rstd[:, 0], (rstd * rel_rstd)[:, 0])
    inp["y_zero"] = s == 0
    # backward on the fp32 statistics a forward would have saved
    mu32, rs32 = mean.to(F32), rstd.to(F32)
    inp["mean32"], inp["rstd32"] = mu32[:, 0].contiguous(), rs32[:, 0].contiguous()
    mu, rs = mu32.double(), rs32.double()
    so = drop_scale(inp["seed_out"], M * D, inp["p_out"]).view(M, D)
    g = inp["dy"].double() * so
    xh = (x - mu) * rs
    gg = g * gm
    a = gg.mean(1, keepdim=True)
    b = (gg * xh).mean(1, keepdim=True)
    d = rs * (gg - a - xh * b)
    e_a = (n + 4) * U * gg.abs().sum(1, keepdim=True) / D
    e_b = (n + 8) * U * (gg * xh).abs().sum(1, keepdim=True) / D
    e_d = rs * (e_a + xh.abs() * e_b + 5 * U * (gg.abs() + a.abs() + (xh * b).abs())) + U * d.abs()
    dx, e_dx = d, e_d
    if inp["addend"] is not None:
        dx = d + inp["addend"].double()
        e_dx = e_d + U * dx.abs()
    R["dx"] = (dx, store_bound(e_dx, dx, dt))
    if inp["dxd"]:
        if inp["rscale"] is not None:
            k = inp["rscale"].double()[torch.arange(M) // inp["rps"]].view(M, 1)
            dxd, e_dxd = k * dx, k * e_dx
        else:
            si = drop_scale(inp["seed_in"], M * D, inp["p_in"]).view(M, D)
            dxd, e_dxd = d * si, si * e_d
            inp["dxd_zero"] = si == 0
        e_dxd = e_dxd + U * dxd.abs()
        R["dxd"] = (dxd, store_bound(e_dxd, dxd, dt))
    nw, blocks = ln_bwd_launch(dt, D, M)
    # additions that can reach one column: the thread's rows, 2 shuffles, the waves' fold, one atomic per
    # block, plus 4 roundings inside a term (loose at 4096 blocks: see the docstring)
    n_c = -(-M // (blocks * nw * 4)) + 2 + nw + blocks + 4
    tg = g * xh
    R["dgamma"] = (inp["dg0"].double() + tg.sum(0), n_c * U * (inp["dg0"].double().abs() + tg.abs().sum(0)))
    R["dbeta"] = (inp["db0"].double() + g.sum(0), n_c * U * (inp["db0"].double().abs() + g.abs().sum(0)))
    return R


def ln_replay(inp):
    """fp32 torch replay of layernorm_fwd_kernel / layernorm_bwd_kernel"""
    dt, M, D = inp["dt"], inp["M"], inp["D"]
    x, gm, bt = inp["x"].float(), inp["gamma"], inp["beta"]
    out = {}
    mean = x.sum(1, keepdim=True) / D
    dlt = x - mean
    rstd = torch.rsqrt((dlt * dlt).sum(1, keepdim=True) / D + torch.tensor(inp["eps"], dtype=F32))
    y = dlt * rstd * gm + bt
    if inp["p_fwd"] > 0:
        y = y * drop_scale(inp["seed_fwd"], M * D, inp["p_fwd"]).view(M, D).float()
    out["y"], out["mean"], out["rstd"] = y.to(dt), mean[:, 0], rstd[:, 0]
    mu, rs = inp["mean32"].view(M, 1), inp["rstd32"].view(M, 1)
    g = inp["dy"].float()
    if inp["p_out"] > 0:
        g = g * drop_scale(inp["seed_out"], M * D, inp["p_out"]).view(M, D).float()
    xh = (x - mu) * rs
    gg = g * gm
    a = gg.sum(1, keepdim=True) / D
    b = (gg * xh).sum(1, keepdim=True) / D
    d = rs * (gg * 1.0 - a - xh * b)
    dx = d + inp["addend"].float() if inp["addend"] is not None else d
    out["dx"] = dx.to(dt)
    if inp["dxd"]:
        if inp["rscale"] is not None:
            out["dxd"] = (inp["rscale"][torch.arange(M) // inp["rps"]].view(M, 1) * dx).to(dt)
        else:
            out["dxd"] = (d * drop_scale(inp["seed_in"], M * D, inp["p_in"]).view(M, D).float()).to(dt)
    out["dgamma"] = inp["dg0"] + (g * xh).sum(0)
    out["dbeta"] = inp["db0"] + g.sum(0)
    return out


def ln_device(ops, inp):
    dt, M, D, dev = inp["dt"], inp["M"], inp["D"], "cuda"
    x, dy = nan_tail(inp["x"], dev), nan_tail(inp["dy"], dev)
    gm, bt = inp["gamma"].to(dev), inp["beta"].to(dev)
    y = nan_out(M, D, dt, dev)
    mean = torch.full((M + GUARD,), float("nan"), dtype=F32, device=dev)
    rstd = torch.full((M + GUARD,), float("nan"), dtype=F32, device=dev)
    ops.layernorm_fwd(x, gm, bt, inp["eps"], y, mean, rstd, M, D, p=inp["p_fwd"], seed=inp["seed_fwd"])
    out = {"y": take("y", y, M), "mean": take("mean", mean, M), "rstd": take("rstd", rstd, M)}
    mu, rs = inp["mean32"].to(dev), inp["rstd32"].to(dev)
    dx = nan_out(M, D, dt, dev)
    dxd = nan_out(M, D, dt, dev) if inp["dxd"] else None
    dgb = torch.full((2, D + GUARD), float("nan"), dtype=F32, device=dev)
    dgb[0, :D], dgb[1, :D] = inp["dg0"].to(dev), inp["db0"].to(dev)
    dg, db = dgb[0], dgb[1]
    v = inp["variant"]
    if v in ("addend", "rs"):
        ad = nan_tail(inp["addend"], dev)
        ops.layernorm_bwd_add(dy, x, mu, rs, gm, ad, dx, dg, db, M, D, dxs=dxd,
                              rscale=inp["rscale"].to(dev) if v == "rs" else None, rps=inp["rps"])
    else:
        ops.layernorm_bwd(dy, x, mu, rs, gm, dx, dxd, dg, db, M, D, p_out=inp["p_out"],
                          seed_out=inp["seed_out"], p_in=inp["p_in"], seed_in=inp["seed_in"])
    torch.cuda.synchronize()
    out["dx"] = take("dx", dx, M)
    if dxd is not None:
        out["dxd"] = take("dxd", dxd, M)
    assert bool(torch.isnan(dgb[:, D:]).all().item()), "dgamma / dbeta: elements beyond D written"
    out["dgamma"], out["dbeta"] = dgb[0, :D].cpu(), dgb[1, :D].cpu()
    return out


def ln_check(tag, inp, R, out, side):
    for k, (ref, bound) in R.items():
        check(f"{tag} {k}", f"{side} ln {k}", out[k], ref, bound)
    if inp["p_fwd"] > 0:
        assert bool((out["y"][inp["y_zero"]] == 0).all()), f"{tag}: dropped y elements not exactly 0"
        assert bool((out["y"][~inp["y_zero"]].double().abs() > 0).float().mean() > 0.99)
    if "dxd_zero" in inp:
        assert bool((out["dxd"][inp["dxd_zero"]] == 0).all()), f"{tag}: dropped dxd elements not exactly 0"


def ln_cases():
    cases = []
    i = 0
    for dt in (BF16, F32):
        for D in LN_D[dt]:
            cases.append(pytest.param(dt, 37, D, EPS_CYCLE[i % 3], "plain", id=f"widths-{dtid(dt)}-D{D}"))
            i += 1
    for dt in (BF16, F32):
        for D, Ms in ((312, (1, 31, 32, 33, 5120, 5128)), (768, (16, 17, 2560, 2566))):
            for M in Ms:
                cases.append(pytest.param(dt, M, D, EPS_CYCLE[i % 3], "plain", id=f"routes-{dtid(dt)}-D{D}-M{M}"))
                i += 1
        for M in (65536, 65537):
            D = 8 if dt == BF16 else 4
            cases.append(pytest.param(dt, M, D, EPS_CYCLE[i % 3], "plain", id=f"routes-{dtid(dt)}-D{D}-M{M}"))
            i += 1
    for dt in (BF16, F32):
        for D, M in ((312, 5128), (768, 2566)):
            for v in ("dxd_pin", "p_out", "addend", "rs", "accum"):   # "plain": the routes cases above
                cases.append(pytest.param(dt, M, D, EPS_CYCLE[i % 3], v, id=f"variants-{v}-{dtid(dt)}-D{D}-M{M}"))
                i += 1
    return cases


LN_CASES = ln_cases()


@gpu
@pytest.mark.parametrize("dt,M,D,eps,variant", LN_CASES)
def test_ln(ops, dt, M, D, eps, variant):
    inp = ln_inputs(dt, M, D, eps, variant, 1000 + D + M)
    R = ln_ref(inp)
    ln_check(f"ln {dtid(dt)} M{M} D{D} {variant}", inp, R, ln_device(ops, inp), "dev")


def test_cpu_replay_ln():
    for c in LN_CASES:
        dt, M, D, eps, variant = c.values
        inp = ln_inputs(dt, M, D, eps, variant, 1000 + D + M)
        R = ln_ref(inp)
        ln_check(f"replay ln {c.id}", inp, R, ln_replay(inp), "cpu")


def test_cpu_dropout_share():
    """the host generator keeps 1 - p of n = 2^20 draws within 4 sigma, for both p and both seeds"""
    n = 1 << 20
    for p in (0.1, 0.3):
        for seed in (SEED_A, SEED_B):
            kept = float((hash_u(seed, np.arange(n, dtype=np.uint64)) >= np.float32(p)).mean())
            sigma = math.sqrt(p * (1 - p) / n)
            assert abs(kept - (1 - float(np.float32(p)))) < 4 * sigma, (p, seed, kept)
    # the first draws of seed 0 against an independent Python-integer splitmix64
    mask = (1 << 64) - 1
    for idx in range(8):
        z = (0 + 0x9E3779B97F4A7C15 * (idx + 1)) & mask
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        assert float(hash_u(0, [idx])[0]) == (z >> 40) * 2.0 ** -24


# ================================================================ embeddings and scatter
V = 50            # vocabulary rows
TN = 5            # positions
TT_KINDS = ["zeros", "ones", "mixed", "none_table", "no_table"]


def emb_cases():
    cases, i = [], 0
    for D in (8, 312, 768):
        for B in (1, 3, 5):
            for dt in (BF16, F32):
                ids_kind = "same" if i % 3 == 0 else "repeats"
                cases.append(pytest.param(dt, B, D, ids_kind, TT_KINDS[i % 5],
                                          id=f"{dtid(dt)}-D{D}-B{B}-{ids_kind}-{TT_KINDS[i % 5]}"))
                i += 1
    return cases


EMB_CASES = emb_cases()


def emb_inputs(dt, B, D, ids_kind, tt_kind, seed):
    g = torch.Generator().manual_seed(seed)
    M = B * TN
    if ids_kind == "same":
        ids = torch.full((M,), 7, dtype=torch.int64)
    else:
        pool = torch.tensor([0, V - 1, 3, 3, 11, 0, V - 1, 20, 11, 3], dtype=torch.int64)
        ids = pool[torch.randint(0, pool.numel(), (M,), generator=g)]
        ids[0], ids[M - 1] = V - 1, 0
    tt = {"zeros": torch.zeros(M, dtype=torch.int64), "ones": torch.ones(M, dtype=torch.int64),
          "mixed": (torch.arange(M) * 7 // 3) % 2, "none_table": None, "no_table": torch.ones(M, dtype=torch.int64)}[tt_kind]
    inp = dict(dt=dt, B=B, D=D, M=M, ids=ids, tt=tt, table=tt_kind != "no_table")
    inp["wemb"], inp["pemb"], inp["temb"] = rnd((V, D), g, F32), rnd((TN, D), g, F32), rnd((2, D), g, F32)
    inp["de"] = rnd((M, D), g, dt)
    inp["dw0"], inp["dp0"], inp["dt0"] = rnd((V, D), g, F32, 2.0), rnd((TN, D), g, F32, 2.0), rnd((2, D), g, F32, 2.0)
    return inp


def emb_ref(inp):
    B, D, M, ids = inp["B"], inp["D"], inp["M"], inp["ids"]
    ty = inp["tt"] if inp["tt"] is not None else torch.zeros(M, dtype=torch.int64)
    pos = torch.arange(M) % TN
    e = inp["wemb"][ids] + inp["pemb"][pos]          # fp32, the kernel's order
    if inp["table"]:
        e = e + inp["temb"][ty]
    R = {"e": e.to(inp["dt"])}
    de = inp["de"].double()
    hit = (ids != 0)
    dw = inp["dw0"].double().index_add(0, ids[hit], de[hit])
    aw = inp["dw0"].double().abs().index_add(0, ids[hit], de[hit].abs())
    cnt = torch.zeros(V, dtype=F64).index_add(0, ids[hit], torch.ones(int(hit.sum()), dtype=F64))
    R["dwemb"] = (dw, ((cnt + 1) * U).view(V, 1) * aw)
    R["dw_untouched"] = cnt == 0
    d3 = de.view(B, TN, D)
    R["dpemb"] = (inp["dp0"].double() + d3.sum(0), (-(-B // 4) + 5) * U * (inp["dp0"].double().abs() + d3.abs().sum(0)))
    if inp["table"]:
        sel = torch.stack([(ty == 0), (ty == 1)]).double()            # [2][M]
        R["dtemb"] = (inp["dt0"].double() + sel @ de,
                      (-(-B // 4) + 4 + TN) * U * (inp["dt0"].double().abs() + sel @ de.abs()))
        R["dt_untouched"] = sel.sum(1) == 0
    return R


def emb_replay(inp):
    B, D, M, ids = inp["B"], inp["D"], inp["M"], inp["ids"]
    ty = inp["tt"] if inp["tt"] is not None else torch.zeros(M, dtype=torch.int64)
    e = inp["wemb"][ids] + inp["pemb"][torch.arange(M) % TN]
    if inp["table"]:
        e = e + inp["temb"][ty]
    de = inp["de"].float()
    hit = ids != 0
    out = {"e": e.to(inp["dt"]), "dwemb": inp["dw0"].index_add(0, ids[hit], de[hit]),
           "dpemb": inp["dp0"] + de.view(B, TN, D).sum(0)}
    if inp["table"]:
        out["dtemb"] = inp["dt0"].clone()
        for k in (0, 1):
            if bool((ty == k).any()):
                out["dtemb"][k] += de[ty == k].sum(0)
    return out


def emb_device(ops, inp):
    dev, dt, D, M = "cuda", inp["dt"], inp["D"], inp["M"]
    ids = inp["ids"].to(dev)
    tt = inp["tt"].to(dev) if inp["tt"] is not None else None
    temb = inp["temb"].to(dev) if inp["table"] else None
    e = nan_out(M, D, dt, dev)
    ops.embed_fwd(ids, tt, inp["wemb"].to(dev), inp["pemb"].to(dev), temb, e, M, TN, D)
    dw, dp, dtb = nan_tail(inp["dw0"], dev), nan_tail(inp["dp0"], dev), nan_tail(inp["dt0"], dev)
    ops.embed_bwd(ids, tt, nan_tail(inp["de"], dev), dw, dp, dtb if inp["table"] else None, M, TN, D)
    torch.cuda.synchronize()
    out = {"e": take("e", e, M), "dwemb": take("dwemb", dw, V), "dpemb": take("dpemb", dp, TN)}
    if inp["table"]:
        out["dtemb"] = take("dtemb", dtb, 2)
    return out


def emb_check(tag, inp, R, out, side):
    assert torch.equal(out["e"], R["e"]), f"{tag}: embedding forward is not the exact fp32 sum, rounded once"
    for k in ("dwemb", "dpemb", "dtemb"):
        if k in R:
            check(f"{tag} {k}", f"{side} emb {k}", out[k], *R[k])
    assert torch.equal(out["dwemb"][R["dw_untouched"]], inp["dw0"][R["dw_untouched"]]), f"{tag}: untouched dwemb rows changed"
    assert torch.equal(out["dwemb"][0], inp["dw0"][0]), f"{tag}: the padding row of dwemb received a gradient"
    if "dtemb" in R:
        u = R["dt_untouched"]
        assert torch.equal(out["dtemb"][u], inp["dt0"][u]), f"{tag}: a token-type row no row names changed"


@gpu
@pytest.mark.parametrize("dt,B,D,ids_kind,tt_kind", EMB_CASES)
def test_embed(ops, dt, B, D, ids_kind, tt_kind):
    inp = emb_inputs(dt, B, D, ids_kind, tt_kind, 77 + D + B)
    emb_check(f"embed {dtid(dt)} D{D} B{B} {ids_kind} {tt_kind}", inp, emb_ref(inp), emb_device(ops, inp), "dev")


def test_cpu_replay_embed():
    for c in EMB_CASES:
        dt, B, D, ids_kind, tt_kind = c.values
        inp = emb_inputs(dt, B, D, ids_kind, tt_kind, 77 + D + B)
        emb_check(f"replay embed {c.id}", inp, emb_ref(inp), emb_replay(inp), "cpu")


@gpu
@pytest.mark.parametrize("dt", [BF16, F32], ids=dtid)
@pytest.mark.parametrize("D", [8, 312, 768])
def test_scatter_rows(ops, dt, D):
    """ldi = D + 8, ldo = D + 24: copied values bit-equal, gap columns and guard rows untouched"""
    dev, R, ldi, ldo = "cuda", 7, D + 8, D + 24
    g = torch.Generator().manual_seed(D)
    src = torch.full((R + GUARD, ldi), float("nan"), dtype=dt, device=dev)
    vals = rnd((R, D), g, dt)
    src[:R, :D] = vals.to(dev)
    dst = torch.full((R + GUARD, ldo), -1024.0, dtype=dt, device=dev)
    ops.scatter_rows(src, dst, R, D, ldi, ldo)
    torch.cuda.synchronize()
    got = dst.cpu()
    it = torch.int16 if dt == BF16 else torch.int32
    assert torch.equal(got[:R, :D].contiguous().view(it), vals.contiguous().view(it)), "copied values differ"
    assert bool((got[:R, D:] == -1024.0).all()) and bool((got[R:] == -1024.0).all()), "gap or guard written"


# ================================================================ text attention
# (T, dh, B, H); the comment names the instantiation <TB, DP> and why the case is there
ATTN_SHAPES = [
    (1, 7, 1, 1),      # <3, 32> smallest T, T = 1
    (48, 32, 3, 5),    # <3, 32> largest T, dh = 32 edge, T = 48 edge
    (1, 33, 1, 1),     # <3, 64> smallest T, dh = 33 edge
    (48, 64, 2, 12),   # <3, 64> largest T
    (49, 26, 3, 5),    # <4, 32> smallest T, T = 49 edge
    (64, 32, 1, 1),    # <4, 32> largest T
    (49, 33, 1, 1),    # <4, 64> smallest T
    (64, 64, 2, 12),   # <4, 64> largest T
    (15, 26, 3, 5), (16, 48, 1, 1), (17, 7, 2, 12), (33, 64, 1, 1), (47, 33, 3, 5), (63, 48, 3, 5), (63, 7, 1, 1),
]
MASKS = ["none", "ones", "prefix", "alternate", "one_key", "full_masked_seq"]


def attn_cases():
    cases = []
    for dt in (BF16, F32):
        for i, (T, dh, B, H) in enumerate(ATTN_SHAPES):
            cases.append(pytest.param(dt, T, dh, B, H, MASKS[i % 6], 0.0, 0,
                                      id=f"{dtid(dt)}-T{T}-dh{dh}-B{B}H{H}-{MASKS[i % 6]}"))
        for T, dh, mk, p, seed in ((47, 26, "prefix", 0.1, SEED_B), (63, 64, "none", 0.3, SEED_A),
                                   (17, 64, "none", 0.1, SEED_A), (49, 26, "alternate", 0.3, SEED_B)):
            cases.append(pytest.param(dt, T, dh, 3, 5, mk, p, seed, id=f"{dtid(dt)}-T{T}-dh{dh}-B3H5-{mk}-p{p}"))
    return cases


ATTN_CASES = attn_cases()


def make_mask(kind, B, T):
    if kind == "none":
        return None
    m = torch.ones(B, T, dtype=torch.int64)
    if kind == "prefix":
        for b in range(B):
            m[b, max(1, T - 1 - 3 * b - T // 3):] = 0
    elif kind == "alternate":
        m[:, 1::2] = 0
    elif kind == "one_key":
        m[:] = 0
        for b in range(B):
            m[b, (5 * b + T // 2) % T] = 1
    elif kind == "full_masked_seq":
        m[B - 1] = 0
        if B > 1:
            m[0, T // 2:] = 0
    return m


def attn_inputs(dt, T, dh, B, H, mk, p, seed, rs):
    g = torch.Generator().manual_seed(rs)
    Dm = H * dh
    inp = dict(dt=dt, T=T, dh=dh, B=B, H=H, p=p, seed=seed, mask=make_mask(mk, B, T))
    inp["qkv"] = rnd((B * T, 3 * Dm), g, dt)
    inp["dctx"] = rnd((B * T, Dm), g, dt)
    inp["scale"] = float(torch.tensor(1.0 / math.sqrt(dh), dtype=F32))
    return inp


def heads(t, B, T, H, dh):
    return t.view(B, T, H, dh).permute(0, 2, 1, 3)          # [B][H][T][dh]


def unheads(t, B, T, H, dh):
    return t.permute(0, 2, 1, 3).reshape(B * T, H * dh)


def attn_ref(inp):
    dt, T, dh, B, H, sc = inp["dt"], inp["T"], inp["dh"], inp["B"], inp["H"], inp["scale"]
    TB = 3 if T <= 48 else 4
    TK = 16 * TB if dt == F32 else -(-16 * TB // 32) * 32
    rT = r_t(dt)
    Dm = H * dh
    qkv = inp["qkv"].double()
    q, k, v = (heads(qkv[:, i * Dm:(i + 1) * Dm], B, T, H, dh) for i in range(3))
    s = q @ k.transpose(2, 3) * sc
    e_s = sc * (dh + 1) * U * (q.abs() @ k.abs().transpose(2, 3))
    if inp["mask"] is not None:
        valid = (inp["mask"] != 0).view(B, 1, 1, T).expand(B, H, T, T)
        dead = ~valid.any(3, keepdim=True)                   # HF: every key at finfo.min -> uniform
        s = torch.where(dead, torch.zeros_like(s), s)
        e_s = torch.where(dead, torch.zeros_like(e_s), e_s)
        live = valid | dead
    else:
        live = torch.ones(B, H, T, T, dtype=torch.bool)
    s = torch.where(live, s, torch.full_like(s, -float("inf")))
    mx = s.max(3, keepdim=True).values
    x = s - mx
    w = torch.exp(x)
    P = w / w.sum(3, keepdim=True)
    xa = torch.where(live, x.abs(), torch.zeros_like(x))
    rel = torch.where(live, e_s + 2 * U * (1 + xa) + U * xa, torch.zeros_like(x))
    e_P = P * (rel + (P * rel).sum(3, keepdim=True) + (4 * TB + 4) * U)
    R = {"P": (P, e_P), "P_zero": ~live}
    m = drop_scale(inp["seed"], B * H * T * T, inp["p"]).view(B, H, T, T)
    Pd = P * m
    ctx = Pd @ v
    e_ctx = (e_P * m + (U + rT) * Pd) @ v.abs() + TK * U * (Pd @ v.abs())
    ctx2 = unheads(ctx, B, T, H, dh)
    R["ctx"] = (ctx2, store_bound(unheads(e_ctx, B, T, H, dh), ctx2, dt))
    # backward, on the fp32 probabilities a forward would have saved
    P32 = P.to(F32)
    inp["P32"] = P32.contiguous()
    Pb = P32.double()
    dO = heads(inp["dctx"].double(), B, T, H, dh)
    dPp = dO @ v.transpose(2, 3)
    e_dp = dh * U * (dO.abs() @ v.abs().transpose(2, 3))
    dP = dPp * m
    dot = (Pb * dP).sum(3, keepdim=True)
    e_dot = (Pb * (m * e_dp + U * dP.abs())).sum(3, keepdim=True) + (4 * TB + 3) * U * (Pb * dP).abs().sum(3, keepdim=True)
    dS = Pb * (dP - dot)
    e_dS = Pb * (m * e_dp + U * dP.abs() + e_dot + U * (dP - dot).abs()) + (U + rT) * dS.abs()
    dq = sc * (dS @ k)
    e_dq = sc * (e_dS @ k.abs() + TK * U * (dS.abs() @ k.abs())) + U * dq.abs()
    dk = sc * (dS.transpose(2, 3) @ q)
    e_dk = sc * (e_dS.transpose(2, 3) @ q.abs() + TK * U * (dS.abs().transpose(2, 3) @ q.abs())) + U * dk.abs()
    Pdb = Pb * m
    dv = Pdb.transpose(2, 3) @ dO
    e_dv = (U + rT + TK * U) * (Pdb.transpose(2, 3) @ dO.abs())
    for nme, val, err in (("dq", dq, e_dq), ("dk", dk, e_dk), ("dv", dv, e_dv)):
        v2 = unheads(val, B, T, H, dh)
        R[nme] = (v2, store_bound(unheads(err, B, T, H, dh), v2, dt))
    if inp["mask"] is not None:
        # keys masked in a sequence that has a valid key: probability 0 in every row, so dk = dv = 0
        mk = (inp["mask"] == 0) & (inp["mask"] != 0).any(1, keepdim=True)
        R["kv_zero_rows"] = mk.reshape(B * T)
    return R


def attn_replay(inp):
    dt, T, dh, B, H, sc = inp["dt"], inp["T"], inp["dh"], inp["B"], inp["H"], inp["scale"]
    Dm = H * dh
    qkv = inp["qkv"].float()
    q, k, v = (heads(qkv[:, i * Dm:(i + 1) * Dm], B, T, H, dh) for i in range(3))
    s = (q @ k.transpose(2, 3)) * torch.tensor(sc, dtype=F32)
    if inp["mask"] is not None:
        bias = torch.where(inp["mask"] == 0, torch.tensor(torch.finfo(F32).min), torch.tensor(0.0)).view(B, 1, 1, T)
        s = s + bias
    e = torch.exp(s - s.max(3, keepdim=True).values)
    P = e * (1.0 / e.sum(3, keepdim=True))
    m = drop_scale(inp["seed"], B * H * T * T, inp["p"]).view(B, H, T, T).float()
    out = {"P": P, "ctx": unheads(((P * m).to(dt).float() @ v), B, T, H, dh).to(dt)}
    Pb = inp["P32"]
    dO = heads(inp["dctx"].float(), B, T, H, dh)
    dP = (dO @ v.transpose(2, 3)) * m
    dS = (Pb * (dP - (Pb * dP).sum(3, keepdim=True))).to(dt).float()
    Pd = (Pb * m).to(dt).float()
    scf = torch.tensor(sc, dtype=F32)
    out["dq"] = unheads((dS @ k) * scf, B, T, H, dh).to(dt)
    out["dk"] = unheads((dS.transpose(2, 3) @ q) * scf, B, T, H, dh).to(dt)
    out["dv"] = unheads(Pd.transpose(2, 3) @ dO, B, T, H, dh).to(dt)
    return out


def attn_device(ops, inp):
    dev, dt, T, dh, B, H = "cuda", inp["dt"], inp["T"], inp["dh"], inp["B"], inp["H"]
    Dm, M = H * dh, B * T
    qkv, dctx = nan_tail(inp["qkv"], dev), nan_tail(inp["dctx"], dev)
    am = inp["mask"].to(dev) if inp["mask"] is not None else None
    ctx = nan_out(M, Dm, dt, dev)
    P = nan_out(B * H * T, T, F32, dev)
    ops.attn_fwd(qkv, am, ctx, P, B, T, H, dh, inp["scale"], p=inp["p"], seed=inp["seed"])
    dqkv = nan_out(M, 3 * Dm, dt, dev)
    ops.attn_bwd(qkv, inp["P32"].to(dev), dctx, dqkv, B, T, H, dh, inp["scale"], p=inp["p"], seed=inp["seed"])
    torch.cuda.synchronize()
    d = take("dqkv", dqkv, M)
    return {"P": take("P", P, B * H * T).view(B, H, T, T), "ctx": take("ctx", ctx, M),
            "dq": d[:, :Dm], "dk": d[:, Dm:2 * Dm], "dv": d[:, 2 * Dm:]}


def attn_check(tag, inp, R, out, side):
    for k in ("P", "ctx", "dq", "dk", "dv"):
        check(f"{tag} {k}", f"{side} attn {k}", out[k], *R[k])
    assert bool((out["P"][R["P_zero"]] == 0).all()), f"{tag}: a masked key has a non-zero probability"
    if "kv_zero_rows" in R:
        z = R["kv_zero_rows"]
        assert bool((out["dk"][z] == 0).all()) and bool((out["dv"][z] == 0).all()), f"{tag}: dk / dv of a masked key not 0"


@gpu
@pytest.mark.parametrize("dt,T,dh,B,H,mk,p,seed", ATTN_CASES)
def test_attn(ops, dt, T, dh, B, H, mk, p, seed):
    inp = attn_inputs(dt, T, dh, B, H, mk, p, seed, 31 * T + dh)
    attn_check(f"attn {dtid(dt)} T{T} dh{dh} B{B} H{H} {mk} p{p}", inp, attn_ref(inp), attn_device(ops, inp), "dev")


def test_cpu_replay_attn():
    for c in ATTN_CASES:
        dt, T, dh, B, H, mk, p, seed = c.values
        inp = attn_inputs(dt, T, dh, B, H, mk, p, seed, 31 * T + dh)
        attn_check(f"replay attn {c.id}", inp, attn_ref(inp), attn_replay(inp), "cpu")


@gpu
def test_attn_dropout_rowsums(ops):
    """ctx with every V = 1 is the row sum of P': the kept set is exactly the host mask's (index
    ((b H + h) T + i) T + j), and a transposed index would move the sums"""
    dt, T, dh, B, H, p, seed = F32, 49, 26, 2, 3, 0.3, SEED_B
    inp = attn_inputs(dt, T, dh, B, H, "none", p, seed, 5)
    Dm = H * dh
    inp["qkv"][:, :2 * Dm] = 0          # uniform P = 1 / T
    inp["qkv"][:, 2 * Dm:] = 1
    R = attn_ref(inp)
    out = attn_device(ops, inp)
    check("dropout rowsum ctx", "dev attn ctx", out["ctx"], *R["ctx"])
    m = drop_scale(seed, B * H * T * T, p).view(B, H, T, T)
    assert len(torch.unique((m != 0).sum(3))) > 3      # the rows differ, so the test can tell them apart


# ================================================================ refusals (nothing is launched)
@gpu
def test_refusals(ops):
    from vlp_amd._lib import HipError, lib, ptr
    dev = "cuda"
    L = lib()
    f = torch.zeros(64, 8, dtype=F32, device=dev)
    i64 = torch.zeros(64, dtype=torch.int64, device=dev)
    a, n = ptr(f), None

    def refused(fn, *args):
        with pytest.raises(HipError, match="hipError 1$"):
            fn(*args)

    # embeddings: M, Tn, D < 1, M % Tn, NULL pointers (Tn == 0 used to divide by zero on the host)
    for M, Tn, D in ((0, 4, 8), (8, 0, 8), (8, 4, 0), (9, 4, 8), (-4, 4, 8), (8, -4, 8)):
        refused(L.vlp_embed_fwd, 0, M, Tn, D, ptr(i64), n, a, a, a, a, 0)
        refused(L.vlp_embed_bwd, 0, M, Tn, D, ptr(i64), n, a, a, a, a, 0)
    for k in range(4):
        args = [ptr(i64), a, a, a]
        args[k] = None
        refused(L.vlp_embed_fwd, 0, 8, 4, 8, args[0], n, args[1], args[2], a, args[3], 0)
        refused(L.vlp_embed_bwd, 0, 8, 4, 8, args[0], n, args[1], args[2], args[3], a, 0)
    L.vlp_embed_fwd(0, 8, 4, 8, ptr(i64), ptr(i64), a, a, n, a, 0)      # tt without a table: ignored
    # scatter_rows
    for R_, D, ldi, ldo in ((0, 8, 8, 8), (4, 0, 8, 8), (4, 8, 7, 8), (4, 8, 8, 7)):
        refused(L.vlp_scatter_rows, 0, R_, D, a, ldi, a, ldo, 0)
    refused(L.vlp_scatter_rows, 0, 4, 8, n, 8, a, 8, 0)
    refused(L.vlp_scatter_rows, 0, 4, 8, a, 8, n, 8, 0)
    # dropout probabilities outside [0, 1)
    for p in (1.0, 1.5, -0.1, float("nan")):
        refused(L.vlp_layernorm_fwd, 0, 8, 8, a, a, a, 1e-5, a, a, a, p, 0, 0)
        refused(L.vlp_layernorm_bwd, 0, 8, 8, a, p, 0, a, a, a, a, a, n, 0.0, 0, a, a, 0)
        refused(L.vlp_layernorm_bwd, 0, 8, 8, a, 0.0, 0, a, a, a, a, a, a, p, 0, a, a, 0)
        refused(L.vlp_attn_fwd, 0, 1, 4, 1, 8, a, n, a, a, 1.0, p, 0, 0)
        refused(L.vlp_attn_bwd, 0, 1, 4, 1, 8, a, a, a, a, 1.0, p, 0, 0)
    # NULL required pointers
    for k in range(6):
        args = [a] * 6
        args[k] = None
        refused(L.vlp_layernorm_fwd, 0, 8, 8, args[0], args[1], args[2], 1e-5, args[3], args[4], args[5], 0.0, 0, 0)
    for k in range(8):
        args = [a] * 8
        args[k] = None
        refused(L.vlp_layernorm_bwd, 0, 8, 8, args[0], 0.0, 0, args[1], args[2], args[3], args[4], args[5], n,
                0.0, 0, args[6], args[7], 0)
        refused(L.vlp_layernorm_bwd_add, 0, 8, 8, args[0], args[1], args[2], args[3], args[4], a, args[5],
                args[6], args[7], 0)
    for k in range(3):
        args = [a] * 3
        args[k] = None
        refused(L.vlp_attn_fwd, 0, 1, 4, 1, 8, args[0], n, args[1], args[2], 1.0, 0.0, 0, 0)
    for k in range(4):
        args = [a] * 4
        args[k] = None
        refused(L.vlp_attn_bwd, 0, 1, 4, 1, 8, args[0], args[1], args[2], args[3], 1.0, 0.0, 0, 0)
    # M < 1 in LayerNorm stays a no-op
    L.vlp_layernorm_fwd(0, 0, 8, n, n, n, 1e-5, n, n, n, 0.0, 0, 0)
    L.vlp_layernorm_bwd(0, 0, 8, n, 0.0, 0, n, n, n, n, n, n, 0.0, 0, n, n, 0)
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((i64 == 0).all())


def test_zz_worst_ratios():
    """prints the table's figures (the maximum over whatever ran in this process)"""
    for k in sorted(WORST):
        print(f"WORST {k:24s} {WORST[k]:.3f}")
        assert WORST[k] <= 1.0
