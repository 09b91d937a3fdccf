"""GPU: the linear probe's kernels (vlp_logreg_pass and the four one-workgroup kernels), the device
path of vlp_amd.metrics.logistic_regression, LinearProbeCallback(fit="device") and the probe-based
experiment through src/train.py.  References: tests/logreg_ref.py (numpy fp64).

Limits of the pass modes, from u = 2^-53, the term counts and the device exp / log1p (at most 1 ulp
each in double precision by the HIP math API's table; 2 is allowed for here).  With
A_i(v) = sum_d |x_id v_d| + |v_D|:

  * a row dot of D + 1 terms in any order is within (D + 2) u A_i(v) of the exact one, so the kernel
    and numpy are within dt_i(v) = 2 (D + 2) u A_i(v) of each other (SCORES; measured error / limit
    at most 0.020 on an MI355X);
  * s = e / (1 + e)^2 has |ds / dt| <= s, and e, the sum, the square and the quotient add fewer than
    8 roundings: |s - s_ref| <= s_ref (dt_i(w) + 16 u) (measured / limit at most 0.114, at N = 1);
  * c = p - y has |dp / dt| <= 1/4: |c - c_ref| <= dc_i = dt_i(w) / 4 + 16 u; for the HVP,
    c = s t(q): dc_i = |t_i(q)| s_i (dt_i(w) + 16 u) + s_i dt_i(q) + 2 u |c_i|;
  * column j sums N products in blocks of 32 and the test adds the G partials: within
    2 (N + G + 2) u sum_i |c_i x_ij| of numpy's, plus sum_i |x_ij| dc_i (GRAD measured / limit at
    most 0.007, HVP 0.068);
  * the loss l = softplus(+-t) has |dl / dt| <= 1 and fewer than 4 roundings:
    sum_i (dt_i(w) + 8 u l_i) + 2 (N + G + 2) u sum_i l_i (measured / limit at most 0.002).

None of these comes from the kernels' output.  The folds (newton_begin, cg_step) equal a numpy fp64
evaluation in the documented order bit for bit; the two values that pass through a square root
(|g|_2 and the CG tolerance) are compared to 4 u, since only +, -, *, / are taken as correctly
rounded.  End to end the gates are those of tests/test_logreg_cpu.py (measured on an MI355X, the
three cases and N = 2051, D = 512: reference gradient 1.7e-9, 1.0e-11, 4.2e-10, 4.0e-9; distance
from the optimum 3.3e-7, 1.7e-9, 3.7e-7, 9.4e-5 within bounds of 7.8e-6, 7.6e-8, 4.1e-4, 1.1e-2;
device against the CPU path 6.3e-10, 3.9e-12, 2.8e-8, 1.8e-7; decision_function error / limit at
most 0.017).
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import logreg_ref as R
from tests.conftest import PKG, ROOT
from tests.test_logreg_cpu import TOL, check_coefficients, check_default_sklearn, cpu_fit, reference

pytestmark = pytest.mark.gpu

U = R.U
T = 1024   # kLrVecThreads
DOWNSTREAM = ["downstream_data.image_size=64", "downstream_data.n_samples=32", "downstream_data.n_val_samples=16",
              "downstream_data.batch_size=4", "downstream_data.num_workers=0"]
# tests/test_gpu_tsne.py's SIZE, but with the 16 training pairs and the default validation sets that the
# pretraining module's precision@15 asserts (12 and 4 rows are too few for it), as tests/test_gpu_train.py
SIZE = ["data.batch_size=4", "data.image_size=64", "data.n_samples=16", "data.num_workers=0",
        "trainer.max_epochs=2", "model.compute_dtype=fp32"]
PROBE = "pretrain/pretrain_resnet34_tinybert_mi355x_probe"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vlp_amd import ops as o
    return o


@pytest.fixture(scope="module")
def M():
    from vlp_amd import metrics
    return metrics


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def absdot(x, v):
    return np.abs(x.astype(np.float64)) @ np.abs(v[:-1]) + abs(v[-1])


def run_pass(ops, mode, xd, y, u, s=None, state=None):
    """(parts summed over the workgroups [D + 2], s, z) of one device pass; NaN-filled outputs."""
    N, D = xd.shape
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")   # noqa: E731
    parts, z = nan(ops.logreg_nparts(N), D + 2), nan(N)
    s = nan(N) if s is None else s
    ops.logreg_pass(mode, xd, None if y is None else dev(y), dev(u), s=s, parts=parts, z=z, state=state)
    return parts.cpu().numpy(), s, z.cpu().numpy()


# (1, 1); (70, 37): row and column tails within three workgroups; (257, 32): one row past eight full
# blocks; (130, 1027): D tail over many chunks, past 1024; (515, 384) through a view with ldx > D
@pytest.mark.parametrize("N,D,pad", [(1, 1, 0), (70, 37, 0), (257, 32, 0), (130, 1027, 0), (515, 384, 64)])
def test_pass_modes_vs_fp64(ops, N, D, pad):
    x, y = R.features(N, D, 11, 1.5)
    rng = np.random.default_rng(N + D)
    w = np.append(rng.standard_normal(D) / np.sqrt(D), 0.3)
    q = np.append(rng.standard_normal(D), -0.7)
    xd = dev(np.pad(x, ((0, 0), (0, pad))))[:, :D] if pad else dev(x)
    assert xd.stride(0) == D + pad or N == 1
    G = ops.logreg_nparts(N)
    xa = np.abs(x.astype(np.float64))
    dtw, dtq = 2 * (D + 2) * U * absdot(x, w), 2 * (D + 2) * U * absdot(x, q)
    sum_u = 2 * (N + G + 2) * U

    z = run_pass(ops, ops.LOGREG_SCORES, xd, None, w)[2]
    zr = R.scores(x, w)
    e_z = (np.abs(z - zr) / dtw).max()

    parts, s_dev, _ = run_pass(ops, ops.LOGREG_GRAD, xd, y, w)
    l, p, s = R.row_terms(zr, y)
    c = p - y
    s_got = s_dev.cpu().numpy()
    e_s = (np.abs(s_got - s) / (s * (dtw + 16 * U))).max()
    gref = np.append(x.astype(np.float64).T @ c, c.sum())
    dc = dtw / 4 + 16 * U
    lim_g = np.append(xa.T @ dc + sum_u * (xa.T @ np.abs(c)), dc.sum() + sum_u * np.abs(c).sum())
    got = parts.sum(0)
    e_g = (np.abs(got[:D + 1] - gref) / lim_g).max()
    lim_l = (dtw + 8 * U * l).sum() + sum_u * l.sum()
    e_l = abs(got[D + 1] - l.sum()) / lim_l

    lparts = run_pass(ops, ops.LOGREG_LOSS, xd, y, w)[0]
    assert np.isnan(lparts[:, :D + 1]).all()                 # LOSS writes the last entry only
    assert np.array_equal(lparts[:, D + 1], parts[:, D + 1])

    hparts = run_pass(ops, ops.LOGREG_HVP, xd, None, q, s=s_dev)[0]
    tq = R.scores(x, q)
    ch = s * tq
    href = np.append(x.astype(np.float64).T @ ch, ch.sum())
    dch = np.abs(tq) * s * (dtw + 16 * U) + s * dtq + 2 * U * np.abs(ch)
    lim_h = np.append(xa.T @ dch + sum_u * (xa.T @ np.abs(ch)), dch.sum() + sum_u * np.abs(ch).sum())
    hgot = hparts.sum(0)
    e_h = (np.abs(hgot[:D + 1] - href) / lim_h).max()
    print(f"N={N} D={D} ldx={D + pad}: error / limit: scores {e_z:.3f}, s {e_s:.3f}, GRAD columns {e_g:.3f}, "
          f"loss {e_l:.3f}, HVP columns {e_h:.3f}")
    assert np.isfinite(got).all() and np.isfinite(hgot).all() and (hparts[:, D + 1] == 0).all()
    assert e_z <= 1 and e_s <= 1 and e_g <= 1 and e_l <= 1 and e_h <= 1

    zero = run_pass(ops, ops.LOGREG_HVP, xd, None, np.zeros(D + 1), s=s_dev)[0]
    assert (zero == 0).all()                                 # q = 0: exact zeros


def test_pass_at_scores_of_750(ops):
    N, D = 70, 37
    x, y = R.features(N, D, 12, 1.5)
    x[:, 0] = np.where(np.arange(N) % 3 == 0, -1.0, 1.0)     # z = +-750 exactly
    u = np.zeros(D + 1)
    u[0] = 750.0
    parts, s, _ = run_pass(ops, ops.LOGREG_GRAD, dev(x), y, u)
    z = R.scores(x, u)
    assert set(np.unique(z)) == {-750.0, 750.0}
    l, p, _ = R.row_terms(z, y)
    assert set(np.unique(p)) == {0.0, 1.0}
    got = parts.sum(0)
    assert np.isfinite(parts).all() and (s == 0).all()
    assert got[D + 1] == l.sum() == 750.0 * ((z > 0) != (y > 0.5)).sum()    # sums of 0 and 750: exact
    assert got[D] == (p - y).sum()                                           # p is exactly 0 or 1
    c = p - y                                                                # in {-1, 0, 1}: only the sums round
    lim = 2 * (N + ops.logreg_nparts(N) + 2) * U * (np.abs(x.astype(np.float64)).T @ np.abs(c))
    assert (np.abs(got[:D] - x.astype(np.float64).T @ c) <= lim).all()


# ---- the folds: numpy in the kernels' order ----
def strided(a):
    """Thread t's sum of a[t], a[t + 1024], ... in order, for the 1024 threads."""
    K = -(-len(a) // T)
    padded = np.zeros(K * T)
    padded[:len(a)] = a
    acc = np.zeros(T)
    for k in range(K):
        acc = acc + padded[k * T:(k + 1) * T]
    return acc


def tree(acc):
    r, o = acc.copy(), T // 2
    while o > 0:
        r[:o] = r[:o] + r[o:2 * o]
        o //= 2
    return r[0]


def fold(parts, N):
    acc = np.zeros(parts.shape[1])
    for g in range(parts.shape[0]):
        acc = acc + parts[g]
    return acc / N


def np_begin(parts, w, N, D, C, tol):
    lam = 1.0 / (C * N)
    g = fold(parts, N)[:D + 1]
    g[:D] = g[:D] + lam * w[:D]
    rs = tree(strided(g * g))
    gmax = np.abs(g).max()                                   # a maximum is the same in any order
    f = tree(strided(parts[:, D + 1])) / N + 0.5 * lam * tree(strided(np.append(w[:D] * w[:D], 0.0)))
    gn = np.sqrt(rs)
    state = [f, gmax, 0.0, None, 0.0, None, rs, min(0.5, np.sqrt(gn)) * gn, float(gmax <= tol or rs == 0.0), gn]
    return np.stack([g, np.zeros_like(g), -g, -g]), state


def np_cg_step(parts, vec, state, N, D, C):
    if state[8]:
        return vec, state
    lam = 1.0 / (C * N)
    g, d, r, q = vec
    hq = fold(parts, N)[:D + 1]
    hq[:D] = hq[:D] + lam * q[:D]
    alpha = state[6] / tree(strided(q * hq))
    d, r = d + alpha * q, r - alpha * hq
    rs = tree(strided(r * r))
    gd = tree(strided(g * d))
    q = r + (rs / state[6]) * q
    out = list(state)
    out[2], out[4], out[6] = gd, state[4] + 1.0, rs
    out[8] = float(np.sqrt(rs) <= state[7])
    return np.stack([g, d, r, q]), out


def same_state(got, want):
    exact = [i for i, v in enumerate(want) if v is not None and i not in (7, 9)]
    return (all(got[i] == want[i] for i in exact)
            and all(abs(got[i] - want[i]) <= 4 * U * abs(want[i]) for i in (7, 9)))


# L = D + 1 of 38 (one entry per thread), 1028 (two for a few threads), 2049 (three); G = 3, 5, 2
@pytest.mark.parametrize("N,D", [(70, 37), (130, 1027), (40, 2048)])
def test_folds_equal_numpy_bit_for_bit(ops, N, D):
    rng = np.random.default_rng(D)
    G, C = ops.logreg_nparts(N), 0.7
    # a small gradient, so that the CG tolerance |g|^1.5 lies well below the residuals of two steps
    parts = 1e-6 * rng.standard_normal((G, D + 2))
    parts[:, D + 1] = 1e6 * np.abs(parts[:, D + 1])
    w = 1e-5 * rng.standard_normal(D + 1)
    vec = torch.full((4, D + 1), float("nan"), dtype=torch.float64, device="cuda")
    state = torch.full((ops.LOGREG_STATE,), -1.0, dtype=torch.float64, device="cuda")
    ops.logreg_newton_begin(N, D, C, dev(parts), dev(w), 1e-12, vec, state)
    vref, sref = np_begin(parts, w, N, D, C, 1e-12)
    assert np.array_equal(vec.cpu().numpy(), vref) and same_state(state.tolist(), sref)
    assert state[8] == 0 and state[3] == -1 and state[5] == -1          # untouched by begin
    for step in range(2):
        q = vref[3]
        hparts = np.zeros((G, D + 2))
        # Hq = a positive diagonal times q: positive curvature, and a residual that stays live
        hparts[:, :D + 1] = rng.uniform(0.5, 1.5, (G, D + 1)) * q * N / G
        ops.logreg_cg_step(N, D, C, dev(hparts), vec, state)
        vref, sref = np_cg_step(hparts, vref, sref, N, D, C)
        assert np.array_equal(vec.cpu().numpy(), vref), step
        assert same_state(state.tolist(), sref) and state[4] == step + 1 and state[8] == 0
    # the trial point and its loss
    wt = torch.full((D + 1,), float("nan"), dtype=torch.float64, device="cuda")
    ops.logreg_trial(N, D, C, dev(w), 0.25, vec, wt, state)
    want = w + 0.25 * vref[1]
    lam = 1.0 / (C * N)
    pen = 0.5 * lam * tree(strided(np.append(want[:D] * want[:D], 0.0)))
    assert np.array_equal(wt.cpu().numpy(), want) and state[5] == pen
    ops.logreg_trial_loss(N, D, dev(parts), state)
    assert state[3] == tree(strided(parts[:, D + 1])) / N + pen


def test_begin_sets_done_at_the_tolerance_and_done_stops_the_budget(ops):
    N, D, C = 70, 37, 1.0
    x, y = R.features(N, D, 13, 1.5)
    rng = np.random.default_rng(5)
    G = ops.logreg_nparts(N)
    parts = 1e-9 * rng.standard_normal((G, D + 2))
    vec = torch.zeros(4, D + 1, dtype=torch.float64, device="cuda")
    state = torch.zeros(ops.LOGREG_STATE, dtype=torch.float64, device="cuda")
    ops.logreg_newton_begin(N, D, C, dev(parts), dev(np.zeros(D + 1)), 1e-8, vec, state)
    assert state[8] == 1 and 0 < state[1] <= 1e-8                        # converged: done at once
    # a live CG state, then the flag by hand: further pairs change nothing
    ops.logreg_newton_begin(N, D, C, dev(rng.standard_normal((G, D + 2))), dev(np.zeros(D + 1)), 1e-8, vec, state)
    assert state[8] == 0
    state[8] = 1.0
    before_v, before_s = vec.clone(), state.clone()
    s = torch.full((N,), 0.25, dtype=torch.float64, device="cuda")
    hp = torch.full((G, D + 2), float("nan"), dtype=torch.float64, device="cuda")
    for _ in range(3):
        ops.logreg_pass(ops.LOGREG_HVP, dev(x), None, vec[3], s=s, parts=hp, state=state)
        ops.logreg_cg_step(N, D, C, hp, vec, state)
    assert torch.equal(vec, before_v) and torch.equal(state, before_s) and torch.isnan(hp).all()
    state[8] = 0.0                                                       # and with it cleared they run
    ops.logreg_pass(ops.LOGREG_HVP, dev(x), None, vec[3], s=s, parts=hp, state=state)
    ops.logreg_cg_step(N, D, C, hp, vec, state)
    assert torch.isfinite(hp).all() and state[4] == 1 and not torch.equal(vec[1], before_v[1])


# ---- end to end ----
@pytest.fixture(scope="module")
def device_fits(M):
    out = {}
    for case in R.CASES + [R.BIG]:
        x, y, _, _, _ = reference(*case)
        out[case] = M.logistic_regression(dev(x), dev(y), tol=TOL)
    return out


@pytest.mark.parametrize("N,D,sep", R.CASES + [R.BIG])
def test_end_to_end(M, device_fits, N, D, sep):
    x, y, xv, yv, ws = reference(N, D, sep)
    fit = device_fits[(N, D, sep)]
    assert fit.converged_ and fit.coef_.is_cuda and fit.coef_.dtype == torch.float64 and fit.coef_.shape == (D,)
    wb = np.append(fit.coef_.cpu().numpy(), float(fit.intercept_))
    print(f"N={N} D={D}: {fit.n_iter_} outer iterations")
    check_coefficients("hip", wb, N, D, sep)
    cpu = cpu_fit(N, D, sep)
    wc = np.append(cpu.coef_.numpy(), float(cpu.intercept_))
    (_, b_dev), (_, b_cpu) = R.distance_bound(x, y, wb, ws), R.distance_bound(x, y, wc, ws)
    print(f"N={N} D={D}: device - CPU path {np.linalg.norm(wb - wc):.3e} (bound {b_dev + b_cpu:.3e})")
    assert np.linalg.norm(wb - wc) <= b_dev + b_cpu
    again = M.logistic_regression(dev(x), dev(y), tol=TOL)
    assert torch.equal(again.coef_, fit.coef_) and torch.equal(again.intercept_, fit.intercept_)
    assert again.n_iter_ == fit.n_iter_
    z = fit.decision_function(dev(xv))
    assert z.is_cuda and z.dtype == torch.float64
    err = np.abs(z.cpu().numpy() - R.scores(xv, wb)) / (2 * (D + 2) * U * absdot(xv, wb))
    print(f"N={N} D={D}: decision_function error / limit {err.max():.3f}")
    assert err.max() <= 1
    assert torch.equal(fit.predict(dev(xv)), (z > 0).long())
    check_default_sklearn("hip", fit, M, dev(xv), dev(yv), N, D, sep, gate=(N, D, sep) in R.CASES[:2])


def test_label_errors_on_device(M):
    x = torch.randn(8, 3, device="cuda")
    with pytest.raises(ValueError, match="one class"):
        M.logistic_regression(x, torch.zeros(8, device="cuda"))
    with pytest.raises(ValueError, match="0 or 1"):
        M.logistic_regression(x, torch.tensor([0, 1, 2, 0, 1, 0, 1, 1], device="cuda"))
    fit = M.logistic_regression(x, torch.tensor([0, 1, 0, 0, 1, 0, 1, 1], device="cuda"), max_iter=1)
    assert fit.converged_ is False and fit.n_iter_ == 1 and fit.loss_ < np.log(2.0)


def test_argument_errors_touch_nothing(ops):
    from vlp_amd._lib import HipError, lib, ptr
    L = lib()
    N, D = 40, 5
    G = ops.logreg_nparts(N)
    x = torch.ones(N, D, device="cuda")
    d = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")   # noqa: E731
    y, u, s, parts, z, vec, state, w, wt = d(N), d(D + 1), d(N), d(G, D + 2), d(N), d(4, D + 1), d(10), d(D + 1), d(D + 1)
    outs = (s, parts, z, vec, state, wt)
    p = ptr

    def passcall(mode=0, N=N, D=D, x=x, ldx=D, y=y, u=u, s=s, parts=parts, z=z):
        return lambda: L.vlp_logreg_pass(mode, N, D, p(x), ldx, p(y), p(u), p(s), p(parts), p(z), p(state), 0)

    bad = [passcall(N=0), passcall(D=0), passcall(D=2049), passcall(ldx=D - 1), passcall(mode=4), passcall(mode=-1),
           passcall(x=None), passcall(u=None), passcall(y=None), passcall(s=None), passcall(parts=None),
           passcall(mode=1, s=None), passcall(mode=2, y=None), passcall(mode=3, z=None),
           lambda: L.vlp_logreg_newton_begin(N, D, 0.0, p(parts), p(w), 1e-8, p(vec), p(state), 0),
           lambda: L.vlp_logreg_newton_begin(N, D, -1.0, p(parts), p(w), 1e-8, p(vec), p(state), 0),
           lambda: L.vlp_logreg_newton_begin(N, D, float("nan"), p(parts), p(w), 1e-8, p(vec), p(state), 0),
           lambda: L.vlp_logreg_newton_begin(0, D, 1.0, p(parts), p(w), 1e-8, p(vec), p(state), 0),
           lambda: L.vlp_logreg_newton_begin(N, 2049, 1.0, p(parts), p(w), 1e-8, p(vec), p(state), 0),
           lambda: L.vlp_logreg_newton_begin(N, D, 1.0, None, p(w), 1e-8, p(vec), p(state), 0),
           lambda: L.vlp_logreg_newton_begin(N, D, 1.0, p(parts), None, 1e-8, p(vec), p(state), 0),
           lambda: L.vlp_logreg_newton_begin(N, D, 1.0, p(parts), p(w), 1e-8, None, p(state), 0),
           lambda: L.vlp_logreg_newton_begin(N, D, 1.0, p(parts), p(w), 1e-8, p(vec), None, 0),
           lambda: L.vlp_logreg_cg_step(N, D, 0.0, p(parts), p(vec), p(state), 0),
           lambda: L.vlp_logreg_cg_step(N, 0, 1.0, p(parts), p(vec), p(state), 0),
           lambda: L.vlp_logreg_cg_step(N, D, 1.0, None, p(vec), p(state), 0),
           lambda: L.vlp_logreg_cg_step(N, D, 1.0, p(parts), None, p(state), 0),
           lambda: L.vlp_logreg_cg_step(N, D, 1.0, p(parts), p(vec), None, 0),
           lambda: L.vlp_logreg_trial(N, D, 0.0, p(w), 1.0, p(vec), p(wt), p(state), 0),
           lambda: L.vlp_logreg_trial(N, D, 1.0, None, 1.0, p(vec), p(wt), p(state), 0),
           lambda: L.vlp_logreg_trial(N, D, 1.0, p(w), 1.0, None, p(wt), p(state), 0),
           lambda: L.vlp_logreg_trial(N, D, 1.0, p(w), 1.0, p(vec), None, p(state), 0),
           lambda: L.vlp_logreg_trial(N, D, 1.0, p(w), 1.0, p(vec), p(wt), None, 0),
           lambda: L.vlp_logreg_trial_loss(0, D, p(parts), p(state), 0),
           lambda: L.vlp_logreg_trial_loss(N, D, None, p(state), 0),
           lambda: L.vlp_logreg_trial_loss(N, D, p(parts), None, 0)]
    for i, call in enumerate(bad):
        with pytest.raises(HipError, match="hipError 1$"):
            call()
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in outs)


# ---- the callback and src/train.py ----
def test_callback_on_device_beside_sklearn():
    """Both fits of the callback on the same module and loaders.  32 training rows of 512 features are
    separable, the case where L-BFGS's tol=1e-4 stops short (tests/test_logreg_cpu.py prints that
    difference and does not gate it): the default-sklearn values are printed beside the device's, and
    the gate is against sklearn run to its limit on the same features, whose validation predictions
    must be the same one for one (so the balanced accuracy is equal) and whose AUROC must agree to
    1e-9.  The optimum does not depend on the row order, so the shuffling train loader is no matter."""
    import functools
    from oracle import weights as W
    from src.data.DownstreamDataModule import DownstreamDataModule
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    from src.utils.LinearProbeCallback import LinearProbeCallback
    import types
    dm = DownstreamDataModule(batch_size=4, num_workers=0, image_size=64, n_samples=32, n_val_samples=16)
    fold, _ = next(dm.get_cv_splits())
    m = VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.AdamW, lr=5e-5),
                             False, False, 512, 312, 128, compute_dtype="fp32", text_dropout=0.0)
    W.apply_recipe(m, 0)
    got = {}
    for fit in ("device", "sklearn"):
        if fit == "sklearn":
            pytest.importorskip("sklearn")
        trainer = types.SimpleNamespace(current_epoch=0, sanity_checking=False, logged_metrics={})
        m.__dict__.pop("logged", None)
        LinearProbeCallback(fold.train_dataloader(), fold.val_dataloader(), every_n_epochs=5,
                            fit=fit).on_validation_start(trainer, m)
        keys = ("downstream_validation/linear_probe_balanced_accuracy", "downstream_validation/linear_probe_auroc")
        assert set(m.logged) == set(keys) == set(trainer.logged_metrics)
        got[fit] = [float(m.logged[k]) for k in keys]
        assert all(0.0 <= v <= 1.0 for v in got[fit]) and got[fit] == [trainer.logged_metrics[k] for k in keys]
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import balanced_accuracy_score, roc_auc_score
    cb = LinearProbeCallback(fold.train_dataloader(), fold.val_dataloader())
    enc = m.image_encoder.eval()
    Xt, yt = cb._extract_features(enc, cb.train_dataloader, m.device)
    Xv, yv = cb._extract_features(enc, cb.val_dataloader, m.device)
    tight = LogisticRegression(tol=1e-12, max_iter=100000).fit(Xt, yt)
    want = [balanced_accuracy_score(yv, tight.predict(Xv)), roc_auc_score(yv, tight.predict_proba(Xv)[:, 1])]
    print(f"(balanced accuracy, AUROC): device {got['device']}, sklearn to its limit {want}, "
          f"default sklearn {got['sklearn']}")
    assert abs(got["device"][0] - want[0]) <= 1e-12 and abs(got["device"][1] - want[1]) <= 1e-9
    with pytest.raises(ValueError, match="fit must be"):
        LinearProbeCallback(fold.train_dataloader(), fold.val_dataloader(), fit="gpu")


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
from src import train as T
from src.utils.config import compose
metrics, objs = T.train(compose("train", {args!r}))
assert not [m for m in sys.modules if m == "sklearn" or m.startswith("sklearn.")], "sklearn was imported"
ck = objs["trainer"].checkpoint_callback
assert ck.monitor == "downstream_validation/linear_probe_balanced_accuracy" and ck.mode == "max"
assert 0.0 <= ck.best_model_score <= 1.0
assert 0.0 <= metrics["downstream_validation/linear_probe_auroc"] <= 1.0
print("BEST", ck.best_model_path)
"""


def test_train_selects_the_checkpoint_on_the_device_probe(tmp_path):
    """The probe experiment through src/train.py in a fresh process (sys.modules shows what it imported)."""
    args = [f"experiment={PROBE}", f"paths.output_dir={tmp_path}", "linear_probe.every_n_epochs=1"] + SIZE + DOWNSTREAM
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, pkg=PKG, args=args)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    best = [l for l in r.stdout.splitlines() if l.startswith("BEST ")][0][5:]
    files = glob.glob(os.path.join(str(tmp_path), "**", "*.ckpt"), recursive=True)
    assert files == [best] and os.path.exists(best)
    name = os.path.basename(best)
    assert name.startswith("vlp-linear_probe_acc-epoch:") and "downstream_val_linear_probe_acc:" in name
    assert 0.0 <= float(name.rsplit(":", 1)[1][:-len(".ckpt")]) <= 1.0
