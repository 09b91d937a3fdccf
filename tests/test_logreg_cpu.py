"""vlp_amd.metrics.logistic_regression (its CPU path, torch fp64), balanced_accuracy and
binary_auroc, against the numpy fp64 references of tests/logreg_ref.py and the recorded
scikit-learn fits of tests/golden/logreg_sklearn.json.  Runs anywhere.

Gates (none comes from the code under test):

  * the gradient at the returned coefficients, evaluated by logreg_ref.loss_grad: its largest
    entry is at most tol = 1e-8 (measured 1.7e-9, 1.0e-11, 3.2e-10);
  * |wb - wb*|_2 <= 2 |g_ref(wb)|_2 / lambda_min(H_ref(wb*)), the strong-convexity bound, with
    wb* from logreg_ref.optimum (gradient <= 1e-13) and lambda_min by eigvalsh (measured distance /
    bound: 3.3e-7 / 7.8e-6, 1.7e-9 / 7.6e-8, 3.3e-7 / 2.6e-4);
  * the largest coefficient difference from sklearn's L-BFGS run to its limit (tol=1e-12) is at
    most the sum of that bound for the returned coefficients and for the golden's own (both lie
    that close to wb*; measured 1.7e-6, 2.4e-6, 3.4e-6 against bounds of 1.3e-4, 4.7e-4, 1.6e-2);
  * on the two overlapping cases the validation predictions equal those of the reference's
    default LogisticRegression(max_iter=1000) one for one (smallest validation |z| 3.9e-2 and
    2.1e-2), so the balanced accuracy is equal; on the separable case the difference is printed and
    not gated: sklearn's tol=1e-4 stops 3.2 away from its own limit in the largest coefficient
    there (measured: 2 of 259 predictions differ, balanced accuracy 0.9551 here vs 0.9441, AUROC
    0.99163 vs 0.99169);
  * balanced_accuracy and binary_auroc equal sklearn.metrics to 1e-12, ties included; for a
    one-class y the recall of the absent class is 0 and the AUROC is 0.0 (BinaryMetrics' rule).
"""
import functools

import numpy as np
import pytest
import torch

from tests import logreg_ref as R

TOL = 1e-8


@functools.lru_cache(maxsize=None)
def reference(N, D, sep):
    """(x, y, xv, yv, wb*) of one case, computed once and shared (nobody writes to them)."""
    x, y, xv, yv = R.case(N, D, sep)
    return x, y, xv, yv, R.optimum(x, y)


@functools.lru_cache(maxsize=None)
def cpu_fit(N, D, sep):
    from vlp_amd import metrics as M
    x, y, _, _, _ = reference(N, D, sep)
    return M.logistic_regression(torch.from_numpy(x), torch.from_numpy(y), tol=TOL)


def check_coefficients(name, wb, N, D, sep):
    """The three coefficient gates of this file for wb [D + 1] (numpy fp64) on case (N, D, sep)."""
    x, y, _, _, ws = reference(N, D, sep)
    g = R.loss_grad(x, y, wb)[1]
    dist, bound = R.distance_bound(x, y, wb, ws)
    gold = R.golden_case(R.load_golden(), N, D)
    assert gold["data_sum"] == float(x.astype(np.float64).sum())
    wg = np.append(np.asarray(gold["coef"]), gold["intercept"])
    _, bound_g = R.distance_bound(x, y, wg, ws)
    diff = np.abs(wb - wg).max()
    print(f"{name} N={N} D={D}: |g|_inf {np.abs(g).max():.3e} (tol {TOL:.0e}); |wb - wb*| {dist:.3e} "
          f"(bound {bound:.3e}); max diff from tight sklearn {diff:.3e} (bound {bound + bound_g:.3e})")
    assert np.isfinite(wb).all()
    assert np.abs(g).max() <= TOL
    assert dist <= bound
    assert diff <= bound + bound_g


def check_default_sklearn(name, fit, M, xv_t, yv_t, N, D, sep, gate):
    """Validation metrics of `fit` beside the recorded default-sklearn probe's."""
    _, _, xv, yv, _ = reference(N, D, sep)
    dflt = R.golden_case(R.load_golden(), N, D)["default"]
    pred = fit.predict(xv_t)
    bacc = M.balanced_accuracy(yv_t, pred)
    auroc = M.binary_auroc(yv_t, fit.decision_function(xv_t))
    flips = int((pred.cpu().numpy() != np.asarray(dflt["pred"])).sum())
    zmin = float(fit.decision_function(xv_t).abs().min())
    print(f"{name} N={N} D={D}: {flips} of {len(yv)} predictions differ from default sklearn; balanced accuracy "
          f"{bacc:.6f} vs {dflt['balanced_accuracy']:.6f}, AUROC {auroc:.6f} vs {dflt['auroc']:.6f}; smallest |z| "
          f"{zmin:.2e}; default sklearn's largest coefficient is {dflt['coef_diff_from_tight']:.2e} from its limit")
    assert 0.0 <= bacc <= 1.0 and 0.0 <= auroc <= 1.0
    assert abs(bacc - R.balanced_accuracy(yv, pred.cpu().numpy())) <= 1e-12
    if gate:
        assert flips == 0 and abs(bacc - dflt["balanced_accuracy"]) <= 1e-12
    return bacc, auroc


@pytest.mark.parametrize("N,D,sep", R.CASES)
def test_coefficients(N, D, sep):
    fit = cpu_fit(N, D, sep)
    assert fit.converged_ and 1 <= fit.n_iter_ < 100
    assert fit.coef_.shape == (D,) and fit.coef_.dtype == torch.float64 and fit.intercept_.dim() == 0
    check_coefficients("cpu", np.append(fit.coef_.numpy(), float(fit.intercept_)), N, D, sep)


def test_the_third_case_is_separable_and_the_others_are_not():
    for i, (N, D, sep) in enumerate(R.CASES):
        x, y, _, _, ws = reference(N, D, sep)
        acc = ((R.scores(x, ws) > 0) == (y > 0.5)).mean()
        assert (acc == 1.0) == (i == 2), (N, D, acc)


@pytest.mark.parametrize("N,D,sep", R.CASES)
def test_against_default_sklearn(N, D, sep):
    from vlp_amd import metrics as M
    _, _, xv, yv, _ = reference(N, D, sep)
    check_default_sklearn("cpu", cpu_fit(N, D, sep), M, torch.from_numpy(xv), torch.from_numpy(yv), N, D, sep,
                          gate=(N, D, sep) != R.CASES[2])


def test_two_fits_are_equal():
    from vlp_amd import metrics as M
    x, y, _, _, _ = reference(*R.CASES[0])
    again = M.logistic_regression(torch.from_numpy(x), torch.from_numpy(y), tol=TOL)
    first = cpu_fit(*R.CASES[0])
    assert torch.equal(again.coef_, first.coef_) and torch.equal(again.intercept_, first.intercept_)


def test_metrics_equal_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    from vlp_amd import metrics as M
    rng = np.random.default_rng(7)
    for n, levels in ((259, None), (400, 7), (64, 2), (5, None)):
        y = (rng.random(n) < 0.3).astype(np.int64)
        y[:2] = (0, 1)
        score = rng.standard_normal(n) if levels is None else rng.integers(0, levels, n).astype(np.float64)
        pred = (score > np.median(score)).astype(np.int64)
        yt, st, pt = torch.from_numpy(y), torch.from_numpy(score), torch.from_numpy(pred)
        assert abs(M.binary_auroc(yt, st) - sk.roc_auc_score(y, score)) <= 1e-12
        assert abs(M.balanced_accuracy(yt, pt) - sk.balanced_accuracy_score(y, pred)) <= 1e-12
    assert abs(M.binary_auroc(torch.tensor([0, 1, 0, 1]), torch.zeros(4)) - 0.5) <= 1e-12   # every score tied


def test_metrics_on_one_class():
    from vlp_amd import metrics as M
    y = torch.ones(6, dtype=torch.long)
    pred = torch.tensor([1, 1, 1, 0, 0, 1])
    assert M.binary_auroc(y, torch.arange(6.0)) == 0.0
    assert M.balanced_accuracy(y, pred) == 0.5 * (4 / 6)          # the absent class's recall counts as 0
    assert M.balanced_accuracy(1 - y, pred) == 0.5 * (2 / 6)


def test_label_errors():
    from vlp_amd import metrics as M
    x = torch.randn(8, 3)
    with pytest.raises(ValueError, match="one class"):
        M.logistic_regression(x, torch.zeros(8))
    with pytest.raises(ValueError, match="one class"):
        M.logistic_regression(x, torch.ones(8, dtype=torch.long))
    with pytest.raises(ValueError, match="0 or 1"):
        M.logistic_regression(x, torch.tensor([0, 1, 2, 0, 1, 0, 1, 1]))
    with pytest.raises(ValueError, match="0 or 1"):
        M.logistic_regression(x, torch.tensor([0, 1, 0.5, 0, 1, 0, 1, 1]))
    with pytest.raises(ValueError):
        M.logistic_regression(x, torch.tensor([0, 1, 0, 0, 1, 0, 1, 1]), C=0.0)
    with pytest.raises(ValueError):
        M.logistic_regression(torch.randn(8, 2049), torch.tensor([0, 1, 0, 0, 1, 0, 1, 1]))


def test_max_iter_one_is_not_converged():
    from vlp_amd import metrics as M
    x, y, _, _, _ = reference(*R.CASES[0])
    fit = M.logistic_regression(torch.from_numpy(x), torch.from_numpy(y), max_iter=1)
    wb = np.append(fit.coef_.numpy(), float(fit.intercept_))
    f0 = R.loss_grad(x, y, np.zeros_like(wb))[0]
    assert fit.converged_ is False and fit.n_iter_ == 1
    assert abs(f0 - np.log(2.0)) <= 1e-15 and R.loss_grad(x, y, wb)[0] < f0
