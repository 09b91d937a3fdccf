"""scikit-learn's own logistic regression on the linear-probe test cases, recorded once so that
the tests need no sklearn fit (and run where sklearn is absent).

    python tests/golden/make_logreg_golden.py

Writes tests/golden/logreg_sklearn.json.  Data: tests/logreg_ref.py::case for the three CPU cases
and the reference-sized one.  Per case:

  coef, intercept   LogisticRegression(tol=1e-12, max_iter=100000): L-BFGS run to its limit
  default           the reference's probe, LogisticRegression(max_iter=1000, solver="lbfgs"), on the
                    259-row validation draw: balanced_accuracy_score of predict, roc_auc_score of
                    predict_proba[:, 1], the predictions themselves, n_iter_, and the largest
                    coefficient difference from the tight fit

Both fits run with warnings turned into errors: neither may warn.  No CPU or GPU code of this
project runs.
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.logreg_ref import BIG, CASES, GOLDEN, case  # noqa: E402


def main():
    import sklearn
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import balanced_accuracy_score, roc_auc_score
    out = {"sklearn": sklearn.__version__, "cases": {}}
    for N, D, sep in CASES + [BIG]:
        x, y, xv, yv = case(N, D, sep)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            tight = LogisticRegression(tol=1e-12, max_iter=100000).fit(x, y)
            dflt = LogisticRegression(max_iter=1000, solver="lbfgs").fit(x, y)
        pred = dflt.predict(xv)
        diff = max(np.abs(dflt.coef_ - tight.coef_).max(), np.abs(dflt.intercept_ - tight.intercept_).max())
        out["cases"][f"{N}x{D}"] = {
            "sep": sep, "data_sum": float(x.astype(np.float64).sum()), "train_accuracy": float(tight.score(x, y)),
            "coef": [float(v) for v in tight.coef_[0]], "intercept": float(tight.intercept_[0]),
            "tight_n_iter": int(tight.n_iter_[0]),
            "default": {"balanced_accuracy": float(balanced_accuracy_score(yv, pred)),
                        "auroc": float(roc_auc_score(yv, dflt.predict_proba(xv)[:, 1])),
                        "pred": [int(v) for v in pred], "n_iter": int(dflt.n_iter_[0]),
                        "coef_diff_from_tight": float(diff)}}
        print(N, D, "tight iters", tight.n_iter_[0], "default iters", dflt.n_iter_[0], "coef diff", diff, flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
