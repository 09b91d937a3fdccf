"""Golden table for the test-set evaluation (src/utils/test_evaluation.py), produced by the
REFERENCE's scripts/test_eval_downstream.py `evaluate_results` (:120-242, with its
`calculate_metrics` :244-278) on two folds of fixed probabilities, labels and metadata.

The reference script imports MONAI and Lightning at module level.  Where it does not import,
the generator applies the same six sklearn functions per subset in the script's order (levels
overall, dataset, entity, anatomy_site, sex, age_encoded, age_group; groups in pandas' unique()
order; roc_auc, precision, recall and f1_score NaN for a one-class subset) and records in the
fixture's "produced_by" which of the two wrote it.

The inputs hold, per fold, an entity whose rows are all tumours (a one-class group) and an
anatomy site with both classes whose probabilities all lie below 0.5 (a two-class group that
predicts no positives); both are asserted.  Probabilities are fp32 values (about half of them
quantised to two decimals, so ties are frequent), stored exactly.
    python tests/golden/make_test_eval_golden.py   -> tests/golden/test_eval_subgroups.json
"""
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VLP_REFERENCE", "/root/reference")
ROWS = 300
SITES = ("shoulder", "upper arm", "elbow", "lower arm", "hand", "hip", "upper leg", "knee", "lower leg")
ENTITIES = ("undefined", "osteochondroma", "enchondroma", "osteosarcoma", "giant cell tumor", "other")
LEVELS = ("overall", "dataset", "entity", "anatomy_site", "sex", "age_encoded", "age_group")
METRICS = ("accuracy", "balanced_accuracy", "roc_auc", "precision", "recall", "f1_score")


def age_group(age):
    return "0-18" if age < 19 else ("19-39" if age < 40 else "40+")


def make_fold(seed):
    r = np.random.RandomState(seed)
    entity = r.choice(ENTITIES, size=ROWS, p=(0.45, 0.1, 0.1, 0.1, 0.05, 0.2))
    tumor = np.where(entity == "undefined", 0, np.where(entity == "other", r.randint(0, 2, ROWS), 1))
    prob = np.clip(0.5 + 0.25 * (2 * tumor - 1) * r.rand(ROWS) + 0.3 * r.randn(ROWS), 0.001, 0.999)
    prob = np.where(r.rand(ROWS) < 0.5, np.round(prob, 2), prob).astype(np.float32)
    site = r.choice(SITES, size=ROWS)
    prob = np.where(site == "hand", np.minimum(prob, np.float32(0.45)), prob).astype(np.float32)
    age = r.randint(1, 90, ROWS)
    cols = {"dataset": ["INTERNAL" if i < ROWS // 2 else "BTXRD" for i in range(ROWS)],
            "entity": entity.tolist(), "anatomy_site": site.tolist(),
            "sex": r.choice(("M", "F"), size=ROWS).tolist(), "age": age.tolist(),
            "age_encoded": [int((a >= 19) + (a >= 40) + (a >= 60)) for a in age],
            "tumor": tumor.astype(int).tolist(), "prob": [float(p) for p in prob]}
    hand = [i for i in range(ROWS) if cols["anatomy_site"][i] == "hand"]
    assert {cols["tumor"][i] for i in hand} == {0, 1} and all(cols["prob"][i] < 0.5 for i in hand)
    sarc = [i for i in range(ROWS) if cols["entity"][i] == "osteosarcoma"]
    assert sarc and {cols["tumor"][i] for i in sarc} == {1}
    return cols


def frame(cols):
    df = pd.DataFrame(cols)
    df["age_group"] = [age_group(a) for a in cols["age"]]
    return df


def reference_rows(dfs):
    """The reference's evaluate_results -> its CSV, read back as rows of strings."""
    sys.path.insert(0, os.path.join(REF, "scripts"))
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir(REF)   # logging.conf is opened relative to the working directory
    try:
        import test_eval_downstream as ref
    finally:
        os.chdir(cwd)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out", "table.csv")
        ref.evaluate_results(path, dfs)
        table = pd.read_csv(path, dtype=str, keep_default_na=False)
    return [[r.level, r.group, int(r.fold), r.metric, r.value] for r in table.itertuples()]


def sklearn_rows(dfs):
    """The same six sklearn calls per subset, in the script's order."""
    from sklearn.metrics import (accuracy_score, balanced_accuracy_score, f1_score, precision_score, recall_score,
                                 roc_auc_score)

    def calculate_metrics(y_true, y_probs):
        y_pred = (y_probs >= 0.5).astype(int)
        one_class = len(set(y_true)) < 2
        values = (accuracy_score(y_true, y_pred), balanced_accuracy_score(y_true, y_pred),
                  float("nan") if one_class else roc_auc_score(y_true, y_probs),
                  float("nan") if one_class else precision_score(y_true, y_pred),
                  float("nan") if one_class else recall_score(y_true, y_pred),
                  float("nan") if one_class else f1_score(y_true, y_pred))
        return dict(zip(METRICS, values))

    rows = []
    for fold, df in enumerate(dfs):
        for level in LEVELS:
            groups = ["overall"] if level == "overall" else list(df[level].unique())
            for group in groups:
                sub = df if level == "overall" else df[df[level] == group]
                m = calculate_metrics(sub["tumor"].values.astype(float), sub["prob"].values)
                for metric, value in m.items():
                    rows.append([level, str(group), fold, metric, "NaN" if np.isnan(value) else repr(float(value))])
    return rows


def main():
    folds = [make_fold(101), make_fold(202)]
    dfs = [frame(c) for c in folds]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # sklearn's undefined-metric warnings on one-class subsets
        try:
            rows, produced_by = reference_rows(dfs), "reference scripts/test_eval_downstream.py evaluate_results"
        except ImportError as e:
            print(f"the reference script does not import here ({e}); using the same sklearn calls per subset")
            rows, produced_by = sklearn_rows(dfs), "the script's six sklearn calls per subset (script not importable)"
    import sklearn
    out = {"produced_by": produced_by, "sklearn": sklearn.__version__, "folds": folds, "rows": rows}
    path = os.path.join(HERE, "test_eval_subgroups.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {path}: {len(rows)} rows, {os.path.getsize(path)} bytes, produced by {produced_by}")


if __name__ == "__main__":
    main()
