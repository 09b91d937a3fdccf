"""CPU: the test-set evaluation's host side -- vlp_amd.metrics.grouped_binary_counts (CPU path),
subgroup_metrics_from_counts, src/utils/test_evaluation.py, DownstreamDataModule.test_dataloader
and the binding of csrc/groupmetric_ops.hip.

Tolerances.  The counts are integers: `==`.  accuracy, precision, recall and f1_score are one
fp64 division of exact integers on both sides (sklearn's, too, up to its own operation order):
1e-12.  balanced_accuracy is a mean of two such quotients: 1e-12.  roc_auc: sklearn's trapezoid
sums at most n fp64 terms of size at most 1, so its error is at most n 2^-53 (4.5e-13 at n = 4096),
while one miscounted pair moves the value by 1 / (n1 n0) >= 1e-6 at these sizes: 1e-9 absolute."""
import csv
import json
import math
import os
import subprocess
import warnings

import pytest
import torch

from tests.groupmetric_cases import NO_GROUP, adversarial_case, brute_counts, random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")
LIB = os.path.join(PKG, "vlp_amd", "libvlp_hip.so")
GOLD = os.path.join(ROOT, "tests", "golden", "test_eval_subgroups.json")
KEYS = ("accuracy", "balanced_accuracy", "roc_auc", "precision", "recall", "f1_score")
RATIO_TOL, AUC_TOL = 1e-12, 1e-9


@pytest.fixture(scope="module")
def M():
    from vlp_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def TE():
    from src.utils import test_evaluation
    return test_evaluation


def same(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or (not math.isnan(a) and not math.isnan(b) and abs(a - b) <= tol)


# ---------------- counts ----------------
def test_adversarial_case_holds_what_it_claims():
    s, y, c, G = adversarial_case()
    assert s.numel() == 40 and len(G) == 3 and set(s.tolist()) <= {0.125, 0.5, 0.625, 0.875}
    assert not (c[0] == 2).any()                                    # an empty declared group
    assert int((c[1] == 3).sum()) == 1                              # a single-row group
    in1 = y[c[1] == 1]
    assert (in1 == 1).any() and not (in1 == 0).any()                # a one-class group
    assert all((c[l] == NO_GROUP).any() for l in range(3)) and (y == 2).sum() == 3


def test_cpu_counts_equal_the_brute_force(M):
    s, y, c, G = adversarial_case()
    got = M.grouped_binary_counts(s, y, c, G)
    assert got.dtype == torch.int64 and got.shape == (sum(G), 6)
    assert got.tolist() == brute_counts(s, y, c, G)
    assert got[2].tolist() == [0] * 6                               # the empty declared group
    # int64 labels with a value outside {0, 1} count as uint8's 2
    y64 = torch.where(y == 2, torch.full_like(y, 7), y).long()
    assert torch.equal(M.grouped_binary_counts(s, y64, c, G), got)


@pytest.mark.parametrize("n,G", [(1, [1]), (257, [2, 5]), (300, [1, 2, 6, 9, 2, 4, 3])])
def test_cpu_counts_random(M, n, G):
    s, y, c, G = random_case(n, G, seed=3)
    assert M.grouped_binary_counts(s, y, c, G).tolist() == brute_counts(s, y, c, G)


def test_one_group_level_is_the_existing_accumulator(M):
    s, y, _, _ = random_case(500, [1], seed=5)
    acc = M.BinaryMetricsDevice()
    acc.update(s, y)
    codes = torch.zeros(1, 500, dtype=torch.uint8)
    assert M.grouped_binary_counts(s, y, codes, [1]).tolist() == [acc.counts()]


# ---------------- metrics vs sklearn ----------------
def sk_metrics(y_true, y_probs):
    """The reference's calculate_metrics (scripts/test_eval_downstream.py:244-278), restated call by call."""
    from sklearn.metrics import (accuracy_score, balanced_accuracy_score, f1_score, precision_score, recall_score,
                                 roc_auc_score)
    y_pred = (y_probs >= 0.5).astype(int)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = {"accuracy": accuracy_score(y_true, y_pred),
               "balanced_accuracy": balanced_accuracy_score(y_true, y_pred)}
        if len(set(y_true)) < 2:
            out.update(roc_auc=float("nan"), precision=float("nan"), recall=float("nan"), f1_score=float("nan"))
        else:
            out.update(roc_auc=roc_auc_score(y_true, y_probs), precision=precision_score(y_true, y_pred),
                       recall=recall_score(y_true, y_pred), f1_score=f1_score(y_true, y_pred))
    return out


def check_against_sklearn(M, s, y, c, G):
    counts = M.grouped_binary_counts(s, y, c, G).tolist()
    cell, seen = 0, 0
    for l, n_g in enumerate(G):
        for g in range(n_g):
            tp, fp, fn, tn, wins, ties = counts[cell]
            cell += 1
            m = (c[l] == g) & (y <= 1)
            if not m.any():
                continue
            got = M.subgroup_metrics_from_counts(tp, fp, fn, tn, 2 * wins + ties)
            want = sk_metrics(y[m].numpy().astype(float), s[m].double().numpy())
            assert tuple(got) == KEYS
            for k in KEYS:
                print(f"level {l} group {g} {k}: {got[k]!r} sklearn {want[k]!r}")
                assert same(got[k], float(want[k]), AUC_TOL if k == "roc_auc" else RATIO_TOL), (l, g, k)
            seen += 1
    return seen


def test_subgroup_metrics_vs_sklearn(M):
    s, y, c, G = adversarial_case()
    assert check_against_sklearn(M, s, y, c, G) == 8      # every cell but the empty group
    for n, Gs, seed in ((300, [1, 2, 6, 9], 1), (4096, [1, 3], 2)):
        s, y, c, G = random_case(n, Gs, seed=seed, quantised=seed == 1)
        check_against_sklearn(M, s, y, c, G)


def test_subgroup_metrics_rules(M):
    f = M.subgroup_metrics_from_counts
    # one class, labels [1, 1, 1], predictions [1, 0, 1]: sklearn 1.7.2 gives 2/3 (the class present)
    got = f(2, 0, 1, 0, 0)
    assert got["accuracy"] == 2 / 3 and got["balanced_accuracy"] == 2 / 3
    assert all(math.isnan(got[k]) for k in KEYS[2:])
    got = f(0, 1, 0, 3, 0)                                # negatives only
    assert got["accuracy"] == 0.75 and got["balanced_accuracy"] == 0.75 and math.isnan(got["roc_auc"])
    got = f(0, 0, 2, 3, 7)                                # two classes, nothing predicted positive
    assert got["precision"] == 0.0 and got["recall"] == 0.0 and got["f1_score"] == 0.0
    assert got["roc_auc"] == 7 / 12 and got["balanced_accuracy"] == 0.5 and got["accuracy"] == 0.6
    assert all(math.isnan(v) for v in f(0, 0, 0, 0, 0).values()) and tuple(f(0, 0, 0, 0, 0)) == KEYS
    # the training-time conventions stay as they were
    assert M.binary_metrics_from_counts(2, 0, 1, 0, 0)["auroc"] == 0.0
    assert M.balanced_accuracy(torch.tensor([1, 1, 1]), torch.tensor([1, 0, 1])) == pytest.approx(1 / 3)


# ---------------- golden: the reference's table ----------------
def test_golden_table(M, TE, tmp_path):
    gold = json.load(open(GOLD))
    assert gold["produced_by"]
    preds = [TE.predictions_from_table(f, torch.tensor(f["prob"], dtype=torch.float64).float())
             for f in gold["folds"]]
    for f, p in zip(gold["folds"], preds):                          # the stored probabilities are fp32 values
        assert p.probs.double().tolist() == f["prob"]
    out = tmp_path / "sub" / "table.csv"
    rows = TE.evaluate_results(str(out), preds)
    with open(out, newline="") as fh:
        table = list(csv.reader(fh))
    assert table[0] == ["level", "group", "fold", "metric", "value"]
    assert len(rows) == len(table) - 1 == len(gold["rows"])
    one_class = no_positive = 0
    for got, line, want in zip(rows, table[1:], gold["rows"]):
        assert [got[0], str(got[1]), got[2], got[3]] == want[:4] == [line[0], line[1], int(line[2]), line[3]]
        a, b, w = float(got[4]), float(line[4]), float(want[4])
        assert (line[4] == "NaN") == math.isnan(a) and same(a, b, 0.0)      # the file holds the returned value
        assert same(a, w, AUC_TOL if got[3] == "roc_auc" else RATIO_TOL), (want, a)
        one_class += got[3] == "roc_auc" and math.isnan(w)
        no_positive += got[3] == "precision" and w == 0.0
    assert one_class >= 1 and no_positive >= 1


# ---------------- the driver's host side ----------------
def test_level_codes_first_appearance_and_group_limit(TE):
    cols = {"dataset": ["B", "A", "B"], "entity": ["x", "x", "y"], "anatomy_site": ["knee", "hip", "knee"],
            "sex": ["F", "M", "F"], "age": [18, 19, 40], "age_encoded": [0, 1, 2], "tumor": [1, 0, 1]}
    p = TE.predictions_from_table(cols, torch.tensor([0.9, 0.2, 0.4]))
    assert p.groups == [["overall"], ["B", "A"], ["x", "y"], ["knee", "hip"], ["F", "M"], ["0", "1", "2"],
                        ["0-18", "19-39", "40+"]]
    assert p.codes.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 1, 0], [0, 1, 2], [0, 1, 2]]
    assert p.tumor.tolist() == [1, 0, 1] and p.codes.dtype == p.tumor.dtype == torch.uint8
    n = 256
    many = {"dataset": ["A"] * n, "entity": [f"e{i}" for i in range(n)], "anatomy_site": ["hip"] * n,
            "sex": ["F"] * n, "age": [30] * n, "age_encoded": [1] * n, "tumor": [0] * n}
    with pytest.raises(ValueError, match="more than 255 groups"):
        TE.predictions_from_table(many, torch.zeros(n))
    ok = {k: v[:255] for k, v in many.items()}
    assert len(TE.predictions_from_table(ok, torch.zeros(255)).groups[2]) == 255


# ---------------- data ----------------
TODAY = {"tumor", "dataset", "image_path", "anatomy_site_encoded", "age_encoded", "sex_encoded", "x-ray-u8"}
EXTRA = {"entity", "anatomy_site", "sex", "age"}


def test_test_dataloader(TE):
    from src.data import DownstreamDataModule as D
    dm = D.DownstreamDataModule(batch_size=16, num_workers=0, image_size=16, n_samples=20, n_val_samples=8,
                                n_test_samples=24)
    loader = dm.test_dataloader(0)
    assert len(loader.dataset) == 48
    batches = list(loader)
    assert [len(b["dataset"]) for b in batches] == [16, 16, 16]
    assert all(set(b) == TODAY | EXTRA for b in batches)
    names = [d for b in batches for d in b["dataset"]]
    assert names == ["INTERNAL"] * 24 + ["BTXRD"] * 24                 # concatenated, not shuffled
    again = list(dm.test_dataloader(0))
    for a, b in zip(batches, again):                                   # deterministic across calls
        assert torch.equal(a["x-ray-u8"], b["x-ray-u8"]) and torch.equal(a["tumor"], b["tumor"])
        assert a["entity"] == b["entity"] and torch.equal(a["age"], b["age"])
    other = next(iter(dm.test_dataloader(1)))                          # the fold selects the seed
    assert not torch.equal(other["x-ray-u8"], batches[0]["x-ray-u8"])
    vocab = {e for e, _ in D.ENTITIES}
    tumor_by_entity = {}
    for b in batches:
        assert b["age"].dtype == torch.long and b["x-ray-u8"].shape == (16, 1, 16, 16)
        for j in range(16):                                            # the metadata agrees with the encodings
            assert b["anatomy_site"][j] == D.ANATOMY_SITES[int(b["anatomy_site_encoded"][j].argmax())]
            assert b["sex"][j] == D.SEXES[int(b["sex_encoded"][j].argmax())]
            age = int(b["age"][j])
            assert int(b["age_encoded"][j].argmax()) == sum(age >= e for e in D.AGE_EDGES) and 0 < age < 120
            assert b["entity"][j] in vocab
            tumor_by_entity.setdefault(b["entity"][j], set()).add(int(b["tumor"][j]))
        for k in ("anatomy_site_encoded", "age_encoded", "sex_encoded"):
            assert torch.equal(b[k].sum(1), torch.ones(16))
    assert any(len(v) == 1 for v in tumor_by_entity.values())          # one-class entity groups occur
    assert {0, 1} <= set().union(*tumor_by_entity.values())
    levels = TE.batch_levels(batches[0])
    assert len(levels) == 7 and levels[0] == ["overall"] * 16 and set(levels[6]) <= {"0-18", "19-39", "40+"}
    capped = D.DownstreamDataModule(batch_size=16, num_workers=0, image_size=16, n_test_samples=24,
                                    try_with_only_n_samples=5)
    assert len(capped.test_dataloader(0).dataset) == 10
    assert [d for b in capped.test_dataloader(0) for d in b["dataset"]] == ["INTERNAL"] * 5 + ["BTXRD"] * 5
    fp32 = D.DownstreamDataModule(batch_size=4, num_workers=0, image_size=16, n_test_samples=4, upload="fp32")
    assert next(iter(fp32.test_dataloader(0)))["x-ray"].shape == (4, 3, 16, 16)
    # the train and validation batches keep exactly today's keys
    folds, _ = next(dm.get_cv_splits())
    assert set(next(iter(folds.train_dataloader()))) == TODAY
    assert all(set(next(iter(v))) == TODAY for v in folds.val_dataloader())


# ---------------- library and binding ----------------
def test_library_exports_and_host_checks():
    from vlp_amd import _lib, ops
    protos = _lib.parse_header()
    assert [a for _, a in protos["vlp_groupmetric_counts"]["args"]] == [
        "n", "scores", "labels", "L", "codes", "cell_base", "out", "ws", "ws_bytes", "stream"]
    assert [a for _, a in protos["vlp_groupmetric_ws_bytes"]["args"]] == ["n", "L", "cells", "bytes"]
    assert os.path.exists(LIB), "libvlp_hip.so is not built: run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"vlp_groupmetric_counts", "vlp_groupmetric_ws_bytes"} <= exported
    L = _lib.lib()
    assert L._dll.vlp_abi_version() == 3          # additive: the ABI version stays
    # the workspace query is host code: one [cells][6] int64 partial per workgroup
    assert ops.groupmetric_ws_bytes(1, 1, 1) == 48
    assert ops.groupmetric_ws_bytes(600, 7, 40) == 3 * 3 * 40 * 48
    for n, lv, cells in ((0, 1, 1), ((1 << 18) + 1, 1, 1), (8, 0, 1), (8, 9, 9), (8, 2, 1), (8, 1, 256)):
        with pytest.raises(_lib.HipError):
            ops.groupmetric_ws_bytes(n, lv, cells)


def test_host_wrapper_raises_before_the_library(monkeypatch):
    from vlp_amd import metrics, ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(ops, "lib", no_library)
    s, y = torch.rand(10), torch.zeros(10, dtype=torch.uint8)
    cases = [(s, y, torch.zeros(9, 10, dtype=torch.uint8), [1] * 9),          # L = 9
             (s, y, torch.zeros(1, 10, dtype=torch.uint8), [256]),           # G = 256
             (s, y, torch.zeros(1, 10, dtype=torch.uint8), [0]),
             (s, y[:9], torch.zeros(1, 10, dtype=torch.uint8), [1]),         # mismatched lengths
             (s, y, torch.zeros(1, 9, dtype=torch.uint8), [1]),
             (s, y, torch.zeros(2, 10, dtype=torch.uint8), [1]),
             (s, y, torch.zeros(0, 10, dtype=torch.uint8), [])]
    for args in cases:
        for fn in (ops.groupmetric_counts, metrics.grouped_binary_counts):
            with pytest.raises(ValueError):
                fn(*args)
