"""GPU: csrc/groupmetric_ops.hip (vlp_groupmetric_counts) through vlp_amd.metrics.grouped_binary_counts
and the test-set evaluation built on it (src/utils/test_evaluation.py, scripts/).

Agreement is `torch.equal` on int64 everywhere: the device compares fp32 scores and bytes and adds
integers, so every cell has one right value, and the CPU path (boolean masks in plain torch, held to
a Python brute force in tests/test_groupmetrics_cpu.py) is the reference.  Sizes: n = 1, 255, 256,
257 cross the 256-row i tile and the 256-row j tile; n = 600 runs three workgroups along i and three
splits of the j range.  The tables of the end-to-end tests are compared with `==` on the floats:
both sides divide the same integers."""
import ctypes
import functools
import math

import pytest
import torch

from tests.groupmetric_cases import adversarial_case, random_case

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 600]
SEVEN = [1, 2, 6, 9, 2, 4, 3]


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vlp_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def ops():
    from vlp_amd import ops as o
    return o


def check(M, s, y, c, G):
    want = M.grouped_binary_counts(s, y, c, G)
    got = M.grouped_binary_counts(s.cuda(), y.cuda(), c.cuda(), G)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == want.shape
    print(f"n={s.numel()} L={len(G)} cells={sum(G)} device sums {got.sum(0).tolist()} cpu {want.sum(0).tolist()}")
    assert torch.equal(got.cpu(), want)
    return got


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L", [1, 8])
def test_counts_equal_the_cpu_path(M, n, L):
    G = [3] if L == 1 else [1, 2, 6, 9, 2, 4, 3, 5]
    check(M, *random_case(n, G, seed=L))
    check(M, *random_case(n, G, seed=L + 10, quantised=False))


@pytest.mark.parametrize("n", [257, 600])
def test_seven_levels_and_a_level_of_255_groups(M, n):
    check(M, *random_case(n, SEVEN, seed=2))
    check(M, *random_case(n, [255], seed=3))
    check(M, *random_case(n, [2, 255, 1], seed=4, no_group_rate=0.0, skip_rate=0.0))


def test_adversarial_mix_and_equal_scores(M):
    got = check(M, *adversarial_case())
    assert got[2].tolist() == [0] * 6                      # the empty declared group
    s, y, c, G = random_case(600, SEVEN, seed=6)
    for v in (0.5, 0.25):                                   # all scores equal: every pair ties
        got = check(M, torch.full_like(s, v), y, c, G)
        assert int(got[:, 4].sum()) == 0 and int(got[0, 5]) > 0
    check(M, s, torch.ones_like(y), c, G)                   # positives only: no pairs
    check(M, s, torch.full_like(y, 2), c, G)                # nothing counted anywhere
    check(M, s, y, torch.full_like(c, 255), G)              # no row in any group


@pytest.mark.parametrize("n", SIZES + [5000])
def test_one_group_level_equals_binmetric_counts(M, ops, n):
    s, y, _, _ = random_case(n, [1], seed=8)
    acc = M.BinaryMetricsDevice()
    acc.update(s.cuda(), y.cuda())
    want = ops.binmetric_counts(n, acc._scores, acc._labels, acc._counts)
    codes = torch.zeros(1, n, dtype=torch.uint8, device="cuda")
    got = ops.groupmetric_counts(s.cuda(), y.cuda(), codes, [1])
    assert torch.equal(got, want[None])
    # and inside seven levels the same row comes back
    s7, y7, c7, G7 = random_case(n, SEVEN, seed=8)
    acc7 = M.BinaryMetricsDevice()
    acc7.update(s7.cuda(), y7.cuda())
    c7[0] = 0
    got7 = ops.groupmetric_counts(s7.cuda(), y7.cuda(), c7.cuda(), G7)
    assert torch.equal(got7[0], ops.binmetric_counts(n, acc7._scores, acc7._labels, acc7._counts))


def test_two_runs_give_identical_bits(M, ops):
    s, y, c, G = (t.cuda() if torch.is_tensor(t) else t for t in random_case(5000, SEVEN, seed=9))
    a = ops.groupmetric_counts(s, y, c, G)
    junk = torch.randint(0, 1 << 30, (1 << 20,), device="cuda")     # recycle the allocator's blocks in between
    del junk
    b = ops.groupmetric_counts(s, y, c, G)
    assert torch.equal(a, b)
    assert torch.equal(a.cpu(), M.grouped_binary_counts(s.cpu(), y.cpu(), c.cpu(), G))


def test_invalid_arguments_are_refused_before_any_launch(ops):
    from vlp_amd._lib import HipError, lib, ptr, stream_of
    n, G = 300, [2, 3]
    s, y, c, _ = (t.cuda() if torch.is_tensor(t) else t for t in random_case(n, G, seed=1))
    out = torch.full((5, 6), -1, dtype=torch.int64, device="cuda")
    nbytes = ops.groupmetric_ws_bytes(n, 2, 5)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")

    def base(*v):
        return ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)

    def call(n=n, scores=ptr(s), labels=ptr(y), L=2, codes=ptr(c), cb=(0, 2, 5), out_p=ptr(out), ws_p=ptr(ws),
             ws_bytes=nbytes):
        lib().vlp_groupmetric_counts(n, scores, labels, L, codes, base(*cb) if cb is not None else None, out_p, ws_p,
                                     ws_bytes, stream_of())

    bad = [dict(scores=None), dict(labels=None), dict(codes=None), dict(cb=None), dict(out_p=None), dict(ws_p=None),
           dict(n=0), dict(n=-1), dict(n=(1 << 18) + 1),
           dict(L=0, cb=(0,)), dict(L=9, cb=tuple(range(10))),
           dict(cb=(0, 0, 5)), dict(cb=(0, 256, 259)), dict(cb=(0, 3, 2)), dict(cb=(1, 3, 6)),
           dict(ws_bytes=nbytes - 8)]
    for kw in bad:
        with pytest.raises(HipError, match="hipError 1$"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == -1).all())                          # nothing was launched
    call()                                                  # the same arguments, valid: the op runs
    assert torch.equal(out, ops.groupmetric_counts(s, y, c, G))


# ---------------- end to end ----------------
DATA = dict(batch_size=16, num_workers=0, image_size=64, n_samples=32, n_val_samples=8, n_test_samples=24)
DATA_ARGV = ["--batch-size", "16", "--num-workers", "0", "--image-size", "64", "--n-test-samples", "24"]
KEYS = ("accuracy", "balanced_accuracy", "roc_auc", "precision", "recall", "f1_score")
LEVELS = ("overall", "dataset", "entity", "anatomy_site", "sex", "age_encoded", "age_group")


def canon(rows):
    """Rows with the value as its shortest round-trip text, so that NaN compares equal to NaN."""
    return [(lv, g, f, m, "NaN" if math.isnan(v) else repr(v)) for lv, g, f, m, v in rows]


def check_table(rows, folds):
    keys = [r[:4] for r in rows]
    assert len(set(keys)) == len(keys) and {r[2] for r in rows} == set(range(folds))
    for fold in range(folds):
        mine = [r for r in rows if r[2] == fold]
        assert [r[3] for r in mine[:6]] == list(KEYS) and mine[0][:2] == ("overall", "overall")
        order = list(dict.fromkeys(r[0] for r in mine))
        assert order == list(LEVELS)
        assert {r[1] for r in mine if r[0] == "dataset"} == {"INTERNAL", "BTXRD"}
        acc = [r[4] for r in mine if r[3] == "accuracy"]
        assert all(math.isfinite(a) and 0.0 <= a <= 1.0 for a in acc)
    return keys


@pytest.fixture(scope="module")
def TE():
    from src.utils import test_evaluation
    return test_evaluation


def make_model(kind):
    from src.models.baseline.FusionModule import FusionModule
    from src.models.baseline.OnlyImagingModule import OnlyImagingModule
    torch.manual_seed(3)
    opt = functools.partial(torch.optim.AdamW, lr=1e-3)
    return (OnlyImagingModule if kind == "imaging" else FusionModule)("resnet34", opt)


@pytest.mark.parametrize("kind", ["imaging", "fusion"])
def test_device_table_equals_the_cpu_table_and_the_script(M, TE, kind, tmp_path):
    from scripts import test_eval_downstream as script
    from src.data.DownstreamDataModule import DownstreamDataModule
    from src.utils.trainer import Trainer
    model = make_model(kind)
    model.train()
    dm = DownstreamDataModule(**DATA)
    pred = TE.collect_probs(model, dm.test_dataloader(0))
    assert model.training                                   # the caller's mode is restored
    assert pred.probs.is_cuda and pred.probs.dtype == torch.float32 and len(pred) == 48
    assert pred.codes.shape == (7, 48) and pred.codes.dtype == pred.tumor.dtype == torch.uint8
    assert bool(((pred.probs > 0) & (pred.probs < 1)).all())
    dev_rows = TE.evaluate_results(str(tmp_path / "dev.csv"), [pred])
    cpu_rows = TE.evaluate_results(str(tmp_path / "cpu.csv"), [pred.cpu()])
    assert canon(dev_rows) == canon(cpu_rows)
    assert (tmp_path / "dev.csv").read_text() == (tmp_path / "cpu.csv").read_text()
    check_table(dev_rows, 1)
    assert any(math.isnan(r[4]) for r in dev_rows if r[0] == "entity")      # one-class entity groups
    # the checkpoint round trip through the script: the same table, two folds from one checkpoint
    ckpt = str(tmp_path / f"{kind}.ckpt")
    Trainer(enable_checkpointing=False).save_checkpoint(ckpt, model)
    out = tmp_path / "script" / "table.csv"
    rows = script.main([str(out), ckpt, ckpt, "--save-predictions", str(tmp_path / "pred")] + DATA_ARGV)
    check_table(rows, 2)
    assert canon([r for r in rows if r[2] == 0]) == canon(dev_rows)
    assert out.read_text().splitlines()[0] == "level,group,fold,metric,value"
    assert len(out.read_text().splitlines()) == len(rows) + 1
    saved = (tmp_path / "pred" / "predictions_fold_1.csv").read_text().splitlines()
    assert saved[0] == "dataset,entity,anatomy_site,sex,age,age_encoded,tumor,prob,age_group" and len(saved) == 49


def test_linear_probe_script(tmp_path):
    from oracle import weights as W
    from scripts import linear_probe_test_eval_downstream as script
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    from src.utils.trainer import Trainer
    m = VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.AdamW, lr=5e-5),
                             False, False, 512, 312, 128, compute_dtype="fp32", text_dropout=0.0)
    W.apply_recipe(m, 0)
    ckpt = str(tmp_path / "vlp.ckpt")
    Trainer(enable_checkpointing=False).save_checkpoint(ckpt, m)
    out = tmp_path / "probe.csv"
    rows = script.main([str(out), ckpt, "--folds", "2", "--n-samples", "32", "--n-val-samples", "8"] + DATA_ARGV)
    check_table(rows, 2)
    assert out.read_text().splitlines()[0] == "level,group,fold,metric,value"
