"""CPU: vlp_amd.metrics.tsne on CPU tensors (the plain torch restatement of sklearn's exact
t-SNE) against scikit-learn, the same gates tests/test_gpu_tsne.py holds the HIP kernels to.

Gates (references and data in tests/tsne_ref.py, recorded sklearn fits in
tests/golden/tsne_sklearn.json; none of the limits comes from the code under test):

  * row entropy: every row of the conditional matrix has, in fp64, an entropy within 1e-5
    (sklearn's own stopping tolerance) of log(perplexity).  The restatement returns the row in
    fp64, so there is no storage slack here; the device test adds the fp32 one.
  * total variation of the joint P against _joint_probabilities: at most max(4 t, 1e-6), t the
    total variation of an independent fp64 numpy restatement (tsne_ref.np_conditional) from
    sklearn, measured in the test (1e-16 here); 1e-6 is the fp32 rounding of a matrix that sums
    to 1 (N^2 entries of relative error 2^-24 sum to at most 2^-24 ~ 6e-8), with room.
  * P symmetric bit for bit, zero diagonal.
  * one iteration against _kl_divergence in fp64.  The fp32 restatement is the yardstick of the
    device test (twice its error, with a floor); here it is held to the floor itself.  Floor: with
    u = 2^-24, a pair's term q^2 (p / Q - 1) (y_i - y_j) takes about 8 roundings, so 8 u per
    term; a row's attraction and repulsion cancel to a fraction of their size, measured 1/4 or
    more on these inputs, so 32 u = 1.9e-6 relative to the gradient's norm.  The KL is a sum of
    p log(p / Q) with sum p = 1 and |log(p / Q)| < 8 on these inputs, each log argument within
    4 u: 32 u = 1.9e-6 absolute.  Measured here: gradient 2.4e-7 .. 5.4e-7, KL 5.5e-8 .. 1.5e-7.
  * the gains + momentum step equals numpy's fp32 _gradient_descent arithmetic bit for bit.
  * end to end at max_iter 300: KL (sklearn's _kl_divergence in fp64 of the returned Y against
    sklearn's P) at most the worst of sklearn's five seeds plus their spread, trustworthiness at
    least the worst minus the spread, two runs equal.
"""
import numpy as np
import pytest
import torch

from tests import tsne_ref as R

U = 2.0 ** -24
GRAD_FLOOR = KL_FLOOR = 32 * U

AFFINITY_CASES = [(20, 19.0, 0), (257, 30.0, 0), (300, 30.0, 10)]


@pytest.fixture(scope="module")
def M():
    from vlp_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def e2e():
    x, _ = R.blobs()
    return x, R.sk_joint(R.sqdist_f32(x), R.PERPLEXITY_E2E)


@pytest.mark.parametrize("N,perplexity,dup", AFFINITY_CASES)
def test_affinities_vs_sklearn(M, N, perplexity, dup):
    x, _ = R.blobs(N, 32, seed=3, dup=dup)
    d2 = R.sqdist_f32(x)
    if dup:
        assert (d2[:dup, N - dup:].diagonal() == 0).all()
    cond = M.tsne_conditional_cpu(torch.from_numpy(d2), perplexity)
    P = M.tsne_joint_cpu(cond).numpy()
    H = R.row_entropy(cond.numpy())
    dev = np.abs(H - np.log(perplexity)).max()
    tv = R.total_variation(P, R.sk_joint(d2, perplexity))
    tv_np = R.total_variation(R.np_joint(R.np_conditional(d2, perplexity)), R.sk_joint(d2, perplexity))
    print(f"N={N}: entropy off by {dev:.3e}; TV {tv:.3e} (numpy restatement {tv_np:.3e})")
    assert dev <= 1e-5
    assert tv <= max(4 * tv_np, 1e-6)
    assert P.dtype == np.float32 and np.array_equal(P, P.T) and (P.diagonal() == 0).all()
    assert (P[~np.eye(N, dtype=bool)] > 0).all()


def test_sqdist_cpu(M):
    x, _ = R.blobs(70, 37, seed=5, dup=3)
    got = M.tsne_sqdist_cpu(torch.from_numpy(x)).numpy()
    ref = R.sqdist_f32(x).astype(np.float64)
    assert (got.diagonal() == 0).all() and np.array_equal(got, got.T) and (got[:3, 67:].diagonal() == 0).all()
    assert np.abs(got - ref).max() <= 2 * (37 + 2) * U * ref.max()


@pytest.mark.parametrize("N", [300, 1030])
@pytest.mark.parametrize("scale", [1e-4, 10.0])
def test_one_iteration_vs_sklearn(M, N, scale):
    x, _ = R.blobs(N, 32, seed=2)
    P = R.sk_joint(R.sqdist_f32(x), 30.0)
    y = R.fixed_y(N, scale)
    for exag in (1.0, 12.0):
        kl64, g64 = R.sk_kl_grad(y, P, exag)
        kl, g = M.tsne_grad_cpu(torch.from_numpy(y), torch.from_numpy(P).float(), exag)
        gerr = np.linalg.norm(g.numpy().astype(np.float64) - g64) / np.linalg.norm(g64)
        print(f"N={N} scale={scale} exag={exag}: grad rel L2 {gerr:.3e}, KL err {abs(kl - kl64):.3e}")
        assert gerr <= GRAD_FLOOR and abs(kl - kl64) <= KL_FLOOR


def step_case(n=64, seed=0):
    """grad, update, gains covering both signs of update * grad, a zero product and gains that the
    0.8 factor takes below the 0.01 floor."""
    rng = np.random.default_rng(seed)
    grad = rng.standard_normal((n, 2)).astype(np.float32)
    update = rng.standard_normal((n, 2)).astype(np.float32)
    update[:4] = 0.0
    gains = rng.uniform(0.5, 3.0, (n, 2)).astype(np.float32)
    gains[4:12] = np.float32(0.012)
    update[4:8] = np.abs(update[4:8]) * np.sign(grad[4:8])      # same sign: 0.012 * 0.8 < 0.01
    update[8:12] = -np.abs(update[8:12]) * np.sign(grad[8:12])  # opposite sign: 0.012 + 0.2
    return grad, update, gains


@pytest.mark.parametrize("momentum,lr", [(0.5, 50.0), (0.8, 85.33333333333333)])
def test_step_equals_numpy(M, momentum, lr):
    grad, update, gains = step_case()
    y = R.fixed_y(64, 3.0)
    gg, u_ref, g_ref = R.np_update(grad, update, gains, momentum, lr)
    assert (g_ref[4:8] == np.float32(0.01)).all() and ((update * grad < 0).any() and (update * grad > 0).any())
    ty, tu, tg = torch.from_numpy(y.copy()), torch.from_numpy(update.copy()), torch.from_numpy(gains.copy())
    out = M.tsne_step_cpu(torch.from_numpy(grad.copy()), ty, tu, tg, momentum, lr)
    assert np.array_equal(out.numpy(), gg) and np.array_equal(tu.numpy(), u_ref) and np.array_equal(tg.numpy(), g_ref)
    assert np.array_equal(ty.numpy(), y + u_ref)


def test_pca_init(M):
    x, _ = R.blobs()
    y = M.tsne_pca_init(torch.from_numpy(x)).numpy().astype(np.float64)
    xc = x.astype(np.float64) - x.astype(np.float64).mean(0)
    _, s, vt = np.linalg.svd(xc, full_matrices=False)
    for c in range(2):
        v = vt[c] * np.sign(vt[c][np.abs(vt[c]).argmax()])
        ref = xc @ v / (s[0] / np.sqrt(len(x))) * 1e-4
        assert np.abs(y[:, c] - ref).max() <= 1e-6 * np.abs(ref).max()
    assert abs(y[:, 0].std() - 1e-4) <= 1e-10


def test_end_to_end_300_iterations(M, e2e):
    from sklearn.manifold import trustworthiness
    x, P = e2e
    golden = R.load_golden()
    assert golden["data_sum"] == float(x.astype(np.float64).sum())
    kl_max, trust_min = R.e2e_gates(golden, 300)
    y, kl_own = M.tsne(torch.from_numpy(x), R.PERPLEXITY_E2E, max_iter=300)
    y2, kl2 = M.tsne(torch.from_numpy(x), R.PERPLEXITY_E2E, max_iter=300)
    assert y.shape == (300, 2) and y.dtype == torch.float32 and torch.isfinite(y).all()
    kl = R.sk_kl_grad(y.numpy(), P)[0]
    trust = trustworthiness(x, y.numpy(), n_neighbors=5)
    print(f"KL {kl:.4f} (own {kl_own:.4f}, gate <= {kl_max:.4f}); trustworthiness {trust:.4f} (gate >= {trust_min:.4f})")
    assert kl <= kl_max and trust >= trust_min
    assert torch.equal(y, y2) and kl_own == kl2


def test_schedule_and_stopping(M, monkeypatch):
    """250 iterations at exaggeration 12 / momentum 0.5, then exaggeration 1 / momentum 0.8 with
    gains and update restarted; checks every 50 iterations and on the last one; both stopping rules."""
    calls = []

    class Fake:
        def __init__(self, x, perplexity):
            self.kl = iter(())

        def start(self, y):
            self.y = y

        def reset(self):
            calls.append("reset")

        def step(self, exag, momentum, lr, check):
            calls.append((exag, momentum, lr, check))

        def read(self):
            return next(Fake.stats)

    monkeypatch.setattr(M, "_CpuDescent", Fake)
    x = torch.from_numpy(R.blobs(60, 8)[0])
    Fake.stats = iter([(5.0 - 0.1 * k, 1.0) for k in range(100)])
    M.tsne(x, 10.0, max_iter=333)
    steps = [c for c in calls if c != "reset"]
    assert calls[0] == "reset" and calls[251] == "reset" and calls.count("reset") == 2 and len(steps) == 333
    assert all(s[:3] == (12.0, 0.5, 50.0) for s in steps[:250]) and all(s[:3] == (1.0, 0.8, 50.0) for s in steps[250:])
    assert [i for i, s in enumerate(steps) if s[3]] == [49, 99, 149, 199, 249, 299, 332]
    # learning_rate "auto" above its floor of 50
    calls.clear()
    Fake.stats = iter([(1.0, 1.0)] * 100)
    M.tsne(torch.zeros(4800, 2) + torch.arange(4800.0)[:, None], 30.0, max_iter=250, early_exaggeration=6.0)
    assert calls[1][2] == 4800 / 6.0 / 4.0
    # no progress for more than 300 iterations after the best check (at 299): stop at 649
    calls.clear()
    Fake.stats = iter([(5.0 - 0.1 * k, 1.0) for k in range(5)] + [(4.0, 1.0)] + [(9.0, 1.0)] * 100)
    M.tsne(x, 10.0, max_iter=1000)
    assert len([c for c in calls if c != "reset"]) == 650
    # gradient norm at or below min_grad_norm at the first check of the second stage
    calls.clear()
    Fake.stats = iter([(5.0, 1.0)] * 5 + [(4.0, 1e-7)] + [(3.0, 1.0)] * 100)
    M.tsne(x, 10.0, max_iter=1000)
    assert len([c for c in calls if c != "reset"]) == 300


def test_errors(M):
    x = torch.zeros(10, 4)
    with pytest.raises(ValueError, match="perplexity"):
        M.tsne(x, perplexity=10.0)
    with pytest.raises(ValueError, match="perplexity"):
        M.tsne(x, perplexity=30.0)
    with pytest.raises(ValueError, match="4 GB"):
        M.tsne(torch.zeros(32769, 1), perplexity=30.0)
    with pytest.raises(ValueError, match="max_iter"):
        M.tsne(x, perplexity=5.0, max_iter=100)
    with pytest.raises(ValueError):
        M.tsne(torch.zeros(10), perplexity=5.0)


def test_evaluate_split_tsne_and_files(tmp_path, monkeypatch):
    """evaluate_split(tsne=True) on a stand-in module: the extra keys, the reference's perplexity
    rule (N - 1 below 30 samples), the files of save_tsne; without the flag, today's keys only."""
    from src.utils import post_fit_evaluation as E

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Linear(6, 5)

        def _unpack(self, batch):
            return (batch["x"],)

        def forward_features(self, x):
            return self.w(x)

        def forward_head(self, f):
            return f.sum(1)

        def features_and_logits(self, batch):
            f = self.forward_features(self._unpack(batch)[0])
            return f, self.forward_head(f)

    g = torch.Generator().manual_seed(0)
    batches = [{"x": torch.randn(6, 6, generator=g) + 3 * (b % 2), "tumor": torch.tensor([0, 1, 0, 1, 1, 0]),
                "dataset": ["INTERNAL", "BTXRD"] * 3} for b in range(2)]
    model = Tiny()
    plain = E.evaluate_split(model, [batches])
    assert set(plain) == {"silhouette_score_based_on_tumor", "silhouette_score_based_on_dataset", "confusion_matrix"}
    seen = {}
    real = E.metrics.tsne

    def short_tsne(x, perplexity):
        seen["p"] = perplexity
        return real(x, perplexity, max_iter=250)

    monkeypatch.setattr(E.metrics, "tsne", short_tsne)
    res = E.evaluate_split(model, [batches], tsne=True)
    assert seen["p"] == 11 and set(res) == set(plain) | {"tsne", "tsne_kl", "tumor", "dataset"}
    assert res["tsne"].shape == (12, 2) and res["tsne"].device.type == "cpu" and np.isfinite(res["tsne_kl"])
    assert {k: res[k] for k in plain} == plain
    E.save_tsne(res, "validation", str(tmp_path / "out"))
    z = np.load(tmp_path / "out" / "tsne_validation.npz")
    assert z["y"].shape == (12, 2) and np.isfinite(z["y"]).all()
    assert z["tumor"].tolist() == res["tumor"] and z["dataset"].tolist() == res["dataset"]
    pytest.importorskip("matplotlib")
    assert (tmp_path / "out" / "tsne_validation.png").stat().st_size > 1000
