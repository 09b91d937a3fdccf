"""sklearn's own exact t-SNE on the end-to-end test data, recorded once so that no test runs
its optimiser (about 2 s per fit).

    python tests/golden/make_tsne_golden.py

Writes tests/golden/tsne_sklearn.json.  Data: tests/tsne_ref.py::blobs (N = 300, D = 32, three
Gaussian blobs, seed 0).  For max_iter 1000 (the device gate) and 300 (the CPU restatement's):
TSNE(n_components=2, perplexity=30, method="exact", max_iter=..., random_state=s) for s = 0..4,
everything else at its default (init="pca", learning_rate="auto").  Per fit: the KL divergence of
its embedding by _kl_divergence in fp64 against _joint_probabilities of the fp32 squared distances
(tests/tsne_ref.py::sqdist_f32), which is what the tests compute for the code under test, and
sklearn.manifold.trustworthiness(X, Y, n_neighbors=5).  No CPU or GPU code of this project runs.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.tsne_ref import GOLDEN, PERPLEXITY_E2E, blobs, sk_joint, sk_kl_grad, sqdist_f32  # noqa: E402


def main():
    import sklearn
    from sklearn.manifold import TSNE, trustworthiness
    x, _ = blobs()
    P = sk_joint(sqdist_f32(x), PERPLEXITY_E2E)
    out = {"sklearn": sklearn.__version__, "N": int(x.shape[0]), "D": int(x.shape[1]), "perplexity": PERPLEXITY_E2E,
           "data_sum": float(np.asarray(x, dtype=np.float64).sum())}
    for max_iter in (1000, 300):
        kl, kl_own, tr = [], [], []
        for seed in range(5):
            t = TSNE(n_components=2, perplexity=PERPLEXITY_E2E, method="exact", max_iter=max_iter,
                     random_state=seed)
            y = t.fit_transform(x)
            kl.append(sk_kl_grad(y, P)[0])
            kl_own.append(float(t.kl_divergence_))
            tr.append(float(trustworthiness(x, y, n_neighbors=5)))
            print(max_iter, seed, kl[-1], kl_own[-1], tr[-1], flush=True)
        out[f"max_iter_{max_iter}"] = {"kl": kl, "kl_divergence_": kl_own, "trustworthiness": tr}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
