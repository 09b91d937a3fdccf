"""Call time of vlp_amd.metrics.tsne (the exact t-SNE of the post-fit evaluation,
csrc/tsne_ops.hip) on one GPU: a host clock around whole calls that end in a device
synchronise (a call holds host work: the PCA init and one small read-back per 50
iterations), and device events around its parts (distances, affinities, a window of
ordinary iterations).

    python tools/tsne_bench.py [--n 4096] [--d 512] [--calls 3] [--out profiles/tsne_bench.json]
    python tools/tsne_bench.py --sklearn-cpu [--n 4096] [--d 512]     # no GPU: sklearn's Barnes-Hut default

Data: three Gaussian blobs from a seeded generator.  Prints one JSON line (and writes
it to --out).  Not a gate and not part of bench.py.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")]


def data(N, D):
    import numpy as np
    rng = np.random.default_rng(0)
    centres = 4.0 * rng.standard_normal((3, D))
    return (centres[np.arange(N) % 3] + rng.standard_normal((N, D))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sklearn-cpu", action="store_true")
    a = ap.parse_args()
    N, D = a.n, a.d
    x = data(N, D)
    if a.sklearn_cpu:
        from sklearn.manifold import TSNE
        t = time.perf_counter()
        m = TSNE(n_components=2, perplexity=30, random_state=42)
        m.fit(x)
        res = {"what": "sklearn TSNE (barnes_hut, defaults) on the host CPUs", "N": N, "D": D,
               "cpus": os.cpu_count(), "seconds": round(time.perf_counter() - t, 2),
               "kl_divergence_": round(float(m.kl_divergence_), 4), "n_iter_": int(m.n_iter_)}
    else:
        import torch
        from vlp_amd import metrics, ops
        if not torch.cuda.is_available():
            raise SystemExit("tsne_bench needs a GPU (or --sklearn-cpu)")
        xd = torch.from_numpy(x).cuda()

        def events(fn, reps):
            fn()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / reps

        secs, kl = [], None
        metrics.tsne(xd)          # warm-up: code objects, allocator
        torch.cuda.synchronize()
        for _ in range(a.calls):
            t = time.perf_counter()
            y, kl = metrics.tsne(xd)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t)
        d2 = ops.tsne_sqdist(xd)
        P = ops.tsne_affinities(d2, 30.0)
        run = metrics._HipDescent(xd, 30.0)
        run.start(y.clone())
        res = {"what": "vlp_amd.metrics.tsne call time (exact, 1000 iterations)", "N": N, "D": D,
               "seconds_per_call": [round(s, 4) for s in secs], "kl": round(kl, 4),
               "ms_sqdist": round(events(lambda: ops.tsne_sqdist(xd), 5), 3),
               "ms_affinities": round(events(lambda: ops.tsne_affinities(d2, 30.0), 5), 3),
               "us_per_iteration": round(1e3 * events(lambda: run.step(1.0, 0.8, 200.0, False), a.iters), 2),
               "P_bytes_read_per_iteration": 4 * N * N}
        del P
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
