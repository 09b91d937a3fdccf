"""Call time of vlp_cluster_dist_sums (the silhouette's per-cluster distance sums,
csrc/retrieval_ops.hip) on one GPU: device events around windows of back-to-back
calls through the C ABI (no label read-back, no host work inside the window).

    python tools/silhouette_bench.py [--n 10000] [--d 512] [--c 2] [--calls 50] [--windows 3]

Prints one JSON line: ms per call for every window and the direct-difference
operation rate (3 N^2 D operations: subtract, multiply, add per pair and column).
Needs an MI355X; there is no CPU path.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    import torch
    from vlp_amd._lib import lib, ptr, stream_of
    if not torch.cuda.is_available():
        raise SystemExit("silhouette_bench needs a GPU")
    N, D, C = a.n, a.d, a.c
    x = torch.randn(N, D, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    ids = (torch.arange(N, device="cuda") % C).int()
    out = torch.empty(N, C, device="cuda")

    def call():
        lib().vlp_cluster_dist_sums(N, N, D, ptr(x), D, ptr(x), D, ptr(ids), C, ptr(out), stream_of())

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.calls):
            call()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / a.calls)
    best = min(ms)
    print(json.dumps({"what": "vlp_cluster_dist_sums call time", "N": N, "D": D, "C": C, "calls_per_window": a.calls,
                      "ms_per_call": [round(m, 4) for m in ms],
                      "tera_ops_per_s_best": round(3.0 * N * N * D / (best * 1e-3) / 1e12, 2)}))


if __name__ == "__main__":
    main()
