"""Time the streaming BN elementwise kernels at the bs=256 ResNet34 sizes against
a plain device copy of the same bytes (torch copy_), to place them against the
achievable HBM rate.
  python tools/ew_bench.py
  python tools/ew_bench.py --accum   the gradient-accumulation passes at the 35.7 M-float arena
                                     (vlp_grad_accum: the extra pass per micro-batch) against
                                     the device copy of the same traffic"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")]
import torch  # noqa: E402
from vlp_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)


def tm(fn, it=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1000


def accum_bench(n=35_700_000):
    """vlp_grad_accum reads acc and g and writes acc: 3 x 4n bytes (3 x 143 MB).  The floor is
    a device copy moving the same bytes (copy_ of 1.5 n floats: 6n read + 6n written)."""
    import json
    acc, g = torch.zeros(n, device=dev), torch.randn(n, device=dev)
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    src, dst = torch.randn(n * 3 // 2, device=dev), torch.empty(n * 3 // 2, device=dev)
    k = ops.grad_sumsq_nparts(n)
    partials, out = torch.zeros(k, dtype=torch.float64, device=dev), torch.zeros(2, device=dev)
    hyp = (1e-3, 0.9, 0.999, 1e-8, 0.01, 3)
    t = {"n_floats": n,
         "copy_3x4n_bytes_us": tm(lambda: dst.copy_(src), 20),
         "grad_accum_us": tm(lambda: ops.grad_accum(acc, g, 1.0, False), 20),
         "grad_accum_first_us": tm(lambda: ops.grad_accum(acc, g, 1.0, True), 20),
         "grad_sumsq_us": tm(lambda: ops.grad_sumsq(g, partials), 20),
         "grad_accum_sumsq_us": tm(lambda: ops.grad_accum_sumsq(acc, g, 1.0, partials), 20),
         "adamw_clip_us": tm(lambda: ops.adamw_clip(p, g, m, v, *hyp, coef=out[1:]), 20),
         "adamw_clip_accum_us": tm(lambda: ops.adamw_clip_accum(p, g, m, v, *hyp, acc=acc, coef=out[1:]), 20)}
    t["grad_accum_over_copy"] = t["grad_accum_us"] / t["copy_3x4n_bytes_us"]
    t["grad_accum_TBps"] = 12 * n / t["grad_accum_us"] / 1e6
    t["copy_TBps"] = 12 * n / t["copy_3x4n_bytes_us"] / 1e6
    print(json.dumps(t), flush=True)


if "--accum" in sys.argv[1:]:
    accum_bench()
    sys.exit(0)

for (H, C) in [(128, 64), (64, 128), (32, 256), (16, 512)]:
    N = 256
    M = N * H * H
    y = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
    idt = torch.randn_like(y)
    out = torch.empty_like(y)
    m = torch.empty(y.numel() // 8, dtype=torch.uint8, device=dev)
    sc, sh = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    mu, ist, gam = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.ones(C, device=dev)
    sg = torch.zeros(C, dtype=torch.float64, device=dev)
    sgx = torch.zeros_like(sg)
    dy = torch.empty_like(y)
    B = y.numel() * 2
    tc = tm(lambda: out.copy_(y))
    t0 = tm(lambda: ops.bn_add_relu(y, sc, sh, None, None, None, out))
    t1 = tm(lambda: ops.bn_add_relu(y, sc, sh, idt, None, None, out, relu_mask=m))
    t2 = tm(lambda: ops.bn_bwd_apply(M, C, idt, None, 1, None, (y, mu, ist, gam, sg, sgx, dy), None, None, y))
    print(f"{H:3d}x{H:<3d}x{C:3d}: copy {tc:7.1f} us {2 * B / tc / 1e6:5.2f} TB/s | "
          f"bn_relu {t0:7.1f} us {2 * B / t0 / 1e6:5.2f} | bn_add_relu+mask {t1:7.1f} us {3.0625 * B / t1 / 1e6:5.2f} | "
          f"bn_bwd_apply {t2:7.1f} us {3 * B / t2 / 1e6:5.2f} TB/s", flush=True)
