"""Split counts and digests of every slab and gradient bit of the split-K weight-gradient entry
points, recorded from a library whose bits are to be kept (tests/test_gpu_wgrad_bits.py reruns
every case).

Needs a GPU.  Run it with the library of the commit to pin, never with the code under test:

    VLP_HIP_LIB=/path/to/that/libvlp_hip.so python tests/golden/make_wgrad_bits.py --commit <its commit>

Writes tests/golden/wgrad_bits.json: the commit, the device and its CU count (the auto split
fills rounds of resident workgroups, so it depends on it), and per case the digest of the host
inputs and the split count.  bf16 cases also hold the sha256 of the slabs ws[: ns * slab] and of
the folded gradient with its guard elements; run() itself asserts that everything past the
slabs written (the unused slabs and the guard past the workspace) and past the gradient still
holds the sentinel.  Those paths have no atomics: equality is exact.  fp32 cases take the
atomics-into-slab-0 fallback, whose bits depend on the order the workgroups finish: only their
split count (1) is recorded.

Cases (CASES), the smallest shapes that reach each route:
  conv     WGRAD_CASES of tests/test_gpu_conv_routes.py under its vlp_set_wgrad_rows_min_images
           handling (the workspace bound binds in rows-3slabs-5images and pp128x384-tight3);
           fp32 on the three shapes of its test_conv_wgrad_ws_fp32_atomics
  stem     (3-channel) and stem1 (single-channel): N = 2 at 64 x 64 (2048 output pixels, one
           split) and N = 4 at 128 x 128 (16384 pixels, several) in a 64-slab workspace, the
           latter again in a workspace of exactly 2 slabs; fp32 at N = 2
  linear   (M, Nout, Kin) = (512, 128, 128) one-tile ring, (65536, 96, 96) gemm_big_kernel,
           (16384, 256, 256) ping-pong, each in the workspace vlp_linear_wgrad_ws_floats asks for
           and again with room for two slabs.  dw starts from zeros.  The entry point returns no
           count: the one recorded is the number of slabs it wrote.
Inputs: one seeded CPU generator per case, rounded to the storage dtype.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests.test_gpu_conv_routes import WGRAD_CASES  # noqa: E402

FIXTURE = os.path.join(HERE, "wgrad_bits.json")
BF16, F32 = torch.bfloat16, torch.float32
GUARD, SENT = 64, -1024.0
U8_MEAN, U8_STD = 127.5, 64.0

CONV_F32 = [c for c in WGRAD_CASES if c[7] in ("big64x192", "bk64x128-1x1s2", "big128x256-3x3s2")]
# (N, H, slabs)
STEM_SHAPES = [(2, 64, 64), (4, 128, 64), (4, 128, 2)]
# (M, Nout, Kin, route)
LINEAR_SHAPES = [(512, 128, 128, "bk"), (65536, 96, 96, "big"), (16384, 256, 256, "pp")]


def cases():
    """[(id, kind, shape row, dtype)] in a fixed order (the index seeds the inputs)."""
    out = [(c, "conv", BF16) for c in WGRAD_CASES] + [(c, "conv", F32) for c in CONV_F32]
    for kind in ("stem", "stem1"):
        out += [(c, kind, BF16) for c in STEM_SHAPES] + [(STEM_SHAPES[0], kind, F32)]
    for c in LINEAR_SHAPES:
        out += [(c + (0,), "linear", BF16), (c + (2,), "linear", BF16)]

    def cid(c, kind):
        if kind == "conv":
            return "x".join(map(str, c[:7])) + f"-{c[7]}-{c[8]}slabs"
        if kind == "linear":
            return "x".join(map(str, c[:3])) + f"-{c[3]}-" + (f"{c[4]}slabs" if c[4] else "full")
        return f"{c[0]}x{c[1]}x{c[1]}-{c[2]}slabs"
    return [(f"{kind}-{cid(c, kind)}-{'fp32' if dt == F32 else 'bf16'}", kind, c, dt) for c, kind, dt in out]


CASES = cases()


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update((t.view(torch.int16) if t.dtype == BF16 else t).numpy().tobytes())
    return h.hexdigest()


def host_inputs(index, kind, c, dt):
    """The operands of the case on the host, and their digest."""
    g = torch.Generator().manual_seed(2000 + index)
    rn = lambda shape: torch.randn(shape, generator=g)
    h = {}
    if kind == "conv":
        N, H, W, C, Co, KH, S = c[:7]
        P = 1 if KH == 3 else 0
        h["x"] = rn((N, H, W, C)).to(dt)
        h["dy"] = rn((N, (H + 2 * P - KH) // S + 1, (W + 2 * P - KH) // S + 1, Co)).to(dt)
    elif kind == "linear":
        h["dy"], h["x"] = rn((c[0], c[1])).to(dt), rn((c[0], c[2])).to(dt)
    else:
        N, H = c[:2]
        if kind == "stem":
            h["x"] = rn((N, 3, H, H))
        else:
            h["x"] = torch.randint(0, 256, (N, 1, H, H), generator=g, dtype=torch.uint8)
        h["dy"] = rn((N, H // 2, H // 2, 64)).to(dt)
    return h, digest(*h.values())


def run(lib, kind, c, dt, h):
    """One call on fresh device copies of `h`: (split count, digest of the slabs written, digest of
    the gradient with its guard); the digests are None for fp32."""
    from vlp_amd import ops
    d = {k: v.cuda() for k, v in h.items()}
    dy, x = d["dy"], d["x"]
    st = torch.cuda.current_stream().cuda_stream
    code = 1 if dt == BF16 else 0
    ns = ctypes.c_int(0)
    if kind == "conv":
        N, H, W, C, Co, KH, S, route, slabs = c
        P = 1 if KH == 3 else 0
        slab, ngrad = Co * KH * KH * C, Co * C * KH * KH
    elif kind == "linear":
        M, Nout, Kin, route, slabs = c
        slab = ngrad = Nout * Kin
        if not slabs:
            n = ctypes.c_longlong(0)
            lib.vlp_linear_wgrad_ws_floats(M, Nout, Kin, ctypes.byref(n))
            slabs = n.value // slab
    else:
        N, H, slabs = c
        slab, ngrad = (64 * 256 if kind == "stem" else 64 * 64), 64 * 3 * 7 * 7
    nws = slabs * slab
    ws = torch.full((nws + GUARD,), SENT, device="cuda")
    grad = torch.full((ngrad + GUARD,), SENT, device="cuda")
    if kind == "conv":
        prev = ctypes.c_int(0)
        lib.vlp_set_wgrad_rows_min_images(1 if route.startswith("rows") else -1, ctypes.addressof(prev))
        try:
            lib.vlp_conv_wgrad_ws(code, dy.data_ptr(), x.data_ptr(), ws.data_ptr(), nws, ctypes.addressof(ns),
                                  N, H, W, C, Co, KH, KH, S, P, st)
        finally:
            lib.vlp_set_wgrad_rows_min_images(prev.value, None)
        lib.vlp_conv_wgrad_fold(Co, C, KH, KH, ns.value, ws.data_ptr(), grad.data_ptr(), st)
    elif kind == "stem":
        _, _, Hp, Wp = ops.stem_geom(H, H)
        xp = torch.zeros(N, Hp, Wp, 4, dtype=dt, device="cuda")
        ops.stem_prep(x, xp)
        lib.vlp_stem_wgrad_ws(code, dy.data_ptr(), xp.data_ptr(), ws.data_ptr(), nws, ctypes.addressof(ns),
                              N, H, H, st)
        lib.vlp_stem_wgrad_fold(ns.value, ws.data_ptr(), grad.data_ptr(), st)
    elif kind == "stem1":
        _, _, Hp, Wp1 = ops.stem1_geom(H, H)
        xs = torch.empty(4, N, Hp, Wp1, dtype=dt, device="cuda")
        ops.stem1_prep_u8(x, xs, U8_MEAN, U8_STD)
        lib.vlp_stem1_wgrad_ws(code, dy.data_ptr(), xs.data_ptr(), ws.data_ptr(), nws, ctypes.addressof(ns),
                               N, H, H, st)
        lib.vlp_stem1_wgrad_fold(ns.value, ws.data_ptr(), grad.data_ptr(), st)
    else:
        grad[:ngrad] = 0
        lib.vlp_linear_wgrad_ws(code, M, Nout, Kin, dy.data_ptr(), Nout, x.data_ptr(), Kin, grad.data_ptr(),
                                ws.data_ptr(), nws, st)
        torch.cuda.synchronize()
        ns.value = int((ws[:nws].view(slabs, slab) != SENT).any(1).sum().item())
    torch.cuda.synchronize()
    assert 1 <= ns.value <= slabs, f"{ns.value} slabs of {slabs} allowed"
    assert bool((ws[ns.value * slab:] == SENT).all().item()), "slab writes past the split count or the workspace"
    assert bool((grad[ngrad:] == SENT).all().item()), "writes past the gradient"
    if dt == F32:
        return ns.value, None, None
    return ns.value, digest(ws[:ns.value * slab]), digest(grad)


def write_fixture(res, path):
    """One line per case."""
    head = {k: v for k, v in res.items() if k != "cases"}
    rows = ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(res["cases"].items()))
    with open(path, "w") as f:
        f.write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": {\n' + rows + "\n}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library VLP_HIP_LIB names")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    from vlp_amd._lib import lib
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cases": {}}
    for i, (cid, kind, c, dt) in enumerate(CASES):
        h, din = host_inputs(i, kind, c, dt)
        ns, slabs, grad = run(lib(), kind, c, dt, h)
        res["cases"][cid] = {"inputs": din, "nsplit": ns}
        if dt == BF16:
            res["cases"][cid].update(slabs=slabs, grad=grad)
        print(f"{cid}: {ns} splits", flush=True)
    write_fixture(res, args.out)
    print(f"{args.out}: {len(CASES)} cases, library of {args.commit}")


if __name__ == "__main__":
    main()
