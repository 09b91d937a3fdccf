"""The ResNet-34 tower's kernel-launch sequence per configuration, recorded on the CPU from a
tower whose launches are to be kept (tests/test_tower_trace_cpu.py reruns every configuration).

Needs the built library (the host predicates are the real ones) and no GPU.  Run it on the commit
to pin, never on the code under test:

    python tests/golden/make_tower_trace.py --commit <that commit>

Writes tests/golden/tower_launch_trace.json: per configuration one line per `ops.<name>(...)`
call vlp_amd/resnet34.py makes, in order.  resnet34.ops is replaced by a recorder (Recorder):
  host predicates (FORWARDED) run for real -- they only compute geometry, no device is touched;
  every other call is bound to the real wrapper's signature, logged and not run.  Required
    parameters are logged in signature order, optional ones as name=value where they differ
    from the default, so positional and keyword spelling do not matter;
  tensors are logged by identity: t<k>, numbered by first appearance, keyed by (storage,
    offset, shape, stride, dtype), with dtype and shape at first appearance.  So the trace
    holds which buffer feeds which operand: a swapped mean / istd or a wrong statistics row
    changes it;
  the (offset, length) handed to run_backward's on_stage_done callback is logged in sequence.
"""
import argparse
import inspect
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(HERE, "tower_launch_trace.json")
FORWARDED = ("conv_out_hw", "stem_geom", "stem1_geom", "stem1_fused_ok", "conv_fwd_act_ok", "conv_dgrad_act_ok")
FWD_OUT = ("conv_fwd", "conv_fwd_act")
DGRAD_OUT = ("conv_dgrad", "conv_dgrad_relu", "conv_dgrad_bn_act", "conv_dgrad_relu_act", "conv_dgrad_relu_ds",
             "conv_dgrad_relu2")
DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64", torch.uint8: "u8", torch.int64: "i64"}
FLAGS = ("_USE_WG_STREAM", "_USE_STEM1", "_USE_STEM_FUSED", "_USE_BWD_ACT", "_USE_DS_FOLD", "_USE_RELU2",
         "_USE_ACT_FUSED")


class Recorder:
    """Stands in for the vlp_amd.ops module inside vlp_amd.resnet34."""

    def __init__(self, real):
        self._real = real
        self.lines = []
        self._names, self._alive = {}, []

    def _tensor(self, t):
        sp = t.untyped_storage().data_ptr()
        key = (sp, t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype)
        name = self._names.get(key)
        if name is not None:
            return name
        self._alive.append(t)   # the allocator must not hand this address to a later tensor
        name = self._names[key] = f"t{len(self._names)}"
        return f"{name}:{DT[t.dtype]}{list(t.shape)}".replace(" ", "")

    def _fmt(self, v):
        if isinstance(v, torch.Tensor):
            return self._tensor(v)
        if isinstance(v, (tuple, list)):
            return "(" + ",".join(self._fmt(e) for e in v) + ")"
        return repr(v)

    def stage_done(self, off, n):
        self.lines.append(f"on_stage_done({off},{n})")

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in FORWARDED:
            return fn
        sig = inspect.signature(fn)

        def call(*a, **kw):
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            parts = []
            for p in sig.parameters.values():
                v = args.arguments[p.name]
                if p.default is inspect.Parameter.empty:
                    parts.append(self._fmt(v))
                elif isinstance(v, torch.Tensor) or v != p.default:
                    parts.append(f"{p.name}={self._fmt(v)}")
            ret, A = None, args.arguments
            if name in FWD_OUT:
                N, H, W, _ = A["x"].shape
                Ho, Wo = self._real.conv_out_hw(H, W, A["KH"], A["KW"], A["S"], A["P"])
                ret = A["out"] if A["out"] is not None else torch.empty((N, Ho, Wo, A["Co"]), dtype=A["x"].dtype)
            elif name in DGRAD_OUT:
                dy = A[next(iter(sig.parameters))]
                ret = A["out"] if A["out"] is not None else torch.empty((dy.shape[0], A["H"], A["W"], A["C"]),
                                                                        dtype=dy.dtype)
            elif name == "pack_conv_batch":
                ret = "<pack_desc>"
            line = f"{name}({','.join(parts)})"
            self.lines.append(line if ret is None else f"{line}->{self._fmt(ret)}")
            return ret
        return call


def _full(dtype, shape, u8=True, training=True, backward=True, steps=1, **flags):
    return {"kind": "tower", "dtype": dtype, "shape": shape, "u8": u8, "training": training,
            "backward": training and backward, "steps": steps, "flags": flags}


def configs():
    from tests.test_gpu_blocks import RANGES
    c = {
        "bf16-u8-512": _full("bf16", 512),
        "bf16-u8-512-eval": _full("bf16", 512, training=False),
        "bf16-u8-512-stem_unfused": _full("bf16", 512, _USE_STEM_FUSED=False),
        "bf16-u8-512-no_act": _full("bf16", 512, _USE_BWD_ACT=False, _USE_ACT_FUSED=False),
        "bf16-u8-512-no_ds_fold-no_relu2": _full("bf16", 512, _USE_DS_FOLD=False, _USE_RELU2=False),
        "bf16-u8-512-no_stem1": _full("bf16", 512, _USE_STEM1=False),
        "bf16-f32-256": _full("bf16", 256, u8=False),
        "fp32-u8-512": _full("fp32", 512),
        "fp32-u8-34": _full("fp32", 34),
        # the second forward on a kept workspace: every per-shape buffer and the pack descriptor cached
        "bf16-u8-512-fwd2": _full("bf16", 512, backward=False, steps=2),
    }
    for name, (lo, hi, hwc) in RANGES.items():
        c["range-" + name] = {"kind": "range", "dtype": "bf16", "lo": lo, "hi": hi, "hwc": hwc, "flags": {}}
    return c


_TOWERS = {}


def _tower(dtype):
    from vlp_amd.resnet34 import ResNet34Tower
    if dtype not in _TOWERS:
        _TOWERS[dtype] = ResNet34Tower(compute_dtype=dtype, device="cpu")
    return _TOWERS[dtype]


def _step(tower, cfg, rec):
    if cfg["kind"] == "range":
        H, W, C = cfg["hwc"]
        out, saved = tower.run_block_range_forward(torch.empty(1, H, W, C, dtype=tower.tdtype), cfg["lo"], cfg["hi"])
        tower.run_block_range_backward(saved, torch.empty_like(out))
        return
    S = cfg["shape"]
    if cfg["u8"]:
        feat, saved = tower.run_forward(None, cfg["training"], x_u8=torch.empty(1, 1, S, S, dtype=torch.uint8))
    else:
        feat, saved = tower.run_forward(torch.empty(1, 3, S, S), cfg["training"])
    if cfg["backward"]:
        tower.run_backward(saved, torch.empty(1, 512), on_stage_done=rec.stage_done)


def trace(cfg):
    """The launch lines of one configuration (of its last step), from a fresh workspace."""
    from vlp_amd import ops, resnet34
    tower = _tower(cfg["dtype"])
    tower._ws = {}
    old = {k: getattr(resnet34, k) for k in FLAGS}
    try:
        for k, v in cfg["flags"].items():
            assert k in FLAGS, k
            setattr(resnet34, k, v)
        for _ in range(cfg.get("steps", 1)):
            rec = resnet34.ops = Recorder(ops)
            _step(tower, cfg, rec)
    finally:
        resnet34.ops = ops
        for k, v in old.items():
            setattr(resnet34, k, v)
        tower._ws = {}
    return rec.lines


def write_fixture(res, path):
    """One line per call."""
    body = ",\n".join(json.dumps(name) + ": [\n" + ",\n".join(json.dumps(l) for l in lines) + "\n]"
                      for name, lines in res["traces"].items())
    with open(path, "w") as f:
        f.write('{"commit": ' + json.dumps(res["commit"]) + ', "traces": {\n' + body + "\n}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose vlp_amd/resnet34.py is recorded")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    res = {"commit": args.commit, "traces": {name: trace(cfg) for name, cfg in configs().items()}}
    write_fixture(res, args.out)
    print(f"{args.out}: " + ", ".join(f"{k} {len(v)}" for k, v in res["traces"].items()))


if __name__ == "__main__":
    main()
