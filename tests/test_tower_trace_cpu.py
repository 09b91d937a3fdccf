"""CPU: the ResNet-34 tower launches the same kernels, in the same order, on the same buffers.

vlp_amd/resnet34.py is the host side of the image tower: it decides which conv / BN / stem kernel
runs and what each operand is.  Every launch goes through its module attribute `ops`, so with a
recorder in that place (tests/golden/make_tower_trace.py: host predicates real, every other call
logged with its tensors named by identity, nothing run) a tower constructed on the CPU yields its
whole launch sequence without a device.  tests/golden/tower_launch_trace.json holds that sequence
per configuration, recorded before the tower's forward and backward were split into routed steps;
the fixture is never regenerated, so any difference is a change of behaviour in resnet34.py.

Configurations (N = 1): bf16 on a 512 x 512 uint8 upload -- training with every route on (fused
stem, conv_fwd_act, both _act data gradients, relu_ds, relu2), a second forward on the kept
workspace, eval, and training with the fused stem / the layer-1 ring fusions / the downsample fold
and the three-sum epilogue / the single-channel stem off; bf16 on a 256 x 256 fp32 NCHW input; fp32
compute at 512 x 512 and at 34 x 34 (stem1_geom refuses Wo = 17: the 3-channel stem); and the bf16
block ranges of tests/test_gpu_blocks.py at that test's input shapes.
"""
import json
import os

import pytest

from tests.conftest import PKG
from tests.golden import make_tower_trace as G

LIB = os.path.join(PKG, "vlp_amd", "libvlp_hip.so")
CONFIGS = G.configs()


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)["traces"]


def test_fixture_covers_every_configuration(golden):
    assert set(golden) == set(CONFIGS)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_launch_trace_is_unchanged(golden, name):
    if not os.path.exists(LIB):
        pytest.skip("libvlp_hip.so not built (run __graft_entry__.build())")
    got, want = G.trace(CONFIGS[name]), golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs\n  now:      {g}\n  recorded: {w}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, {len(want)} recorded"
