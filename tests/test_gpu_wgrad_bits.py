"""The split count and every slab and gradient bit of the split-K weight-gradient entry points
(vlp_conv_wgrad_ws, vlp_stem_wgrad_ws, vlp_stem1_wgrad_ws with their folds, vlp_linear_wgrad_ws)
against tests/golden/wgrad_bits.json, which tests/golden/make_wgrad_bits.py recorded from the
library of the commit the fixture names: the host code before one split resolution
(resolve_ksplit of csrc/gemm.h) and one slab plan (plan_slabs of csrc/conv_ops.hip) replaced its
copies.  The fixture is never regenerated from the code under test: a route, a split count, a
chunk length or a fold order that changes moves a bit and fails here.  The cases, their shapes
and their inputs are the generator's own (its docstring lists them).

The auto split fills rounds of resident workgroups, so it depends on the device's CU count: on
a device with another count than the recorded one the comparison is void, and the test fails
(it does not skip).

Each case's host inputs are digested first: a failure there says that the input generator (or
torch's random stream) changed, not the kernels.  bf16 cases have no atomics and are compared
by sha256; fp32 cases take the atomics fallback and only their split count (1) is compared
(tests/test_gpu_conv_routes.py holds their values against fp64).
"""
import json

import pytest
import torch

from tests.golden import make_wgrad_bits as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lib():
    from vlp_amd._lib import lib as l
    return l()


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_case(golden):
    assert set(golden["cases"]) == {c[0] for c in G.CASES} and len(G.CASES) == len(golden["cases"])


@pytest.mark.parametrize("index", range(len(G.CASES)), ids=[c[0] for c in G.CASES])
def test_wgrad_bits(lib, golden, index):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == golden["cus"], f"{cus} CUs, the fixture was recorded on {golden['cus']}: splits are not comparable"
    cid, kind, c, dt = G.CASES[index]
    want = golden["cases"][cid]
    h, din = G.host_inputs(index, kind, c, dt)
    assert din == want["inputs"], f"inputs changed ({cid}): the kernels were not compared"
    ns, slabs, grad = G.run(lib, kind, c, dt, h)
    print(f"{cid}: {ns} splits, recorded {want['nsplit']}")
    assert ns == want["nsplit"], f"{cid}: other split count than the library of {golden['commit']}"
    if dt == G.F32:
        assert ns == 1
        return
    assert slabs == want["slabs"], f"{cid}: other slab bits than the library of {golden['commit']}"
    assert grad == want["grad"], f"{cid}: other gradient bits than the library of {golden['commit']}"
