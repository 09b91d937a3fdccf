"""Every output bit of the convolution data-gradient entry points against
tests/golden/dgrad_bits.json, the digests tests/golden/make_dgrad_bits.py recorded from the
library of the commit the fixture names (the host dispatch before dgrad_s1 / dgrad_s2 /
with_dgrad_relu_epi of csrc/conv_ops.hip replaced its copies).  The fixture is never
regenerated from the code under test: a route, an epilogue operand or a launch argument that
changes moves a bit and fails here.  The cases, their shapes and their inputs are the
generator's own (its docstring lists the routes and the shapes that reach them).

Each case's host inputs are digested first: a failure there says that the input generator (or
torch's random stream) changed, not the kernels.

Outputs (dx / g with their guard rows, dy_out of the two _act entry points) are deterministic
and compared by sha256.  The BN sums are not: each of the P workgroups that cover a column adds
ONE fp32 partial (its own rows, summed in a fixed order) to the fp64 statistic with an atomic,
in whatever order the workgroups finish, and the stat_rep replicas are added on the host.  So a
recorded sum and a rerun are two summation trees over the same P fp64 leaves t_1 .. t_P.  Any
tree of P - 1 fp64 additions is within gamma_(P-1) * sum |t_i| of the exact sum
(gamma_k = k u / (1 - k u), u = 2^-53), so two trees differ by at most
2 gamma_(P-1) sum |t_i| <= P * 2^-52 * sum |t_i| (P (P - 1) u <= 1 for any grid).  P is the
case's launch grid (the last field of its shape row).  sum |t_i| is bounded on the host in fp64
from the device output and the case's operands: |t_i| <= (1 + 2^-7) sum over the workgroup's
rows of |g * f|, f = 1, xhat(y) or xhat(yd) -- the factor covers the bf16 rounding of the stored
g (2^-8; the sums take g before it), the fp32 evaluation of (y - mean) * invstd * g and the fp32
partial sum of at most 1024 rows (2^-13).  The assertion per channel is
    |new - recorded| <= P * 2^-52 * (1 + 2^-7) * sum_pixels |out * f|
a reordering bound, not a measured one (P <= 2 gives bit-equal sums: addition commutes).
"""
import json

import pytest
import torch

from tests.golden import make_dgrad_bits as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ops():
    from vlp_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_case(golden):
    assert set(golden["cases"]) == {c[0] for c in G.CASES} and len(G.CASES) == len(golden["cases"])


@pytest.mark.parametrize("index", range(len(G.CASES)), ids=[c[0] for c in G.CASES])
def test_dgrad_bits(ops, golden, index):
    cid, c, epi, dt, fused = G.CASES[index]
    want = golden["cases"][cid]
    h, din = G.host_inputs(index, c, dt)
    assert din == want["inputs"], f"inputs changed ({cid}): the kernels were not compared"
    got, totals, out = G.run(ops, index, c, epi, dt, fused, h)
    assert got == want["out"], f"{cid}: other output bits than the library of {golden['commit']}"
    recorded = G.unpack_stats(want["stats"], c[3])
    assert len(totals) == len(recorded)
    P = c[8]
    o = out.double().cpu()
    f = [torch.ones_like(o), (h["y"].double() - h["mean"].double()) * h["invstd"].double(),
         (h["yd"].double() - h["meand"].double()) * h["invstdd"].double()]
    for k, (new, rec) in enumerate(zip(totals, recorded)):
        bound = P * 2.0 ** -52 * (1 + 2.0 ** -7) * (o * f[k]).abs().sum((0, 1, 2))
        d = (new - rec).abs()
        print(f"{cid} stat{k + 1}: P {P}, worst |new - recorded| / bound {(d / (bound + 1e-300)).max().item():.3f}, "
              f"{int((d > 0).sum())} of {d.numel()} channels differ")
        assert bool((d <= bound).all()), f"{cid} stat{k + 1}: beyond the reordering bound"
