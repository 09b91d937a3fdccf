"""Helpers shared by tests/test_gpu_text_routes.py, tests/test_gpu_flash_routes.py and
tests/test_gpu_stem_routes.py: storage dtypes, the dropout hash of csrc/common.h on the host,
NaN-guarded buffers, the per-element gate, and (stem suite) the staged-rounding and sum bounds.
No tests and no fixtures live here."""
import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
GUARD = 8          # NaN rows after every output


def dtid(dt):
    return "fp32" if dt == F32 else "bf16"


def epc(dt):
    return 8 if dt == BF16 else 4


def r_t(dt):
    return 2.0 ** -8 if dt == BF16 else 0.0


def gpu_ops():
    """vlp_amd.ops, or a skip without a GPU (each test file wraps this in its own fixture)"""
    import pytest
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlp_amd import ops as o
    return o


# ---------------------------------------------------------------- dropout hash (csrc/common.h)
def hash_u(seed, idx):
    """hash_uniform: splitmix64 of seed + golden * (idx + 1), top 24 bits * 2^-24 (float32)."""
    idx = np.asarray(idx, dtype=np.uint64)
    z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def drop_scale(seed, n, p):
    """[n] float64 tensor: the fp32 value 1 / (1 - p) where kept, 0 where dropped (p == 0: ones)."""
    if p <= 0.0:
        return torch.ones(n, dtype=F64)
    keep = hash_u(seed, np.arange(n, dtype=np.uint64)) >= np.float32(p)
    s = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(keep.astype(np.float64) * float(s))


# ---------------------------------------------------------------- buffers
def rnd(shape, g, dt, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g, dtype=F64) * scale + shift).to(dt)


def nan_out(rows, cols, dt, dev):
    return torch.full((rows + GUARD, cols), float("nan"), dtype=dt, device=dev)


def nan_tail(t, dev):
    """copy of the 2-D input t on dev followed by GUARD NaN rows the kernel must not read"""
    buf = torch.full((t.shape[0] + GUARD,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=dev)
    buf[:t.shape[0]].copy_(t)
    return buf


def take(name, buf, rows):
    """owned rows of a NaN-guarded buffer on the CPU; the guard must still be NaN"""
    assert bool(torch.isnan(buf[rows:]).all().item()), f"{name}: rows beyond the output written"
    return buf[:rows].cpu()


def store_bound(e, ref, dt):
    return e + r_t(dt) * (ref.abs() + e)


# ---------------------------------------------------------------- the gate
def check_into(worst, name, fam, got, ref, bound):
    """every element finite and |got - ref| <= bound; the worst ratio is kept in worst[fam]"""
    got = got.double()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    d = (got - ref).abs()
    ratio = float((d / (bound + 1e-300)).max()) if ref.numel() else 0.0
    nviol = int((~(d <= bound)).sum())
    worst[fam] = max(worst.get(fam, 0.0), ratio)
    print(f"{name}: worst |err|/bound {ratio:.3f}, violations {nviol} of {ref.numel()}")
    assert nviol == 0, f"{name}: {nviol} of {ref.numel()} elements beyond the bound (worst ratio {ratio:.2f})"


# ---------------------------------------------------------------- staged roundings and sums (stem suite)
EPS32 = 2.0 ** -23


def staged(acc64, noise):
    """bf16(acc64) and, per element, what a flip of that rounding may move it by: one ulp where acc64
    lies within `noise` of a rounding boundary (where fp32 and fp64 accumulation can round apart),
    zero elsewhere (the convolution suite's `staged`)."""
    v = acc64.to(BF16).double()
    m, e = torch.frexp(v.abs())
    ulp = torch.ldexp(torch.ones_like(v), e - 8) * (v != 0)
    d = (acc64 - v).abs()
    near = (ulp / 2 - d) <= noise
    near |= (m == 0.5) & ((ulp / 4 - d).abs() <= noise)   # below a power of two the spacing halves
    return v, torch.where(near, ulp, torch.zeros_like(ulp))


def sum_bound(noise_f, gf, T, dims):
    """2 * (sum noise * |f| + (T + 4) * eps32 * sum |g * f|) over `dims`: the per-element deviation carried
    linearly into a sum whose fp32 partials are T terms deep (the convolution suite's `sum_bound`)."""
    return 2.0 * (noise_f.sum(dims) + (T + 4) * EPS32 * gf.abs().sum(dims))


def emu_sum(v32, T):
    """[rows][C] fp32 -> [C] fp64: fp32 partial sums of T rows, then fp64 (a kernel's reduction, emulated)"""
    v = v32.reshape(-1, v32.shape[-1])
    pad = (-v.shape[0]) % T
    if pad:
        v = torch.cat([v, torch.zeros(pad, v.shape[1], dtype=v.dtype)])
    return v.view(-1, T, v.shape[1]).sum(1).double().sum(0)
