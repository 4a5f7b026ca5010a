"""skp_resize_bilinear and its adjoint skp_resize_bilinear_bwd against float64 (tests/loss_ref.py), through
ops.resize_bilinear with autograd and through ops.aggregate(upsample_res=...), the adjoint's production caller.

The adjoint gathers over a window computed in float arithmetic on the index; the cases go up, down, to the
same side, from and to one pixel, and across non-integer ratios in both directions.  Bounds are 4·e_cpu,
e_cpu = max|oracle_fp32 − float64| / max(1, max|float64|) on these inputs, measured and asserted by
tests/test_loss_ref_cpu.py (two digits, rounded up): resize 1.1e-7, its adjoint 1.1e-7, the aggregate
backward 1.1e-7.
"""
import numpy as np
import pytest
import torch

import loss_ref as L
from oracle import skp_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# 4 · e_cpu per compared quantity (tests/test_loss_ref_cpu.py holds the oracle to a quarter of each)
BOUND = {
    "resize": 4.4e-7,
    "resize_adjoint": 4.4e-7,
    "aggregate_bwd": 4.4e-7,
}
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    yield
    print("\nlargest GPU error per quantity: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(SEEN.items())))


def T(a, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).requires_grad_(grad)


def N(t):
    return t.detach().cpu().numpy()


def close(name, got, ref, slack=1.0):
    e = L.err(got, ref)
    SEEN[name] = max(SEEN.get(name, 0.0), e)
    assert e <= slack * BOUND[name], (name, e, slack * BOUND[name])


@pytest.mark.parametrize("C,R,Ro", L.RESIZE_CASES)
def test_resize_bilinear_vs_float64(C, R, Ro):
    from stablekeypoints_amd import ops
    x_np, g_np = L.resize_case(C, R, Ro)
    x = T(x_np, grad=True)
    out = ops.resize_bilinear(x, Ro)
    out.backward(T(g_np))
    assert out.shape == (C, Ro, Ro) and x.grad.shape == (C, R, R)
    close("resize", N(out), L.resize(x_np, Ro))
    close("resize_adjoint", N(x.grad), L.resize_adjoint(g_np, R))


def test_aggregate_upsampled_backward():
    """ops.aggregate(layers, indices, upsample_res=80) with a backward pass: two layers (2, 32·32, 12), one
    token gathered twice.  Against float64 at 4·e_cpu, and against O.collect_maps_bwd at 5·e_cpu: the
    kernel within 4·e_cpu of float64 and the oracle within e_cpu of it."""
    from stablekeypoints_amd import ops
    layers_np, dmap = L.aggregate_case()
    idx = list(L.AGG["indices"])
    layers = [T(a, grad=True) for a in layers_np]
    out = ops.aggregate(layers, indices=torch.tensor(idx), upsample_res=L.AGG["Ro"])
    assert np.allclose(N(out), O.collect_maps(layers_np, upsample_res=L.AGG["Ro"], indices=idx), atol=1e-6)
    out.backward(T(dmap))
    ref64 = L.aggregate_bwd(L.AGG["shape"], L.AGG["n_layers"], dmap, L.AGG["Ro"], idx)
    ref32 = O.collect_maps_bwd([L.AGG["shape"]] * L.AGG["n_layers"], dmap, upsample_res=L.AGG["Ro"], indices=idx)
    for t, r32 in zip(layers, ref32):
        close("aggregate_bwd", N(t.grad), ref64)
        close("aggregate_bwd", N(t.grad), r32, slack=1.25)
