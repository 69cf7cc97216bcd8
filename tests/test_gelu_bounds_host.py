"""CPU: the error bounds csrc/gv_common.h states for its polynomial GELU and GELU', over the whole input domain.

linear_plan_cases.gelu_ref / dgelu_ref emulate gelu_f / dgelu_f (f32 arithmetic, fused multiply-adds carried in f64;
tests/test_leading_dims_gpu.py shows that the device computes exactly these functions) and are compared here with the f64
erf-GELU x Phi(x) and its exact derivative Phi(x) + x phi(x), on every finite bfloat16 value, every finite float16 value and
a dense f32 grid on [-6, 6].  The bounds are the header's, none of them is tuned to what the emulation gives:
    |gelu err| <= 1.7e-4 on -4 <= x <= 4;   relative error <= 7.4e-5 for x > 4 (the result is x Phi_fit(4): the absolute error grows
    with x there);   for x < -4: |err| <= 7.4e-5 |x| (the result is x Phi_fit(-4): the true tail of the function as built -- a change
    that bounds it is a deliberate edit of this line and of the header);
    |gelu' err| <= 3.8e-4 for every x."""
import math

import pytest
import torch

import linear_plan_cases as lc


def _all16(dtype):
    """every finite value of a 16-bit format, as f32"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).float()
    return v[torch.isfinite(v)]


@pytest.fixture(scope="module", params=["bfloat16", "float16", "f32_grid"])
def xs(request):
    if request.param == "f32_grid":
        return torch.linspace(-6.0, 6.0, 240001, dtype=torch.float64).float()
    return _all16(getattr(torch, request.param))


def _phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _Phi(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))       # erfc: no cancellation in the left tail


def test_gelu_bounds(xs):
    x = xs.double()
    ref = x * _Phi(x)
    err = (lc.gelu_ref(xs).double() - ref).abs()
    mid, hi, lo = (x >= -4.0) & (x <= 4.0), x > 4.0, x < -4.0
    assert mid.any() and hi.any() and lo.any()
    rel = err[hi] / ref[hi]
    tail = err[lo] / x[lo].abs()
    print("gelu: max |err| on [-4, 4] %.4g, max relative err on x > 4 %.4g, max |err| / |x| on x < -4 %.4g" % (float(err[mid].max()), float(rel.max()), float(tail.max())))
    assert float(err[mid].max()) <= 1.7e-4
    assert float(rel.max()) <= 7.4e-5
    assert float(tail.max()) <= 7.4e-5


def test_dgelu_bound(xs):
    x = xs.double()
    err = (lc.dgelu_ref(xs).double() - (_Phi(x) + x * _phi(x))).abs()
    k = int(err.argmax())
    print("gelu': max |err| %.4g at x = %.6g" % (float(err[k]), float(x[k])))
    assert float(err.max()) <= 3.8e-4
