"""GPU: the leading dimensions of every GEMM-class entry point, and the device's GELU / GELU' against their emulation.

include/gipvit.h gives gv_linear five leading dimensions, gv_linear_dw_group three per problem and the full-row entry points three to
five each.  tests/leading_dims_cases.py embeds every matrix of a call in a larger buffer -- NaN around what the call reads, a fixed bit
pattern around what it writes, guards behind the contiguous outputs -- and compares the call with the same call on compact operands,
bit for bit; integer operands make the expectation exact as well.  A stride that is the width where the leading dimension was meant, or
a ragged edge that is read and only saved by a zero in the other operand, fails here."""
import os
import subprocess
import sys

import pytest
import torch

import leading_dims_cases as ldc
import linear_plan_cases as lpc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = torch.float32
CASES = ldc.cases()


def ops():
    from gipvit import ops as o
    return o


def L():
    from gipvit import _lib
    return _lib


@pytest.fixture(scope="module")
def ws(dev):
    """the split-K scratch; leading_dims_cases.run fills it with NaN in front of every call"""
    return torch.empty(L().lib.gv_linear_workspace_bytes() // 4, dtype=f32, device=dev)


def test_cases_name_every_family():
    """(no GPU: the case list alone) every kernel family of the GEMM-class entry points is the asserted kernel of some case"""
    names = {c["kernel"] for c in CASES}
    for family in ("gemm_kernel<false, false", "gemm_kernel<false, true", "gemm_kernel<true, true", "false, -1>", "gemm_deep_kernel<false, false",
                   "gemm_deep_kernel<true, true, float, true, 16>", "gemm_kernel<false, false, float, true, 16>", "gemm_kernel<false, true, float, true, 16>",
                   "dw8_kernel<false>", "dw8_kernel<true>", "gemm_dw_group_kernel", "dw8_group_kernel", "linear_f32_kernel",
                   "panel_kernel<4, 8, 64, false, 0, 0, 0>", "panel_kernel<4, 8, 64, false, 0, 0, 1>", "panel_kernel<4, 8, 64, true, 1, 0, 0>",
                   "panel_kernel<4, 8, 64, true, 1, 0, 1>", "panel_kernel<4, 8, 64, false, 0, 1, 0>", "panel_kernel<7, 8, 64, false, 0, 1, 0>") + tuple(
                       "panel_kernel<4, 8, 64, %s, 2, %d, 1>" % (tb, ep) for tb, ep in (("true", 0), ("false", 1), ("false", 2), ("false", 3), ("true", 4), ("false", 5))):
        assert any(family in n for n in names), family
    assert len({c["id"] for c in CASES}) == len(CASES) and {c["group"] for c in CASES} == set(ldc.GROUPS)


@pytest.mark.parametrize("pads", ldc.PADS)
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_framed_operands(dev, ws, case, pads):
    """One case on one pad set: padding and guards of every written buffer bit-unchanged, outputs bit-identical to the compact call's, the
    kernel the case names on both, the exact result where there is one (tests/leading_dims_cases.py check)."""
    ldc.check(ops(), L(), case, dev, ws, pads)


@pytest.mark.parametrize("group", ldc.GROUPS)
def test_framed_operands_cu_budget_248(dev, group):
    """The same checks with the launches sized for 248 CUs (a data-parallel run): the budget is read once per process, so the group's
    cases run in a process of their own -- that process is what this test is about."""
    env = dict(os.environ, GIPVIT_CU_BUDGET="248")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "leading_dims_cases.py"), group], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    assert r.stdout.strip().splitlines()[-1].endswith("CU budget 248")


def test_linear_rejects_unaligned_leading_dims(dev):
    """what the minimum pad set stands on: one element less and the entry point refuses (GV_E_ALIGN), before any launch"""
    o = ops()
    A = torch.zeros(64, 72, dtype=o.bf16, device=dev); B = torch.zeros(64, 72, dtype=o.bf16, device=dev); C = torch.zeros(64, 72, dtype=o.bf16, device=dev)
    for kw, msg in ((dict(lda=68), "lda/ldb"), (dict(ldb=68), "lda/ldb"), (dict(ldc=66), "ldc")):
        with pytest.raises(L().GipvitError, match=msg):
            o.linear(A, B, C, 64, 64, 64, **kw)
    out = torch.zeros(64, 392, device=dev); W = torch.zeros(384, 72, dtype=o.bf16, device=dev)
    with pytest.raises(L().GipvitError, match="misaligned"):
        o.linear_ln_fwd(A, W, out, 64, 64, lda=72, ldw=72, ldo=385)
    with pytest.raises(L().GipvitError, match="misaligned"):
        o.linear_ln_fwd(A, W, out, 64, 64, lda=68, ldw=72)


# ------------------------------------------------------------------------------------------ GELU / GELU' on the device
def _all16(dtype):
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def test_gelu_on_the_device_is_the_emulated_polynomial(dev):
    """gv_linear with A = 0, f32 C, BIAS | GELU: the accumulator is 0 + bias[n] exactly, so C[m, n] = gelu_f(bias[n]).  bias sweeps every
    finite bfloat16 and float16 value and a dense f32 grid on [-6, 6]; the result is compared BITWISE with linear_plan_cases.gelu_ref,
    whose error bounds tests/test_gelu_bounds_host.py holds.  Non-finite inputs are excluded (nothing downstream defines a value for
    them)."""
    o = ops()
    sweep = torch.cat([_all16(torch.bfloat16).float(), _all16(torch.float16).float(), torch.linspace(-6.0, 6.0, 65536, dtype=torch.float64).float()])
    sweep = sweep[torch.isfinite(sweep)]
    sweep = torch.cat([sweep, torch.zeros(-len(sweep) % 8)])
    M, N, K = 16, len(sweep), 32
    A, B = torch.zeros(M, K, dtype=o.bf16, device=dev), torch.zeros(N, K, dtype=o.bf16, device=dev)
    C = torch.full((M, N), 9.0, dtype=f32, device=dev)
    o.linear(A, B, C, M, N, K, epilogue=lpc.BIAS | lpc.GELU, bias=sweep.to(dev))
    want = lpc.gelu_ref(sweep + 0.0).view(torch.int32)                  # (0 + bias: -0 enters the epilogue as +0)
    got = C.cpu().view(torch.int32)
    bad = got != want[None, :]
    print("gelu: %d inputs, %d rows, %d mismatches" % (N, M, int(bad.sum())))
    assert not bool(bad.any()), [(float(sweep[n]), float(C[0, n]), float(lpc.gelu_ref(sweep[n:n + 1]))) for n in bad[0].nonzero().flatten()[:8].tolist()]


def test_dgelu_on_the_device_is_the_emulated_polynomial(dev):
    """BIAS | DGELU with A = 0 and bias = 1: C = 1 x dgelu_f(aux_in).  aux_in holds all 65 536 bit patterns of the build's 16-bit format as
    a 256 x 256 matrix; the finite ones are compared BITWISE with linear_plan_cases.dgelu_ref.  Non-finite inputs are excluded."""
    o = ops()
    aux = _all16(o.bf16).view(256, 256)
    M = N = 256
    A, B = torch.zeros(M, 32, dtype=o.bf16, device=dev), torch.zeros(N, 32, dtype=o.bf16, device=dev)
    C = torch.full((M, N), 9.0, dtype=f32, device=dev)
    o.linear(A, B, C, M, N, 32, epilogue=lpc.BIAS | lpc.DGELU, bias=torch.ones(N, device=dev), aux_in=aux.to(dev))
    fin = torch.isfinite(aux.float())
    want, got = lpc.dgelu_ref(aux.float()).view(torch.int32), C.cpu().view(torch.int32)
    bad = (got != want) & fin
    print("gelu': %d finite inputs, %d mismatches" % (int(fin.sum()), int(bad.sum())))
    assert int(fin.sum()) > 63000 and not bool(bad.any()), [(float(aux[i, j]), float(C[i, j])) for i, j in bad.nonzero()[:8].tolist()]
