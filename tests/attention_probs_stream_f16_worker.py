"""Run by tests/test_attention_probs_stream_gpu.py in a process of its own with GIPVIT_ACT_FORMAT=f16 (one process computes in one
16-bit format): gv_attention_probs_stream of the float16 build (libgipvit_hip_f16.so) on probes A and C at N = 289 and 1 025, on the
lse of that build's gv_attention_fwd_stream, for q_rows = N (block form) and 1 (row form), into a buffer with sentinel-filled guards
before and behind p.  Every probe value is exactly representable in float16 (+-4 codes, zeros; probe C's randn keys are
bf16-rounded, which float16 holds exactly down to 2^-17).  Prints one line per check and 'PROBS STREAM F16 OK' at the end; any failure
is an exception (non-zero exit)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("GIPVIT_ACT_FORMAT") == "f16"

from gipvit import _lib, ops                                                              # noqa: E402
from test_attention_probes_host import H, N_IMG, SCALE, build, pack_qkv                   # noqa: E402
from test_attention_probs_stream_host import check_probs_selector, check_probs_uniform    # noqa: E402

assert _lib.lib.gv_act_format() == 1 and ops.bf16 is torch.float16
dev = torch.device("cuda:0")
GUARD, SENT = 37, -12345.0

for N in (289, 1025):
    for probe, check in (("A", check_probs_selector), ("C", check_probs_uniform)):
        case = build(probe, N)
        qkv = pack_qkv(case, N_IMG, H, torch.float16).to(dev)
        _, lse = ops.attention_fwd_stream(qkv, N_IMG, N, H, SCALE)
        for q_rows in (N, 1):
            n = N_IMG * H * q_rows * N
            buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=dev)
            p = buf[GUARD:GUARD + n].view(N_IMG, H, q_rows, N)
            ops.attention_probs_stream(qkv, lse, N_IMG, N, H, SCALE, q_rows, p=p)
            torch.cuda.synchronize()
            assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all()), "the kernel wrote outside p"
            got = p.reshape(N_IMG * H, q_rows, N).cpu()
            check(got, case, q_rows)
            print(f"probe {probe} N={N} q_rows={q_rows}: max p {float(got.max()):.6g}, max |row sum - 1| {float((got.double().sum(-1) - 1).abs().max()):.3e}")
print("PROBS STREAM F16 OK")
