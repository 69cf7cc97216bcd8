"""Run by tests/test_attention_stream_gpu.py in a process of its own with GIPVIT_ACT_FORMAT=f16 (one process computes in one 16-bit
format): gv_attention_fwd_stream of the float16 build (libgipvit_hip_f16.so) on probes A, C and D at N = 289 and 1 025, into
guarded buffers.  Every probe value is exactly representable in float16 (integers up to 8, +-4 codes); probe D's randn data is
bf16-rounded, which float16 holds exactly down to 2^-17.  Prints one line per check and 'STREAM F16 OK' at the end; any failure is
an exception (non-zero exit)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("GIPVIT_ACT_FORMAT") == "f16"

from gipvit import _lib, ops                                                              # noqa: E402
from test_attention_probes_host import H, N_IMG, SCALE, build, pack_qkv, unpack_lse, unpack_rows   # noqa: E402
from test_attention_stream_host import STREAM_CHECKS                                      # noqa: E402

assert _lib.lib.gv_act_format() == 1 and ops.bf16 is torch.float16
dev = torch.device("cuda:0")
GUARD, SENT = 8, -768.0


def guarded(rows, cols, dtype):
    buf = torch.full(((rows + GUARD) * cols,), SENT, dtype=dtype, device=dev)
    return buf, buf[:rows * cols].view(rows, cols)


for N in (289, 1025):
    for probe in "ACD":
        case = build(probe, N)
        qkv = pack_qkv(case, N_IMG, H, torch.float16).to(dev)
        obuf, out = guarded(N_IMG * N, H * 64, torch.float16)
        lbuf, lse = guarded(N_IMG * H, N, torch.float32)
        ops.attention_fwd_stream(qkv, N_IMG, N, H, SCALE, o=out, lse=lse.view(N_IMG, H, N))
        torch.cuda.synchronize()
        assert bool((obuf[out.numel():] == SENT).all()) and bool((lbuf[lse.numel():] == SENT).all()), "a kernel wrote behind its output buffer"
        got = dict(o=unpack_rows(out, N_IMG, H), lse=unpack_lse(lse, N_IMG, H))
        STREAM_CHECKS[probe](got, case, parts=("o", "lse"))
        print(f"probe {probe} N={N}: max |lse err| {float((got['lse'] - case['lse']).abs().max()):.3e}, max |o err| {float((got['o'] - case['o']).abs().max()):.3e}")
print("STREAM F16 OK")
