"""Run by tests/test_attention_stream_bwd_gpu.py in a process of its own with GIPVIT_ACT_FORMAT=f16 (one process computes in one
16-bit format): gv_attention_fwd_stream + gv_attention_bwd_stream of the float16 build (libgipvit_hip_f16.so) on probes A and D at
N = 289 and 1 025, dq / dk / dv held to the probes' checks, every output and the delta scratch in guarded buffers.  Every value of
probe A is exactly representable in float16 (integers up to 8, +-4 codes); probe D's randn data is bf16-rounded, which float16
holds exactly down to 2^-17.  Prints one line per check and 'STREAM BWD F16 OK' at the end; any failure is an exception (non-zero
exit)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("GIPVIT_ACT_FORMAT") == "f16"

from gipvit import _lib, ops                                                              # noqa: E402
from test_attention_probes_host import H, N_IMG, SCALE, build, pack_qkv, pack_rows, unpack_dqkv   # noqa: E402
from test_attention_stream_bwd_host import BWD_PARTS, bwd_check                           # noqa: E402

assert _lib.lib.gv_act_format() == 1 and ops.bf16 is torch.float16
dev = torch.device("cuda:0")
GUARD, SENT = 8, -768.0
f16 = torch.float16


def guarded(rows, cols, dtype):
    buf = torch.full(((rows + GUARD) * cols,), SENT, dtype=dtype, device=dev)
    return buf, buf[:rows * cols].view(rows, cols)


for N in (289, 1025):
    for probe in "AD":
        case = build(probe, N)
        qkv = pack_qkv(case, N_IMG, H, f16).to(dev)
        d_o = pack_rows(case["d_o"], N_IMG, H, f16).to(dev)
        bufs = dict(o=guarded(N_IMG * N, H * 64, f16), lse=guarded(N_IMG * H, N, torch.float32), dqkv=guarded(N_IMG * N, 3 * H * 64, f16),
                    delta=guarded(N_IMG * H, N, torch.float32))
        out, lse, dqkv, delta = (bufs[k][1] for k in ("o", "lse", "dqkv", "delta"))
        ops.attention_fwd_stream(qkv, N_IMG, N, H, SCALE, o=out, lse=lse.view(N_IMG, H, N))
        ops.attention_bwd_stream(qkv, out, d_o, lse.view(N_IMG, H, N), N_IMG, N, H, SCALE, dqkv=dqkv, delta=delta.view(-1))
        torch.cuda.synchronize()
        for name, (buf, view) in bufs.items():
            assert bool((buf[view.numel():] == SENT).all()), f"a kernel wrote behind {name}"
        dq, dk, dv = unpack_dqkv(dqkv, N_IMG, H)
        got = dict(dq=dq, dk=dk, dv=dv)
        bwd_check(probe)(got, case)
        print(f"probe {probe} N={N}: " + "  ".join(f"max |{n} err| {float((got[n] - case[n]).abs().max()):.3e}" for n in BWD_PARTS[probe]))
print("STREAM BWD F16 OK")
