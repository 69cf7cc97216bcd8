"""Run by tests/test_global_pool_gpu.py in a process of its own with GIPVIT_ACT_FORMAT=f16 (one process computes in one 16-bit
format): gv_token_mean_fwd / gv_token_mean_bwd of the float16 build (libgipvit_hip_f16.so) at (3, 17, 384) under the contracts of
tests/test_global_pool_host.py, and one supervised step of a mean-pooled vit_tiny against that module's reference at the gates
of tests/test_engine_gpu.py (logits 2e-2 of max |ref|, loss 1e-3, per-parameter gradient 5e-2, gradient norm 1e-2).  Prints one
line per check and 'POOL F16 OK' at the end; any failure is an exception (non-zero exit)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("GIPVIT_ACT_FORMAT") == "f16"

from gipvit import _lib, ops                                     # noqa: E402
from gipvit.engine import SupervisedEngine                       # noqa: E402
from oracle import vit_oracle as vo                              # noqa: E402  (checker only)
import test_global_pool_host as H                                # noqa: E402
from test_global_pool_gpu import check_grads, run_pool_kernels   # noqa: E402

assert _lib.lib.gv_act_format() == 1 and ops.bf16 is torch.float16
dev = torch.device("cuda:0")

for with_scale in (True, False):
    for act in (torch.float16, torch.float32):
        ratio = run_pool_kernels(ops, dev, 3, 17, 384, act, with_scale)
    print(f"token mean 3x17x384 gb_scale={with_scale}: forward error / bound {ratio:.3f}", flush=True)

torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
p = H.avg_params("vit_tiny", 64, 2, seed=0)
tiles = vo.synth_tiles(8, 64, seed=1234)
tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(5))
eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, device=dev, global_pool="avg")
assert eng.scaler is not None and eng.grp.gb.dtype is torch.float16
eng.load_state(p)
loss_r, grads_r, logits_r = H.avg_forward_backward(p, tiles, tgt, "vit_tiny", 64)
eng.forward_backward(tiles.to(dev), tgt.to(dev))
torch.cuda.synchronize()
dlog, dl = float((eng.logits.cpu() - logits_r).abs().max()), abs(float(eng.loss) - float(loss_r))
assert dlog <= 2e-2 * float(logits_r.abs().max()) and dl <= 1e-3, (dlog, float(logits_r.abs().max()), dl)
worst, gn = check_grads(eng.grads(), grads_r, ("fc_norm.weight", "fc_norm.bias", "blocks.11.mlp.fc2.bias"))      # grads(): the scale divided out
print(f"avg step vit_tiny: scale {float(eng.scaler.state[0]):g}  logits err {dlog:.2e}  |dloss| {dl:.2e}  worst grad {worst[0]:.2e} ({worst[1]})  "
      f"grad-norm rel {gn:.2e}", flush=True)
print("POOL F16 OK")
