"""The cases of tests/traces/probe_outputs.json and how a case becomes device calls: the four CASES of tests/test_mil_host.py through
gv_mil_train / gv_mil_predict and the four of tests/test_survival_host.py through gv_surv_train / gv_surv_predict.

Shared by the recorder (tools/probe_outputs_record.py), the digest test (tests/test_probe_bits_gpu.py) and, for the training runs
(``mil_train_gpu`` / ``surv_train_gpu``), the reference tests of tests/test_mil_gpu.py and tests/test_survival_gpu.py.  A fixture
row holds the case's name and, under ``sha256``, the SHA-256 of what the recorder's library left: the packed parameters and both
moments after the case's epochs, the ``loss_sum`` rows, and one predict of the trained model with attn and score (the MIL one
with labels: prob and loss; the survival one: risk).  Inputs are built on the CPU from the case tables.  The kernels use no
atomics and every sum has a fixed order, so a build that computes what the recorded one computed reproduces every digest."""
import hashlib
import json
import os

import numpy as np
import torch

import test_mil_host as mh
import test_survival_host as sh

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "traces", "probe_outputs.json")
f32 = torch.float32


def cases():
    return [dict(id="mil_" + n, probe="mil", case=i) for i, n in enumerate(mh.CASE_IDS)] + \
           [dict(id="surv_" + n, probe="surv", case=i) for i, n in enumerate(sh.CASE_IDS)]


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def row_id(r):
    return r["id"]


def pad(x, ldx):
    """x [N, F] as a view with row stride ldx (the padding holds NaN)."""
    buf = torch.full((x.shape[0], ldx), float("nan"), dtype=f32)
    buf[:, :x.shape[1]] = x
    return buf


def poison(kind, dev, *dims):
    """The scratch ops keeps per device for ``kind``, all-ones bit patterns (NaN) for the next call: a slot a launch reads without
    an earlier launch having written it would show as a NaN in the result."""
    from gipvit import ops
    ops._scratch(kind, dev, *dims).fill_(255)


def mil_train_gpu(dev, x, ptr, labels, packed0, perms, batch, L, C, lr, wd, ldx=None, max_bag=None, beta1=mh.BETA1, beta2=mh.BETA2, scale=None):
    """The epochs on the device -> (params, m, v packed, loss_sum per epoch [epochs]), host tensors."""
    from gipvit import ops
    F = x.shape[1]
    xd = (pad(x, ldx).to(dev)[:, :F] if ldx and ldx > F else x.to(dev))
    P = packed0.clone().to(dev)
    m, v = torch.zeros_like(P), torch.zeros_like(P)
    ptr_d, y = torch.from_numpy(np.asarray(ptr).astype(np.int32)).to(dev), torch.as_tensor(np.asarray(labels)).to(dev, torch.int32)
    order = torch.from_numpy(np.asarray(perms).astype(np.int32)).to(dev)
    epochs, n = order.shape
    mb = int(np.diff(np.asarray(ptr)).max()) if max_bag is None else max_bag
    loss = torch.zeros(epochs, 1, dtype=f32, device=dev)
    poison("mil", dev, batch, mb, L, C, F)
    steps = -(-n // batch)
    for e in range(epochs):
        ops.mil_train(P, m, v, xd, ptr_d, y, order[e], loss[e], L, C, batch, mb, e * steps, lr, mh.cosine_scale(e, epochs) if scale is None else scale,
                      wd, beta1, beta2, mh.EPS)
    torch.cuda.synchronize()
    return P.cpu(), m.cpu(), v.cpu(), loss.cpu().reshape(-1)


def surv_train_gpu(dev, x, ptr, time, event, packed0, perms, batch, L, lr, wd, ldx=None, max_bag=None, beta1=mh.BETA1, beta2=mh.BETA2, scale=None,
                   step0=None, state=None):
    """The epochs on the device -> (params, m, v packed, loss_sum per epoch [epochs, 2]), host tensors."""
    from gipvit import ops
    F = x.shape[1]
    xd = (pad(x, ldx).to(dev)[:, :F] if ldx and ldx > F else x.to(dev))
    P = packed0.clone().to(dev)
    m, v = (torch.zeros_like(P), torch.zeros_like(P)) if state is None else (state[0].clone().to(dev), state[1].clone().to(dev))
    ptr_d = torch.from_numpy(np.asarray(ptr).astype(np.int32)).to(dev)
    t_d = torch.from_numpy(np.asarray(time, dtype=np.float32)).to(dev)
    e_d = torch.from_numpy(np.asarray(event).astype(np.int32)).to(dev)
    order = torch.from_numpy(np.asarray(perms).astype(np.int32)).to(dev)
    epochs, n = order.shape
    mb = int(np.diff(np.asarray(ptr)).max()) if max_bag is None else max_bag
    loss = torch.zeros(epochs, 2, dtype=f32, device=dev)
    poison("surv", dev, batch, mb, L, F)
    steps = -(-n // batch)
    for e in range(epochs):
        ops.surv_train(P, m, v, xd, ptr_d, t_d, e_d, order[e], loss[e], L, batch, mb, e * steps if step0 is None else step0, lr,
                       mh.cosine_scale(e, epochs) if scale is None else scale, wd, beta1, beta2, mh.EPS)
    torch.cuda.synchronize()
    return P.cpu(), m.cpu(), v.cpu(), loss.cpu()


def run(row, dev):
    """One row: the case's epochs, then one predict of the trained model -> {output name: host tensor}."""
    from gipvit import ops
    mil = row["probe"] == "mil"
    mod = mh if mil else sh
    c = mod.CASES[row["case"]]
    s = mod.case_setup(c)
    L, F, C = c["L"], c["F"], c.get("C", 1)
    packed0 = mh.pack(s["params0"], L, C, F)
    if mil:
        P, m, v, loss_sum = mil_train_gpu(dev, s["x"], s["ptr"], s["labels"], packed0, s["perms"], c["batch"], L, C, c["lr"], c["wd"], ldx=c["ldx"])
    else:
        P, m, v, loss_sum = surv_train_gpu(dev, s["x"], s["ptr"], s["time"], s["event"], packed0, s["perms"], c["batch"], L, c["lr"], c["wd"],
                                           ldx=c["ldx"])
    n, mb = len(c["sizes"]), max(c["sizes"])
    x = pad(s["x"], c["ldx"]).to(dev)[:, :F]
    ptr = torch.from_numpy(s["ptr"].astype(np.int32)).to(dev)
    if mil:
        poison("mil", dev, min(n, 64), mb, L, C, F)
        out = ops.mil_predict(P.to(dev), x, ptr, L, C, mb, labels=s["labels"].to(dev, torch.int32), want_attn=True, want_score=True)
    else:
        poison("surv", dev, min(n, 64), mb, L, F)
        out = ops.surv_predict(P.to(dev), x, ptr, L, mb, want_attn=True, want_score=True)
    torch.cuda.synchronize()
    return dict(params=P, m=m, v=v, loss_sum=loss_sum, **{k: t.cpu() for k, t in out.items()})


def digests(out):
    """{name: SHA-256 of the f32 buffer's bytes on the host}"""
    return {name: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for name, t in out.items()}
