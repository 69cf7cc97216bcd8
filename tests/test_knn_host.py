"""CPU: the k-NN vote entry point refuses bad arguments through the ABI without touching a GPU, its workspace query, the f64
reference the GPU tests hold gv_knn_vote to (pinned against a brute-force loop), the monitor's metric helper (against sklearn and a
hand-computed slide mean) and the driver's --knn-* flags (refusals before any GPU work; inert without --knn-monitor)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def knn_reference(q, bank, labels, k, temp, C):
    """DINO's knn_classifier in f64: (votes [Q, C], top_sim [Q, k] descending, top_idx [Q, k], all similarities [Q, Nb]).
    votes[q, c] = sum over the k most similar bank rows of exp(sim / temp) * [label == c]."""
    sim = q.double() @ bank.double().t()
    top_sim, top_idx = sim.topk(k, dim=1, largest=True, sorted=True)
    w = (top_sim / temp).exp()
    lab = labels.long()[top_idx]
    ok = (lab >= 0) & (lab < C)                                       # a label outside [0, C) votes for nobody
    votes = torch.zeros(q.shape[0], C, dtype=torch.float64)
    votes.scatter_add_(1, lab.clamp(0, C - 1), w * ok)
    return votes, top_sim, top_idx, sim


def knn_inputs(Q, Nb, D, C, seed):
    """The seeded inputs of the GPU cases: normalised random rows, random labels."""
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(Q, D, generator=g), dim=1)
    bank = torch.nn.functional.normalize(torch.randn(Nb, D, generator=g), dim=1)
    labels = torch.randint(0, C, (Nb,), generator=g)
    return q, bank, labels


def _lib():
    from gipvit import _lib as L
    return L


def test_knn_vote_abi_errors():
    L = _lib()
    ok = dict(q=4096, bank=8192, labels=12288, votes=16384, top_sim=20480, top_idx=24576, workspace=28672, workspace_bytes=1 << 30,
              Q=70, Nb=1003, D=192, k=20, C=2, n_split=0, ldq=192, ldb=192, inv_temp=1.0 / 0.07)      # never dereferenced: rejected first

    def rc(**kw):
        return L.lib.gv_knn_vote(ctypes.byref(L.gv_knn_vote_args(**dict(ok, **kw))), None)

    def err():
        return L.lib.gv_last_error().decode()
    assert L.lib.gv_knn_vote(None, None) == -3
    for name in ("q", "bank", "labels", "votes", "workspace"):
        assert rc(**{name: None}) == -3 and "null" in err(), name
    assert rc(Q=0) == -1 and "Q >= 1" in err()
    for k in (0, 65):
        assert rc(k=k) == -1 and "1 <= k <= 64" in err(), k
    assert rc(k=41, Nb=40) == -1 and "k <= Nb" in err()
    for D in (0, 190, 1028):
        assert rc(D=D, ldq=1028, ldb=1028) == -1 and "1024" in err() and "multiple of 4" in err(), D
    for C in (0, 33):
        assert rc(C=C) == -1 and "1 <= C <= 32" in err(), C
    assert rc(ldq=188) == -1 and "ldq >= D" in err()
    assert rc(ldb=188) == -1 and "ldb >= D" in err()
    assert rc(ldq=194) == -2 and "multiples of 4" in err()
    assert rc(ldb=198) == -2 and "multiples of 4" in err()
    assert rc(q=4096 + 4) == -2 and "16-byte aligned" in err()
    assert rc(bank=8192 + 8) == -2 and "16-byte aligned" in err()
    for ns in (-1, 33):
        assert rc(n_split=ns) == -1 and "n_split <= min(32, Nb)" in err(), ns
    assert rc(n_split=6, Nb=5, k=5) == -1 and "n_split" in err()
    need = L.lib.gv_knn_workspace_bytes(70, 1003, 20, 3)
    assert need == 3 * 70 * 20 * 8
    assert rc(n_split=3, workspace_bytes=need - 1) == -1 and str(need) in err() and "workspace" in err()
    assert rc(top_sim=None, top_idx=None, workspace_bytes=0) == -1 and "workspace" in err()      # NULL top-k outputs are not the defect


def test_knn_workspace_bytes():
    L = _lib()
    ws = L.lib.gv_knn_workspace_bytes
    assert ws(1, 1, 1, 0) > 0 and ws(8192, 65536, 20, 0) > 0
    for n_split in (1, 3, 32):                                         # forced split count: one (sim, idx) list per query and split
        assert ws(70, 1003, 20, n_split) == n_split * 70 * 20 * 8
        sizes_q = [ws(Q, 4099, 10, n_split) for Q in (1, 70, 128, 129, 1025, 8192)]
        sizes_k = [ws(130, 4099, k, n_split) for k in (1, 10, 20, 64)]
        assert sizes_q == sorted(sizes_q) and len(set(sizes_q)) == len(sizes_q) and sizes_k == sorted(sizes_k) and len(set(sizes_k)) == len(sizes_k)
    sizes_s = [ws(130, 4099, 10, s) for s in range(1, 33)]
    assert sizes_s == sorted(sizes_s) and len(set(sizes_s)) == 32
    # n_split = 0 resolves as the call would: never more than 32 lists per query, one per split of at least 1024 bank rows
    assert ws(70, 1003, 20, 0) == 70 * 20 * 8 and ws(130, 4099, 10, 0) == 4 * 130 * 10 * 8
    assert ws(8192, 65536, 20, 0) == 4 * 8192 * 20 * 8 and ws(128, 1 << 20, 20, 0) == 32 * 128 * 20 * 8
    for bad in ((0, 10, 1, 0), (1, 10, 0, 0), (1, 10, 65, 0), (1, 10, 11, 0), (1, 10, 1, -1), (1, 10, 1, 33), (1, 10, 1, 11)):
        assert ws(*bad) == -1 and L.lib.gv_last_error().decode().startswith("gv_knn_workspace_bytes"), bad


def test_knn_reference_matches_brute_force():
    Q, Nb, D, k, C, temp = 7, 23, 8, 5, 3, 0.07
    q, bank, labels = knn_inputs(Q, Nb, D, C, seed=5)
    labels[4] = -1
    labels[9] = C                                                      # out-of-range labels vote for nobody
    votes, top_sim, top_idx, sim = knn_reference(q, bank, labels, k, temp, C)
    assert votes.shape == (Q, C) and top_sim.shape == top_idx.shape == (Q, k) and sim.shape == (Q, Nb)
    qd, bd = q.double().tolist(), bank.double().tolist()
    for i in range(Q):
        sims = [sum(a * b for a, b in zip(qd[i], bd[j])) for j in range(Nb)]
        order = sorted(range(Nb), key=lambda j: (-sims[j], j))[:k]
        assert order == top_idx[i].tolist()
        want = [0.0] * C
        for j in order:
            if 0 <= int(labels[j]) < C:
                want[int(labels[j])] += math.exp(sims[j] / temp)
        for c in range(C):
            assert abs(float(votes[i, c]) - want[c]) <= 1e-12 * max(want[c], 1.0), (i, c)
        assert all(abs(float(top_sim[i, r]) - sims[j]) <= 1e-15 for r, j in enumerate(order))
    assert any(4 in top_idx[i].tolist() or 9 in top_idx[i].tolist() for i in range(Q))      # the out-of-range rows were among the neighbours


def test_knn_metrics_against_sklearn_and_hand_computed_slide_mean():
    from sklearn.metrics import roc_auc_score
    from gipvit.knn import knn_metrics
    votes = np.array([[3.0, 1.0], [1.0, 3.0], [2.0, 2.0], [0.5, 1.5], [4.0, 1.0], [1.0, 1.5], [0.0, 2.0], [3.0, 2.0]])
    labels = np.array([0, 0, 0, 1, 1, 1, 1, 0])
    slides = np.array([10, 10, 10, 7, 7, 3, 3, 5])                     # slide 10 (label 0), 7 (1), 3 (1), 5 (0)
    m = knn_metrics(votes, labels, slides)
    assert list(m) == ["knn_top1", "knn_auc_per_patch", "knn_auc_per_slide"]
    # arg-max, the lowest class on a tie: predictions 0 1 0 1 0 1 1 0 -> hits 1 0 1 1 0 1 1 1
    assert m["knn_top1"] == 100.0 * 6 / 8
    score = votes[:, 1] / votes.sum(1)
    assert abs(m["knn_auc_per_patch"] - roc_auc_score(labels, score)) < 1e-12
    slide_score = [(0.25 + 0.75 + 0.5) / 3, (0.75 + 0.2) / 2, (0.6 + 1.0) / 2, 0.4]
    assert abs(m["knn_auc_per_slide"] - roc_auc_score([0, 1, 1, 0], slide_score)) < 1e-12
    assert m["knn_auc_per_slide"] == 0.75                              # 0.5 / 0.475 / 0.8 / 0.4: one of the four (pos, neg) pairs is inverted
    # string slide names work alike; one class only: top-1 alone; one label only: the AUC is NaN, as in validate()
    assert knn_metrics(votes, labels, [f"s{v}" for v in slides]) == m
    assert list(knn_metrics(votes[:, :1], np.zeros(8, dtype=int), slides)) == ["knn_top1"]
    assert math.isnan(knn_metrics(votes, np.zeros(8, dtype=int), slides)["knn_auc_per_patch"])
    with pytest.raises(ValueError):
        knn_metrics(votes, labels[:5], slides)


def _train():
    sys.path.insert(0, ROOT)
    import train
    return train


@pytest.mark.parametrize("flags,word", [
    (["--knn-monitor"], "--knn-monitor"),                                                    # without --dino
    (["--dino", "--knn-monitor", "--knn-k", "0"], "--knn-k"),
    (["--dino", "--knn-monitor", "--knn-k", "65"], "--knn-k"),
    (["--dino", "--knn-monitor", "--knn-temp", "0"], "--knn-temp"),
    (["--dino", "--knn-monitor", "--knn-temp", "-0.07"], "--knn-temp"),
    (["--dino", "--knn-monitor", "--knn-rate", "0"], "--knn-rate"),
    (["--dino", "--knn-monitor", "--eval-metric", "loss"], "--eval-metric"),
    (["--dino", "--knn-monitor", "--test_fold", "-1"], "--test_fold"),
])
def test_driver_refuses_before_any_gpu_work(flags, word):
    train = _train()
    args, _ = train.parse_args(["--model", "vit_tiny"] + flags)
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, lambda m: None)
    assert word in str(e.value)


def test_knn_flags_are_inert_without_the_monitor():
    train = _train()
    base, _ = train.parse_args(["--model", "vit_tiny", "--dino"])
    assert (base.knn_monitor, base.knn_k, base.knn_temp, base.knn_bank_tiles, base.knn_rate) == (False, 20, 0.07, None, 1)
    assert train.check_supported(base, lambda m: None) is None
    # values the monitor would refuse change nothing and are not refused while it is off, with and without --dino
    for extra in (["--dino"], []):
        off, _ = train.parse_args(["--model", "vit_tiny", "--knn-k", "500", "--knn-temp", "-1", "--knn-rate", "0", "--knn-bank-tiles", "0",
                                   "--eval-metric", "loss", "--test_fold", "-1"] + extra)
        assert not off.knn_monitor and train.check_supported(off, lambda m: None) is None
        ref, _ = train.parse_args(["--model", "vit_tiny", "--eval-metric", "loss", "--test_fold", "-1"] + extra)
        differ = {k for k in vars(ref) if getattr(ref, k) != getattr(off, k)}
        assert differ == {"knn_k", "knn_temp", "knn_rate", "knn_bank_tiles"}, differ
    on, _ = train.parse_args(["--model", "vit_tiny", "--dino", "--knn-monitor", "--knn-k", "5", "--knn-temp", "0.1", "--knn-bank-tiles", "7", "--knn-rate", "2"])
    assert train.check_supported(on, lambda m: None) is None and (on.knn_k, on.knn_temp, on.knn_bank_tiles, on.knn_rate) == (5, 0.1, 7, 2)


def test_gap_condition_of_the_gpu_cases():
    """The seeded GPU cases (tests/test_knn_gpu.py) are well posed: every query's f64 gap between its k-th and (k + 1)-th similarity is
    at least 1e-5, so a kernel within 2e-6 of the f64 similarities must return the reference's neighbour set."""
    from test_knn_gpu import CASES
    for Q, Nb, D, k, C, seed in CASES:
        q, bank, labels = knn_inputs(Q, Nb, D, C, seed)
        sim = q.double() @ bank.double().t()
        if k < Nb:
            s = sim.sort(dim=1, descending=True).values
            assert float((s[:, k - 1] - s[:, k]).min()) >= 1e-5, (Q, Nb, D, k, seed)
        assert float((q @ bank.t() - sim).abs().max()) <= 2.5e-7      # a CPU f32 product against f64 on these inputs
