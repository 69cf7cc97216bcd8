"""GPU: gv_knn_vote against the f64 reference of tests/test_knn_host.py (neighbour sets, similarities, votes), its invariance to
the number of bank splits, the tie rule, strided queries / NULL top-k outputs, the monitor on a real encoder and the driver."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from test_knn_host import knn_inputs, knn_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TEMP = 0.07
# (Q, Nb, D, k, C, seed): a ragged query tile, a ragged last chunk, every encoder width, k = 64, k == Nb < one chunk, two query
# tiles x four splits.  f64 gap between the k-th and (k + 1)-th similarity >= 1e-5 for every query of every case (asserted below).
CASES = [(70, 1003, 192, 20, 2, 3), (70, 1003, 384, 20, 2, 1), (33, 517, 768, 64, 5, 0), (5, 40, 192, 40, 3, 0), (130, 4099, 384, 10, 2, 0)]
_ref_cache = {}


def _case(case):
    """Inputs and f64 reference of a case, computed once and shared (never modified)."""
    if case not in _ref_cache:
        Q, Nb, D, k, C, seed = case
        q, bank, labels = knn_inputs(Q, Nb, D, C, seed)
        _ref_cache[case] = (q, bank, labels) + knn_reference(q, bank, labels, k, TEMP, C)
    return _ref_cache[case]


def _poisoned_workspace(dev, Q, Nb, k, n_split=0):
    """The scratch ops.knn_vote keeps per device, all-ones (similarity NaN, index -1) for the next call: made large enough here, so
    that the call takes this buffer and not fresh, mostly zero, torch.empty memory.  The merge takes a list entry as an index only
    inside [0, Nb) (csrc/knn.hip), so a slot the scan never stored shows as a missing neighbour / NaN similarity, never as a read."""
    from gipvit import ops
    ops._scratch("knn", dev, Q, Nb, k, n_split).fill_(255)


def _vote(dev, q, bank, labels, k, C, n_split=0, want_topk=True):
    from gipvit import ops
    _poisoned_workspace(dev, q.shape[0], bank.shape[0], k, n_split)
    out = ops.knn_vote(q.to(dev), bank.to(dev), labels.to(dev, torch.int32), k, TEMP, C, n_split=n_split, want_topk=want_topk)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out) if want_topk else out.cpu()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "Q%d-Nb%d-D%d-k%d-C%d" % c[:5])
def test_knn_vote_matches_reference(dev, case):
    Q, Nb, D, k, C, seed = case
    q, bank, labels, votes_ref, sim_ref, idx_ref, sim = _case(case)
    if k < Nb:
        s = sim.sort(dim=1, descending=True).values
        gap = float((s[:, k - 1] - s[:, k]).min())
        print(f"min f64 gap between similarity k and k + 1: {gap:.3e}")
        assert gap >= 1e-5                                               # for every query: none is excluded
    votes, top_sim, top_idx = _vote(dev, q, bank, labels, k, C)
    assert votes.shape == (Q, C) and top_sim.shape == (Q, k) and top_idx.shape == (Q, k) and top_idx.dtype == torch.int32
    assert int(top_idx.min()) >= 0 and int(top_idx.max()) < Nb
    assert torch.equal(top_idx.long().sort(dim=1).values, idx_ref.sort(dim=1).values)       # the neighbour SET of every query
    assert bool((top_sim[:, 1:] <= top_sim[:, :-1]).all())
    serr = float((top_sim.double() - sim.gather(1, top_idx.long())).abs().max())
    verr = float(((votes.double() - votes_ref).abs() / votes_ref.abs().clamp_min(1e-300)).max())
    print(f"max |top_sim - f64 similarity of the returned rows| {serr:.3e}, max relative vote error {verr:.3e}")
    assert serr <= 2e-6
    assert bool(((votes_ref > 0) | (votes == 0)).all()) and verr <= 1e-4


@pytest.mark.parametrize("case", [CASES[0], CASES[-1]], ids=["Q70-Nb1003", "Q130-Nb4099"])
def test_knn_vote_is_invariant_to_the_split_count(dev, case):
    Q, Nb, D, k, C, seed = case
    q, bank, labels = _case(case)[:3]
    outs = [_vote(dev, q, bank, labels, k, C, n_split=s) for s in (1, 3, 0)]
    for votes, top_sim, top_idx in outs[1:]:
        assert torch.equal(top_idx.sort(dim=1).values, outs[0][2].sort(dim=1).values)
        assert torch.equal(top_sim.view(torch.int32), outs[0][1].view(torch.int32))          # bitwise
        assert torch.equal(top_idx, outs[0][2]) and torch.equal(votes, outs[0][0])            # same order: same sums
    again = _vote(dev, q, bank, labels, k, C, n_split=3)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, outs[1]))      # and run to run


@pytest.mark.parametrize("n_split", [1, 2])
def test_knn_vote_tie_rule(dev, n_split):
    """Every bank row twice (i and i + 64): among equal similarities the smaller index ranks first, so a query's result holds both
    copies, or i alone, or neither -- never i + 64 alone -- whichever split a copy lives in."""
    Q, D, k, H = 9, 192, 21, 64
    g = torch.Generator().manual_seed(2)
    q = torch.nn.functional.normalize(torch.randn(Q, D, generator=g), dim=1)
    h = torch.nn.functional.normalize(torch.randn(H, D, generator=g), dim=1)
    labels = torch.randint(0, 2, (2 * H,), generator=g)
    votes, top_sim, top_idx = _vote(dev, q, torch.cat([h, h]), labels, k, 2, n_split=n_split)
    bits = top_sim.view(torch.int32)
    lone = 0
    for r in range(Q):
        got = top_idx[r].tolist()
        assert len(set(got)) == k and bool((top_sim[r, 1:] <= top_sim[r, :-1]).all())
        for i in range(H):
            assert not (i + H in got and i not in got), (r, i)
            if i in got and i + H in got:
                assert int(bits[r, got.index(i)]) == int(bits[r, got.index(i + H)])           # the copies' similarities are bitwise equal
                assert got.index(i) + 1 == got.index(i + H)                                   # ... and the smaller index comes first
            lone += i in got and i + H not in got
    assert lone == Q                                                       # k is odd: every query's last neighbour is a lone first copy


def test_knn_vote_strided_queries_and_null_outputs(dev):
    from gipvit import ops
    case = CASES[0]
    Q, Nb, D, k, C, seed = case
    q, bank, labels, votes_ref = _case(case)[:4]
    wide = torch.full((Q, D + 8), 7.0, device=dev)
    wide[:, 4:4 + D] = q.to(dev)
    qs = wide[:, 4:4 + D]                                                  # row stride D + 8, base 16 bytes into the buffer
    assert qs.stride() == (D + 8, 1) and qs.data_ptr() % 16 == 0
    votes, top_sim, top_idx = _vote(dev, q, bank, labels, k, C)
    _poisoned_workspace(dev, Q, Nb, k)
    v2, s2, i2 = ops.knn_vote(qs, bank.to(dev), labels.to(dev, torch.int32), k, TEMP, C, want_topk=True)
    _poisoned_workspace(dev, Q, Nb, k)
    v3 = ops.knn_vote(qs, bank.to(dev), labels.to(dev, torch.int32), k, TEMP, C)      # votes only: top_sim / top_idx NULL
    torch.cuda.synchronize()
    assert torch.equal(v2.cpu(), votes) and torch.equal(s2.cpu(), top_sim) and torch.equal(i2.cpu(), top_idx) and torch.equal(v3.cpu(), votes)
    assert float(((votes.double() - votes_ref).abs() / votes_ref).max()) <= 1e-4
    # labels outside [0, C) vote for nobody and are never used as an index
    bad = labels.clone()
    bad[::3] = -5
    bad[1::3] = C + 1000000
    vb = _vote(dev, q, bank, bad, k, C, want_topk=False)
    vref = knn_reference(q, bank, bad, k, TEMP, C)[0]
    assert float((vb.double() - vref).abs().max() / vref.max()) <= 1e-4
    with pytest.raises(TypeError):
        ops.knn_vote(qs.double(), bank.to(dev), labels.to(dev, torch.int32), k, TEMP, C)
    with pytest.raises(ValueError):
        ops.knn_vote(qs, torch.zeros(Nb, 2 * D, device=dev)[:, ::2], labels.to(dev, torch.int32), k, TEMP, C)      # column stride 2


def _monitor(dev, img, seed=0):
    from gipvit.engine import FeatureExtractor
    from gipvit.knn import KnnMonitor
    from gipvit import models as M
    runner = FeatureExtractor("vit_tiny", img, batch=8, device=dev)
    runner.load_state(M.init_vit_state("vit_tiny", img, 0, seed=seed))
    return runner, KnnMonitor(runner, k=5, temp=TEMP, num_classes=2)


def test_monitor_matches_reference_on_the_runners_features(dev):
    from gipvit import data as D
    from gipvit.knn import knn_metrics
    runner, mon = _monitor(dev, 64)
    bank_loader, query_loader = D.SyntheticSlides(4, 12, 64, tiles_per_iter=5, seed=11), D.SyntheticSlides(4, 12, 64, tiles_per_iter=7, seed=23)
    assert mon.build_bank(bank_loader) == 48 and mon.bank.shape == (48, 192) and mon.bank.dtype == torch.float32
    assert mon.bank_labels.dtype == torch.int32 and mon.bank_labels.tolist() == [0] * 12 + [1] * 12 + [0] * 12 + [1] * 12
    got = mon.evaluate(query_loader)
    assert list(got) == ["knn_top1", "knn_auc_per_patch", "knn_auc_per_slide"]
    # the same numbers from the runner's own features through the f64 reference
    def feats(loader):
        f = torch.cat([runner.run(mb["Data"].to(dev))[0] for mb in loader]).cpu()
        return torch.nn.functional.normalize(f.double(), dim=1)
    fb, fq = feats(bank_loader), feats(query_loader)
    assert float((mon.bank.cpu().double() - fb).abs().max()) <= 1e-6     # gv_l2norm_fwd_f32 of the same rows
    lab = torch.tensor([0] * 12 + [1] * 12 + [0] * 12 + [1] * 12)
    votes, _, _, sim = knn_reference(fq, fb, lab, 5, TEMP, 2)
    s = sim.sort(dim=1, descending=True).values
    print(f"min f64 gap between similarity 5 and 6: {float((s[:, 4] - s[:, 5]).min()):.3e}")
    assert float((s[:, 4] - s[:, 5]).min()) >= 1e-5                      # well posed: an f32 product cannot change a neighbour set
    want = knn_metrics(votes.numpy(), lab.numpy(), np.repeat(np.arange(4), 12))
    print("monitor", dict(got), "reference", dict(want))
    assert got["knn_top1"] == want["knn_top1"]
    assert abs(got["knn_auc_per_patch"] - want["knn_auc_per_patch"]) <= 1e-6 and abs(got["knn_auc_per_slide"] - want["knn_auc_per_slide"]) <= 1e-6
    assert 0.0 <= got["knn_top1"] <= 100.0 and 0.0 <= got["knn_auc_per_patch"] <= 1.0
    # slides whose label is outside [0, C) are left out of the bank
    one = type(mon)(runner, k=5, temp=TEMP, num_classes=1)
    assert one.build_bank(bank_loader) == 24 and list(one.evaluate(query_loader)) == ["knn_top1"]


def test_monitor_feeds_the_centred_window_of_larger_tiles(dev):
    from gipvit import data as D
    runner, mon = _monitor(dev, 64)
    loader = D.SyntheticSlides(2, 6, 96, tiles_per_iter=4, seed=5)       # 96-px tiles into the 64-px runner
    assert mon.build_bank(loader) == 12
    manual = torch.cat([runner.run(mb["Data"][:, 16:80, 16:80, :].contiguous().to(dev))[0] for mb in loader])
    manual = torch.nn.functional.normalize(manual.double(), dim=1).cpu()
    assert float((mon.bank.cpu().double() - manual).abs().max()) <= 1e-6
    edge = torch.cat([runner.run(mb["Data"][:, :64, :64, :].contiguous().to(dev))[0] for mb in loader])
    assert float((mon.bank.cpu().double() - torch.nn.functional.normalize(edge.double(), dim=1).cpu()).abs().max()) > 1e-4      # not the corner window
    assert set(mon.evaluate(D.SyntheticSlides(2, 5, 96, tiles_per_iter=4, seed=6))) == {"knn_top1", "knn_auc_per_patch", "knn_auc_per_slide"}


def test_driver_writes_knn_metrics_and_picks_model_best_on_them(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import train
    base = ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "1024", "--batches-per-epoch", "2", "--epochs", "2",
            "--lr", "1e-4", "--warmup-epochs", "0", "--log-interval", "1", "--output", str(tmp_path), "--seed", "3", "--knn-monitor", "--knn-k", "5"]
    names = ["eval_knn_top1", "eval_knn_auc_per_patch", "eval_knn_auc_per_slide"]
    assert train.main(base + ["--experiment", "every"]) == 0
    rows = list(csv.DictReader(open(tmp_path / "every" / "summary.csv")))
    assert len(rows) == 2
    for r in rows:
        assert 0.0 <= float(r["eval_knn_top1"]) <= 100.0 and all(0.0 <= float(r[n]) <= 1.0 for n in names[1:]) and float(r["train_loss"]) > 0
    best = torch.load(tmp_path / "every" / "model_best.pth.tar", weights_only=True)
    top1 = [float(r["eval_knn_top1"]) for r in rows]
    assert best["metric"] == max(top1) and best["epoch"] == (1 if top1[1] > top1[0] else 0)      # increasing, chosen on knn_top1
    assert torch.load(tmp_path / "every" / "last.pth.tar", weights_only=True)["metric"] == top1[1]
    # --knn-rate 2: the first epoch is not evaluated, the columns stay; --eval-metric auc_per_slide resolves to knn_auc_per_slide
    assert train.main(base + ["--experiment", "second", "--knn-rate", "2", "--eval-metric", "auc_per_slide"]) == 0
    rows = list(csv.DictReader(open(tmp_path / "second" / "summary.csv")))
    assert len(rows) == 2 and all(rows[0][n] == "" for n in names) and all(rows[1][n] != "" for n in names)
    best = torch.load(tmp_path / "second" / "model_best.pth.tar", weights_only=True)
    assert best["epoch"] == 1 and best["metric"] == float(rows[1]["eval_knn_auc_per_slide"])
    assert "metric" not in torch.load(tmp_path / "second" / "checkpoint-0.pth.tar", weights_only=True)
