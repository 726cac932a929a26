"""Long-horizon parity (BASELINE.json metric: "... + AUC parity"): the HIP model and the CPU oracle start from the same
parameters and train for 120 optimizer steps on the bundled Tmall sample (configs[0]; the loop of
train_score.py:219-258 with its periodic validation pass, :144-163) -- every step's training loss, and every
evaluation's validation log-loss / AUC / MRR / NDCG@10, must stay together.  Every other HIP-vs-oracle comparison in
this suite stops after 1 - 3 optimizer steps.  Also: the same trajectory through two virtual ranks of the row-sharded
path, and one step at configs[1]'s exact shape (B = 256) against the oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import NAMES, batch_tuple
from test_gpu_cfg1 import pipeline, _loader      # noqa: F401  (module fixture: the sample's graph and target lines)

pytestmark = pytest.mark.gpu

STEPS, EVAL_EVERY, BATCH = 120, 60, 32      # (validation at steps 0, 60 and 120: each is 43 oracle passes of 100 candidates)


def _sample_batches(pipeline):
    c, g, r, targets = pipeline
    T = c["time_slice_num"] - c["start_time"] - 1
    args = (r["feature_size"], c["eb_dim"], c["hidden_size"], T, c["obj_per_time_slice"], c["user_fnum"], c["item_fnum"])
    train = [tuple(t.cpu().numpy() for t in b.tensors) for b in _loader(c, g, targets, "train", BATCH)]
    vali = [tuple(t.cpu().numpy() for t in b.tensors) for b in _loader(c, g, targets, "validation", 100)]        # 43 lines x (1 + 99)
    return args, train, vali


def _evaluate(model, vali, lam):
    from score_amd import harness
    return harness.evaluate(model, vali, lam)       # (logloss, auc, ndcg_5, ndcg_10, hr_1, hr_5, hr_10, mrr, mean loss)


def _check_eval(step, eg, eo):
    assert abs(eg[0] - eo[0]) < 1e-3, ("validation log-loss", step, eg[0], eo[0])
    assert round(eg[1], 3) == round(eo[1], 3) or abs(eg[1] - eo[1]) < 5e-4, ("validation AUC", step, eg[1], eo[1])
    assert abs(eg[7] - eo[7]) < 1e-3 and abs(eg[3] - eo[3]) < 1e-3, ("MRR / NDCG@10", step, eg[7], eo[7], eg[3], eo[3])


def test_120_steps_stay_on_the_oracles_trajectory(pipeline):
    from score_amd.model import SCORE
    args, train, vali = _sample_batches(pipeline)
    cfg = so.Cfg(*args, model_type="SCORE")
    P = so.init_params(cfg, 3)
    m = SCORE(*args)
    m.set_params(P)
    om = so.OracleModel(*args, model_type="SCORE", params={k: v.copy() for k, v in P.items()})
    lam, lr = 1e-4, 1e-3
    worst, olosses = 0.0, []
    for step in range(STEPS):
        if step % EVAL_EVERY == 0:
            _check_eval(step, _evaluate(m, vali, lam), _evaluate(om, vali, lam))
        b = train[step % len(train)]
        lg = m.train(None, b, lr, lam, keep_prob=1.0)
        lo = om.train(None, b, lr, lam, keep_prob=1.0)
        olosses.append(lo)
        worst = max(worst, abs(lg - lo) / max(abs(lo), 1e-6))
        assert abs(lg - lo) < 1e-3 * max(abs(lo), 1e-6), (step, lg, lo)
    eg, eo = _evaluate(m, vali, lam), _evaluate(om, vali, lam)
    _check_eval(STEPS, eg, eo)
    # the run learned something (the check above is not two constant predictors agreeing)
    assert np.mean(olosses[-6:]) < 0.7 * np.mean(olosses[:6])
    print("worst relative training-loss gap over %d steps: %.2e; final validation AUC %.4f / %.4f" % (STEPS, worst, eg[1], eo[1]))


def test_two_virtual_ranks_follow_one_device_for_120_steps(pipeline):
    """the row-sharded path (table rows on rank row % 2, all-to-all exchanges in-process) on the sample: rank r trains on
    the r-th half of every batch, the single device on the whole batch -- same losses along the whole run, same validation
    metrics at the end"""
    from score_amd.dist import ShardedSCORE
    from score_amd.model import SCORE
    from test_gpu_dist import run_ranks
    args, train, vali = _sample_batches(pipeline)
    train = [b for b in train if b[6].shape[0] % 2 == 0]
    cfg = so.Cfg(*args, model_type="SCORE")
    P = so.init_params(cfg, 3)
    lam, lr = 1e-4, 1e-3

    def half(b, r):
        n = b[6].shape[0] // 2
        return tuple(x[r * n:(r + 1) * n] for x in b)

    def fn(rank, comm):
        m = ShardedSCORE(*args, comm=comm, model_type="SCORE")
        m.backend.m.set_params(P)
        losses = []
        for step in range(STEPS):
            b = half(train[step % len(train)], rank)
            nb = half(train[(step + 1) % len(train)], rank) if step + 1 < STEPS else None
            losses.append(m.train(None, b, lr, lam, keep_prob=1.0, next_batch=nb))
        preds = [m.eval(None, half(v, rank), lam)[0] for v in vali]
        torch.cuda.synchronize()
        return losses, preds

    res = run_ranks(2, fn)
    ref = SCORE(*args)
    ref.set_params(P)
    for step in range(STEPS):
        lref = ref.train(None, train[step % len(train)], lr, lam, keep_prob=1.0)
        for r in range(2):
            assert abs(res[r][0][step] - lref) < 1e-3 * max(abs(lref), 1e-6), (step, r, res[r][0][step], lref)
    # validation predictions after the 120 steps: the two runs add their gradients in different orders, and 120 Adam steps amplify
    # that (measured: largest |dp| 1.3e-2 on one of 4,300 candidates, mean 2.1e-4) -- so the bound on a single prediction
    # is loose, the one on their mean and on the AUC is not
    from sklearn.metrics import roc_auc_score
    pr, pg, labels = [], [], []
    for i, v in enumerate(vali):
        pr += ref.eval(None, v, lam)[0]
        pg += list(res[0][1][i]) + list(res[1][1][i])
        labels += v[6].tolist()
    pr, pg = np.asarray(pr), np.asarray(pg)
    assert np.abs(pg - pr).max() < 3e-2 and np.abs(pg - pr).mean() < 5e-4, (np.abs(pg - pr).max(), np.abs(pg - pr).mean())
    assert abs(roc_auc_score(labels, pg) - roc_auc_score(labels, pr)) < 5e-4


@pytest.mark.parametrize("seed", [7, 1, 2, 3, 4])
def test_cfg2_exact_shape_one_step_vs_oracle(seed):
    """BASELINE.json configs[1] at its own shape and batch size (U = 100 K, I = 50 K, T = 10, K = 5, D = 16, H = 32, B = 256):
    gradients, two TF-Adam steps and the predictions against the oracle (smoke() runs the shape at B = 64).  Arbitrary batches
    (until round 5: the one batch whose relu pre-activations all kept 1e-5 from the kink): the first 256
    samples of two loader batches that own no relu unit within 1e-5 of its kink (helpers.away_from_relu_kinks)"""
    from score_amd.synth import make_world
    from helpers import away_from_relu_kinks
    from test_gpu_model import make_model, close, LOGIT_TOL
    world, kw = make_world("cfg2")
    B = kw.pop("batch")
    assert B == 256
    cfg = so.Cfg(kw["feature_size"], kw["eb_dim"], kw["hidden_size"], kw["max_time_len"], kw["obj_per_time_slice"],
                 kw["user_fnum"], kw["item_fnum"], "SCORE")
    P = so.init_params(cfg, 11)
    pool = [dict(zip(NAMES, world.batch(B, s_))) for s_ in (seed, seed + 100)]
    pool = {k: np.concatenate([np.asarray(p_[k]) for p_ in pool]) for k in NAMES}
    # what the oracle's forward pass alone (on the CPU) drops from the pool of 512 at thr = 1e-5, per seed; the cap is that plus 2
    counted = {7: 6, 1: 5, 2: 6, 3: 5, 4: 2}
    b, _, keep = away_from_relu_kinks(cfg, P, pool, max_dropped=counted[seed] + 2)
    assert keep.size >= B
    b = {k: np.ascontiguousarray(v[:B]) for k, v in b.items()}
    m = make_model(cfg, P)
    assert m.persample_form(B, 8)            # (the per-sample whole-model kernels: csrc/persample.h)
    m.forward_backward(batch_tuple(b), 0.0, 1.0)
    g = m.get_grads()
    oo, go = so.loss_and_grads(cfg, P, b, 0.0)
    rows = np.unique(np.concatenate([b[k].ravel() for k in NAMES[:6]]))
    for k in go:
        a, o = g[k].reshape(np.asarray(go[k]).shape), np.asarray(go[k])
        if k == "emb_mtx":
            a, o = a[rows], o[rows]
        ok, err = close(a, o, rtol=3e-4, atol=2e-6)
        assert ok, (k, err, oo["relu_margin"])
    assert oo["relu_margin"] >= 1e-5
    if seed != 7:
        return                                     # (the optimizer steps and the AUC on one batch: the others add nothing to them)
    om = so.OracleModel(cfg.N, cfg.D, cfg.H, cfg.T, cfg.K, cfg.Fu, cfg.Fi, "SCORE", params={k: v.copy() for k, v in P.items()})
    for _ in range(2):
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        lo = om.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo))
    pg, lab, _ = m.eval(None, batch_tuple(b), 1e-4)
    po, _, _ = om.eval(None, batch_tuple(b), 1e-4)
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < LOGIT_TOL
    from sklearn.metrics import roc_auc_score
    assert round(roc_auc_score(lab, pg), 4) == round(roc_auc_score(lab, po), 4)
