"""The line-form ranking pass on the GPU (GRU4Rec.rank / Caser.rank; csrc/rank.hip, score_rank_forward): a target line's history
encoded once, its candidates scored by one head launch.  Against the float64 restatement of the split head (tests/rank_cases.py)
and against eval on the same expanded batch -- the bounds tests/test_gpu_gru4rec.py::_check holds the pass to --, the ranks the
two give, lengths and ids at their edges, verify=True, and evaluate_device(shared_history=True) on the bundled Tmall sample."""
import functools
import os

import numpy as np
import pytest
import torch

import rank_cases as rc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

Y_TOL, LOSS_TOL = 1e-4, 2e-5              # max |dy| ; |dloss| relative to max(1, |loss|): test_gpu_gru4rec.py::_check
E2E_GAP = 2e-4                            # the end-to-end test's gap condition on eval's scores
E2E_MAX_EXCLUDED = 2                      # lines of the sample it may set aside


def _model(kind, c, P, flags=0, **kw):
    from score_amd import model as M
    m = M.MODELS[kind](*c.args, **kw)
    m.set_params(P)
    m.debug_flags = flags
    return m


@functools.lru_cache(maxsize=None)
def _want(i, reg):
    """the restatement of case i (computed once per (case, reg_lambda), never modified)"""
    kind, c, P, b, L, n_cand = rc.case(i)
    y, loss = rc.restated(kind, c, P, b, L, n_cand, reg)
    y.setflags(write=False)
    return y, loss


def _hold(what, y, loss, want_y, want_loss):
    dy = float(np.abs(np.asarray(y, dtype=np.float64) - want_y).max())
    print(what, "loss", loss, want_loss, "max |dy|", dy)
    assert dy < Y_TOL, (what, dy)
    assert abs(loss - want_loss) < LOSS_TOL * max(1.0, abs(want_loss)), (what, loss, want_loss)


def _rank_and_eval(m, bt, reg, n_cand, what, want=None):
    """rank and eval on one batch, held to each other and (where given) to the restatement -> (rank's y, eval's y)"""
    y, lab, loss = m.rank(None, bt, reg, neg_sample_num=n_cand - 1)
    ey, elab, eloss = m.eval(None, bt, reg)
    assert lab == elab == np.asarray(bt[4]).tolist() and len(y) == len(ey) == len(lab)
    if want is not None:
        _hold(what + " rank vs restatement", y, loss, *want)
        _hold(what + " eval vs restatement", ey, eloss, *want)
    _hold(what + " rank vs eval", y, loss, np.asarray(ey, dtype=np.float64), eloss)
    return np.asarray(y, dtype=np.float32), np.asarray(ey, dtype=np.float32)


@pytest.mark.parametrize("i", range(len(rc.CASES)), ids=rc.IDS)
def test_rank_against_the_restatement_and_eval(i):
    kind, c, P, b, L, n_cand = rc.case(i)
    m = _model(kind, c, P)
    bt = rc.REF[kind].batch_tuple(b)
    for reg in (0.0, 1e-3):
        _rank_and_eval(m, bt, reg, n_cand, "%s reg %g" % (rc.IDS[i], reg), _want(i, reg))


@pytest.mark.parametrize("i", [0, 7, 9], ids=[rc.IDS[0], rc.IDS[7], rc.IDS[9]])
def test_rank_with_biases_and_bn1_off_their_initial_values(i):
    """fc1's bias enters once, through the line part, and bn1's beta on both sides of the split: blind at TF's initial zeros"""
    kind, c, P, b, L, n_cand = rc.case(i, moved=True)
    m = _model(kind, c, P)
    for reg in (0.0, 1e-3):
        _rank_and_eval(m, rc.REF[kind].batch_tuple(b), reg, n_cand, rc.IDS[i] + " moved", rc.restated(kind, c, P, b, L, n_cand, reg))


@pytest.mark.parametrize("i", range(len(rc.CASES)), ids=rc.IDS)
def test_rank_and_eval_give_equal_ranks(i):
    """A condition on the inputs, not a tolerance: every line's positive is at least MIN_GAP from every negative (asserted from
    the restatement alone), ten times the bound both passes are held to -- so the positive's rank cannot differ."""
    from score_amd import harness as h
    kind, c, P, b, L, n_cand = rc.case(i)
    gaps = rc.line_gaps(_want(i, 0.0)[0], L, n_cand)
    print(rc.IDS[i], "smallest positive-to-negative gap %.3g" % float(gaps.min()))
    assert gaps.min() >= rc.MIN_GAP
    m = _model(kind, c, P)
    bt = rc.REF[kind].batch_tuple(b)
    y, ey = _rank_and_eval(m, bt, 0.0, n_cand, rc.IDS[i])
    ids = torch.from_numpy(np.ascontiguousarray(b["target_item"][:, 0])).cuda()
    got, ranks = h.ranking_quality_device(torch.from_numpy(y).cuda(), ids, n_cand - 1, return_ranks=True)
    want, eranks = h.ranking_quality_device(torch.from_numpy(ey).cuda(), ids, n_cand - 1, return_ranks=True)
    print(rc.IDS[i], "ranks", ranks.tolist(), "metrics", got)
    assert torch.equal(ranks, eranks) and got == want


def _g4r_lines(L=3, n_cand=10, seed=1, dims=(16, 32, 9, 3, 4)):
    c = rc.cfg_of("GRU4Rec", dims)
    return c, rc.params_of("GRU4Rec", c), rc.line_batch("GRU4Rec", c, L, n_cand, seed)


def test_lines_of_length_one_T_and_above_T_in_one_batch():
    L, n_cand = 3, 10
    c, P, b = _g4r_lines(L, n_cand)
    b["user_seq_length"] = np.repeat(np.asarray([1, c.T, c.T + 3], dtype=np.int32), n_cand)
    m = _model("GRU4Rec", c, P)
    _rank_and_eval(m, rc.REF["GRU4Rec"].batch_tuple(b), 1e-3, n_cand, "lengths 1, T, T + 3",
                   rc.restated("GRU4Rec", c, P, b, L, n_cand, 1e-3))


def test_active_slices_from_the_model_against_all_slices():
    """lengths <= 4 < T = 9: the batch computes 4 slices (score_rank_batch_t.active_slices from the model) or all of them"""
    L, n_cand = 3, 10
    c, P, b = _g4r_lines(L, n_cand)
    b["user_seq_length"] = np.repeat(np.asarray([2, 4, 1], dtype=np.int32), n_cand)
    bt = rc.REF["GRU4Rec"].batch_tuple(b)
    want = rc.restated("GRU4Rec", c, P, b, L, n_cand, 0.0)
    m = _model("GRU4Rec", c, P)
    assert m.device_batch(bt).active_slices == 4
    ya, _ = _rank_and_eval(m, bt, 0.0, n_cand, "active slices 4", want)
    m.skip_masked_slices = False
    assert m.device_batch(bt).active_slices == 0
    y0, _ = _rank_and_eval(m, bt, 0.0, n_cand, "all slices", want)
    assert np.abs(ya.astype(np.float64) - y0).max() < Y_TOL


@pytest.mark.parametrize("kind,i", [("GRU4Rec", 2), ("Caser", 7)])
def test_a_candidate_with_the_dummy_id(kind, i):
    """id 0 is the masked row: a whole candidate of zeros, and one field of another candidate"""
    _, c, P, b, L, n_cand = rc.case(i)
    b["target_item"][n_cand + 1, :] = 0
    b["target_item"][L * n_cand - 1, c.Fi - 1] = 0
    _rank_and_eval(_model(kind, c, P), rc.REF[kind].batch_tuple(b), 0.0, n_cand, kind + " id 0", rc.restated(kind, c, P, b, L, n_cand))


@pytest.mark.parametrize("field,named", [("target_item", "batch_data[3] (target_item)"), ("user_seq", "batch_data[0] (user_seq)"),
                                         ("target_user", "batch_data[2] (target_user)")])
def test_an_id_outside_the_table_raises_and_the_next_call_succeeds(field, named):
    """feature_size itself, in the last candidate of the last line's ragged tile (or in the line's own tensors): a NaN loss, a
    ValueError that names the tensor, no variable touched, and the next good call gives what a fresh model gives"""
    L, n_cand = 3, 17
    c, P, good = _g4r_lines(L, n_cand, seed=3, dims=(16, 16, 9, 3, 4))
    good["user_seq_length"][:] = c.T
    m, clean = _model("GRU4Rec", c, P), _model("GRU4Rec", c, P)
    bad = {k: v.copy() for k, v in good.items()}
    if field == "target_item":
        bad[field][L * n_cand - 1, 0] = c.N
    else:       # (the line's first sample is the one the pass reads)
        bad[field][(2 * n_cand,) + (0,) * (bad[field].ndim - 1)] = c.N
    bt = rc.REF["GRU4Rec"].batch_tuple
    _, _, loss = m.rank_async(bt(bad), 1e-4, neg_sample_num=n_cand - 1)
    assert torch.isnan(loss).item()
    with pytest.raises(ValueError) as ei:
        m.check_ids()
    assert named in str(ei.value), str(ei.value)
    with pytest.raises(ValueError) as ei:
        m.rank(None, bt(bad), 1e-4, neg_sample_num=n_cand - 1)
    assert named in str(ei.value), str(ei.value)
    assert torch.equal(m.table, clean.table) and torch.equal(m.w, clean.w)
    assert m.rank(None, bt(good), 1e-4, neg_sample_num=n_cand - 1) == clean.rank(None, bt(good), 1e-4, neg_sample_num=n_cand - 1)


def test_verify_names_the_tensor_that_differs_within_a_line():
    L, n_cand = 3, 10
    c, P, b = _g4r_lines(L, n_cand)
    m = _model("GRU4Rec", c, P)
    bt = rc.REF["GRU4Rec"].batch_tuple
    m.rank_async(bt(b), 0.0, neg_sample_num=n_cand - 1, verify=True)          # a batch made of lines passes
    mid = n_cand + n_cand // 2                                                # the middle of the second line
    for field, where in (("user_seq", (mid, 3, 1)), ("user_seq_length", (mid,)), ("target_user", (mid, 2))):
        bad = {k: v.copy() for k, v in b.items()}
        bad[field][where] += 1
        with pytest.raises(ValueError, match=r"\(%s\) is not constant within every line of 10 samples" % field):
            m.rank_async(bt(bad), 0.0, neg_sample_num=n_cand - 1, verify=True)
        y = m.rank_async(bt(bad), 0.0, neg_sample_num=n_cand - 1)[0].clone()  # the default trusts the loader: the line's first history
        y0 = m.rank_async(bt(b), 0.0, neg_sample_num=n_cand - 1, verify=False)[0]
        assert float((y - y0).abs().max()) < Y_TOL     # (a longer length in mid-line may add a computed slice: not bit for bit)
    both = {k: v.copy() for k, v in b.items()}
    both["user_seq"][mid, 0, 0] += 1
    both["target_user"][mid, 0] += 1
    with pytest.raises(ValueError, match=r"batch_data\[0\] \(user_seq\)"):    # the first offending tensor
        m.rank_async(bt(both), 0.0, neg_sample_num=n_cand - 1, verify=True)
    with pytest.raises(ValueError, match="not made of lines"):
        m.rank_async(bt(b), 0.0, neg_sample_num=n_cand)


def test_c_abi_refusals_on_the_device():
    """a workspace one byte short is refused before any launch; so are null pointers"""
    import ctypes as C
    from score_amd import _lib
    from score_amd.model import _ptr
    L, n_cand = 3, 10
    c, P, b = _g4r_lines(L, n_cand)
    m = _model("GRU4Rec", c, P)
    db = m.device_batch(rc.REF["GRU4Rec"].batch_tuple(b))
    ws, y, loss = m._rank_buffers(L, n_cand)
    y.fill_(-7.0)
    t = db.tensors
    first = lambda x: x.view(L, n_cand, -1)[:, 0].contiguous()
    useq, ln, tu = first(t[0]), first(t[7]), first(t[4])
    st = m._state(ws)
    call = lambda rb, yy=y: m.lib.score_rank_forward(C.byref(m.cfg), C.byref(st), C.byref(rb), 0.0, _ptr(yy), _ptr(loss), m._stream())
    rb = _lib.RankBatch(_ptr(useq), _ptr(ln), _ptr(tu), _ptr(t[5]), _ptr(t[6]), L, n_cand, 0)
    st.workspace_bytes = _lib.rank_workspace_bytes(m.cfg, L, n_cand) - 1
    assert call(rb) == -3                                   # SCORE_E_WORKSPACE
    st.workspace_bytes = ws.numel() * 4
    assert call(_lib.RankBatch(_ptr(useq), _ptr(ln), _ptr(tu), None, _ptr(t[6]), L, n_cand, 0)) == -1
    assert call(rb, None) == -1
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())                          # nothing ran
    assert call(rb) == 0
    want = rc.restated("GRU4Rec", c, P, b, L, n_cand, 0.0)
    _hold("ctypes call", y.cpu().numpy(), float(loss[0].item()), *want)


# ---- end to end: the bundled Tmall sample's validation lines through the device loader -------------------------------------
def _tmall_validation(kind, seed):
    from score_amd import dataprep as dp
    from score_amd import model as M
    from score_amd.pointdata import DeviceDataLoaderUserSeq
    log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
    stores, r = dp.tmall_point_stores(log, dual=False, batch_size=1000)
    st = stores["validation"]
    T, neg = 50, 99
    m = M.MODELS[kind](r["feature_size"], 16, 32, T, 3, 4, seed=seed)
    return m, list(DeviceDataLoaderUserSeq(1000, T, None, None, neg, None, None, model=m, store=st)), neg


def close_pairs(scores, labels, thr):
    """positive-negative pairs over the WHOLE evaluation whose scores differ by less than thr, and n_pos * n_neg"""
    s, lab = np.asarray(scores, dtype=np.float64), np.asarray(labels).astype(bool)
    neg = np.sort(s[~lab])
    near = sum(int(np.searchsorted(neg, p + thr, "left") - np.searchsorted(neg, p - thr, "right")) for p in s[lab])
    return near, int(lab.sum()) * int((~lab).sum())


# (model, model seed, training steps before the evaluation).  An untrained model's scores lie close together (their standard
# deviation over the sample is ~0.1, with 99 negatives per line), so most seeds set more than two lines aside: over the seeds
# 1 .. 40 the count is 2 .. 12 for GRU4Rec and 2 .. 10 for Caser.  The seed of an untrained row is the first one, from 1 on, at
# which eval's own scores set aside at most two lines (GRU4Rec 7: lines 5 and 24; Caser 13: two lines).  The trained row is the
# same GRU4Rec after 60 steps on these lines at lr = 1e-2, where every positive is at least 0.38 from every negative and no
# line is set aside.  (Caser after such steps scores every candidate within 1e-20 of 0: no row.)
E2E_CASES = [("GRU4Rec", 7, 0), ("GRU4Rec", 7, 60), ("Caser", 13, 0)]


@pytest.mark.parametrize("kind,seed,train_steps", E2E_CASES)
def test_evaluate_device_with_shared_history_on_the_tmall_sample(kind, seed, train_steps):
    """evaluate_device(shared_history=True) against shared_history=False on the sample's validation lines (44 lines of 1 + 99; at
    batch size 1000 the loader yields the whole batches: 40 lines).  The six ranking metrics are equal IF every line's positive
    is at least 2e-4 from its negatives in eval's own scores; lines that are not are reported and set aside -- at most 2, or the
    test fails.  Log-loss and mean loss are held to the pass's bounds; AUC may move by the share of positive-negative pairs
    that close (each such pair can change order, and a pair that changes order moves AUC by at most 1 / (n_pos * n_neg))."""
    from score_amd import harness as h
    m, batches, neg = _tmall_validation(kind, seed)
    per = neg + 1
    reg = 1e-4
    assert len(batches) == 4 and all(b.B == 1000 for b in batches)
    for k in range(train_steps):
        m.train(None, batches[k % 4], 1e-2, reg)
    off = h.evaluate_device(m, batches, reg, neg_sample_num=neg)
    on = h.evaluate_device(m, batches, reg, neg_sample_num=neg, shared_history=True)
    # the condition, from eval's predictions alone
    ey = torch.cat([m.eval_async(b, reg)[0].clone() for b in batches]).cpu().numpy()
    lab = torch.cat([b.tensors[6] for b in batches]).cpu().numpy()
    ids = torch.cat([b.tensors[5][:, 0] for b in batches])
    n_lines = ey.size // per
    assert (lab.reshape(n_lines, per)[:, 0] == 1).all() and lab.sum() == n_lines
    gaps = rc.line_gaps(ey, n_lines, per)
    failing = np.nonzero(gaps < E2E_GAP)[0]
    print(kind, "lines", n_lines, "lines set aside (gap < %g):" % E2E_GAP, failing.tolist(), "their gaps", gaps[failing].tolist())
    assert failing.size <= E2E_MAX_EXCLUDED
    ry = torch.cat([m.rank_async(b, reg, neg_sample_num=neg)[0].clone() for b in batches]).cpu().numpy()
    assert np.abs(ry.astype(np.float64) - ey).max() < Y_TOL
    if failing.size == 0:
        assert on[2:8] == off[2:8], (on, off)
    else:       # the metrics over the lines that meet the condition
        keep = np.setdiff1d(np.arange(n_lines), failing)
        sel = torch.from_numpy((keep[:, None] * per + np.arange(per)[None, :]).reshape(-1)).cuda()
        dev = lambda y: torch.from_numpy(np.ascontiguousarray(y)).cuda()
        assert h.ranking_quality_device(dev(ry)[sel], ids[sel], neg) == h.ranking_quality_device(dev(ey)[sel], ids[sel], neg)
    print(kind, "shared", on, "per sample", off)
    assert abs(on[0] - off[0]) < LOSS_TOL * max(1.0, abs(off[0]))            # log-loss
    assert abs(on[8] - off[8]) < LOSS_TOL * max(1.0, abs(off[8]))            # mean batch loss
    near, pairs = close_pairs(ey, lab, E2E_GAP)
    print(kind, "positive-negative pairs closer than %g: %d of %d; |dAUC| %.3g" % (E2E_GAP, near, pairs, abs(on[1] - off[1])))
    assert abs(on[1] - off[1]) <= near / pairs


def test_evaluate_device_default_is_the_parents_loop_bit_for_bit():
    """without shared_history evaluate_device is eval_async per batch, as before: its 9-tuple equals that loop's, exactly"""
    from score_amd import harness as h
    c, P, _ = _g4r_lines()
    m = _model("GRU4Rec", c, P)
    neg = 9
    batches = [rc.REF["GRU4Rec"].batch_tuple(rc.line_batch("GRU4Rec", c, 4, neg + 1, 40 + k)) for k in range(2)]
    got = h.evaluate_device(m, batches, 1e-4, neg_sample_num=neg)
    preds, labels, iids, losses = [], [], [], []
    for bd in batches:
        db = m.device_batch(bd)
        pred, label, loss = m.eval_async(db, 1e-4)
        preds.append(pred.clone()); labels.append(label); losses.append(loss.clone())
        iids.append(db.tensors[5][:, 0])
    preds, labels, iids = torch.cat(preds), torch.cat(labels), torch.cat(iids)
    auc, logloss = h.auc_logloss_device(preds, labels)
    want = (logloss, auc) + h.ranking_quality_device(preds, iids, neg) + (float(torch.stack(losses).mean().item()),)
    assert got == want
    assert h.evaluate_device(m, batches, 1e-4, neg, False) == want
