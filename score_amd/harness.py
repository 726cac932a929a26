"""Host-side harness around the hot path: the evaluation loop and ranking metrics the reference's
driver wraps around model.eval (code/score/train_score.py:94-163).  Pure NumPy/Python, no TF."""
import math
import time

import numpy as np

TEST_NEG_SAMPLE_NUM = 99          # train_score.py:19: one positive + 99 negatives per target line


def getNDCG_at_K(ranklist, target_item, k):
    """log 2 / log(rank + 2) if the positive is ranked in the top k, else 0 (train_score.py:104-108)."""
    for i in range(min(k, len(ranklist))):
        if ranklist[i] == target_item:
            return math.log(2) / math.log(i + 2)
    return 0


def getHR_at_K(ranklist, target_item, k):
    return 1 if target_item in ranklist[:k] else 0


def getMRR(ranklist, target_item):
    for i, it in enumerate(ranklist):
        if it == target_item:
            return 1. / (i + 1)
    return 0


def _ranked(preds, target_iids, per_line):
    p = np.asarray(preds, dtype=np.float64).reshape(-1, per_line)
    ids = np.asarray(target_iids).reshape(-1, per_line)
    # descending score.  The reference calls np.argsort with its default kind, whose order among EQUAL scores
    # depends on NumPy's build (introsort / SIMD sort); a stable sort pins it (equal scores: larger index
    # first after the reversal) -- the rule score_ranking_quality implements on the device
    order = np.argsort(p, axis=1, kind="stable")[:, ::-1]
    ranked = np.take_along_axis(ids, order, axis=1)
    # 0-based rank of the first entry equal to the positive's id (column 0 of every line)
    hit = ranked == ids[:, :1]
    return hit.argmax(axis=1)


def get_ranking_quality(preds, target_iids, neg_sample_num=TEST_NEG_SAMPLE_NUM):
    """(NDCG@5, NDCG@10, HR@1, HR@5, HR@10, MRR) over lines of 1 + neg_sample_num candidates
    (train_score.py:122-142)."""
    r = _ranked(preds, target_iids, neg_sample_num + 1).astype(np.float64)
    gain = math.log(2) / np.log(r + 2)
    return (float(np.mean(np.where(r < 5, gain, 0.0))), float(np.mean(np.where(r < 10, gain, 0.0))),
            float(np.mean(r < 1)), float(np.mean(r < 5)), float(np.mean(r < 10)), float(np.mean(1.0 / (r + 1))))


def get_ndcg(preds, target_iids, neg_sample_num=TEST_NEG_SAMPLE_NUM):
    return get_ranking_quality(preds, target_iids, neg_sample_num)[0]


def evaluate(model, batches, reg_lambda, sess=None, neg_sample_num=TEST_NEG_SAMPLE_NUM, verbose=False):
    """train_score.py:144-163: run model.eval over the batches of a target file and return
    (logloss, auc, ndcg_5, ndcg_10, hr_1, hr_5, hr_10, mrr, mean batch loss)."""
    from sklearn.metrics import log_loss, roc_auc_score
    preds, labels, target_iids, losses = [], [], [], []
    t = time.time()
    for batch_data in batches:
        pred, label, loss = model.eval(sess, batch_data, reg_lambda)
        preds += pred
        labels += label
        losses.append(loss)
        # the target item ids: batch_data[5] of the slice models' 8-tuple (train_score.py:152), batch_data[3] of a point model's
        # 5-tuple (train_time_point_models.py:146) -- the model says which; a DeviceBatch holds them as its tensor 5
        ids = batch_data.tensors[5] if hasattr(batch_data, "tensors") else batch_data[getattr(model, "target_item_field", 5)]
        if hasattr(ids, "cpu"):                   # device batches (DeviceGraphLoader) hand tensors over
            ids = ids.cpu().numpy()
        target_iids += np.array(ids)[:, 0].tolist()
    logloss = log_loss(labels, preds)
    auc = roc_auc_score(labels, preds)
    loss = sum(losses) / len(losses)
    ndcg_5, ndcg_10, hr_1, hr_5, hr_10, mrr = get_ranking_quality(preds, target_iids, neg_sample_num)
    if verbose:
        print("EVAL TIME: %.4fs" % (time.time() - t))
    return logloss, auc, ndcg_5, ndcg_10, hr_1, hr_5, hr_10, mrr, loss


TRAIN_NEG_SAMPLE_NUM = 1          # train_score.py:18


def train_loop(model, train_batches, vali_batches, lr, reg_lambda, train_batch_size, dataset_size, sess=None,
               epochs=6, save_path=None, evaluate_fn=None, neg_sample_num=TEST_NEG_SAMPLE_NUM, log=print, feed_ahead=True):
    """The training loop train_score.py:165-275 wraps around model.train / model.eval, rule for rule:

      * one evaluation before the first step (:205);
      * ``eval_iter_num = (dataset_size // 3) // (train_batch_size / (1 + TRAIN_NEG_SAMPLE_NUM))`` (:217, a float
        floor: three validation passes per epoch) -- every eval_iter_num-th step the mean training loss since the
        last evaluation is recorded and the validation set is evaluated (:230-245);
      * the model is saved whenever the new validation MRR beats every earlier one (:246-252);
      * early stop, only after the first epoch and with more than two evaluations (:254-258): MRR fell twice in
        a row, or improved by <= 0.001 twice in a row;
      * at most ``epochs`` (6, :219) passes over the training targets, a fresh loader per epoch (:222).

    ``train_batches`` / ``vali_batches``: zero-argument callables returning a fresh iterable of batches (the
    reference constructs a new GraphLoader each time).  ``evaluate_fn(model, batches, reg_lambda)`` defaults to
    evaluate_device when the model has eval_async, else evaluate.  Returns a dict with the curves the reference
    pickles (:264-266), the index of the best validation MRR and ``best_mrr`` (its return value, :275)."""
    if evaluate_fn is None:
        if hasattr(model, "eval_async"):
            evaluate_fn = lambda m, b, r: evaluate_device(m, b, r, neg_sample_num)
        else:
            evaluate_fn = lambda m, b, r: evaluate(m, b, r, sess, neg_sample_num)
    curves = dict(train_losses=[], vali_losses=[], vali_ndcgs_5=[], vali_ndcgs_10=[], vali_hrs_1=[], vali_hrs_5=[],
                  vali_hrs_10=[], vali_mrrs=[])

    # A model sharded over several ranks (score_amd.dist.ShardedSCORE): every train / eval call is a collective, so all
    # ranks must take the same branches.  The validation metrics every rule below looks at are therefore the MEAN over
    # the ranks (each rank evaluates its own validation shard), and an epoch ends for everybody as soon as any rank's
    # loader runs out (ranks may hold different numbers of batches); checkpoints are then all from the same step.
    comm = getattr(model, "comm", None)
    multi = comm is not None and getattr(comm, "world", 1) > 1

    def across_ranks(values, op="mean"):
        if not multi:
            return list(values)
        import torch
        dev = getattr(model, "device", "cpu")
        t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=dev)
        comm.all_reduce_sum(t)
        out = t.cpu().tolist()
        return [v / comm.world for v in out] if op == "mean" else out

    def validate():
        _, _, n5, n10, h1, h5, h10, mrr, loss = evaluate_fn(model, vali_batches(), reg_lambda)
        n5, n10, h1, h5, h10, mrr, loss = across_ranks((n5, n10, h1, h5, h10, mrr, loss))
        for k, v in (("vali_ndcgs_5", n5), ("vali_ndcgs_10", n10), ("vali_hrs_1", h1), ("vali_hrs_5", h5),
                     ("vali_hrs_10", h10), ("vali_mrrs", mrr), ("vali_losses", loss)):
            curves[k].append(v)
        return n5, n10, h1, h5, h10, mrr, loss

    step, saves = 0, []
    n5, n10, h1, h5, h10, mrr, vloss = validate()
    log("STEP %d  LOSS TRAIN: NULL  LOSS VALI: %.4f  NDCG@5 VALI: %.4f  NDCG@10 VALI: %.4f  HR@1 VALI: %.4f  "
        "HR@5 VALI: %.4f  HR@10 VALI: %.4f  MRR VALI: %.4f" % (step, vloss, n5, n10, h1, h5, h10, mrr))
    early_stop = False
    eval_iter_num = (dataset_size // 3) // (train_batch_size / (1 + TRAIN_NEG_SAMPLE_NUM))
    if eval_iter_num < 1:
        raise ValueError("dataset_size %d too small for batch size %d: eval_iter_num = %r" %
                         (dataset_size, train_batch_size, eval_iter_num))
    losses_step = []
    vali_mrrs = curves["vali_mrrs"]
    # a model whose train() takes next_batch= (the row-sharded ShardedSCORE) is fed one batch ahead: its index plan and
    # row requests for batch t+1 then run under step t instead of on its critical path (two host read-backs per step)
    import inspect
    try:
        ahead = "next_batch" in inspect.signature(model.train).parameters
    except (TypeError, ValueError):
        ahead = False

    use_async = not ahead and hasattr(model, "train_async") and hasattr(model, "device")
    # ... and the single-device model's train_async takes the upcoming batch as a hint (SCOREBASE.apply_adam(next_batch=): with
    # the time-tiled table optimizer its rows are brought up to date beside this step's tail instead of in front of the next
    # forward pass).  Only device-resident batches qualify -- what model.feed() yields
    try:
        async_hint = use_async and "next_batch" in inspect.signature(model.train_async).parameters
    except (TypeError, ValueError):
        async_hint = False

    def with_next(it):
        it = iter(it)
        try:
            cur = next(it)
        except StopIteration:
            return
        for nxt in it:
            yield cur, nxt
            cur = nxt
        yield cur, None

    def steps_agreed(source):
        """several ranks, once per EPOCH: if every rank's loader has a length, the ranks agree on min(length) with one small
        all-reduce (each rank writes its length into its own slot) and the epoch then needs no per-step agreement -- an
        all-reduce plus a host read-back ahead of every step drains the stream each time, and the host could no longer run
        ahead of the GPU (which is what train_async, feed() and next_batch= are for).  None: some loader has no length"""
        if not multi:
            return None
        n = len(source) if hasattr(source, "__len__") else -1
        slots = [0.0] * (2 * comm.world)
        slots[comm.rank] = 1.0 if n >= 0 else 0.0
        slots[comm.world + comm.rank] = float(max(n, 0))
        got = across_ranks(slots, op="sum")
        if sum(got[:comm.world]) < comm.world:
            return None
        return int(min(got[comm.world:]))

    def in_step(pairs, n_steps=None):
        """several ranks: stop together.  n_steps (steps_agreed): exactly that many steps, the look-ahead batch of the last
        one dropped, no collective.  Otherwise a step is taken only if EVERY rank still has a batch for it (one small
        all-reduce per step, ahead of the step's own collectives); the look-ahead batch is dropped when some rank has
        none, so nobody prefetches for a step that will not happen"""
        if not multi:
            for p in pairs:
                yield p
            return
        it = iter(pairs)
        if n_steps is not None:
            for i in range(n_steps):
                p = next(it, None)
                if p is None:        # a loader whose __len__ overstates what it yields: say so here, on this rank, instead of
                    raise RuntimeError("train_loop: the loader of rank %d ended after %d of the %d batches its len() promised "
                                       "(the other ranks are inside that step's collectives: they time out)" % (comm.rank, i, n_steps))
                yield (p[0], p[1] if i + 1 < n_steps else None)
            return
        while True:
            p = next(it, None)
            have = across_ranks((0.0 if p is None else 1.0, 0.0 if (p is None or p[1] is None) else 1.0), op="sum")
            if have[0] < comm.world:
                return
            yield (p[0], p[1] if have[1] == comm.world else None)
    for epoch in range(epochs):
        if early_stop:
            break
        # host feed tuples (nested lists, as GraphLoader yields them) are converted and uploaded a batch or two ahead on a
        # worker thread (SCOREBASE.feed), under the step that is running
        source = train_batches()
        n_agreed = steps_agreed(source)
        if hasattr(model, "feed") and feed_ahead:
            source = model.feed(source)
        for batch_data, next_data in in_step(with_next(source), n_agreed):
            if early_stop:
                break
            if ahead:
                loss = model.train(sess, batch_data, lr, reg_lambda, next_batch=next_data)
            elif use_async:
                # the loss stays on the device until the next evaluation needs the mean: the host does not wait for the
                # GPU every step, so preparing batch t+1 (list flattening, loader work) overlaps step t
                if async_hint and next_data is not None and hasattr(next_data, "flat"):
                    loss = model.train_async(batch_data, lr, reg_lambda, next_batch=next_data).clone()
                else:
                    loss = model.train_async(batch_data, lr, reg_lambda).clone()
            else:
                loss = model.train(sess, batch_data, lr, reg_lambda)
            step += 1
            losses_step.append(loss)
            if step % eval_iter_num == 0:
                if use_async:
                    import torch
                    losses_step = torch.stack(losses_step).cpu().tolist()
                    if any(v != v for v in losses_step) and hasattr(model, "check_ids"):
                        model.check_ids()       # a NaN loss is how an out-of-range feature id shows (SCOREBASE.check_ids)
                train_loss = sum(losses_step) / len(losses_step)
                curves["train_losses"].append(train_loss)
                losses_step = []
                n5, n10, h1, h5, h10, mrr, vloss = validate()
                log("STEP %d  LOSS TRAIN: %.4f  LOSS VALI: %.4f  NDCG@5 VALI: %.4f  NDCG@10 VALI: %.4f  HR@1 VALI: %.4f  "
                    "HR@5 VALI: %.4f  HR@10 VALI: %.4f  MRR VALI: %.4f" % (step, train_loss, vloss, n5, n10, h1, h5, h10, mrr))
                if vali_mrrs[-1] > max(vali_mrrs[:-1]):
                    saves.append(step)
                    if save_path is not None:
                        model.save(sess, save_path)
                if len(vali_mrrs) > 2 and epoch > 0:
                    if vali_mrrs[-1] < vali_mrrs[-2] and vali_mrrs[-2] < vali_mrrs[-3]:
                        early_stop = True
                    if (vali_mrrs[-1] - vali_mrrs[-2]) <= 0.001 and (vali_mrrs[-2] - vali_mrrs[-3]) <= 0.001:
                        early_stop = True
        # the tail of an epoch after its last evaluation was never looked at: a batch with an id outside the table there would
        # leave the sticky status word set and every later optimizer step suppressed without anybody hearing of it
        if use_async and hasattr(model, "check_ids"):
            model.check_ids()
    if hasattr(model, "check_ids"):
        model.check_ids()
    index = int(np.argmax(vali_mrrs))
    curves.update(best_index=index, best_mrr=vali_mrrs[index], steps=step, saved_at_steps=saves,
                  eval_iter_num=eval_iter_num, early_stopped=early_stop)
    return curves


def ranking_quality_device(preds, target_iids, neg_sample_num=TEST_NEG_SAMPLE_NUM, return_ranks=False):
    """get_ranking_quality on the device (score_ranking_quality, include/score_hip.h): preds float32 and
    target_iids int32 device tensors of n_lines * (1 + neg_sample_num) entries.  One 6-float read-back."""
    import ctypes as C
    import torch
    from . import _lib
    lib = _lib.load()
    per = neg_sample_num + 1
    preds = preds.reshape(-1).contiguous().float()
    ids = target_iids.reshape(-1).contiguous().to(torch.int32)
    n_lines = preds.numel() // per
    if n_lines * per != preds.numel() or ids.numel() != preds.numel():
        raise ValueError("preds / target_iids must hold n_lines * (1 + neg_sample_num) entries")
    out = torch.empty((6,), dtype=torch.float32, device=preds.device)
    ranks = torch.empty((n_lines,), dtype=torch.int32, device=preds.device)
    scratch = torch.empty((6 * n_lines,), dtype=torch.float32, device=preds.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.score_ranking_quality(p(preds), p(ids), n_lines, per, p(out), p(ranks), p(scratch), scratch.numel(),
                                         C.c_void_p(torch.cuda.current_stream(preds.device).cuda_stream)),
               "score_ranking_quality")
    res = tuple(float(x) for x in out.cpu().tolist())
    return (res, ranks) if return_ranks else res


def auc_logloss_device(preds, labels):
    """(roc_auc_score, log_loss) of device tensors preds float32 [n], labels int32 [n] (score_auc_logloss)."""
    import ctypes as C
    import torch
    from . import _lib
    lib = _lib.load()
    preds = preds.reshape(-1).contiguous().float()
    labels = labels.reshape(-1).contiguous().to(torch.int32)
    n = preds.numel()
    if labels.numel() != n or n == 0:
        raise ValueError("preds and labels must be non-empty and of equal length")
    out = torch.empty((2,), dtype=torch.float64, device=preds.device)
    scratch = torch.empty((int(lib.score_auc_scratch_bytes(n)),), dtype=torch.uint8, device=preds.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.score_auc_logloss(p(preds), p(labels), n, p(out), p(scratch), scratch.numel(),
                                     C.c_void_p(torch.cuda.current_stream(preds.device).cuda_stream)),
               "score_auc_logloss")
    auc, ll = out.cpu().tolist()
    return auc, ll


def evaluate_device(model, batches, reg_lambda, neg_sample_num=TEST_NEG_SAMPLE_NUM, shared_history=False):
    """evaluate() with predictions, ids and labels kept on the device: one forward per batch
    (model.eval_async), ranking metrics by score_ranking_quality, AUC / log-loss by score_auc_logloss; two
    small read-backs at the end.  Returns the same 9-tuple as evaluate().

    shared_history=True (GRU4Rec, Caser): every batch goes through model.rank_async instead -- the history of a target line's
    1 + neg_sample_num samples is encoded once, not once per candidate (the loaders write the same history for all of them).
    Predictions differ from eval_async's by the order of fc1's sum only; everything else here is unchanged."""
    import torch
    preds, labels, iids, losses = [], [], [], []
    for batch_data in batches:
        db = model.device_batch(batch_data)
        if shared_history:
            pred, label, loss = model.rank_async(db, reg_lambda, neg_sample_num=neg_sample_num)
        else:
            pred, label, loss = model.eval_async(db, reg_lambda)
        preds.append(pred.clone()); labels.append(label); losses.append(loss.clone())
        iids.append(db.tensors[5][:, 0])
    preds, labels, iids = torch.cat(preds), torch.cat(labels), torch.cat(iids)
    ndcg_5, ndcg_10, hr_1, hr_5, hr_10, mrr = ranking_quality_device(preds, iids, neg_sample_num)
    auc, logloss = auc_logloss_device(preds, labels)
    loss = float(torch.stack(losses).mean().item())
    if loss != loss and hasattr(model, "check_ids"):
        model.check_ids()       # (a NaN loss is how an id outside the table shows: raised HERE, not blamed on the next train step)
    return (logloss, auc, ndcg_5, ndcg_10, hr_1, hr_5, hr_10, mrr, loss)


def catalog_quality_device(top_idx, target_idx):
    """The six numbers of get_ranking_quality, in its order -- (NDCG@5, NDCG@10, HR@1, HR@5, HR@10, MRR) -- from top-k lists over a
    whole catalogue (model.recommend_async): top_idx [n_lines, k] catalogue indices, best first, target_idx [n_lines] the
    positive's index.  The positive's rank is its position in the list; a positive that is not in the list counts 0 everywhere,
    so MRR is truncated at k.  Needs k >= 10.  Tensors on any device; one 6-float read-back.  (rank_quality_device takes exact
    ranks from model.item_ranks_async instead: no truncation.)"""
    import torch
    top = top_idx.reshape(top_idx.shape[0], -1)
    n, k = top.shape
    if k < 10:
        raise ValueError("catalog_quality_device needs lists of k >= 10 items, got k = %d" % k)
    tgt = target_idx.reshape(-1).to(device=top.device, dtype=top.dtype)
    if tgt.numel() != n or n == 0:
        raise ValueError("top_idx [n_lines, k] and target_idx [n_lines] must name the same, non-zero number of lines")
    hit = top == tgt[:, None]
    found = hit.any(1)
    r = hit.to(torch.int32).argmax(1).to(torch.float64)              # 0-based rank of the first hit (0 where there is none)
    gain = math.log(2) / torch.log(r + 2)
    zero = torch.zeros_like(gain)
    f = lambda cond: (found & cond).to(torch.float64).mean()
    out = torch.stack([torch.where(found & (r < 5), gain, zero).mean(), torch.where(found & (r < 10), gain, zero).mean(),
                       f(r < 1), f(r < 5), f(r < 10), torch.where(found, 1.0 / (r + 1), zero).mean()])
    return tuple(float(x) for x in out.cpu().tolist())


# ---- the four evaluate_catalog* functions: two line sources (_loader_lines, _store_lines) times two measures (the k best through
# recommend*_async and catalog_quality_device; the exact rank through item_ranks*_async and rank_quality_device)
def _check_candidates(name, candidates):
    if candidates is not None and candidates != "line":
        raise ValueError("%s: candidates must be None or \"line\", got %r" % (name, candidates))


def _loader_lines(name, model, batches, catalog, neg_sample_num, exclude_history, candidates):
    """The target lines of a loader's eval batches (lines of 1 + neg_sample_num samples, the first candidate the positive), per
    batch: (lines, active_slices, L, the positives' item ids, their catalogue indices, exclude: with exclude_history the users'
    histories without the positive, own: with candidates="line" each line's own items).  ValueError, per batch, for a positive
    the catalogue does not hold."""
    import torch
    n_cand = 1 + neg_sample_num
    for batch_data in batches:
        db = model.device_batch(batch_data)
        lines = model.lines_of(db, neg_sample_num)
        L = int(lines[1].numel())
        pos_ids = db.tensors[5].view(L, n_cand, -1)[:, 0, 0].contiguous()
        tgt, found = catalog.indices_of(pos_ids)
        if not bool(found.all().item()):
            raise ValueError("%s: a line's positive item is not in the catalogue" % name)
        exclude = None
        if exclude_history is not None:
            exclude = _history_exclusions(exclude_history, lines[2][:, 0], pos_ids)
        own = None
        if candidates == "line":
            own = (torch.arange(L + 1, device=pos_ids.device, dtype=torch.int64) * n_cand,
                   db.tensors[5].view(L, n_cand, -1)[:, :, 0].reshape(-1))
        yield lines, db.active_slices, L, pos_ids, tgt, exclude, own


def _store_lines(name, model, store, catalog, candidates, lines_per_call):
    """A PointLogStore's own target lines, straight from the store's tensors (no expanded batch, no strided copies, nothing read
    back), lines_per_call at a time: (the lines' users, L, the positives' item ids -- the first of each line's line_items --,
    their catalogue indices, which of them the catalogue holds, own: with candidates="line" each line's own items,
    max_candidates for them)"""
    import torch
    if getattr(model, "rank_unsupported", None) is not None:
        raise NotImplementedError("%s has no catalogue pass: %s" % (type(model).__name__, model.rank_unsupported))
    if store._dev is None:
        raise ValueError("%s: the store must be on a device (build='device' or .to_device())" % name)
    n_lines, per_line, step = int(store.n_lines), int(store.per_line), int(lines_per_call)
    if n_lines <= 0 or step <= 0:
        raise ValueError("%s: no target lines, or lines_per_call <= 0" % name)
    users = store._dev["line_user"][:n_lines]
    items = store._dev["line_items"][:n_lines * per_line].view(n_lines, per_line)
    for a in range(0, n_lines, step):
        b = min(n_lines, a + step)
        L = b - a
        pos_ids = items[a:b, 0].contiguous()
        tgt, found = catalog.indices_of(pos_ids)
        own, longest = None, None
        if candidates == "line":
            own = (torch.arange(L + 1, device=pos_ids.device, dtype=torch.int64) * per_line, items[a:b].reshape(-1))
            longest = per_line
        yield users[a:b], L, pos_ids, tgt, found, own, longest


def _catalog_measure(name, model, founds, measure, *lists):
    """The end of the four: each list of per-call tensors concatenated, measure(*them), check_ids -> (the numbers, the tensors).
    founds (the store forms): one flag a call, read back here, once; ValueError unless all are set"""
    import torch
    if founds is not None and not bool(torch.stack(founds).all().item()):
        raise ValueError("%s: a line's positive item is not in the catalogue" % name)
    whole = [torch.cat(x) for x in lists]
    numbers = measure(*whole)
    if hasattr(model, "check_ids"):
        model.check_ids()
    return numbers, whole


def evaluate_catalog(model, batches, catalog, neg_sample_num=TEST_NEG_SAMPLE_NUM, k=10, exclude_history=None, return_lists=False,
                     candidates=None):
    """Ranking metrics against the WHOLE catalogue instead of the sampled negatives: for every target line of a loader's eval
    batches (lines of 1 + neg_sample_num samples, the first candidate the positive) the model's k best items of `catalog`
    (model.recommend_async), then catalog_quality_device on the positive's position -> its six numbers.

    exclude_history: a PointLogStore -- the items of each user's history are excluded from the user's list, the positive
    itself never.  return_lists: also the lists and the positives' catalogue indices, (six, top_idx [n_lines, k], target_idx).

    candidates="line": every line is restricted to its own 1 + neg_sample_num items -- the reference's sampled protocol on the
    catalogue route (repeated negatives collapse; negatives the catalogue does not hold drop out; the positive is always in the
    list).  None: the whole catalogue.  Anything else raises ValueError."""
    import torch
    _check_candidates("evaluate_catalog", candidates)
    tops, tgts = [], []
    for lines, active, L, pos_ids, tgt, exclude, own in _loader_lines("evaluate_catalog", model, batches, catalog, neg_sample_num,
                                                                      exclude_history, candidates):
        top = model.recommend_async(lines, catalog, k=k, exclude=exclude, active_slices=active, candidates=own)[0]
        tops.append(top.clone()); tgts.append(tgt.to(torch.int32))
    six, (top, tgt) = _catalog_measure("evaluate_catalog", model, None, catalog_quality_device, tops, tgts)
    return (six, top, tgt) if return_lists else six


def evaluate_catalog_users(model, store, catalog, k=10, exclude_history=True, candidates=None, lines_per_call=100,
                           return_lists=False):
    """evaluate_catalog over a PointLogStore's own target lines without a loader: a line's user is line_user, its positive the
    first of its line_items, taken straight from the store's tensors, lines_per_call lines a call of
    model.recommend_users_async -- no expanded batch, no strided copies, no read-back per batch.  exclude_history: each user's
    history in the store is excluded, the positive itself never.  candidates="line": every line is restricted to its own
    1 + neg_sample_num items.  Returns what evaluate_catalog(loader batches of the same store, catalog, exclude_history=store or
    None, ...) returns: the six numbers, with return_lists also (top_idx [n_lines, k], target_idx [n_lines])."""
    import torch
    _check_candidates("evaluate_catalog_users", candidates)
    tops, tgts, founds = [], [], []
    for users, L, pos_ids, tgt, found, own, longest in _store_lines("evaluate_catalog_users", model, store, catalog, candidates,
                                                                    lines_per_call):
        top = model.recommend_users_async(users, store, catalog, k=k, exclude_history=bool(exclude_history), keep=pos_ids,
                                          candidates=own, max_candidates=longest)[0]
        tops.append(top.clone()); tgts.append(tgt.to(torch.int32)); founds.append(found.all())
    six, (top, tgt) = _catalog_measure("evaluate_catalog_users", model, founds, catalog_quality_device, tops, tgts)
    return (six, top, tgt) if return_lists else six


def rank_quality_device(ahead, state=None):
    """(NDCG@5, NDCG@10, HR@1, HR@5, HR@10, MRR, mean_rank) from exact ranks (model.item_ranks_async): ahead [n] the number of
    items in front of each target, i.e. its 0-based rank r.  catalog_quality_device's formulas on r = ahead -- gain
    log 2 / log(r + 2) under the cutoff, 1 / (r + 1) for MRR, which is NOT truncated here -- and mean_rank, the mean of r + 1
    over the targets that count.  A target with ahead < 0 (not in the catalogue) counts 0 in the six and not in mean_rank, as a
    miss does there; with `state` given so does one with state <= 0 (not among the line's scored items).  An excluded target
    (state 2) counts with its rank against the rest.  Tensors on any device; one 7-float read-back."""
    import torch
    r = ahead.reshape(-1)
    if r.numel() == 0:
        raise ValueError("rank_quality_device: no targets")
    found = r >= 0
    if state is not None:
        st = state.reshape(-1).to(r.device)
        if st.numel() != r.numel():
            raise ValueError("rank_quality_device: ahead and state must name the same targets")
        found = found & (st > 0)
    r = r.clamp(min=0).to(torch.float64)
    gain = math.log(2) / torch.log(r + 2)
    zero = torch.zeros_like(gain)
    f = lambda cond: (found & cond).to(torch.float64).mean()
    n_found = found.to(torch.float64).sum()
    mean_rank = torch.where(found, r + 1, zero).sum() / n_found.clamp(min=1)
    out = torch.stack([torch.where(found & (r < 5), gain, zero).mean(), torch.where(found & (r < 10), gain, zero).mean(),
                       f(r < 1), f(r < 5), f(r < 10), torch.where(found, 1.0 / (r + 1), zero).mean(), mean_rank])
    return tuple(float(x) for x in out.cpu().tolist())


def evaluate_catalog_ranks(model, batches, catalog, neg_sample_num=TEST_NEG_SAMPLE_NUM, exclude_history=None, candidates=None):
    """evaluate_catalog with the positive's EXACT rank in place of its position in a top-k list: for every target line of a
    loader's eval batches the positive is the single target of model.item_ranks_async, then rank_quality_device -> its seven
    numbers.  The first five equal evaluate_catalog's at any k >= 10; MRR is not truncated.  exclude_history, candidates: as
    evaluate_catalog takes them (the positive itself is never excluded)."""
    import torch
    _check_candidates("evaluate_catalog_ranks", candidates)
    aheads, states = [], []
    for lines, active, L, pos_ids, tgt, exclude, own in _loader_lines("evaluate_catalog_ranks", model, batches, catalog,
                                                                      neg_sample_num, exclude_history, candidates):
        targets = (torch.arange(L + 1, device=pos_ids.device, dtype=torch.int64), tgt.to(torch.int32).contiguous(), 1)
        out = model.item_ranks_async(lines, catalog, targets, exclude=exclude, active_slices=active, candidates=own)
        aheads.append(out[0].clone()); states.append(out[2].clone())
    return _catalog_measure("evaluate_catalog_ranks", model, None, rank_quality_device, aheads, states)[0]


def evaluate_catalog_ranks_users(model, store, catalog, exclude_history=True, candidates=None, lines_per_call=100):
    """evaluate_catalog_ranks over a PointLogStore's own target lines without a loader, the route of evaluate_catalog_users:
    lines_per_call lines a call of model.item_ranks_users_async, the line's positive its single target, no read-back per call.
    The user's whole history is excluded (exclude_history); a positive inside it is ranked against the rest (state 2), which is
    the rank it has in evaluate_catalog_users' lists, where it alone is kept.  -> rank_quality_device's seven numbers."""
    import torch
    _check_candidates("evaluate_catalog_ranks_users", candidates)
    aheads, states, founds = [], [], []
    for users, L, pos_ids, tgt, found, own, longest in _store_lines("evaluate_catalog_ranks_users", model, store, catalog,
                                                                    candidates, lines_per_call):
        targets = (torch.arange(L + 1, device=pos_ids.device, dtype=torch.int64),
                   torch.where(found, tgt, torch.full_like(tgt, -1)).to(torch.int32).contiguous(), 1)      # (-1: not held)
        out = model.item_ranks_users_async(users, store, catalog, targets, exclude_history=bool(exclude_history),
                                           candidates=own, max_candidates=longest)
        aheads.append(out[0].clone()); states.append(out[2].clone()); founds.append(found.all())
    return _catalog_measure("evaluate_catalog_ranks_users", model, founds, rank_quality_device, aheads, states)[0]


def _history_exclusions(store, user_ids, keep_ids):
    """CSR pair (offsets [L + 1], item ids) of the L users' histories in a PointLogStore -- user u's run of user_hist_seq, all of
    it, not only the part a batch reads -- without each line's own keep id.  A user id the store does not know has none."""
    import torch
    dev = user_ids.device
    as_dev = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)
    off, seq = as_dev(store.user_hist_off).to(torch.int64), as_dev(store.user_hist_seq).reshape(-1)
    U = int(off.numel()) - 1
    u = user_ids.to(torch.int64)
    known = (u >= 1) & (u <= U)
    uc = u.clamp(1, U)
    start = off[uc - 1]
    n = torch.where(known, off[uc] - start, torch.zeros_like(start))
    out_off = torch.cat([torch.zeros((1,), dtype=torch.int64, device=dev), torch.cumsum(n, 0)])
    total = int(out_off[-1].item())
    j = torch.arange(total, device=dev, dtype=torch.int64)
    line = torch.searchsorted(out_off, j, right=True) - 1
    items = seq[start[line] + (j - out_off[line])].to(torch.int64)
    items = torch.where(items == keep_ids.to(torch.int64)[line], torch.full_like(items, -1), items)     # (-1: in no catalogue)
    return out_off, items
