#!/usr/bin/env python
"""Time of CCMR's data path from its raw rating log: dataprep.remap_ccmr_log on the host (numpy) against build="device"
(csrc/ccmr.hip and the two compactions) -- the uploads and the rows' download included -- and against the kernels alone (columns
already uploaded, nothing downloaded but the compactions' counts).  Then the negative lists plus ONE target build (prediction
time 40, 99 negatives) under the cell rule: targets.UserNegLists.from_events and gen_target_lines on the host against
score_neg_lists_build and score_target_build_lists on columns that are already on the device.

One JSON line (appended to --out, default profiles/ccmr_prep_time.jsonl): after one warm-up of every kind, `--pairs` rounds,
each taking the kinds in alternating order (the next round with host and device exchanged), every kind bracketed by
torch.cuda.synchronize(); medians and the spread (min, max) of the rounds in milliseconds.

The log: --events events (3.0 M) over 20 k users / 40 k items, about a fifth of them rated 1 .. 3, dates from 150 days before
the start to the end of slice 40 (a third of them in slices 37 .. 40, so the prediction slices are filled); one movie_info line
per item and a second one for every eighth item.

  python tools/ccmr_prep_time.py [--pairs 3] [--events 3000000] [--out FILE]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U, I, VOCAB = 20000, 40000, (8000, 20000, 63, 1044)


def synth(events):
    """-> (log int64 [n, 4], movie_info int64 [m, 5])"""
    rng = np.random.default_rng(7)
    n = int(events)
    day = rng.integers(-150, 41 * 90, n)
    day[:n // 3] = rng.integers(37 * 90, 41 * 90, n // 3)
    first = datetime.date(2005, 5, 19)
    table = np.asarray([int((first + datetime.timedelta(days=d)).strftime("%Y%m%d")) for d in range(-150, 41 * 90)], dtype=np.int64)
    rating = np.where(rng.random(n) < 0.2, rng.integers(1, 4, n), rng.integers(4, 6, n))
    log = np.stack([rng.integers(0, U, n), rng.integers(0, I, n), rating, table[day + 150]], axis=1)
    log = log[rng.permutation(n)]
    items = np.concatenate([rng.permutation(I), np.arange(0, I, 8)])
    feat = np.stack([np.where(rng.random(len(items)) < 0.1, -1, rng.integers(0, v - 1, len(items))) for v in VOCAB], axis=1)
    return np.ascontiguousarray(log), np.ascontiguousarray(np.concatenate([items[:, None], feat], axis=1))


def measure(log, movie, pairs):
    import torch
    from score_amd import dataprep as dp
    from score_amd import logremap as lr
    from score_amd.targets import TargetStore, UserNegLists
    keep = {}
    c = dp.CCMR
    start_day = dp._ordinal(c["start_date"])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def host():
        keep["host"] = dp.remap_ccmr_log(log, movie, U, I, VOCAB)

    def device():
        keep["device"] = dp.remap_ccmr_log(log, movie, U, I, VOCAB, build="device")

    dev = lr.device_of()
    raw, _ = lr.upload_columns(log, 4, dev)
    mv, _ = lr.upload_columns(movie, 5, dev)

    def kernels():
        cols, flat = lr.ccmr_prep(raw, mv, U, I, VOCAB, start_day, c["delta_days"])
        keep["kernels"] = (lr.log_compact(cols[:4], cols[4]), lr.log_compact(cols[:2], cols[5]), flat)

    host()
    device()
    h, d = keep["host"], keep["device"]
    pt, neg = c["pred_time_test"], c["test_neg"]

    def host_targets():
        nl = UserNegLists.from_events(h["neg_uid"], h["neg_iid"], U)
        keep["host_targets"] = TargetStore.from_log(h["uid"], h["iid"], h["t_idx"], U, I, pt, neg, c["start_time"], 11, build="host",
                                                    neg_lists=nl)

    def device_targets():
        nl = UserNegLists.from_events(d["neg_uid"], d["neg_iid"], U, build="device")
        keep["device_targets"] = TargetStore.from_log(d["uid"], d["iid"], d["t_idx"], U, I, pt, neg, c["start_time"], 11,
                                                      build="device", neg_lists=nl)

    kinds = [("host_ms", host), ("device_ms", device), ("kernels_ms", kernels), ("host_lists_targets_ms", host_targets),
             ("device_lists_targets_ms", device_targets)]
    for _, fn in kinds:                                  # warm-up: the library, the kernels' code objects, the allocator
        fn()
    times = {k: [] for k, _ in kinds}
    for r in range(pairs):
        order = kinds if r % 2 == 0 else [kinds[1], kinds[0], kinds[2], kinds[4], kinds[3]]
        for k, fn in order:
            times[k].append(timed(fn))
    h, d = keep["host"], keep["device"]
    same = all(np.array_equal(d[k].cpu().numpy(), h[k]) for k in ("uid", "iid", "t_idx", "time_key", "neg_uid", "neg_iid")) and \
        np.array_equal(d["item_rows"], h["item_rows"])
    same_lines = all(np.array_equal(a, b) for a, b in zip(keep["host_targets"].arrays(), keep["device_targets"].arrays()))
    line = dict(what="ccmr_prep_time", events=int(len(log)), negative_events=int(len(h["neg"])), movie_lines=int(len(movie)), users=U,
                items=I, feature_size=int(h["feature_size"]), target_lines=int(keep["host_targets"].n_lines), pairs=pairs,
                device=torch.cuda.get_device_name(), device_equals_host=bool(same), targets_equal=bool(same_lines))
    for k, v in times.items():
        line[k] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--events", type=int, default=3000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ccmr_prep_time.jsonl"))
    a = ap.parse_args()
    log, movie = synth(a.events)
    line = json.dumps(measure(log, movie, a.pairs))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
