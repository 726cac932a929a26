#!/usr/bin/env python
"""Time of the first link of the data path, the remap of a raw Tmall log (ids in order of first appearance, feature rows,
15-day slices): dataprep.remap_tmall_log on the host (numpy and a Python loop over the dates; what every pipeline ran so far)
against build="device" (csrc/logremap.hip) -- the raw upload and the rows' download included -- and against the kernels alone
(columns already uploaded, rows left on the device).  Then tmall_pipeline(build="device", draws="cell", targets="device") end to
end with remap="host" against remap="device".

Per shape one JSON line (appended to --out, default profiles/log_remap_time.jsonl): after one warm-up of every kind, `--pairs`
rounds, each taking the kinds in alternating order (the next round with host and device exchanged), every kind bracketed by
torch.cuda.synchronize(); medians and the spread (min, max) of the rounds in milliseconds.

Shapes: "sample", the bundled Tmall sample log; "synth", a raw log over the seeded Tmall-shaped log of
tools/graph_build_time.py -- --events events (3.0 M) over 20 k users / 40 k items and 14 slices, raw ids scattered over 31 bits,
categories, sellers and brands derived from the item (brand -1 among them), a date inside each event's slice.

  python tools/log_remap_time.py [--shapes sample,synth] [--pairs 3] [--events 3000000] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def raw_shape(name, events):
    """-> (name, raw log int64 [n, 6])"""
    if name == "sample":
        return name, np.load(os.path.join(ROOT, "tests", "golden", "tmall_sample_log.npz"))["log"]
    import graph_build_time as gbt
    sh = gbt.synth_shape(events)
    rng = np.random.default_rng(7)
    uid, iid, t = sh["uid"].astype(np.int64), sh["iid"].astype(np.int64), sh["t"].astype(np.int64)
    day = t * 15 + rng.integers(0, 15, len(t))                       # days since 2015-05-01, inside the event's slice
    first = datetime.date(2015, 5, 1)
    mmdd = np.asarray([(first + datetime.timedelta(days=d)).month * 100 + (first + datetime.timedelta(days=d)).day
                       for d in range(int(day.max()) + 1)], dtype=np.int64)[day]
    raw = np.stack([uid * 104729 % (2 ** 31 - 1), iid * 48611 % (2 ** 31 - 1), iid % 1200, iid % 5000, iid % 3000 - 1, mmdd], axis=1)
    return name, raw


def measure(name, raw, pairs):
    import torch
    from score_amd import dataprep as dp
    from score_amd import logremap as lr
    keep = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def host():
        keep["host"] = dp.remap_tmall_log(raw)

    def device():
        keep["device"] = dp.remap_tmall_log(raw, build="device")

    dev = lr.device_of()
    up, _ = lr.upload_columns(raw, 6, dev)
    cols = [up[j] for j in range(5)] + [torch.remainder(up[0], 9).to(torch.int32), torch.remainder(up[0], 3).to(torch.int32)]
    bits = lr.key_bits_of(int(min(c.min() for c in cols)), int(max(c.max() for c in cols)))

    def kernels():
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        keep["kernels"] = (lr.log_slices_tmall(up[5], status),
                           lr.log_remap(cols, bits, tables=((0, (5, 6)), (1, (2, 3, 4))), download=False))

    pipe = lambda remap: dp.tmall_pipeline(raw, build="device", draws="cell", targets="device", remap=remap)

    def pipeline_host():
        keep["pipeline_host"] = pipe("host")

    def pipeline_device():
        keep["pipeline_device"] = pipe("device")

    kinds = [("host_ms", host), ("device_ms", device), ("kernels_ms", kernels), ("pipeline_host_remap_ms", pipeline_host),
             ("pipeline_device_remap_ms", pipeline_device)]
    for _, fn in kinds:                                  # warm-up: the library, the kernels' code objects, the allocator
        fn()
    times = {k: [] for k, _ in kinds}
    for r in range(pairs):
        order = kinds if r % 2 == 0 else [kinds[1], kinds[0], kinds[2], kinds[4], kinds[3]]
        for k, fn in order:
            times[k].append(timed(fn))
    h, d = keep["host"], keep["device"]
    same = all(np.array_equal(d[k].cpu().numpy(), h[k]) for k in ("uid", "iid", "t_idx")) and \
        all(np.array_equal(d[k], h[k]) for k in ("user_rows", "item_rows")) and d["vocab_sizes"] == h["vocab_sizes"]
    (_, _, th), (_, _, td) = keep["pipeline_host"], keep["pipeline_device"]
    same_lines = all(np.array_equal(a, b) for n in th for a, b in zip(th[n].arrays(), td[n].arrays()))
    line = dict(what="log_remap_time", shape=name, events=int(len(raw)), users=int(h["n_users"]), items=int(h["n_items"]),
                feature_size=int(h["feature_size"]), key_bits=bits, pairs=pairs, device=torch.cuda.get_device_name(),
                device_equals_host=bool(same), pipeline_targets_equal=bool(same_lines))
    for k, v in times.items():
        line[k] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="sample,synth")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--events", type=int, default=3000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_remap_time.jsonl"))
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        name, raw = raw_shape(shape, a.events)
        line = json.dumps(measure(name, raw, a.pairs))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
