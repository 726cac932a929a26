#!/usr/bin/env python
"""Build time of the temporal graph store: TemporalGraph.from_log on the host (draws="stream", today's default and the
yardstick; draws="cell") against the device build (build="device", csrc/graphbuild.hip), and what the host graph's upload costs.

Per shape one JSON line (appended to --out, default profiles/graph_build_time.jsonl): after one warm-up build of every kind,
`--pairs` rounds, each taking the builds in alternating order (host stream, device, host cell, upload; the next round
with host stream and device exchanged), whole builds bracketed by torch.cuda.synchronize(); medians and the spread (min,
max) of the rounds in milliseconds.  The device build is also run once more with a synchronisation after every stage, which gives its split into
sort (both sides' 1-hop), shuffle + count (per side: the over-long cells' two sorts, the count kernel, the scan) and fill.

Shapes: "sample", the bundled Tmall sample log (tests/golden/tmall_sample_log.npz) at the Tmall constants; "synth", a seeded
Tmall-shaped log of --events events (3.0 M) over 20 k users / 40 k items and 14 slices with a skewed item popularity, caps
10 / 100.

  python tools/graph_build_time.py [--shapes sample,synth] [--pairs 3] [--events 3000000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sample_shape():
    from score_amd import dataprep as dp
    raw = np.load(os.path.join(ROOT, "tests", "golden", "tmall_sample_log.npz"))["log"]
    r = dp.remap_tmall_log(raw)
    c = dp.TMALL
    return dict(name="sample", uid=r["uid"], iid=r["iid"], t=r["t_idx"], U=r["n_users"], I=r["n_items"],
                S=c["graph_time_slice_num"], m1=c["max_1hop"], m2=c["max_2hop"], ur=r["user_rows"], ir=r["item_rows"])


def synth_shape(n_events, U=20000, I=40000, S=14):
    rng = np.random.default_rng(2015)
    uid = 1 + np.minimum((U * rng.random(n_events) ** 1.5).astype(np.int64), U - 1)
    iid = U + 1 + np.minimum((I * rng.random(n_events) ** 3).astype(np.int64), I - 1)
    t = rng.integers(0, S, n_events)
    return dict(name="synth", uid=uid, iid=iid, t=t, U=U, I=I, S=S, m1=10, m2=100,
                ur=np.arange(1, U + 1, dtype=np.int32)[:, None].repeat(3, 1),
                ir=np.arange(U + 1, U + I + 1, dtype=np.int32)[:, None].repeat(4, 1))


def store_bytes(g):
    n = 0
    for csr, deg in ((g.user_csr, g.user_degrees), (g.item_csr, g.item_degrees)):
        n += sum(int(np.asarray(csr[k]).nbytes) for k in ("off1", "nbr1", "off2", "nbr2")) + int(np.asarray(deg).nbytes)
    return n


def measure(sh, pairs):
    import torch
    from score_amd.graph import TemporalGraph
    args = (sh["uid"], sh["iid"], sh["t"], sh["U"], sh["I"], sh["S"], sh["ur"], sh["ir"])
    kw = dict(max_1hop=sh["m1"], max_2hop=sh["m2"], seed=11)
    keep = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def host_stream():
        keep["stream"] = TemporalGraph.from_log(*args, **kw)

    def host_cell():
        keep["cell"] = TemporalGraph.from_log(*args, draws="cell", **kw)

    def device():
        keep["device"] = TemporalGraph.from_log(*args, build="device", draws="cell", **kw)

    def upload():
        keep["cell"].to_device(mode="is")

    kinds = [("host_stream_ms", host_stream), ("device_ms", device), ("host_cell_ms", host_cell), ("upload_ms", upload)]
    for _, fn in (kinds[2], kinds[1], kinds[3]):         # warm-up: the library, the kernels' code objects, the allocator
        fn()
    times = {k: [] for k, _ in kinds}
    for r in range(pairs):
        order = kinds if r % 2 == 0 else [kinds[1], kinds[0], kinds[2], kinds[3]]
        for k, fn in order:
            times[k].append(timed(fn)[0])
    split = {}
    TemporalGraph._from_log_device(*args, sh["m1"], sh["m2"], 11, None, timings=split)
    d, h = keep["device"], keep["cell"]
    same = all(np.array_equal(getattr(d, s)[k], getattr(h, s)[k]) for s in ("user_csr", "item_csr")
               for k in ("off1", "nbr1", "off2", "nbr2"))
    same = same and np.array_equal(d.user_degrees, h.user_degrees) and np.array_equal(d.item_degrees, h.item_degrees)
    line = dict(what="graph_build_time", shape=sh["name"], events=int(len(sh["uid"])), users=int(sh["U"]), items=int(sh["I"]),
                slices=int(sh["S"]), max_1hop=sh["m1"], max_2hop=sh["m2"], pairs=pairs,
                device=torch.cuda.get_device_name(), device_equals_host_cell=bool(same),
                store_bytes=store_bytes(h), store_bytes_stream=store_bytes(keep["stream"]),
                device_split_ms={k: round(v * 1e3, 3) for k, v in split.items()})
    for k, v in times.items():
        line[k] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="sample,synth")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--events", type=int, default=3000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_build_time.jsonl"))
    a = ap.parse_args()
    for name in a.shapes.split(","):
        sh = sample_shape() if name == "sample" else synth_shape(a.events)
        line = json.dumps(measure(sh, a.pairs))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
