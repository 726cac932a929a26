#!/usr/bin/env python
"""Build time of the target lines of one prediction slice, and of the loader constructor behind each form:
dataprep.gen_target_lines on the host (draws="stream", the default and what the parent path runs; draws="cell") against
targets.TargetStore.from_log(build="device") (csrc/targetgen.hip), the upload of the log included; then
DeviceGraphLoader.__init__ over the Python lines (the per-line list parse) against the same constructor over the store (the
tensor hand-over).

Per shape one JSON line (appended to --out, default profiles/target_build_time.jsonl): after one warm-up of every kind,
`--pairs` rounds, each taking the kinds in alternating order (the next round with host stream and device exchanged), every
kind bracketed by torch.cuda.synchronize(); medians and the spread (min, max) of the rounds in milliseconds.
parent_path_ms = host stream lines + the list-parsing constructor, device_path_ms = device build + the store constructor.

Shapes: "sample", the bundled Tmall sample log at the Tmall constants (test slice, 99 negatives); "synth", the seeded
Tmall-shaped log of tools/graph_build_time.py, --events events (3.0 M) over 20 k users / 40 k items and 14 slices.

  python tools/target_build_time.py [--shapes sample,synth] [--pairs 3] [--events 3000000] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(sh, pairs, pred, neg=99, start=0, T=11, K=10):
    import torch
    from score_amd import dataprep as dp
    from score_amd.graph import DeviceGraphLoader, TemporalGraph
    from score_amd.targets import TargetStore
    args = (sh["uid"], sh["iid"], sh["t"], sh["U"], sh["I"], pred, neg, start, 11)
    g = TemporalGraph.from_log(sh["uid"], sh["iid"], sh["t"], sh["U"], sh["I"], sh["S"], sh["ur"], sh["ir"], max_1hop=sh["m1"],
                               max_2hop=sh["m2"], seed=11, build="device", draws="cell")
    keep = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def host_stream():
        keep["stream"] = dp.gen_target_lines(*args)

    def host_cell():
        keep["cell"] = dp.gen_target_lines(*args, draws="cell")

    def device():
        keep["device"] = TargetStore.from_log(*args, build="device")

    loader = lambda lines: DeviceGraphLoader(g, 100 * (1 + neg), lines, start, pred, neg, T, K)

    def loader_lines():
        keep["loader_lines"] = loader(keep["stream"])

    def loader_store():
        keep["loader_store"] = loader(keep["device"])

    kinds = [("host_stream_ms", host_stream), ("device_ms", device), ("host_cell_ms", host_cell),
             ("loader_lines_ms", loader_lines), ("loader_store_ms", loader_store)]
    for _, fn in kinds:                                  # warm-up: the library, the kernels' code objects, the allocator
        fn()
    times = {k: [] for k, _ in kinds}
    for r in range(pairs):
        order = kinds if r % 2 == 0 else [kinds[1], kinds[0], kinds[2], kinds[4], kinds[3]]
        for k, fn in order:
            times[k].append(timed(fn))
    line = dict(what="target_build_time", shape=sh["name"], events=int(len(sh["uid"])), users=int(sh["U"]), items=int(sh["I"]),
                pred_time=pred, neg_sample_num=neg, lines=len(keep["cell"]), pairs=pairs, device=torch.cuda.get_device_name(),
                device_equals_host_cell=bool(keep["device"].lines() == keep["cell"]))
    for k, v in times.items():
        line[k] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    line["parent_path_ms"] = round(line["host_stream_ms"]["median"] + line["loader_lines_ms"]["median"], 3)
    line["device_path_ms"] = round(line["device_ms"]["median"] + line["loader_store_ms"]["median"], 3)
    return line


def main():
    import graph_build_time as gbt
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="sample,synth")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--events", type=int, default=3000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_build_time.jsonl"))
    a = ap.parse_args()
    for name in a.shapes.split(","):
        sh = gbt.sample_shape() if name == "sample" else gbt.synth_shape(a.events)
        line = json.dumps(measure(sh, a.pairs, pred=11))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
