"""ms per call of "the k best items for L users named by id, without what they already had" on a point baseline, by two routes:
"parent" (what the library offered before recommend_users_async: a device loader batch of the L target lines -- L * 100
samples --, model.lines_of, harness._history_exclusions, recommend_async(exclude=)) and "users" (recommend_users_async:
PointLogStore.user_lines, ItemCatalog.history_exclusions, recommend_async(exclude_idx=)).  Both with the history excluded
("excl") and without ("plain"); "passes" times the two new device passes alone (user_lines; history_exclusions).
GRU4Rec at the Tmall point shape (tools/point_catalog_time.py) over tools/point_loader_time.py's synthetic log -- 20,000 users,
3.0 M events, 40,000 items, the catalogue --, k = 10, L = 1, 10, 100 users taken from the store's own target lines.
Every (case, route, variant) runs in a fresh process: `warmup` untimed calls, then `steps` timed ones, wall clock between two
device synchronisations; host_ms is the wall clock of the same loop up to the point where the last call has returned, before
the second synchronisation (what the Python in front of the kernels costs when the device keeps up).  The two routes alternate
--pairs times; per (case, variant) one JSON line with every pair's figures, the medians and spreads (max - min) goes to stdout and
is appended to --out.

    python tools/recommend_users_time.py                                                   # every case
    python tools/recommend_users_time.py --case L10 --route users --variant excl           # one process
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
TMALL = dict(N=1529672, D=16, H=32, T=50, Fu=3, Fi=4)
K, NEG, CALLS = 10, 99, 16          # CALLS: distinct groups of L lines a process cycles through
CASES = {"L1": 1, "L10": 10, "L100": 100}
ROUTES = ("parent", "users")
VARIANTS = ("excl", "plain")


def world(L):
    """the model, the log store with CALLS * L target lines (batches of L lines), the catalogue over the store's items"""
    import numpy as np
    import torch
    import point_loader_time as plt
    from score_amd import dataprep as dp
    from score_amd import model as M
    from score_amd import pointdata as pd
    torch.cuda.set_device(0)
    g = plt.synth_log("eval1000")
    U, I = len(g["user_rows"]), len(g["item_rows"])
    rng = np.random.default_rng(3)
    lines = [(int(rng.integers(1, U + 1)), [int(x) for x in rng.integers(U + 1, U + I + 1, 1 + NEG)]) for _ in range(CALLS * L)]
    st = pd.PointLogStore(g["uid"], g["iid"], g["time_key"], g["t_idx"], lines, g["start"], g["pred"], dp.POINT_HIST_MAX_LEN, NEG,
                          L * (1 + NEG), g["user_rows"], g["item_rows"], False, build="device")
    s = TMALL
    m = M.GRU4Rec(s["N"], s["D"], s["H"], s["T"], s["Fu"], s["Fi"])
    cat = M.ItemCatalog(m, g["item_rows"])
    cat.refresh()
    return m, st, cat, len(g["uid"])


def run_one(case, route, variant, steps, warmup):
    import torch
    from score_amd import harness as h
    from score_amd import pointdata as pd
    L = CASES[case]
    m, st, cat, n_events = world(L)
    T, per = TMALL["T"], 1 + NEG
    excl = variant == "excl"
    users_all = st._dev["line_user"]
    pos_all = st._dev["line_items"].view(-1, per)[:, 0].contiguous()
    state = dict(loader=None, i=0)

    def parent():
        if state["loader"] is None or state["i"] % CALLS == 0:
            state["loader"] = iter(pd.DeviceDataLoaderUserSeq(L * per, T, None, None, NEG, None, None, model=m, store=st))
        state["i"] += 1
        b = next(state["loader"])
        lines = m.lines_of(b, NEG)
        pos = b.tensors[5].view(L, per, -1)[:, 0, 0].contiguous()
        ex = h._history_exclusions(st, lines[2][:, 0], pos) if excl else None
        return m.recommend_async(lines, cat, k=K, exclude=ex, active_slices=b.active_slices)

    def users():
        a = (state["i"] % CALLS) * L
        state["i"] += 1
        return m.recommend_users_async(users_all[a:a + L], st, cat, k=K, exclude_history=excl, keep=pos_all[a:a + L])

    def passes_lines():
        a = (state["i"] % CALLS) * L
        state["i"] += 1
        return st.user_lines(users_all[a:a + L], T)

    def passes_excl():
        a = (state["i"] % CALLS) * L
        state["i"] += 1
        return cat.history_exclusions(st, users_all[a:a + L], pos_all[a:a + L])

    def timed(step):
        state["i"] = 0
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return round((t2 - t0) * 1e3 / steps, 4), round((t1 - t0) * 1e3 / steps, 4)
    out = dict(case=case, route=route, variant=variant, L=L, steps=steps, warmup=warmup, n_events=n_events, n_items=cat.N, k=K)
    if route == "passes":
        out["user_lines_ms"], out["user_lines_host_ms"] = timed(passes_lines)
        out["history_exclusions_ms"], out["history_exclusions_host_ms"] = timed(passes_excl)
        out["max_user_events"], out["excl_capacity"] = st.max_user_events, max(1, L * min(st.max_user_events, cat.N))
    else:
        out["ms_per_call"], out["host_ms_per_call"] = timed(parent if route == "parent" else users)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=tuple(CASES))
    ap.add_argument("--route", choices=ROUTES + ("passes",))
    ap.add_argument("--variant", choices=VARIANTS, default="excl")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=3, help="alternating (parent, users) pairs per case and variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_users_time.jsonl"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per fresh process")
    a = ap.parse_args()
    if a.case and a.route:
        print(json.dumps(run_one(a.case, a.route, a.variant, a.steps, a.warmup)), flush=True)
        return

    def fresh(case, route, variant):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--route", route, "--variant", variant,
                            "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=a.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit("%s, %s, %s: exit status %d" % (case, route, variant, p.returncode))
        return json.loads(p.stdout.strip().splitlines()[-1])

    for case in (a.case,) if a.case else tuple(CASES):
        alone = fresh(case, "passes", "excl")
        for variant in VARIANTS:
            res = {r: [] for r in ROUTES}
            host = {r: [] for r in ROUTES}
            for _ in range(a.pairs):
                for r in ROUTES:
                    one = fresh(case, r, variant)
                    res[r].append(one["ms_per_call"])
                    host[r].append(one["host_ms_per_call"])
            line = dict(model="GRU4Rec", case=case, variant=variant, L=CASES[case], n_items=alone["n_items"], n_events=alone["n_events"],
                        k=K, steps=a.steps, warmup=a.warmup, pairs=a.pairs, **TMALL)
            for r in ROUTES:
                line[r + "_ms"] = res[r]
                line[r + "_median_ms"] = round(statistics.median(res[r]), 4)
                line[r + "_spread_ms"] = round(max(res[r]) - min(res[r]), 4)
                line[r + "_host_median_ms"] = round(statistics.median(host[r]), 4)
            spread = max(line["parent_spread_ms"], line["users_spread_ms"])
            line["parent_over_users"] = round(line["parent_median_ms"] / line["users_median_ms"], 3)
            line["users_faster_in_pairs"] = sum(u < p for p, u in zip(res["parent"], res["users"]))
            line["users_faster_in_every_pair_by_more_than_twice_the_spread"] = bool(
                all(p - u > 2 * spread for p, u in zip(res["parent"], res["users"])))
            for k in ("user_lines_ms", "user_lines_host_ms", "history_exclusions_ms", "history_exclusions_host_ms", "max_user_events",
                      "excl_capacity"):
                line[k] = alone[k]
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
