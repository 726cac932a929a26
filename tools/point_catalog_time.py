"""ms per call of "the k best items of a whole catalogue for L users" on a point baseline, in its two forms: "rank_topk"
(rank_async on the expanded batch of L * N samples -- every line against every catalogue row -- plus torch.topk over the
[L, N] scores: the only way to that answer without the catalogue pass) and "catalog" (recommend_async with the catalogue
already built; csrc/catalog.hip).  "build" times the catalogue build alone (score_catalog_build: zcat for all N items).
GRU4Rec at the reference's Tmall point shape (train_time_point_models.py:15-35: N_features = 1,529,672, D = 16, H = 32, T = 50,
Fu = 3, Fi = 4) against a catalogue of 40,000 items, k = 10, for L = 1, 10 and 100 lines.
Every (case, form) runs in a fresh process: `warmup` untimed calls, then `steps` timed ones on pre-staged device tensors
(random ids; history lengths up to 300, so most lines run all T steps), wall clock between two device synchronisations.  The
two forms alternate --pairs times; per case one JSON line with every pair's figures, the medians, the spread (max - min) and
the catalogue form's share of the 157 TFLOP/s fp32 matrix peak (fc2 alone: 2 * 200 * 80 flop a pair) goes to stdout and is
appended to --out.

    python tools/point_catalog_time.py --pairs 3                                   # the three cases
    python tools/point_catalog_time.py --case L100 --form catalog --steps 100 --warmup 10      # one process
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMALL = dict(N=1529672, D=16, H=32, T=50, Fu=3, Fi=4)
N_ITEMS, K = 40000, 10
CASES = {"L1": 1, "L10": 10, "L100": 100}
FORMS = ("rank_topk", "catalog")
PEAK_FP32_MATRIX = 157.3e12


def run_one(case, form, steps, warmup, model="GRU4Rec"):
    sys.path.insert(0, ROOT)
    import torch
    from score_amd import model as M
    s = dict(TMALL)
    L, n_items = CASES[case], N_ITEMS
    torch.cuda.set_device(0)
    m = M.MODELS[model](s["N"], s["D"], s["H"], s["T"], s["Fu"], s["Fi"])
    g = torch.Generator(device="cuda").manual_seed(7)
    dev = dict(device="cuda", dtype=torch.int32, generator=g)
    T, Fu, Fi = s["T"], s["Fu"], s["Fi"]
    ids = lambda *sh: torch.randint(1, s["N"], sh, **dev)
    rows = ids(n_items, Fi)
    rows[:, 0] = torch.sort(torch.randperm(s["N"] - 1, device="cuda", generator=g)[:n_items] + 1).values.to(torch.int32)
    lines = (ids(L, T, Fi), torch.randint(1, 301, (L,), **dev), ids(L, Fu))
    if form == "rank_topk":
        over = lambda x: x.repeat_interleave(n_items, 0)
        label = (torch.arange(L * n_items, device="cuda") % n_items == 0).to(torch.int32)
        batch = m.device_batch((over(lines[0]), over(lines[1]), over(lines[2]), rows.repeat(L, 1), label))

        def step():
            y = m.rank_async(batch, 0.0, neg_sample_num=n_items - 1)[0]
            return torch.topk(y.view(L, n_items), K, dim=1)
    else:
        cat = M.ItemCatalog(m, rows)
        cat.refresh()
        act = M.active_slices(m, int(lines[1].max().item()))
        if form == "catalog":
            step = lambda: m.recommend_async(lines, cat, k=K, active_slices=act)
        else:
            def step():
                cat.version = None
                cat.refresh()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return dict(model=model, case=case, form=form, ms_per_call=round(ms, 4), steps=steps, warmup=warmup, L=L, n_items=n_items, k=K, **s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=tuple(CASES))
    ap.add_argument("--form", choices=FORMS + ("build",))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--baseline-steps", type=int, default=20, help="timed calls of the rank_topk form (one is L * N samples)")
    ap.add_argument("--pairs", type=int, default=3, help="alternating (rank_topk, catalog) pairs per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_catalog_time.jsonl"), help="the file the case lines are appended to")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per fresh process")
    a = ap.parse_args()
    if a.case and a.form:
        print(json.dumps(run_one(a.case, a.form, a.steps, a.warmup)), flush=True)
        return

    def fresh(case, form, steps, warmup):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--form", form, "--steps", str(steps),
                            "--warmup", str(warmup)], capture_output=True, text=True, timeout=a.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit("%s, %s: exit status %d" % (case, form, p.returncode))
        return json.loads(p.stdout.strip().splitlines()[-1])["ms_per_call"]

    for case in (a.case,) if a.case else tuple(CASES):
        res = {f: [] for f in FORMS}
        for _ in range(a.pairs):
            res["rank_topk"].append(fresh(case, "rank_topk", a.baseline_steps, max(2, a.warmup // 5)))
            res["catalog"].append(fresh(case, "catalog", a.steps, a.warmup))
        med = {f: statistics.median(res[f]) for f in FORMS}
        line = dict(model="GRU4Rec", case=case, L=CASES[case], n_items=N_ITEMS, k=K, steps=a.steps, baseline_steps=a.baseline_steps,
                    warmup=a.warmup, pairs=a.pairs, **TMALL)
        for f in FORMS:
            line[f + "_ms"] = res[f]
            line[f + "_median_ms"] = round(med[f], 4)
            line[f + "_spread_ms"] = round(max(res[f]) - min(res[f]), 4)
        line["rank_topk_over_catalog"] = round(med["rank_topk"] / med["catalog"], 3)
        line["catalog_faster_in_pairs"] = sum(c < r for r, c in zip(res["rank_topk"], res["catalog"]))
        line["catalog_beats_baseline_by_more_than_the_spread"] = bool(
            med["rank_topk"] - med["catalog"] > max(line["rank_topk_spread_ms"], line["catalog_spread_ms"]))
        line["catalog_fc2_share_of_fp32_matrix_peak"] = round(2.0 * 200 * 80 * CASES[case] * N_ITEMS / (med["catalog"] * 1e-3) / PEAK_FP32_MATRIX, 4)
        line["build_ms"] = fresh(case, "build", a.steps, a.warmup) if case == "L1" else None
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
