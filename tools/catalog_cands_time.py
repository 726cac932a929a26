"""ms per call of "the k best of each user's own C candidates out of a catalogue", in its three forms: "cands"
(recommend_async(candidates=...) with the lists already mapped: score_catalog_topk_in, csrc/catalog.hip), "gather_topk" (the
whole-catalogue call with all_logits, then a gather of the listed columns and torch.topk) and "rank_topk" (rank_async on the
expanded batch of L * C samples plus torch.topk; the lists have one length here, which that form needs).  At C = N a fourth
form, "catalog" (recommend_async without candidates), stands beside them.
GRU4Rec at the reference's Tmall point shape (tools/point_catalog_time.py: the same model, lines and catalogue of 40,000 items,
k = 10) for L = 1, 10 and 100 users and C = 100, 1,000, 10,000 and N candidates a user, drawn without replacement, ascending.
Every (case, form) runs in a fresh process: `warmup` untimed calls, then `steps` timed ones on pre-staged device tensors, wall
clock between two device synchronisations.  The forms alternate --pairs times; per case one JSON line with every round's
figures, the medians and the spreads (max - min) goes to stdout and is appended to --out.

    python tools/catalog_cands_time.py --users L10                                  # the four C of one L
    python tools/catalog_cands_time.py --users L10 --cands 1000 --form cands --steps 100 --warmup 10       # one process
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from point_catalog_time import CASES, K, N_ITEMS, TMALL          # noqa: E402

CANDS = (100, 1000, 10000, N_ITEMS)
FORMS = ("gather_topk", "rank_topk", "cands")


def run_one(case, n_cand, form, steps, warmup, model="GRU4Rec"):
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
    cand = torch.rand((L, n_items), device="cuda", generator=g).argsort(1)[:, :n_cand].sort(1).values       # [L, C] ascending
    cand_off = torch.arange(L + 1, device="cuda", dtype=torch.int64) * n_cand
    cand_idx = cand.reshape(-1).to(torch.int32).contiguous()
    if form == "rank_topk":
        over = lambda x: x.repeat_interleave(n_cand, 0)
        label = (torch.arange(L * n_cand, device="cuda") % n_cand == 0).to(torch.int32)
        batch = m.device_batch((over(lines[0]), over(lines[1]), over(lines[2]), rows[cand.reshape(-1)], label))

        def step():
            y = m.rank_async(batch, 0.0, neg_sample_num=n_cand - 1)[0]
            v, p = torch.topk(y.view(L, n_cand), K, dim=1)
            return cand.gather(1, p), v
    else:
        cat = M.ItemCatalog(m, rows)
        cat.refresh()
        act = M.active_slices(m, int(lines[1].max().item()))
        if form == "cands":
            step = lambda: m.recommend_async(lines, cat, k=K, active_slices=act, candidates=(cand_off, cand_idx, n_cand))
        elif form == "catalog":
            step = lambda: m.recommend_async(lines, cat, k=K, active_slices=act)
        else:
            def step():
                full = m.recommend_async(lines, cat, k=K, active_slices=act, all_logits=True)[2]
                v, p = torch.topk(full.gather(1, cand), K, dim=1)
                return cand.gather(1, p), v
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return dict(model=model, case=case, form=form, ms_per_call=round(ms, 4), steps=steps, warmup=warmup, L=L, n_items=n_items,
                n_cand=n_cand, k=K, **s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", choices=tuple(CASES))
    ap.add_argument("--cands", type=int, choices=CANDS)
    ap.add_argument("--form", choices=FORMS + ("catalog",))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--baseline-steps", type=int, default=20, help="timed calls of the rank_topk form (one is L * C samples)")
    ap.add_argument("--pairs", type=int, default=3, help="alternating rounds of the forms per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catalog_cands_time.jsonl"), help="the file the case lines are appended to")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per fresh process")
    a = ap.parse_args()
    if a.users and a.cands and a.form:
        print(json.dumps(run_one(a.users, a.cands, a.form, a.steps, a.warmup)), flush=True)
        return

    def fresh(case, n_cand, form):
        steps, warmup = (a.baseline_steps, max(2, a.warmup // 5)) if form == "rank_topk" else (a.steps, a.warmup)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--users", case, "--cands", str(n_cand), "--form", form,
                            "--steps", str(steps), "--warmup", str(warmup)], capture_output=True, text=True, timeout=a.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit("%s, C = %d, %s: exit status %d" % (case, n_cand, form, p.returncode))
        return json.loads(p.stdout.strip().splitlines()[-1])["ms_per_call"]

    for case in (a.users,) if a.users else tuple(CASES):
        for n_cand in (a.cands,) if a.cands else CANDS:
            forms = FORMS + (("catalog",) if n_cand == N_ITEMS else ())
            res = {f: [] for f in forms}
            for _ in range(a.pairs):
                for f in forms:
                    res[f].append(fresh(case, n_cand, f))
            med = {f: statistics.median(res[f]) for f in forms}
            line = dict(model="GRU4Rec", case=case, L=CASES[case], n_items=N_ITEMS, n_cand=n_cand, k=K, steps=a.steps,
                        baseline_steps=a.baseline_steps, warmup=a.warmup, pairs=a.pairs, **TMALL)
            for f in forms:
                line[f + "_ms"] = res[f]
                line[f + "_median_ms"] = round(med[f], 4)
                line[f + "_spread_ms"] = round(max(res[f]) - min(res[f]), 4)
            for f in forms[:-1] if n_cand != N_ITEMS else ("gather_topk", "rank_topk", "catalog"):
                line[f + "_over_cands"] = round(med[f] / med["cands"], 3)
                line["cands_faster_than_%s_in_rounds" % f] = sum(c < r for r, c in zip(res[f], res["cands"]))
                line["cands_beats_%s_by_more_than_the_spread" % f] = bool(
                    med[f] - med["cands"] > max(line[f + "_spread_ms"], line["cands_spread_ms"]))
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
