"""ms per call of "where does one given item stand for each of L users in the whole catalogue", in its forms: "ranks"
(item_ranks_async: the counting form of the scoring kernel, csrc/catalog.hip), "topk" (recommend_async(k = 10): the same sweep
with the k-best list, for comparison) and "logits_count" (the route without the counting form: recommend_async(all_logits=True)
writes L x N logits, torch ops compare and count them, the exclusions applied by hand through a mask).
GRU4Rec at the reference's Tmall point shape (tools/point_catalog_time.py: the same model, lines and catalogue of 40,000
items) for L = 1, 10 and 100 users, one target each, without exclusions and with 300 excluded items a user (a long history).
Every (case, form) runs in a fresh process: `warmup` untimed calls, then `steps` timed ones on pre-staged device tensors, wall
clock between two device synchronisations.  The forms alternate --pairs times; per case one JSON line with every round's
figures, the medians and the spreads (max - min) goes to stdout and is appended to --out.

--tree DIR takes score_amd from another checkout (built there): the forms "topk" and "logits_count" need nothing of the counting
form, so a checkout without it gives the figures to compare with; its lines carry "tree".

    python tools/catalog_ranks_time.py --users L10                                       # both exclusion settings of one L
    python tools/catalog_ranks_time.py --users L10 --excl 300 --form ranks --steps 100 --warmup 10       # one process
    python tools/catalog_ranks_time.py --tree ../parent --forms topk,logits_count         # another checkout
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

FORMS = ("topk", "ranks", "logits_count")
EXCL = (0, 300)


def run_one(case, n_excl, form, steps, warmup, tree, model="GRU4Rec"):
    sys.path.insert(0, tree)
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
    tgt = torch.randint(0, n_items, (L,), **dev)
    excl = None
    if n_excl:
        e = torch.rand((L, n_items), device="cuda", generator=g).argsort(1)[:, :n_excl].sort(1).values       # [L, n_excl] ascending
        excl = (torch.arange(L + 1, device="cuda", dtype=torch.int64) * n_excl, e.reshape(-1).to(torch.int32).contiguous())
        excl_line = torch.arange(L, device="cuda").repeat_interleave(n_excl)
        excl_col = excl[1].long()
    cat = M.ItemCatalog(m, rows)
    cat.refresh()
    act = M.active_slices(m, int(lines[1].max().item()))
    if form == "ranks":
        targets = (torch.arange(L + 1, device="cuda", dtype=torch.int64), tgt.contiguous(), 1)
        step = lambda: m.item_ranks_async(lines, cat, targets, exclude_idx=excl, active_slices=act)
    elif form == "topk":
        step = lambda: m.recommend_async(lines, cat, k=K, exclude_idx=excl, active_slices=act)
    else:
        col = torch.arange(n_items, device="cuda")
        t64 = tgt.long()

        def step():
            full = m.recommend_async(lines, cat, k=K, exclude_idx=excl, active_slices=act, all_logits=True)[2]
            own = full.gather(1, t64[:, None])
            ahead = (full > own) | ((full == own) & (col[None, :] < t64[:, None]))
            if excl is not None:
                gone = torch.zeros((L, n_items), dtype=torch.bool, device="cuda")
                gone[excl_line, excl_col] = True
                ahead &= ~gone
            return ahead.sum(1), own
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return dict(model=model, case=case, form=form, ms_per_call=round(ms, 4), steps=steps, warmup=warmup, L=L, n_items=n_items,
                n_excl=n_excl, k=K, **s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", choices=tuple(CASES))
    ap.add_argument("--excl", type=int, choices=EXCL)
    ap.add_argument("--form", choices=FORMS)
    ap.add_argument("--forms", default=",".join(FORMS), help="the forms a case alternates between")
    ap.add_argument("--tree", default=ROOT, help="the checkout score_amd is taken from")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=3, help="alternating rounds of the forms per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catalog_ranks_time.jsonl"), help="the file the case lines are appended to")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per fresh process")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if a.users and a.excl is not None and a.form:
        print(json.dumps(run_one(a.users, a.excl, a.form, a.steps, a.warmup, tree)), flush=True)
        return
    forms = tuple(f for f in a.forms.split(",") if f)
    if not forms or any(f not in FORMS for f in forms):
        raise SystemExit("--forms: a comma-separated choice of %s" % (FORMS,))

    def fresh(case, n_excl, form):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--users", case, "--excl", str(n_excl), "--form", form,
                            "--steps", str(a.steps), "--warmup", str(a.warmup), "--tree", tree],
                           capture_output=True, text=True, timeout=a.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit("%s, %d excluded, %s: exit status %d" % (case, n_excl, form, p.returncode))
        return json.loads(p.stdout.strip().splitlines()[-1])["ms_per_call"]

    for case in (a.users,) if a.users else tuple(CASES):
        for n_excl in (a.excl,) if a.excl is not None else EXCL:
            res = {f: [] for f in forms}
            for _ in range(a.pairs):
                for f in forms:
                    res[f].append(fresh(case, n_excl, f))
            med = {f: statistics.median(res[f]) for f in forms}
            line = dict(model="GRU4Rec", case=case, L=CASES[case], n_items=N_ITEMS, n_excl=n_excl, targets_per_line=1, k=K,
                        steps=a.steps, warmup=a.warmup, pairs=a.pairs, **TMALL)
            if tree != ROOT:
                line["tree"] = os.path.basename(tree)
            for f in forms:
                line[f + "_ms"] = res[f]
                line[f + "_median_ms"] = round(med[f], 4)
                line[f + "_spread_ms"] = round(max(res[f]) - min(res[f]), 4)
            if "ranks" in forms:
                for f in forms:
                    if f != "ranks":
                        line[f + "_over_ranks"] = round(med[f] / med["ranks"], 3)
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
