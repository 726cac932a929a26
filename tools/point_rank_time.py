"""ms per evaluation call of a point baseline over target LINES, in its two forms: "eval" (eval_async on the expanded batch of
B = L * C samples: the history encoder runs once per sample, as in the reference's loop, train_time_point_models.py:127-154) and
"rank" (rank_async: once per line, then one head launch over the L * C candidates; csrc/rank.hip).  GRU4Rec and Caser at the
reference's Tmall point shape (train_time_point_models.py:15-35: N = 1,529,672, D = 16, H = 32, T = 50, Fu = 3, Fi = 4), at
  10x100: L = 10 lines of C = 100 candidates, the reference's evaluation batch      100x100: L = 100
Every (model, case, form) runs in a fresh process: `warmup` untimed calls, then `steps` timed ones over a few pre-staged device
batches made of lines (random ids; history lengths as the loader reports them, up to 300, so most lines run all T steps), wall
clock between two device synchronisations.  The two forms alternate --pairs times; per (model, case) one JSON line with every
pair's figures, the medians and the spread (max - min) goes to stdout and is appended to --out.

    python tools/point_rank_time.py --pairs 3                                   # both models, both cases
    python tools/point_rank_time.py --model Caser --case 100x100 --pairs 3
    python tools/point_rank_time.py --model GRU4Rec --case 10x100 --form rank --steps 200 --warmup 20      # one process
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
CASES = {"10x100": dict(L=10, C=100), "100x100": dict(L=100, C=100)}
MODELS = ("GRU4Rec", "Caser")
FORMS = ("eval", "rank")


def run_one(model, case, form, steps, warmup, n_batches=4):
    sys.path.insert(0, ROOT)
    import torch
    from score_amd.model import MODELS as M
    s = dict(TMALL, **CASES[case])
    torch.cuda.set_device(0)
    m = M[model](s["N"], s["D"], s["H"], s["T"], s["Fu"], s["Fi"])
    g = torch.Generator(device="cuda").manual_seed(7)
    dev = dict(device="cuda", dtype=torch.int32, generator=g)
    L, C, T, Fu, Fi = s["L"], s["C"], s["T"], s["Fu"], s["Fi"]
    ids = lambda *sh: torch.randint(1, s["N"], sh, **dev)
    over = lambda x: x.repeat_interleave(C, 0)        # a line's tensor written for each of its C samples, as the loader does
    label = (torch.arange(L * C, device="cuda") % C == 0).to(torch.int32)
    batches = [m.device_batch((over(ids(L, T, Fi)), over(torch.randint(1, 301, (L,), **dev)), over(ids(L, Fu)), ids(L * C, Fi), label))
               for _ in range(n_batches)]

    def step(i):
        if form == "rank":
            m.rank_async(batches[i % n_batches], 1e-4, neg_sample_num=C - 1)
        else:
            m.eval_async(batches[i % n_batches], 1e-4)
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return dict(model=model, case=case, form=form, ms_per_call=round(ms, 4), steps=steps, warmup=warmup, **s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=MODELS)
    ap.add_argument("--case", choices=tuple(CASES))
    ap.add_argument("--form", choices=FORMS)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3, help="alternating (eval, rank) pairs per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_rank_time.jsonl"), help="the file the case lines are appended to")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per fresh process")
    a = ap.parse_args()
    if a.model and a.case and a.form:
        print(json.dumps(run_one(a.model, a.case, a.form, a.steps, a.warmup)), flush=True)
        return
    for model in (a.model,) if a.model else MODELS:
        for case in (a.case,) if a.case else tuple(CASES):
            res = {f: [] for f in FORMS}
            for _ in range(a.pairs):
                for form in FORMS:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", model, "--case", case, "--form", form,
                                        "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True,
                                       timeout=a.timeout)
                    if p.returncode != 0:
                        sys.stderr.write(p.stderr[-3000:])
                        raise SystemExit("%s, %s, %s: exit status %d" % (model, case, form, p.returncode))
                    res[form].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_call"])
            med = {f: statistics.median(res[f]) for f in FORMS}
            line = dict(model=model, case=case, steps=a.steps, warmup=a.warmup, pairs=a.pairs, **dict(TMALL, **CASES[case]))
            for f in FORMS:
                line[f + "_ms"] = res[f]
                line[f + "_median_ms"] = round(med[f], 4)
                line[f + "_spread_ms"] = round(max(res[f]) - min(res[f]), 4)
            line["eval_over_rank"] = round(med["eval"] / med["rank"], 3)
            line["rank_faster_in_pairs"] = sum(r < e for e, r in zip(res["eval"], res["rank"]))
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
