"""ms per training step (and per evaluation call) of a point baseline (point_models/point_model.py:123-469:
GRU4Rec, Caser, SVD++, DELF, DEEMS, SASRec) through
the reference's train() / eval signatures, at the reference's point-model shapes (train_time_point_models.py:15-35, 353-354):
Tmall, N = 1,529,672, D = 16, H = 32, T = 50, Fu = 3, Fi = 4,
  train100: B = 100      train200: B = 200      eval1000: forward only (eval_async), B = 1000
each in both forms of the two stacked recurrences: "stacked" (csrc/gru_stack.hip, one kernel each way) and "composed"
(debug_flags bit 13: one layer per launch with the projection GEMM between them -- kernels the other model types run too).
--model Caser times the Caser baseline (form "caser": csrc/caser.hip) against GRU4Rec's stacked form, alternating, same protocol;
--model DELF the DELF baseline (form "delf": csrc/delf.hip; its batches carry a second history and length).
--model DEEMS alternates DEEMS's own two forms on DELF's batches: "deems" (csrc/deems.hip: both towers in one launch each way, both
recurrences in one grouped launch each way) and "deems_composed" (debug_flags bits 6 | 13: the towers layer by layer, one
recurrence per launch).
--model SVDpp times the SVD++ baseline (form "svdpp": csrc/svdpp.hip, one launch each way) against GRU4Rec's stacked form at
train200 and eval1000.
--model SASRec times the SASRec baseline (form "sasrec": csrc/sasrec.hip, the attention in one launch each way, the shared head over
2 T - 2 rows per sample; train() at its default keep_prob 0.8) against GRU4Rec's stacked form at train200 and eval1000.
Every (case, form) runs in a fresh process: `warmup` untimed steps, then `steps` timed ones over a few pre-staged device
batches (random ids; history lengths as the loader reports them, up to 300, so most samples run all T steps), wall clock
between two device synchronisations.  With --pairs n the two forms alternate n times.

    python tools/point_step_time.py                          # three cases x two forms, one JSON line each
    python tools/point_step_time.py --pairs 3                # ... three alternating pairs per case
    python tools/point_step_time.py --case train200 --form composed --steps 200 --warmup 20
    python tools/point_step_time.py --model Caser --pairs 3  # three cases, (GRU4Rec stacked, Caser) alternating three times
    python tools/point_step_time.py --model DELF --pairs 3   # ... (GRU4Rec stacked, DELF)
    python tools/point_step_time.py --model DEEMS --pairs 3  # ... (DEEMS fused, DEEMS composed)
    python tools/point_step_time.py --model SVDpp --pairs 3  # train200 and eval1000, (GRU4Rec stacked, SVD++) alternating three times
    python tools/point_step_time.py --model SASRec --pairs 3 # ... (GRU4Rec stacked, SASRec)
    python tools/point_step_time.py --case train200 --form stacked --profile-steps 30     # no timing: a short run for a profiler
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMALL = dict(N=1529672, D=16, H=32, T=50, Fu=3, Fi=4)
CASES = {"train100": dict(B=100, train=True), "train200": dict(B=200, train=True), "eval1000": dict(B=1000, train=False)}
FORMS = {"stacked": 0, "composed": 8192, "caser": 0, "delf": 0, "deems": 0, "deems_composed": 64 | 8192,
         "svdpp": 0, "sasrec": 0}      # debug_flags of a form
FORM_MODEL = {"stacked": "GRU4Rec", "composed": "GRU4Rec", "caser": "Caser", "delf": "DELF", "deems": "DEEMS", "deems_composed": "DEEMS",
              "svdpp": "SVDpp", "sasrec": "SASRec"}
PAIRS = {"GRU4Rec": ("stacked", "composed"), "Caser": ("stacked", "caser"), "DELF": ("stacked", "delf"),
         "DEEMS": ("deems", "deems_composed"), "SVDpp": ("stacked", "svdpp"),
         "SASRec": ("stacked", "sasrec")}     # what --model alternates
MODEL_CASES = {"SVDpp": ("train200", "eval1000"), "SASRec": ("train200", "eval1000")}      # the cases --model runs without --case (default: all three)


def run_one(case, form, steps, warmup, n_batches=4, H=None):
    sys.path.insert(0, ROOT)
    import torch
    from score_amd.model import MODELS
    s = dict(TMALL, **CASES[case])
    if H:
        s["H"] = H
    torch.cuda.set_device(0)
    m = MODELS[FORM_MODEL[form]](s["N"], s["D"], s["H"], s["T"], s["Fu"], s["Fi"])
    m.debug_flags = FORMS[form]
    g = torch.Generator(device="cuda").manual_seed(7)
    dev = dict(device="cuda", dtype=torch.int32, generator=g)
    B, T, Fu, Fi = s["B"], s["T"], s["Fu"], s["Fi"]
    ids = lambda *sh: torch.randint(1, s["N"], sh, **dev)
    lens = lambda: torch.randint(1, 301, (B,), **dev)
    if FORM_MODEL[form] in ("DELF", "DEEMS"):      # (the 7-tuple: a second history, of users, with lengths of its own)
        batches = [m.device_batch((ids(B, T, Fi), lens(), ids(B, T, Fu), lens(), ids(B, Fu), ids(B, Fi),
                                   torch.randint(0, 2, (B,), **dev))) for _ in range(n_batches)]
    else:
        batches = [m.device_batch((ids(B, T, Fi), lens(), ids(B, Fu), ids(B, Fi), torch.randint(0, 2, (B,), **dev)))
                   for _ in range(n_batches)]

    def step(i):
        if s["train"]:
            m.train(None, batches[i % n_batches], 1e-3, 1e-4)
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
    return dict(model=FORM_MODEL[form], case=case, form=form, ms_per_step=round(ms, 4), steps=steps, warmup=warmup, **s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=tuple(CASES))
    ap.add_argument("--form", choices=tuple(FORMS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", choices=tuple(PAIRS), default="GRU4Rec", help="the model whose two forms (Caser / DELF / SVDpp / SASRec: GRU4Rec stacked and the model) alternate")
    ap.add_argument("--pairs", type=int, default=1, help="alternating pairs per case")
    ap.add_argument("--hidden", type=int, default=0, help="another hidden size than the reference's 32")
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many steps after the warm-up and print nothing timed")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per fresh process")
    a = ap.parse_args()
    if a.case and a.form:
        r = run_one(a.case, a.form, a.profile_steps or a.steps, a.warmup, H=a.hidden)
        if a.profile_steps:
            r.pop("ms_per_step")
        print(json.dumps(r), flush=True)
        return
    for case in (a.case,) if a.case else MODEL_CASES.get(a.model, tuple(CASES)):
        first, second = PAIRS[a.model]
        res = {f: [] for f in FORMS}
        for _ in range(a.pairs):
            for form in (a.form,) if a.form else (first, second):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--form", form, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup), "--hidden", str(a.hidden)], capture_output=True, text=True,
                                   timeout=a.timeout)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-3000:])
                    raise SystemExit("%s, %s: exit status %d" % (case, form, p.returncode))
                r = json.loads(p.stdout.strip().splitlines()[-1])
                res[form].append(r["ms_per_step"])
                print(json.dumps(r), flush=True)
        if res[first] and res[second]:
            print("%s: %s %s ms, %s %s ms; %s faster in %d of %d pairs"
                  % (case, first, res[first], second, res[second], first, sum(x < y for x, y in zip(res[first], res[second])),
                     len(res[first])), flush=True)


if __name__ == "__main__":
    main()
