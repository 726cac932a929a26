"""ms per training step of the two slice baselines, RRN and GCMC (slice_models/slice_model.py:155-203), through the reference's
train() signature, at two shapes:
  a: the reference's own slice-model run (train_time_slice_models.py): N = 1,529,672, D = 16, H = 32, T = 11, K = 10,
     Fu = 3, Fi = 4, B = 200
  b: the same table with cfg-3's widths: D = 64, H = 128, T = 20, B = 1024
Every (model, shape) runs in a fresh process: `warmup` untimed steps, then `steps` timed ones over a few pre-staged device
batches (random ids, random lengths), wall clock between two device synchronisations.

    python tools/slice_step_time.py                  # all four runs, one line each
    python tools/slice_step_time.py --model GCMC --shape a --steps 200 --warmup 20
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"a": dict(N=1529672, D=16, H=32, T=11, K=10, Fu=3, Fi=4, B=200),
          "b": dict(N=1529672, D=64, H=128, T=20, K=10, Fu=3, Fi=4, B=1024)}


def run_one(model_type, shape, steps, warmup, n_batches=4):
    sys.path.insert(0, ROOT)
    import torch
    from score_amd.model import MODELS
    s = SHAPES[shape]
    torch.cuda.set_device(0)
    m = MODELS[model_type](s["N"], s["D"], s["H"], s["T"], s["K"], s["Fu"], s["Fi"])
    g = torch.Generator(device="cuda").manual_seed(7)
    dev = dict(device="cuda", dtype=torch.int32, generator=g)
    B, T, K, Fu, Fi = s["B"], s["T"], s["K"], s["Fu"], s["Fi"]
    batches = []
    for _ in range(n_batches):
        ids = lambda *sh: torch.randint(1, s["N"], sh, **dev)
        batches.append(m.device_batch((ids(B, T, K, Fi), ids(B, T, K, Fu), ids(B, T, K, Fu), ids(B, T, K, Fi), ids(B, Fu),
                                       ids(B, Fi), torch.randint(0, 2, (B,), **dev), torch.randint(1, T + 1, (B,), **dev))))
    for i in range(warmup):
        m.train(None, batches[i % n_batches], 1e-3, 1e-4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        m.train(None, batches[i % n_batches], 1e-3, 1e-4)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return dict(model=model_type, shape=shape, ms_per_step=round(ms, 4), steps=steps, warmup=warmup, **s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("RRN", "GCMC"))
    ap.add_argument("--shape", choices=tuple(SHAPES))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per fresh process")
    a = ap.parse_args()
    if a.model and a.shape:
        print(json.dumps(run_one(a.model, a.shape, a.steps, a.warmup)), flush=True)
        return
    res = {}
    for shape in (a.shape,) if a.shape else tuple(SHAPES):
        for mt in (a.model,) if a.model else ("RRN", "GCMC"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", mt, "--shape", shape, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-3000:])
                raise SystemExit("%s at shape %s: exit status %d" % (mt, shape, p.returncode))
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res[(mt, shape)] = r["ms_per_step"]
            print(json.dumps(r), flush=True)
        if ("RRN", shape) in res and ("GCMC", shape) in res:
            print("shape %s: RRN %.3f ms/step, GCMC %.3f ms/step (%.2fx)"
                  % (shape, res[("RRN", shape)], res[("GCMC", shape)], res[("GCMC", shape)] / res[("RRN", shape)]), flush=True)


if __name__ == "__main__":
    main()
