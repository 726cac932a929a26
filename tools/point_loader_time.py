"""What feeding a point baseline from FILES costs, host loader against device loader (score_amd/pointdata.py), at the Tmall point
shape of tools/point_step_time.py (N = 1,529,672, D = 16, H = 32, T = 50, Fu = 3, Fi = 4) for GRU4Rec (DataLoaderUserSeq) and
DEEMS (DataLoaderDualSeq) at
  train200: B = 200, 1 negative per line      eval1000: forward only (eval_async), B = 1000, 99 negatives per line.
The files are written from a seed into a temporary directory: histories of 1 - 299 ids, both feature dictionaries.  Every
measurement runs in a fresh process and is one JSON line (stdout and --out, default profiles/point_loader_time.jsonl):
  what = "loaders":  ms per batch of the host loader alone (second pass over the files), of the host loader + DeviceBatch
                     (the upload included, one synchronisation at the end of the pass), and of the device loader (store built
                     before, its parse + upload reported as store_s; one synchronisation at the end of the pass);
  what = "pass":     end-to-end ms per step over a whole pass of train() / eval_async() fed by one of the two loaders -- wall clock
                     between two device synchronisations, a warm-up of `--warmup` steps first; the two loaders alternate
                     --pairs (3) times.  A device-loader pass builds its loader on the store of the warm-up's, as a training
                     script does per epoch.

  what = "from_log": (--from-log) the same two shapes -- DEEMS eval1000 (dual, 99 negatives, B = 1000) and GRU4Rec train200
                     (single, B = 200) -- fed from a synthetic LOG of 20,000 users whose histories run 1 - 299 events over
                     40,000 items: bytes of the log store (score_amd.pointdata.PointLogStore) against the file store's
                     (PointSeqStore over the files dataprep.point_history_lines / write_point_files write), the device build
                     against the numpy build, and ms per batch of score_point_batch_assemble_log against
                     score_point_batch_assemble on the same lines: whole passes between two synchronisations, the two forms
                     alternating --pairs times after a warm-up pass each; medians and the spread (max - min) of each.

    python tools/point_loader_time.py                               # GRU4Rec and DEEMS, both cases
    python tools/point_loader_time.py --model DEEMS --case eval1000
    python tools/point_loader_time.py --from-log
"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TMALL = dict(N=1529672, D=16, H=32, T=50, Fu=3, Fi=4)
CASES = {"train200": dict(B=200, neg=1, train=True, batches=40), "eval1000": dict(B=1000, neg=99, train=False, batches=12)}
DUAL = {"GRU4Rec": False, "DEEMS": True}


def write_files(d, case, seed=7):
    """target / user history / item history files and the two dictionaries of a case (one line more than whole batches)"""
    import numpy as np
    c = CASES[case]
    rng = np.random.default_rng(seed)
    per = 1 + c["neg"]
    n_lines = c["batches"] * (c["B"] // per) + 1
    users = rng.choice(np.arange(1, TMALL["N"]), 20000, replace=False)
    items = rng.choice(np.arange(1, TMALL["N"]), 40000, replace=False)
    seq = lambda pool: ",".join(map(str, rng.choice(pool, int(rng.integers(1, 300)))))
    with open(os.path.join(d, "target.txt"), "w") as t, open(os.path.join(d, "hist.txt"), "w") as h, \
            open(os.path.join(d, "ihist.txt"), "w") as ih:
        for _ in range(n_lines):
            t.write("%d,%s\n" % (rng.choice(users), ",".join(map(str, rng.choice(items, per)))))
            h.write(seq(items) + "\n")
            ih.write("\t".join(seq(users) for _ in range(per)) + "\n")
    for nm, pool, F in (("ufeat.pkl", users, TMALL["Fu"]), ("ifeat.pkl", items, TMALL["Fi"])):
        feats = rng.integers(1, TMALL["N"], (len(pool), F - 1))
        with open(os.path.join(d, nm), "wb") as f:
            pickle.dump({str(int(k)): [int(x) for x in row] for k, row in zip(pool, feats)}, f)


def _loaders(d, model_name, case):
    """-> (host(), device(model=None, store=None)) constructors over the case's files"""
    from score_amd import pointdata as pd
    c = CASES[case]
    p = lambda n: os.path.join(d, n)
    files = (p("target.txt"), p("hist.txt")) + ((p("ihist.txt"),) if DUAL[model_name] else ())
    tail = (c["neg"], p("ufeat.pkl"), p("ifeat.pkl"))
    H, Dv = (pd.DataLoaderDualSeq, pd.DeviceDataLoaderDualSeq) if DUAL[model_name] else (pd.DataLoaderUserSeq, pd.DeviceDataLoaderUserSeq)
    return (lambda: H(c["B"], TMALL["T"], *files, *tail)), (lambda **kw: Dv(c["B"], TMALL["T"], *files, *tail, **kw))


def _model(model_name):
    import torch
    from score_amd.model import MODELS
    torch.cuda.set_device(0)
    s = TMALL
    return MODELS[model_name](s["N"], s["D"], s["H"], s["T"], s["Fu"], s["Fi"])


def run_loaders(d, model_name, case):
    import torch
    from score_amd.model import DeviceBatch
    host, device = _loaders(d, model_name, case)
    m = _model(model_name)
    for b in host():          # first pass: the page cache and the loader's row caches see the files
        pass
    t0 = time.perf_counter()
    n = sum(1 for _ in host())
    host_ms = (time.perf_counter() - t0) * 1e3 / n
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in host():
        DeviceBatch(m, b)
    torch.cuda.synchronize()
    host_db_ms = (time.perf_counter() - t0) * 1e3 / n
    t0 = time.perf_counter()
    first = device(model=m)
    torch.cuda.synchronize()
    store_s = time.perf_counter() - t0
    for b in first:           # (warm-up: the kernel's code object, the allocator's blocks)
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in device(model=m, store=first.store):
        pass
    torch.cuda.synchronize()
    dev_ms = (time.perf_counter() - t0) * 1e3 / n
    return dict(what="loaders", model=model_name, case=case, batches=n, host_ms_per_batch=round(host_ms, 4),
                host_devicebatch_ms_per_batch=round(host_db_ms, 4), device_ms_per_batch=round(dev_ms, 4), store_s=round(store_s, 3))


def run_pass(d, model_name, case, loader, warmup):
    import torch
    host, device = _loaders(d, model_name, case)
    m = _model(model_name)
    train = CASES[case]["train"]

    def step(b):
        if train:
            m.train(None, b, 1e-3, 1e-4)
        else:
            m.eval_async(m.device_batch(b), 1e-4)
    first = device(model=m) if loader == "device" else host()
    for i, b in enumerate(first):
        if i >= warmup:
            break
        step(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for b in (device(model=m, store=first.store) if loader == "device" else host()):
        step(b)
        n += 1
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / n
    return dict(what="pass", model=model_name, case=case, loader=loader, steps=n, warmup=warmup, ms_per_step=round(ms, 4))


def synth_log(case, seed=7, n_users=20000, n_items=40000):
    """a remapped log (users 1 .. U, items U + 1 .. U + I) whose user histories run 1 - 299 events, days of May - August 2015
    (all inside the window [0, 8)), its tables and the case's target lines (one line more than whole batches)"""
    import numpy as np
    from score_amd import dataprep as dp
    c = CASES[case]
    rng = np.random.default_rng(seed)
    U, I = n_users, n_items
    counts = rng.integers(1, 300, U)
    uid = np.repeat(np.arange(1, U + 1), counts)
    uid = uid[rng.permutation(len(uid))]
    iid = rng.integers(U + 1, U + I + 1, len(uid))
    days = np.asarray([m * 100 + d for m in (5, 6, 7, 8) for d in range(1, 29)])
    mmdd = rng.choice(days, len(uid))
    per = 1 + c["neg"]
    lines = [(int(rng.integers(1, U + 1)), [int(x) for x in rng.integers(U + 1, U + I + 1, per)])
             for _ in range(c["batches"] * (c["B"] // per) + 1)]
    user_rows = np.concatenate([np.arange(1, U + 1)[:, None], rng.integers(U + I + 1, TMALL["N"], (U, TMALL["Fu"] - 1))], axis=1)
    item_rows = np.concatenate([np.arange(U + 1, U + I + 1)[:, None], rng.integers(U + I + 1, TMALL["N"], (I, TMALL["Fi"] - 1))], axis=1)
    return dict(uid=uid, iid=iid, time_key=mmdd, t_idx=dp.tmall_slice_index(mmdd), lines=lines, user_rows=user_rows,
                item_rows=item_rows, start=0, pred=8)


def run_from_log(d, model_name, case, pairs):
    import statistics
    import numpy as np
    import torch
    from score_amd import dataprep as dp
    from score_amd import pointdata as pd
    torch.cuda.set_device(0)
    c, dual, T = CASES[case], DUAL[model_name], TMALL["T"]
    g = synth_log(case)
    args = (g["uid"], g["iid"], g["time_key"], g["t_idx"], g["lines"], g["start"], g["pred"], dp.POINT_HIST_MAX_LEN, c["neg"],
            c["B"], g["user_rows"], g["item_rows"], dual)
    build_s = {}
    for build in ("device", "device", "host"):          # (the first device build loads the code objects: the second is reported)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = pd.PointLogStore(*args, build=build)
        torch.cuda.synchronize()
        build_s[build] = time.perf_counter() - t0
        if build == "device":
            log_store = st
    t0 = time.perf_counter()
    users, items = dp.point_history_lines(g["uid"], g["iid"], g["time_key"], g["t_idx"], g["lines"], g["start"], g["pred"])
    tf, uf, itf, ud, idd = dp.write_point_files(d, g["lines"], users, items, g["user_rows"], g["item_rows"])
    write_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    file_store = pd.PointSeqStore(tf, uf, itf if dual else None, T, c["neg"], c["B"], ud, idd).to_device()
    torch.cuda.synchronize()
    parse_s = time.perf_counter() - t0
    names = ("user_off", "user_seq", "user_len", "item_off", "item_seq", "item_len", "target_user", "target_item")
    file_bytes = sum(int(getattr(file_store, k).nbytes) for k in names if getattr(file_store, k) is not None)
    Dv = pd.DeviceDataLoaderDualSeq if dual else pd.DeviceDataLoaderUserSeq
    files = (None, None, None) if dual else (None, None)

    def one_pass(store):
        loader = Dv(c["B"], T, *files, c["neg"], None, None, store=store)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in loader)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    # the two forms yield the same batches (checked on the first one), then the timed passes
    a, b = next(Dv(c["B"], T, *files, c["neg"], None, None, store=log_store)), next(Dv(c["B"], T, *files, c["neg"], None, None, store=file_store))
    same = all(bool(torch.equal(a[k], b[k])) for k in range(len(a)))
    for st in (log_store, file_store):
        one_pass(st)
    ms = {"log": [], "file": []}
    for _ in range(pairs):
        ms["log"].append(one_pass(log_store))
        ms["file"].append(one_pass(file_store))
    r4 = lambda x: round(x, 4)
    return dict(what="from_log", model=model_name, case=case, events=int(len(g["uid"])), lines=log_store.n_lines,
                batches=log_store.n_batches, same_first_batch=same, log_store_bytes=log_store.store_bytes(), file_store_bytes=file_bytes,
                build_device_s=round(build_s["device"], 4), build_host_s=round(build_s["host"], 4),
                files_write_s=round(write_s, 3), files_parse_upload_s=round(parse_s, 3),
                log_ms_per_batch=[r4(x) for x in ms["log"]], file_ms_per_batch=[r4(x) for x in ms["file"]],
                log_ms_median=r4(statistics.median(ms["log"])), file_ms_median=r4(statistics.median(ms["file"])),
                log_ms_spread=r4(max(ms["log"]) - min(ms["log"])), file_ms_spread=r4(max(ms["file"]) - min(ms["file"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--from-log", action="store_true", help="log store against file store: bytes, build time, ms per batch")
    ap.add_argument("--model", choices=tuple(DUAL))
    ap.add_argument("--case", choices=tuple(CASES))
    ap.add_argument("--pairs", type=int, default=3, help="alternating (host, device) passes per model and case")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_loader_time.jsonl"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per fresh process")
    ap.add_argument("--dir", help=argparse.SUPPRESS)          # (a child: the files are here)
    ap.add_argument("--what", choices=("loaders", "pass", "from_log"), help=argparse.SUPPRESS)
    ap.add_argument("--loader", choices=("host", "device"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.what == "from_log":
        print(json.dumps(dict(run_from_log(a.dir, a.model, a.case, a.pairs), **TMALL)), flush=True)
        return
    if a.what:
        r = run_loaders(a.dir, a.model, a.case) if a.what == "loaders" else run_pass(a.dir, a.model, a.case, a.loader, a.warmup)
        print(json.dumps(dict(r, **TMALL)), flush=True)
        return

    def child(*args):
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(x) for x in args], capture_output=True, text=True,
                           timeout=a.timeout)
        if p.returncode != 0:        # (nothing more is started on the GPU after a process that failed)
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit("%s: exit status %d" % (" ".join(str(x) for x in args), p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        return json.loads(line)
    if a.from_log:
        with tempfile.TemporaryDirectory() as root:
            for model_name, case in (("DEEMS", "eval1000"), ("GRU4Rec", "train200")):
                if (a.model and a.model != model_name) or (a.case and a.case != case):
                    continue
                d = os.path.join(root, case)
                os.makedirs(d)
                child("--what", "from_log", "--dir", d, "--model", model_name, "--case", case, "--pairs", a.pairs)
        return
    with tempfile.TemporaryDirectory() as root:
        for case in (a.case,) if a.case else tuple(CASES):
            d = os.path.join(root, case)
            os.makedirs(d)
            write_files(d, case)
            for model_name in (a.model,) if a.model else tuple(DUAL):
                common = ("--dir", d, "--model", model_name, "--case", case, "--warmup", a.warmup)
                child("--what", "loaders", *common)
                res = {"host": [], "device": []}
                for _ in range(a.pairs):
                    for loader in ("host", "device"):
                        res[loader].append(child("--what", "pass", "--loader", loader, *common)["ms_per_step"])
                print("%s %s: ms per step, host loader %s, device loader %s" % (model_name, case, res["host"], res["device"]), flush=True)


if __name__ == "__main__":
    main()
