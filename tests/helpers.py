"""Shared test helpers: golden loading, oracle config construction."""
import os
import subprocess
import sys

import numpy as np

from oracle import score_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The oracle is torch on the CPU, and the float32 results of torch's CPU kernels depend on the host: MKL picks its GEMM and
# vector-math code by CPU vendor and instruction set, so an Intel and an AMD host differ in the last bits of the same call.
# What the G1 / G3 goldens pin bit for bit is therefore computed -- by tests/golden/make_golden.py and by the tests that
# reproduce it -- in a process that fixes that choice before MKL's first call: MKL's conditional numerical reproducibility
# mode, one thread.  There TFAdam's square root is also the IEEE one its ApplyAdam restatement stands for (torch takes a
# float32 sqrt through MKL's vector math, which does not round it correctly on every host).
REPRODUCIBLE_ENV = {"MKL_CBWR": "COMPATIBLE", "MKL_NUM_THREADS": "1", "OMP_NUM_THREADS": "1"}


def reproducible_mode():
    """First thing in a process started with REPRODUCIBLE_ENV (run_reproducibly, tests/golden/make_golden.py)."""
    import torch
    assert all(os.environ.get(k) == v for k, v in REPRODUCIBLE_ENV.items()), "start the process with REPRODUCIBLE_ENV"
    torch.set_num_threads(1)
    torch.sqrt = lambda x: torch.from_numpy(np.sqrt(x.numpy()))       # (TFAdam's only torch.sqrt: IEEE, as ApplyAdam)


def run_reproducibly(code, timeout=600):
    """Run `code` in a fresh interpreter in reproducible_mode(), with tests/ and the repository on its path."""
    here = os.path.dirname(os.path.abspath(__file__))
    prelude = ("import sys\nsys.path[:0] = [%r, %r]\nimport helpers\nhelpers.reproducible_mode()\n"
               % (here, os.path.dirname(here)))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", prelude + code],
                         capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **REPRODUCIBLE_ENV))
    assert out.returncode == 0, out.stderr[-2000:]
NAMES = ("user_1hop", "user_2hop", "item_1hop", "item_2hop",
         "target_user", "target_item", "label", "length")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    N, D, H, T, K, Fu, Fi = [int(x) for x in z["cfg"]]
    cfg = so.Cfg(N, D, H, T, K, Fu, Fi, str(z["model_type"]))
    batch = {k[3:]: z[k] for k in z.files if k.startswith("in/") and k[3:] in NAMES}
    params = {k[6:]: z[k] for k in z.files if k.startswith("param/")}
    return cfg, params, batch, z


def batch_tuple(batch):
    return tuple(batch[n] for n in NAMES)


def random_batch(rng, cfg, B, zero_frac=0.2):
    c = cfg
    sh = {"user_1hop": (B, c.T, c.K, c.Fi), "user_2hop": (B, c.T, c.K, c.Fu),
          "item_1hop": (B, c.T, c.K, c.Fu), "item_2hop": (B, c.T, c.K, c.Fi),
          "target_user": (B, c.Fu), "target_item": (B, c.Fi)}
    b = {}
    for k, s in sh.items():
        a = rng.integers(1, c.N, s)
        if len(s) == 4:
            a[rng.random(s[:2]) < zero_frac] = 0
        b[k] = a.astype(np.int32)
    b["label"] = rng.integers(0, 2, (B,)).astype(np.int32)
    b["length"] = rng.integers(1, c.T + 1, (B,)).astype(np.int32)
    return b


def away_from_relu_kinks(cfg, params, batch, thr=1e-5, keep_prob=1.0, dropout_masks=None, max_dropped=None):
    """The batch without the samples that have a relu pre-activation within `thr` of the kink in the oracle's forward pass
    (co-attention scores, dense_3 / dense_4, fc1 / fc2: 10^5 units and more per batch).  A relu network's gradient is
    discontinuous there: two correct fp32 passes whose pre-activation of ONE unit differs in the last bit differ by that
    unit's whole gradient, so a comparison of gradients has to leave such units -- and what depends on them -- out.  Every
    unit belongs to one sample and nothing crosses the batch (oracle.forward "relu_margin_per_sample"), so what depends on a
    unit is its sample: dropping the sample drops exactly that, and the rest of the batch is compared on ARBITRARY inputs
    (no hand-picked seeds).  At most `max_dropped` samples may go (default: a quarter of the batch).
    Returns (batch, dropout_masks or None, indices kept)."""
    import torch
    with torch.no_grad():
        out = so.forward(cfg, so.to_torch_params(params), so.to_torch_batch(batch), keep_prob,
                         [torch.as_tensor(np.asarray(m)) for m in dropout_masks] if dropout_masks is not None else None, 0.0)
    per = np.asarray(out["relu_margin_per_sample"])
    keep = np.nonzero(per >= thr)[0]
    check_dropped(per.size, keep.size, max_dropped)
    b = {k: np.ascontiguousarray(np.asarray(v)[keep]) for k, v in batch.items()}
    dm = [np.ascontiguousarray(np.asarray(m)[keep]) for m in dropout_masks] if dropout_masks is not None else None
    return b, dm, keep


def check_dropped(n, kept, max_dropped=None):
    """The cap of the three away_from_relu_kinks helpers: at most `max_dropped` of the n samples may sit on a relu kink
    (None: a quarter of the batch), and one sample at least stays."""
    if max_dropped is None:
        assert kept >= max(1, (3 * n) // 4), "more than a quarter of the batch sits on a relu kink: %d of %d" % (n - kept, n)
    else:
        assert kept >= 1 and n - kept <= max_dropped, "%d of %d samples sit on a relu kink, at most %d may" % (n - kept, n, max_dropped)
