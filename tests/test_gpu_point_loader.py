"""The device-resident point loaders (score_amd/pointdata.py: PointSeqStore, DeviceDataLoaderUserSeq, DeviceDataLoaderDualSeq;
csrc/pointloader.hip) on the GPU.  The yardstick is always the host loaders DataLoaderUserSeq / DataLoaderDualSeq on the same
files -- themselves pinned to the reference's own output by the fixtures g7 / g8 (tests/test_gru4rec_cpu.py,
tests/test_delf_cpu.py) -- and every comparison is exact integer equality.

Caser refuses max_time_len < 50 (conv2d's kernel height), so no Caser exists for the fixtures' T <= 7: their active_slices are
compared under GRU4Rec (single form) and DELF / DEEMS (dual form), and Caser's under the synthetic T = 50 case."""
import os
import pickle

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from score_amd.pointdata import DataLoaderDualSeq, DataLoaderUserSeq, DeviceDataLoaderDualSeq, DeviceDataLoaderUserSeq

pytestmark = pytest.mark.gpu
TAGS = ("both", "nouser", "noitem", "none", "neg99")


def _write_case(z, tag, d, dual):
    """tests/test_gru4rec_cpu.py::_write_case / tests/test_delf_cpu.py::_write_case -> (B, L, neg, [paths as the loaders take them])"""
    os.makedirs(d)
    paths = []
    for key in (("target", "hist", "ihist") if dual else ("target", "hist")):
        p = os.path.join(d, key + ".txt")
        with open(p, "w") as f:
            f.write("".join(str(l) + "\n" for l in z["%s/%s" % (tag, key)]))
        paths.append(p)
    feats = []
    for nm in ("ufeat", "ifeat"):
        if "%s/%s_keys" % (tag, nm) in z.files:
            dct = {str(int(k)): [int(x) for x in row] for k, row in zip(z["%s/%s_keys" % (tag, nm)], z["%s/%s_rows" % (tag, nm)])}
            p = os.path.join(d, nm + ".pkl")
            with open(p, "wb") as f:
                pickle.dump(dct, f)
            feats.append(p)
        else:
            feats.append(None)
    B, L, neg = [int(x) for x in z[tag + "/cfg"]]
    return B, L, neg, paths, feats


def _host(dual, B, L, neg, paths, feats):
    return (DataLoaderDualSeq if dual else DataLoaderUserSeq)(B, L, *paths, neg, *feats)


def _device(dual, B, L, neg, paths, feats, **kw):
    return (DeviceDataLoaderDualSeq if dual else DeviceDataLoaderUserSeq)(B, L, *paths, neg, *feats, **kw)


def _synth(d, seed, n_lines, per_line, L, Fu, Fi, short_lines=0, id_base=1500000, n_ids=400):
    """seeded files: histories of 1 .. 3 L ids (the first `short_lines` lines and their item sequences below L), both
    dictionaries, ids above id_base, one extra target line (the partial batch) and two item sequences more than used"""
    rng = np.random.default_rng(seed)
    os.makedirs(d)
    users = id_base + 1 + np.arange(n_ids)
    items = id_base + 1 + n_ids + np.arange(n_ids)
    pick = lambda pool, lo, hi: ",".join(str(x) for x in rng.choice(pool, int(rng.integers(lo, hi + 1))))
    t, h, ih = [], [], []
    for l in range(n_lines + 1):
        hi = L - 1 if l < short_lines else 3 * L
        t.append("%d,%s" % (rng.choice(users), ",".join(str(x) for x in rng.choice(items, per_line))))
        h.append(pick(items, 1, hi))
        ih.append("\t".join(pick(users, 1, hi) for _ in range(per_line + 2)))
    paths = []
    for nm, lines in (("target", t), ("hist", h), ("ihist", ih)):
        paths.append(os.path.join(d, nm + ".txt"))
        with open(paths[-1], "w") as f:
            f.write("".join(x + "\n" for x in lines))
    feats = []
    for nm, pool, F in (("ufeat", users, Fu), ("ifeat", items, Fi)):
        feats.append(os.path.join(d, nm + ".pkl"))
        with open(feats[-1], "wb") as f:
            pickle.dump({str(int(k)): [int(x) for x in rng.integers(1, id_base, F - 1)] for k in pool}, f)
    return paths, feats


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """every g7 / g8 case: its files and the host loader's batches (computed once, never modified)"""
    root = str(tmp_path_factory.mktemp("point_loader"))
    out = {}
    for dual, name in ((False, "g7_point_loader.npz"), (True, "g8_dual_loader.npz")):
        z = np.load(os.path.join(GOLDEN, name))
        assert set(str(t) for t in z["tags"]) == set(TAGS)
        for tag in TAGS:
            B, L, neg, paths, feats = _write_case(z, tag, os.path.join(root, "%s_%d" % (tag, dual)), dual)
            host = list(_host(dual, B, L, neg, paths, feats))
            assert len(host) == int(z[tag + "/n_batches"]) > 0
            out[(dual, tag)] = (B, L, neg, paths, feats, host)
    return out


def _models(dual, N, T, Fu, Fi):
    from score_amd import model as M
    kinds = (M.DELF, M.DEEMS) if dual else ((M.GRU4Rec, M.Caser) if T >= M.Caser.CONV_L else (M.GRU4Rec,))
    return [k(N, 4, 16, T, Fu, Fi, seed=3) for k in kinds]


def _check_batches(dual, loader, host):
    """every batch of `loader`, copied back, against the host loader's tuples: the fields through __getitem__, the unused
    device tensors, the batch count; without a model active_slices is 0"""
    from score_amd.model import DeviceBatch
    n = 7 if dual else 5
    assert len(loader) == len(host)
    got = list(loader)
    assert len(got) == len(host)
    for i, (db, want) in enumerate(zip(got, host)):
        assert isinstance(db, DeviceBatch) and len(db) == n and db.B == len(want[-1]) and len(db.tensors) == (9 if dual else 8)
        for k in range(n):
            x = db[k]
            assert x.dtype == torch.int32 and tuple(x.shape) == want[k].shape, (i, k)
            assert np.array_equal(x.cpu().numpy(), want[k]), (i, k)
        for k in ((1, 3) if dual else (1, 2, 3)):
            assert not bool(db.tensors[k].any()), (i, k)
        assert db.active_slices == 0
    with pytest.raises(StopIteration):
        next(loader)
    return got


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("dual", [False, True])
def test_fixture_cases_equal_the_host_loader(cases, dual, tag):
    from score_amd.model import DeviceBatch
    B, L, neg, paths, feats, host = cases[(dual, tag)]
    first = _device(dual, B, L, neg, paths, feats)
    _check_batches(dual, first, host)
    first.close()
    Fu, Fi = host[0][-3].shape[1], host[0][-2].shape[1]
    for m in _models(dual, 64, L, Fu, Fi):           # (no step runs: the table's size does not matter)
        again = _device(dual, B, L, neg, paths, feats, model=m, store=first.store)
        assert again.store is first.store
        for db, want in zip(again, host):
            assert db.active_slices == DeviceBatch(m, want).active_slices, (type(m).__name__, tag)
    if tag != "both":
        return
    for T, fu, fi in ((L + 1, Fu, Fi), (L, Fu + 1, Fi), (L, Fu, Fi + 1)):       # a model of another shape is refused
        with pytest.raises(ValueError):
            _device(dual, B, L, neg, paths, feats, model=_models(dual, 64, T, fu, fi)[0], store=first.store)
    with pytest.raises(ValueError):                                             # and so is a model fed the other tuple
        _device(dual, B, L, neg, paths, feats, model=_models(not dual, 64, L, Fu, Fi)[0], store=first.store)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("point_synth"))
    # lines_per_batch 1 (B = per_line = 3) and 7 (B = 14); T = 50 with Fi = 4 (200-word spans: 16-byte aligned) and Fu = 3
    # (150-word spans: every second one is not); the first lines short, so that batches below T exist
    out = {}
    for name, B, neg, n_lines, short in (("one", 3, 2, 5, 2), ("seven", 14, 1, 21, 7)):
        paths, feats = _synth(os.path.join(root, name), 11, n_lines, 1 + neg, 50, 3, 4, short_lines=short)
        out[name] = (B, 50, neg, paths, feats)
    return out


@pytest.mark.parametrize("name", ["one", "seven"])
@pytest.mark.parametrize("dual", [False, True])
def test_synthetic_case_at_the_loop_edges(synth, dual, name):
    from score_amd.model import DeviceBatch
    B, L, neg, paths, feats = synth[name]
    paths = paths if dual else paths[:2]
    host = list(_host(dual, B, L, neg, paths, feats))
    assert len(host) == (6 if name == "one" else 3)         # (22 lines in batches of 7: the last one is dropped)
    assert min(int(b[0][..., 0].min()) for b in host) > 1500000 and host[0][0].shape == (B, 50, 4)
    lens = np.concatenate([b[1] for b in host] + ([b[3] for b in host] if dual else []))
    assert lens.min() >= 1 and (lens > L).any() and (lens < L).any()
    if dual:
        assert host[0][2].shape == (B, 50, 3) and any((b[3] > L).any() for b in host)
    first = _device(dual, B, L, neg, paths, feats)
    _check_batches(dual, first, host)
    seen = set()
    for m in _models(dual, 64, L, 3, 4):
        again = _device(dual, B, L, neg, paths, feats, model=m, store=first.store)
        for db, want in zip(again, host):
            assert db.active_slices == DeviceBatch(m, want).active_slices, type(m).__name__
            seen.add((type(m).__name__, db.active_slices > 0))
    # a batch below T and one at T for the models that read the lengths; all T always for Caser
    for kind in (("DELF", "DEEMS") if dual else ("GRU4Rec",)):
        assert (kind, True) in seen and (kind, False) in seen
    assert dual or ("Caser", True) not in seen


@pytest.mark.parametrize("dual", [False, True])
def test_a_second_loader_on_the_first_ones_store_yields_the_same_batches(cases, dual):
    B, L, neg, paths, feats, host = cases[(dual, "both")]
    first = _device(dual, B, L, neg, paths, feats)
    a = [db.flat.clone() for db in first]
    second = _device(dual, B, L, neg, [None] * len(paths), [None, None], store=first.store)      # (the files are not read again)
    assert second.store is first.store
    b = _check_batches(dual, second, host)
    # (whole flat buffers are not compared: the padding words between the tensors are not written)
    assert len(a) == len(b) == len(host)
    with pytest.raises(ValueError):
        _device(dual, B, L + 1, neg, paths, feats, store=first.store)


def _small_files(d, dual, T, B, neg, n_batches, N):
    """ids below N for a model that really steps: users 1 .. 59, items 60 .. 139, feature ids 140 .. N - 1"""
    rng = np.random.default_rng(5)
    os.makedirs(d)
    per = 1 + neg
    users, items = np.arange(1, 60), np.arange(60, 140)
    pick = lambda pool: ",".join(str(x) for x in rng.choice(pool, int(rng.integers(1, 2 * T))))
    n = n_batches * (B // per) + 1
    lines = {"target": ["%d,%s" % (rng.choice(users), ",".join(str(x) for x in rng.choice(items, per))) for _ in range(n)],
             "hist": [pick(items) for _ in range(n)], "ihist": ["\t".join(pick(users) for _ in range(per)) for _ in range(n)]}
    paths = []
    for nm in (("target", "hist", "ihist") if dual else ("target", "hist")):
        paths.append(os.path.join(d, nm + ".txt"))
        with open(paths[-1], "w") as f:
            f.write("".join(x + "\n" for x in lines[nm]))
    feats = []
    for nm, pool, F in (("ufeat", users, 2), ("ifeat", items, 3)):
        feats.append(os.path.join(d, nm + ".pkl"))
        with open(feats[-1], "wb") as f:
            pickle.dump({str(int(k)): [int(x) for x in rng.integers(140, N, F - 1)] for k in pool}, f)
    return paths, feats


@pytest.mark.parametrize("kind", ["GRU4Rec", "DEEMS"])
def test_training_from_the_device_loader_is_bit_identical_to_training_from_the_host_loader(tmp_path, kind):
    from score_amd import model as M
    dual = kind == "DEEMS"
    N, T, B, neg = 200, 6, 8, 1
    paths, feats = _small_files(str(tmp_path / "f"), dual, T, B, neg, 3, N)
    host = list(_host(dual, B, T, neg, paths, feats))
    assert len(host) == 3
    runs = []
    for fed in ("device", "host"):
        m = M.MODELS[kind](N, 4, 16, T, 2, 3, seed=7)
        batches = _device(dual, B, T, neg, paths, feats, model=m) if fed == "device" else host
        losses = [m.train(None, b, 1e-2, 1e-4) for b in batches]
        assert len(losses) == 3
        torch.cuda.synchronize()
        runs.append((np.asarray(losses, dtype=np.float64), m.get_params()))
    (la, pa), (lb, pb) = runs
    print("losses device-fed", la.tolist(), "host-fed", lb.tolist())
    assert np.isfinite(la).all() and np.array_equal(la, lb)
    assert sorted(pa) == sorted(pb)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


def test_evaluate_device_over_both_loaders(cases):
    from score_amd import harness
    from score_amd import model as M
    B, L, neg, paths, feats, host = cases[(False, "neg99")]
    assert neg == 99
    N = 1 + max(int(x.max()) for b in host for x in (b[0], b[2], b[3]))
    m = M.GRU4Rec(N, 4, 16, L, host[0][2].shape[1], host[0][3].shape[1], seed=5)
    want = harness.evaluate_device(m, host, 1e-4, neg_sample_num=neg)
    got = harness.evaluate_device(m, _device(False, B, L, neg, paths, feats, model=m), 1e-4, neg_sample_num=neg)
    print("evaluate_device host-fed", want, "device-fed", got)
    assert len(got) == 9 and got == want
    # harness.evaluate (the host-side metrics) takes the loader as it is, too
    assert harness.evaluate(m, _device(False, B, L, neg, paths, feats), 1e-4, neg_sample_num=neg) == \
        harness.evaluate(m, host, 1e-4, neg_sample_num=neg)


def test_train_loop_takes_the_device_loaders_unchanged(tmp_path):
    """harness.train_loop (feed-ahead thread, next_batch look-ahead, evaluate_device per validation pass) over device loaders
    that share one store per file set, against the same loop over the host loaders: the same curves, the same variables"""
    from score_amd import harness
    from score_amd import model as M
    N, T, B, neg = 200, 6, 8, 1
    paths, feats = _small_files(str(tmp_path / "f"), False, T, B, neg, 4, N)
    runs = []
    for fed in ("device", "host"):
        m = M.GRU4Rec(N, 4, 16, T, 2, 3, seed=7)
        if fed == "device":
            store = _device(False, B, T, neg, paths, feats, model=m).store
            make = lambda: _device(False, B, T, neg, paths, feats, model=m, store=store)
        else:
            make = lambda: _host(False, B, T, neg, paths, feats)
        curves = harness.train_loop(m, make, make, 1e-2, 1e-4, B, 24, epochs=2, neg_sample_num=neg, log=lambda *a: None)
        runs.append((curves, m.get_params()))
    (ca, pa), (cb, pb) = runs
    assert ca["steps"] >= 4 and len(ca["vali_mrrs"]) >= 3 and ca == cb
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
