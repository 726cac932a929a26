"""PointSeqStore (score_amd/pointdata.py) without a GPU: the store's host arrays, cut into batches by a few lines of numpy
here, against the batches the reference's own loaders produced (tests/golden/g7_point_loader.npz, g8_dual_loader.npz); its
per-batch length extremes against the host loaders'; the exception types of malformed input; the store / loader consistency
check; and that a device loader refuses to exist without a device while the store does not."""
import os
import pickle

import numpy as np
import pytest
import torch

import delf_ref as dr
import gru4rec_ref as gr
from helpers import GOLDEN
from score_amd.pointdata import (DataLoaderDualSeq, DataLoaderUserSeq, DeviceDataLoaderDualSeq, DeviceDataLoaderUserSeq,
                                 PointSeqStore)


def _write_case(z, tag, d, dual):
    """tests/test_gru4rec_cpu.py::_write_case / tests/test_delf_cpu.py::_write_case: the case's files as the fixture holds them.
    -> (target, hist, ihist or None, ufeat or None, ifeat or None)"""
    names = ("target", "hist", "ihist") if dual else ("target", "hist")
    out = []
    for key in names:
        p = os.path.join(str(d), key + ".txt")
        with open(p, "w") as f:
            f.write("".join(str(l) + "\n" for l in z["%s/%s" % (tag, key)]))
        out.append(p)
    if not dual:
        out.append(None)
    for nm in ("ufeat", "ifeat"):
        if "%s/%s_keys" % (tag, nm) in z.files:
            dct = {str(int(k)): [int(x) for x in row] for k, row in zip(z["%s/%s_keys" % (tag, nm)], z["%s/%s_rows" % (tag, nm)])}
            p = os.path.join(str(d), nm + ".pkl")
            with open(p, "wb") as f:
                pickle.dump(dct, f)
            out.append(p)
        else:
            out.append(None)
    return out


def _history(off, seq, rows, h, L):
    r = seq[off[h]:off[h + 1]][-L:]                                     # the last max_len ids ...
    r = np.concatenate([r, np.repeat(r[-1:], L - len(r))])              # ... the last one repeated
    return rows[r]


def rebuild_batch(st, b):
    """batch b of the store as the host loaders' tuple (5 fields, or 7 for a dual store)"""
    L, per, lpb = st.max_len, st.per_line, st.lines_per_batch
    lines = np.repeat(np.arange(b * lpb, (b + 1) * lpb), per)
    samples = np.arange(b * lpb * per, (b + 1) * lpb * per)
    useq = np.stack([_history(st.user_off, st.user_seq, st.item_rows, l, L) for l in lines])
    out = [useq, st.user_len[lines]]
    if st.dual:
        out += [np.stack([_history(st.item_off, st.item_seq, st.user_rows, s, L) for s in samples]), st.item_len[samples]]
    out += [st.user_rows[st.target_user[lines]], st.item_rows[st.target_item[samples]],
            (samples % per == 0).astype(np.int32)]
    return tuple(out)


@pytest.mark.parametrize("dual", [False, True])
def test_store_rebuilds_the_reference_loaders_batches(tmp_path, dual):
    z = np.load(os.path.join(GOLDEN, "g8_dual_loader.npz" if dual else "g7_point_loader.npz"))
    feed = dr.FEED if dual else gr.FEED
    tags = [str(t) for t in z["tags"]]
    assert set(tags) == {"both", "nouser", "noitem", "none", "neg99"}
    for tag in tags:
        d = tmp_path / tag
        d.mkdir()
        B, L, neg = [int(x) for x in z[tag + "/cfg"]]
        tf, hf, ihf, uf, itf = _write_case(z, tag, d, dual)
        st = PointSeqStore(tf, hf, ihf, L, neg, B, uf, itf)
        assert st.dual == dual and st.n_batches == int(z[tag + "/n_batches"]) > 0, tag
        assert st.n_lines == st.n_batches * (B // (1 + neg)) < len(z[tag + "/target"])          # the partial batch is dropped
        assert (np.diff(st.user_off) <= L).all() and (np.diff(st.user_off) >= 1).all()          # only the last max_len are kept
        host = DataLoaderDualSeq(B, L, tf, hf, ihf, neg, uf, itf) if dual else DataLoaderUserSeq(B, L, tf, hf, neg, uf, itf)
        host = list(host)
        assert len(host) == st.n_batches
        for i in range(st.n_batches):
            got = rebuild_batch(st, i)
            assert len(got) == len(feed)
            for nm, x in zip(feed, got):
                want = z["%s/b%d/%s" % (tag, i, nm)]
                assert x.dtype == np.int32 and x.shape == want.shape, (tag, i, nm)
                assert np.array_equal(x, want), (tag, i, nm)
            lens = [host[i][1]] + ([host[i][3]] if dual else [])
            assert int(st.batch_max_user_len[i]) == int(host[i][1].max()), (tag, i)
            assert int(st.batch_max_len[i]) == max(int(x.max()) for x in lens), (tag, i)
            assert int(st.batch_min_len[i]) == min(int(x.min()) for x in lens), (tag, i)
        # compacted tables: one row per key that occurs, the id in column 0
        assert len(np.unique(st.item_rows[:, 0])) == len(st.item_rows) and len(np.unique(st.user_rows[:, 0])) == len(st.user_rows)


def _files(d, target, hist, ihist=None, ufeat=None, ifeat=None):
    out = []
    for nm, txt in (("t", target), ("h", hist), ("i", ihist)):
        if txt is None:
            out.append(None)
            continue
        (d / nm).write_text(txt)
        out.append(str(d / nm))
    for nm, dct in (("u.pkl", ufeat), ("it.pkl", ifeat)):
        if dct is None:
            out.append(None)
            continue
        with open(str(d / nm), "wb") as f:
            pickle.dump(dct, f)
        out.append(str(d / nm))
    return out


def _both_raise(exc, B, L, neg, tf, hf, ihf, uf, itf):
    """the store raises at construction what the host loader raises when it reaches that batch"""
    with pytest.raises(exc):
        list(DataLoaderDualSeq(B, L, tf, hf, ihf, neg, uf, itf) if ihf else DataLoaderUserSeq(B, L, tf, hf, neg, uf, itf))
    with pytest.raises(exc):
        PointSeqStore(tf, hf, ihf, L, neg, B, uf, itf)


def test_malformed_input_raises_what_the_host_loader_raises(tmp_path):
    def d(name):
        p = tmp_path / name
        p.mkdir()
        return p
    # batch size no multiple of 1 + neg
    tf, hf, ihf, uf, itf = _files(d("a"), "1,2,3\n", "4,5\n")
    with pytest.raises(ValueError):
        PointSeqStore(tf, hf, None, 4, 1, 5)
    # an empty history line; a history file shorter than the target file
    _both_raise(ValueError, 2, 4, 1, *_files(d("b"), "1,2,3\n1,2,3\n", "4,5\n\n"))
    _both_raise(ValueError, 2, 4, 1, *_files(d("c"), "1,2,3\n1,2,3\n", "4,5\n"))
    # the item side: an empty sequence, a file that is too short, fewer sequences than 1 + neg
    _both_raise(ValueError, 2, 4, 1, *_files(d("e"), "1,2,3\n", "4,5\n", "6\t\n"))
    _both_raise(ValueError, 2, 4, 1, *_files(d("f"), "1,2,3\n1,2,3\n", "4,5\n4\n", "6\t7\n"))
    _both_raise(IndexError, 2, 4, 1, *_files(d("g"), "1,2,3\n", "4,5\n", "6,7\n"))
    # ids missing from a dictionary: a history id, a target item, the user; and in the dual form a user of an item sequence
    items = {"2": [9], "3": [9], "4": [9], "5": [9]}
    users = {"1": [8, 8], "6": [8, 8], "7": [8, 8]}
    _both_raise(KeyError, 2, 4, 1, *_files(d("h"), "1,2,3\n", "4,55\n", None, users, items))
    _both_raise(KeyError, 2, 4, 1, *_files(d("j"), "1,2,33\n", "4,5\n", None, users, items))
    _both_raise(KeyError, 2, 4, 1, *_files(d("k"), "11,2,3\n", "4,5\n", None, users, items))
    _both_raise(KeyError, 2, 4, 1, *_files(d("l"), "1,2,3\n", "4,5\n", "6,77\t7\n", users, items))
    # the file's tail is never looked at: a malformed line behind the last whole batch raises nothing
    tf, hf, ihf, uf, itf = _files(d("m"), "1,2,3\n1,2,3\n1,x,y\n", "4,5\n4\n\n", None, users, items)
    st = PointSeqStore(tf, hf, None, 4, 1, 4, uf, itf)
    assert st.n_batches == 1 and st.n_lines == 2
    for x, w in zip(rebuild_batch(st, 0), next(DataLoaderUserSeq(4, 4, tf, hf, 1, uf, itf))):
        assert np.array_equal(x, w)
    # habits: the last character of a line is dropped unseen, only the first 1 + neg items are used, ids are normalised
    tf, hf, ihf, uf, itf = _files(d("n"), "1,2,3,99,98\n1,2,37", "04,5\n4,51", None, users, items)
    st = PointSeqStore(tf, hf, None, 4, 1, 4, uf, itf)
    (want,) = list(DataLoaderUserSeq(4, 4, tf, hf, 1, uf, itf))
    for x, w in zip(rebuild_batch(st, 0), want):
        assert np.array_equal(x, w)
    assert st.item_rows[st.user_seq, 0].tolist() == [4, 5, 4, 5] and st.item_rows[st.target_item, 0].tolist() == [2, 3, 2, 3]


def test_dual_store_keeps_the_rebinding_and_all_sequences_of_a_line(tmp_path):
    tf, hf, ihf, uf, itf = _files(tmp_path, "1,2,3\n", "1,2,3\n", "4,5\t6\t7,8\n")
    st = PointSeqStore(tf, hf, ihf, 4, 1, 2)
    (want,) = list(DataLoaderDualSeq(2, 4, tf, hf, ihf, 1, None, None))
    for x, w in zip(rebuild_batch(st, 0), want):
        assert np.array_equal(x, w)
    assert st.user_rows[st.target_user, 0].tolist() == [8]           # the last id of the line's LAST sequence, used or not
    assert st.item_len.tolist() == [2, 1]


def test_store_refuses_a_loader_built_with_other_arguments(tmp_path):
    tf, hf, ihf, uf, itf = _files(tmp_path, "1,2,3\n1,2,3\n", "4,5\n4,5,6\n", "6\t7\n6,7\t8\n")
    st = PointSeqStore(tf, hf, None, 4, 1, 2)
    dual = PointSeqStore(tf, hf, ihf, 4, 1, 2)
    for B, L, neg in ((4, 4, 1), (2, 5, 1), (2, 4, 0)):
        with pytest.raises(ValueError):
            DeviceDataLoaderUserSeq(B, L, tf, hf, neg, None, None, store=st)
        with pytest.raises(ValueError):
            DeviceDataLoaderDualSeq(B, L, tf, hf, ihf, neg, None, None, store=dual)
    with pytest.raises(ValueError):                                   # a single-form store under the dual loader, and back
        DeviceDataLoaderDualSeq(2, 4, tf, hf, ihf, 1, None, None, store=st)
    with pytest.raises(ValueError):
        DeviceDataLoaderUserSeq(2, 4, tf, hf, 1, None, None, store=dual)
    with pytest.raises(ValueError):                                   # (the loaders' own check, before any store)
        DeviceDataLoaderUserSeq(5, 4, tf, hf, 1, None, None)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                             # the matching arguments get as far as the device
            DeviceDataLoaderUserSeq(2, 4, tf, hf, 1, None, None, store=st)
        with pytest.raises(RuntimeError):
            DeviceDataLoaderDualSeq(2, 4, tf, hf, ihf, 1, None, None)
        with pytest.raises(RuntimeError):
            st.to_device()


def test_abi_entry_and_struct():
    import ctypes as C
    from score_amd import _lib
    lib = _lib.load()
    assert "score_point_batch_assemble" in _lib.EXPORTS and hasattr(lib, "score_point_batch_assemble")
    assert C.sizeof(_lib.PointStore) == 8 + 10 * 8 + 3 * 8 + 2 * 4
    # the struct's own size check, and the argument checks in front of the launch (host only: nothing is launched)
    st = _lib.PointStore()
    out = _lib.BatchOut()
    assert lib.score_point_batch_assemble(C.byref(st), 0, 1, 2, 4, 1, 1, C.byref(out), None, None) == -1
    st.struct_bytes = C.sizeof(_lib.PointStore)
    assert lib.score_point_batch_assemble(C.byref(st), 0, 1, 2, 4, 1, 1, C.byref(out), None, None) == -1
