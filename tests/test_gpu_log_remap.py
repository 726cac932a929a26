"""The raw log's remap ON THE DEVICE (csrc/logremap.hip: score_log_remap, score_log_slices, score_log_compact;
dataprep.remap_tmall_log / remap_taobao_log(build="device"), tmall_pipeline(remap="device")) against the host build --
itself pinned to a plain-Python restatement and to the reference's own code in test_log_remap_cpu.py.  Exact integers; the
outputs are poisoned first, with pad words behind them, and every build gets a fresh poisoned workspace."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import remap_cases as rc
from score_amd import _lib
from score_amd import dataprep as dp

pytestmark = pytest.mark.gpu
POISON = -0x5A5A5A5B
E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
PAD = 3                                            # poisoned words / rows behind the last: nothing may be written there


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def host_remap(cols, tables=()):
    """the host build's rule on raw columns (dataprep._first_appearance, bases chained from 1; later rows overwrite)"""
    base, ids, counts = 1, [], []
    for c in cols:
        r, k = dp._first_appearance(np.asarray(c).astype(np.int64))
        ids.append((r + base).astype(np.int32))
        counts.append(k)
        base += k
    rows = []
    for ent, feats in tables:
        t = np.zeros((counts[ent], 1 + len(feats)), dtype=np.int32)
        t[ids[ent] - (1 + sum(counts[:ent]))] = np.stack([ids[ent]] + [ids[f] for f in feats], axis=1)
        rows.append(t)
    return ids, counts, rows


@functools.lru_cache(maxsize=None)
def host_case(n, key_bits, n_cols, tables):
    ids, counts, rows = host_remap(rc.raw_columns(n, key_bits, n_cols), tables)
    for a in ids + rows:
        a.setflags(write=False)
    return ids, counts, rows


class Remap(object):
    """one device remap through the C ABI into poisoned outputs"""

    def __init__(self, cols, key_bits, tables=(), temp_short=0):
        self.lib, self.dev = _lib.load(), torch.device("cuda")
        self.n, self.k, self.tables = len(cols[0]) if len(cols) else 0, len(cols), tables
        n = max(self.n, 1)
        self.cols = [up(c) if len(c) else torch.zeros((1,), dtype=torch.int32, device=self.dev) for c in cols]
        self.ids = [torch.full((n + PAD,), POISON, dtype=torch.int32, device=self.dev) for _ in cols]
        need = int(self.lib.score_log_remap_temp_bytes(n, min(max(self.k, 1), 8)))
        assert need > 0
        self.temp = torch.full((need,), 0x5A, dtype=torch.uint8, device=self.dev)
        self.temp_bytes = need - temp_short
        a = self.args = _lib.LogRemap()
        a.struct_bytes, a.n_events, a.n_cols, a.key_bits, a.n_tables = C.sizeof(_lib.LogRemap), self.n, self.k, key_bits, len(tables)
        for c in range(min(self.k, 8)):
            a.cols[c], a.ids[c] = self.cols[c].data_ptr(), self.ids[c].data_ptr()
        for t, (ent, feats) in enumerate(tables):
            a.tables[t].entity, a.tables[t].n_feat = ent, len(feats)
            for j, f in enumerate(feats):
                a.tables[t].feat[j] = f
        self.widths = [1 + len(f) for _, f in tables]
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.counts = (C.c_int64 * 8)(*([-77] * 8))
        self.out([4] * len(tables))

    def out(self, n_rows):
        # (4 * r * w words: a multiple of 16 bytes, so the widths 4 and 8 take the 16-byte stores)
        self.rows = [torch.full(((r + PAD) * w,), POISON, dtype=torch.int32, device=self.dev) for r, w in zip(n_rows, self.widths)]

    def count(self):
        return self.lib.score_log_remap(C.byref(self.args), None, None, self.counts, self.temp.data_ptr(), self.temp_bytes,
                                        self.stream)

    def fill(self, caps):
        ptrs = (C.c_void_p * max(len(self.rows), 1))(*[r.data_ptr() for r in self.rows])
        caps = (C.c_int64 * max(len(self.rows), 1))(*caps)
        return self.lib.score_log_remap(C.byref(self.args), ptrs, caps, None, self.temp.data_ptr(), self.temp_bytes, self.stream)

    def run(self, cap_short=0):
        assert self.count() == 0
        got = [int(self.counts[e]) for e, _ in self.tables]
        self.out(got)
        if self.tables and min(got) - cap_short > 0:
            assert self.fill([g - cap_short for g in got]) == 0
        torch.cuda.synchronize()
        return self

    def rows_poison(self):
        torch.cuda.synchronize()
        return all(bool((r == POISON).all()) for r in self.rows)

    def all_poison(self):
        return self.rows_poison() and all(bool((i == POISON).all()) for i in self.ids) and list(self.counts) == [-77] * 8


def assert_equals_host(b, want, written=None):
    ids, counts, rows = want
    assert [int(x) for x in b.counts][:b.k] == list(counts) and list(b.counts)[b.k:] == [-77] * (8 - b.k)
    for c in range(b.k):
        got = b.ids[c].cpu().numpy()
        assert np.array_equal(got[:b.n], ids[c]) and (got[b.n:] == POISON).all(), c
    for t, (w, r) in enumerate(zip(b.widths, rows)):
        got = b.rows[t].cpu().numpy().reshape(-1, w)
        m = len(r) if written is None else written[t]
        assert len(got) == len(r) + PAD and np.array_equal(got[:m], r[:m]) and (got[m:] == POISON).all(), t


TABLES3 = ((0, (1, 2)), (1, (2,)))


@pytest.mark.parametrize("n", rc.EVENT_COUNTS)
def test_event_counts_at_the_sort_tile_and_scan_chunk_edges(n):
    cols = rc.raw_columns(n, 32, 3)
    assert cols[0][0] == -1 and (n == 1 or cols[0][n - 1] == rc.INT32_MIN)
    assert_equals_host(Remap(cols, 32, TABLES3).run(), host_case(n, 32, 3, TABLES3))


@pytest.mark.parametrize("key_bits", rc.KEY_BITS)
def test_key_widths_at_the_sorts_pass_edges(key_bits):
    n = rc.SORT_TILE + 5
    cols = rc.raw_columns(n, key_bits, 3)
    widest = max(int(c.view(np.uint32).max()) for c in cols)
    assert widest.bit_length() == key_bits and (key_bits < 32 or (cols[0] == rc.INT32_MIN).any())
    assert_equals_host(Remap(cols, key_bits, TABLES3).run(), host_case(n, key_bits, 3, TABLES3))
    if key_bits > 1:                               # one bit too few declared: found on the device, reported after the wait
        b = Remap(cols, key_bits - 1, TABLES3)
        assert b.count() == E_BADARG and b.rows_poison() and list(b.counts) == [-77] * 8
    else:
        b = Remap((np.asarray([0, 1, 2, 1], dtype=np.int32),), 1, ((0, ()),))
        assert b.count() == E_BADARG and b.rows_poison() and list(b.counts) == [-77] * 8


def test_dict_rule_and_host_rule_agree_on_a_case():
    """the yardstick of this file (dataprep._first_appearance) against the plain dict rule, on negative patterns too"""
    cols = rc.raw_columns(rc.SCAN_TILE + 1, 32, 3)
    ids, counts, rows = host_case(rc.SCAN_TILE + 1, 32, 3, TABLES3)
    dids, dcounts = rc.first_appearance_ids(cols)
    assert list(counts) == dcounts and all(np.array_equal(a, b) for a, b in zip(ids, dids))
    assert np.array_equal(rows[0], rc.last_rows(dids, dcounts, 0, (1, 2))) and np.array_equal(rows[1], rc.last_rows(dids, dcounts, 1, (2,)))


def test_degenerate_vocabularies():
    n = rc.SCAN_TILE + 1
    equal = np.full(n, -7, dtype=np.int32)
    distinct = (np.arange(n, dtype=np.int64)[::-1] * 2654435761 % (1 << 32)).astype(np.uint32).view(np.int32)
    assert len(set(distinct.tolist())) == n
    late = np.full(n, 5, dtype=np.int32)
    late[n - 1] = 3                                # a value whose first appearance is the last event
    cols = (equal, distinct, late)
    tables = ((1, (0, 2)), (2, (1,)))
    b = Remap(cols, 32, tables).run()
    assert_equals_host(b, host_remap(cols, tables))
    assert [int(x) for x in b.counts][:3] == [1, n, 2]
    ids = [i.cpu().numpy()[:n] for i in b.ids]
    assert (ids[0] == 1).all() and np.array_equal(ids[1], np.arange(2, n + 2)) and ids[2][n - 1] == n + 3 and (ids[2][:n - 1] == n + 2).all()


@pytest.mark.parametrize("n_cols", [8, 1])
def test_columns_are_chained_on_the_device_with_one_host_wait(n_cols):
    n = rc.SORT_TILE + 1
    cols = rc.raw_columns(n, 25, n_cols)
    tables = ((0, tuple(range(1, 8))), (7, ())) if n_cols == 8 else ((0, ()),)
    b = Remap(cols, 25, tables)
    lib = b.lib
    torch.cuda.synchronize()
    w0 = lib.score_log_host_waits()
    assert b.count() == 0
    w1 = lib.score_log_host_waits()
    got = [int(b.counts[e]) for e, _ in tables]
    b.out(got)
    assert b.fill(got) == 0
    w2 = lib.score_log_host_waits()
    torch.cuda.synchronize()
    assert (w1 - w0, w2 - w1) == (1, 0)            # the counts of ALL columns in one wait; the fill waits for nothing
    want = host_remap(cols, tables)
    assert_equals_host(b, want)                    # (ids, so every column's base, and the counts)
    assert len(set(want[1])) >= min(n_cols, 5)     # vocabularies of different sizes


def _rows_case():
    """entity column 0: value 7 occurs first, in the middle and last, with different features each time; width-1 and width-8
    tables"""
    n = 600
    rng = np.random.Generator(np.random.PCG64(3))
    cols = [rng.integers(0, 40, n).astype(np.int32)] + [rng.integers(0, 5 + 3 * j, n).astype(np.int32) for j in range(7)]
    for p, v in ((0, 100), (300, 200), (n - 1, 300)):
        cols[0][p] = 7
        for j in range(1, 8):
            cols[j][p] = v + j
    cols[0][1:300][cols[0][1:300] == 7] = 8
    cols[0][301:n - 1][cols[0][301:n - 1] == 7] = 8
    return tuple(cols)


def test_feature_rows_take_the_last_event_at_width_1_and_8():
    cols = _rows_case()
    tables = ((0, tuple(range(1, 8))), (3, ()))
    b = Remap(cols, 9, tables)
    assert b.count() == 0 and b.rows_poison()      # rows == NULL: the row buffers stay as they were
    want = host_remap(cols, tables)
    b = Remap(cols, 9, tables).run()
    assert_equals_host(b, want)
    ids = want[0]
    row = b.rows[0].cpu().numpy().reshape(-1, 8)[0]                # value 7 appears first: row 0
    assert row.tolist() == [1] + [int(ids[j][599]) for j in range(1, 8)]
    assert row.tolist() != [1] + [int(ids[j][0]) for j in range(1, 8)] and row.tolist() != [1] + [int(ids[j][300]) for j in range(1, 8)]
    assert b.rows[0].data_ptr() % 16 == 0 and b.rows[1].shape[0] == (want[1][3] + PAD)
    # width 4 (the item rows' width) from an odd word offset: the stores fall back to single words
    t4 = ((0, (1, 2, 3)),)
    b = Remap(cols, 9, t4)
    assert b.count() == 0
    k = int(b.counts[0])
    buf = torch.full((1 + (k + PAD) * 4,), POISON, dtype=torch.int32, device="cuda")
    b.rows = [buf[1:]]
    assert b.rows[0].data_ptr() % 16 == 4 and b.fill([k]) == 0
    torch.cuda.synchronize()
    assert_equals_host(b, host_remap(cols, t4))
    assert int(buf[0]) == POISON


@pytest.mark.parametrize("tables", [((0, tuple(range(1, 8))), (3, ())), ((1, (2, 3, 4)), (0, (5,)))])
def test_a_cap_one_row_short_leaves_the_last_row_alone(tables):
    cols = _rows_case()
    want = host_remap(cols, tables)
    b = Remap(cols, 9, tables).run(cap_short=1)
    assert_equals_host(b, want, written=[len(r) - 1 for r in want[2]])


def test_two_remaps_share_nothing():
    """a second remap in a workspace the first one used (no clearing in between) gives its own ids and rows"""
    n = rc.SORT_TILE + 5
    a = Remap(rc.raw_columns(n, 24, 3), 24, TABLES3).run()
    b = Remap(rc.raw_columns(n, 13, 3), 13, TABLES3)
    b.temp[:] = a.temp
    assert_equals_host(b.run(), host_case(n, 13, 3, TABLES3))


def test_abi_errors_are_refused_before_any_launch():
    cols = rc.raw_columns(100, 12, 3)
    b = Remap(cols, 12, TABLES3, temp_short=1)
    assert b.count() == E_WORKSPACE and b.fill([4, 4]) == E_WORKSPACE and b.all_poison()
    b = Remap(cols, 12, TABLES3)
    b.args.struct_bytes -= 8
    assert b.count() == E_BADARG and b.fill([4, 4]) == E_BADARG and b.all_poison()
    for k in (0, 9):
        b = Remap(cols, 12, TABLES3)
        b.args.n_cols = k
        assert b.count() == E_BADARG and b.fill([4, 4]) == E_BADARG and b.all_poison(), k
    b = Remap(cols, 12, TABLES3)
    b.args.n_events = 0
    assert b.count() == E_BADARG and b.fill([4, 4]) == E_BADARG and b.all_poison()
    for kb in (0, 33):
        b = Remap(cols, kb, TABLES3)
        assert b.count() == E_BADARG and b.all_poison(), kb
    b = Remap(cols, 12, ((3, ()),))                # a table's entity outside the columns
    assert b.count() == E_BADARG and b.all_poison()
    b = Remap(cols, 12, ((0, (1, 5)),))            # a feature column outside the columns
    assert b.count() == E_BADARG and b.all_poison()
    b = Remap(cols, 12, TABLES3)
    assert b.fill([4, 0]) == E_BADARG and b.all_poison()
    lib = _lib.load()
    assert lib.score_log_remap_temp_bytes(2 ** 31, 3) == -1 and lib.score_log_remap_temp_bytes(0, 3) == -1
    assert lib.score_log_remap_temp_bytes(10, 9) == -1 and lib.score_log_compact_temp_bytes(2 ** 31) == -1


# ---- slices ---------------------------------------------------------------------------------------------------------------
def _slices_tmall(mmdd):
    lib = _lib.load()
    n = len(mmdd)
    t = torch.full((n + PAD,), POISON, dtype=torch.int32, device="cuda")
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    d = up(mmdd)
    rc_ = lib.score_log_slices(_lib.LOG_SLICES_TMALL, d.data_ptr(), None, n, 0, 0, 0, t.data_ptr(), None, status.data_ptr(),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc_, t.cpu().numpy(), int(status[0])


def test_tmall_slices_on_every_date_of_2015():
    v = rc.valid_dates_2015()
    want = dp.tmall_slice_index(v)
    rc_, got, status = _slices_tmall(v)
    assert rc_ == 0 and status == 0 and np.array_equal(got[:365], want) and (got[365:] == POISON).all()
    assert want[v < 501].max() == -1 and want[v == 430][0] == -1 and want[v == 101][0] == -8 and got[v.tolist().index(501)] == 0
    log = np.array(rc.tmall_sample()[:50])
    for bad in rc.INVALID_DATES + (-501, 1232, 100, 632):
        rc_, _, status = _slices_tmall(np.asarray([501, bad, 1231]))
        assert rc_ == 0 and status == 1, bad
    for bad in rc.INVALID_DATES:
        log[17, 5] = bad
        with pytest.raises(ValueError, match="MMDD"):
            dp.remap_tmall_log(log, build="device")
        with pytest.raises(ValueError):
            dp.remap_tmall_log(log)
    lib = _lib.load()
    t = torch.zeros((4,), dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.score_log_slices(_lib.LOG_SLICES_TMALL, t.data_ptr(), None, 4, 0, 0, 0, t.data_ptr(), None, None, s) == E_BADARG
    assert lib.score_log_slices(_lib.LOG_SLICES_EPOCH, t.data_ptr(), None, 4, 0, 9, 0, t.data_ptr(), t.data_ptr(), None, s) == E_BADARG
    assert lib.score_log_slices(2, t.data_ptr(), None, 4, 0, 9, 1, t.data_ptr(), t.data_ptr(), t.data_ptr(), s) == E_BADARG
    assert lib.score_log_slices(_lib.LOG_SLICES_EPOCH, t.data_ptr(), None, 0, 0, 9, 1, t.data_ptr(), t.data_ptr(), None, s) == E_BADARG


def _epoch_and_compact(log, start, end, delta):
    """score_log_slices(epoch) and score_log_compact through the C ABI into poisoned outputs -> (keep, t_idx, compacted
    [user, item, category, t_idx], kept, n_kept, waits)"""
    lib = _lib.load()
    n = len(log)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cols = [up(log[:, j]) for j in range(5)]
    t_idx = torch.full((n + PAD,), POISON, dtype=torch.int32, device="cuda")
    keep = torch.full((n + PAD,), POISON, dtype=torch.int32, device="cuda")
    assert lib.score_log_slices(_lib.LOG_SLICES_EPOCH, cols[4].data_ptr(), cols[3].data_ptr(), n, start, end, delta,
                                t_idx.data_ptr(), keep.data_ptr(), None, s) == 0
    need = int(lib.score_log_compact_temp_bytes(n))
    temp = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    out = [torch.full((n + PAD,), POISON, dtype=torch.int32, device="cuda") for _ in range(5)]
    cin = (C.c_void_p * 4)(*[c.data_ptr() for c in (cols[0], cols[1], cols[2], t_idx)])
    cout = (C.c_void_p * 4)(*[o.data_ptr() for o in out[:4]])
    n_kept = C.c_int64(-77)
    assert lib.score_log_compact(cin, cout, 4, keep.data_ptr(), n, out[4].data_ptr(), n, C.byref(n_kept), temp.data_ptr(),
                                 need - 1, s) == E_WORKSPACE and n_kept.value == -77
    w0 = lib.score_log_host_waits()
    assert lib.score_log_compact(cin, cout, 4, keep.data_ptr(), n, out[4].data_ptr(), n, C.byref(n_kept), temp.data_ptr(),
                                 need, s) == 0
    waits = lib.score_log_host_waits() - w0
    torch.cuda.synchronize()
    return keep.cpu().numpy(), t_idx.cpu().numpy(), [o.cpu().numpy() for o in out[:4]], out[4].cpu().numpy(), int(n_kept.value), waits


def _check_taobao(log, start, end, delta):
    n = len(log)
    h = dp.remap_taobao_log(log, start, end, delta)
    keep, t_idx, comp, kept, m, waits = _epoch_and_compact(log, start, end, delta)
    want_keep = np.zeros(n, dtype=np.int32)
    want_keep[h["kept"]] = 1
    assert m == len(h["kept"]) and waits == 1
    assert np.array_equal(keep[:n], want_keep) and (keep[n:] == POISON).all() and (t_idx[n:] == POISON).all()
    assert np.array_equal(t_idx[:n][want_keep == 1], h["t_idx"]) and (t_idx[:n][want_keep == 0] == -1).all()
    for j in range(3):
        assert np.array_equal(comp[j][:m], log[h["kept"], j].astype(np.int32)) and (comp[j][m:] == POISON).all(), j
    assert np.array_equal(comp[3][:m], h["t_idx"]) and (comp[3][m:] == POISON).all()
    assert np.array_equal(kept[:m], h["kept"]) and (kept[m:] == POISON).all()
    d = dp.remap_taobao_log(log, start, end, delta, build="device")
    assert set(d) == set(h)
    for k in h:
        if k in ("uid", "iid", "t_idx", "kept"):
            assert torch.is_tensor(d[k]) and d[k].is_cuda and d[k].dtype == torch.int32, k
            assert np.array_equal(d[k].cpu().numpy(), h[k]), k
        elif isinstance(h[k], np.ndarray):
            assert isinstance(d[k], np.ndarray) and d[k].dtype == np.int32 and d[k].shape == h[k].shape and np.array_equal(d[k], h[k]), k
        else:
            assert d[k] == h[k], k
    return m


def test_epoch_slices_compaction_and_taobao_remap_on_g11():
    g = rc.g11()
    start, end, delta = g["start_end"].tolist()
    assert _check_taobao(g["raw"], start, end, delta) == len(g["remapped"])


@pytest.mark.parametrize("n", rc.EVENT_COUNTS)
def test_epoch_slices_and_compaction_at_the_tile_edges(n):
    log, start, end, delta = rc.taobao_log(n, "mixed")
    m = _check_taobao(log, start, end, delta)
    assert n < 10 or 0 < m < n


@pytest.mark.parametrize("mode", ["none", "all", "last"])
@pytest.mark.parametrize("n", [1, rc.SCAN_TILE + 1, rc.SORT_TILE + 1])
def test_keep_none_all_and_only_the_last_event(mode, n):
    log, start, end, delta = rc.taobao_log(n, mode)
    assert _check_taobao(log, start, end, delta) == {"none": 0, "all": n, "last": 1}[mode]


# ---- end to end, on the bundled Tmall sample ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    raw = rc.tmall_sample()
    host = dp.tmall_pipeline(raw, build="device", draws="cell", targets="device")
    dev = dp.tmall_pipeline(raw, build="device", draws="cell", targets="device", remap="device")
    return dict(raw=raw, host=host, dev=dev)


def test_device_remap_of_the_sample_equals_the_host_dict_key_for_key(sample):
    h = dp.remap_tmall_log(sample["raw"])
    d = dp.remap_tmall_log(sample["raw"], build="device")
    assert set(d) == set(h) | {"time_key"}
    for k in ("uid", "iid", "t_idx"):
        assert d[k].is_cuda and d[k].dtype == torch.int32 and np.array_equal(d[k].cpu().numpy(), h[k]), k
    assert d["time_key"].is_cuda and np.array_equal(d["time_key"].cpu().numpy(), sample["raw"][:, 5])
    for k in ("user_rows", "item_rows"):
        assert isinstance(d[k], np.ndarray) and d[k].dtype == np.int32 and np.array_equal(d[k], h[k]), k
    for k in ("n_users", "n_items", "feature_size", "vocab_sizes"):
        assert d[k] == h[k], k
    assert (d["n_users"], d["n_items"], d["feature_size"]) == (62, 5915, 9274) and (sample["raw"][:, 4] == -1).any()
    # a given profile is uploaded and used as it is
    age, gender = sample["raw"][:, 1] % 5, sample["raw"][:, 2] % 2
    h = dp.remap_tmall_log(sample["raw"], age=age, gender=gender)
    d = dp.remap_tmall_log(sample["raw"], age=age, gender=gender, build="device")
    assert np.array_equal(d["user_rows"], h["user_rows"]) and d["vocab_sizes"] == h["vocab_sizes"]
    # an int64 log is narrowed on the device; a value outside int32 is found there and refused
    assert sample["raw"].dtype == np.int32
    d = dp.remap_tmall_log(sample["raw"].astype(np.int64), build="device")
    assert np.array_equal(d["iid"].cpu().numpy(), dp.remap_tmall_log(sample["raw"])["iid"])
    for bad in (2 ** 31, -2 ** 31 - 1):
        log = sample["raw"][:40].astype(np.int64)
        log[7, 3] = bad
        with pytest.raises(ValueError, match="int32"):
            dp.remap_tmall_log(log, build="device")


def test_pipeline_graph_and_targets_equal_over_both_remaps(sample):
    (gh, rh, th), (gd, rd, td) = sample["host"], sample["dev"]
    assert torch.is_tensor(rd["uid"]) and isinstance(rh["uid"], np.ndarray)
    for a, b in ((gd.user_csr, gh.user_csr), (gd.item_csr, gh.item_csr)):
        for k in ("off1", "nbr1", "off2", "nbr2"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for side, n_ent in (("user", gh.U), ("item", gh.I)):
        for e in (0, 1, n_ent // 2, n_ent - 1):
            for hop in (1, 2):
                for t in range(gh.S):
                    assert np.array_equal(gd.cell(side, hop, e, t), gh.cell(side, hop, e, t)), (side, hop, e, t)
    assert np.array_equal(gd.user_rows, gh.user_rows) and np.array_equal(gd.item_rows, gh.item_rows)
    for name in ("train", "validation", "test"):
        (au, ai), (bu, bi) = td[name].arrays(), th[name].arrays()
        assert td[name].on_device and len(au) > 0 and np.array_equal(au, bu) and np.array_equal(ai, bi), name
    # the host target rule on the device remap's columns (a download), the same lines
    _, _, lines = dp.tmall_pipeline(sample["raw"], build="device", draws="cell", remap="device")
    assert lines["test"] == th["test"].lines()


def test_point_stores_equal_over_both_remaps(sample):
    from score_amd.pointdata import DeviceDataLoaderDualSeq
    B = {"train": 8, "validation": 200, "test": 200}
    kw = dict(batch_size=B, targets="device", draws="cell")
    dev, rd = dp.tmall_point_stores(sample["raw"], remap="device", **kw)
    host, _ = dp.tmall_point_stores(sample["raw"], **kw)
    assert torch.is_tensor(rd["time_key"])
    for name, neg in (("train", 1), ("validation", 99), ("test", 99)):
        a, b = dev[name], host[name]
        assert a.n_lines == b.n_lines > 0 and a.n_batches == b.n_batches >= 1, name
        mk = lambda st: DeviceDataLoaderDualSeq(B[name], 20, None, None, None, neg, None, None, store=st)
        n = 0
        for x, y in zip(mk(a), mk(b)):
            assert len(x) == len(y) == 7 and all(torch.equal(x[k], y[k]) for k in range(7)), name
            n += 1
            if n == 2:
                break
        assert n >= 1
