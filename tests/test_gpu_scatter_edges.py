"""The embedding-gradient path below the model at its seams (the rows of tests/scatter_cases.py; their CPU twin is
tests/test_scatter_cases_cpu.py): score_segment_sum_rows -- pull_kernel and pull_fixup_kernel -- at every window size, lane-group
width, chain class, long-chain split and run-end distance; score_rows_accumulate / _multi against a float32 loop in source order;
score_index_plan's de-duplication products against numpy; score_auc_logloss against exact rational arithmetic.  Every scatter row
first asserts the structure it claims to reach (and that the restated geometry is score_pull_geometry's), then its numbers: the
exact fill bit for bit, the rounding fill inside gamma(m - 1) sum|src|.  Run with -s: each row prints the kernels' worst error as
a share of that bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from score_amd import _lib
import scatter_cases as sc

pytestmark = pytest.mark.gpu

_WORST = [0.0, 0.0]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _segment_sum(D, rows_dev, src_dev, n_out, out0, flags0, scratch_bytes=None, n=None):
    """one score_segment_sum_rows call on fresh copies of out0 / flags0 (flags0 None: no row_flags); (status, out, flags)"""
    lib = _lib.load()
    n = rows_dev.numel() if n is None else n
    need = int(lib.score_segment_sum_scratch_bytes(n, D))
    assert need > 0
    scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
    out = torch.from_numpy(out0).cuda()
    flags = torch.from_numpy(flags0).cuda() if flags0 is not None else None
    rc = lib.score_segment_sum_rows(_p(rows_dev), _p(src_dev), n, D, n_out, _p(out), _p(flags), _p(scratch),
                                    need if scratch_bytes is None else scratch_bytes(need), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), flags.cpu().numpy() if flags is not None else None


# ---------------------------------------------------------------------------------------------- score_segment_sum_rows
@pytest.mark.parametrize("name", list(sc.SCATTER_ROWS))
def test_scatter_row(name):
    lib = _lib.load()
    r = sc.SCATTER_ROWS[name]
    inp = sc.scatter_inputs(r)
    # the structure first: a row that does not reach its seam fails here, it does not test another one
    st = sc.structure(inp.keys, r.D)
    sc.check_claim(r, st)
    geo = [C.c_int32(0) for _ in range(4)]
    assert lib.score_pull_geometry(st.n, r.D, *[C.byref(g) for g in geo]) == 0
    assert tuple(g.value for g in geo) == (st.window, st.lanes, st.gpb, sc.LONG_CHAIN)
    rows_dev = torch.from_numpy(inp.rows).cuda()
    worst = sc.Worst(0.0, 0.0)
    for kind in ("exact", "rounding"):
        src = sc.scatter_fill(r, kind)
        src_dev = torch.from_numpy(src).cuda()
        rc, out, flags = _segment_sum(r.D, rows_dev, src_dev, inp.n_out, inp.out0, inp.flags0)
        assert rc == 0 and lib.score_pull_last_form() == 0, (name, rc)           # the owner-side sum: always pull_kernel
        rc2, out2, _ = _segment_sum(r.D, rows_dev, src_dev, inp.n_out, inp.out0, None)       # again, without row_flags
        assert rc2 == 0 and np.array_equal(out.view(np.uint32), out2.view(np.uint32)), (name, kind, "two runs differ")
        worst = sc.scatter_judge(r, kind, src, out, flags)
    _WORST[:] = [max(a, b) for a, b in zip(_WORST, worst)]
    print("%s: window %d, %d lanes, max L %d, %d long: kernels at %.6f of the rounding bound, %.3f in runs of three and more "
          "(worst so far %.6f, %.3f)" % ((name, st.window, st.lanes, st.max_L, st.n_long) + tuple(worst) + tuple(_WORST)))
    assert worst.all <= 1.0


def test_scatter_refusals_leave_out_untouched():
    lib = _lib.load()
    r = sc.SCATTER_ROWS["width_d16"]
    inp = sc.scatter_inputs(r)
    n = len(inp.rows)
    rows_dev = torch.from_numpy(inp.rows).cuda()
    wide = torch.ones((n, 260), device="cuda")
    out260 = np.full((inp.n_out, 260), 5.0, np.float32)

    def untouched(res, out0):
        rc, out, flags = res
        assert np.array_equal(out, out0) and np.array_equal(flags, inp.flags0)
        return rc

    src_dev = torch.from_numpy(sc.scatter_fill(r, "exact")).cuda()
    # the op needs 64 bytes less than score_segment_sum_scratch_bytes answers (the query's slack): one byte below THAT is refused,
    # one byte below the query's answer is still enough and the result the same
    assert untouched(_segment_sum(16, rows_dev, src_dev, inp.n_out, inp.out0, inp.flags0, lambda need: need - 65), inp.out0) \
        == sc.E_WORKSPACE
    rc, out, flags = _segment_sum(16, rows_dev, src_dev, inp.n_out, inp.out0, inp.flags0, lambda need: need - 1)
    assert rc == 0 and sc.scatter_judge(r, "exact", sc.scatter_fill(r, "exact"), out, flags).all == 0.0
    # D % 4: before anything is launched.  D = 260: 128 lanes a group -- the launcher's SCORE_E_SHAPE, after the sort inside scratch
    assert untouched(_segment_sum(6, rows_dev, wide, inp.n_out, out260[:, :6].copy(), inp.flags0), out260[:, :6]) == sc.E_BADARG
    assert untouched(_segment_sum(260, rows_dev, wide, inp.n_out, out260, inp.flags0), out260) == sc.E_SHAPE
    assert untouched(_segment_sum(16, rows_dev, src_dev, 0, inp.out0, inp.flags0), inp.out0) == sc.E_BADARG
    assert untouched(_segment_sum(16, rows_dev, src_dev, inp.n_out, inp.out0, inp.flags0, n=0), inp.out0) == 0     # nothing to do
    out = torch.from_numpy(inp.out0).cuda()
    scratch = torch.empty((1 << 20,), dtype=torch.uint8, device="cuda")
    for args in ((None, _p(src_dev), _p(out), _p(scratch)), (_p(rows_dev), None, _p(out), _p(scratch)),
                 (_p(rows_dev), _p(src_dev), None, _p(scratch)), (_p(rows_dev), _p(src_dev), _p(out), None)):
        assert lib.score_segment_sum_rows(args[0], args[1], n, 16, inp.n_out, args[2], None, args[3], 1 << 20, _stream()) \
            == sc.E_BADARG
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), inp.out0)


# ---------------------------------------------------------------------------------------------- score_rows_accumulate(_multi)
def _acc_device(r):
    src, out0, flags0 = sc.acc_inputs(r)
    # (one slot of padding behind the lists: an empty tensor's pointer is null)
    rows_all = np.concatenate(list(r.lists) + [np.zeros(1, np.int32)])
    src_all = np.concatenate([src, np.zeros((1, r.D), np.float32)])
    return src, out0, flags0, torch.from_numpy(rows_all).cuda(), torch.from_numpy(src_all).cuda()


@pytest.mark.parametrize("name", list(sc.ACC_ROWS))
def test_accumulate_row(name):
    """one score_rows_accumulate per source in source order, and score_rows_accumulate_multi: each bit for bit the float32 loop
    in source order -- also for rows that enter in state 2, where what is there comes first"""
    lib = _lib.load()
    r = sc.ACC_ROWS[name]
    src, out0, flags0, rows_dev, src_dev = _acc_device(r)
    want, want_flags = sc.acc_reference(r, src, out0, flags0)
    offs = np.concatenate([[0], np.cumsum([len(l) for l in r.lists])]).astype(np.int64)
    got = {}
    for mode in ("per-source", "multi"):
        out, flags = torch.from_numpy(out0).cuda(), torch.from_numpy(flags0).cuda()
        if mode == "per-source":
            for q in range(len(r.lists)):
                a, b = int(offs[q]), int(offs[q + 1])
                rc = lib.score_rows_accumulate(_p(rows_dev[a:]), _p(src_dev[a:]), b - a, r.D, r.n_out, _p(out), _p(flags), _stream())
                assert rc == 0, (name, q, rc)
        else:
            o = (C.c_int64 * len(offs))(*offs.tolist())
            rc = lib.score_rows_accumulate_multi(_p(rows_dev), _p(src_dev), o, len(r.lists), r.D, r.n_out, _p(out), _p(flags),
                                                 _stream())
            assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        got[mode] = (out.cpu().numpy(), flags.cpu().numpy())
        sc.acc_judge(r, want, want_flags, *got[mode])
    assert np.array_equal(got["multi"][0].view(np.uint32), got["per-source"][0].view(np.uint32))


def test_accumulate_refusals():
    lib = _lib.load()
    r = sc.ACC_ROWS["eight_sources_d256"]
    src, out0, flags0, rows_dev, src_dev = _acc_device(r)
    out, flags = torch.from_numpy(out0).cuda(), torch.from_numpy(flags0).cuda()
    o65 = (C.c_int64 * 66)(*([0] * 66))
    o64 = (C.c_int64 * 65)(*([0] * 65))
    multi = lambda o, ns, D: lib.score_rows_accumulate_multi(_p(rows_dev), _p(src_dev), o, ns, D, r.n_out, _p(out), _p(flags), _stream())
    assert multi(o65, 65, 256) == sc.E_BADARG and multi(o64, 64, 256) == 0 and multi(o64, 0, 256) == sc.E_BADARG
    assert multi(o64, 8, 260) == sc.E_BADARG and multi(o64, 8, 6) == sc.E_BADARG
    one = lambda D: lib.score_rows_accumulate(_p(rows_dev), _p(src_dev), 3, D, r.n_out, _p(out), _p(flags), _stream())
    assert one(260) == sc.E_BADARG and one(6) == sc.E_BADARG and one(0) == sc.E_BADARG
    assert lib.score_rows_accumulate(_p(rows_dev), _p(src_dev), 3, 256, r.n_out, _p(out), None, _stream()) == sc.E_BADARG
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), out0.view(np.uint32)) and np.array_equal(flags.cpu().numpy(), flags0)


# ---------------------------------------------------------------------------------------------- score_index_plan
def _plan_products(c, t, debug_flags):
    """score_index_plan(n_shards = G, dedup = 1) on a model's workspace, no process group; the products read back through the
    layout's plan_meta / plan_unique_rows / plan_remap"""
    from score_amd.model import SCORE, DeviceBatch
    m = SCORE(c.N, 4, 8, c.T, c.K, c.Fu, c.Fi)
    db = DeviceBatch.empty(m, c.B, c.active)
    for i in range(6):
        db.tensors[i].copy_(torch.from_numpy(t[i]).reshape(db.tensors[i].shape))
    db.tensors[6].zero_()
    db.tensors[7].fill_(sc.plan_active(c))
    lay, ws = m._workspace(c.B)
    sizes = [t[f].size for f in sc.FEED_OF_SEG]
    out = []
    for flags in debug_flags:
        m.debug_flags = flags
        st = m._state(ws)
        word = torch.zeros((1,), dtype=torch.int32, device="cuda")
        st.id_status = word.data_ptr()
        remap = [ws[lay.plan_remap[g]:lay.plan_remap[g] + sizes[g]].view(torch.int32) for g in range(6)]
        for x in remap:
            x.fill_(sc.REMAP_SENTINEL)
        meta = ws[lay.plan_meta:lay.plan_meta + 2 + c.G].view(torch.int32)
        meta.fill_(-1)
        rc = m.lib.score_index_plan(C.byref(m.cfg), C.byref(st), C.byref(db.struct), c.G, 1, m._stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, flags, rc)
        mh = meta.cpu().numpy()
        U = int(mh[0])
        assert 1 <= U <= sc.plan_occurrences(c), (c.name, U)
        uniq = ws[lay.plan_unique_rows:lay.plan_unique_rows + U].view(torch.int32).cpu().numpy()
        out.append(sc.PlanProducts(U, mh[1:2 + c.G].copy(), uniq, [x.cpu().numpy() for x in remap], int(word.item())))
    m.debug_flags = 0
    return out


@pytest.mark.parametrize("name", list(sc.PLAN_ROWS))
def test_index_plan_row(name):
    c = sc.PLAN_ROWS[name]
    t = sc.plan_inputs(c)
    prods = _plan_products(c, t, sc.PLAN_SORT_FLAGS)
    sc.plan_judge(c, t, prods[0])
    for p, flags in zip(prods[1:], sc.PLAN_SORT_FLAGS[1:]):                    # both sort forms: the same products bit for bit
        assert p.U == prods[0].U and p.id_status == prods[0].id_status, (name, flags)
        assert np.array_equal(p.offsets, prods[0].offsets) and np.array_equal(p.unique_rows, prods[0].unique_rows), (name, flags)
        for a, b in zip(p.remap, prods[0].remap):
            assert np.array_equal(a, b), (name, flags)


# ---------------------------------------------------------------------------------------------- score_auc_logloss
@pytest.mark.parametrize("name", list(sc.AUC_ROWS))
def test_auc_logloss_row(name):
    from score_amd import harness as h
    r = sc.AUC_ROWS[name]
    p, y = sc.auc_inputs(r)
    want_auc, want_ll = sc.auc_reference(p, y)
    auc, ll = h.auc_logloss_device(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda())
    print("%s: auc %r (want %s), log-loss off by %.2e" % (name, auc, want_auc if want_auc is None else float(want_auc),
                                                         abs(ll - want_ll)))
    sc.auc_judge(r, want_auc, want_ll, auc, ll)
    auc2, ll2 = h.auc_logloss_device(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda())
    assert (auc2 == auc or want_auc is None) and ll2 == ll                      # fixed partition, fixed order: the same bits again
