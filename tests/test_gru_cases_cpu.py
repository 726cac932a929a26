"""The rows of tests/test_gpu_gru_edges.py (tests/gru_cases.py) judged on the oracle alone, no GPU: the restated route gives every
row the family, waves and direction it names, the rows reach every edge they are there for, and the same recurrence evaluated in
float32 on the CPU stays within a QUARTER of the bounds the GPU test holds the kernels to against float64 (so an fp32 kernel can
meet them with room to spare).  Run with -s: every row prints its measured float32 errors as shares of the bounds."""
import numpy as np
import pytest
import torch

import gru_cases as gc

ROWS = gc.ROWS


def test_every_row_has_the_route_it_names():
    for name, r in ROWS.items():
        assert gc.route(r.H, r.T, 0) == r.fwd and gc.route(r.H, r.T, 1) == r.bwd, name
        for f in (r.fwd, r.bwd):
            assert f is None or (gc.unpack(gc.pack(f)) == f and gc.pack(f) > 0)
    # the refusal asymmetry: 3 * 32 * (H + 1) * 4 <= 160 KiB up to H = 425, 32 * (4 H + 3) * 4 only up to H = 319
    assert gc.route(319, 2, 1) == gc.Form(gc.LDS, 4, 1) and gc.route(320, 2, 1) is None
    assert gc.route(425, 2, 0) == gc.Form(gc.LDS, 4, 0) and gc.route(426, 2, 0) is None
    assert ROWS["h320_b2_t2"].bwd is None and ROWS["h320_b2_t2"].fwd == gc.Form(gc.LDS, 4, 0)


def test_the_rows_reach_every_edge():
    rows = list(ROWS.values())
    forms = {f for r in rows for f in (r.fwd, r.bwd) if f}
    assert forms == {gc.Form(fam, w, d) for fam, w in ((gc.X3, 8), (gc.REG, 4), (gc.LDS, 4)) for d in (0, 1)} | {gc.Form(gc.REG, 2, 1)}
    for H in (16, 32, 64, 128):
        assert {1, 15, 16, 17, 33} <= {r.B for r in rows if r.H == H}
    for H in (20, 48, 256):
        assert {1, 31, 32, 33} <= {r.B for r in rows if r.H == H}
    assert {1, 2, 3, 4, 5} <= {r.T for r in rows if r.H == 128}
    assert {19, 20, 21} <= {r.T for r in rows if r.H == 32}
    assert [r.bwd.waves for r in rows if r.H == 32 and r.T in (19, 20, 21)] == [4, 2, 2]
    for fam in (gc.X3, gc.REG, gc.LDS):
        mine = [r for r in rows if r.fwd.family == fam]
        assert any(r.T == 50 for r in mine)
        assert {"mixed", "zero", "full"} <= {r.lengths for r in mine}
        assert any(r.null_final for r in mine) and any(r.null_dfinal for r in mine)
        assert any(r.pad for r in mine) and any(not r.pad for r in mine)
    assert any(r.H == 32 and r.T == 50 and r.bwd.waves == 2 for r in rows)
    for r in rows:
        L = gc.lengths(r)
        if r.lengths == "mixed" and r.B >= 5:
            assert L[0] == 0 and L[r.B // 2] == 0 and L[-1] == 0 and (L == r.T).any() and (L > r.T).sum() == 1
            assert len({0, r.B // 2, r.B - 1, 1, 2}) == 5
        elif r.lengths == "zero":
            assert not L.any()
        else:
            assert (L == r.T).all()


@pytest.mark.parametrize("name", list(ROWS))
def test_fp32_recurrence_stays_within_a_quarter_of_the_bounds(name):
    r = ROWS[name]
    inp = gc.inputs(r)
    ref, dwg, dwc = gc.recurrence(r, inp, torch.float64)
    got, _, _ = gc.recurrence(r, inp, torch.float32)
    e = gc.compare(r, inp, got, ref, dwg, dwc)
    print("%s: fp32 CPU errors as shares of the bounds: %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(e.items()))))
    assert max(e.values()) <= 0.25, (name, e)
    # the reference itself: a length above T is T, a dead sample's state stays 0, something is live unless the row says otherwise
    live = gc.live_mask(r, inp)
    assert live.any() == (r.lengths != "zero")
    assert not ref.final[inp.length == 0].any() and not ref.out[~live].any() and not ref.dxproj[~live].any()
    over = inp.length > r.T
    if over.any():
        assert np.array_equal(ref.final[over], ref.out[over, r.T - 1])
    if live.any() and r.T > 1:
        assert np.abs(ref.dxproj[:, :, :r.H]).max() > 1e-3 and np.abs(dwg).max() > 1e-3          # the recurrent path carries gradient
