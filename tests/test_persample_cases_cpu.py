"""The inputs of tests/test_gpu_persample_edges.py (tests/persample_cases.py) judged on the oracle alone, no GPU: the kink filter
keeps the sample that keeps every slice computed and drops what the table records, every batch has the properties its row
claims (run with -s, each case prints its dropped count, A, instance and group sizes), and the table reaches every kernel instance, group size and tile edge it is there for."""
import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import away_from_relu_kinks
import persample_cases as pc

# the slot counts / group sizes each row names (call 0: Fi D / 4 slots, call 1: Fu D / 4), its I = (Fu + Fi) D and its instance
CLAIMS = {
    "smallest": dict(geom=((1, 1), (1, 1)), I=8, inst=(5, 1)),
    "gs2_a16": dict(geom=((4, 4), (2, 2)), I=24, inst=(5, 1)),
    "k4_a32": dict(geom=((16, 16), (12, 16)), I=112, inst=(5, 2)),
    "k5_a48_wide": dict(geom=((32, 32), (16, 16)), I=192, inst=(5, 3)),
    "k6_a33": dict(geom=((8, 8), (6, 8)), I=56, inst=(10, 3)),
    "k6_a32_stride": dict(geom=((8, 8), (4, 4)), I=48, inst=(10, 2)),
    "i140_k9": dict(geom=((20, 32), (15, 16)), I=140, inst=(10, 1)),
    "gs64_k7_a48": dict(geom=((40, 64), (8, 8)), I=192, inst=(10, 3)),
    "gs64_k8_a48_layered": dict(geom=((40, 64), (8, 8)), I=192, inst=(10, 3)),
    "user_wide": dict(geom=((32, 32), (16, 16)), I=192, inst=(5, 2)),
    "item_wide": dict(geom=((32, 32), (16, 16)), I=192, inst=(5, 2)),
    "b512": dict(geom=((4, 4), (3, 4)), I=28, inst=(5, 1)),
    "b513_layered": dict(geom=((4, 4), (3, 4)), I=28, inst=(5, 1)),
    "lengths_over_T": dict(geom=((16, 16), (12, 16)), I=112, inst=(10, 1)),
    "all_lengths_zero": dict(geom=((16, 16), (12, 16)), I=112, inst=(5, 1)),
}


@pytest.mark.parametrize("name", list(pc.CASES))
def test_case_is_what_its_row_claims(name):
    r = pc.CASES[name]
    cfg, P, b_all = pc.raw_batch(name)
    # the filter on its own, uncapped: what it drops is what the table records (the tests' cap is that + 2), never above a
    # quarter of the batch, nothing at all from a batch of five or fewer
    _, _, kept_all = away_from_relu_kinks(cfg, P, b_all, max_dropped=r.gen - 1)
    dropped = r.gen - kept_all.size
    print("%s: dropped %d of %d, A = %d, instance <%d,%d>, slots / group size %s, I = %d, %s"
          % ((name, dropped, r.gen, pc.computed_slices(r)) + pc.instance(r) + (pc.gather_geometry(r), (r.Fu + r.Fi) * r.D, r.form)))
    assert dropped <= r.dropped + 2 and r.dropped <= r.B // 4 and (r.B > 5 or r.dropped == 0 == dropped)
    c = pc.case(name)
    b = c.batch
    Bk = b["label"].shape[0]
    assert c.kept[0] == 0 and Bk >= r.B - r.dropped - 2 and (r.gen == r.B or Bk == r.B)
    assert np.array_equal(c.kept, kept_all[:Bk])
    assert np.array_equal(b_all["label"], np.arange(r.gen) % 2) and np.array_equal(b["label"], b_all["label"][c.kept])
    # geometry
    assert pc.gather_geometry(r) == CLAIMS[name]["geom"] and (r.Fu + r.Fi) * r.D == CLAIMS[name]["I"] == cfg.Du + cfg.Di
    assert pc.instance(r) == CLAIMS[name]["inst"]
    assert cfg.H == 32 and cfg.Dhead == (1 if r.mt != "SCORE" else 2) * 32 + CLAIMS[name]["I"]
    # lengths
    L = b["length"]
    if r.lengths == "zero":
        assert np.all(L == 0) and pc.computed_slices(r) == 1
    elif r.lengths == "over":
        assert int((L > r.T).sum()) >= 3 and int((L == r.T).sum()) >= 1 and int(L.max()) == 3 * r.T and int(L.min()) < r.T
    else:
        assert int(L.max()) == r.A == int(L[0]) and int(L.min()) >= 1
    if name == "k6_a32_stride":
        assert int(L.max()) == 32 < r.T == 40
    # a fifth of the slices' ids are zero (helpers.random_batch), some inside live slices
    if Bk * r.T >= 20:
        assert any((b[k].reshape(Bk, r.T, -1) == 0).all(2).any() for k in ("user_1hop", "user_2hop", "item_1hop", "item_2hop"))
    with torch.no_grad():
        out = so.forward(cfg, so.to_torch_params(P), so.to_torch_batch(b))
    assert out["relu_margin"] >= 1e-5


def test_table_covers_every_instance_and_edge():
    per = [pc.CASES[n] for n in pc.PERSAMPLE]
    inst = {(5 if r.K <= 5 else 10, -(-pc.computed_slices(r) // 16)) for r in per}
    assert inst == {(k, m) for k in (5, 10) for m in (1, 2, 3)}
    assert {8, 24, 140, 192} <= {(r.Fu + r.Fi) * r.D for r in per}
    assert {1, 2, 4, 8, 16, 32, 64} == {gs for r in per for _, gs in pc.gather_geometry(r)}
    assert {1, 16, 32, 33, 48} <= {pc.computed_slices(r) for r in per}
    assert {1, 4, 5, 6, 7, 9, 10} <= {r.K for r in per}
    assert {1, 512} <= {r.B for r in per}
    assert {"SCORE", "SCORE_USER", "SCORE_ITEM"} == {r.mt for r in per}
    # both sides of PS_MAX_B and of the LDS bound: the layered rows are their per-sample neighbours plus one
    a, b = pc.CASES["b512"], pc.CASES["b513_layered"]
    assert b.form == "layered" and a.form == "persample" and b._replace(B=512, gen=520, dropped=a.dropped, form=a.form) == a
    a, b = pc.CASES["gs64_k7_a48"], pc.CASES["gs64_k8_a48_layered"]
    assert b.form == "layered" and a.form == "persample" and b._replace(K=7, form=a.form) == a
