"""The inputs of tests/test_gpu_score_head_edges.py (tests/score_head_cases.py) judged on the oracle alone, no GPU: the kink filter
drops what the table records and leaves the batch size the row names, the Python mirror of the four launch rules gives every row the
forms it states, the float32 oracle meets the bounds of the GPU test against the float64 oracle on every row (so an fp32 pass CAN
meet them: shown from the reference alone), and each parameter case has the property it is there for (run with -s: each case
prints its dropped count, its forms and its float32-against-float64 errors)."""
import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import away_from_relu_kinks
import score_head_cases as hc


def close(a, b, rtol, atol):
    """tests/test_gpu_model.py::close (that module is a GPU module: restated, not imported)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if max(np.abs(a).max(), np.abs(b).max()) < 1e-7:
        return True, 0.0
    scale = max(np.abs(b).max(), 1e-12)
    return np.abs(a - b).max() <= atol + rtol * scale, float(np.abs(a - b).max() / scale)


def _masks(c):
    return [torch.as_tensor(m) for m in c.masks] if c.masks is not None else None


@pytest.mark.parametrize("name", hc.SHAPE_CASES)
def test_case_is_what_its_row_claims(name):
    r = hc.CASES[name]
    cfg, P, b_all, masks = hc.raw_batch(name)
    # the filter on its own, uncapped: what it drops is what the table records (the tests' cap is that + 2), never above a
    # quarter of the batch, nothing at all from a batch of five or fewer
    _, _, kept_all = away_from_relu_kinks(cfg, P, b_all, keep_prob=r.keep, dropout_masks=masks, max_dropped=r.gen - 1)
    dropped = r.gen - kept_all.size
    f = hc.mirror(r)
    print("%s: dropped %d of %d, Dh = %d, forms %s" % (name, dropped, r.gen, hc.dims(r)[0], tuple(f)))
    assert dropped == r.dropped and r.dropped <= r.B // 4 and (r.B > 5 or r.dropped == 0)
    c = hc.case(name)
    b = c.batch
    assert b["label"].shape[0] == r.B == c.kept.size and np.array_equal(c.kept, kept_all[:r.B])
    assert np.array_equal(b["label"], b_all["label"][c.kept]) and np.array_equal(b_all["label"], np.arange(r.gen) % 2)
    assert cfg.Dhead == hc.dims(r)[0] and all(v.shape[0] == r.B for v in b.values())
    # the launch rules give the row the forms it names
    assert f == r.forms, (name, f, r.forms)
    assert hc.unpack(hc.pack(f)) == f
    # every slice is computed, and the lengths are what the row says
    L = b["length"]
    assert int(L.max()) >= r.T
    if r.lengths == "ends_zero":
        assert L[0] == 0 and L[-1] == 0 and int((L == r.T).sum()) >= 1
    elif r.lengths == "over":
        assert {0, 1, r.T, r.T + 1, 3 * r.T} <= set(L.tolist()) and int((L > r.T).sum()) >= 3
    else:
        assert int(L.min()) >= 1 and int(L.max()) == r.T
    if r.keep < 1.0:
        assert c.masks[0].shape == (r.B, hc.FC1) and c.masks[1].shape == (r.B, hc.FC2) and r.B % 16 != 0
        assert 0.7 < c.masks[0].mean() < 0.9 and 0.7 < c.masks[1].mean() < 0.9
    # the float32 oracle against the float64 oracle, at the bounds the GPU test holds the kernels to
    o32, g32 = so.loss_and_grads(cfg, P, b, 0.0, r.keep, _masks(c))
    o64, g64 = so.loss_and_grads(cfg, P, b, 0.0, r.keep, _masks(c), dtype=torch.float64)
    assert o32["relu_margin"] >= 1e-5
    l32, l64 = float(o32["loss"].detach()), float(o64["loss"].detach())
    assert abs(l32 - l64) < hc.LOSS_TOL * max(1.0, abs(l64))
    worst = ("", 0.0)
    for k in ("y_pred", "logit"):
        d = float(np.abs(o32[k].detach().numpy() - o64[k].detach().numpy()).max())
        assert d < hc.Y_TOL, (k, d)
    for k in ("att_score", "head_inp"):
        ok, err = close(o32[k].detach().numpy(), o64[k].detach().numpy(), hc.RTOL, hc.ATOL)
        worst = max(worst, (k, err), key=lambda t: t[1])
        assert ok, (k, err)
    for k in g64:
        ok, err = close(g32[k], g64[k], hc.RTOL, hc.ATOL)
        worst = max(worst, (k, err), key=lambda t: t[1])
        assert ok, (k, err)
        assert np.isfinite(g64[k]).all()
    assert np.all(g64["emb_mtx"][0] == 0)
    print("    float32 against float64 oracle: |dloss| %.2e, worst array %s %.2e" % (abs(l32 - l64), worst[0], worst[1]))


@pytest.mark.parametrize("name", hc.PARAM_CASES)
def test_parameter_case_has_its_property(name):
    r = hc.CASES[name]
    c = hc.case(name)
    assert hc.mirror(r) == r.forms and c.batch["label"].shape[0] == r.B and np.array_equal(c.batch["label"], np.arange(r.B) % 2)
    with torch.no_grad():
        out = so.forward(c.cfg, so.to_torch_params(c.P), so.to_torch_batch(c.batch))
    y, w, L = out["y_pred"].numpy(), out["att_score"].numpy(), c.batch["length"]
    assert y.dtype == np.float32 and np.isfinite(y).all() and np.isfinite(w).all()
    if name == "sigmoid_01":
        print("%s: y == 0 on %d samples, y == 1 on %d of %d" % (name, int((y == 0).sum()), int((y == 1).sum()), r.B))
        assert (y == 0.0).any() and (y == 1.0).any()
    elif name == "softmax_onehot":
        multi = L > 1
        assert multi.sum() >= r.B // 2
        print("%s: smallest largest weight of a row with more than one live slice %.6f" % (name, float(w[multi].max(1).min())))
        assert np.all((w[multi] > 0.999).sum(1) == 1)
    elif name == "softmax_uniform":
        for i in range(r.B):
            n = min(int(L[i]), r.T)
            assert np.all(w[i, :n] == np.float32(1) / np.float32(n)) and np.all(w[i, n:] == 0)
    elif name == "dead_relus":
        P = so.to_torch_params(c.P)
        inv = P["bn1/gamma"] * (1.0 / np.sqrt(1.0 + so.BN_EPS))
        zf1 = (out["head_inp"] * inv + P["bn1/beta"]) @ P["fc1/kernel"] + P["fc1/bias"]
        assert float(zf1.max()) < -100.0                                   # f1 = 0 everywhere, with room
        _, g = so.loss_and_grads(c.cfg, c.P, c.batch, 0.0)
        front = [k for k in g if not k.startswith(("fc2", "fc3")) and k != "fc1/bias"]
        assert "emb_mtx" in front and "fc1/kernel" in front and "bn1/gamma" in front and len(front) >= 20
        for k in front:
            assert np.all(g[k] == 0), k
        assert np.abs(g["fc3/bias"]).max() > 0


def test_table_covers_every_seam():
    rows = [hc.CASES[n] for n in hc.SHAPE_CASES]
    f = [r.forms for r in rows]
    assert {x.hf for x in f} == {1, 2} and {x.ny for x in f} == {1, 2, 4}
    assert {(x.af_S, x.af_KQ) for x in f} >= {(0, 0), (1, 36), (1, 44), (1, 52), (1, 84), (1, 148), (2, 36), (4, 36)}
    assert {(x.ab_S, x.ab_pool) for x in f} == {(0, 0), (1, 1), (2, 1), (4, 1), (4, 0)}
    # k-steps per lane quarter of the head's forward: below one chunk, one chunk, into the second, two chunks, into the second trip
    assert {12, 16, 20, 32, 36} <= {((hc.dims(r)[0] + 15) & ~15) // 4 for r in rows}
    # both sides of every threshold, by rows that differ in nothing else
    C = hc.CASES
    for a, b, field in (("b496", "b497", "B"), ("b2048_ny2", "b2049_ny1", "B"), ("pool_in", "pool_out", "B"),
                        ("lds_s1_in", "lds_s1_out", "T"), ("lds_s4_in", "lds_s4_to_s2", "T")):
        ra, rb = C[a], C[b]
        assert getattr(rb, field) == getattr(ra, field) + 1
        assert rb._replace(forms=ra.forms, gen=ra.gen, dropped=ra.dropped, **{field: getattr(ra, field)}) == ra and rb.forms != ra.forms
    # the LDS bound of the attention's forward: inside by less than one slice's worth, outside by less than one
    assert hc.LDS_BOUND - 123 * 4 < hc.attn_fwd_lds(1, 247, 144) <= hc.LDS_BOUND < hc.attn_fwd_lds(1, 248, 144)
    assert hc.attn_fwd_lds(4, 61, 144) <= hc.LDS_BOUND < hc.attn_fwd_lds(4, 62, 144)
    # head backward shares at Dh = 528: 33 column tiles dealt 9, 9, 9, 6 -- wave 0 of the first three shares takes two tiles
    nt = (hc.dims(C["dh528"])[0] + 15) // 16
    per = -(-nt // 4)
    assert nt == 33 and [min(nt, (y + 1) * per) - y * per for y in range(4)] == [9, 9, 9, 6]
    assert (hc.dims(C["dh496"])[0], hc.dims(C["dh512"])[0]) == (496, 512)
    # rows per workgroup of the attention
    assert {1, 16, 17, 33} <= {r.T for r in rows if r.B == 3}
    assert C["s2_t8"].B % 2 == 1 and 2 * C["s2_t8"].T == 16 and C["s4_ns3"].B % 4 == 3 and C["b1025_ny2"].B % 4 == 1
    assert C["t129"].T > (512 // 1) // 4
    assert {"SCORE", "RCA", "SCORE_USER", "SCORE_ITEM"} == {r.mt for r in rows}
