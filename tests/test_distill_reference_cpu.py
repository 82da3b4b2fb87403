"""CPU: the float64 restatement of the distillation losses (tests/distill_reference.py) reproduces the reference goldens of
tests/golden/distill.npz, and the cases of tests/distill_cases.py are what they claim to be (conditions on the inputs and on the
restatement alone, no measurement of the kernels)."""
import numpy as np
import pytest

import distill_cases as C
import distill_reference as D

LEFT_OUT_CAP = 0.01          # the largest share of a case's gradient values that may sit within MARGIN of a decision


def _pixel(g):
    return (g["voxel"][0] * int(g["osf"]), g["voxel"][1] * int(g["osf"]))


# ---- the goldens -----------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_corners_valid_and_mask_goldens(golden):
    g = golden("distill")
    corners, valid = D.box_corners(g["gt"], g["pc_range"], _pixel(g))
    np.testing.assert_array_equal(valid, g["valid"])
    np.testing.assert_allclose(corners, g["corners_px"], rtol=1e-5, atol=2e-5)
    mask = D.gaussian_mask(g["gt"], g["pc_range"], _pixel(g), 20, 20)
    assert mask.dtype == np.float32
    np.testing.assert_array_equal(mask, g["resp_a_mask"])
    np.testing.assert_array_equal(mask, g["resp_b_mask"])


@pytest.mark.parametrize("name,fn", [("feat", D.feature_loss), ("rel", D.relation_loss)])
def test_restatement_reproduces_box_loss_goldens(golden, name, fn):
    g = golden("distill")
    r = fn(g[f"{name}_s"], g[f"{name}_t"], g["corners_px"], g["valid"])
    np.testing.assert_allclose(r["loss"], float(g[f"{name}_loss"]), rtol=2e-5)
    # the golden gradient is a float32 evaluation: where it sits on a sign it could not decide (the relation golden has student and
    # teacher of equal scale, its Gram diagonal differs by 1e-5) the two may disagree, everywhere else they agree
    keep = ~r["left_out"]
    assert keep.mean() > 0.5
    np.testing.assert_allclose(r["grad"][keep], g[f"{name}_grad"][keep], rtol=2e-4, atol=1e-6)
    assert float(np.abs(r["grad"][~np.broadcast_to(r["touched"].reshape(2, 1, 20, 20), r["grad"].shape)]).max()) == 0.0


@pytest.mark.parametrize("tag,clamp", [("a", 1e-4), ("b", 1e-3)])
def test_restatement_reproduces_response_goldens(golden, tag, clamp):
    g = golden("distill")
    logits = [g[f"resp_{tag}_s{i}_hm"].astype(np.float64) for i in range(2)]
    prob = [1 / (1 + np.exp(-x)) for x in logits]
    s_hm = [np.clip(p, clamp, 1 - clamp) for p in prob]
    t_hm = [g[f"resp_{tag}_t{i}_hm"] for i in range(2)]
    s_reg = [g[f"resp_{tag}_s{i}_{h}"] for i in range(2) for h in C.HEADS]
    t_reg = [g[f"resp_{tag}_t{i}_{h}"] for i in range(2) for h in C.HEADS]
    r = D.response_loss(s_hm, t_hm, s_reg, t_reg, g[f"resp_{tag}_mask"], np.float32(clamp), np.float32(1 - clamp), 1.0, 2.0)
    np.testing.assert_allclose(r["cls"], float(g[f"resp_{tag}_cls"]), rtol=2e-5)
    np.testing.assert_allclose(r["reg"], float(g[f"resp_{tag}_reg"]), rtol=2e-5)
    k = 0
    for i in range(2):
        for h in C.HEADS:
            np.testing.assert_allclose(r["g_reg"][k], g[f"resp_{tag}_g{i}_{h}"], rtol=2e-4, atol=1e-7)
            k += 1
        # the golden's heat-map gradient is by the logit: through the clamped sigmoid
        inside = (prob[i] > clamp) & (prob[i] < 1 - clamp)
        keep = ~np.broadcast_to(r["left_out"][:, None], inside.shape)
        by_logit = r["g_hm"][i] * prob[i] * (1 - prob[i]) * inside
        np.testing.assert_allclose(by_logit[keep], g[f"resp_{tag}_g{i}_hm"][keep], rtol=2e-4, atol=1e-7)


# ---- the builders' conditions ----------------------------------------------------------------------------------------------------
def _share_left_out(res, C_):
    touched = int(res["touched"].sum()) * C_
    return float(res["left_out"].sum()) / max(touched, 1)


def test_box_geometry_is_what_the_cases_claim():
    geo = C.box_geometry()
    H, W = C.BOX_H, C.BOX_W
    assert H != W
    corners, valid = geo["corners"], geo["valid"]
    assert valid.tolist() == [[True] * 7 + [False] * 2] * 2
    assert not geo["gt"][1, C.BOX_ROWS_1["zero_row"]].any()               # an all-zero row inside the valid range
    kp = D.key_points(corners)
    tp = D.taps(kp, H, W)
    ins = tp["inside"]
    r0, r1 = C.BOX_ROWS_0, C.BOX_ROWS_1
    assert ins[0, r0["inside"]].all()
    assert not ins[0, r0["outside"]].any()
    for name in ("low_a", "high_a", "low_b", "high_b"):                   # straddling: some key points sample padding, some do not
        per_kp = ins[0, r0[name]].all(-1)
        assert per_kp.any() and not ins[0, r0[name]].all(), name
    assert tp["iy"][0, r0["low_a"]].min() < -1 and tp["iy"][0, r0["high_a"]].max() > H
    assert tp["ix"][0, r0["low_b"]].min() < -1 and tp["ix"][0, r0["high_b"]].max() > W
    # exact positions, in float32 as well as in float64
    for dt in (np.float64, np.float32):
        t = D.taps(D.key_points(corners, dt), H, W)
        assert (t["ix"][1, r1["centre"], 0], t["iy"][1, r1["centre"], 0]) == (22.0, 13.0)
        assert t["w"][1, r1["centre"], 0].tolist() == [1.0, 0.0, 0.0, 0.0]
        for kpi in (0, 3, 8):                                             # corners 0, 3 and their mid-point
            assert t["ix"][1, r1["minus_half"], kpi] == -0.5
            assert t["inside"][1, r1["minus_half"], kpi].tolist() == [False, True, False, True]
        for kpi in (1, 2, 6):
            assert t["ix"][1, r1["w_minus_half"], kpi] == W - 0.5
            assert t["inside"][1, r1["w_minus_half"], kpi].tolist() == [True, False, True, False]
        for row in ("zero_size", "zero_row"):
            assert (t["pix"][1, r1[row]] == t["pix"][1, r1[row], 0]).all()   # nine key points, 36 terms, four pixels
    assert (kp[1, r1["zero_row"]] == [20.0, 12.0]).all()                  # the world origin
    assert (corners[1, r1["twin_a"]] == corners[1, r1["twin_b"]]).all()
    # corners_of_gt: what the corner kernel is compared with (the three rewritten boxes moved by less than a pixel)
    assert float(np.abs(geo["corners_of_gt"][0] - corners).max()) < 0.5


@pytest.mark.parametrize("C_", C.BOX_CHANNELS)
@pytest.mark.parametrize("kind", [0, 1], ids=["feature", "relation"])
def test_box_cases_keep_off_the_decisions(kind, C_):
    c = C.box_case(kind, C_)
    r64, r32 = c["f64"], c["f32"]
    share = _share_left_out(r64, C_)
    print(f"kind {kind} C {C_}: {int(r64['left_out'].sum())} gradient values within MARGIN of a decision ({share:.2%})")
    assert share <= LEFT_OUT_CAP
    # the agreeing box: its pixels belong to no other box, its decisions are exactly zero, and so is the gradient there
    (b, pix), = c["agree_pixels"]
    m = C.BOX_ROWS_0["agree"]
    tp = r64["taps"]
    others = [k for k in range(C.BOX_M) if k != m and c["valid"][b, k]]
    other_pix = np.unique(tp["pix"][b, others][tp["inside"][b, others]])
    assert len(pix) >= 4 and not np.intersect1d(pix, other_pix).size
    for r in (r64, r32):
        assert not r["decision"][b, m].any()
        assert not r["grad"].reshape(2, C_, -1)[b][:, pix].any()
        assert not r["grad"].reshape(2, C_, -1).transpose(0, 2, 1)[~r["touched"]].any()
    if kind == 1:
        # every diagonal entry of the Gram difference of a box with a non-zero row is decided (the 3x teacher); the rows of a key
        # point that samples only padding are exactly zero on both sides
        dec = r64["decision"].reshape(2, C.BOX_M, 9, 9)
        diag = np.abs(np.diagonal(dec, axis1=2, axis2=3))
        kp_in = tp["inside"].any(-1)
        for b in range(2):
            for k in range(C.BOX_M):
                if not c["valid"][b, k] or (b, k) == (0, m):
                    continue
                assert (diag[b, k][kp_in[b, k]] >= D.MARGIN).all(), (b, k, diag[b, k])
                assert not dec[b, k][~kp_in[b, k]].any()
        assert not dec[0, C.BOX_ROWS_0["outside"]].any()                   # nine zero-norm rows


@pytest.mark.parametrize("kind", [0, 1], ids=["feature", "relation"])
@pytest.mark.parametrize("name", list(C.SCATTER_CASES))
def test_scatter_cases_are_crowded_and_decided(name, kind):
    c = C.scatter_case(name, kind)
    cfg = C.SCATTER_CASES[name]
    M, valid = cfg["M"], c["valid"]
    share = _share_left_out(c["f64"], cfg["C"])
    run = C.longest_run(c["f64"], valid)
    print(f"{name} kind {kind}: longest run {run} terms, {share:.2%} of the gradient values left out")
    assert share <= LEFT_OUT_CAP
    assert run > 256                                                      # a run crosses thread, wave and 256-entry boundaries
    assert valid[:, 0].all() and valid[:, -1].all() and int((~valid).sum()) == 3 * cfg["B"]
    # the first and the last box own pixels nobody else touches: losing the terms of either shows
    tp = c["f64"]["taps"]
    for b in range(cfg["B"]):
        for m in (0, M - 1):
            own = np.unique(tp["pix"][b, m][tp["inside"][b, m]])
            rest = [k for k in range(M) if k != m and valid[b, k]]
            assert own.size and not np.intersect1d(own, np.unique(tp["pix"][b, rest][tp["inside"][b, rest]])).size
            assert np.abs(c["f64"]["grad"].reshape(cfg["B"], cfg["C"], -1)[b][:, own]).max() > 0
    terms = 36 * M
    if name == "m56":
        assert terms <= 2048 < 36 * (M + 1)
    if name == "m227":
        assert terms <= 8192 < 36 * (M + 1)
    if name == "m455":
        assert terms <= 16384 < 36 * (M + 1)
    if name == "map_wide":
        tbits = 13
        assert terms <= 1 << tbits and cfg["H"] * cfg["W"] == 1 << (32 - tbits)
    if name.startswith("map"):
        assert int(tp["pix"][0, M - 1][tp["inside"][0, M - 1]].max()) == cfg["H"] * cfg["W"] - 1   # the largest pixel index


@pytest.mark.parametrize("clamp", [1e-4, 1e-3])
@pytest.mark.parametrize("ntasks", [6, 8])
def test_response_cases_hold_their_constructed_pixels(ntasks, clamp):
    c = C.response_case(ntasks, clamp)
    B, HW = C.RESP_B, C.RESP_H * C.RESP_W
    assert HW > 256 and HW % 256 != 0
    assert len(c["s_hm"]) == ntasks and len(c["s_reg"]) == 6 * ntasks
    r = c["f64"]
    flat = lambda x: x.reshape(B, -1, HW)
    dec, arg = r["decision"].reshape(B, HW), r["arg"].reshape(B, HW)
    share = float(r["left_out"].mean())
    print(f"{ntasks} tasks clamp {clamp}: {int(r['left_out'].sum())} of {B * HW} pixels within MARGIN of smax == tmax")
    assert share <= LEFT_OUT_CAP
    first = np.cumsum((0,) + c["ncls"])
    # the tie: two equal maxima in different tasks, the gradient on the first one only
    b, p = C.PIX_TIE
    (t0, c0), (t1, c1) = C.TIE_AT
    assert flat(c["s_hm"][t0])[b, c0, p] == flat(c["s_hm"][t1])[b, c1, p] == np.concatenate([flat(x) for x in c["s_hm"]], 1)[b, :, p].max()
    assert arg[b, p] == first[t0] + c0 and dec[b, p] > 0.1
    assert flat(r["g_hm"][t0])[b, c0, p] > 0 and flat(r["g_hm"][t1])[b, c1, p] == 0
    # smax == tmax on the upper clamp: no gradient
    b, p = C.PIX_EQ
    assert dec[b, p] == 0 and all(not flat(g)[b, :, p].any() for g in r["g_hm"]) and c["mask"].reshape(B, HW)[b, p] > 0
    # every teacher channel on the lower clamp
    b, p = C.PIX_LOW
    smax = max(flat(x)[b, :, p].max() for x in c["s_hm"])
    assert np.isclose(smax - dec[b, p], clamp, rtol=1e-6)
    teacher = np.concatenate([flat(x) for x in c["t_hm"]], 1)
    assert (teacher == 40).sum() > 10 and (teacher == -40).sum() > 10
    b, p = C.PIX_REG
    assert all(not flat(g)[b, :, p].any() for g in r["g_reg"]) and any(flat(g)[b, :, p].any() for g in r["g_hm"])
    for b, p in C.PIX_MASK0:
        assert all(not flat(g)[b, :, p].any() for g in r["g_hm"] + r["g_reg"])
    assert C.PIX_MASK0[0][1] == HW - 1 and C.PIX_MASK0[2][1] == 256       # the last pixel of the ragged workgroup, the first of it


@pytest.mark.parametrize("S", [7, 9, 10])
def test_mask_case_draws_the_boxes_it_claims(S):
    c = C.mask_case(S)
    H, W, r = C.MASK_H, C.MASK_W, C.MASK_R
    assert H != W and C.MASK_PIXEL[0] != C.MASK_PIXEL[1]
    boxes = D.mask_boxes(c["gt"], C.MASK_PC_MIN, C.MASK_PIXEL)
    assert boxes == c["expect"]
    mask = c["mask"]
    one = lambda b, cx, cy: D.gaussian_mask(np.asarray([[C._mask_row(cx, cy, r)]], np.float32), C.MASK_PC_MIN, C.MASK_PIXEL, H, W)[0]
    # outside by less than r and by exactly r: something is drawn; by r + 1 and far: nothing (the window is empty)
    for d, drawn in ((r - 1, True), (r, True), (r + 1, False), (C.FAR, False)):
        for cx, cy in ((-d, 5), (W - 1 + d, 5), (5, -d), (5, H - 1 + d)):
            assert bool(one(0, cx, cy).any()) == drawn, (d, cx, cy)
    g_edge = np.float32(np.exp(-(r * r) / (2 * ((2 * r + 1) / 6) ** 2)))
    assert mask[0, 7, 0] == g_edge and mask[0, 9, W - 1] == g_edge        # exactly r outside: the window's last column at dy = 0
    if S >= 9:
        assert mask[1, 0, 10] == g_edge and mask[1, H - 1, 12] == g_edge
    assert mask[0, 3, 14] == 1.0 and mask[0, 16, 20] == 1.0 and mask[0, 18, 9] == 1.0   # radius 0, dimensions 0, a NaN dimension
    assert np.isnan(c["gt"][0, 10, 3])
    both = np.maximum(one(0, -2, 2), one(0, 1, 4))
    assert (both > 0).sum() < (one(0, -2, 2) > 0).sum() + (one(0, 1, 4) > 0).sum()           # they overlap
    assert (mask[0, :4, :5] == both[:4, :5]).all() and (one(0, -2, 2)[1:4, :2] > 0).all() and (one(0, 1, 4)[1:4, :2] > 0).all()
    # the zero-sum row in the middle: the mask ignores the real boxes after it, `valid` covers them
    assert not c["gt"][1, 9].any() and c["gt"][1, 10].any() and c["gt"][1, 11].any()
    assert mask[1, 10, 20] == 0.0 and mask[1, 12, 6] == 0.0
    assert c["valid"].tolist() == [[True] * 12, [True] * 12, [True] + [False] * 11]
    assert (mask[1, H // 2, W // 2] == 1.0) == (S >= 9)                   # the row that is zero in the seven box columns only
    assert not mask[2].any()
    m1 = C.mask_case_m1()
    assert D.mask_boxes(m1["gt"], C.MASK_PC_MIN, C.MASK_PIXEL) == m1["expect"]
    assert m1["valid"].tolist() == [[True]] * 3 and not m1["mask"][1].any() and m1["mask"][2, 3, 0] == 1.0
