"""CPU: the definition of the rotation / scale / flip test-time-augmentation merge (tests/tta_affine_reference.py) checked
against itself -- pure flips against the flip restatement, constant fields under every value rule, the coverage rule -- and
the view resolution, the per-view parameters and the view builder of ops/tta.py."""
import itertools

import numpy as np
import pytest
import torch

import tta_affine_reference as A
import tta_reference as R

EPS64 = float(np.finfo(np.float64).eps)
ROTS = (0.0, 90.0, 7.5, -7.5, 22.5, 180.0)
SCALES = (0.9, 1.0, 1.1)
FLIPS = ((0, 0), (1, 0), (0, 1), (1, 1))
R_DOUBLE = ((0, 0), (0, 1), (1, 0), (1, 1))


def test_pure_flips_equal_the_flip_restatement():
    """Non-square grid and cells, range symmetric about 0: every subset order of the four flips, all heads, both dim modes."""
    rng = np.random.default_rng(0)
    B, H, W = 2, 5, 7
    pc_range = [-6.0, -4.0, -5.0, 6.0, 4.0, 3.0]
    for views in (((0, 0),), ((1, 0), (0, 0)), R_DOUBLE, ((1, 1), (0, 0), (0, 1), (1, 0))):
        tasks = R.random_maps(rng, len(views) * B, H, W)
        for no_log in (False, True):
            want = R.merge64(tasks, views, no_log)
            got = A.merge64(tasks, views, pc_range, no_log)
            for t in range(len(tasks)):
                for k in want[t]:
                    tol = 16 * EPS64 * np.maximum(np.abs(want[t][k]), float(max(H, W)))
                    assert (np.abs(got[t][k] - want[t][k]) <= tol).all(), (views, no_log, t, k)


def _constant_scene(views, pc_range, H, W, no_log):
    """In the original frame every cell predicts centre = cell centre + delta, z0, dims d0, yaw psi0, velocity v0 and one hm
    probability; each view's maps are the perfect prediction of the transformed scene."""
    delta, z0, d0, psi0, v0, p0, q0 = np.array([0.31, -0.22]), -0.7, np.array([4.2, 1.9, 1.6]), 0.4, np.array([1.5, -2.5]), 0.3, 0.6
    cell = np.array([(pc_range[3] - pc_range[0]) / W, (pc_range[4] - pc_range[1]) / H])
    base = {"hm": np.log(p0 / (1 - p0)), "reg": 0.5 + delta / cell, "height": z0, "dim": d0 if no_log else np.log(d0),
            "rot": np.array([np.sin(psi0), np.cos(psi0)]), "vel": v0, "iou": q0}
    rows = {k: [] for k in base}
    for view in views:
        L, _ = A.linear(view)
        s = A.general(view)[1]
        cs, sn = (L / s) @ np.array([np.cos(psi0), np.sin(psi0)])
        rows["hm"].append(np.array([base["hm"]]))
        rows["reg"].append(0.5 + (L @ delta) / cell)
        rows["height"].append(np.array([s * z0]))
        rows["dim"].append(s * d0 if no_log else np.log(s * d0))
        rows["rot"].append(np.array([sn, cs]))
        rows["vel"].append(L @ v0)
        rows["iou"].append(np.array([q0]))
    stack = {k: np.broadcast_to(np.stack(v)[:, :, None, None], (len(views), len(v[0]), H, W)).copy() for k, v in rows.items()}
    return [stack], {k: np.atleast_1d(v) for k, v in base.items()}


@pytest.mark.parametrize("no_log", [False, True])
@pytest.mark.parametrize("flip", FLIPS, ids=lambda f: f"flip{f[0]}{f[1]}")
def test_constant_field_is_equivariant(flip, no_log):
    """Rotations 0, 90, +-7.5, 22.5, 180 x scales 0.9, 1, 1.1 with one flip state, after the identity; non-square cells,
    asymmetric range: the merge returns the original constants at every pixel.  Pins every value rule and the reg rule."""
    H, W = 9, 11
    pc_range = [-3.0, -10.0, -5.0, 9.0, 6.0, 3.0]
    views = [(0.0, 1.0, 0, 0)] + [(r, s) + flip for r, s in itertools.product(ROTS, SCALES) if (r, s) + flip != (0.0, 1.0, 0, 0)]
    tasks, base = _constant_scene(views, pc_range, H, W, no_log)
    got = A.merge64(tasks, views, pc_range, no_log)[0]
    geo = [A.sample_geometry(T.reshape(-1), H, W)[4] for T, _, _, _ in A.transforms(views, pc_range, H, W)]
    assert sum(g.sum() for g in geo[1:]) > 4 * H * W           # the other views do take part
    for k, v in base.items():
        assert np.abs(got[k] - v[None, :, None, None]).max() <= 1e-12, (k, np.abs(got[k] - v[None, :, None, None]).max())


def test_uncovered_ring_is_the_merge_of_the_other_views():
    rng = np.random.default_rng(3)
    B, H, W = 2, 12, 10
    pc_range = [-5.0, -6.0, -5.0, 5.0, 6.0, 3.0]
    views = [(0.0, 1.0, 0, 0), (0.0, 1.25, 0, 0), (0.0, 1.0, 1, 0)]
    tasks = R.random_maps(rng, len(views) * B, H, W)
    covered = A.sample_geometry(A.transforms(views, pc_range, H, W)[1][0].reshape(-1), H, W)[4]
    ring = ~covered
    assert ring[0].all() and ring[-1].all() and ring[:, 0].all() and ring[:, -1].all() and covered[H // 2, W // 2]
    assert 0.2 < ring.mean() < 0.8
    others = [{k: np.concatenate([a[:B], a[2 * B:]], 0) for k, a in t.items()} for t in tasks]
    for no_log in (False, True):
        got = A.merge64(tasks, views, pc_range, no_log)
        want = A.merge64(others, [views[0], views[2]], pc_range, no_log)
        for t in range(len(tasks)):
            for k in got[t]:
                assert np.array_equal(got[t][k][..., ring], want[t][k][..., ring]), (t, k)
                assert not np.array_equal(got[t][k][..., covered], want[t][k][..., covered]), (t, k)


def test_view_resolution():
    from unidistill_amd.ops import tta
    assert tta.resolve_views("double_flip") == tta.DOUBLE_FLIP
    assert tta.resolve_views([(1, 0), (0, 0)]) == ((1, 0), (0, 0))
    # 4-tuples that are all pure flips, at most four: the flip path's pairs
    assert tta.resolve_views([(0, 1, 0, 0), (0.0, 1.0, 1, 1)]) == ((0, 0), (1, 1))
    got = tta.resolve_views([(0, 0), (7.5, 1, 0, 0), (0, 1.05, True, 0)])
    assert got == ((0.0, 1.0, 0, 0), (7.5, 1.0, 0, 0), (0.0, 1.05, 1, 0)) and all(type(v[0]) is float and type(v[2]) is int for v in got)
    assert len(tta.resolve_views([(0, 1, 0, 0)] * 5)) == 5 and len(tta.resolve_views([(0, 1, 0, 0)] * 5)[0]) == 4
    assert len(tta.resolve_views([(0, 1, 0, 0)] + [(3.0, 1, 0, 0)] * 15)) == 16
    with pytest.raises(ValueError, match="16"):
        tta.resolve_views([(0, 1, 0, 0)] + [(3.0, 1, 0, 0)] * 16)
    with pytest.raises(ValueError):
        tta.resolve_views([(0, 0)] * 5)                                   # pairs alone keep their limit of four
    for bad in ((0, 0.0, 0, 0), (0, -1.0, 0, 0), (0, float("nan"), 0, 0), (0, float("inf"), 0, 0)):
        with pytest.raises(ValueError, match="scale"):
            tta.resolve_views([(0, 1, 0, 0), bad])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rotation"):
            tta.resolve_views([(0, 1, 0, 0), (bad, 1.0, 0, 0)])
    for first in ((5.0, 1.0, 0, 0), (0.0, 1.1, 0, 0), (90.0, 1.0, 1, 0)):
        with pytest.raises(ValueError, match="view 0"):
            tta.resolve_views([first, (0, 1, 0, 0)])
    with pytest.raises(ValueError):
        tta.resolve_views([(0, 1, 0, 0), (1, 2, 3)])
    assert tta.resolve_views([(0, 1, 1, 0), (5.0, 1.0, 0, 0)])[0] == (0.0, 1.0, 1, 0)      # view 0 may be a flip


def test_views_product():
    from unidistill_amd.ops import tta
    assert tta.views() == [(0.0, 1.0) + f for f in tta.DOUBLE_FLIP]
    got = tta.views(rotations=(0, 7.5, -7.5), scales=(1, 0.95), flips=None)
    assert got == [(0.0, 1.0, 0, 0), (0.0, 0.95, 0, 0), (7.5, 1.0, 0, 0), (7.5, 0.95, 0, 0), (-7.5, 1.0, 0, 0), (-7.5, 0.95, 0, 0)]
    assert tta.views(rotations=(0, 12.5), flips=[(0, 0), (1, 0)]) == [(0.0, 1.0, 0, 0), (0.0, 1.0, 1, 0), (12.5, 1.0, 0, 0), (12.5, 1.0, 1, 0)]
    assert tta.resolve_views(got) == tuple(got)
    for kw in ({"rotations": (5, 0)}, {"scales": (1.1, 1.0)}, {"flips": [(1, 0), (0, 0)]}, {"rotations": ()}):
        with pytest.raises(ValueError):
            tta.views(**kw)


def test_affine_params():
    from unidistill_amd.ops import lidar_prep, tta
    views = [(0, 1, 1, 0), (90, 1, 0, 0), (180, 1, 0, 1), (270, 1, 1, 1), (-90, 1, 0, 0), (7.5, 1.1, 0, 1), (0, 0.9, 0, 0)]
    for view in views:
        assert np.abs(tta.view_matrix(view) - lidar_prep.bev_transform_matrix(view[0], view[1], 0, view[2], view[3])).max() <= 4 * EPS64 * view[1]
    # square symmetric grid with a cell that is no binary fraction: flips and quarter turns are exact cell permutations
    H = W = 180
    pc_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    table, ratio = tta.affine_params(views, pc_range, H, W)
    assert ratio == 1.0 and table.shape == (7, 11) and table.dtype == np.float64
    for row in table[:5]:
        assert set(np.abs(row[[0, 1, 3, 4]])) == {0.0, 1.0} and set(row[[2, 5]]) <= {0.0, 180.0} and row[10] == 1.0
        assert np.array_equal(row[[0, 1, 3, 4]].reshape(2, 2) @ row[6:10].reshape(2, 2), np.eye(2))
    want, wratio = A.params_of(views, pc_range, H, W)
    assert np.array_equal(table, want) and ratio == wratio
    # non-square cells, asymmetric range: T = C^-1 A C by the matrices themselves
    pc_range, H, W = [-3.0, -10.0, -5.0, 9.0, 6.0, 3.0], 9, 11
    general = [(0, 1, 0, 0)] + views[1:]
    table, ratio = tta.affine_params(general, pc_range, H, W)
    C = np.array([[12.0 / W, 0, -3.0], [0, 16.0 / H, -10.0], [0, 0, 1]])
    assert abs(ratio - (12.0 / W) / (16.0 / H)) <= 2 * EPS64
    for view, row in zip(general, table):
        Am = tta.view_matrix(view)
        A3 = np.array([[Am[0, 0], Am[0, 1], 0], [Am[1, 0], Am[1, 1], 0], [0, 0, 1]])
        T = np.linalg.inv(C) @ A3 @ C
        assert np.abs(row[:6].reshape(2, 3) - T[:2]).max() <= 1e-13
        assert np.abs(row[6:10].reshape(2, 2) - np.linalg.inv(T[:2, :2])).max() <= 1e-13
    assert np.array_equal(table, A.params_of(general, pc_range, H, W)[0])
    with pytest.raises(ValueError, match="view 0"):
        tta.affine_params([(0, 1, 1, 0), (5, 1, 0, 0)], pc_range, H, W)       # view 0 flips x on a range not symmetric in x


def view_builder_case(device):
    """flip_views with general views on a batch with points, images and a bda_mat (shared with the GPU test)."""
    from unidistill_amd.ops import tta
    g = torch.Generator().manual_seed(0)
    B, N = 2, 50
    points = torch.randn(B, N, 5, generator=g) * 20
    points[:, -7:] = 0                                             # padding rows
    points, bda = points.to(device), torch.randn(B, 4, 4, generator=g).to(device)
    batch = {"points": points, "imgs": torch.randn(B, 1, 1, 3, 4, 4, generator=g).to(device),
             "mats_dict": {"bda_mat": bda, "intrin_mats": torch.randn(B, 1, 1, 4, 4, generator=g).to(device)}, "other": 5}
    views = [(0, 1, 0, 0), (10.0, 1.0, 0, 0), (0, 1.05, 1, 0), (0, 1, 1, 1), (-90, 0.9, 0, 1)]
    out = tta.flip_views(batch, views)
    V = len(views)
    assert out["points"].shape == (V * B, N, 5) and out["imgs"].shape[0] == V * B and out["other"] == 5
    assert out["mats_dict"]["intrin_mats"].shape[0] == V * B and torch.equal(out["mats_dict"]["intrin_mats"][B:2 * B], batch["mats_dict"]["intrin_mats"])
    for v, view in enumerate(views):
        Am = tta.view_matrix(view)
        got = out["points"][v * B:(v + 1) * B]
        want = points[..., :3].double().cpu().numpy() @ Am[:3, :3].T
        assert np.abs(got[..., :3].double().cpu().numpy() - want).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()
        assert torch.equal(got[..., 3:], points[..., 3:])
        assert torch.equal(out["mats_dict"]["bda_mat"][v * B:(v + 1) * B], torch.from_numpy(Am).float().to(device) @ bda)
    # pure-flip views are what flip_views always built, bit for bit (the padding rows' -0 included)
    flips = tta.flip_views(batch, [(0, 0), (1, 1)])
    for a, b in ((0, 0), (3, 1)):
        assert torch.equal(out["points"][a * B:(a + 1) * B].view(torch.int32), flips["points"][b * B:(b + 1) * B].view(torch.int32))
        assert torch.equal(out["mats_dict"]["bda_mat"][a * B:(a + 1) * B], flips["mats_dict"]["bda_mat"][b * B:(b + 1) * B])
    # a list of clouds, and images without a bda_mat
    lst = tta.flip_views({"points": [points[0], points[1, :30]], "imgs": batch["imgs"]}, views)
    assert len(lst["points"]) == V * B and lst["points"][2 * B + 1].shape == (30, 5)
    assert torch.equal(lst["points"][1 * B], out["points"][1 * B])
    assert torch.equal(lst["mats_dict"]["bda_mat"][2 * B], torch.from_numpy(tta.view_matrix(views[2])).float().to(device))


def test_view_builder_on_a_cpu_batch():
    view_builder_case(torch.device("cpu"))
