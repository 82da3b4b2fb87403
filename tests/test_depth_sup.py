"""CPU: the depth-supervision ops refuse CPU tensors, and the float64 restatement the GPU tests compare against
(tests/depth_sup_ref.py) is itself checked: its loss against a hand-expanded example, its near-edge exclusion against a cap."""
import math

import numpy as np
import pytest
import torch

import depth_sup_ref as R
from unidistill_amd import synthetic as syn
from unidistill_amd.ops import depth_sup

D_BOUND, FINAL_DIM, DS = [2.0, 58.0, 0.5], (256, 704), 16
CLOUD_SEED, CLOUD_POINTS, CLOUD_SHORT = 7, 20000, 3000


def random_cloud_case():
    """The input of the GPU test 'random cloud vs restatement': B = 2, 20 000 synthetic LiDAR points per sample, sample 1 is
    3 000 points shorter and zero-padded; a 6-camera rig with a BDA flip + rotation + scale."""
    g = syn.rng(CLOUD_SEED)
    s2e, intrin, ida, bda = syn.camera_rig(g, B=2, ncam=6, bda_aug=True)
    c0, c1 = syn.lidar_cloud(g, CLOUD_POINTS, 1), syn.lidar_cloud(g, CLOUD_POINTS, 1)
    return syn.pad_clouds([c0, c1[:len(c0) - CLOUD_SHORT]]), s2e[:, 0], intrin[:, 0], ida[:, 0], bda


def test_ops_refuse_cpu_tensors():
    pts, s2e, intrin, ida, bda = (torch.from_numpy(a) for a in random_cloud_case())
    with pytest.raises(RuntimeError, match="GPU only"):
        depth_sup.lidar_depth_labels(pts, s2e, intrin, ida, bda, D_BOUND, FINAL_DIM, DS)
    with pytest.raises(RuntimeError, match="GPU only"):
        depth_sup.depth_loss(torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int32))


def test_restatement_loss_matches_hand_expansion():
    """Three bins, three pixels: an ordinary one, one whose labelled bin has log p < -100 (clamped), one where another bin has
    p == 1 in float64, so log(1 - p) = -inf is clamped as well; a fourth pixel without a label does not count."""
    x = torch.tensor([[0.3, -1.2, 2.0], [0.0, -150.0, 1.0], [200.0, 0.0, 0.0], [5.0, 5.0, 5.0]], dtype=torch.float64)
    lab = torch.tensor([2, 1, 1, -1])
    loss, dx = R.depth_loss(x.t().reshape(1, 3, 1, 4), lab.reshape(1, 1, 4))
    e = [math.exp(v) for v in (0.3, -1.2, 2.0)]
    p = [v / sum(e) for v in e]
    pix0 = -math.log(1 - p[0]) - math.log(1 - p[1]) - math.log(p[2])
    s1 = 1.0 + math.exp(-1.0) + math.exp(-151.0)                         # logits - max = (-1, -151, 0)
    pix1 = -math.log(1 - math.exp(-1.0) / s1) + 100.0 - math.log(1 - 1.0 / s1)
    pix2 = 100.0 + 100.0 - math.log(1 - math.exp(-200.0))                # bin 0: log(1 - 1) clamped; bin 1: log p = -200 clamped
    assert abs(float(loss) - (pix0 + pix1 + pix2) / 3) <= 1e-12 * (pix0 + pix1 + pix2)
    assert torch.isfinite(dx).all() and float(dx[0, :, 0, 3].abs().max()) == 0.0
    # no labelled pixel at all: exactly zero, zero gradient
    loss0, dx0 = R.depth_loss(x.t().reshape(1, 3, 1, 4), torch.full((1, 1, 4), -1))
    assert float(loss0) == 0.0 and float(dx0.abs().max()) == 0.0


def test_restatement_marks_few_cells_near_edge():
    """The GPU test excludes the cells the restatement marks near-edge.  At most 2 % of the cells may be excluded, and the input
    must label enough cells to mean something: a condition on the test input, checked here so the exclusion cannot grow."""
    pts, s2e, intrin, ida, bda = random_cloud_case()
    assert pts.shape[0] == 2 and np.all(pts[1, -CLOUD_SHORT:] == 0) and np.any(pts[0, -1] != 0)
    dmin, label, near = R.depth_labels(pts, s2e, intrin, ida, bda, D_BOUND, FINAL_DIM, DS)
    print(f"near-edge cells: {int(near.sum())} of {near.size} ({100.0 * near.mean():.3f} %); labelled {int((label >= 0).sum())}")
    assert near.mean() <= 0.02
    assert ((label >= 0) & ~near).reshape(2, 6, -1).sum(-1).max() > 100
    assert np.array_equal(label >= 0, np.isfinite(dmin) & (dmin < D_BOUND[1]))


def test_restatement_inverts_the_forward_chain():
    """Points built with LSSFPN's forward chain (numpy's own inverse) land in the cell and at the depth they were built from."""
    pts, s2e, intrin, ida, bda = random_cloud_case()
    fH, fW = FINAL_DIM[0] // DS, FINAL_DIM[1] // DS
    v, u = np.meshgrid((np.arange(fH) + 0.5) * DS, (np.arange(fW) + 0.5) * DS, indexing="ij")
    d = np.full(u.size, D_BOUND[0] + 57.5 * D_BOUND[2])
    xyz = R.frustum_points(s2e[1, 4], intrin[1, 4], ida[1, 4], bda[1], u.ravel(), v.ravel(), d)
    P, mz, A = R.camera_projection(s2e[1, 4], intrin[1, 4], ida[1, 4], bda[1])
    uu, vv, dd = R.project(P, mz, A, xyz)
    assert np.abs(uu - u.ravel()).max() < 1e-6 and np.abs(vv - v.ravel()).max() < 1e-6 and np.abs(dd - d).max() < 1e-9
