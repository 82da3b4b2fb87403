"""CPU: the numpy float64 restatement of the PointPillars encoder (tests/pillars_reference.py) against the reference modules' own
float64 output (tests/golden/pillars_*.npz, written by tests/golden/make_pillar_goldens.py), to 1e-12 relative."""
import glob
import os

import numpy as np
import pytest

import pillars_reference as R
from conftest import GOLDEN

CASES = sorted(os.path.basename(p)[len("pillars_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "pillars_*.npz")))


def _close(got, ref, what):
    tol = 1e-12 * max(float(np.abs(ref).max()), 1e-300)
    assert float(np.abs(got - ref).max()) <= tol, (what, float(np.abs(got - ref).max()), tol)


def test_all_cases_present():
    assert CASES == ["m1", "m63", "m64", "m65", "m65b", "m777"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_float64(golden, name):
    g = golden("pillars_" + name)
    M, P, C, F, abs_xyz, dist, nx, ny, B = (int(v) for v in g["cfg"])
    coords, num = g["coords"], g["num"]
    gamma, beta = g["gamma"].astype(np.float64), g["beta"].astype(np.float64)
    feat = R.row_features(g["voxels"], coords, num, g["voxel_size"], g["pc_range"], bool(abs_xyz), bool(dist))
    assert feat.shape == (M, P, g["weight"].shape[1])
    gy = R.scatter(g["gy_pillars"], coords, B, ny, nx, fill=float(g["gy_empty"]))
    tr = R.forward(feat, g["weight"], gamma, beta)
    _close(tr["out"], g["train/feats"], "train features")
    _close(R.scatter(tr["out"], coords, B, ny, nx), g["train/bev"], "train BEV map")
    rm, rv = R.running_update(g["running_mean"].astype(np.float64), g["running_var"].astype(np.float64), tr["mean"], tr["var"], M * P)
    _close(rm, g["train/running_mean"], "running mean")
    _close(rv, g["train/running_var"], "running var")
    ev = R.forward(feat, g["weight"], gamma, beta, g["running_mean"], g["running_var"])
    _close(ev["out"], g["eval/feats"], "eval features")
    for mode, fwd in (("train", tr), ("frozen", ev)):
        assert float(g["mark_" + mode].mean()) <= 0.01
        assert np.array_equal(R.knife_edges(fwd, num, gamma), g["mark_" + mode])
        dW, dg, db = R.backward(feat, g["weight"], gamma, fwd, gy, coords, frozen=mode == "frozen")
        _close(dW, g[mode + "/dW"], mode + " dW")
        _close(dg, g[mode + "/dgamma"], mode + " dgamma")
        _close(db, g[mode + "/dbeta"], mode + " dbeta")
