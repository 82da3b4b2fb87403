"""Writes tests/golden/pillars_<case>.npz from the REFERENCE's own PillarVFE / PFNLayer / PointPillarScatter, run on the CPU.

    python tests/golden/make_pillar_goldens.py /path/to/reference/checkout

The two reference files are pure PyTorch; they are loaded from the checkout by path (no other part of the reference is
imported), run in float64 and in float32, in train mode, in eval mode and with frozen statistics (norm.eval() inside a training
graph).  Arrays only are stored: inputs, weights, float64 outputs and gradients, and per quantity the measured
max |float32 - float64| of the reference itself ("err/<name>"), which the GPU tests use as their tolerance (times 4).  Never
imported by a test.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pillars_reference as R  # noqa: E402

VOXEL = [0.6, 0.6, 8.0]
# name: M, P, C, F, use_absolute_xyz, with_distance, (nx, ny), seed
CASES = {
    "m1": (1, 5, 32, 4, True, False, (12, 20), 11),
    "m63": (63, 20, 64, 5, True, True, (12, 20), 12),
    "m64": (64, 20, 256, 5, True, False, (12, 20), 13),
    "m65": (65, 5, 256, 4, False, True, (12, 20), 14),
    "m65b": (65, 20, 64, 4, False, False, (12, 20), 15),
    "m777": (777, 5, 32, 5, False, False, (20, 28), 16),
}
B = 3
MAX_SKIPPED = 0.01
GY_EMPTY = 0.5


def load_reference(root):
    """PillarVFE, PFNLayer, PointPillarScatter from the checkout's two files, inside a stand-in package for the relative import."""
    vfe_dir = os.path.join(root, "unidistill", "layers", "blocks_3d", "det3d", "vfe")
    bev_dir = os.path.join(root, "unidistill", "layers", "blocks_2d", "det3d", "map_to_bev")
    pkg = types.ModuleType("_ref_vfe")
    pkg.__path__ = [vfe_dir]
    sys.modules["_ref_vfe"] = pkg
    sys.dont_write_bytecode = True

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    load("_ref_vfe.vfe_template", os.path.join(vfe_dir, "vfe_template.py"))
    vfe = load("_ref_vfe.pillar_vfe", os.path.join(vfe_dir, "pillar_vfe.py"))
    sc = load("_ref_scatter", os.path.join(bev_dir, "pointpillar_scatter.py"))
    return vfe.PillarVFE, vfe.PFNLayer, sc.PointPillarScatter


def make_inputs(M, P, F, nx, ny, seed):
    """Pillars of samples 0 and 2 of B = 3 (sample 1 owns none), unique cells, num == 1, num == P and in between."""
    rng = np.random.default_rng(seed)
    pcr = [-VOXEL[0] * nx / 2, -VOXEL[1] * ny / 2, -5.0, VOXEL[0] * nx / 2, VOXEL[1] * ny / 2, 3.0]
    cells = rng.permutation(2 * nx * ny)[:M]
    b = np.where(cells < nx * ny, 0, 2)
    cell = cells % (nx * ny)
    coords = np.stack([b, np.zeros(M, np.int64), cell // nx, cell % nx], 1).astype(np.int32)
    num = rng.integers(1, P + 1, M).astype(np.int32)
    num[rng.random(M) < 0.2] = 1
    num[rng.random(M) < 0.2] = P
    if M == 1:
        num[:] = max(2, P // 2)
    vox = np.zeros((M, P, F), np.float32)
    u = rng.random((M, P, 3))
    vox[:, :, 0] = pcr[0] + (coords[:, 3:4] + u[:, :, 0]) * VOXEL[0]
    vox[:, :, 1] = pcr[1] + (coords[:, 2:3] + u[:, :, 1]) * VOXEL[1]
    vox[:, :, 2] = pcr[2] + u[:, :, 2] * VOXEL[2]
    vox[:, :, 3:] = rng.random((M, P, F - 3))
    vox *= (np.arange(P)[None, :] < num[:, None])[:, :, None]
    return vox, coords, num, pcr, rng


def run_reference(classes, dtype, case, vox, coords, num, pcr, params, gy):
    PillarVFE, _, PointPillarScatter = classes
    M, P, C, F, abs_xyz, dist, (nx, ny), _ = case
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    out = {}
    for mode in ("train", "eval", "frozen"):
        vfe = PillarVFE(use_norm=True, with_distance=dist, use_absolute_xyz=abs_xyz, num_filters=[C], num_point_features=F,
                        voxel_size=VOXEL, point_cloud_range=pcr).to(dtype)
        scatter = PointPillarScatter(C, (nx, ny, 1))
        sd = {"pfn_layers.0.linear.weight": t(params["weight"]), "pfn_layers.0.norm.weight": t(params["gamma"]),
              "pfn_layers.0.norm.bias": t(params["beta"]), "pfn_layers.0.norm.running_mean": t(params["running_mean"]),
              "pfn_layers.0.norm.running_var": t(params["running_var"]),
              "pfn_layers.0.norm.num_batches_tracked": torch.tensor(0)}
        assert list(vfe.state_dict().keys()) == list(sd.keys())
        vfe.load_state_dict(sd)
        vfe.train(mode != "eval")
        if mode == "frozen":
            vfe.pfn_layers[0].norm.eval()
        tc = torch.from_numpy(coords)
        with torch.set_grad_enabled(mode != "eval"):
            feats = vfe(t(vox), tc, torch.from_numpy(num)).reshape(M, C)
            bev = scatter(feats, tc)
            if bev.shape[0] < B:      # M == 1: the reference sizes the batch from the largest sample index present
                bev = torch.cat([bev, bev.new_zeros((B - bev.shape[0],) + tuple(bev.shape[1:]))], 0)
            out[mode + "/feats"] = feats.detach().double().numpy()
            out[mode + "/bev"] = bev.detach().double().numpy()
            if mode != "eval":
                (bev * t(gy)).sum().backward()
                pfn = vfe.pfn_layers[0]
                out[mode + "/dW"] = pfn.linear.weight.grad.double().numpy()
                out[mode + "/dgamma"] = pfn.norm.weight.grad.double().numpy()
                out[mode + "/dbeta"] = pfn.norm.bias.grad.double().numpy()
        if mode == "train":
            out["train/running_mean"] = vfe.pfn_layers[0].norm.running_mean.double().numpy()
            out["train/running_var"] = vfe.pfn_layers[0].norm.running_var.double().numpy()
            out["keys"] = list(vfe.state_dict().keys())
    return out


def tainted_channels(marks):
    return marks.any(0)


def make_case(classes, name, case):
    M, P, C, F, abs_xyz, dist, (nx, ny), seed = case
    K = F + (6 if abs_xyz else 3) + (1 if dist else 0)
    for attempt in range(50):      # the seed is moved until the reference alone stays within the knife-edge cap
        vox, coords, num, pcr, rng = make_inputs(M, P, F, nx, ny, seed + 1000 * attempt)
        bound = 1.0 / np.sqrt(K)
        params = dict(weight=rng.uniform(-bound, bound, (C, K)).astype(np.float32),
                      gamma=rng.uniform(0.5, 1.5, C).astype(np.float32), beta=(0.3 * rng.standard_normal(C)).astype(np.float32),
                      running_mean=(0.3 * rng.standard_normal(C)).astype(np.float32),
                      running_var=rng.uniform(0.5, 2.0, C).astype(np.float32))
        # upstream BEV gradient: seeded values at the pillars' cells (stored as [M, C]), GY_EMPTY at every empty cell
        gy_pillars = rng.standard_normal((M, C)).astype(np.float32)
        gy = R.scatter(gy_pillars, coords, B, ny, nx, fill=GY_EMPTY)
        feat = R.row_features(vox, coords, num, VOXEL, pcr, abs_xyz, dist)
        g64 = params["gamma"].astype(np.float64)
        f_train = R.forward(feat, params["weight"], g64, params["beta"].astype(np.float64))
        f_eval = R.forward(feat, params["weight"], g64, params["beta"].astype(np.float64), params["running_mean"],
                           params["running_var"])
        marks = {"train": R.knife_edges(f_train, num, g64), "frozen": R.knife_edges(f_eval, num, g64)}
        share = max(float(m.mean()) for m in marks.values())
        chan = max(float(tainted_channels(m).mean()) for m in marks.values())
        if share <= MAX_SKIPPED and chan <= MAX_SKIPPED:
            break
    else:
        raise AssertionError(f"{name}: no seed within the knife-edge cap")
    ref64 = run_reference(classes, torch.float64, case, vox, coords, num, pcr, params, gy)
    ref32 = run_reference(classes, torch.float32, case, vox, coords, num, pcr, params, gy)
    assert share <= MAX_SKIPPED and chan <= MAX_SKIPPED, (name, share, chan)
    rec = dict(voxels=vox, coords=coords, num=num, pc_range=np.asarray(pcr), voxel_size=np.asarray(VOXEL), gy_pillars=gy_pillars,
               gy_empty=np.asarray(GY_EMPTY, np.float32),
               cfg=np.asarray([M, P, C, F, int(abs_xyz), int(dist), nx, ny, B], np.int64), keys=np.asarray(ref64["keys"]),
               mark_train=marks["train"], mark_frozen=marks["frozen"], **params)
    for k, v in ref64.items():
        if k == "keys":
            continue
        if k == "eval/bev":                    # the scatter of eval/feats: checked, not stored (file size)
            assert np.array_equal(v, R.scatter(ref64["eval/feats"], coords, B, ny, nx))
        elif k == "frozen/feats" or k == "frozen/bev":
            assert np.array_equal(v, ref64[k.replace("frozen", "eval")])
        else:
            rec[k] = v
        if k not in ("frozen/feats", "frozen/bev"):
            rec["err/" + k] = np.asarray(np.abs(ref32[k] - v).max())
    np.savez_compressed(os.path.join(HERE, f"pillars_{name}.npz"), **rec)
    size = os.path.getsize(os.path.join(HERE, f"pillars_{name}.npz"))
    print(f"pillars_{name}.npz: {size} bytes, seed attempt {attempt}, marked share {share:.2e}, "
          + ", ".join(f"{k[4:]} {float(v):.2e}" for k, v in rec.items() if k.startswith("err/")))
    assert size < 1 << 20


def main():
    torch.set_num_threads(1)
    classes = load_reference(sys.argv[1])
    for name, case in CASES.items():
        make_case(classes, name, case)


if __name__ == "__main__":
    main()
