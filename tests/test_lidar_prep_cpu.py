"""CPU: the loader side of the LiDAR input chain (ops/input_prep.py CollectLidarSweeps / BevAffineTransformation /
ObjectRangeFilter) against the reference golden tests/golden/lidar_chain.npz -- seeded BDA draws, host box transform
and box / label filtering, bda_mat, the recorded device plans -- plus a numpy evaluation of exactly the arithmetic
ud_lidar_prep_* does from those plans, which must give the golden's points bit for bit.  The C entry points reject bad
plans on the host before anything is launched.

The golden comes from the reference's own Compose([CollectLidarSweeps(), BevAffineTransformation(...),
ObjectRangeFilter(...)]) (eval sample: no BDA) under np.random.seed(SEED), on the stand-ins of
tests/golden/_ref_import.py.  Regenerate it where the reference tree is available:
    UNIDISTILL_REF=<reference checkout> python tests/test_lidar_prep_cpu.py"""
import copy
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BDA_CONF = dict(rot_lim=(-45.0, 45.0), scale_lim=(0.90, 1.10), trans_lim=(0.5, 0.5, 0.5), flip_dx_ratio=0.5,
                flip_dy_ratio=0.5)                                                 # base_nuscenes_cfg.py bda_aug_cfg
PCR = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]                                        # base_nuscenes_cfg.py
SEED = 20231017
N_SAMPLES = 4                      # 0..2 training (BDA), 3 eval (no BDA)
TRAIN = (True, True, True, False)
WITH_IMGS = (True, False, True, False)
NAMES = np.array(["car", "truck", "pedestrian", "barrier", "bicycle"])


def _pose(rng):
    a = rng.uniform(-np.pi, np.pi)
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    m[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    m[:3, 3] = rng.normal(scale=[300.0, 300.0, 1.0])
    return m


def _cloud(rng, n, scale=30.0, shift=0.0):
    p = np.zeros((n, 5), np.float32)
    p[:, :2] = rng.normal(scale=scale, size=(n, 2)) + shift
    p[:, 2] = rng.normal(scale=2.0, size=n)
    p[:, 3] = rng.integers(0, 256, size=n)
    p[:, 4] = rng.integers(0, 32, size=n)                                         # ring: replaced by the time lag
    return p


def _edge_points():
    """Key-frame rows of the eval sample (no BDA: they reach the range test unchanged)."""
    up, dn = (lambda v: np.nextafter(np.float32(v), np.float32(np.inf))), (lambda v: np.nextafter(np.float32(v),
                                                                                                  np.float32(-np.inf)))
    nan = np.float32(np.nan)
    xy = [(-54.0, 0.0), (54.0, 0.0), (0.0, -54.0), (0.0, 54.0), (-54.0, -54.0), (54.0, 54.0),      # on the bounds
          (dn(-54.0), 0.0), (up(54.0), 0.0), (0.0, dn(-54.0)), (0.0, up(54.0)),                   # 1 ulp outside
          (nan, 0.0), (0.0, nan), (np.float32(np.inf), 0.0), (-0.0, -0.0), (-0.0, 1.5)]
    p = np.zeros((len(xy) + 2, 5), np.float32)
    p[:len(xy), :2] = xy
    p[:len(xy), 3] = 7.0
    p[len(xy)] = (1.0, 2.0, 40.0, 1.0, 3.0)                                        # z far out of range: kept
    p[len(xy) + 1] = (-0.0, 3.0, -0.0, -0.0, 9.0)                                  # -0.0 everywhere
    return p


def _boxes(rng, m, far=False):
    b = np.zeros((m, 9), np.float32)
    b[:, :2] = rng.uniform(-70, 70, size=(m, 2)) + (300.0 if far else 0.0)
    b[:, 2] = rng.uniform(-2, 1, size=m)
    b[:, 3:6] = rng.uniform(0.5, 5.0, size=(m, 3))
    b[:, 6] = rng.uniform(-np.pi, np.pi, size=m)
    b[:, 7:9] = rng.normal(scale=3.0, size=(m, 2))
    return b


def make_inputs():
    """The four samples' raw inputs (closed form from a fixed default_rng stream, stored in the golden too)."""
    rng = np.random.default_rng(4242)
    samples = []
    sizes = [[3000, 2500, 0, 2200], [2600, 2400, 1900], [2000, 1800], [2800, 2000, 1700]]
    for k in range(N_SAMPLES):
        key_l2e, key_e2g = _pose(rng), _pose(rng)
        key_l2e[:3, 3] = [0.94, 0.0, 1.84]
        ts = 1533151603547590 + k * 500000
        far = k == 2                                                               # every point out of range
        pts = _cloud(rng, sizes[k][0], shift=400.0 if far else 0.0)
        if k == 3:
            pts = np.concatenate([_edge_points(), pts])
        sweeps, infos = [], []
        for j, n in enumerate(sizes[k][1:]):
            pose = key_e2g.copy()
            pose[:3, 3] += rng.normal(scale=[2.0, 2.0, 0.05])
            sweeps.append(_cloud(rng, n, shift=400.0 if far else 0.0))
            infos.append({"sweep_lidar_to_ego": pose, "sweep_lidar_timestamp": ts - 50000 * (j + 1) - 123})
        if k == 1:
            boxes = np.zeros((0, 9), np.float32)                                    # zero boxes
        elif k == 3:
            boxes = np.concatenate([_boxes(rng, 6), np.array([
                [55.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0],                     # 4 corners on x = 54: kept
                [55.0, 55.0, 4.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0],                    # exactly one corner inside: kept
                [np.nextafter(np.float32(55.0), np.float32(99)), 0.0, 0.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0],  # out
                [0.0, 0.0, 9.0, 2.0, 2.0, 2.0, 0.3, 0.0, 0.0]], np.float32),      # above the z range: out
                _boxes(rng, 3, far=True)])                                         # entirely outside
        else:
            boxes = np.concatenate([_boxes(rng, 12), _boxes(rng, 2, far=True)])
        labels = rng.integers(0, 5, size=len(boxes)).astype(np.int64)
        samples.append({"points": pts, "sweep_points": sweeps, "gt_boxes": boxes, "gt_labels": labels,
                        "gt_names": NAMES[labels],
                        "info": {"ego_to_global": key_e2g, "lidar_to_ego": key_l2e, "timestamp": ts,
                                 "sweep_lidar_infos": infos}})
    return samples


def data_dicts(g):
    """The samples' input data_dicts from the golden (fresh copies)."""
    out = []
    for k in range(N_SAMPLES):
        p = f"s{k}_"
        ns = int(g[p + "nsweeps"])
        infos = [{"sweep_lidar_to_ego": g[p + f"sweep{j}_pose"], "sweep_lidar_timestamp": int(g[p + f"sweep{j}_ts"])}
                 for j in range(ns)]
        d = {"points": g[p + "key"].copy(), "sweep_points": [g[p + f"sweep{j}"].copy() for j in range(ns)],
             "gt_boxes": g[p + "boxes_in"].copy(), "gt_labels": g[p + "labels_in"].copy(),
             "gt_names": g[p + "names_in"].copy(),
             "info": {"ego_to_global": g[p + "e2g"], "lidar_to_ego": g[p + "l2e"], "timestamp": int(g[p + "ts"]),
                      "sweep_lidar_infos": infos}}
        if WITH_IMGS[k]:
            d["imgs"] = {"CAM_FRONT": np.zeros((2, 2, 3), np.uint8)}
        out.append(d)
    return out


def pipeline(mod, train):
    ts = [mod.CollectLidarSweeps()]
    if train:
        ts.append(mod.BevAffineTransformation(**BDA_CONF))
    ts.append(mod.ObjectRangeFilter(PCR))
    return ts


def run_loader_side(g):
    """Our loader-side classes over the golden's samples under the seed, in the reference's Compose convention."""
    from unidistill_amd.ops import input_prep as ip
    np.random.seed(SEED)
    outs = []
    for k, d in enumerate(data_dicts(g)):
        for t in pipeline(ip, TRAIN[k]):                                           # transforms3d.Compose.forward
            d = t(d)
        outs.append(d)
    return outs


def emulate_device(clouds, aug):
    """numpy evaluation of ud_lidar_prep_*'s arithmetic from a lidar_aug record: per row ((m0 x + m1 y) + m2 z) + m3
    in float64 rounded to float32 (sweeps), the same with the BDA matrix on that result, float32 range test."""
    D = clouds[0].shape[1]

    def xf(p, m):
        x, y, z = (p[:, i].astype(np.float64) for i in range(3))
        return np.stack([(((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3]) for k in range(3)], 1).astype(
            np.float32)
    rows = []
    for s, c in enumerate(clouds):
        r = c.copy()
        if s > 0:
            r[:, :3] = xf(c, aug["sweep_mats"][s - 1])
        if D == 5:
            r[:, 4] = 0.0 if s == 0 else aug["time_lags"][s - 1]
        rows.append(r)
    r = np.concatenate(rows)
    if aug["bda_mat"] is not None:
        r[:, :3] = xf(r, aug["bda_mat"])
    if aug["range"] is not None:
        q = aug["range"]
        with np.errstate(invalid="ignore"):
            r = r[(r[:, 0] >= q[0]) & (r[:, 0] <= q[3]) & (r[:, 1] >= q[1]) & (r[:, 1] <= q[4])]
    return r


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_golden_covers_the_edge_cases(golden):
    g = golden("lidar_chain")
    counts = [len(g[f"s{k}_points"]) for k in range(N_SAMPLES)]
    assert counts[2] == 0 and all(c > 0 for k, c in enumerate(counts) if k != 2)   # one sample fully outside
    assert len(g["s1_boxes_in"]) == 0 and len(g["s3_boxes"]) < len(g["s3_boxes_in"])
    assert any(len(g[f"s{k}_sweep{j}"]) == 0 for k in range(N_SAMPLES) for j in range(int(g[f"s{k}_nsweeps"])))
    p3 = g["s3_points"]
    assert np.signbit(p3[:, 0]).any() and (p3[:, 2] == 40.0).any()                # -0.0 and z out of range survive
    assert not np.isnan(p3).any() and (p3[:, 0] == 54.0).any() and (p3[:, 1] == -54.0).any()
    assert os.path.getsize(os.path.join(HERE, "golden", "lidar_chain.npz")) < 1 << 20


def test_bda_draws_match_reference(golden):
    from unidistill_amd.ops import input_prep as ip
    g = golden("lidar_chain")
    np.random.seed(SEED)
    t = ip.BevAffineTransformation(**BDA_CONF)
    for k in range(3):
        rot, scale, trans, fx, fy = t.sample_augs()
        want = g[f"s{k}_augs"]
        got = np.array([rot, scale, *trans, float(fx), float(fy)], np.float64)
        np.testing.assert_array_equal(bits(got), bits(want))


def test_boxes_labels_and_bda_mat_match_reference(golden):
    g = golden("lidar_chain")
    for k, d in enumerate(run_loader_side(g)):
        p = f"s{k}_"
        np.testing.assert_array_equal(bits(d["gt_boxes"]), bits(g[p + "boxes"]))
        assert d["gt_boxes"].dtype == np.float32 and d["gt_boxes"].shape == g[p + "boxes"].shape
        np.testing.assert_array_equal(d["gt_labels"], g[p + "labels"])
        np.testing.assert_array_equal(d["gt_names"], g[p + "names"])
        if WITH_IMGS[k] and TRAIN[k]:
            np.testing.assert_array_equal(bits(d["bda_mat"]), bits(g[p + "bda_mat"]))
        else:
            assert "bda_mat" not in d                                             # no imgs (or eval): not stored
        assert "sweep_lidar_infos" not in d["info"]


def test_recorded_plans(golden):
    from unidistill_amd.ops import input_prep as ip
    g = golden("lidar_chain")
    for k, d in enumerate(run_loader_side(g)):
        p = f"s{k}_"
        a = d["lidar_aug"]
        ns = int(g[p + "nsweeps"])
        np.testing.assert_array_equal(d["points"], g[p + "key"])                  # clouds stay raw
        assert len(d["sweep_points"]) == ns
        assert a["segments"] == [len(g[p + "key"])] + [len(g[p + f"sweep{j}"]) for j in range(ns)]
        for j in range(ns):
            m = ip.sweep_to_key_matrix(g[p + "l2e"], g[p + "e2g"], g[p + f"sweep{j}_pose"])
            np.testing.assert_array_equal(bits(a["sweep_mats"][j]), bits(m))
            assert a["time_lags"].dtype == np.float32
            assert a["time_lags"][j] == np.float32((int(g[p + "ts"]) - int(g[p + f"sweep{j}_ts"])) / 1e6)
        if TRAIN[k]:
            np.testing.assert_array_equal(bits(a["bda_mat"]), bits(g[p + "bda_mat"]))
        else:
            assert a["bda_mat"] is None
        np.testing.assert_array_equal(a["range"], np.array(PCR, np.float32))


def test_device_arithmetic_from_plans_reproduces_golden_points(golden):
    """What the kernels compute, evaluated in numpy from the recorded plans, equals the reference's points."""
    g = golden("lidar_chain")
    for k, d in enumerate(run_loader_side(g)):
        got = emulate_device([d["points"]] + list(d["sweep_points"]), d["lidar_aug"])
        want = g[f"s{k}_points"]
        assert got.shape == want.shape
        np.testing.assert_array_equal(bits(got), bits(want))


def test_runs_in_reference_compose_convention():
    """A Compose-like loop over the three classes (``data_dict = t(data_dict)``); no points: boxes only."""
    from unidistill_amd.ops import input_prep as ip
    np.random.seed(0)
    d = {"gt_boxes": np.array([[0, 0, 0, 1, 1, 1, 0], [90, 0, 0, 1, 1, 1, 0]], np.float32),
         "gt_labels": np.array([1, 2])}
    for t in [ip.BevAffineTransformation(**dict(BDA_CONF, rot_lim=(0.0, 0.0), trans_lim=(0.0, 0.0, 0.0),
                                                flip_dx_ratio=0.0, flip_dy_ratio=0.0, scale_lim=(1.0, 1.0))),
              ip.ObjectRangeFilter(PCR)]:
        d = t(d)
    assert "lidar_aug" not in d and "bda_mat" not in d
    np.testing.assert_array_equal(d["gt_labels"], [1])
    # a lone key frame without CollectLidarSweeps still gets a plan
    d = ip.ObjectRangeFilter(PCR)({"points": np.zeros((3, 4), np.float32), "gt_boxes": np.zeros((0, 7), np.float32)})
    assert d["lidar_aug"]["segments"] == [3] and len(d["lidar_aug"]["sweep_mats"]) == 0
    with pytest.raises(ValueError):                                               # range before BDA: refused
        ip.BevAffineTransformation(**BDA_CONF)(d)


def test_plan_validation_errors():
    from unidistill_amd.ops import input_prep as ip
    c = [np.zeros((4, 5), np.float32), np.zeros((2, 5), np.float32)]
    aug = {"segments": [4, 2], "sweep_mats": np.eye(4)[None], "time_lags": np.zeros(1, np.float32),
           "bda_mat": None, "range": None}
    with pytest.raises(RuntimeError, match="GPU only"):
        ip.lidar_prep_host_clouds([c], [aug], "cpu")
    with pytest.raises(ValueError):                                               # segments do not match
        ip.lidar_prep_host_clouds([c], [dict(aug, segments=[4, 3])], "cuda")
    with pytest.raises(ValueError):                                               # dtype
        ip.lidar_prep_host_clouds([[x.astype(np.float64) for x in c]], [aug], "cuda")
    with pytest.raises(ValueError):                                               # D < 3
        ip.lidar_prep_host_clouds([[np.zeros((4, 2), np.float32)]], [None], "cuda")
    with pytest.raises(ValueError):                                               # sweep matrices missing
        ip.lidar_prep_host_clouds([c], [dict(aug, sweep_mats=np.zeros((0, 4, 4)))], "cuda")


def test_c_entry_points_reject_bad_plans(hip_lib):
    """The launchers validate the plan on the host before any launch: every call here fails in that check (no device
    pointer is ever dereferenced; the dummy addresses are never reached)."""
    i64 = lambda v: np.ascontiguousarray(np.asarray(v, np.int64))
    seg, sseg = i64([0, 4, 6]), i64([0, 2])
    fake = 1 << 40                                                                 # never dereferenced

    def count(seg=seg, sseg=sseg, S=2, B=1, D=5, rows=6, pts=fake, seg_dev=fake, par=fake, counts=fake):
        return hip_lib.ud_lidar_prep_count(pts, rows, D, seg.ctypes.data, sseg.ctypes.data, S, B, seg_dev, fake, par,
                                           fake, counts, None, 0, None)

    def compact(counts_host=i64([3]), nmax=3, out_rows=3, out=fake, compact=0, D=5, seg=seg):
        return hip_lib.ud_lidar_prep_compact(fake, 6, D, seg.ctypes.data, sseg.ctypes.data, 2, 1, fake, fake, fake,
                                             fake, counts_host.ctypes.data, fake, nmax, compact, out, out_rows, None, 0,
                                             None)
    assert count(seg=i64([0, 4, 3])) == -1                                        # offsets not monotonic
    assert count(seg=i64([0, 4, 9])) == -1                                        # past the rows
    assert count(sseg=i64([0, 1])) == -1                                          # samples do not cover the segments
    assert count(D=2) == -1                                                       # D < 3
    assert count(pts=None) == -1                                                  # null with rows > 0
    assert count(seg_dev=None) == -1 and count(par=None) == -1 and count(counts=None) == -1
    many = 65
    assert count(seg=i64(np.zeros(many + 1)), sseg=i64([0, many]), S=many, rows=0) == -1   # too many segments
    assert count(B=70000, sseg=i64(np.zeros(70001))) == -1
    assert hip_lib.ud_lidar_prep_count(fake, 6, 5, None, sseg.ctypes.data, 2, 1, fake, fake, fake, fake, fake, None, 0,
                                       None) == -1                                # null host offsets
    assert count() == -2                                                          # a valid plan, but no workspace
    assert compact(counts_host=i64([7])) == -1                                    # more kept rows than rows
    assert compact(nmax=2) == -1                                                  # nmax below a count
    assert compact(out_rows=2) == -1                                              # output too small
    assert compact(out=None) == -1
    assert compact(D=1) == -1
    assert compact() == -2                                                        # valid, no workspace
    assert hip_lib.ud_lidar_prep_workspace_bytes(seg.ctypes.data, sseg.ctypes.data, 2, 1) > 0
    assert hip_lib.ud_lidar_prep_workspace_bytes(i64([0, 4, 3]).ctypes.data, sseg.ctypes.data, 2, 1) == 0
    # an empty batch is a no-op, not an error
    assert hip_lib.ud_lidar_prep_count(None, 0, 5, i64([0]).ctypes.data, i64([0]).ctypes.data, 0, 0, None, None, None,
                                       None, None, None, 0, None) == 0


def write_golden(ref):
    """Reference side: transforms3d.Compose([CollectLidarSweeps(), BevAffineTransformation(**BDA_CONF),
    ObjectRangeFilter(PCR)]) per training sample, without the BDA for the eval sample, under np.random.seed(SEED)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import _ref_import
    _ref_import.REF_ROOT = ref
    _ref_import.install()
    from unidistill.data.multisensorfusion import transforms3d as T
    draws = []

    class Recording(T.BevAffineTransformation):
        def sample_augs(self):
            a = super().sample_augs()
            draws.append(np.array([a[0], a[1], *a[2], float(a[3]), float(a[4])], np.float64))
            return a
    T_rec = types.SimpleNamespace(CollectLidarSweeps=T.CollectLidarSweeps, BevAffineTransformation=Recording,
                                  ObjectRangeFilter=T.ObjectRangeFilter)
    out = {}
    samples = make_inputs()
    np.random.seed(SEED)
    for k, s in enumerate(samples):
        p = f"s{k}_"
        out[p + "key"], out[p + "nsweeps"] = s["points"], np.array(len(s["sweep_points"]))
        for j, (c, inf) in enumerate(zip(s["sweep_points"], s["info"]["sweep_lidar_infos"])):
            out[p + f"sweep{j}"], out[p + f"sweep{j}_pose"] = c, inf["sweep_lidar_to_ego"]
            out[p + f"sweep{j}_ts"] = np.array(inf["sweep_lidar_timestamp"], np.int64)
        out[p + "l2e"], out[p + "e2g"] = s["info"]["lidar_to_ego"], s["info"]["ego_to_global"]
        out[p + "ts"] = np.array(s["info"]["timestamp"], np.int64)
        out[p + "boxes_in"], out[p + "labels_in"], out[p + "names_in"] = s["gt_boxes"], s["gt_labels"], s["gt_names"]
        d = copy.deepcopy(s)
        if WITH_IMGS[k]:
            d["imgs"] = {"CAM_FRONT": np.zeros((2, 2, 3), np.uint8)}
        d = T.Compose(pipeline(T_rec, TRAIN[k])).forward(d)
        out[p + "points"], out[p + "boxes"] = d["points"], d["gt_boxes"]
        out[p + "labels"], out[p + "names"] = d["gt_labels"], d["gt_names"]
        if TRAIN[k]:
            out[p + "augs"] = draws[-1]
            from unidistill.data.multisensorfusion.functional import bev_transform
            a = draws[-1]
            out[p + "bda_mat"] = bev_transform(np.zeros((0, 7), np.float32), a[0], a[1], a[2:5], bool(a[5]),
                                               bool(a[6]))[1]
            if WITH_IMGS[k]:
                assert np.array_equal(d["bda_mat"], out[p + "bda_mat"])
    path = os.path.join(HERE, "golden", "lidar_chain.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)", [len(out[f"s{k}_points"]) for k in range(4)])


if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd")]
    os.environ.setdefault("UD_RANDOM_INIT", "1")
    write_golden(os.environ["UNIDISTILL_REF"])
