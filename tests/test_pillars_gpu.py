"""GPU: the PointPillars encoder (csrc/pillars.hip, ops/pillars.py, layers/pillars.py) against the reference modules' own
float64 output (tests/golden/pillars_*.npz).

Tolerance: per quantity, 4 x the golden's measured max |reference float32 - reference float64| ("err/<name>"; the margin covers a
different but fixed summation order).  (Pillar, channel) elements the generator marked as ReLU / max knife edges taint their channel's
argmax-dependent gradients, which are skipped; at most 1 % may be skipped.
Measured worst kernel error / tolerance per case: see DESIGN 2.26."""
import numpy as np
import pytest
import torch

import pillars_reference as R

pytestmark = pytest.mark.gpu

CASES = ["m1", "m63", "m64", "m65", "m65b", "m777"]


def _cfg(g):
    M, P, C, F, abs_xyz, dist, nx, ny, B = (int(v) for v in g["cfg"])
    return M, P, C, F, bool(abs_xyz), bool(dist), nx, ny, B


def _modules(g, with_weights=True):
    from unidistill_amd.layers.pillars import PillarVFE, PointPillarScatter
    M, P, C, F, abs_xyz, dist, nx, ny, B = _cfg(g)
    vfe = PillarVFE(use_norm=True, with_distance=dist, use_absolute_xyz=abs_xyz, num_filters=[C], num_point_features=F,
                    voxel_size=[float(v) for v in g["voxel_size"]], point_cloud_range=[float(v) for v in g["pc_range"]])
    sc = PointPillarScatter(C, (nx, ny, 1))
    if with_weights:
        sd = {"pfn_layers.0.linear.weight": g["weight"], "pfn_layers.0.norm.weight": g["gamma"], "pfn_layers.0.norm.bias": g["beta"],
              "pfn_layers.0.norm.running_mean": g["running_mean"], "pfn_layers.0.norm.running_var": g["running_var"]}
        res = vfe.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
        assert not res.unexpected_keys and not [k for k in res.missing_keys if not k.endswith("num_batches_tracked")]
    return vfe.cuda(), sc


def _inputs(g):
    c = lambda k: torch.from_numpy(g[k]).cuda()
    M, P, C, F, abs_xyz, dist, nx, ny, B = _cfg(g)
    gy = torch.from_numpy(R.scatter(g["gy_pillars"], g["coords"], B, ny, nx, fill=float(g["gy_empty"]))).cuda()
    return c("voxels"), c("coords"), c("num"), gy


def _check(got, g, key, what, keep=None, ref=None):
    ref, tol = g[key] if ref is None else ref, 4.0 * float(g["err/" + key])
    got = got.detach().double().cpu().numpy()
    if keep is not None:
        got, ref = got[keep], ref[keep]
    err = float(np.abs(got - ref).max())
    print(f"{what}: max error {err:.3e}, tolerance {tol:.3e} (4 x reference fp32 error), max |ref| {float(np.abs(ref).max()):.3e}")
    assert err <= tol, (what, err, tol)


def _grads(vfe):
    pfn = vfe.pfn_layers[0]
    return pfn.linear.weight.grad, pfn.norm.weight.grad, pfn.norm.bias.grad


@pytest.mark.parametrize("name", CASES)
def test_forward_backward_vs_goldens(golden, hip_lib, name):
    g = golden("pillars_" + name)
    M, P, C, F, abs_xyz, dist, nx, ny, B = _cfg(g)
    vox, coords, num, gy = _inputs(g)
    # train: batch statistics
    vfe, _ = _modules(g)
    vfe.train()
    bev, feats = vfe.encode(vox, coords, num, B, ny, nx, return_pillars=True)
    assert bev.shape == (B, C, ny, nx) and feats.shape == (M, C)
    bev.backward(gy)
    _check(feats, g, "train/feats", name + " train features")
    _check(bev, g, "train/bev", name + " train BEV map")
    norm = vfe.pfn_layers[0].norm
    _check(norm.running_mean, g, "train/running_mean", name + " running mean")
    _check(norm.running_var, g, "train/running_var", name + " running var")
    assert int(norm.num_batches_tracked) == 1
    for mode in ("train", "frozen"):
        if mode == "frozen":          # running statistics inside a training graph
            vfe, _ = _modules(g)
            vfe.train()
            vfe.pfn_layers[0].norm.eval()
            bev = vfe.encode(vox, coords, num, B, ny, nx)
            bev.backward(gy)
            _check(bev.permute(0, 2, 3, 1)[coords[:, 0].long(), coords[:, 2].long(), coords[:, 3].long()], g, "eval/feats",
                   name + " frozen-statistics features")
            assert torch.equal(vfe.pfn_layers[0].norm.running_mean.cpu(), torch.from_numpy(g["running_mean"]))
        marks = g["mark_" + mode]
        share = float(marks.mean())
        keep = ~marks.any(0)
        print(f"{name} {mode}: marked share {share:.2e}, channels skipped {int((~keep).sum())} of {C}")
        assert share <= 0.01 and float((~keep).mean()) <= 0.01
        dW, dg, db = _grads(vfe)
        _check(dW, g, mode + "/dW", f"{name} {mode} dW", keep)
        _check(dg, g, mode + "/dgamma", f"{name} {mode} dgamma", keep)
        _check(db, g, mode + "/dbeta", f"{name} {mode} dbeta", keep)
    # eval
    vfe, _ = _modules(g)
    vfe.eval()
    with torch.no_grad():
        bev, feats = vfe.encode(vox, coords, num, B, ny, nx, return_pillars=True)
    _check(feats, g, "eval/feats", name + " eval features")
    # eval/bev is not stored (file size): it is the scatter of eval/feats, which the generator asserted on the reference
    _check(bev, g, "eval/bev", name + " eval BEV map", ref=R.scatter(g["eval/feats"], g["coords"], B, ny, nx))


@pytest.mark.parametrize("name", CASES)
def test_untouched_cells_and_scatter_placement(golden, hip_lib, name):
    g = golden("pillars_" + name)
    M, P, C, F, abs_xyz, dist, nx, ny, B = _cfg(g)
    vox, coords, num, _ = _inputs(g)
    for train in (True, False):
        vfe, sc = _modules(g)
        vfe.train(train)
        with torch.no_grad():
            bev, feats = vfe.encode(vox, coords, num, B, ny, nx, return_pillars=True)
        put = torch.zeros((B, C, ny, nx), device="cuda")
        put[coords[:, 0].long(), :, coords[:, 2].long(), coords[:, 3].long()] = feats
        assert torch.equal(bev, put), "the scatter is an index-put of the [M, C] features, bit for bit"
        occupied = torch.zeros((B, ny, nx), dtype=torch.bool, device="cuda")
        occupied[coords[:, 0].long(), coords[:, 2].long(), coords[:, 3].long()] = True
        assert int(occupied.sum()) == M and not occupied[1].any()              # sample 1 owns no pillar
        assert float(bev.permute(0, 2, 3, 1)[~occupied].abs().max()) == 0.0
        assert bev.permute(0, 2, 3, 1).is_contiguous()                         # the layout LidarEncoder returns
        # the two modules called as the reference calls them: fused through vfe.fuse, and unfused through the sparse scatter
        with torch.no_grad():
            vfe2, sc2 = _modules(g)
            vfe2.train(train)
            assert torch.equal(sc2(vfe2(vox, coords, num), coords, batch_size=B), bev)
            vfe3, sc3 = _modules(g)
            vfe3.train(train).fuse(sc3)
            assert torch.equal(sc3(vfe3(vox, coords, num, batch_size=B), coords), bev)


@pytest.mark.parametrize("name", CASES)
def test_reproducible_and_independent_of_pillar_order(golden, hip_lib, name):
    g = golden("pillars_" + name)
    M, P, C, F, abs_xyz, dist, nx, ny, B = _cfg(g)
    vox, coords, num, gy = _inputs(g)
    runs = []
    for _ in range(2):
        vfe, _ = _modules(g)
        vfe.train()
        bev = vfe.encode(vox, coords, num, B, ny, nx)
        bev.backward(gy)
        runs.append([bev.detach().clone()] + [t.clone() for t in _grads(vfe)]
                    + [vfe.pfn_layers[0].norm.running_mean.clone(), vfe.pfn_layers[0].norm.running_var.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    vfe, _ = _modules(g)
    vfe.eval()
    perm = torch.from_numpy(np.random.default_rng(3).permutation(M)).cuda()
    with torch.no_grad():
        a = vfe.encode(vox, coords, num, B, ny, nx)
        b = vfe.encode(vox[perm].contiguous(), coords[perm].contiguous(), num[perm].contiguous(), B, ny, nx)
    assert torch.equal(a, b)


def _small_encoder(max_points=20, C=64):
    from unidistill_amd.layers.pillars import PillarLidarEncoder
    cfg = dict(type="pillars", point_cloud_range=[-6.0, -3.6, -5.0, 6.0, 3.6, 3.0], voxel_size=[0.6, 0.6, 8.0], grid_size=[20, 12, 1],
               max_num_points=max_points, max_voxels=(400, 400), src_num_point_features=5, use_num_point_features=5,
               num_filters=[C])
    torch.manual_seed(0)
    return PillarLidarEncoder(cfg).cuda()


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform([-7.0, -4.0, -6.0, 0.0, 0.0], [7.0, 4.0, 4.0, 1.0, 1.0], (n, 5)).astype(np.float32)
    return torch.from_numpy(pts).cuda()


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("train", [True, False])
def test_encoder_equals_op_on_voxelizer_output(hip_lib, ragged, train):
    from unidistill_amd.ops.pillars import pillar_encode
    from unidistill_amd.ops.voxelize import voxelize_batch
    enc = _small_encoder()
    enc.train(train)
    points = [_cloud(900, 1), _cloud(700 if ragged else 900, 2), _cloud(900, 3)]
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        got = enc(points)
    assert got.shape == (3, 64, 12, 20) and got.permute(0, 2, 3, 1).is_contiguous()
    vz = enc.voxelizer
    if ragged:
        voxels, coords, num = vz(points)
    else:
        voxels, coords, num, _, _ = voxelize_batch(torch.stack(points), vz.voxel_size, vz.point_cloud_range, vz.max_num_points,
                                                   vz.max_voxels, want_voxels=True, want_mean=False)
    assert voxels.shape[1:] == (20, 5) and int(num.max()) > 1 and int(num.min()) >= 1
    enc.load_state_dict(state)                      # the running statistics the first pass started from
    pfn = enc.vfe.pfn_layers[0]
    with torch.no_grad():
        ref = pillar_encode(voxels, coords, num, pfn.linear.weight, pfn.norm, 3, 12, 20, vz.voxel_size, vz.point_cloud_range)
    assert torch.equal(got, ref)
    if not ragged:                                  # the one-read path against voxelize_batch's own read per call
        enc.load_state_dict(state)
        enc.one_read = False
        with torch.no_grad():
            assert torch.equal(enc(points), got)
        calls = []
        real = torch.Tensor.cpu
        enc.one_read = True
        try:
            torch.Tensor.cpu = lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1]
            with torch.no_grad():
                enc(points)
        finally:
            torch.Tensor.cpu = real
        assert len(calls) == 1, len(calls)


@pytest.mark.parametrize("name", ["m63", "m65"])
def test_state_dict_keys_and_golden_weights(golden, hip_lib, name):
    g = golden("pillars_" + name)
    M, P, C, F, abs_xyz, dist, nx, ny, B = _cfg(g)
    vfe, sc = _modules(g, with_weights=False)
    assert list(vfe.state_dict().keys()) == [str(k) for k in g["keys"]]
    assert not list(sc.state_dict().keys())
    sd = dict(zip([str(k) for k in g["keys"]], (g["weight"], g["gamma"], g["beta"], g["running_mean"], g["running_var"],
                                               np.asarray(0, np.int64))))
    vfe.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    vfe.eval()
    vox, coords, num, _ = _inputs(g)
    with torch.no_grad():
        feats = vfe(vox, coords, num)
    _check(feats, g, "eval/feats", name + " eval features from a loaded state dict")


def _sha(tensors):
    import hashlib
    return hashlib.sha256(torch.cat([t.detach().flatten().float() for t in tensors]).cpu().numpy().tobytes()).hexdigest()


def _two_steps(make_step, batch_kw):
    from unidistill_amd import train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    step = make_step()
    tr = train.Trainer(step, device=dev, channels_last=True)
    batch = train.synthetic_batch(dev, **batch_kw)
    trainable = [n for n, p in step.model.named_parameters() if p.requires_grad]
    for i in range(2):
        out = tr.step(batch)
        assert torch.isfinite(out["loss"]), i
        if i == 0:
            missing = [n for n, p in step.model.named_parameters() if p.requires_grad and p.grad is None]
            assert not missing, missing[:5]
            assert all(torch.isfinite(p.grad).all() for p in step.model.parameters() if p.grad is not None)
    torch.cuda.synchronize()
    return step, _sha(tr.params), len(trainable)


def test_detect_step_with_pillar_encoder(hip_lib):
    from unidistill_amd import train
    from unidistill_amd.layers.pillars import PillarLidarEncoder
    make = lambda: train.DetectStep(model=train.build_model("lidar", lidar_encoder="pillars"))
    kw = dict(batch_size=1, with_imgs=False)
    step, sha0, n = _two_steps(make, kw)
    assert isinstance(step.model.lidar_encoder, PillarLidarEncoder) and n > 50
    assert int(step.model.lidar_encoder.vfe.pfn_layers[0].norm.num_batches_tracked) == 2
    _, sha1, _ = _two_steps(make, kw)
    assert sha0 == sha1, "parameters after two steps differ between two fresh runs"
    # validation with the trained model: the proposal layer's per-sample predictions

    class _Sink:
        def add_batch(self, *a):
            self.got = a
    sink = _Sink()
    dev = torch.device("cuda:0")
    batch = train.synthetic_batch(dev, batch_size=1, with_imgs=False)
    preds = train.ValidationStep(step.model, sink)(batch, ["s0"], torch.eye(4, device=dev).unsqueeze(0))
    assert len(preds) == 1 and {"pred_boxes", "pred_scores", "pred_labels"} <= set(preds[0]) and sink.got[1] is preds
    assert step.model.training


def test_distill_step_with_pillar_student(hip_lib):
    from unidistill_amd import train
    from unidistill_amd.layers.pillars import PillarLidarEncoder
    make = lambda: train.DistillStep("lidar_exp_distill_camera", student=train.build_model("lidar", lidar_encoder="pillars"))
    kw = dict(batch_size=1, ncam=1)
    step, sha0, n = _two_steps(make, kw)
    assert isinstance(step.model.lidar_encoder, PillarLidarEncoder) and step.teacher_model.lidar_encoder is None
    assert all(p.grad is None for p in step.teacher_model.parameters())
    _, sha1, _ = _two_steps(make, kw)
    assert sha0 == sha1, "parameters after two steps differ between two fresh runs"


def test_pillar_student_under_a_lidar_teacher_uses_prepare(hip_lib):
    """The teacher-overlap path calls the teacher's lidar_encoder.prepare(): a pillar teacher answers it like the sparse one."""
    enc = _small_encoder()
    points = [_cloud(900, 1), _cloud(900, 2)]
    with torch.no_grad():
        prepared = enc.prepare(points)
        assert torch.equal(enc(points, prepared), enc(points))


def test_stacked_layers_and_unsupported_sizes(hip_lib):
    from unidistill_amd.layers.pillars import PillarVFE
    kw = dict(use_norm=True, with_distance=False, use_absolute_xyz=True, num_point_features=5, voxel_size=[0.6, 0.6, 8.0],
              point_cloud_range=[-6.0, -3.6, -5.0, 6.0, 3.6, 3.0])
    with pytest.raises(NotImplementedError, match="stacked PFN layers"):
        PillarVFE(num_filters=[64, 64], **kw)
    assert hip_lib.ud_pillar_workspace_bytes(100, 20, 5, 256, 1) > 0
    for bad in ((100, 20, 5, 48, 1), (100, 20, 5, 288, 1), (100, 20, 2, 64, 1), (100, 20, 9, 64, 1), (100, 65, 5, 64, 1), (0, 20, 5, 64, 1)):
        assert hip_lib.ud_pillar_workspace_bytes(*bad) == 0, bad
