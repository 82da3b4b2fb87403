"""GPU: the fused LiDAR input chain (ud_lidar_prep_count / ud_lidar_prep_compact through collate_fn,
lidar_prep_host_clouds and points_range_filter) against the reference golden tests/golden/lidar_chain.npz and a numpy
oracle of the reference's chain + fill_batch_tensor."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_lidar_prep_cpu as cpu                                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PCR = cpu.PCR


def fill_batch(points):
    """collate_fn.fill_batch_tensor (nuscenes_multimodal.py:441-463) for a list of float32 [Ni, D] arrays."""
    n = max(len(p) for p in points)
    out = np.zeros((len(points), n, points[0].shape[1]), np.float32)
    for b, p in enumerate(points):
        out[b, :len(p)] = p
    return out


def oracle_chain(clouds, aug):
    """The reference's CollectLidarSweeps -> BevAffineTransformation -> ObjectRangeFilter on the points, in numpy
    (oracle.points_transform is numpy's float64 matmul, as the reference)."""
    D = clouds[0].shape[1]
    parts = [clouds[0].copy()]
    if D == 5:
        parts[0][:, -1] = 0.0
    for j, c in enumerate(clouds[1:]):
        parts.append(oracle.points_transform(c, aug["sweep_mats"][j], aug["time_lags"][j] if D == 5 else None))
    p = np.concatenate(parts)
    if aug["bda_mat"] is not None:
        p = oracle.points_transform(p, aug["bda_mat"])
    if aug["range"] is not None:
        r = aug["range"]
        p = p[(p[:, 0] >= r[0]) & (p[:, 0] <= r[3]) & (p[:, 1] >= r[1]) & (p[:, 1] <= r[4])]
    return p


def golden_batch(g, D=5):
    outs = cpu.run_loader_side(g)
    data = []
    for d in outs:
        raw = [d["points"][:, :D].copy()] + [s[:, :D].copy() for s in d["sweep_points"]]
        data.append({"points_raw": raw, "lidar_aug": d["lidar_aug"]})
    return data


def bits(t):
    return np.ascontiguousarray(t).view(np.uint32)


def test_collate_matches_golden_bit_exact(hip_lib, golden):
    from unidistill_amd.ops import input_prep as ip
    g = golden("lidar_chain")
    data = golden_batch(g)
    want = fill_batch([g[f"s{k}_points"] for k in range(cpu.N_SAMPLES)])
    got = ip.collate_fn(data, device=DEV)["points"]
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.float32
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(want))


@pytest.mark.parametrize("D", [3, 4])
def test_collate_d3_d4_vs_oracle(hip_lib, golden, D):
    from unidistill_amd.ops import input_prep as ip
    g = golden("lidar_chain")
    data = golden_batch(g, D)
    want = fill_batch([oracle_chain(d["points_raw"], d["lidar_aug"]) for d in data])
    got = ip.collate_fn(data, device=DEV)["points"]
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(want))


def _full_batch(rng, B=4, sweeps=10, n=34720, D=5):
    clouds, plans = [], []
    for b in range(B):
        cs = [cpu._cloud(rng, int(n + rng.integers(-300, 300)), scale=35.0)[:, :D] for _ in range(sweeps)]
        l2e, e2g = cpu._pose(rng), cpu._pose(rng)
        mats = []
        for _ in range(sweeps - 1):
            pose = e2g.copy()
            pose[:3, 3] += rng.normal(scale=[3.0, 3.0, 0.1])
            mats.append(oracle.sweep_to_key_matrix(l2e, e2g, pose))
        from unidistill_amd.ops import input_prep as ip
        bda = ip.bev_transform_matrix(rng.uniform(-45, 45), rng.uniform(0.9, 1.1), rng.normal(scale=0.5, size=3),
                                      rng.uniform() < 0.5, rng.uniform() < 0.5)
        plans.append({"segments": [len(c) for c in cs], "sweep_mats": np.stack(mats),
                      "time_lags": rng.uniform(0, 0.5, sweeps - 1).astype(np.float32), "bda_mat": bda,
                      "range": np.array(PCR, np.float32)})
        clouds.append([np.ascontiguousarray(c) for c in cs])
    return clouds, plans


def test_full_size_batch_vs_oracle_and_repeatable(hip_lib):
    """4 samples x 10 clouds x ~34 720 points with random poses and BDA; three calls give identical results; the host
    inputs are not touched."""
    from unidistill_amd.ops import input_prep as ip
    rng = np.random.default_rng(11)
    clouds, plans = _full_batch(rng)
    keep = [[c.copy() for c in cs] for cs in clouds]
    want = fill_batch([oracle_chain(cs, p) for cs, p in zip(clouds, plans)])
    outs = [ip.lidar_prep_host_clouds(clouds, plans, DEV) for _ in range(3)]
    torch.cuda.synchronize()
    got = outs[0].cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(want))
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    for a, b in zip(keep, clouds):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(bits(x), bits(y))


def test_points_range_filter_vs_oracle(hip_lib):
    from unidistill_amd.ops import input_prep as ip
    rng = np.random.default_rng(5)
    sizes = [5000, 0, 1, 70000, 300]
    pts = cpu._cloud(rng, sum(sizes), scale=45.0)
    pts[::97, 0] = np.nan
    pts[::89, 1] = 54.0
    seg = np.cumsum([0] + sizes)
    x = torch.from_numpy(pts).to(DEV)
    x0 = x.clone()
    got, counts = ip.points_range_filter(x, PCR, seg)
    wants = [pts[a:b][(pts[a:b, 0] >= -54) & (pts[a:b, 0] <= 54) & (pts[a:b, 1] >= -54) & (pts[a:b, 1] <= 54)]
             for a, b in zip(seg, seg[1:])]
    assert list(counts) == [len(w) for w in wants]
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(np.concatenate(wants)))
    assert torch.equal(x.view(torch.int32), x0.view(torch.int32))                 # NaN rows included
    whole, c1 = ip.points_range_filter(x, PCR)
    assert list(c1) == [sum(counts)] and torch.equal(whole, got)


def test_all_samples_empty(hip_lib):
    from unidistill_amd.ops import input_prep as ip
    D = 5
    far = np.full((10, D), 500.0, np.float32)
    aug = {"segments": [10, 0], "sweep_mats": np.eye(4)[None], "time_lags": np.zeros(1, np.float32),
           "bda_mat": None, "range": np.array(PCR, np.float32)}
    out = ip.lidar_prep_host_clouds([[far, far[:0]], [far, far[:0]]], [aug, aug], DEV)
    assert tuple(out.shape) == (2, 0, D)
    out = ip.lidar_prep_host_clouds([[far[:0]]], [None], DEV)
    assert tuple(out.shape) == (1, 0, D)


def test_collate_returns_before_pending_work_on_current_stream(hip_lib):
    """The count readback waits on the input stream only: with a long torch.cuda._sleep queued on the current stream,
    collate_fn returns while that work is still pending; the result is ordered after it and correct."""
    from unidistill_amd.ops import input_prep as ip
    rng = np.random.default_rng(3)
    clouds, plans = _full_batch(rng, B=2, sweeps=3, n=20000)
    want = fill_batch([oracle_chain(cs, p) for cs, p in zip(clouds, plans)])
    ip.lidar_prep_host_clouds(clouds, plans, DEV)                                # warm: stream, staging, library
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    torch.cuda._sleep(1_000_000)
    e.record()
    e.synchronize()
    cycles = int(1_000_000 * 2000.0 / max(s.elapsed_time(e), 1e-3))            # ~2 s of sleep
    cur = torch.cuda.current_stream()
    torch.cuda._sleep(cycles)
    data = [{"points_raw": cs, "lidar_aug": p} for cs, p in zip(clouds, plans)]
    out = ip.collate_fn(data, device=DEV)["points"]
    assert cur.query() is False                                                  # the sleep is still running
    y = out * 1.0                                                                # ordered after the result on cur
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(want))


def test_distill_step_same_losses_both_routes(hip_lib, golden):
    """One fp32 DistillStep at B = 4: the golden's raw clouds + plans through collate_fn vs the reference-processed
    clouds through the existing ``points`` path give bit-equal losses."""
    from unidistill_amd import train
    from unidistill_amd.ops import input_prep as ip
    g = golden("lidar_chain")
    dev = torch.device(DEV)
    torch.manual_seed(0)
    np.random.seed(0)
    step = train.DistillStep("camera_exp_distill_lidar")
    tr = train.Trainer(step, device=dev, channels_last=True)
    B = cpu.N_SAMPLES
    base = train.synthetic_batch(dev, B)
    data = golden_batch(g)
    batches = []
    for route in ("raw", "host"):
        samples = []
        for k in range(B):
            d = {"gt_boxes": base["gt_boxes"][k].cpu().numpy(), "gt_labels": base["gt_labels"][k].cpu().numpy(),
                 "imgs": base["imgs"][k].cpu().numpy(),
                 "mats_dict": {key: v[k].cpu().numpy() for key, v in base["mats_dict"].items()}}
            if route == "raw":
                d.update(data[k])
            else:
                d["points"] = g[f"s{k}_points"]
            samples.append(d)
        batches.append(ip.collate_fn(samples, device=dev))
    assert torch.equal(batches[0]["points"], batches[1]["points"])
    losses = []
    for batch in batches:
        out = tr.module(batch)
        torch.cuda.synchronize()
        losses.append({k: v.detach().cpu() for k, v in out.items() if torch.is_tensor(v) and v.numel() == 1})
    assert losses[0].keys() == losses[1].keys() and "loss" in losses[0]
    for k in losses[0]:
        assert torch.equal(losses[0][k], losses[1][k]), k
        assert torch.isfinite(losses[0][k]).all(), k


def test_staged_upload_reuse_regrowth_and_stream_order(hip_lib):
    """ops/staging.py staged_upload with byte payloads and no kernel: 4 KiB, then 2 KiB of other bytes through the same
    pinned buffer (reuse), then 1 MiB + 16 (the buffer grows past its 1 MiB floor), each issued while the caller's
    non-default stream has a fill pending; once that stream is synchronised the device bytes are the host bytes."""
    from unidistill_amd.ops import staging
    dev = torch.device(DEV)
    torch.cuda.synchronize()
    staging._buffers.pop(dev.index, None)                   # start below the floor whatever ran before in this process
    rng = np.random.default_rng(11)
    side = torch.cuda.Stream(device=dev)
    sent, sizes = [], []
    with torch.cuda.stream(side):
        for n in (4096, 2048, (1 << 20) + 16):
            payload = rng.integers(0, 256, n, dtype=np.uint8)
            torch.empty(1 << 20, dtype=torch.uint8, device=dev).fill_(n % 251)      # pending on the caller's stream

            def fill(host, d, payload=payload):
                assert host.shape == (n,) and d.numel() == n
                host[:] = payload
            up, = staging.staged_upload(dev, n, fill, lambda d, s: (d,))
            sent.append((payload, up, up.clone()))          # the clone runs on the caller's stream, behind the wait
            sizes.append(staging._buffers[dev.index][0].numel())
        side.synchronize()
    assert sizes == [1 << 20, 1 << 20, (1 << 20) + 16]
    for payload, up, copy in sent:
        want = torch.from_numpy(payload)
        assert torch.equal(up.cpu(), want) and torch.equal(copy.cpu(), want)
