"""Independent numpy float64 restatement of the PointPillars encoder (PillarVFE with one PFNLayer + PointPillarScatter):
forward in batch-statistics and running-statistics mode, the running-statistics update, and the gradients of the Linear weight
and the BatchNorm affine pair for an upstream BEV gradient.  Written from the definition of the layers, not from any
implementation; tests/test_pillars_reference_cpu.py holds it to the reference's own float64 output (tests/golden/pillars_*.npz).
"""
import numpy as np

EPS, MOMENTUM = 1e-3, 0.01
KNIFE = 1e-5      # knife-edge threshold, in units of the channel's standard deviation (x-hat units times |gamma|)


def row_features(voxels, coords, num, voxel_size, pc_range, use_absolute_xyz, with_distance):
    """[M, P, F] rows -> [M, P, K] augmented rows, padded rows (row >= num) zero."""
    v = np.asarray(voxels, np.float64)
    M, P, F = v.shape
    xyz = v[:, :, :3]
    mean = xyz.sum(1, keepdims=True) / np.asarray(num, np.float64).reshape(M, 1, 1)
    centre = np.stack([coords[:, 3 - a].astype(np.float64) * voxel_size[a] + (voxel_size[a] / 2 + pc_range[a]) for a in range(3)], 1)
    parts = [v if use_absolute_xyz else v[:, :, 3:], xyz - mean, xyz - centre[:, None, :]]
    if with_distance:
        parts.append(np.sqrt((xyz * xyz).sum(2, keepdims=True)))
    mask = (np.arange(P)[None, :] < np.asarray(num)[:, None]).astype(np.float64)
    return np.concatenate(parts, 2) * mask[:, :, None]


def forward(feat, weight, gamma, beta, running_mean=None, running_var=None, eps=EPS):
    """feat [M, P, K], weight [C, K].  Batch statistics over all M * P rows unless running statistics are given.
    -> dict: z [M, P, C], mean, var (biased), y (BatchNorm output), out [M, C] (max of relu), arg [M, C] (first maximal row)."""
    z = feat @ np.asarray(weight, np.float64).T
    if running_mean is None:
        flat = z.reshape(-1, z.shape[2])
        mean, var = flat.mean(0), flat.var(0)
    else:
        mean, var = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (z - mean) * invstd
    y = xhat * gamma + beta
    r = np.maximum(y, 0.0)
    return dict(z=z, mean=mean, var=var, invstd=invstd, xhat=xhat, y=y, out=r.max(1), arg=r.argmax(1))


def running_update(running_mean, running_var, mean, var, n, momentum=MOMENTUM):
    return ((1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * var * n / (n - 1))


def scatter(out, coords, B, ny, nx, fill=0.0):
    """[M, C] -> [B, C, ny, nx], `fill` (zero) where no pillar lies."""
    bev = np.full((B, out.shape[1], ny, nx), fill, out.dtype)
    bev[coords[:, 0], :, coords[:, 2], coords[:, 3]] = out
    return bev


def backward(feat, weight, gamma, fwd, gbev, coords, frozen):
    """-> (dW [C, K], dgamma [C], dbeta [C]) for the upstream gradient gbev [B, C, ny, nx]."""
    M, P, C = fwd["z"].shape
    dy_out = gbev[coords[:, 0], :, coords[:, 2], coords[:, 3]].astype(np.float64)          # [M, C]
    dy = np.zeros((M, P, C))
    mi, ci = np.meshgrid(np.arange(M), np.arange(C), indexing="ij")
    dy[mi, fwd["arg"], ci] = dy_out * (fwd["out"] > 0)
    dbeta = dy.sum((0, 1))
    dgamma = (dy * fwd["xhat"]).sum((0, 1))
    if frozen:
        dz = dy * (gamma * fwd["invstd"])
    else:
        n = M * P
        dz = gamma * fwd["invstd"] * (dy - dbeta / n - fwd["xhat"] * dgamma / n)
    dW = np.einsum("mpc,mpk->ck", dz, feat)
    return dW, dgamma, dbeta


def knife_edges(fwd, num, gamma):
    """bool [M, C]: the float64 gap between the best and the second-best row, or the winner's distance from the ReLU's kink, is below
    KNIFE of the channel's standard deviation.  All padded rows of a pillar are ONE candidate (identical values, zero feature
    rows: any of them gives the same sums)."""
    y = fwd["y"]
    M, P, C = y.shape
    cand = np.where((np.arange(P)[None, :] <= np.asarray(num)[:, None])[:, :, None], y, -np.inf)   # real rows + the first padded row
    top = np.sort(cand, 1)
    best = top[:, -1]
    second = top[:, -2] if P > 1 else np.full_like(best, -np.inf)
    tol = KNIFE * np.abs(gamma)
    # two rows below the kink tie at relu = 0 with a zero gradient either way: only a positive winner's gap matters
    return ((best > 0) & (best - np.maximum(second, 0.0) < tol)) | (np.abs(best) < tol)
