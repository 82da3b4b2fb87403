"""Float64 restatement of the LiDAR depth supervision (csrc/depth_sup.hip, ops/depth_sup.py); a helper, not a test.

Labels: numpy float64 with the products and sums in the order the kernel evaluates them (no fused multiply-add on either side),
so the comparisons (range, image bounds, cell, bin) are the kernel's own except where a value sits within rounding of a border;
``near_edge`` marks the cells where that can happen.  Loss: ``binary_cross_entropy(softmax(x.double()), onehot)`` with autograd
on the CPU."""
import numpy as np
import torch

PX_EPS = 1e-3      # pixels: distance to a cell / image border below which a point's cell is not trusted
D_EPS = 1e-4       # metres: distance to a bin edge, to d_bound[0] / d_bound[1], or to the cell's minimum from another bin


def inv4x4(a):
    """Gauss-Jordan with partial pivoting in float64: the operation order of ud_inv4x4 (csrc/lss_geom.h)."""
    m = np.zeros((4, 8), np.float64)
    m[:, :4] = np.asarray(a, np.float64)
    m[:, 4:] = np.eye(4)
    for c in range(4):
        piv, best = c, abs(m[c, c])
        for r in range(c + 1, 4):
            if abs(m[r, c]) > best:
                best, piv = abs(m[r, c]), r
        if best == 0.0:
            return None
        if piv != c:
            m[[c, piv]] = m[[piv, c]]
        inv = 1.0 / m[c, c]
        m[c] = m[c] * inv
        for r in range(4):
            if r != c:
                f = m[r, c]
                if f != 0.0:
                    m[r] = m[r] - f * m[c]
    return m[:, 4:].copy()


def _matmul_seq(a, b, kmax):
    """acc = a[r,0]*b[0,c]; acc += a[r,k]*b[k,c] for k = 1..kmax-1 (separately rounded)."""
    out = np.zeros((a.shape[0], b.shape[1]), np.float64)
    for r in range(a.shape[0]):
        for c in range(b.shape[1]):
            acc = a[r, 0] * b[0, c]
            for k in range(1, kmax):
                acc = acc + a[r, k] * b[k, c]
            out[r, c] = acc
    return out


def camera_projection(s2e, intrin, ida, bda):
    """One camera's 28 doubles as k_depth_setup builds them: P = K3 . Minv[0:3] (3x4), Minv row z (4), ida rows 0..2 (3x4)."""
    s2e, intrin, ida = (np.asarray(t, np.float32).astype(np.float64) for t in (s2e, intrin, ida))
    m = s2e if bda is None else _matmul_seq(np.asarray(bda, np.float32).astype(np.float64), s2e, 4)
    minv = inv4x4(m)
    if minv is None:
        minv = np.full((4, 4), np.nan)
    return _matmul_seq(intrin[:3, :3], minv[:3], 3), minv[2].copy(), ida[:3].copy()


def _row4(m, x, y, z):
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]


def project(P, mz, A, xyz):
    """xyz float64[N, 3] -> (u, v, d) float64[N] in the kernel's operation order."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        xp, yp, w, qz = _row4(P[0], x, y, z), _row4(P[1], x, y, z), _row4(P[2], x, y, z), _row4(mz, x, y, z)
        u0, v0 = xp / w, yp / w
        u = ((A[0, 0] * u0 + A[0, 1] * v0) + A[0, 2] * qz) + A[0, 3]
        v = ((A[1, 0] * u0 + A[1, 1] * v0) + A[1, 2] * qz) + A[1, 3]
        d = ((A[2, 0] * u0 + A[2, 1] * v0) + A[2, 2] * qz) + A[2, 3]
    return u, v, d


def depth_bins(d_bound):
    return int(torch.arange(*[float(v) for v in d_bound], dtype=torch.float).numel())


def depth_labels(points, sensor2ego, intrin, ida, bda, d_bound, final_dim, downsample_factor):
    """points f32[B, Nmax, >= 3]; matrices [B, ncam, 4, 4]; bda [B, 4, 4] or None
    -> dmin f32[B, ncam, fH, fW] (+inf where empty), label i32 (-1 where empty), near_edge bool (same shape)."""
    points = np.asarray(points, np.float32)
    B, ncam = sensor2ego.shape[:2]
    H, W = final_dim
    ds = float(downsample_factor)
    fH, fW = H // downsample_factor, W // downsample_factor
    lo, hi, step = (float(v) for v in d_bound)
    D = depth_bins(d_bound)
    dmin = np.full((B, ncam, fH, fW), np.inf, np.float32)
    near = np.zeros((B, ncam, fH, fW), bool)
    for b in range(B):
        p = points[b, :, :3]
        keep = np.isfinite(p).all(1) & ~((p[:, 0] == 0) & (p[:, 1] == 0) & (p[:, 2] == 0))
        xyz = p[keep].astype(np.float64)
        for c in range(ncam):
            P, mz, A = camera_projection(sensor2ego[b, c], intrin[b, c], ida[b, c], None if bda is None else bda[b])
            u, v, d = project(P, mz, A, xyz)
            fin = np.isfinite(u) & np.isfinite(v) & np.isfinite(d)
            u, v, d = u[fin], v[fin], d[fin]
            ok = (d >= lo) & (d < hi) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
            fh, fw = np.floor(v[ok] / ds).astype(np.int64), np.floor(u[ok] / ds).astype(np.int64)
            inside = (fh < fH) & (fw < fW)
            fh, fw, dk = fh[inside], fw[inside], d[ok][inside]
            d32 = dk.astype(np.float32)
            cell = dmin[b, c].reshape(-1)                                  # a view
            np.minimum.at(cell, fh * fW + fw, d32)
            # ---- cells whose result a last-bit difference could move
            loose = (d >= lo - D_EPS) & (d < hi + D_EPS) & (u >= -PX_EPS) & (u < W + PX_EPS) & (v >= -PX_EPS) & (v < H + PX_EPS)
            ul, vl, dl = u[loose], v[loose], d[loose]
            near_u = (np.abs(ul - np.round(ul / ds) * ds) <= PX_EPS) | (np.abs(ul - W) <= PX_EPS)
            near_v = (np.abs(vl - np.round(vl / ds) * ds) <= PX_EPS) | (np.abs(vl - H) <= PX_EPS)
            rel = dl - lo
            near_d = (np.abs(rel - np.round(rel / step) * step) <= D_EPS) | (np.abs(dl - hi) <= D_EPS)
            flag = near_u | near_v | near_d
            nm = near[b, c]
            for du in (-PX_EPS, 0.0, PX_EPS):                              # every cell such a point could be put into
                for dv in (-PX_EPS, 0.0, PX_EPS):
                    ch = np.floor((vl[flag] + dv) / ds).astype(np.int64)
                    cw = np.floor((ul[flag] + du) / ds).astype(np.int64)
                    g = (ch >= 0) & (ch < fH) & (cw >= 0) & (cw < fW)
                    nm[ch[g], cw[g]] = True
            # a point within D_EPS of its cell's minimum but in another bin
            mins = cell[fh * fW + fw].astype(np.float64)
            other = (dk - mins <= D_EPS) & (np.floor((dk - lo) / step) != np.floor((mins - lo) / step))
            nm[fh[other], fw[other]] = True
    with np.errstate(invalid="ignore"):
        k = np.floor((dmin.astype(np.float64) - lo) / step)
    label = np.where(np.isfinite(dmin) & (k >= 0) & (k < D), k, -1).astype(np.int32)
    return dmin, label, near


def frustum_points(sensor2ego, intrin, ida, bda, u, v, d):
    """The forward chain of LSSFPN.get_geometry in float64: image points (u, v) at depth d [N] of one camera -> ego xyz [N, 3]."""
    s2e, K, A = (np.asarray(t, np.float32).astype(np.float64) for t in (sensor2ego, intrin, ida))
    p = np.linalg.inv(A) @ np.stack([u, v, d, np.ones_like(d)])
    q = np.linalg.inv(K[:3, :3]) @ np.stack([p[0] * p[2], p[1] * p[2], p[2]])
    m = s2e if bda is None else np.asarray(bda, np.float32).astype(np.float64) @ s2e
    return (m @ np.concatenate([q, np.ones((1, q.shape[1]))]))[:3].T


def depth_loss(x, label):
    """x: float tensor [BN, D, fH, fW] (any strides / dtype), label: int tensor [BN, fH, fW]
    -> (loss float64 scalar tensor, dx float64 tensor [BN, D, fH, fW]) on the CPU."""
    xd = x.detach().double().cpu().contiguous().requires_grad_(True)
    lab = label.detach().cpu().long().reshape(xd.shape[0], xd.shape[2], xd.shape[3])
    loss = depth_loss_expr(xd, lab)
    loss.backward()
    return loss.detach(), xd.grad


def depth_loss_expr(x, lab):
    """The loss as plain PyTorch ops in x's own dtype and on its device (fp32 on the GPU: the tolerance yardstick)."""
    D = x.shape[1]
    fg = (lab >= 0) & (lab < D)
    p = torch.softmax(x, 1).permute(0, 2, 3, 1)[fg]                       # [nfg, D]
    t = torch.nn.functional.one_hot(lab[fg].long(), D).to(p.dtype)
    return torch.nn.functional.binary_cross_entropy(p, t, reduction="sum") / max(1, int(fg.sum()))
