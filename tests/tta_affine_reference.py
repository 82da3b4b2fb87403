"""numpy restatement of the rotation / scale / flip test-time-augmentation merge (csrc/tta_merge_affine.hip).

Maps are lists over tasks of dicts {head: array [rows, c, H, W]}; the views of B samples are stacked view-major (view v of
sample b is row v * B + b); a view is (rot_deg, scale, flip_dx, flip_dy) or a pair (flip_dx, flip_dy); pc_range is
[x_min, y_min, z_min, x_max, y_max, z_max].

Geometry (``transforms``).  Cell (x, y) of the H x W map covers [x, x+1) x [y, y+1) in cell units u; world = u * cell +
range_min.  A_v = F S R is the view's BEV transform (L its 2x2 block in metres), T = C^-1 A_v C takes original-frame u to
view-frame u, Ti is the inverse of T's linear part.  sin / cos of multiples of 90 degrees are exactly 0 / +-1; an offset of
T within 1e-9 cells of an integer is that integer.  Output pixel p samples view v at q = T (p + 1/2): g = q - 1/2,
i0 = floor(g), f = g - i0, neighbours i0, i0 + 1 per axis with weights 1 - f, f.  A view contributes at p only if every
neighbour of non-zero weight lies inside the map; the result is the sum over the contributing views, in their order,
divided by their number.

  merge64   the definition in float64.  Per neighbour n, brought into the original frame before the blend: hm sigma(h)
            (1 - p carried beside p; the result is a logit); reg Ti (n + reg - T's offset) - p; height z / s; dim exp(d) / s,
            then log (no_log: d / s); rot: (cos, sin) multiplied by Q^-1 = s L^-1, channels (sin, cos); vel L^-1 v; iou as it
            is.  ``raw=True`` returns the mean probability / mean size instead of the logit / log.
  merge32   positions and weights in float64, the value arithmetic one float32 operation at a time in the kernel's order:
            per view m0, m1 = float32 coefficients; per neighbour (y0x0, y0x1, y1x0, y1x1, zero weights skipped)
            t = m0 * a0 [+ m1 * a1] [float32(constant) + t], w = float32(wy * wx), blend = w t (+ w t ...); the views
            added in order from the first that contributes; * float32(1) / float32(n).  ``params`` = (table [V, 11], cell_x /
            cell_y) as the kernel is given them (T row-major, Ti row-major, s); by default this module's own.
"""
import numpy as np

HEADS = ("hm", "reg", "height", "dim", "rot", "vel", "iou")


def general(view):
    view = tuple(view)
    return (0.0, 1.0) + view if len(view) == 2 else view


def _sincos(rot_deg):
    q = rot_deg / 90.0
    if q == np.floor(q):
        return [(0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0)][int(q) % 4]
    return float(np.sin(np.deg2rad(rot_deg))), float(np.cos(np.deg2rad(rot_deg)))


def linear(view):
    """L (metres, 2x2) of A_v = F S R, and its inverse R^T F / s."""
    rot, s, fx, fy = general(view)
    sn, cs = _sincos(float(rot))
    F = np.diag([-1.0 if fx else 1.0, -1.0 if fy else 1.0])
    R = np.array([[cs, -sn], [sn, cs]])
    return F @ (s * R) + 0.0, (R.T @ F) / s + 0.0


def transforms(views, pc_range, H, W):
    """Per view (T [2, 3], Ti [2, 2], L^-1 [2, 2], s)."""
    lo = np.array([pc_range[0], pc_range[1]], np.float64)
    size = np.array([pc_range[3] - pc_range[0], pc_range[4] - pc_range[1]], np.float64)
    n = np.array([W, H], np.float64)
    cell = size / n
    out = []
    for view in views:
        L, Li = linear(view)
        T, Ti = np.zeros((2, 3)), np.zeros((2, 2))
        for i in range(2):
            for j in range(2):
                r = 1.0 if cell[i] == cell[j] else cell[j] / cell[i]
                T[i, j] = L[i, j] * r
                Ti[i, j] = Li[i, j] * r
            off = (L[i, 0] * lo[0] + L[i, 1] * lo[1] - lo[i]) * n[i] / size[i]
            T[i, 2] = np.round(off) if abs(off - np.round(off)) < 1e-9 else off
        out.append((T, Ti, Li, float(general(view)[1])))
    return out


def params_of(views, pc_range, H, W):
    """(table [V, 11], cell_x / cell_y) in the layout the kernel takes."""
    tr = transforms(views, pc_range, H, W)
    table = np.array([list(T.reshape(-1)) + list(Ti.reshape(-1)) + [s] for T, Ti, _, s in tr], np.float64)
    cx, cy = (pc_range[3] - pc_range[0]) / W, (pc_range[4] - pc_range[1]) / H
    return table, (1.0 if cx == cy else cx / cy)


def sample_geometry(T, H, W):
    """x0, y0 (int), fx, fy (float64), valid: [H, W] each."""
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    qx = T[0] * (px + 0.5) + T[1] * (py + 0.5) + T[2]
    qy = T[3] * (px + 0.5) + T[4] * (py + 0.5) + T[5]
    gx, gy = qx - 0.5, qy - 0.5
    x0, y0 = np.floor(gx), np.floor(gy)
    fx, fy = gx - x0, gy - y0
    valid = (x0 >= 0) & (x0 + (fx != 0) <= W - 1) & (y0 >= 0) & (y0 + (fy != 0) <= H - 1)
    x0, y0 = np.where(valid, x0, 0).astype(np.int64), np.where(valid, y0, 0).astype(np.int64)
    return x0, y0, fx, fy, valid, px, py


def _neighbours(x0, y0, fx, fy, H, W):
    """(xs, ys, wx, wy, skip) of the four neighbours in the kernel's order; a skipped neighbour has weight 0 and is not read
    (its index is clipped only so that the gather is legal)."""
    for jy in (0, 1):
        for jx in (0, 1):
            skip = ((fx == 0) if jx else np.zeros_like(fx, bool)) | ((fy == 0) if jy else np.zeros_like(fy, bool))
            yield (np.minimum(x0 + jx, W - 1), np.minimum(y0 + jy, H - 1), fx if jx else 1.0 - fx, fy if jy else 1.0 - fy, skip)


def merge64(tasks, views, pc_range, no_log, raw=False):
    V = len(views)
    rows, _, H, W = tasks[0]["hm"].shape
    assert rows % V == 0, (rows, V)
    B = rows // V
    tr = transforms(views, pc_range, H, W)
    geo = [sample_geometry(T.reshape(-1), H, W) for T, _, _, _ in tr]
    count = sum(g[4].astype(np.float64) for g in geo)
    assert (count >= 1).all(), "some pixel is covered by no view"
    out = []
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for heads in tasks:
            res = {}
            for name, a in heads.items():
                a = a.astype(np.float64)
                acc = np.zeros((B,) + a.shape[1:])
                acc_q = np.zeros_like(acc)
                for v, ((T, Ti, Li, s), (x0, y0, fx, fy, valid, px, py)) in enumerate(zip(tr, geo)):
                    av = a[v * B:(v + 1) * B]
                    val, val_q = np.zeros_like(acc), np.zeros_like(acc)
                    for xs, ys, wx, wy, skip in _neighbours(x0, y0, fx, fy, H, W):
                        w = np.where(skip, 0.0, wy * wx)
                        nb = av[:, :, ys, xs]
                        if name == "hm":
                            t = np.where(nb >= 0, 1.0 / (1.0 + np.exp(-nb)), np.exp(nb) / (1.0 + np.exp(nb)))
                            val_q += w * np.where(nb >= 0, np.exp(-nb) / (1.0 + np.exp(-nb)), 1.0 / (1.0 + np.exp(nb)))
                        elif name == "reg":
                            cx, cy = xs + nb[:, 0] - T[0, 2], ys + nb[:, 1] - T[1, 2]
                            t = np.stack([Ti[0, 0] * cx + Ti[0, 1] * cy - px, Ti[1, 0] * cx + Ti[1, 1] * cy - py], 1)
                        elif name == "height" or (name == "dim" and no_log):
                            t = nb / s
                        elif name == "dim":
                            t = np.exp(nb) / s
                        elif name == "rot":
                            Qi = s * Li
                            cs, sn = nb[:, 1], nb[:, 0]
                            t = np.stack([Qi[1, 0] * cs + Qi[1, 1] * sn, Qi[0, 0] * cs + Qi[0, 1] * sn], 1)
                        elif name == "vel":
                            t = np.stack([Li[0, 0] * nb[:, 0] + Li[0, 1] * nb[:, 1], Li[1, 0] * nb[:, 0] + Li[1, 1] * nb[:, 1]], 1)
                        else:
                            t = nb
                        val += np.where(skip, 0.0, w * t)
                    acc += np.where(valid, val, 0.0)
                    acc_q += np.where(valid, val_q, 0.0)
                acc /= count
                if name == "hm":
                    acc_q /= count
                    res[name] = acc if raw else np.log(acc) - np.log(acc_q)
                elif name == "dim" and not no_log:
                    res[name] = acc if raw else np.log(acc)
                else:
                    res[name] = acc
            out.append(res)
    return out


def merge32(tasks, views, pc_range, no_log, params=None):
    f = np.float32
    V = len(views)
    rows, _, H, W = tasks[0]["hm"].shape
    assert rows % V == 0, (rows, V)
    B = rows // V
    table, ratio = params_of(views, pc_range, H, W) if params is None else params
    table = np.asarray(table, np.float64).reshape(V, 11)
    geo = [sample_geometry(table[v, :6], H, W) for v in range(V)]
    count = sum(g[4].astype(np.int64) for g in geo)
    assert (count >= 1).all(), "some pixel is covered by no view"
    out = []
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for heads in tasks:
            res = {}
            for name, a in heads.items():
                assert a.dtype == np.float32
                C = a.shape[1]
                wide32 = name == "hm" or (name == "dim" and not no_log)
                vec2 = name in ("reg", "rot", "vel")
                acc = np.zeros((B, C, H, W), f)
                n = np.zeros((H, W), np.int64)
                for v, (x0, y0, fx, fy, valid, px, py) in enumerate(geo):
                    t6, ti, s = table[v, :6], table[v, 6:10], table[v, 10]
                    inv_s = 1.0 / s
                    li = [ti[0], ti[1] * ratio, ti[2] / ratio, ti[3]]
                    m = np.zeros((C, 2), f)                                  # per output channel: m0 on a0, m1 on a1
                    m[:, 0] = f(1)
                    if name == "height" or (name == "dim" and no_log):
                        m[:, 0] = f(inv_s)
                    elif name == "reg":
                        m[:] = [[f(ti[0]), f(ti[1])], [f(ti[2]), f(ti[3])]]
                    elif name == "vel":
                        m[:] = [[f(li[0]), f(li[1])], [f(li[2]), f(li[3])]]
                    elif name == "rot":
                        m[:] = [[f(s * li[3]), f(s * li[2])], [f(s * li[1]), f(s * li[0])]]
                    av = a[v * B:(v + 1) * B]
                    val = np.zeros((B, C, H, W), f)
                    for j, (xs, ys, wx, wy, skip) in enumerate(_neighbours(x0, y0, fx, fy, H, W)):
                        w = (wy * wx).astype(f)
                        nb = av[:, :, ys, xs]
                        if name == "hm":
                            t = f(1) / (f(1) + np.exp(-nb))
                        elif name == "dim" and not no_log:
                            t = np.exp(nb) * f(inv_s)
                        elif vec2:
                            t = m[None, :, 0, None, None] * nb[:, 0:1] + m[None, :, 1, None, None] * nb[:, 1:2]
                            if name == "reg":
                                cn = np.stack([ti[0] * (xs - t6[2]) + ti[1] * (ys - t6[5]) - px,
                                               ti[2] * (xs - t6[2]) + ti[3] * (ys - t6[5]) - py], 0).astype(f)
                                t = cn[None] + t
                        else:
                            t = m[None, :, 0, None, None] * nb
                        assert t.dtype == f and t.shape == val.shape, (name, t.dtype, t.shape)
                        val = w * t if j == 0 else np.where(skip, val, val + w * t)
                    first = valid & (n == 0)
                    acc = np.where(first, val, np.where(valid, acc + val, acc))
                    n += valid
                acc = acc * (f(1) / n.astype(f))
                if name == "hm":
                    acc = np.minimum(acc, f(1))
                    acc = np.log(acc) - np.log1p(-acc)
                elif wide32:
                    acc = np.log(acc)
                assert acc.dtype == f
                res[name] = acc
            out.append(res)
    return out
