"""Target assignment of the CenterPoint heads, restated over ALL anchors in numpy float64.

Written from the description of the operation, to be compared with ``ud_assign_targets`` (csrc/assign.hip) and
with the two tensor-op formulations of ``FCOSAssigner``: plain loops over samples and tasks, every one of the
w * h anchors a candidate of every box; no candidate window, no bitmap, no torch.

Per sample and task:
  * rows up to the last one whose box columns (all but the class column) do not sum to zero are valid, row 0
    always;
  * a valid row is a member of the task that lists its class id (truncated toward zero); an id that no task
    lists is a member of none;
  * members are ordered by (offset of the class inside the task, row index);
  * the positives are the union over the members of the ``topk`` anchors nearest to the member's centre; among
    anchors at equal distance the lower anchor index is taken first;
  * a positive is assigned its nearest member, the first in member order on a tie;
  * the positives in ascending anchor order fill the first K slots (ind, mask, cat, box encoding); the heat
    map is set at every positive, those beyond K included.

Centres are in voxel units from the range's lower corner, anchor (ix, iy) is at (ix, iy) * out_size_factor and
has the index iy * w + ix.  The encoding of a box (x, y, z, dx, dy, dz, yaw, extra...) at an anchor (ax, ay):
  ((cx - ax) / osf, (cy - ay) / osf, z, log(dx), log(dy), log(dz), sin(yaw'), cos(yaw'), extra...),
yaw' = yaw wrapped into [-pi, pi), zero-padded to ``default_box_dims`` columns.  All of it is computed in
float64 on the float32 inputs.

Besides the targets the function returns how close every decision it took was: the relative gap, in squared
distance, between the k-th and the (k+1)-th nearest anchor of a member and between the nearest and the second
nearest member at a positive.  ``row_margin[b, m]`` is the smallest gap of any decision row m took part in, so
that a generator can redraw exactly the boxes whose outcome float32 rounding could decide.
"""
import numpy as np


def _rel_gap(lo, hi):
    """(hi - lo) / hi for 0 <= lo <= hi; 0 where both are 0 (a tie at distance zero)."""
    return np.where(hi > 0, (hi - lo) / np.where(hi > 0, hi, 1.0), 0.0)


def assign_reference(gt, tasks, class_map, grid_wh, out_size_factor, pc_range, voxel_size, topk, K,
                     default_box_dims):
    """gt f32[B, M, cols] (last column = class id); tasks = list of lists of class names; class_map name -> id;
    grid_wh = (w, h) anchors.  Returns (targets, margin, row_margin): targets[key][t] for key in heatmap
    f32[B, nc_t, h, w], ind i64[B, K], mask bool[B, K], cat i64[B, K], box_encoding f64[B, K, enc_dim], and
    row i64[B, K], the input row behind each filled slot (-1 elsewhere)."""
    gt = np.asarray(gt)
    assert gt.dtype == np.float32 and gt.ndim == 3
    B, M, cols = gt.shape
    w, h = int(grid_wh[0]), int(grid_wh[1])
    A = w * h
    s = float(out_size_factor)
    k = min(int(topk), A)
    n_extra = cols - 1 - 7
    enc_dim = max(8 + n_extra, int(default_box_dims))
    g64 = gt.astype(np.float64)
    ax = np.tile(np.arange(w, dtype=np.float64) * s, h)          # anchor a = iy * w + ix
    ay = np.repeat(np.arange(h, dtype=np.float64) * s, w)
    out = {key: {} for key in ("heatmap", "ind", "mask", "cat", "box_encoding", "row")}
    for t, names in enumerate(tasks):
        out["heatmap"][t] = np.zeros((B, len(names), h, w), np.float32)
        out["ind"][t] = np.zeros((B, K), np.int64)
        out["mask"][t] = np.zeros((B, K), bool)
        out["cat"][t] = np.zeros((B, K), np.int64)
        out["box_encoding"][t] = np.zeros((B, K, enc_dim), np.float64)
        out["row"][t] = np.full((B, K), -1, np.int64)             # input row a slot was encoded from
    row_margin = np.full((B, M), np.inf)
    for b in range(B):
        box = g64[b, :, :-1]
        ids = np.trunc(g64[b, :, -1])
        nonzero = np.flatnonzero(box.sum(1) != 0)
        last = int(nonzero[-1]) if nonzero.size else 0
        for t, names in enumerate(tasks):
            rows, offs = [], []
            for off, name in enumerate(names):
                for m in range(last + 1):
                    if ids[m] == class_map[name]:
                        rows.append(m)
                        offs.append(off)
            if not rows:
                continue
            rows, offs = np.array(rows), np.array(offs)
            mb = box[rows]
            cx = (mb[:, 0] - pc_range[0]) / voxel_size[0]
            cy = (mb[:, 1] - pc_range[1]) / voxel_size[1]
            d = (ax[None, :] - cx[:, None]) ** 2 + (ay[None, :] - cy[:, None]) ** 2      # [members, A]
            positive = np.zeros(A, bool)
            for r in range(len(rows)):
                dr = d[r]
                part = np.partition(dr, [k - 1, k] if k < A else [k - 1])
                vk = part[k - 1]
                below = np.flatnonzero(dr < vk)
                equal = np.flatnonzero(dr == vk)[:k - below.size]     # ties: lower anchor index first
                positive[below] = True
                positive[equal] = True
                if k < A:
                    row_margin[b, rows[r]] = min(row_margin[b, rows[r]], float(_rel_gap(vk, part[k])))
            pos = np.flatnonzero(positive)                            # ascending anchor order
            dp = d[:, pos]
            near = dp.argmin(0)                                       # first member on a tie
            if len(rows) > 1:
                two = np.partition(dp, 1, axis=0)[:2]
                gap = _rel_gap(two[0], two[1])
                r_i, p_i = np.nonzero(dp <= two[1][None, :])           # the nearest and all that tie for second
                np.minimum.at(row_margin[b], rows[r_i], gap[p_i])
            hm = out["heatmap"][t][b].reshape(len(names), A)
            hm[offs[near], pos] = 1.0
            n = min(pos.size, K)
            p, q = pos[:n], near[:n]
            out["ind"][t][b, :n] = p
            out["mask"][t][b, :n] = True
            out["cat"][t][b, :n] = offs[q]
            out["row"][t][b, :n] = rows[q]
            bx = mb[q]
            yaw = bx[:, 6] - np.floor(bx[:, 6] / (2 * np.pi) + 0.5) * (2 * np.pi)
            e = out["box_encoding"][t][b]
            e[:n, 0] = (cx[q] - ax[p]) / s
            e[:n, 1] = (cy[q] - ay[p]) / s
            e[:n, 2] = bx[:, 2]
            with np.errstate(divide="ignore"):
                e[:n, 3] = np.log(bx[:, 3] / voxel_size[0] * voxel_size[0])
                e[:n, 4] = np.log(bx[:, 4] / voxel_size[1] * voxel_size[1])
                e[:n, 5] = np.log(bx[:, 5])
            e[:n, 6] = np.sin(yaw)
            e[:n, 7] = np.cos(yaw)
            if n_extra > 0:
                e[:n, 8:8 + n_extra] = bx[:, 7:]
    return out, float(row_margin.min()) if row_margin.size else np.inf, row_margin


def encoding_bound(gt, ref, grid_wh, out_size_factor, pc_range, voxel_size):
    """Float32 error bound of every element of the encodings in ``ref`` (the targets assign_reference returned
    for ``gt``), dict t -> f64[B, K, enc_dim].  No fixed constant: four float32 spacings at the largest
    intermediate value of the column's formula, from the case's own inputs.
      columns 0, 1   4 * spacing(max(|centre|, |anchor|)) / out_size_factor: centre and anchor are formed and
                     subtracted at that magnitude, then divided
      log columns    4 * spacing(|log v|) + spacing(v) / v: the operand dx / vs * vs carries one spacing itself
      sin, cos       4 * spacing(1) + spacing(|yaw|): the wrap into [-pi, pi) is done at |yaw|'s magnitude
      z, extras      0 (copies)
    Unfilled slots and non-finite reference values get 0: they must match exactly, or in kind."""
    gt = np.asarray(gt).astype(np.float64)
    w = int(grid_wh[0])
    s = float(out_size_factor)
    sp = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    bounds = {}
    for t, enc in ref["box_encoding"].items():
        bnd = np.zeros_like(enc)
        for b, n in enumerate(ref["mask"][t].sum(1)):
            if not n:
                continue
            bx = gt[b, ref["row"][t][b, :n]]
            ind = ref["ind"][t][b, :n]
            cx = (bx[:, 0] - pc_range[0]) / voxel_size[0]
            cy = (bx[:, 1] - pc_range[1]) / voxel_size[1]
            bnd[b, :n, 0] = 4 * sp(np.maximum(np.abs(cx), (ind % w) * s)) / s
            bnd[b, :n, 1] = 4 * sp(np.maximum(np.abs(cy), (ind // w) * s)) / s
            for c in (3, 4, 5):
                v = bx[:, c]
                ok = v > 0
                v1 = np.where(ok, v, 1.0)
                bnd[b, :n, c] = np.where(ok, 4 * sp(np.log(v1)) + sp(v1) / v1, 0.0)
            bnd[b, :n, 6] = bnd[b, :n, 7] = 4 * sp(np.ones(n)) + sp(bx[:, 6])
        bounds[t] = bnd
    return bounds
