"""float64 numpy restatement of the GT-database build and the seeded generators of its tests.

The inside test is OpenPCDet's check_pt_in_box3d in float64 (``inside_margin`` of gt_paste_reference.py), the owner of a
row is the lowest-numbered box of its scene that contains it, an object's cloud is ``points[owner == i]`` in row order
with the box's float32 centre subtracted in float32.  The kernel decides in float32, so a row within ROW_MARGIN of a box
face could fall either way: the generators RE-DRAW every such row, ``owners`` reports how many are left, and every test
asserts that number is 0 -- no row is ever left out of a comparison."""
import math

import numpy as np

from gt_paste_reference import ROW_MARGIN, inside_margin

LIMIT = 54.0                # every coordinate stays inside +-54 m
CLASSES = ["car", "truck", "bicycle"]


# ---- the restatement --------------------------------------------------------------------------------------------
def inside_all(points, boxes):
    """-> (inside bool [N, M], near bool [N]: the row lies within ROW_MARGIN of the binding face of some box).  A box
    with a non-finite entry contains nothing and is near nothing; a non-finite row is in no box."""
    n, m = len(points), len(boxes)
    inside, near = np.zeros((n, m), bool), np.zeros(n, bool)
    finite = np.isfinite(points[:, :3].astype(np.float64)).all(axis=1)
    for j in range(m):
        if not np.isfinite(boxes[j, :7].astype(np.float64)).all():
            continue
        with np.errstate(invalid="ignore"):
            ins, nr = inside_margin(points[:, :3], boxes[j, :7])
        inside[:, j] = ins & finite
        near |= nr & finite
    return inside, near


def owners(points, seg, boxes, box_off):
    """-> (owner int32 [rows]: index within the scene of the first containing box or -1, number of near rows)."""
    owner = np.full(len(points), -1, np.int32)
    near_rows = 0
    for b in range(len(seg) - 1):
        p, bx = points[seg[b]:seg[b + 1]], boxes[box_off[b]:box_off[b + 1]]
        inside, near = inside_all(p, bx)
        near_rows += int(near.sum())
        if inside.shape[1]:
            owner[seg[b]:seg[b + 1]] = np.where(inside.any(axis=1), inside.argmax(axis=1), -1)
    return owner, near_rows


def extract(points, seg, boxes, box_off, owner):
    """-> (clouds f32 [total, D] in (scene, box) order, rows per box int64 [Mtot])."""
    clouds, counts = [], []
    for b in range(len(seg) - 1):
        p, o = points[seg[b]:seg[b + 1]], owner[seg[b]:seg[b + 1]]
        for i in range(box_off[b + 1] - box_off[b]):
            r = p[o == i].copy()
            r[:, :3] = r[:, :3] - boxes[box_off[b] + i, :3].astype(np.float32)       # float32 - float32
            clouds.append(r)
            counts.append(len(r))
    out = np.concatenate(clouds) if clouds else np.zeros((0, points.shape[1]), np.float32)
    return out.astype(np.float32, copy=False), np.asarray(counts, np.int64)


def brute_owner(points, boxes):
    """The same rule as a plain loop (math, float64): for the check of the restatement itself."""
    out = []
    for p in points:
        own = -1
        for j, b in enumerate(boxes):
            b = [float(np.float32(v)) for v in b[:7]]
            if not all(math.isfinite(v) for v in b) or not all(math.isfinite(float(v)) for v in p[:3]):
                continue
            sx, sy = float(p[0]) - b[0], float(p[1]) - b[1]
            lx = sx * math.cos(b[6]) + sy * math.sin(b[6])
            ly = -sx * math.sin(b[6]) + sy * math.cos(b[6])
            if abs(float(p[2]) - b[2]) <= b[5] / 2 and abs(lx) < b[3] / 2 + 1e-5 and abs(ly) < b[4] / 2 + 1e-5:
                own = j
                break
        out.append(own)
    return np.asarray(out, np.int32)


# ---- generators -------------------------------------------------------------------------------------------------
def grid_boxes(rng, n, W=9, nx=12, pitch=8.0):
    """n boxes, one per cell of an nx-wide grid of ``pitch`` metres: dx <= 5, dy <= 2.5, any yaw, so the diagonal stays
    below the pitch less the jitter and no two of them overlap.  Columns 7.. hold a velocity."""
    b = np.zeros((n, W), np.float32)
    k = np.arange(n)
    ny = (n + nx - 1) // nx
    b[:, 0] = (k % nx - (nx - 1) / 2) * pitch + rng.uniform(-0.5, 0.5, n)
    b[:, 1] = (k // nx - (ny - 1) / 2) * pitch + rng.uniform(-0.5, 0.5, n)
    b[:, 2] = rng.uniform(-1.5, 0.5, n)
    b[:, 3:6] = rng.uniform([1.5, 1.0, 1.0], [5.0, 2.5, 3.0], (n, 3))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    b[:, 7:] = rng.normal(scale=2.0, size=(n, W - 7))
    return b


def _draw(rng, n, boxes, share_in, D):
    """n rows: ``share_in`` of them around the boxes (local coordinates within 0.6 of the extents: most inside, some
    just outside), the rest anywhere in +-45 m.  Column 3 is left for the caller's row ids."""
    p = np.zeros((n, D), np.float32)
    p[:, 0:2] = rng.uniform(-45.0, 45.0, (n, 2))
    p[:, 2] = rng.uniform(-3.0, 2.0, n)
    ok = np.nonzero(np.isfinite(boxes[:, :7]).all(axis=1))[0] if len(boxes) else np.zeros(0, np.int64)
    if len(ok) and share_in > 0:
        pick = np.nonzero(rng.uniform(size=n) < share_in)[0]
        b = boxes[ok[rng.integers(0, len(ok), len(pick))]]
        u = rng.uniform(-0.6, 0.6, (len(pick), 3)) * b[:, 3:6]
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        p[pick, 0] = b[:, 0] + u[:, 0] * c - u[:, 1] * s
        p[pick, 1] = b[:, 1] + u[:, 0] * s + u[:, 1] * c
        p[pick, 2] = b[:, 2] + u[:, 2]
    if D > 4:
        p[:, 4:] = rng.uniform(0, 0.5, (n, D - 4)).astype(np.float32)
    return p


def scene_points(rng, n, boxes, share_in=0.5, D=5, extra=None):
    """n rows for one scene with boxes ``boxes`` (``extra``: rows to put first, e.g. shared points of two boxes); every
    row within ROW_MARGIN of a face of any of the scene's boxes is drawn again until none is left; ids in column 3."""
    p = _draw(rng, n, boxes, share_in, D)
    if extra is not None:
        p[:len(extra), :3] = extra
    for _ in range(100):
        near = inside_all(p, boxes)[1]
        if not near.any():
            break
        p[near] = _draw(rng, int(near.sum()), boxes, 0.0, D)
    assert np.abs(p[:, :3]).max() < LIMIT
    p[:, 3] = np.arange(n)
    return p


def _centre_rows(rng, box, n, spread=0.2):
    """n positions in the middle of ``box`` (local coordinates within ``spread`` of the extents)."""
    u = rng.uniform(-spread, spread, (n, 3)) * box[3:6]
    c, s = np.cos(box[6]), np.sin(box[6])
    return np.stack([box[0] + u[:, 0] * c - u[:, 1] * s, box[1] + u[:, 0] * s + u[:, 1] * c, box[2] + u[:, 2]], 1)


def _cat(scenes):
    """[(points, boxes)] -> (points, seg, boxes, box_off) back to back."""
    seg = np.concatenate([[0], np.cumsum([len(p) for p, _ in scenes])]).astype(np.int64)
    box_off = np.concatenate([[0], np.cumsum([len(b) for _, b in scenes])]).astype(np.int64)
    return np.concatenate([p for p, _ in scenes]), seg, np.concatenate([b for _, b in scenes]), box_off


OWNER_SEED = 5190113


def owner_case():
    """B = 2: 1 000 rows x 7 boxes and 300 rows x 3 boxes, D = 5, W = 9.  Scene 0: box 4 overlaps box 1 (a copy moved by
    0.4 m) and shares points with it, box 5 holds no point (it sits at (50, 50), the rows stay inside +-45 m), box 6 has
    a NaN yaw; rows 10 and 500 of scene 0 and row 7 of scene 1 have a NaN coordinate.
    -> (points, seg, boxes, box_off)."""
    rng = np.random.default_rng(OWNER_SEED)
    b0 = grid_boxes(rng, 7, nx=3)
    b0[4] = b0[1]
    b0[4, :2] += 0.4
    p0 = scene_points(rng, 1000, b0, extra=_centre_rows(rng, b0[1], 25))
    b0[5, :6] = (50.0, 50.0, 0.0, 2.0, 2.0, 2.0)            # after the draw: moved away from its rows
    b0[6, 6] = np.nan                                       # after the draw: rows lie where the box would be
    b1 = grid_boxes(rng, 3, nx=2)
    p1 = scene_points(rng, 300, b1)
    p0[10, 0], p0[500, 1], p1[7, 2] = np.nan, np.nan, np.nan
    return _cat([(p0, b0), (p1, b1)])


def chunk_case():
    """One scene of 600 rows and 130 boxes (more than two LDS chunks of 64); box 100 is box 10 moved by 0.3 m, so the two
    overlap across chunks and share points.  -> (points, seg, boxes, box_off)."""
    rng = np.random.default_rng(OWNER_SEED + 1)
    b = grid_boxes(rng, 130)
    b[100] = b[10]
    b[100, :2] += 0.3
    p = scene_points(rng, 600, b, share_in=0.6, extra=_centre_rows(rng, b[10], 20))
    return _cat([(p, b)])


def empty_case():
    """Three scenes: 300 rows x 2 boxes, 200 rows x NO box, 257 rows x 3 boxes.  -> (points, seg, boxes, box_off)."""
    rng = np.random.default_rng(OWNER_SEED + 2)
    scenes = []
    for n, m in ((300, 2), (200, 0), (257, 3)):
        b = grid_boxes(rng, m, nx=2)
        scenes.append((scene_points(rng, n, b), b))
    return _cat(scenes)


def builder_scenes():
    """Three scenes of 700, 255 and 1 030 rows for the builder.  Scene 0: box 0 is a truck, box 1 a car that overlaps it
    (shared points go to the truck, also when trucks are not used), box 2 a car without points (at (50, 50)), box 3 a
    small car with three points, box 4 a bicycle, box 5 a "barrier" (not a class of the database).
    -> list of (points f32 [N, 5], boxes f32 [M, 9], names object [M])."""
    rng = np.random.default_rng(OWNER_SEED + 3)
    out = []
    b = grid_boxes(rng, 6, nx=3)
    b[1] = b[0]
    b[1, :2] += 0.4
    b[3, 3:6] = (0.6, 0.6, 0.6)
    extra = np.concatenate([_centre_rows(rng, b[0], 20), _centre_rows(rng, b[3], 3)])
    drawn = b.copy()
    drawn[2:4, 3:6] = np.nan                               # no row is drawn around the empty and the small car
    p = scene_points(rng, 700, drawn, extra=extra)
    b[2, :6] = (50.0, 50.0, 0.0, 2.0, 2.0, 2.0)
    out.append((p, b, np.array(["truck", "car", "car", "car", "bicycle", "barrier"], object)))
    for n, m in ((255, 4), (1030, 9)):
        b = grid_boxes(rng, m, nx=3)
        out.append((scene_points(rng, n, b), b, np.array(CLASSES, object)[rng.integers(0, 3, m)]))
    return out


def paste_scene():
    """One 2 000-row scene with 6 separate boxes, for the round trip through the paste.  -> (points, boxes)."""
    rng = np.random.default_rng(OWNER_SEED + 4)
    b = grid_boxes(rng, 6, nx=3)
    return scene_points(rng, 2000, b), b
