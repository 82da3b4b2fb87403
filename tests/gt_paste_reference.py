"""float64 numpy restatement of the GT-sampling paste and the seeded generators of its tests.

Collision is the separating-axis test on the two BEV rectangles (``sat_gap`` > 0: disjoint, < 0: overlapping), the
inside test is OpenPCDet's check_pt_in_box3d in float64, the selection rule is DataBaseSampler's, the order is
concatenate([objects in candidate order, scene]), then BDA and the range filter.  Positions are the float32 values the
chain forms (the float64-apply, float32-round transform of csrc/points_xform.h, covered bit for bit by the lidar_prep
tests); only the DECISIONS are taken in float64, and a row / pair whose decision lies within a small margin of its
boundary is reported as ``near`` so that a test can leave it out."""
import numpy as np

PAIR_MARGIN = 1e-3          # |separating-axis gap| below this: the pair is not compared
ROW_MARGIN = 1e-4           # a row this close to a removal-box face or the range limit is not compared
PCR = np.array([-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], np.float32)


# ---- collision and selection ------------------------------------------------------------------------------------
def _corners(b):
    b = np.asarray(b, np.float64)
    c, s = np.cos(b[6]), np.sin(b[6])
    loc = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64) * (b[3] / 2, b[4] / 2)
    return b[:2] + loc @ np.array([[c, s], [-s, c]])


def sat_gap(a, b):
    """Largest separation of the two rectangles over their four edge normals (metres): > 0 the rectangles are disjoint
    and at least that far apart along an axis, < 0 they overlap by that much on every axis.  NaN boxes: +inf."""
    if not (np.isfinite(np.asarray(a[:7], np.float64)).all() and np.isfinite(np.asarray(b[:7], np.float64)).all()):
        return np.inf
    ca, cb = _corners(a), _corners(b)
    gap = -np.inf
    for yaw in (a[6], b[6]):
        for ax in (np.array([np.cos(yaw), np.sin(yaw)]), np.array([-np.sin(yaw), np.cos(yaw)])):
            pa, pb = ca @ ax, cb @ ax
            gap = max(gap, pa.min() - pb.max(), pb.min() - pa.max())
    return float(gap)


def gaps(cand, gt):
    """-> (candidate x scene gaps [Nc, M], candidate x candidate gaps [Nc, Nc] with +inf on the diagonal)."""
    n, m = len(cand), len(gt)
    g1 = np.array([[sat_gap(cand[i], gt[j]) for j in range(m)] for i in range(n)], np.float64).reshape(n, m)
    g2 = np.full((n, n), np.inf)
    for i in range(n):
        for j in range(i + 1, n):
            g2[i, j] = g2[j, i] = sat_gap(cand[i], cand[j])
    return g1, g2


def select(cand, group, gt):
    """DataBaseSampler's rule.  -> (accept bool [Nc], near bool [Nc]: the candidate takes part in a pair whose gap is
    below PAIR_MARGIN, so float32 clipping may decide it (or what depends on it) either way)."""
    cand, group = np.asarray(cand), np.asarray(group)
    n = len(cand)
    g1, g2 = gaps(cand, gt)
    finite = np.isfinite(cand[:, :7].astype(np.float64)).all(axis=1) if n else np.zeros(0, bool)
    accept = np.zeros(n, bool)
    for g in sorted(set(group.tolist())):
        for i in np.nonzero(group == g)[0]:
            same = (group == g)
            ok = finite[i] and not (g1[i] < 0).any()
            ok = ok and not (g2[i][accept & ~same] < 0).any()           # accepted candidates of earlier groups
            ok = ok and not (g2[i][same & finite] < 0).any()            # every other candidate of its own group
            accept[i] = ok
        # (accept of this group is only read by later groups: ``accept & ~same`` above)
    near = (np.abs(g1) < PAIR_MARGIN).any(axis=1) | (np.abs(g2) < PAIR_MARGIN).any(axis=1) if n else np.zeros(0, bool)
    return accept, near


def near_pair_share(cand, gt):
    g1, g2 = gaps(cand, gt)
    iu = np.triu_indices(len(cand), 1)
    vals = np.concatenate([g1.reshape(-1), g2[iu]])
    return float((np.abs(vals) < PAIR_MARGIN).mean()) if len(vals) else 0.0


def lattice_boxes(rng, n, existing=(), cells=10, pitch=9.0, clear=0.05):
    """n boxes on a jittered lattice; every pair (among them and with ``existing``) overlaps or clears by >= clear."""
    out = []
    pool = list(existing)
    while len(out) < n:
        cell = rng.integers(0, cells, 2)
        b = np.zeros(7, np.float32)
        b[:2] = (cell - cells / 2 + 0.5) * pitch + rng.uniform(-3.0, 3.0, 2)
        b[2] = rng.uniform(-1.5, 0.5)
        b[3:6] = rng.uniform([1.5, 1.0, 1.0], [6.0, 3.0, 3.0])
        b[6] = rng.uniform(-np.pi, np.pi)
        if all(abs(sat_gap(b, o)) >= clear for o in pool):
            out.append(b)
            pool.append(b)
    return np.stack(out) if out else np.zeros((0, 7), np.float32)


SELECT_SEED = 20240611


def selection_case():
    """B = 3: (Nc, M) = (0, 5), (40 in 10 groups, 0), (63 in 3 groups, 50); a NaN candidate in sample 1.
    -> list of (cand f32 [Nc, 7], group int32 [Nc], gt f32 [M, 7])."""
    rng = np.random.default_rng(SELECT_SEED)
    s0 = (np.zeros((0, 7), np.float32), np.zeros(0, np.int32), lattice_boxes(rng, 5))
    c1 = lattice_boxes(rng, 40, cells=7)
    c1[17, 4] = np.nan
    s1 = (c1, np.repeat(np.arange(10, dtype=np.int32), 4), np.zeros((0, 7), np.float32))
    g2 = lattice_boxes(rng, 50)
    c2 = lattice_boxes(rng, 63, existing=list(g2))
    s2 = (c2, np.repeat(np.array([2, 5, 9], np.int32), 21), g2)
    return [s0, s1, s2]


# ---- the chain --------------------------------------------------------------------------------------------------
def xform(p, m):
    """csrc/points_xform.h: ((m0 x + m1 y) + m2 z) + m3 in float64, rounded to float32."""
    x, y, z = (p[:, i].astype(np.float64) for i in range(3))
    return np.stack([(((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3]) for k in range(3)], 1).astype(np.float32)


def inside_margin(xyz, box):
    """check_pt_in_box3d in float64 for float32 positions: -> (inside bool [N], near bool [N])."""
    p = xyz.astype(np.float64)
    b = np.asarray(box, np.float32).astype(np.float64)
    sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
    c, s = np.cos(b[6]), np.sin(b[6])
    lx, ly = sx * c + sy * s, -sx * s + sy * c
    mz = b[5] / 2 - np.abs(p[:, 2] - b[2])                      # >= 0 inside
    mx = b[3] / 2 + 1e-5 - np.abs(lx)                           # > 0 inside
    my = b[4] / 2 + 1e-5 - np.abs(ly)
    inside = (mz >= 0) & (mx > 0) & (my > 0)
    lo = np.minimum(np.minimum(mz, mx), my)
    return inside, np.abs(lo) < ROW_MARGIN                       # the binding face is closer than the margin


def chain(clouds, aug, db_points, db_offsets, db_boxes, paste, accept):
    """One sample.  clouds: key frame + sweeps (float32 [Ni, D]); aug: its lidar_aug record (sweep_mats, time_lags,
    bda_mat, range); paste: dict(cand_idx, remove_extra_width) or None; accept: bool per candidate.
    -> (rows f32 [N, D] every input row in output order after all transforms, keep bool [N], near bool [N])."""
    D = clouds[0].shape[1]
    rows, is_obj, gate = [], [], []
    rm = []
    if paste is not None:
        for c, i in enumerate(np.asarray(paste["cand_idx"], np.int64)):
            r = db_points[db_offsets[i]:db_offsets[i + 1]].copy()
            t = np.eye(4)
            t[:3, 3] = db_boxes[i, :3]
            r[:, :3] = xform(r, t)
            rows.append(r)
            is_obj.append(np.ones(len(r), bool))
            gate.append(np.full(len(r), bool(accept[c])))
            if accept[c]:
                b = db_boxes[i, :7].astype(np.float32).copy()
                b[3:6] += np.asarray(paste["remove_extra_width"], np.float32)
                rm.append(b)
    for s, c in enumerate(clouds):
        r = c.copy()
        if s > 0:
            r[:, :3] = xform(c, np.asarray(aug["sweep_mats"][s - 1], np.float64))
        if D == 5:
            r[:, 4] = 0.0 if s == 0 else aug["time_lags"][s - 1]
        rows.append(r)
        is_obj.append(np.zeros(len(r), bool))
        gate.append(np.ones(len(r), bool))
    r, is_obj, keep = np.concatenate(rows), np.concatenate(is_obj), np.concatenate(gate)
    near = np.zeros(len(r), bool)
    for b in rm:
        ins, nr = inside_margin(r[:, :3], b)
        keep &= ~(ins & ~is_obj)
        near |= nr & ~is_obj
    if aug.get("bda_mat") is not None:
        r[:, :3] = xform(r, np.asarray(aug["bda_mat"], np.float64))
    if aug.get("range") is not None:
        q = np.asarray(aug["range"], np.float32).astype(np.float64)
        x, y = r[:, 0].astype(np.float64), r[:, 1].astype(np.float64)
        keep &= (x >= q[0]) & (x <= q[3]) & (y >= q[1]) & (y <= q[4])
        for v, lim in ((x, q[0]), (x, q[3]), (y, q[1]), (y, q[4])):
            near |= np.abs(v - lim) < ROW_MARGIN
    return r, keep, near


# ---- generators of the chain tests --------------------------------------------------------------------------------
CHAIN_SEED = 77012
CLASSES = ["car", "truck", "bicycle"]


def make_database(rng, D=5):
    """12 objects with 1, 5 and 300 rows in turn, box-centred clouds; well separated boxes within 25 m of the origin,
    object 11 entirely outside the range (x = 200 m).  -> (points, offsets, boxes f32 [12, 9], class_ids)."""
    n = 12
    sizes = [1, 5, 300] * 4
    boxes = np.zeros((n, 9), np.float32)
    ang = np.arange(n) * (2 * np.pi / n)
    boxes[:, 0], boxes[:, 1] = 16.0 * np.cos(ang), 16.0 * np.sin(ang)        # a ring: neighbours 8.3 m apart
    boxes[:, :2] += rng.uniform(-0.5, 0.5, (n, 2))
    boxes[:, 2] = rng.uniform(-1.0, 0.0, n)
    boxes[:, 3:6] = rng.uniform([2.0, 1.5, 1.5], [5.0, 2.5, 2.5], (n, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, n)
    boxes[:, 7:9] = rng.normal(scale=2.0, size=(n, 2))
    boxes[11, 0] = 200.0
    pts = []
    for k in range(n):
        u = rng.uniform(-0.5, 0.5, (sizes[k], 3)) * boxes[k, 3:6] * 0.98
        c, s = np.cos(boxes[k, 6]), np.sin(boxes[k, 6])
        p = np.zeros((sizes[k], D), np.float32)
        p[:, 0], p[:, 1], p[:, 2] = u[:, 0] * c - u[:, 1] * s, u[:, 0] * s + u[:, 1] * c, u[:, 2]
        p[:, 3] = 100000 + sum(sizes[:k]) + np.arange(sizes[k])                  # a unique id per row (exact in float32)
        if D > 4:
            p[:, 4] = rng.uniform(0, 0.5, sizes[k]).astype(np.float32)           # a stored time lag: kept
        pts.append(p)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(pts), offsets, boxes, np.arange(n) % 3


def scene(rng, n, D=5):
    """A sample of n scene rows in a key frame and two sweeps (n // 2, n // 4, the rest), dense around the ring of
    database boxes, plus its sweep matrices / time lags."""
    parts = [n // 2, n // 4, n - n // 2 - n // 4]
    clouds = []
    for k in parts:
        p = np.zeros((k, D), np.float32)
        a, rad = rng.uniform(0, 2 * np.pi, k), rng.normal(16.0, 2.5, k)
        p[:, 0], p[:, 1], p[:, 2] = rad * np.cos(a), rad * np.sin(a), rng.uniform(-2.0, 1.0, k)
        p[:, 3] = sum(len(c) for c in clouds) + np.arange(k)                      # a unique id per scene row
        clouds.append(p)
    mats = []
    for _ in range(2):
        a = rng.normal(scale=0.02)
        m = np.eye(4)
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, 3] = rng.normal(scale=[0.5, 0.5, 0.02])
        mats.append(m)
    aug = {"segments": parts, "sweep_mats": np.stack(mats), "time_lags": np.array([0.05, 0.1], np.float32),
           "bda_mat": None, "range": None}
    return clouds, aug


def bda_setup():
    """A fixed BDA: (matrix inputs for bev_transform_matrix, the (rotate, scale, flip_dx, flip_dy) box parameters)."""
    return (20.0, 1.05, (0.3, -0.2, 0.1), True, False), (20.0, 1.05, True, False)


def chain_cases(D=5):
    """The chain tests' inputs: -> (database arrays, {case: list of B = 2 samples}); a sample is
    dict(clouds, aug, paste (cand_idx, cand_group, gt_boxes, remove_extra_width) or None).  Scene rows per sample come
    from {tile - 1, tile, tile + 1, 3 * tile + 7} with tile = 256 (k_lidar's kTile); objects have 1, 5 and 300 rows."""
    rng = np.random.default_rng(CHAIN_SEED)
    db = make_database(rng, D)
    boxes = db[2]
    none = np.zeros((0, 7), np.float32)

    def smp(n, idx=None, groups=None, gt=none, rew=(0.0, 0.0, 0.0)):
        clouds, aug = scene(rng, n, D)
        paste = None if idx is None else {"cand_idx": np.array(idx, np.int64), "cand_group": np.array(groups, np.int32),
                                          "gt_boxes": np.asarray(gt, np.float32), "remove_extra_width": rew}
        return {"clouds": clouds, "aug": aug, "paste": paste}

    hit1 = boxes[1:2, :7].copy()
    hit1[:, :2] += 0.3                                             # a scene box on top of object 1: it is rejected
    cases = {
        # object 11 lies at x = 200 m: accepted, pasted, and gone after the range filter
        "mixed": [smp(255, [0, 1, 2, 5], [0, 0, 0, 1], hit1), smp(256, [2, 11, 4], [0, 1, 2])],
        "extra_width": [smp(257, [0, 2, 5, 8], [0, 1, 1, 3], rew=(0.2, 0.2, 0.2)),
                        smp(775, [3, 4], [0, 0], rew=(0.2, 0.2, 0.2))],
        "all_rejected": [smp(256, [2, 5], [0, 1], boxes[[2, 5], :7]), smp(257, [8], [0], boxes[[8], :7])],
        "no_candidates": [smp(255, [], []), smp(775)],
    }
    return db, cases


def compare_sample(got, rows, keep, near):
    """Device rows ``got`` f32 [K, D] of one sample against the reference (``chain``): every definitely kept row is
    there, bit for bit and in order, and any other row the device kept is a ``near`` row.  Rows are told apart by the
    unique id the generators put in column 3.  -> the number of near rows (for the 1 % cap)."""
    ids_ref = rows[:, 3].astype(np.int64)
    assert len(set(ids_ref.tolist())) == len(ids_ref)
    pos = {int(v): k for k, v in enumerate(ids_ref)}
    where = np.array([pos[int(v)] for v in got[:, 3]], np.int64)
    assert (np.diff(where) > 0).all(), "output order is not the input order"
    kept = np.zeros(len(rows), bool)
    kept[where] = True
    sure = ~near
    assert (kept[sure] == keep[sure]).all(), "a row far from every boundary was kept / dropped wrongly"
    np.testing.assert_array_equal(got.view(np.uint32), rows[where].view(np.uint32))
    return int(near.sum())
