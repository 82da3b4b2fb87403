"""The case matrix of the target-assignment tests, shared by the CPU file (tensor-op formulations) and the GPU
file (ud_assign_targets): every case is the smallest shape that reaches the path its name says, drawn from a fixed
seed, with its float64 reference (tests/assign_reference.py) computed once and never changed.

Grid and units.  Unless a case says otherwise: out_size_factor 8, voxel 0.25 m, so a cell is 2 m, and the range
starts at (-w, -h) metres for a w x h anchor grid.  Centres are drawn in cells (anchor ix sits at ix) and
quantised to 2^-14 m.  With these dyadic settings the centre in voxel units is exact in float32, so float32 and
float64 squared distances differ by their own rounding only (a few 2^-24, relative); the redraw margin of 1e-5
is far above that, and no decision of a drawn case hangs on float32 rounding -- not on how a sum of squares is
contracted either.  The case `inexact_voxel` keeps the 0.075 m voxel of the nuScenes configuration (not a
float32 number; the range corner is one, as it is there) on a grid small enough (centres < 96 voxels, one
float32 spacing of a centre < 1e-6 cells) for the margin still to cover the rounding of the centre.

Redraws.  A box whose smallest decision margin (see assign_reference) is below MARGIN gets a new centre from the
same distribution; `n_redrawn` counts them, and the tests assert it stays within 1 % of the case's boxes.
"""
import functools
from types import SimpleNamespace

import numpy as np

from assign_reference import assign_reference, encoding_bound

TASKS = [["car"], ["truck", "bus"], ["barrier"]]
NAMES = [n for t in TASKS for n in t]
CLASS_MAP = {n: i + 1 for i, n in enumerate(NAMES)}
NCLS = len(NAMES) + 1                     # size of the class table (ids 0 .. NCLS - 1)
OSF = 8
MARGIN = 1e-5
OUTSIDE = (1, 7, 8, 12, 40)

# id -> (builder name, keyword arguments); launches = 1 where the fused path runs the kernel, 0 where it falls back
_SPECS = {}


def _spec(cid, kind, **kw):
    _SPECS[cid] = (kind, kw)


for _k in (1, 3, 9):
    _spec(f"grid9_top{_k}", "uniform", w=9, h=9, M=1, n_valid=[1, 1], topk=_k)
_spec("grid20x13", "uniform", w=20, h=13, M=40, n_valid=[40, 17])
_spec("grid13x20", "uniform", w=13, h=20, M=40, n_valid=[40, 17])
_spec("grid70x66_scan_carry", "uniform", w=70, h=66, M=60, n_valid=[60])
_spec("grid180_strides", "uniform", w=180, h=180, M=300, n_valid=[300, 290], tasks=2)
_spec("m512_limit", "uniform", w=32, h=32, M=512, n_valid=[512])
_spec("m513_fallback", "uniform", w=32, h=32, M=513, n_valid=[513], launches=0)
_spec("overflow_K50", "uniform", w=32, h=32, M=60, n_valid=[60, 5], one_class=True, max_objs=50)
_spec("overflow_K1", "uniform", w=32, h=32, M=60, n_valid=[60, 5], one_class=True, max_objs=1)
_spec("cols8_no_velocity", "uniform", w=16, h=12, M=12, n_valid=[12, 5], cols=8, with_velocity=False)
_spec("cols8_padded", "uniform", w=16, h=12, M=12, n_valid=[12, 5], cols=8)
_spec("cols10", "uniform", w=16, h=12, M=12, n_valid=[12, 5], cols=10)
_spec("cols12", "uniform", w=16, h=12, M=12, n_valid=[12, 5], cols=12)
_spec("top10_fallback", "uniform", w=16, h=12, M=12, n_valid=[12, 5], topk=10, launches=0)
for _d in OUTSIDE:
    _spec(f"outside_{_d}_cells", "outside", w=32, h=32, D=_d)
_spec("crowded", "crowded", w=32, h=32, M=40)
_spec("class_ids", "class_ids", w=16, h=12)
_spec("degenerate_rows", "degenerate", w=16, h=12)
_spec("inexact_voxel", "uniform", w=12, h=9, M=10, n_valid=[10, 4], voxel=0.075, pc_range=[-4.0, -3.0])
_spec("ties_top3", "ties", w=24, h=12, topk=3)
_spec("ties_top9", "ties", w=24, h=12, topk=9)

CASE_IDS = list(_SPECS)
RANDOM_IDS = [c for c in CASE_IDS if _SPECS[c][0] != "ties"]
TIE_IDS = [c for c in CASE_IDS if _SPECS[c][0] == "ties"]


def _metres(cfg, u, v):
    """Cell coordinates -> metres, quantised to 2^-14 m."""
    cell = OSF * cfg.voxel
    q = lambda m: np.round(np.asarray(m, np.float64) * 16384.0) / 16384.0
    return q(cfg.pc_range[0] + np.asarray(u) * cell), q(cfg.pc_range[1] + np.asarray(v) * cell)


def _fill_rest(rng, gt, b, rows, ids):
    """Everything but the centre of rows `rows` of sample b: z, sizes, yaw over +-6 rad (it wraps), extras, class."""
    n, cols = len(rows), gt.shape[2]
    gt[b, rows, 2] = rng.standard_normal(n)
    gt[b, rows, 3:6] = rng.uniform(0.5, 3.5, (n, 3))
    gt[b, rows, 6] = rng.uniform(-6.0, 6.0, n)
    gt[b, rows, 7:cols - 1] = rng.standard_normal((n, cols - 8))
    gt[b, rows, cols - 1] = ids


def _build_uniform(rng, cfg, M, n_valid, one_class=False, **_):
    """Centres uniform over the anchor range and up to 1.5 cells beyond it."""
    gt = np.zeros((len(n_valid), M, cfg.cols), np.float32)
    top = 1 if one_class else len(cfg.names)
    for b, n in enumerate(n_valid):
        _fill_rest(rng, gt, b, np.arange(n), rng.integers(1, top + 1, n))
    live = [(b, m) for b, n in enumerate(n_valid) for m in range(n)]
    centre = lambda b, m: (rng.uniform(-1.5, cfg.w + 0.5), rng.uniform(-1.5, cfg.h + 0.5))
    return gt, live, centre


def _build_outside(rng, cfg, D, **_):
    """Centres D cells (plus a fraction) outside the outermost anchors.  Sample 0: far outside in x, within half
    a cell of the first / last row; sample 1: the same with x and y exchanged; sample 2: far outside in both;
    sample 3: far outside one border, mid-edge along it."""
    w, h = cfg.w, cfg.h
    far = lambda n, lo: -D if lo else n - 1 + D          # cells; a fraction is added away from the grid
    near = lambda n, lo: 0 if lo else n - 1
    spots = [[("far", lx, "near", ly) for lx in (1, 0) for ly in (1, 0)],
             [("near", lx, "far", ly) for lx in (1, 0) for ly in (1, 0)],
             [("far", lx, "far", ly) for lx in (1, 0) for ly in (1, 0)],
             [("far", 1, "mid", 0), ("far", 0, "mid", 0), ("mid", 0, "far", 1), ("mid", 0, "far", 0)]]
    gt = np.zeros((4, 4, cfg.cols), np.float32)
    for b in range(4):
        _fill_rest(rng, gt, b, np.arange(4), 1 + (np.arange(4) + b) % len(cfg.names))

    def coord(kind, lo, n):
        f = rng.uniform(0.05, 0.45)
        if kind == "far":
            return far(n, lo) + (-f if lo else f)
        if kind == "near":
            return near(n, lo) + (f if lo else -f) * rng.choice([1.0, -1.0])
        return n / 2 + rng.uniform(-0.45, 0.45)

    def centre(b, m):
        kx, lx, ky, ly = spots[b][m]
        return coord(kx, lx, w), coord(ky, ly, h)
    return gt, [(b, m) for b in range(4) for m in range(4)], centre


def _build_crowded(rng, cfg, M, **_):
    """M boxes within 1.5 cells of each other, classes of two tasks: most positives are shared."""
    gt = np.zeros((2, M, cfg.cols), np.float32)
    mid = [(11.3, 20.6), (-0.2, 30.9)]                   # the second crowd straddles a corner of the range
    for b in range(2):
        _fill_rest(rng, gt, b, np.arange(M), rng.integers(1, 4, M))
    centre = lambda b, m: (mid[b][0] + rng.uniform(-0.75, 0.75), mid[b][1] + rng.uniform(-0.75, 0.75))
    return gt, [(b, m) for b in range(2) for m in range(M)], centre


def _build_class_ids(rng, cfg, **_):
    """Ids outside the class table among valid rows: 0, negative, NCLS, 63, 64, 200; 1.9 truncates to 1."""
    ids = [1.0, 2.0, 0.0, -1.0, float(NCLS), 63.0, 64.0, 200.0, 1.9, 3.0, 4.0, 2.0]
    gt = np.zeros((2, len(ids), cfg.cols), np.float32)
    _fill_rest(rng, gt, 0, np.arange(len(ids)), ids)
    _fill_rest(rng, gt, 1, np.arange(len(ids)), ids[::-1])
    centre = lambda b, m: (rng.uniform(-1.5, cfg.w + 0.5), rng.uniform(-1.5, cfg.h + 0.5))
    return gt, [(b, m) for b in range(2) for m in range(len(ids))], centre


def _build_degenerate(rng, cfg, **_):
    """Sample 0: a zero-size box (log 0 = -inf) and an all-zero row before the last valid one; sample 1: all rows
    zero; sample 2: boxes of the first task only, so the other tasks have no member."""
    M = 10
    gt = np.zeros((3, M, cfg.cols), np.float32)
    _fill_rest(rng, gt, 0, np.arange(8), rng.integers(1, len(cfg.names) + 1, 8))
    gt[0, 3, 3:6] = 0.0
    _fill_rest(rng, gt, 2, np.arange(6), np.ones(6))
    live = [(0, m) for m in range(8) if m != 5] + [(2, m) for m in range(6)]
    centre = lambda b, m: (rng.uniform(-1.5, cfg.w + 0.5), rng.uniform(-1.5, cfg.h + 0.5))

    def finish():
        gt[0, 5] = 0.0
    return gt, live, centre, finish


def _build_ties(rng, cfg, **_):
    """Exact ties, every coordinate exact in float32.  The rules the kernel follows, and the reference states:
    among anchors at equal distance the lower anchor index is taken first; among boxes at equal distance from
    a positive the first in task order (class offset, then row) wins.
      rows 0-2  car on an anchor, on the midpoint between two anchors of a row, on the centre of a cell
      row 3     bus and row 4 truck, a quarter cell either side of an anchor: truck is first in task order
      row 5     truck on the corner anchor of the grid
      row 6     barrier on a column midpoint, 12 cells outside the last row: its nearest anchors are one row,
                and the two columns 4.5 cells away tie for the ninth place
    """
    cells = [(3.0, 3.0), (8.5, 3.0), (14.5, 3.5), (5.25, 8.0), (4.75, 8.0), (0.0, 0.0), (11.5, cfg.h - 1 + 12.0)]
    ids = [1, 1, 1, 3, 2, 2, 4]
    gt = np.zeros((1, len(cells), cfg.cols), np.float32)
    _fill_rest(rng, gt, 0, np.arange(len(cells)), ids)
    x, y = _metres(cfg, [c[0] for c in cells], [c[1] for c in cells])
    gt[0, :, 0], gt[0, :, 1] = x, y
    return gt, [], None


_BUILDERS = {"uniform": _build_uniform, "outside": _build_outside, "crowded": _build_crowded,
             "class_ids": _build_class_ids, "degenerate": _build_degenerate, "ties": _build_ties}


def reference_of(cfg, gt):
    return assign_reference(gt, cfg.tasks, cfg.class_map, (cfg.w, cfg.h), OSF, cfg.pc_range, cfg.voxel_size,
                            cfg.topk, cfg.K, cfg.default_box_dims)


@functools.lru_cache(maxsize=None)
def case(cid):
    """-> namespace: the assigner's settings, gt f32[B, M, cols], ref (targets), bound (per task), n_boxes,
    n_redrawn, launches, exact_ties."""
    kind, kw = _SPECS[cid]
    tasks = TASKS[:kw.get("tasks", len(TASKS))]
    voxel = kw.get("voxel", 0.25)
    cfg = SimpleNamespace(
        id=cid, w=kw["w"], h=kw["h"], tasks=tasks, names=[n for t in tasks for n in t],
        class_map={n: CLASS_MAP[n] for t in tasks for n in t}, topk=kw.get("topk", 9),
        max_objs=kw.get("max_objs", 200), K=kw.get("max_objs", 200), with_velocity=kw.get("with_velocity", True),
        cols=kw.get("cols", 10), voxel=voxel, voxel_size=[voxel, voxel],
        pc_range=kw.get("pc_range", [-kw["w"] * OSF * voxel / 2, -kw["h"] * OSF * voxel / 2]), launches=kw.get("launches", 1),
        exact_ties=kind == "ties")
    cfg.default_box_dims = 10 if cfg.with_velocity else 8
    rng = np.random.default_rng(sum(cid.encode()) * 7919 + len(cid))
    built = _BUILDERS[kind](rng, cfg, **kw)
    gt, live, centre = built[:3]
    for b, m in live:
        gt[b, m, 0], gt[b, m, 1] = _metres(cfg, *centre(b, m))
    if len(built) > 3:
        built[3]()
    n_redrawn = 0
    while True:
        ref, margin, row_margin = reference_of(cfg, gt)
        close = [bm for bm in live if row_margin[bm] < MARGIN]
        if cfg.exact_ties or not close:
            break
        for b, m in close:
            gt[b, m, 0], gt[b, m, 1] = _metres(cfg, *centre(b, m))
        n_redrawn += len(close)
    gt.setflags(write=False)
    cfg.gt, cfg.ref, cfg.margin = gt, ref, margin
    cfg.bound = encoding_bound(gt, ref, (cfg.w, cfg.h), OSF, cfg.pc_range, cfg.voxel_size)
    cfg.n_boxes, cfg.n_redrawn = max(len(live), 1), n_redrawn
    return cfg


def make_assigner(cfg):
    from unidistill_amd.layers.center_head import FCOSAssigner
    tasks = [dict(num_class=len(t), class_names=list(t)) for t in cfg.tasks]
    return FCOSAssigner(out_size_factor=OSF, tasks=tasks, dense_reg=1, gaussian_overlap=0.1, max_objs=cfg.max_objs,
                        min_radius=2, mapping=dict(cfg.class_map), grid_size=[cfg.w * OSF, cfg.h * OSF, 40],
                        pc_range=cfg.pc_range, voxel_size=cfg.voxel_size, assign_topk=cfg.topk,
                        with_velocity=cfg.with_velocity)


# largest |error| / bound seen per encoding column in this process (printed by the tests, -s shows it)
worst_ratio = {}


def check(got, cfg, what):
    """Targets of FCOSAssigner.assign_targets (torch, any device) against the case's reference: integer targets
    and heat maps exactly, encodings within the case's bound with infinities in the same places, `_stacked`
    consistent with the per-task outputs."""
    import torch
    ref = cfg.ref
    ncmax = max(len(t) for t in cfg.tasks)
    for t, names in enumerate(cfg.tasks):
        hm, ind, mask, cat = (got[k][t].cpu() for k in ("heatmap", "ind", "mask", "cat"))
        assert hm.dtype == torch.float32 and ind.dtype == torch.int64 and mask.dtype == torch.bool \
            and cat.dtype == torch.int64, (what, t)
        for key, val in (("heatmap", hm), ("ind", ind), ("mask", mask), ("cat", cat)):
            assert val.shape == ref[key][t].shape, (what, key, t, val.shape)
            diff = np.argwhere(val.numpy() != ref[key][t])
            assert diff.size == 0, f"{what}: {key}[{t}] differs at {len(diff)} places, first {diff[0]}"
        enc = got["box_encoding"][t].cpu()
        assert enc.dtype == torch.float32 and enc.shape == ref["box_encoding"][t].shape, (what, t, enc.shape)
        e, r, bnd = enc.numpy().astype(np.float64), ref["box_encoding"][t], cfg.bound[t]
        assert np.array_equal(np.isinf(e), np.isinf(r)) and np.array_equal(np.sign(e[np.isinf(r)]), np.sign(r[np.isinf(r)])), \
            f"{what}: infinities of box_encoding[{t}] differ"
        assert not np.isnan(e).any(), (what, t)
        fin = np.isfinite(r)
        err = np.where(fin, np.abs(np.where(fin, e, 0.0) - np.where(fin, r, 0.0)), 0.0)
        for c in range(err.shape[2]):
            ratio = np.where(bnd[..., c] > 0, err[..., c] / np.where(bnd[..., c] > 0, bnd[..., c], 1.0),
                             np.where(err[..., c] > 0, np.inf, 0.0))
            key = min(c, 8)
            worst_ratio[key] = max(worst_ratio.get(key, 0.0), float(ratio.max(initial=0.0)))
        over = np.argwhere(err > bnd)
        assert over.size == 0, (f"{what}: box_encoding[{t}] beyond its bound at {len(over)} places, first "
                                f"{over[0]}: error {err[tuple(over[0])]:.3e}, bound {bnd[tuple(over[0])]:.3e}")
    st = got["_stacked"]
    assert tuple(st["heatmap"].shape) == (len(cfg.tasks), cfg.gt.shape[0], ncmax, cfg.h, cfg.w), what
    for t, names in enumerate(cfg.tasks):
        shm = st["heatmap"][t].cpu()
        assert torch.equal(shm[:, :len(names)], got["heatmap"][t].cpu()) and not shm[:, len(names):].any(), (what, t)
        for key in ("ind", "mask", "box_encoding"):
            a, b = st[key][t].cpu(), got[key][t].cpu()
            assert a.dtype == b.dtype and torch.equal(a, b), (what, key, t)
