"""numpy restatement of the flip test-time-augmentation merge (csrc/tta_merge.hip).

Maps are lists over tasks of dicts {head: array [rows, c, H, W]}; the views of B samples are stacked view-major
(view v of sample b is row v * B + b); a view is (flip_dx, flip_dy), flip_dx mirroring the x axis (the last array axis).

  merge64    the definition in float64.  hm is averaged as a probability, with 1 - p carried beside p so that the logit
             keeps its relative accuracy at both ends; ``raw=True`` returns the mean probability / mean size instead of
             the logit / log.
  merge32    the same steps one float32 operation at a time, in the kernel's order: view 0's term, + view 1's, ...,
             then * float32(1) / float32(V); sigmoid = 1 / (1 + exp(-h)), logit(m) = log(m) - log1p(-m).
  make_views the inverse: the stacked views whose merge is ``base``.
"""
import numpy as np

HEADS = ("hm", "reg", "height", "dim", "rot", "vel", "iou")
LINEAR = ("reg", "height", "rot", "vel", "iou")


def _spatial(a, view):
    """a[..., y, x] -> a[..., ys, xs] with the view's source pixel: flips are their own inverse."""
    if view[1]:
        a = a[..., ::-1, :]
    if view[0]:
        a = a[..., :, ::-1]
    return a


def _rule(head, a, view, one):
    """The value rule of a flip on the channels of one head (an involution): applied to a view's map it gives the term
    in the unflipped frame, applied to a base map it gives the view's map."""
    fx, fy = view
    a = a.copy()
    if head == "reg":
        if fx:
            a[:, 0] = one - a[:, 0]
        if fy:
            a[:, 1] = one - a[:, 1]
    elif head == "rot":                      # (sin, cos): yaw -> pi - yaw under flip_dx, -> -yaw under flip_dy
        if fy:
            a[:, 0] = -a[:, 0]
        if fx:
            a[:, 1] = -a[:, 1]
    elif head == "vel":
        if fx:
            a[:, 0] = -a[:, 0]
        if fy:
            a[:, 1] = -a[:, 1]
    return a


def _terms(head, a, views, dtype):
    """Per view, the un-flipped term of one head: [V][B, c, H, W]."""
    V = len(views)
    assert a.shape[0] % V == 0, (a.shape, V)
    B = a.shape[0] // V
    return [_rule(head, np.ascontiguousarray(_spatial(a[v * B:(v + 1) * B].astype(dtype), view)), view, dtype(1))
            for v, view in enumerate(views)]


def merge64(tasks, views, no_log, raw=False):
    out = []
    V = len(views)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for heads in tasks:
            res = {}
            for name, a in heads.items():
                t = _terms(name, a, views, np.float64)
                if name == "hm":
                    p = sum(np.where(x >= 0, 1.0 / (1.0 + np.exp(-x)), np.exp(x) / (1.0 + np.exp(x))) for x in t) / V
                    q = sum(np.where(x >= 0, np.exp(-x) / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))) for x in t) / V
                    res[name] = p if raw else np.log(p) - np.log(q)
                elif name == "dim" and not no_log:
                    m = sum(np.exp(x) for x in t) / V
                    res[name] = m if raw else np.log(m)
                else:
                    res[name] = sum(t) / V
            out.append(res)
    return out


def merge32(tasks, views, no_log):
    out = []
    f = np.float32
    inv = f(1) / f(len(views))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for heads in tasks:
            res = {}
            for name, a in heads.items():
                t = _terms(name, a, views, np.float32)
                if name == "hm":
                    t = [f(1) / (f(1) + np.exp(-x)) for x in t]
                elif name == "dim" and not no_log:
                    t = [np.exp(x) for x in t]
                acc = t[0]
                for x in t[1:]:
                    acc = acc + x
                acc = acc * inv
                if name == "hm":
                    acc = np.log(acc) - np.log1p(-acc)
                elif name == "dim" and not no_log:
                    acc = np.log(acc)
                assert acc.dtype == np.float32
                res[name] = acc
            out.append(res)
    return out


def make_views(base, views):
    """base: list over tasks of {head: [B, c, H, W]} -> the [V * B, c, H, W] stack whose merge is base (dtype kept)."""
    out = []
    for heads in base:
        res = {}
        for name, a in heads.items():
            one = a.dtype.type(1)
            res[name] = np.concatenate([np.ascontiguousarray(_spatial(_rule(name, a, view, one), view)) for view in views], 0)
        out.append(res)
    return out


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-x)), np.exp(x) / (1.0 + np.exp(x)))


def random_maps(rng, rows, H, W, ncs=(1, 2), vel=True, iou=True, grid=None):
    """Random head maps for ``rows`` samples: hm logits in [-12, 12], reg in [0, 1), dim in [-2, 3].  ``grid``: every
    value a multiple of 1 / grid (few mantissa bits: sums of up to four equal values and 1 - r are then exact)."""
    def draw(c, lo, hi):
        a = rng.uniform(lo, hi, (rows, c, H, W))
        if grid:
            a = np.floor(a * grid) / grid
        return a.astype(np.float32)
    tasks = []
    for nc in ncs:
        d = {"hm": draw(nc, -12, 12), "reg": draw(2, 0, 1), "height": draw(1, -3, 3), "dim": draw(3, -2, 3),
             "rot": draw(2, -1, 1)}
        if vel:
            d["vel"] = draw(2, -4, 4)
        if iou:
            d["iou"] = draw(1, -1, 1)
        tasks.append(d)
    return tasks


def encode_boxes(boxes, H, W, cell):
    """One 9-column box per pixel -> {reg, height, dim, rot, vel} maps [1, c, H, W] of a BEV range symmetric about 0 with
    square cells of ``cell`` metres, as the head's targets are encoded (layers/center_head.FCOSAssigner): reg = the
    centre's offset from its cell's corner in cells, dim = log size, rot = (sin yaw, cos yaw).  Also returns the pixel
    (iy, ix) of every box."""
    boxes = np.asarray(boxes, np.float64)
    cx = (boxes[:, 0] + W * cell / 2) / cell
    cy = (boxes[:, 1] + H * cell / 2) / cell
    ix, iy = np.floor(cx).astype(int), np.floor(cy).astype(int)
    maps = {"reg": np.zeros((1, 2, H, W)), "height": np.zeros((1, 1, H, W)), "dim": np.zeros((1, 3, H, W)),
            "rot": np.zeros((1, 2, H, W)), "vel": np.zeros((1, 2, H, W))}
    assert len(set(zip(iy.tolist(), ix.tolist()))) == len(boxes), "one box per pixel"
    maps["reg"][0, 0, iy, ix] = cx - ix
    maps["reg"][0, 1, iy, ix] = cy - iy
    maps["height"][0, 0, iy, ix] = boxes[:, 2]
    maps["dim"][0, :, iy, ix] = np.log(boxes[:, 3:6])
    maps["rot"][0, 0, iy, ix] = np.sin(boxes[:, 6])
    maps["rot"][0, 1, iy, ix] = np.cos(boxes[:, 6])
    maps["vel"][0, :, iy, ix] = boxes[:, 7:9]
    return maps, iy, ix
