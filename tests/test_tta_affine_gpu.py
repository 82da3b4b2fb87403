"""GPU: the rotation / scale / flip test-time-augmentation merge kernel (csrc/tta_merge_affine.hip through ops.tta) against
the numpy restatement of tests/tta_affine_reference.py.

The bound follows test_tta_merge_gpu.py, per element: |kernel - merge64| <= |merge32 - merge64| + K * eps32 * |value|, with
hm compared as a probability and a logarithmic dim as a size (where they are averaged), K = 4 the factor of that test.  Why
it holds: the linear heads (reg, height, rot, vel, iou, dim under no_log) follow merge32 one float32 operation at a time, so
their error is merge32's own; hm and a logarithmic dim are carried in double and rounded once, and half an ulp of a logit
below 16 in magnitude is at most 4 eps32, which moves the probability by at most 4 eps32 * p (1 - p)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import tta_affine_reference as A
import tta_reference as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
K = 4.0
KMAX = 3
# (B, H, W, pc_range): non-square maps, no multiples of the wave size, more than one workgroup; non-square cells on an
# asymmetric range, and square cells on a symmetric one
SHAPES = {"7x10": (2, 7, 10, [-3.0, -10.0, -5.0, 9.0, 6.0, 3.0]), "33x29": (2, 33, 29, [-11.6, -13.2, -5.0, 11.6, 13.2, 3.0])}
VIEWS = {
    "rot3": [(0.0, 1.0, 0, 0), (7.5, 1.0, 0, 0), (-7.5, 1.0, 0, 0)],
    "scale3": [(0.0, 1.0, 0, 0), (0.0, 0.95, 0, 0), (0.0, 1.05, 0, 0)],
    "flip4_x_rot2": [(r, 1.0, fx, fy) for r in (0.0, 12.5) for fx, fy in ((0, 0), (0, 1), (1, 0), (1, 1))],
    "v16": [(r, s, fx, fy) for r in (0.0, 6.0) for s in (1.0, 0.97) for fx, fy in ((0, 0), (0, 1), (1, 0), (1, 1))],
}
# (nbox, iou head, no_log)
CONFIGS = {"nus_iou_log": (9, True, False), "kitti_plain_nolog": (7, False, True)}


def _to_device(tasks, layout):
    """nchw: one contiguous tensor per head.  packed: channel slices of one channels-last map with every head padded to KMAX
    channels (NaN in the padding), as PackedSepHeads._split hands them out."""
    dev = torch.device("cuda:0")
    if layout == "nchw":
        return [{k: torch.from_numpy(v).to(dev) for k, v in t.items()} for t in tasks]
    rows, _, H, W = tasks[0]["hm"].shape
    n = sum(len(t) for t in tasks)
    z = torch.full((rows, n * KMAX + 2, H, W), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
    out, g = [], 0
    for t in tasks:
        d = {}
        for k, v in t.items():
            z[:, g * KMAX:g * KMAX + v.shape[1]] = torch.from_numpy(v).to(dev)
            d[k] = z[:, g * KMAX:g * KMAX + v.shape[1]]
            g += 1
        out.append(d)
    return out


def _host(outs):
    return [{k: v.cpu().numpy() for k, v in t.items()} for t in outs]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _back(k, no_log):
    if k == "hm":
        return R.sigmoid64
    if k == "dim" and not no_log:
        return lambda x: np.exp(np.asarray(x, np.float64))
    return lambda x: np.asarray(x, np.float64)


def _check(got, tasks, views, pc_range, no_log, what):
    """got (host) against merge32 / merge64 of the stacked views ``tasks``; prints the largest error / bound per head."""
    from unidistill_amd.ops import tta
    _, _, H, W = tasks[0]["hm"].shape
    m32 = A.merge32(tasks, views, pc_range, no_log, params=tta.affine_params(views, pc_range, H, W))
    m64 = A.merge64(tasks, views, pc_range, no_log, raw=True)
    worst = {}
    for t, g in enumerate(got):
        assert set(g) == set(tasks[t]), (set(g), set(tasks[t]))
        for k, a in g.items():
            assert a.dtype == np.float32 and a.shape == m32[t][k].shape, (k, a.shape)
            back, val = _back(k, no_log), m64[t][k]
            err32 = np.abs(back(m32[t][k]) - val)
            bound = err32 + K * EPS32 * np.abs(val)
            err = np.abs(back(a) - val)
            ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
            worst[k] = max(worst.get(k, 0.0), float(ratio.max()))
            assert (err <= bound).all(), (what, t, k, float(ratio.max()))
            if k != "hm" and not (k == "dim" and not no_log):       # the design: these are merge32, bit for bit
                assert np.array_equal(_bits(a), _bits(m32[t][k])), f"{what}: task {t} head {k} is not bitwise merge32"
    print(f"{what}: device error / bound = {worst}")


@pytest.mark.parametrize("views", list(VIEWS), ids=list(VIEWS))
@pytest.mark.parametrize("config", list(CONFIGS), ids=list(CONFIGS))
@pytest.mark.parametrize("layout", ["nchw", "packed"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_merge_against_restatement(hip_lib, shape, layout, config, views):
    from unidistill_amd.ops import tta
    (B, H, W, pc_range), views = SHAPES[shape], VIEWS[views]
    nbox, iou, no_log = CONFIGS[config]
    rng = np.random.default_rng(zlib.crc32(repr((shape, layout, config, views)).encode()))
    tasks = R.random_maps(rng, len(views) * B, H, W, ncs=(1, 2), vel=nbox == 9, iou=iou)
    dheads = _to_device(tasks, layout)
    outs = tta.merge(dheads, views, pc_range, no_log=no_log, nbox=nbox)
    for o in outs:
        for k, v in o.items():
            assert v.shape[0] == B and v.dtype == torch.float32
            assert v.stride(2) == W * v.stride(3)                  # the proposal layer's one-pixel-stride condition
            assert (v.stride(3) == 1) == (layout == "nchw")        # the outputs follow the inputs' layout
    _check(_host(outs), tasks, views, pc_range, no_log, f"{shape} {layout} {config} V={len(views)}")
    again = tta.merge(dheads, views, pc_range, no_log=no_log, nbox=nbox)           # two launches give equal bytes
    for o, a in zip(outs, again):
        for k in o:
            assert np.array_equal(_bits(o[k].cpu().numpy()), _bits(a[k].cpu().numpy())), k


LINEAR = ("reg", "height", "rot", "vel", "iou")
QUARTER_TURNS = [(0.0, 1.0, 0, 0), (90.0, 1.0, 0, 0), (0.0, 1.0, 1, 0), (180.0, 1.0, 0, 1), (270.0, 1.0, 1, 1), (0.0, 1.0, 1, 1),
                 (-90.0, 1.0, 1, 0), (0.0, 1.0, 0, 1)]


@pytest.mark.parametrize("layout", ["nchw", "packed"])
def test_quarter_turns_and_flips_are_exact(hip_lib, layout):
    """Square grid, symmetric range, inputs on multiples of 2^-10: every view hits cell indices with weights 1 and 0, sums of
    eight values and 1 / 8 are exact, so the linear heads ARE the definition's permutation and sign rules (merge64, which is
    exact here), bit for bit; and the flip-only views give the same linear-head bits through ud_tta_merge."""
    from unidistill_amd.ops import tta
    B, H, W = 2, 12, 12
    pc_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    views = QUARTER_TURNS
    for T, _, _, _ in A.transforms(views, pc_range, H, W):
        _, _, fx, fy, valid, _, _ = A.sample_geometry(T.reshape(-1), H, W)
        assert valid.all() and not fx.any() and not fy.any()
    tasks = R.random_maps(np.random.default_rng(11), len(views) * B, H, W, grid=1024)
    got = _host(tta.merge(_to_device(tasks, layout), views, pc_range, no_log=False, nbox=9))
    m64 = A.merge64(tasks, views, pc_range, False)
    for t, g in enumerate(got):
        for k in LINEAR:
            assert np.array_equal(m64[t][k].astype(np.float32).astype(np.float64), m64[t][k])          # exact in float32
            assert np.array_equal(_bits(g[k] + np.float32(0)), _bits(m64[t][k].astype(np.float32) + np.float32(0))), (t, k)
    _check(got, tasks, views, pc_range, False, f"quarter turns {layout}")
    # the flip-only views of the same stack: the new kernel (4-tuples) and the flip kernel (pairs) agree
    flips = [i for i, v in enumerate(views) if v[0] == 0.0]
    sub = [{k: np.concatenate([a[i * B:(i + 1) * B] for i in flips], 0) for k, a in t.items()} for t in tasks]
    dsub = _to_device(sub, layout)
    new = _host(tta.affine_merge(dsub, [views[i] for i in flips], pc_range, no_log=False, nbox=9))
    old = _host(tta.flip_merge(dsub, [views[i][2:] for i in flips], no_log=False, nbox=9))
    for t in range(len(sub)):
        for k in LINEAR:
            assert np.array_equal(_bits(new[t][k] + np.float32(0)), _bits(old[t][k] + np.float32(0))), (t, k)
        for k in ("hm", "dim"):
            assert np.abs(new[t][k].astype(np.float64) - old[t][k]).max() <= 2 * EPS32 * 16, (t, k)


def test_pure_flip_views_take_the_flip_kernel(hip_lib):
    """The public path with pure-flip views, given as 4-tuples: the same bits as flip_merge on the same inputs."""
    from unidistill_amd.ops import tta
    B, H, W = 2, 7, 10
    pc_range = [-5.0, -3.5, -5.0, 5.0, 3.5, 3.0]
    tasks = R.random_maps(np.random.default_rng(12), 3 * B, H, W)
    d = _to_device(tasks, "packed")
    got = _host(tta.merge(d, [(0, 1, 1, 0), (0.0, 1.0, 0, 0), (0, 1, 1, 1)], pc_range, no_log=False, nbox=9))
    want = _host(tta.flip_merge(d, [(1, 0), (0, 0), (1, 1)], no_log=False, nbox=9))
    for t in range(len(tasks)):
        assert set(got[t]) == set(want[t])
        for k in want[t]:
            assert np.array_equal(_bits(got[t][k]), _bits(want[t][k])), (t, k)
    with pytest.raises(ValueError, match="y axis"):                    # and the flip path's range check with it
        tta.merge(d, [(0, 1, 0, 0), (0, 1, 0, 1)], [-5.0, -3.0, -5.0, 5.0, 4.0, 3.0], no_log=False, nbox=9)


@pytest.mark.parametrize("layout", ["nchw", "packed"])
def test_uncovered_ring(hip_lib, layout):
    """A scale-1.25 view leaves an outer ring uncovered: there the result is the merge of the other views alone, bit for bit."""
    from unidistill_amd.ops import tta
    B, H, W = 2, 12, 10
    pc_range = [-5.0, -6.0, -5.0, 5.0, 6.0, 3.0]
    views = [(0.0, 1.0, 0, 0), (0.0, 1.25, 0, 0), (0.0, 1.0, 1, 0)]
    tasks = R.random_maps(np.random.default_rng(13), len(views) * B, H, W)
    ring = ~A.sample_geometry(A.transforms(views, pc_range, H, W)[1][0].reshape(-1), H, W)[4]
    assert ring[0].all() and ring[:, 0].all() and not ring[H // 2, W // 2]
    others = [{k: np.concatenate([a[:B], a[2 * B:]], 0) for k, a in t.items()} for t in tasks]
    got = _host(tta.merge(_to_device(tasks, layout), views, pc_range, no_log=False, nbox=9))
    want = _host(tta.affine_merge(_to_device(others, layout), [views[0], views[2]], pc_range, no_log=False, nbox=9))
    for t in range(len(tasks)):
        for k in got[t]:
            assert np.array_equal(_bits(got[t][k][..., ring]), _bits(want[t][k][..., ring])), (t, k)
            assert not np.array_equal(got[t][k][..., ~ring], want[t][k][..., ~ring]), (t, k)
    _check(got, tasks, views, pc_range, False, f"ring {layout}")


@pytest.mark.parametrize("layout", ["nchw", "packed"])
def test_extreme_logits(hip_lib, layout):
    """Rows of -inf, -40, 40, inf in hm under rotated and scaled views: never NaN, and the mean probability is the definition's."""
    from unidistill_amd.ops import tta
    vals = np.array([-np.inf, -40.0, -40.0, 40.0, 40.0, np.inf, -40.0, np.inf], np.float32)
    B, H, W = 1, len(vals), 9
    pc_range = [-4.5, -4.0, -5.0, 4.5, 4.0, 3.0]
    views = [(0.0, 1.0, 0, 0), (7.5, 1.0, 0, 0), (0.0, 1.05, 1, 0), (90.0, 0.9, 0, 1)]
    tasks = R.random_maps(np.random.default_rng(14), len(views) * B, H, W, ncs=(1, 2))
    for t in tasks:
        t["hm"][:] = vals[None, None, :, None]
    tasks[1]["hm"][:, 1] = np.inf
    tasks[1]["hm"][1:, 0] = -np.inf
    got = _host(tta.merge(_to_device(tasks, layout), views, pc_range, no_log=False, nbox=9))
    want = A.merge64(tasks, views, pc_range, False, raw=True)
    for t, g in enumerate(got):
        assert not any(np.isnan(a).any() for a in g.values())
        assert np.abs(R.sigmoid64(g["hm"]) - want[t]["hm"]).max() <= 1e-6
    assert (got[1]["hm"][:, 1] == np.inf).all() and np.isinf(got[0]["hm"]).any() and np.isfinite(got[0]["hm"]).any()


def test_argument_checks(hip_lib):
    from unidistill_amd.ops import tta
    B, H, W = 1, 6, 8
    pc_range = [-4.0, -3.0, -5.0, 4.0, 3.0, 3.0]
    ident, turn = (0.0, 1.0, 0, 0), (5.0, 1.0, 0, 0)
    tasks = _to_device(R.random_maps(np.random.default_rng(15), 2 * B, H, W), "nchw")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for views in ([ident] + [turn] * 16, [ident, (0.0, 0.0, 0, 0)], [ident, (0.0, float("nan"), 0, 0)], [turn, ident],
                  [ident, turn, turn]):                                   # the last: 2 rows are no multiple of 3 views
        with pytest.raises(ValueError):
            tta.merge(tasks, views, pc_range, no_log=False, nbox=9)
    assert torch.cuda.memory_allocated() == before                       # raised before any output was allocated
    with pytest.raises(RuntimeError, match="GPU only"):
        tta.merge([{k: v.cpu() for k, v in t.items()} for t in tasks], [ident, turn], pc_range, no_log=False, nbox=9)
    # the C entry refuses the same on its own: a good table first, then one fault at a time
    good, ratio = tta.affine_params([ident, turn], pc_range, H, W)
    tta.affine_merge_table(tasks, good, ratio, no_log=False, nbox=9)
    for col, value in ((10, 0.0), (10, -1.0), (10, float("nan")), (10, float("inf")), (2, float("nan")), (7, float("inf"))):
        bad = good.copy()
        bad[1, col] = value
        with pytest.raises(RuntimeError, match="ud_tta_merge_affine"):
            tta.affine_merge_table(tasks, bad, ratio, no_log=False, nbox=9)
    with pytest.raises(RuntimeError, match="ud_tta_merge_affine"):
        tta.affine_merge_table(tasks, good[::-1], ratio, no_log=False, nbox=9)          # view 0 rotated
    with pytest.raises(RuntimeError, match="ud_tta_merge_affine"):
        tta.affine_merge_table(tasks, good, 0.0, no_log=False, nbox=9)
    n = 7
    arr = (ctypes.c_void_p * n)(*[None] * n)
    st = (ctypes.c_longlong * (3 * n))()
    nc = (ctypes.c_int * 1)(1)
    table = (ctypes.c_double * (11 * 17))(*(list(good[0]) * 17))
    for V in (0, 17):
        assert hip_lib.ud_tta_merge_affine(arr, st, arr, st, nc, table, 1.0, V, 1, 1, H, W, 0, None) != 0
    assert hip_lib.ud_tta_merge_affine(arr, st, arr, st, nc, None, 1.0, 1, 1, 1, H, W, 0, None) != 0      # a null table
    assert hip_lib.ud_tta_merge_affine(None, st, arr, st, nc, table, 1.0, 1, 1, 1, H, W, 0, None) != 0
    assert hip_lib.ud_tta_merge_affine(arr, st, arr, st, nc, table, 1.0, 1, 1, 1, H, W, 0, None) != 0     # no hm
    del tasks
