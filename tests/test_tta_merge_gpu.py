"""GPU: the flip test-time-augmentation merge kernel (csrc/tta_merge.hip through ops.tta.flip_merge) against the numpy
restatement of tests/tta_reference.py.

Linear heads (reg, height, rot, vel, iou, and dim under no_log) are bitwise merge32: their arithmetic is 1 - r, a negation,
up to three additions and one multiplication, none of which can be contracted.  hm and dim are compared where they are
averaged -- as probability / size -- with merge64; the bound is 4x the largest error merge32 itself shows against merge64 on
the same inputs plus eps32 * value (device expf / logf differ from libm by a few ulp)."""
import zlib

import numpy as np
import pytest
import torch

import tta_reference as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
KMAX = 3
SHAPES = [(2, 5, 7), (1, 6, 10), (2, 3, 257)]          # odd centre line; H != W; a row longer than a wave
VIEWS = {"v1": ((0, 0),), "v2_flipped_first": ((1, 0), (0, 0)), "v4": ((0, 0), (0, 1), (1, 0), (1, 1)),
         "v4_shuffled": ((1, 1), (0, 0), (0, 1), (1, 0))}
# (nbox, iou head, no_log)
CONFIGS = {"nus_iou_log": (9, True, False), "kitti_plain_nolog": (7, False, True)}


def _to_device(tasks, layout):
    """nchw: one contiguous tensor per head.  packed: channel slices of one channels-last map with every head padded to
    KMAX channels, as PackedSepHeads._split hands them out."""
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


def _check(got, tasks, views, no_log, what):
    """got (host) against merge32 / merge64 of the stacked views ``tasks``; prints the observed error over the bound."""
    m32, m64 = R.merge32(tasks, views, no_log), R.merge64(tasks, views, no_log, raw=True)
    worst = {}
    for t, g in enumerate(got):
        assert set(g) == set(tasks[t]), (set(g), set(tasks[t]))
        for k, a in g.items():
            assert a.dtype == np.float32 and a.shape == m32[t][k].shape, (k, a.shape)
            if k in R.LINEAR or (k == "dim" and no_log):
                assert np.array_equal(_bits(a), _bits(m32[t][k])), f"{what}: task {t} head {k} is not bitwise merge32"
                continue
            val = m64[t][k]
            back = R.sigmoid64 if k == "hm" else (lambda x: np.exp(np.asarray(x, np.float64)))
            err32 = np.abs(back(m32[t][k]) - val).max()
            bound = 4.0 * err32 + EPS32 * np.abs(val)
            err = np.abs(back(a) - val)
            worst[k] = max(worst.get(k, 0.0), float((err / bound).max()))
            assert err32 > 0 and (err <= bound).all(), (what, t, k, float(err.max()), float(err32))
    print(f"{what}: device error / bound = {worst}")


@pytest.mark.parametrize("views", list(VIEWS), ids=list(VIEWS))
@pytest.mark.parametrize("config", list(CONFIGS), ids=list(CONFIGS))
@pytest.mark.parametrize("layout", ["nchw", "packed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_merge_against_restatement(hip_lib, shape, layout, config, views):
    from unidistill_amd.ops import tta
    (B, H, W), views = shape, VIEWS[views]
    nbox, iou, no_log = CONFIGS[config]
    rng = np.random.default_rng(zlib.crc32(repr((shape, layout, config, views)).encode()))
    tasks = R.random_maps(rng, len(views) * B, H, W, ncs=(1, 2), vel=nbox == 9, iou=iou)
    dheads = _to_device(tasks, layout)
    outs = tta.flip_merge(dheads, views, no_log=no_log, nbox=nbox)
    for o in outs:
        for k, v in o.items():
            assert v.shape[0] == B and v.dtype == torch.float32
            assert v.stride(2) == W * v.stride(3)                  # the proposal layer's one-pixel-stride condition
            assert (v.stride(3) == 1) == (layout == "nchw")        # the outputs follow the inputs' layout
    _check(_host(outs), tasks, views, no_log, f"{shape} {layout} {config} V={len(views)}")
    again = tta.flip_merge(dheads, views, no_log=no_log, nbox=nbox)         # two runs give equal bytes
    for o, a in zip(outs, again):
        for k in o:
            assert np.array_equal(_bits(o[k].cpu().numpy()), _bits(a[k].cpu().numpy())), k


def test_vel_is_left_out_of_seven_column_boxes(hip_lib):
    from unidistill_amd.ops import tta
    rng = np.random.default_rng(1)
    tasks = R.random_maps(rng, 4, 5, 7, vel=True, iou=True)
    outs = tta.flip_merge(_to_device(tasks, "nchw"), VIEWS["v2_flipped_first"], no_log=False, nbox=7)
    assert all("vel" not in o and "iou" in o for o in outs)
    _check(_host(outs), [{k: v for k, v in t.items() if k != "vel"} for t in tasks], VIEWS["v2_flipped_first"], False, "nbox 7")


@pytest.mark.parametrize("layout", ["nchw", "packed"])
@pytest.mark.parametrize("views", ["v2_flipped_first", "v4"])
def test_identity_on_exact_values(hip_lib, layout, views):
    """base on multiples of 2^-10 (1 - r, and the sum of up to four equal values, are exact): the merge of make_views(base)
    gives the linear heads back bit for bit, and hm / dim within the bound."""
    from unidistill_amd.ops import tta
    views = VIEWS[views]
    rng = np.random.default_rng(2)
    base = R.random_maps(rng, 2, 6, 10, grid=1024)
    stack = R.make_views(base, views)
    got = _host(tta.flip_merge(_to_device(stack, layout), views, no_log=False, nbox=9))
    for t, g in enumerate(got):
        for k in R.LINEAR:
            assert np.array_equal(_bits(g[k]), _bits(base[t][k] + np.float32(0))), (t, k)     # (+ 0: a base -0 comes back as +0)
    _check(got, stack, views, False, f"identity {layout} V={len(views)}")
    for t, g in enumerate(got):                                       # and against the base itself, same bound
        for k, back in (("hm", R.sigmoid64), ("dim", lambda x: np.exp(np.asarray(x, np.float64)))):
            val = back(base[t][k])
            err32 = np.abs(back(R.merge32(stack, views, False)[t][k]) - val).max()
            assert (np.abs(back(g[k]) - val) <= 4.0 * err32 + EPS32 * val).all(), (t, k)


@pytest.mark.parametrize("layout", ["nchw", "packed"])
def test_extreme_logits(hip_lib, layout):
    """Rows of +-30, +-90, +-200: never NaN; where every view holds the same value the output rises with it (+-inf allowed)."""
    from unidistill_amd.ops import tta
    vals = np.array([-200.0, -90.0, -30.0, 30.0, 90.0, 200.0], np.float32)
    H, W, B = len(vals), 7, 1
    base = R.random_maps(np.random.default_rng(6), B, H, W, ncs=(1,))
    base[0]["hm"][:] = vals[None, None, :, None]
    # x flips keep the rows: every view holds the row's value
    views = ((0, 0), (1, 0))
    out = _host(tta.flip_merge(_to_device(R.make_views(base, views), layout), views, no_log=False, nbox=9))[0]["hm"]
    assert not np.isnan(out).any()
    rows = out[0, 0, :, 0].astype(np.float64)
    assert all(rows[i] <= rows[i + 1] for i in range(H - 1)), rows
    assert rows[0] <= -199.0 and rows[-1] == np.inf and np.isfinite(rows[2]) and (out == out[..., :1]).all()
    # all four flips, with one view saturated at +200 and one at -200: means of 0s, 1s and values between, all finite
    views = ((0, 0), (0, 1), (1, 0), (1, 1))
    stack = R.make_views(base, views)
    stack[0]["hm"][1] = 200.0
    stack[0]["hm"][2] = -200.0
    out = _host(tta.flip_merge(_to_device(stack, layout), views, no_log=False, nbox=9))[0]
    assert np.isfinite(out["hm"]).all() and np.isfinite(out["dim"]).all()
    want = R.merge64(stack, views, False, raw=True)[0]["hm"]
    assert 0.25 <= want.min() and want.max() <= 0.75 and np.abs(R.sigmoid64(out["hm"]) - want).max() <= 1e-6


def test_argument_checks(hip_lib):
    """V = 0, V = 5 and a batch that is no multiple of V raise before any launch (the outputs are never allocated)."""
    from unidistill_amd.ops import tta
    tasks = _to_device(R.random_maps(np.random.default_rng(7), 6, 3, 4), "nchw")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for views in ([], [(0, 0)] * 5, [(0, 0), (1, 0), (0, 1), (1, 1)]):                # 6 rows are no multiple of 4
        with pytest.raises(ValueError):
            tta.flip_merge(tasks, views, no_log=False, nbox=9)
    with pytest.raises(ValueError):
        tta.flip_merge(tasks, [(0, 0), (1, 0)], no_log=False, nbox=8)
    bad = [dict(t) for t in tasks]
    bad[1]["rot"] = bad[1]["rot"][:, :1]
    with pytest.raises(ValueError, match="rot"):
        tta.flip_merge(bad, [(0, 0), (1, 0)], no_log=False, nbox=9)
    with pytest.raises(RuntimeError, match="GPU only"):
        tta.flip_merge([{k: v.cpu() for k, v in t.items()} for t in tasks], [(0, 0), (1, 0)], no_log=False, nbox=9)
    assert torch.cuda.memory_allocated() == before
    # the C entry refuses the same on its own
    import ctypes
    n = 7
    arr = (ctypes.c_void_p * n)(*[None] * n)
    st = (ctypes.c_longlong * (3 * n))()
    for V in (0, 5):
        assert hip_lib.ud_tta_merge(arr, st, arr, st, (ctypes.c_int * 1)(1), (ctypes.c_int * 10)(), V, 1, 1, 3, 4, 0, None) != 0
    assert hip_lib.ud_tta_merge(arr, st, arr, st, (ctypes.c_int * 1)(1), (ctypes.c_int * 10)(), 2, 1, 1, 3, 4, 0, None) != 0   # no hm
