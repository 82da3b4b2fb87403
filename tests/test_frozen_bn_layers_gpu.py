"""GPU: an eval-mode BatchNorm inside a training graph (frozen_bn / frozen_encoder / norm_eval) runs on the hand-written kernels
through every layer that has one: no library BatchNorm op is dispatched, forward or backward, and blocks with frozen BatchNorm
match the same module in float64 PyTorch on the CPU."""
import collections
import copy

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu


class _BnWatch(TorchDispatchMode):
    """Counts every ATen BatchNorm op (aten::native_batch_norm*, cudnn_batch_norm*, miopen_batch_norm*, their _legit / backward
    forms); written after the convolution / GEMM watch of tests/test_no_library_gpu.py."""

    def __init__(self):
        super().__init__()
        self.hits = collections.Counter()
        self.ops = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        self.ops += 1
        if "batch_norm" in name:
            self.hits[(name, tuple(tuple(a.shape) for a in args if torch.is_tensor(a))[:1])] += 1
        return func(*args, **(kwargs or {}))


def _no_bn_op(w):
    assert w.ops > 0
    assert not w.hits, "library BatchNorm ops:\n" + "\n".join(f"{n:4d} x {k}" for k, n in w.hits.most_common())


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _randomize_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.copy_(torch.empty(m.num_features).normal_(0, 0.1, generator=g))
                m.running_var.copy_(torch.empty(m.num_features).uniform_(0.5, 1.5, generator=g))
                m.weight.copy_(torch.empty(m.num_features).uniform_(0.6, 1.4, generator=g))
                m.bias.copy_(torch.empty(m.num_features).normal_(0, 0.2, generator=g))
    return module


def _freeze_bn(module):
    module.train()
    for m in module.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    return module


def test_the_watch_sees_a_library_batchnorm():
    """The watch itself: torch's BatchNorm on the GPU, forward and backward, is counted."""
    bn = torch.nn.BatchNorm2d(16).cuda().eval()
    x = torch.randn(2, 16, 4, 4, device="cuda", requires_grad=True)
    with _BnWatch() as w:
        bn(x).sum().backward()
    assert sum(w.hits.values()) >= 2, w.hits


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("affine_grad", [True, False], ids=["affine", "frozen-affine"])
def test_batchnorm_act_eval_with_a_gradient_runs_no_library_batchnorm(hip_lib, dtype, affine_grad):
    from unidistill_amd import _lib
    from unidistill_amd.layers.dense import batchnorm_act
    bn = _randomize_bn(torch.nn.BatchNorm2d(64, eps=1e-3), 1).cuda().eval()
    bn.requires_grad_(affine_grad)
    x = _cl(torch.randn(2, 64, 9, 13, device="cuda").to(dtype)).requires_grad_(True)
    r = _cl(torch.randn(2, 64, 9, 13, device="cuda").to(dtype)).requires_grad_(True)
    names = ("bn_act.k_fwd", "bn_act.k_bwd_frozen_sums", "bn_act.k_bwd_frozen_dx", "bn_act.k_bwd_reduce", "bn_act.k_bwd_dx")
    for n in names:
        _lib.prof_read(n, reset=True)
    _lib.prof_enable(True)
    try:
        with _BnWatch() as w:
            y = batchnorm_act(bn, x, r, True)
            y.float().square().sum().backward()
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
    _no_bn_op(w)
    assert [_lib.prof_read(n)[1] for n in names] == [1, int(affine_grad), int(not affine_grad), 0, 0]
    assert x.grad is not None and r.grad is not None and (bn.weight.grad is not None) == affine_grad


def test_frozen_fold_cache_is_dropped_by_invalidate_caches(hip_lib):
    """Frozen affine parameters (frozen_encoder): the eval-mode fold is cached per version of the four tensors on running_var;
    ops.invalidate_caches (Trainer.load_state_dict, ema_weights) drops it, a raw rewrite without it would be served stale."""
    from unidistill_amd.ops import bn_act as hb, invalidate_caches
    bn = _randomize_bn(torch.nn.BatchNorm2d(32), 2).cuda().eval().requires_grad_(False)
    x = _cl(torch.randn(1, 32, 3, 5, device="cuda")).requires_grad_(True)
    y0 = hb.bn_act(bn, x).detach().clone()
    assert getattr(bn.running_var, "_ud_bn_eval", None) is not None
    bn.weight.data.mul_(2.0)                                  # .data: no version bump
    assert invalidate_caches(bn) >= 1
    assert getattr(bn.running_var, "_ud_bn_eval", None) is None
    y1 = hb.bn_act(bn, x)
    assert not torch.equal(y0, y1)
    y1.sum().backward()
    assert x.grad is not None and bn.weight.grad is None


def test_resnet50_norm_eval_in_train_mode_runs_no_library_batchnorm(hip_lib, monkeypatch):
    monkeypatch.setenv("UD_RANDOM_INIT", "1")
    from unidistill_amd import train
    from unidistill_amd.layers.image import ResNet
    torch.manual_seed(0)
    net = ResNet(depth=50, norm_eval=True, frozen_stages=0, init_cfg=dict(type="Pretrained", checkpoint="torchvision://resnet50"))
    net.init_weights()
    net = train.to_channels_last(_randomize_bn(net, 3).cuda()).train()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert bns and not any(m.training for m in bns) and net.layer1[0].conv1.training
    before = [(m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()) for m in bns]
    x = torch.randn(1, 3, 64, 96, device="cuda")
    with _BnWatch() as w:
        outs = net(x)
        sum(o.float().square().mean() for o in outs).backward()
    torch.cuda.synchronize()
    _no_bn_op(w)
    for m, (rm, rv, nbt) in zip(bns, before):
        assert torch.equal(m.running_mean, rm) and torch.equal(m.running_var, rv) and torch.equal(m.num_batches_tracked, nbt)
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert net.conv1.weight.grad is None and net.bn1.weight.grad is None            # the frozen stem takes none


def test_sparse_basic_block_with_frozen_bn_runs_no_library_batchnorm(hip_lib):
    from functools import partial
    from unidistill_amd.layers.lidar import SparseBasicBlock
    from unidistill_amd.ops import spconv as sp
    rng = np.random.default_rng(21)
    shape = (2, 7, 18, 20)
    coords = np.argwhere(rng.random(shape) < 0.3).astype(np.int32)
    torch.manual_seed(3)
    norm = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    blk = _freeze_bn(_randomize_bn(SparseBasicBlock(32, 32, norm_fn=norm, indice_key="r"), 4).cuda())
    feat = torch.from_numpy(rng.standard_normal((len(coords), 32)).astype(np.float32)).cuda().requires_grad_(True)
    x = sp.SparseConvTensor(feat, torch.from_numpy(coords).cuda(), shape[1:], shape[0])
    with _BnWatch() as w:
        blk(x).features.square().mean().backward()
    torch.cuda.synchronize()
    _no_bn_op(w)
    assert feat.grad is not None and bool(torch.isfinite(feat.grad).all())
    for m in (blk.bn1, blk.bn2):
        assert m.weight.grad is not None and int(m.num_batches_tracked) == 0
    assert blk.conv1.weight.grad is not None and float(blk.conv1.weight.grad.abs().max()) > 0


def test_fp32_packed_head_with_frozen_bn_runs_no_library_batchnorm(hip_lib):
    """The packed head in fp32 mode, BatchNorm in eval, input requiring a gradient: bn_act on the folded vectors + the grouped
    tail instead of torch.nn.functional.batch_norm."""
    from unidistill_amd import _lib
    from unidistill_amd.layers.center_head import PackedSepHeads
    torch.manual_seed(0)
    heads = [{"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "hm": (2, 2)}, {"reg": (2, 2), "hm": (1, 2)}]
    m = PackedSepHeads(64, heads, head_conv=64, final_kernel=3).cuda().eval()
    with torch.no_grad():
        m.bn_running_mean.normal_(0, 0.1); m.bn_running_var.uniform_(0.5, 1.5)
    before = (m.bn_running_mean.clone(), m.bn_running_var.clone(), m.bn_num_batches_tracked.clone())
    x = _cl(torch.randn(2, 64, 24, 20, device="cuda")).requires_grad_(True)
    with _lib.strict(True), _BnWatch() as w:
        o = m(x)
        sum(v.square().mean() for d in o for v in d.values()).backward()
    torch.cuda.synchronize()
    _no_bn_op(w)
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    assert m.bn_weight.grad is not None and m.c1_weight.grad is not None and m.c2_weight.grad is not None
    for t, b in zip((m.bn_running_mean, m.bn_running_var, m.bn_num_batches_tracked), before):
        assert torch.equal(t, b)


def _block_vs_float64(module, x, run):
    """module (GPU, fp32, train mode with frozen BatchNorm) against its float64 copy on the CPU: output, input gradient and every
    convolution weight gradient.  Bounds: the existing block-level fp32 tests' -- 1e-4 of the output's max
    (test_conv2d_f32_gpu.py::test_fp32_trunk_routes_to_the_fp32_kernels_and_matches_library, test_image_branch_f32_gpu.py against
    float64) and 2e-4 of each gradient's max (test_conv2d_f32_gpu.py::test_fp32_training_step_has_no_library_weight_gradient);
    the input gradient is the same back-propagated chain the first layers' weight gradients are made of and takes their bound.
    The float32 PyTorch module's own error on the CPU is printed next to each figure."""
    ref64 = copy.deepcopy(module).double().cpu()
    ref32 = copy.deepcopy(module).cpu()
    outs = {}
    for tag, mod, xin in (("hip", module, x), ("f64", ref64, x.double().cpu()), ("f32", ref32, x.cpu())):
        mod.zero_grad(set_to_none=True)
        xin = (_cl(xin) if tag == "hip" else xin).detach().requires_grad_(True)
        if tag == "hip":
            with _BnWatch() as w:
                y = run(mod, xin)
                y.square().mean().backward()
            torch.cuda.synchronize()
            _no_bn_op(w)
        else:
            y = run(mod, xin)
            y.square().mean().backward()
        outs[tag] = dict(y=y.detach().double().cpu(), dx=xin.grad.double().cpu(),
                         **{n: p.grad.double().cpu() for n, p in mod.named_parameters() if p.dim() == 4})
    assert len(outs["hip"]) > 3 and set(outs["hip"]) == set(outs["f64"])
    bad = []
    for n, r in outs["f64"].items():
        f = 1e-4 if n == "y" else 2e-4
        e_hip = float((outs["hip"][n] - r).abs().max()) / float(r.abs().max())
        e_f32 = float((outs["f32"][n] - r).abs().max()) / float(r.abs().max())
        print(f"  {n}: hand kernels {e_hip:.2e}, float32 PyTorch (CPU) {e_f32:.2e} of max |float64|, bound {f:.0e}")
        if not e_hip <= f:
            bad.append((n, e_hip, f))
    assert not bad, bad


def test_bev_backbone_block_with_frozen_bn_vs_float64(hip_lib):
    from unidistill_amd.layers.bev import BaseBEVBackbone
    torch.manual_seed(0)
    net = _freeze_bn(_randomize_bn(BaseBEVBackbone([1, 1], [1, 2], [64, 128], [1, 2], [64, 64], 64), 5).cuda())
    x = torch.randn(2, 64, 24, 40, device="cuda")
    _block_vs_float64(net, x, lambda m, t: m(t)[0])


def test_resnet_bottleneck_with_frozen_bn_vs_float64(hip_lib):
    from unidistill_amd.layers.image import Bottleneck
    torch.manual_seed(1)
    net = _freeze_bn(_randomize_bn(Bottleneck(256, 64), 6).cuda())
    x = torch.randn(2, 256, 12, 20, device="cuda")
    _block_vs_float64(net, x, lambda m, t: m(t))


def test_camera_detect_step_with_frozen_bn(hip_lib, monkeypatch):
    """One DetectStep("camera") forward + backward (one camera, one sample) with frozen_bn=True under UD_STRICT: finite loss, the
    camera encoder's BatchNorm buffers bit-identical, a finite non-zero gradient on every trainable convolution weight of the
    encoder, no library BatchNorm op."""
    monkeypatch.setenv("UD_RANDOM_INIT", "1")
    from unidistill_amd import _lib, train
    from unidistill_amd.ops import wgrad_stream
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with _lib.strict(True):
        model = train.build_model("camera", frozen_bn=True)
        tr = train.Trainer(train.DetectStep("camera", model=model), device=dev, channels_last=True)
        enc = model.camera_encoder
        bns = [m for m in enc.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        assert len(bns) > 50 and not any(m.training for m in bns) and model.bev_encoder.training
        before = [(m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()) for m in bns]
        batch = train.synthetic_batch(dev, 1, ncam=1, with_points=False)
        with _BnWatch() as w:
            out = tr.module(batch)
            out["loss"].backward()
            wgrad_stream.join()
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out["loss"]))
    hits = {k: n for k, n in w.hits.items()}
    assert not hits, hits
    for m, (rm, rv, nbt) in zip(bns, before):
        assert torch.equal(m.running_mean, rm) and torch.equal(m.running_var, rv) and torch.equal(m.num_batches_tracked, nbt)
    convs = [(n, p) for n, p in enc.named_parameters() if p.dim() == 4 and p.requires_grad]
    assert len(convs) > 50
    for n, p in convs:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
