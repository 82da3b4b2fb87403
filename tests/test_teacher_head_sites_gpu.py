"""The frozen distillation teacher's head on the work units that hold a response-mask site (csrc/head_sites.hip, the unit list of
k_conv3x3_wino4_f32, the site form of k_gtail_fwd) against the dense run of the same kernels.

At every site with mask > 0 the tail output must equal the dense run's: bit for bit where the unit schedule has no stream-K piece;
where it has one the cut points move with the unit list, so the summation order may differ, and the bound is the one
tests/test_conv2d_f32_gpu.py applies to the F(4x4) forward against float64 (1e-4 of the output's max).  Everywhere else the output
is exactly zero.  The hidden tensor is pre-filled with NaN: a finite output at every site proves that the tail reads no unit the
convolution skipped (the one-pixel dilation and the rounding to unit footprints)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F4_BOUND = 1e-4          # tests/test_conv2d_f32_gpu.py::test_conv3x3_winograd_f4_kernel_vs_fp64: of the output's max
GRID = 256               # persistent workgroups of the F(4x4) launch


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _has_stream_k(units, nchunks):
    """The launcher's rule (csrc/conv2d_f32_wino4.hip: w4_sched_core) at its default mode."""
    G = min(units, GRID)
    r = units % G if G else 0
    if not r:
        return False
    ln = -(-r * nchunks // G)
    ln += ln & 1
    return ln + 16 < (nchunks + 8) * 9 // 10


def _masks(B, H, W, block, strip):
    """name -> mask f32[B, H, W].  block / strip: (width, height) in pixels of the convolution's units and the tail's strips."""
    z = lambda: torch.zeros(B, H, W)
    out = {"zero": z(), "all": torch.rand(B, H, W) * 0.9 + 0.1}
    m = z(); m[0, 0, 0] = 1.0; out["corner"] = m
    m = z(); m[1, H - 1, W // 2] = 0.5; out["last-row"] = m
    m = z(); m[0, H // 2, W - 1] = 0.25; out["last-col"] = m
    # one pixel on each side of the first unit boundary and of the first strip boundary that lie inside the map
    for name, (uw, uh) in (("unit", block), ("strip", strip)):
        if uh < H:
            m = z(); m[0, uh - 1, 3] = 1.0; out[name + "-edge-above"] = m
            m = z(); m[0, uh, 3] = 1.0; out[name + "-edge-below"] = m
        if uw < W:
            m = z(); m[1, 2, uw - 1] = 1.0; out[name + "-edge-left"] = m
            m = z(); m[1, 2, uw] = 1.0; out[name + "-edge-right"] = m
    m = z()
    m[0, 1:5, 2:7] = torch.rand(4, 5) + 0.01
    m[1, H - 4:H - 1, W - 6:W - 2] = torch.rand(3, 4) + 0.01
    out["two-blobs"] = m
    return out


class _Case:
    """One (G, KM, H, W): inputs, parameters and the dense run, shared by the masks."""

    def __init__(self, G, KM, H, W, sk):
        from unidistill_amd import _lib
        from unidistill_amd.ops import conv2d_f32 as c, head_tail_f32 as ht
        self.G, self.KM, self.H, self.W, self.B = G, KM, H, W, 2
        g = torch.Generator().manual_seed(G * 1000 + KM * 100 + H)
        C = G * 64
        self.x = _cl(torch.randn(2, 64, H, W, generator=g).cuda())
        self.w1 = (torch.randn(C, 64, 3, 3, generator=g) * (9 * 64) ** -0.5).cuda()
        self.b1 = torch.randn(C, generator=g).cuda()
        self.bn = [t.cuda() for t in (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1,
                                      torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5)]   # gamma, beta, mean, var
        self.w2 = (torch.randn(G * KM, 64, 3, 3, generator=g) * (9 * 64) ** -0.5).cuda()
        self.b2 = torch.randn(G * KM, generator=g).cuda()
        self.sk = sk
        lib = _lib.load()
        lib.ud_conv3x3_wino4_stream_k(sk)
        try:
            with torch.no_grad():
                self.y = c._launch3(self.x, self.w1, self.b1)
                gm, bt, mean, var = self.bn
                self.z = ht.bn_relu_group_tail(self.y, gm, bt, mean, var, False, 0.1, 1e-5, None, None, self.w2, self.b2, G, KM)
        finally:
            lib.ud_conv3x3_wino4_stream_k(-1)

    def restricted(self, mask):
        from unidistill_amd import _lib
        from unidistill_amd.ops import conv2d_f32 as c, head_sites, head_tail_f32 as ht
        lib = _lib.load()
        lib.ud_conv3x3_wino4_stream_k(self.sk)
        try:
            sites = head_sites.build(mask, self.G, self.KM)
            y = torch.full_like(self.y, float("nan"))
            c.conv3x3_units(self.x, self.w1, self.b1, sites.conv_units, y=y)
            gm, bt, mean, var = self.bn
            z = ht.bn_relu_group_tail_sites(y, gm, bt, mean, var, 1e-5, self.w2, self.b2, self.G, self.KM, sites)
        finally:
            lib.ud_conv3x3_wino4_stream_k(-1)
        return sites, y, z


@pytest.fixture(scope="module")
def small_maps():
    from unidistill_amd.ops import conv2d_f32 as c
    old = (c.USE_WINOGRAD, c.WINO4_MIN_FILL, c.USE_WINO4)
    c.USE_WINOGRAD, c.WINO4_MIN_FILL, c.USE_WINO4 = True, 0.0, True      # the F(4x4) kernel on maps that do not fill its blocks
    yield
    c.USE_WINOGRAD, c.WINO4_MIN_FILL, c.USE_WINO4 = old


_cases = {}


def _case(key):
    if key not in _cases:
        _cases[key] = _Case(*key)
    return _cases[key]


# (G, KM, H, W, stream-K mode): G = 3 never reaches a stream-K tail (12 units at most); G = 130 does with two and four listed
# blocks at 20 x 20 (260 / 520 units on 256 workgroups) and with both blocks at 13 x 19 -- run with the tail (mode 2: the bound)
# and held to whole units (mode 0: bit-identical)
CASES = [(3, 1, 20, 20, 2), (3, 2, 13, 19, 2), (3, 3, 20, 20, 2), (3, 3, 13, 19, 2),
         (130, 3, 20, 20, 2), (130, 3, 20, 20, 0), (130, 2, 13, 19, 2), (130, 2, 13, 19, 0)]


@pytest.mark.parametrize("key", CASES, ids=lambda k: "G%d-KM%d-%dx%d-sk%d" % k)
def test_restricted_head_matches_dense_on_mask_sites(hip_lib, small_maps, key):
    case = _case(key)
    G, KM, H, W, sk = key
    from unidistill_amd.ops import conv2d_f32 as c
    block = c.unit_block_pixels(H, W)
    strip = (16, hip_lib.ud_head_tail_f32_strip_rows(2, H, W, G, KM))
    nblk = 2 * (-(-W // block[0])) * (-(-H // block[1]))
    if sk == 2 and G == 130:      # the wide case does take the stream-K tail + fix-up when every block is listed
        assert _has_stream_k(nblk * G, 16)
    if G == 3:
        assert not any(_has_stream_k(n * G, 16) for n in range(nblk + 1))
    torch.manual_seed(7)
    zmax = float(case.z.abs().max())
    for name, m in _masks(2, H, W, block, strip).items():
        mask = m.cuda()
        sites, y, z = case.restricted(mask)
        on = (mask > 0)[:, None].expand_as(z)
        n_units = int(sites.conv_units[0])
        # bit-identical unless a stream-K piece exists in either schedule (the dense run walks all nblk blocks)
        exact = sk == 0 or not (_has_stream_k(n_units * G, 16) or _has_stream_k(nblk * G, 16))
        diff = float((z - case.z)[on].abs().max()) if bool(on.any()) else 0.0
        print(f"{name}: units {n_units}/{nblk} strips {int(sites.tail_strips[0])}/{sites.tail_strips.numel() - 1} "
              f"max |restricted - dense| on sites {diff:.3e} (exact required: {exact})")
        assert bool(torch.isfinite(z).all()), name
        assert torch.count_nonzero(z[~on]) == 0, name                       # exactly zero off the sites
        if exact:
            assert torch.equal(z[on], case.z[on]), name
        else:
            assert diff <= F4_BOUND * zmax, (name, diff, zmax)
        # the lists: ascending, and exactly the units / strips the rule names
        units = sites.conv_units[1:1 + n_units].cpu()
        assert bool((units[1:] > units[:-1]).all())
        grown = torch.nn.functional.max_pool2d((mask > 0).float()[:, None], 3, 1, 1)
        want = torch.nn.functional.max_pool2d(grown, (block[1], block[0]), ceil_mode=True).flatten().nonzero().flatten().cpu()
        assert torch.equal(units.long(), want), name
        ns = int(sites.tail_strips[0])
        wants = torch.nn.functional.max_pool2d((mask > 0).float()[:, None], (strip[1], strip[0]), ceil_mode=True)
        assert torch.equal(sites.tail_strips[1:1 + ns].cpu().long(), wants.flatten().nonzero().flatten().cpu()), name
        # skipped units keep what the hidden tensor held; listed units hold the dense values (to the same rule)
        listed = torch.nn.functional.interpolate(
            torch.nn.functional.max_pool2d(grown, (block[1], block[0]), ceil_mode=True), scale_factor=(block[1], block[0]))[:, :, :H, :W] > 0
        lh = listed.expand_as(y)
        assert bool(torch.isnan(y[~lh]).all()), name
        if exact:
            assert torch.equal(y[lh], case.y[lh]), name
        elif bool(lh.any()):
            assert float((y - case.y)[lh].abs().max()) <= F4_BOUND * float(case.y.abs().max()), name
        if name == "zero":
            assert n_units == 0 and ns == 0 and torch.count_nonzero(z) == 0 and bool(torch.isnan(y).all())


def test_response_distill_loss_same_with_restricted_teacher_maps(hip_lib, small_maps):
    """PackedSepHeads (one task, seven heads: 28 units, no stream-K piece) frozen in eval mode: ResponseDistillLoss forward and
    backward from the dense and from the restricted teacher maps, bit for bit."""
    from unidistill_amd.layers.center_head import PackedSepHeads
    from unidistill_amd.ops import distill as D
    torch.manual_seed(11)
    heads = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2), iou=(1, 2), hm=(2, 2))
    B, H, W = 2, 20, 20
    t_head = PackedSepHeads(64, [heads]).cuda().eval()
    with torch.no_grad():
        t_head.bn_running_mean.normal_(0, 0.1)
        t_head.bn_running_var.uniform_(0.5, 1.5)
        t_head.c2_weight.normal_(0, 0.05)
    for p in t_head.parameters():
        p.requires_grad = False
    x = _cl(torch.randn(B, 64, H, W, device="cuda"))
    mask = torch.zeros(B, H, W, device="cuda")
    mask[0, 2:7, 3:8] = torch.rand(5, 5, device="cuda") + 0.01
    mask[1, 15:19, 14:20] = torch.rand(4, 6, device="cuda") + 0.01
    with torch.no_grad():
        dense = t_head(x)
        restricted = t_head(x, site_mask=mask)
        assert t_head._site_path(x, mask)
    on = mask > 0
    for k in heads:
        assert torch.equal(dense[0][k][on[:, None].expand_as(dense[0][k])], restricted[0][k][on[:, None].expand_as(dense[0][k])])
        assert torch.count_nonzero(restricted[0][k][~on[:, None].expand_as(dense[0][k])]) == 0
    student = [{k: (torch.rand(B, n, H, W, device="cuda") * 0.98 + 0.01) for k, (n, _) in heads.items()}]
    results = []
    for teacher in (dense, restricted):
        s = [{k: v.clone().requires_grad_(True) for k, v in student[0].items()}]
        lc, lr = D.ResponseDistillLoss(s, teacher, None, None, None, None, clamp=1e-4, weight=mask.sum(), mask=mask)
        (lc + lr).backward()
        results.append((lc.detach(), lr.detach(), [s[0][k].grad for k in heads]))
    (lc0, lr0, g0), (lc1, lr1, g1) = results
    assert torch.equal(lc0, lc1) and torch.equal(lr0, lr1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # grad mode on, or a training-mode head: the full map, as before
    assert not t_head.train()._site_path(x, mask)
    t_head.eval()
    with torch.enable_grad():
        assert not t_head._site_path(x, mask)
