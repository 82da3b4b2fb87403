"""Inputs and layouts the detection-loss tests share; a helper, not a test.

The focal and regression cases of tests/test_det_loss_reference_cpu.py (conditions on the inputs) and tests/test_det_loss_reference_gpu.py
(the kernels against the float64 restatement), each built once on the CPU with its float64 and float32 restatement, and the two head
layouts the kernels are called with (also used by tests/test_det_loss_rot_gpu.py)."""
import functools
import math

import torch

import det_loss_reference as D
import rot_iou_reference as R

SX, SY = 0.6, 0.8
ALPHA, GAMMA = 0.25, 2
WIDTH = (2, 1, 3, 2, 2, 1)          # reg height dim rot vel iou
NAMES = ("reg", "height", "dim", "rot", "vel", "iou")


# ---- head layouts ----------------------------------------------------------------------------------------------------------------
def preds_from_planes(planes, packed, H, W):
    """Head tensors [B, c, H, W] per task from planes [T,B,11,HW]: separate contiguous leaves, or channel slices of ONE packed leaf with
    a spare channel between the heads (what PackedSepHeads returns).  -> (preds, leaves, slots)."""
    T, B = planes.shape[:2]
    preds, leaves = [], []
    if packed:
        pk = torch.zeros(B, T * 11 + T * 6, H, W, device="cuda")
        c = 0
        slots = []
        for t in range(T):
            j = 0
            for wd in WIDTH:
                pk[:, c:c + wd] = planes[t, :, j:j + wd].reshape(B, wd, H, W).cuda()
                slots.append((c, wd))
                c += wd + 1
                j += wd
        pk.requires_grad_(True)
        leaves.append(pk)
        it = iter(slots)
        for t in range(T):
            preds.append({nm: pk[:, c0:c0 + wd] for nm, (c0, wd) in zip(NAMES, (next(it) for _ in NAMES))})
        return preds, leaves, slots
    for t in range(T):
        pd, j = {}, 0
        for nm, wd in zip(NAMES, WIDTH):
            pd[nm] = planes[t, :, j:j + wd].reshape(B, wd, H, W).cuda().contiguous().requires_grad_(True)
            leaves.append(pd[nm])
            j += wd
        preds.append(pd)
    return preds, leaves, None


def plane_grads(leaves, slots, packed, T, B, HW):
    """-> [T,B,11,HW] gradient planes on the CPU (zeros where a head got none)."""
    out = torch.zeros(T, B, 11, HW)
    if packed:
        gr = leaves[0].grad.cpu()
        it = iter(slots)
        for t in range(T):
            j = 0
            for wd in WIDTH:
                c0, _ = next(it)
                out[t, :, j:j + wd] = gr[:, c0:c0 + wd].reshape(B, wd, HW)
                j += wd
        used = torch.zeros(gr.shape[1], dtype=torch.bool)
        for c0, wd in slots:
            used[c0:c0 + wd] = True
        assert float(gr[:, ~used].abs().max()) == 0.0          # the spare channels between the heads stay untouched
        return out
    it = iter(leaves)
    for t in range(T):
        j = 0
        for wd in WIDTH:
            leaf = next(it)
            if leaf.grad is not None:
                out[t, :, j:j + wd] = leaf.grad.cpu().reshape(B, wd, HW)
            j += wd
    return out


def gathered(planes, ind):
    """planes [T,B,11,HW], ind [T,B,K] -> the head values at the slots' pixels [T,B,K,11]."""
    T, B, K = ind.shape
    return planes.gather(3, ind[:, :, None, :].expand(T, B, 11, K)).permute(0, 1, 3, 2)


# ---- focal cases -----------------------------------------------------------------------------------------------------------------
FOCAL_CASES = {
    "two_trips": dict(ncls=(1, 2, 1), B=2, H=96, W=90),                    # n = B ncm HW = 34560 per task: 3 trips of the 16384-thread grid
    "tiny": dict(ncls=(1, 2, 1), B=1, H=5, W=7),                           # n = 70: most blocks idle
    "eight_tasks": dict(ncls=(1, 2, 3, 1, 2, 3, 1, 2), B=1, H=9, W=11),    # the largest task count the kernels take
}
FIXED_LOGITS = (12.0, -12.0, 9.0, -9.0)     # +-12: outside the sigmoid clamp (zero gradient); +-9: just inside (+-log 9999 = +-9.21)


def fixed_positions(ncls_t, B, HW):
    """(b, c, first pixel) of the two runs of four fixed logits in a task: the first pixels of the map, and the last ones."""
    return ((0, 0, 0), (B - 1, ncls_t - 1, HW - 4))


@functools.lru_cache(maxsize=None)
def focal_case(name):
    """-> dict: logits (T f32 tensors [B,ncls_t,H,W]), gt f32 [T,B,ncm,H,W], weights w_pos / w_neg [T] and w_p [T,B,ncm,H,W] (f64), and per
    dtype ("f64", "f32") the restatement's prob, pos, neg and d/dlogits of sum(w_pos pos) + sum(w_neg neg) (+ sum(w_p prob): "dl";
    without: "dl_noprob"), all as float64."""
    cfg = FOCAL_CASES[name]
    ncls, B, H, W = cfg["ncls"], cfg["B"], cfg["H"], cfg["W"]
    T, ncm, HW = len(ncls), max(ncls), H * W
    g = torch.Generator().manual_seed(1000 + len(name))
    logits = []
    for t in range(T):
        x = (torch.randn(B, ncls[t], HW, generator=g, dtype=torch.float64) * 2 - 2.2).float()
        while True:                                       # no logit next to the sigmoid clamp's bounds: redraw, deterministically
            close = (x.abs().double() - D.LOGIT_CLAMP).abs() < 1e-3
            if not bool(close.any()):
                break
            x[close] = (torch.randn(int(close.sum()), generator=g, dtype=torch.float64) * 2 - 2.2).float()
        logits.append(x)
    u = torch.rand(T, B, ncm, HW, generator=g)
    soft = torch.rand(T, B, ncm, HW, generator=g) * 0.9 + 0.05
    gt = torch.zeros(T, B, ncm, HW)
    gt[u < 0.08] = soft[u < 0.08]                        # the Gaussian's slopes: in (0, 1), counted by neither sum
    gt[u < 0.01] = 1.0                                   # exact peaks (in the padded channels too, where nothing may read them)
    for t in range(T):
        for (b, c, p0), vals in zip(fixed_positions(ncls[t], B, HW), ((1.0, 0.0, 1.0, 0.0), (0.0, 1.0, 0.0, 1.0))):
            logits[t][b, c, p0:p0 + 4] = torch.tensor(FIXED_LOGITS)
            gt[t, b, c, p0:p0 + 4] = torch.tensor(vals)
    last = gt[T - 1, :, :ncls[T - 1]]
    last[last == 1] = 0.5                                # the last task has no positive at all
    logits = [x.reshape(B, -1, H, W) for x in logits]
    gt = gt.reshape(T, B, ncm, H, W)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    w_pos, w_neg, w_p = 0.5 + rnd(T), 0.5 + rnd(T), rnd(T, B, ncm, H, W) - 0.5
    out = dict(logits=logits, gt=gt, ncls=ncls, w=(w_pos, w_neg, w_p), shape=(T, B, ncm, H, W))
    for key, dt in (("f64", torch.float64), ("f32", torch.float32)):
        leaves = [x.detach().to(dt).clone().requires_grad_(True) for x in logits]
        prob, pos, neg = D.focal_ref(leaves, gt, ALPHA, GAMMA)
        sums = (w_pos.to(dt) * pos).sum() + (w_neg.to(dt) * neg).sum()
        dl_noprob = torch.autograd.grad(sums, leaves, retain_graph=True)
        dl = torch.autograd.grad(sums + (w_p.to(dt) * prob).sum(), leaves)
        out[key] = dict(prob=prob.detach().double(), pos=pos.detach().double(), neg=neg.detach().double(),
                        dl=[v.double() for v in dl], dl_noprob=[v.double() for v in dl_noprob])
    return out


# ---- regression cases ------------------------------------------------------------------------------------------------------------
T_REG = 3
REG_CASES = {
    "two_trips": dict(B=8, K=300, H=24, W=20),           # 2400 slots per task: a second trip of the 8 x 256 grid, 352 slots long
    "tiny": dict(B=1, K=3, H=9, W=9),
    "edges": dict(B=1, K=32, H=9, W=9),                  # every slot constructed: one decision branch each
}
EDGE_DISTANCE = 0.05                                     # how far every constructed slot stays from every decision


def _random_codes(n, seed):
    """R.random_codes plus velocity and IoU-head columns -> (code f32 [n,11], tgt f32 [n,10]); rows within MARGIN of the nearest-BEV
    switch r = pi/4 (prediction or target) are drawn again, from the next seeds, until none is left."""
    def draw(s):
        g = torch.Generator().manual_seed(7000 + s)
        pred, tcode = R.random_codes(n, SX, SY, seed=s)
        u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1
        return torch.cat([pred, u(n, 2), u(n, 1)], 1).float(), torch.cat([tcode, u(n, 2)], 1).float()
    code, tgt = draw(seed)
    for s in range(seed + 1, seed + 50):
        _, dist = D.bev_target(code.double()[None, None], tgt.double()[None, None], SX, SY)
        close = dist[0, 0] < 2 * R.MARGIN
        if not bool(close.any()):
            return code, tgt
        c2, t2 = draw(s)
        code[close], tgt[close] = c2[close], t2[close]
    raise AssertionError("could not draw codes away from the nearest-BEV switch")


def _edge_slots(t):
    """The 32 constructed slots of task t -> (code f64 [32,11], tgt f64 [32,10], nan_slot).  Boxes are written in metres and encoded;
    code columns 3, 4, 5 are the extents along x, z, y (the loss's pairing), the nearest-BEV box reads 3 and 4."""
    K = REG_CASES["edges"]["K"]
    tb = torch.tensor([0.2 + 0.05 * t, -0.1, 0.3, 4.0, 1.6, 2.0, 0.3])                 # x y z, extents (x, z, y), yaw
    tvel = torch.tensor([0.5, -0.4])
    rows, trows = [], []

    def slot(off=(1.0, -0.6, 0.5), scale=(0.7, 0.7, 0.7), yaw=0.45, r=1.3, tyaw=0.3, logit=None, sincos=None, diou=0.3,
             dvel=(0.2, -0.3)):
        tbox = tb.clone().double()
        tbox[6] = tyaw
        pbox = tbox.clone()
        pbox[:3] += torch.tensor(off, dtype=torch.float64)
        pbox[3:6] *= torch.tensor(scale, dtype=torch.float64)
        pbox[6] = yaw
        code = R.encode(pbox, SX, SY, r)
        for j, v in (logit or {}).items():
            code[3 + j] = v
        if sincos is not None:
            code[6], code[7] = sincos
        vel = tvel.double() + torch.tensor(dvel, dtype=torch.float64)
        rows.append(torch.cat([code, vel, torch.tensor([diou], dtype=torch.float64)]))     # the IoU head: filled in below (tar + diou)
        trows.append(torch.cat([R.encode(tbox, SX, SY), tvel.double()]))

    inside = dict(off=(0.35, 0.12, 0.1))
    slot()                                                            # 0: partial overlap, another side binding in each axis
    slot(off=(4.0, -0.6, 0.5))                                        # 1: no overlap in x
    slot(off=(1.0, -2.5, 0.5))                                        # 2: no overlap in y
    slot(off=(1.0, -0.6, 2.0))                                        # 3: no overlap in z
    slot(**inside)                                                    # 4: prediction strictly inside the target
    slot(**inside, scale=(1.5, 1.5, 1.5))                             # 5: target strictly inside the prediction
    slot(logit={0: 85.0})                                             # 6: a dim logit above the exp guard (80)
    slot(logit={1: math.log(40.0)})                                   # 7: exp above the cap of 30
    slot(off=(1.0, -2.5, 0.5), logit={2: -8.0})                       # 8: exp below the floor of 1e-3 (that axis: no overlap)
    slot(**inside, logit={0: -2.5, 1: -2.5, 2: -2.5})                 # 9: volume below its floor of 1e-3
    slot(sincos=(0.0, 0.0))                                           # 10: atan2(0, 0)
    slot(yaw=math.pi / 4 + EDGE_DISTANCE)                             # 11, 12: either side of the nearest-BEV switch
    slot(yaw=math.pi / 4 - EDGE_DISTANCE, r=1.0)
    slot(yaw=math.pi - 0.02)                                          # 13, 14: either side of atan2's cut
    slot(yaw=-(math.pi - 0.02))
    slot(diou=EDGE_DISTANCE)                                          # 15, 16: the IoU head just above / below its target
    slot(diou=-EDGE_DISTANCE)
    for k in range(17, K):                                            # the rest: the binding sides, signs and the target's switch vary
        sg = -1.0 if k % 2 else 1.0
        slot(off=(sg * (0.9 + 0.02 * k), -sg * (0.5 + 0.01 * k), sg * 0.45), scale=(0.6 + 0.01 * k, 0.95 - 0.01 * k, 0.7),
             yaw=sg * (0.2 + 0.03 * (k - 17)), r=0.6 + 0.04 * k, tyaw=1.2 if k % 3 == 0 else -sg * 0.6, diou=sg * 0.25,
             dvel=(sg * 0.2, 0.15))
    return torch.stack(rows), torch.stack(trows), 17


@functools.lru_cache(maxsize=None)
def reg_inputs(name):
    """-> dict of CPU tensors: planes f32 [T,B,11,HW], ind [T,B,K] (unique per task and sample), mask, tgt f32 [T,B,K,10], num_obj f32 [T],
    w = (w_box [T,10], w_iou [T], w_aw [T]) f64, nan_at = (t, b, k) of the one NaN velocity target."""
    cfg = REG_CASES[name]
    B, K, H, W = cfg["B"], cfg["K"], cfg["H"], cfg["W"]
    T, HW = T_REG, H * W
    g = torch.Generator().manual_seed(300 + len(name))
    ind = torch.stack([torch.randperm(HW, generator=g)[:K] for _ in range(T * B)]).reshape(T, B, K)
    if name == "edges":
        parts = [_edge_slots(t) for t in range(T)]
        code = torch.stack([p[0] for p in parts]).reshape(T, B, K, 11).float()
        tgt = torch.stack([p[1] for p in parts]).reshape(T, B, K, 10).float()
        tar, _ = D.bev_target(code.double(), tgt.double(), SX, SY)           # of the rounded inputs: the IoU head sits diou off it
        code[..., 10] = (tar + code[..., 10].double()).float()
        mask = torch.ones(T, B, K, dtype=torch.bool)
        nan_at = (0, 0, parts[0][2])
        cnt = mask.float().sum(dim=(1, 2))
        num_obj = cnt * torch.tensor([1.0, 0.75, 1.0])
    else:
        code, tgt = _random_codes(T * B * K, seed={"two_trips": 21, "tiny": 2}[name])
        code, tgt = code.reshape(T, B, K, 11), tgt.reshape(T, B, K, 10)
        if name == "two_trips":
            mask = torch.rand(T, B, K, generator=g) < 0.5
            nan_at = (0, 3, 7)
            mask[nan_at] = True
            cnt = mask.float().sum(dim=(1, 2))
            num_obj = cnt * torch.tensor([1.0, 0.75, 1.0])                   # task 1: a fractional cross-rank mean
        else:
            mask = torch.tensor([[[True, True, True]], [[False, True, False]], [[False, False, False]]])
            nan_at = (0, 0, 1)
            num_obj = torch.tensor([3.0, 0.25, 0.0])                         # task 1: one local positive, a mean below 1; task 2: empty
    tgt[nan_at][8] = float("nan")                                            # a NaN velocity target, as nuScenes has them
    planes = (torch.randn(T, B, 11, HW, generator=g, dtype=torch.float64) * 0.3).float()
    planes.scatter_(3, ind[:, :, None, :].expand(T, B, 11, K), code.permute(0, 1, 3, 2))
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    return dict(planes=planes, ind=ind, mask=mask, tgt=tgt, num_obj=num_obj.float(), w=(0.5 + u(T, 10), 0.5 + u(T), 0.5 + u(T)),
                nan_at=nan_at, shape=(T, B, K, H, W))


@functools.lru_cache(maxsize=None)
def reg_case(name, nb, only_box=False):
    """reg_inputs plus, per dtype ("f64", "f32"), the restatement's (box, iou_loss, iou_aware, grad by the gathered values [T,B,K,11],
    margin) as float64; the differentiated sum is sum(w_box box) + sum(w_iou iou_loss) + sum(w_aw iou_aware), or its first term alone."""
    c = dict(reg_inputs(name))
    w_box, w_iou, w_aw = c["w"]
    for key, dt in (("f64", torch.float64), ("f32", torch.float32)):
        gath = gathered(c["planes"].to(dt), c["ind"]).clone().requires_grad_(True)
        box, il, aw, margin = D.reg_ref(gath, c["tgt"].to(dt), c["mask"], c["num_obj"], SX, SY, nb)
        total = (box * w_box[:, :nb].to(dt)).sum()
        if not only_box:
            total = total + (il * w_iou.to(dt)).sum() + (aw * w_aw.to(dt)).sum()
        grad, = torch.autograd.grad(total, gath)
        c[key] = (box.detach().double(), il.detach().double(), aw.detach().double(), grad.double(), margin)
    return c


def positive_pixels_distinct(ind, mask):
    """ind, mask [..., K] -> True if the positive slots of every row name pairwise distinct pixels: what the regression backward, which
    stores and does not accumulate, takes for granted."""
    ind, mask = ind.reshape(-1, ind.shape[-1]).cpu(), mask.reshape(-1, mask.shape[-1]).cpu()
    return all(int(torch.unique(i[m]).numel()) == int(m.sum()) for i, m in zip(ind, mask))
