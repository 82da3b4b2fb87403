"""Float64 BatchNorm (+ residual) (+ ReLU) reference for the streaming kernels of csrc/bn_act.hip, with input conditioning and
per-element error bounds derived from the kernels' arithmetic (not from a tensor's max).

Everything works on [P, C] row tensors (a channels-last map is x.permute(0, 2, 3, 1).reshape(-1, C)) on any device.  Used by
tests/test_bn_reference_cpu.py (the reference against torch, the bounds against mutated results) and by the GPU tests.

Notation of the kernels (bn_act.hip:10-12): scale = gamma * invstd, shift = beta - mean * scale,
z = x * scale + shift (+ residual), y = act(z), dr = dy * [z > 0], dbeta = sum dr, dgamma = invstd * sum dr (x - mean),
dx = scale * dr + k2 * x + k0, k2 = -scale * dgamma / P * invstd, k0 = -scale * dbeta / P - k2 * mean.
"""
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
MARGIN = 1e-3             # conditioned inputs keep every |pre-activation| >= MARGIN (tests assert the bound on z stays below it)


# ---- launch geometry of bn_act.hip (slices_for, stream_grid, the _final kernels): which path a shape reaches -----------------
def geometry(P, C):
    """Mirror of bn_act.hip's launch arithmetic for a [P, C] tensor."""
    gw = 64 if C % 64 == 0 else (32 if C % 32 == 0 else 16)
    groups = C // gw
    lanes = 2048 // gw                                  # GroupMap<GW>::kLanes: pixel lanes of one reduction workgroup
    s = 2048 // max(groups, 1)
    s = min(s, -(-P // lanes))
    s = max(s, 1)
    capped = s > 1024
    slices = min(s, 1024)
    chunks = C // 8
    ch = 1
    while ch < chunks and ch < 256:
        ch <<= 1
    s_lanes = 256 // ch
    cblocks = -(-chunks // ch)
    s_slices = max(min(-(-P // s_lanes), max(4096 // cblocks, 1)), 1)
    final_t = 256 if slices > 128 else 64
    return dict(gw=gw, lanes=lanes, slices=slices, capped=capped, rows_per_lane=-(-P // (slices * lanes)),
                final_t=final_t, stats_unrolled=slices > 48, bwd_unrolled=slices > 3 * final_t,
                stream_ch=ch, stream_lanes=s_lanes, stream_cblocks=cblocks, stream_slices=s_slices,
                trips=-(-P // (s_slices * s_lanes)), pow2_chunks=(chunks & (chunks - 1)) == 0)


def chain_lengths(P, C):
    """Longest fp32 summation chains of the two reductions (Higham: |error| <= gamma_n * sum|terms|, gamma_n ~ n u).
    stats: a lane's rows + the workgroup's sequential lane sum (k_bn_stats_partial); the slices are added in double.
    bwd: the same + k_bn_bwd_final's fp32 pass: <= ceil(slices / T) + 2 adds per thread, 6 shuffle levels, T / 64 waves."""
    g = geometry(P, C)
    n_stats = g["rows_per_lane"] + g["lanes"] + 1
    t = g["final_t"]
    n_bwd = n_stats + -(-g["slices"] // t) + 2 + 6 + t // 64
    return n_stats, n_bwd


# ---- the reference ------------------------------------------------------------------------------------------------------------
def batch_stats(x):
    """-> mean, biased var of float64 rows x [P, C]."""
    x = x.double()
    mean = x.mean(0)
    d = x - mean
    return mean, (d * d).mean(0)


def from_stats(x, mean, var, gamma, beta, eps, residual=None, relu=True, dy=None, mask=None):
    """Forward (and backward when dy is given) of y = act((x - mean) invstd gamma + beta (+ residual)) for given statistics,
    everything float64.  mask overrides the ReLU mask [z > 0] (the tests' mutations)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    P = x.shape[0]
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    xhat = (x - mean) * invstd
    z = xhat * gamma + beta
    if residual is not None:
        z = z + residual.double()
    if mask is None:
        mask = z > 0
    y = torch.where(mask, z, torch.zeros_like(z)) if relu else z
    out = dict(z=z, y=y, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift)
    if dy is None:
        return out
    dy = dy.double()
    dr = torch.where(mask, dy, torch.zeros_like(dy)) if relu else dy
    dbeta = dr.sum(0)
    dgamma = (dr * xhat).sum(0)
    k2 = -scale * dgamma / P * invstd
    k0 = -scale * dbeta / P - k2 * mean
    out.update(dr=dr, dres=dr, dbeta=dbeta, dgamma=dgamma, k0=k0, k2=k2,
               dx=scale * (dr - dbeta / P - xhat * dgamma / P))
    return out


def reference(x, gamma, beta, eps, residual=None, relu=True, dy=None, momentum=None, running_mean=None, running_var=None,
              training=True):
    """BatchNorm over rows x [P, C] in float64: training mode with batch statistics (+ the running buffers' update, unbiased
    variance), or eval mode with the running buffers.  -> dict of float64 tensors: z (pre-activation), y, mean, var (biased),
    invstd, scale, shift, and with dy: dr, dx, dres, dgamma, dbeta, k0, k2; with running buffers: running_mean, running_var."""
    if not training:
        return from_stats(x, running_mean.double(), running_var.double(), gamma, beta, eps, residual, relu, None)
    P = x.shape[0]
    if P < 2:
        raise ValueError("training-mode BatchNorm needs more than one value per channel")
    mean, var = batch_stats(x)
    out = from_stats(x, mean, var, gamma, beta, eps, residual, relu, dy)
    if running_mean is not None:
        m = float(momentum)
        out["running_mean"] = (1 - m) * running_mean.double() + m * mean
        out["running_var"] = (1 - m) * running_var.double() + m * var * (P / (P - 1))
    return out


# ---- input conditioning --------------------------------------------------------------------------------------------------------
def ulp(t, dtype):
    """Spacing of `dtype` numbers at |t| (float64 tensor): 2^(e - p) with p = 8 (bf16) or 24 (fp32) mantissa bits."""
    p = 8 if dtype == torch.bfloat16 else 24
    _, e = torch.frexp(t.double())
    return torch.pow(2.0, (e - p).to(torch.float64))


def condition(x, gamma, beta, eps, residual=None, margin=MARGIN, max_iter=10):
    """Move the elements of x (rows [P, C], kernel dtype) whose float64 pre-activation lies within `margin` of the ReLU
    threshold away from it: nudge, round to x's dtype, recompute the statistics, repeat.  -> (x', min |z|, number of elements
    moved).  The ReLU mask is not differentiable at 0, and the kernel (fmaf(x, scale, shift)) and any reference round z
    differently: an element within their disagreement of 0 can take either branch."""
    dt = x.dtype
    g = gamma.double()
    orig = x
    for _ in range(max_iter):
        mean, var = batch_stats(x)
        z = from_stats(x, mean, var, gamma, beta, eps, residual, relu=False)["z"]
        near = z.abs() < margin
        zmin = float(z.abs().min())
        if not bool(near.any()):
            break
        gain = (g / torch.sqrt(var + eps)).expand_as(z)             # dz / dx (the statistics' own change is second order)
        side = torch.where(z >= 0, torch.ones_like(z), -torch.ones_like(z))
        step = side * torch.sign(gain) * torch.maximum(2 * margin / gain.abs(), ulp(x, dt))
        x = torch.where(near, (x.double() + step).to(dt), x)
    else:
        mean, var = batch_stats(x)
        zmin = float(from_stats(x, mean, var, gamma, beta, eps, residual, relu=False)["z"].abs().min())
    return x, zmin, int((x != orig).sum())


# ---- per-element bounds --------------------------------------------------------------------------------------------------------
def stat_bounds(x, ref, n_stats, eps, pivot=True):
    """Bounds on the kernel's mean / var / invstd / scale / shift (k_bn_stats_partial + k_bn_stats_final).
    pivot: sums of d = x - x[0] (the stand-alone pass); else unshifted sums (a convolution epilogue, see partial_bounds)."""
    x = x.double()
    P = x.shape[0]
    d = x - x[0] if pivot else x
    s1, s2 = d.abs().sum(0), (d * d).sum(0)
    da = (n_stats + 1) * U32 * s1                        # fp32 chains of <= n_stats adds, + the per-slice rounding
    dq = (n_stats + 2) * U32 * s2                        # + one rounding of d * d per term
    return stats_from_sum_bounds(ref, d.sum(0) / P, da / P, dq / P, eps)


def stats_from_sum_bounds(ref, m, dm, dq_p, eps):
    """Propagate the bounds dm on sum/P and dq_p on sumsq/P through k_bn_stats_final's double arithmetic (v = q/P - m^2) and its
    fp32 outputs (one rounding each, U32 * |value|)."""
    dmean = dm + U32 * ref["mean"].abs()
    dvar = dq_p + (2 * m.abs() + dm) * dm
    dvar_out = dvar + U32 * ref["var"]
    inv = ref["invstd"]
    dinv = 0.5 * inv ** 3 * dvar + U32 * inv                              # d(v + eps)^-1/2 = -1/2 (v + eps)^-3/2 dv
    sc = ref["scale"]
    g = (sc / inv).abs()
    dsc = g * dinv + U32 * sc.abs()                                         # gamma * invstd, one rounding
    dsh = ref["mean"].abs() * dsc + sc.abs() * dmean + 2 * U32 * (ref["shift"].abs() + (ref["mean"] * sc).abs())
    return dict(mean=dmean, var=dvar_out, invstd=dinv, scale=dsc, shift=dsh, _dvar=dvar)


def eval_stat_bounds(ref, running_mean):
    """Eval mode: the op folds the running buffers in fp32 torch arithmetic (rsqrt(rv + eps), gamma * invstd, beta - rm * scale):
    4 ulp for the add + rsqrt, one rounding per product / difference."""
    inv, sc = ref["invstd"], ref["scale"]
    dinv = 4 * U32 * inv
    dsc = (sc / inv).abs() * dinv + U32 * sc.abs()
    dsh = running_mean.double().abs() * dsc + 2 * U32 * (ref["shift"].abs() + (running_mean.double() * sc).abs())
    return dict(invstd=dinv, scale=dsc, shift=dsh)


def bounds(x, ref, dtype, eps, residual=None, momentum=None, running_mean=None, running_var=None, sb=None):
    """Per-element (per-channel for the vectors) bounds |kernel - float64 reference| for the outputs of ud_bn_stats* +
    ud_bn_act_fwd* + ud_bn_act_bwd* on rows x [P, C] (already in the kernel's dtype).  sb: statistics bounds (stat_bounds by
    default, the stand-alone pass; partial_bounds-based for a convolution epilogue; eval_stat_bounds in eval mode)."""
    x = x.double()
    P, C = x.shape
    n_stats, n_bwd = chain_lengths(P, C)
    if sb is None:
        sb = stat_bounds(x, ref, n_stats, eps)
    sc, sh = ref["scale"], ref["shift"]
    r = residual.double().abs() if residual is not None else 0.0
    # z = fmaf(x, scale, shift) (+ r): the propagated statistics error + one rounding per fma / add of the terms' magnitudes
    dz = x.abs() * sb["scale"] + sb["shift"] + 2 * U32 * ((x * sc).abs() + sh.abs() + r)
    out = dict(z=dz, **{k: v for k, v in sb.items() if not k.startswith("_")})
    # y: relu is 1-Lipschitz; fp32 stores z as is; bf16 rounds it: + one ulp here, the exact rule is bf16_forward_mismatches
    out["y"] = dz + (ulp(ref["y"].abs() + dz, dtype) if dtype == torch.bfloat16 else 0.0)
    if running_mean is not None:
        m = float(momentum)
        # (1 - m) rm + m mu in fp32: the mean's error times m + one rounding per term and for the sum (momentum itself rounded)
        out["running_mean"] = m * sb["mean"] + 4 * U32 * ((1 - m) * running_mean.double().abs() + m * ref["mean"].abs())
        unb = ref["var"] * (P / max(P - 1, 1))
        out["running_var"] = m * sb["_dvar"] * (P / max(P - 1, 1)) + \
            4 * U32 * ((1 - m) * running_var.double().abs() + m * unb)
    if "dx" not in ref:
        return out
    dr = ref["dr"]
    xm = x - ref["mean"]
    # sums of dr and dr (x - mean) in fp32 chains of <= n_bwd adds; (x - mean) rounded and multiplied (2 roundings per term);
    # the kernel subtracts its own mean: + dmean * sum|dr|
    sa = dr.abs().sum(0)
    da = (n_bwd + 1) * U32 * sa
    dq = (n_bwd + 3) * U32 * (dr * xm).abs().sum(0) + sb["mean"] * sa
    inv, dinv, dsc = ref["invstd"], sb["invstd"], sb["scale"]
    q = (dr * xm).sum(0)
    ddg = q.abs() * dinv + inv * dq + U32 * ref["dgamma"].abs()
    dg = ref["dgamma"]
    k2, k0 = ref["k2"], ref["k0"]
    # k2 = -scale * (dg * (1/P)) * invstd and k0 = -scale * (a * (1/P)) - k2 * mean, one rounding per operation
    dk2 = (dg / P * inv).abs() * dsc + (sc * inv / P).abs() * ddg + (sc * dg / P).abs() * dinv + 4 * U32 * k2.abs()
    dk0 = (ref["dbeta"] / P).abs() * dsc + sc.abs() * da / P + ref["mean"].abs() * dk2 + k2.abs() * sb["mean"] + \
        4 * U32 * ((sc * ref["dbeta"] / P).abs() + (k2 * ref["mean"]).abs())
    # dx = fmaf(scale, dr, fmaf(k2, x, k0)): the propagated errors of scale, k2, k0 + two roundings of the terms' magnitudes
    ddx = dr.abs() * dsc + x.abs() * dk2 + dk0 + 2 * U32 * ((sc * dr).abs() + (k2 * x).abs() + k0.abs())
    if dtype == torch.bfloat16:
        ddx = ddx + ulp(ref["dx"].abs() + ddx, dtype)        # + one output ulp (round to nearest is half of it)
    out.update(dx=ddx, dbeta=da, dgamma=ddg, k0=dk0, k2=dk2, dres=torch.zeros_like(dr))   # dres = dy * mask: exact
    return out


def bf16_forward_mismatches(y, ref_y, dz):
    """bf16 mode: y must be the float64 result rounded to bf16, except where the float64 value lies within dz (the bound on the
    kernel's fp32 z) of a bf16 rounding boundary; there a neighbour is right too.  -> (mismatch mask, ambiguous mask, error
    mask: mismatches outside the ambiguous set, or further than dz + one ulp from the float64 value -- more than one ulp only
    where dz itself exceeds the bf16 spacing, i.e. |z| near 0 after cancellation)."""
    v = ref_y.double()
    b = v.to(torch.float32).to(torch.bfloat16).double()       # not ambiguous => every rounding path gives this value
    sp = ulp(b, torch.bfloat16)
    m, _ = torch.frexp(b)
    half_low = torch.where(m.abs() == 0.5, sp / 4, sp / 2)      # at a power of two the spacing below is half the one above
    ambiguous = (v - b).abs() >= half_low - dz
    got = y.double()
    mism = got != b
    bad = mism & (~ambiguous | ((got - v).abs() > dz + sp))
    return mism, ambiguous, bad


def violations(got, ref, bnd, names, index_info=None):
    """-> list of messages, one per output in `names` whose |got - ref| exceeds its bound anywhere; each lists the worst elements
    with (row, channel), the float64 pre-activation and both values, so that a failure classifies itself."""
    msgs = []
    for n in names:
        g, r, b = got[n].double(), ref[n].double(), bnd[n]
        b = b.expand_as(r) if torch.is_tensor(b) else torch.full_like(r, float(b))
        err = (g - r).abs()
        bad = ~(err <= b)                    # NaN counts as bad
        nbad = int(bad.sum())
        if nbad == 0:
            continue
        idx = bad.nonzero()[:8].tolist()
        lines = []
        for i in idx:
            t = tuple(i)
            z = f" z={float(ref['z'][t]):+.6e}" if (r.dim() == 2 and "z" in ref) else ""
            lines.append(f"  {t}:{z} got={float(g[t]):+.9e} ref={float(r[t]):+.9e} |err|={float(err[t]):.3e} "
                         f"bound={float(b[t]):.3e}")
        msgs.append(f"{n}: {nbad} of {r.numel()} elements outside the bound\n" + "\n".join(lines))
    return msgs


def partial_bounds(y, ref, eps, tile_rows=128):
    """Statistics from a convolution epilogue's per-tile (sum, sum of squares) of the stored output y (rows [P, C]): every
    producer reduces a tile of <= 128 output rows with fp32 adds in some order (+ one rounding of each square and of the
    tile's result); the tiles are added in double.  -> (bound on sum/P, bound on sumsq/P, statistics bounds)."""
    y = y.double()
    P = y.shape[0]
    n = tile_rows
    dm = (n + 1) * U32 * y.abs().sum(0) / P
    dq = (n + 2) * U32 * (y * y).sum(0) / P
    return dm, dq, stats_from_sum_bounds(ref, y.sum(0) / P, dm, dq, eps)


def var_error_ratio_bound(ratio, n=128):
    """Relative bound on the variance from unshifted partials at |mean| / std = ratio (E|y| <= |mean| + std):
    dv / var <= (n + 2) u (1 + ratio^2) + 2 ratio (n + 1) u (ratio + 1) + O(u^2)."""
    return (n + 2) * U32 * (1 + ratio ** 2) + 2 * ratio * (n + 1) * U32 * (ratio + 1)

