"""Float64 restatement of the depth metric (csrc/depth_metric.hip), written from its definition; numpy only.

Per pixel with a finite dmin whose bin b = floor((dmin - d_lo) / d_step) lies in [0, D):  p = softmax over the D logits,
dhat = sum_j p_j (d_lo + (j + 0.5) d_step), ahat = the first arg-max bin, d = dmin, e = dhat - d, and the twelve terms
  count, |e|, |e| / d, e^2 / d, e^2, (ln dhat - ln d)^2, [q < 1.25], [q < 1.25^2], [q < 1.25^3] with q = max(dhat / d, d / dhat),
  [ahat == b], [|ahat - b| <= 1], -ln max(p_b, 1e-44)
summed into state[n mod groups, r] for the first r with edges[r] <= d < edges[r + 1] (none: counted nowhere).
``torch_fp32_state`` is the same expression with plain PyTorch float32 ops: the yardstick the GPU test measures against."""
import numpy as np

T = 12
INTEGER_TERMS = (0, 6, 7, 8, 9, 10)
FLOAT_TERMS = (1, 2, 3, 4, 5, 11)


def pixel_terms(logits, dmin, d_lo, d_step):
    """logits [BN, D, fH, fW], dmin [BN, fH, fW] -> dict of per-pixel float64 arrays [BN, fH, fW]: labelled (bool), b, terms
    [BN, fH, fW, 12] (zero where unlabelled), and for the knife-edge checks q, gap (top-two logit gap) and d."""
    x = np.asarray(logits, dtype=np.float64)
    d32 = np.asarray(dmin, dtype=np.float32)
    BN, D = x.shape[:2]
    d = d32.astype(np.float64).reshape(BN, *x.shape[2:])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        k = np.floor((d - d_lo) / d_step)
        labelled = np.isfinite(d) & (k >= 0) & (k < D)
        b = np.where(labelled, k, 0).astype(np.int64)
        ds = np.where(labelled, d, 1.0)
        z = x - x.max(1, keepdims=True)
        ez = np.exp(z)
        p = ez / ez.sum(1, keepdims=True)
        centre = (d_lo + (np.arange(D) + 0.5) * d_step).reshape(1, D, 1, 1)
        dhat = (p * centre).sum(1)
        ahat = x.argmax(1)                                   # numpy: the first of equal maxima
        pb = np.take_along_axis(p, b[:, None], 1)[:, 0]
        e = dhat - ds
        q = np.maximum(dhat / ds, ds / dhat)
        lg = np.log(dhat) - np.log(ds)
        top2 = np.sort(x, 1)[:, -2:] if D > 1 else np.stack([x[:, 0] - np.inf, x[:, 0]], 1)
        terms = np.stack([np.ones_like(e), np.abs(e), np.abs(e) / ds, e * e / ds, e * e, lg * lg, q < 1.25, q < 1.25 ** 2,
                          q < 1.25 ** 3, ahat == b, np.abs(ahat - b) <= 1, -np.log(np.maximum(pb, 1e-44))], -1).astype(np.float64)
    terms[~labelled] = 0.0
    return {"labelled": labelled, "b": b, "terms": terms, "q": q, "gap": top2[:, 1] - top2[:, 0], "d": d, "dhat": dhat,
            "ahat": ahat}


def bucket_of(d, labelled, edges):
    r = np.full(d.shape, -1, np.int64)
    for i in range(len(edges) - 2, -1, -1):                  # descending, so that the FIRST matching bucket stays
        with np.errstate(invalid="ignore"):
            r[labelled & (d >= edges[i]) & (d < edges[i + 1])] = i
    return r


def depth_metric_state(logits, dmin, d_lo, d_step, edges, groups=1, pix=None):
    """-> state float64 [groups, len(edges) - 1, 12]."""
    pix = pixel_terms(logits, dmin, d_lo, d_step) if pix is None else pix
    r = bucket_of(pix["d"], pix["labelled"], edges)
    BN = r.shape[0]
    state = np.zeros((groups, len(edges) - 1, T))
    for n in range(BN):
        for i in range(len(edges) - 1):
            state[n % groups, i] += pix["terms"][n][r[n] == i].sum(0)
    return state


def knife_edges(pix, edges):
    """Number of labelled pixels on which a decision of the metric could flip with fp32 rounding: a delta threshold, the
    arg-max, a range edge."""
    bad = pix["gap"] <= 1e-3
    for k in (1, 2, 3):
        bad |= np.abs(pix["q"] - 1.25 ** k) <= 1e-4
    for e in edges:
        if np.isfinite(e):
            with np.errstate(invalid="ignore"):
                bad |= np.abs(pix["d"] - e) <= 1e-4
    return int((bad & pix["labelled"]).sum())


def torch_fp32_state(logits, dmin, d_lo, d_step, edges, groups=1):
    """The same expression with plain PyTorch float32 ops on the tensors' own device (softmax, expectation, masks, sums);
    -> float64 numpy state [groups, len(edges) - 1, 12] of the float32 results."""
    import torch
    x = logits.float()
    BN, D = x.shape[:2]
    d = dmin.reshape(BN, *x.shape[2:]).float()
    k = torch.floor((d.double() - d_lo) / d_step)
    labelled = torch.isfinite(d) & (k >= 0) & (k < D)
    b = torch.where(labelled, k, torch.zeros_like(k)).long()
    ds = torch.where(labelled, d, torch.ones_like(d))
    p = torch.softmax(x, 1)
    centre = (d_lo + (torch.arange(D, device=x.device, dtype=torch.float64) + 0.5) * d_step).float().view(1, D, 1, 1)
    dhat = (p * centre).sum(1)
    ahat = x.argmax(1)
    pb = p.gather(1, b[:, None])[:, 0]
    e = dhat - ds
    q = torch.maximum(dhat / ds, ds / dhat)
    lg = torch.log(dhat) - torch.log(ds)
    one = torch.ones_like(e)
    f = lambda m: m.float()
    terms = torch.stack([one, e.abs(), e.abs() / ds, e * e / ds, e * e, lg * lg, f(q < 1.25), f(q < 1.25 ** 2), f(q < 1.25 ** 3),
                         f(ahat == b), f((ahat - b).abs() <= 1), -torch.log(pb.clamp(min=1e-44))], -1)
    state = torch.zeros((groups, len(edges) - 1, T), dtype=torch.float32, device=x.device)
    for i in range(len(edges) - 1):
        inside = labelled & (d.double() >= edges[i]) & (d.double() < edges[i + 1])
        for j in range(i):
            inside &= ~((d.double() >= edges[j]) & (d.double() < edges[j + 1]))
        for g in range(groups):
            sel = inside[g::groups]
            state[g, i] = torch.where(sel[..., None], terms[g::groups], torch.zeros_like(terms[g::groups])).sum((0, 1, 2))
    return state.double().cpu().numpy()
