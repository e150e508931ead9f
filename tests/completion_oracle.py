"""Plain numpy specifications of the completion metrics (r2dm_amd/csrc/completion.hip), written from their definitions and sharing no
code with the library: the ten per-sample sums in float64, the confusion matrix as an ``np.bincount`` and the beam interpolation as a loop
over the pixels whose linear mode evaluates ``a + (b - a) * t`` in ``np.float32``."""
import numpy as np

RAW = ("unknown", "evaluated", "both", "false_returns", "abs_depth", "sq_depth", "abs_depth_both", "sq_depth_both", "abs_reflectance",
       "sq_reflectance")


def error_sums(pred, target, known, lo, hi):
    """pred, target (B,5,H,W) float32, known (B,1,H,W) -> (B,10) float64.  Every float32 value is widened first, so the differences are
    exact; the sums are numpy's pairwise float64 sums over the selected pixels (no products with masks: a NaN outside a set stays outside)."""
    pred, target, known = (np.asarray(a, dtype=np.float32) for a in (pred, target, known))
    lo, hi = np.float32(lo), np.float32(hi)
    out = np.zeros((pred.shape[0], 10), np.float64)
    for b in range(pred.shape[0]):
        r, rp = target[b, 0].ravel(), pred[b, 0].ravel()
        rho, rhop = target[b, 4].ravel().astype(np.float64), pred[b, 4].ravel().astype(np.float64)
        with np.errstate(invalid="ignore"):
            U = known[b, 0].ravel() == 0
            G = (lo < r) & (r < hi)
            P = (lo < rp) & (rp < hi)
        E, Bo = U & G, U & G & P
        rhat = np.where(P, rp, np.float32(0)).astype(np.float64)
        d = rhat - r.astype(np.float64)
        e = rhop - rho
        out[b] = [U.sum(), E.sum(), Bo.sum(), (U & P & ~G).sum(), np.abs(d[E]).sum(), (d[E] * d[E]).sum(), np.abs(d[Bo]).sum(),
                  (d[Bo] * d[Bo]).sum(), np.abs(e[E]).sum(), (e[E] * e[E]).sum()]
    return out


def derived(raw):
    """(...,10) -> dict of the derived values, NaN where the denominator is 0"""
    raw = np.asarray(raw, np.float64)

    def ratio(num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, num / den, np.nan)

    U, E, Bo, fr = (raw[..., k] for k in range(4))
    return {"mae_depth": ratio(raw[..., 4], E), "rmse_depth": np.sqrt(ratio(raw[..., 5], E)), "mae_depth_both": ratio(raw[..., 6], Bo),
            "rmse_depth_both": np.sqrt(ratio(raw[..., 7], Bo)), "mae_reflectance": ratio(raw[..., 8], E),
            "rmse_reflectance": np.sqrt(ratio(raw[..., 9], E)), "return_recall": ratio(Bo, E), "false_return_rate": ratio(fr, U - E)}


def confusion(pred, target, classes, mask=None):
    """int64 labels (B,P) -> (B,C,C) int64 counts [b][target][pred] over the pixels whose mask is not 0; every counted label must be in
    [0, classes)"""
    pred, target = np.asarray(pred, np.int64), np.asarray(target, np.int64)
    B = pred.shape[0]
    out = np.zeros((B, classes, classes), np.int64)
    for b in range(B):
        keep = np.ones(pred[b].shape, bool) if mask is None else np.asarray(mask[b]) != 0
        t, p = target[b][keep], pred[b][keep]
        assert ((t >= 0) & (t < classes) & (p >= 0) & (p < classes)).all()
        out[b] = np.bincount(t * classes + p, minlength=classes * classes).reshape(classes, classes)
    return out


def iou(conf, ignore=(0,)):
    """(C,C) counts [target][pred] -> (per-class IoU with NaN for absent and ignored classes, mIoU over the others)"""
    conf = np.array(conf, np.float64)
    for c in ignore:
        conf[c, :] = 0
    tp = np.diag(conf)
    union = conf.sum(0) + conf.sum(1) - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        per = np.where(union > 0, tp / union, np.nan)
    per[list(ignore)] = np.nan
    ok = ~np.isnan(per)
    return per, (per[ok].mean() if ok.any() else np.nan)


def fill(x, rows, mode, nodata=-1.0):
    """x (B,C,H,W) float32, rows (B,H) (non-zero = known) -> (B,C,H,W) float32, pixel by pixel"""
    x = np.asarray(x, np.float32)
    rows = np.asarray(rows) != 0
    nodata = np.float32(nodata)
    B, C, H, W = x.shape
    out = np.empty_like(x)
    for b in range(B):
        known = [h for h in range(H) if rows[b, h]]
        for h in range(H):
            if rows[b, h]:
                out[b, :, h] = x[b, :, h]
                continue
            above, below = [k for k in known if k < h], [k for k in known if k > h]
            up, dn = (max(above) if above else None), (min(below) if below else None)
            for w in range(W):
                ua = up is not None and x[b, 0, up, w] != nodata
                ub = dn is not None and x[b, 0, dn, w] != nodata
                if not ua and not ub:
                    out[b, :, h, w] = nodata
                elif ua and ub and mode == "linear":
                    t = np.float32(h - up) / np.float32(dn - up)
                    for c in range(C):
                        a, e = x[b, c, up, w], x[b, c, dn, w]
                        out[b, c, h, w] = np.float32(a + np.float32(np.float32(e - a) * t))
                elif ua and ub:
                    out[b, :, h, w] = x[b, :, up if h - up <= dn - h else dn, w]
                else:
                    out[b, :, h, w] = x[b, :, up if ua else dn, w]
    return out
