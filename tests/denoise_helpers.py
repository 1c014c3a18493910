"""The denoiser's arithmetic of include/ptgpu.h (pt_denoise_device and the
prepare step of pt_film_denoise_device) restated in numpy float32, one
elementwise operation per line over whole shifted frames: numpy rounds each
operation to float32 and never fuses two, and its `/` and np.sqrt are
correctly rounded, so the device filter must agree with this bit for bit.  A
skipped tap leaves the sums untouched through np.where; nothing is ever
multiplied by 0 to drop it.

Layouts: cv (H, W, 4) float32 = {r, g, b, v}; feat (2, H, W, 4) float32 =
{N, bsdf as int32 bits}, {P, z}; row 0 is the bottom row, as the frame."""
import numpy as np

F = np.float32
INF = F(np.inf)
K = (F(0.375), F(0.25), F(0.0625))  # the 5-tap B3 spline
G = (F(0.5), F(0.25))               # the 3x3 variance prefilter, per axis
DEFAULTS = {"iterations": 5, "normal_squarings": 7, "sigma_l": 4.0}


def shifted(a: np.ndarray, ox: int, oy: int, fill) -> np.ndarray:
    """out[y, x] = a[y + oy, x + ox], `fill` where that lies outside the frame."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def lum(c: np.ndarray) -> np.ndarray:
    a = F(0.2126) * c[..., 0]
    b = F(0.7152) * c[..., 1]
    d = F(0.0722) * c[..., 2]
    s = a + b
    return s + d


def dot3(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    x = a[..., 0] * b[..., 0]
    y = a[..., 1] * b[..., 1]
    z = a[..., 2] * b[..., 2]
    s = x + y
    return s + z


def iteration(cv, feat, step, normal_squarings, sigma_l, sigma_p):
    """One a-trous iteration with tap distance `step`."""
    assert cv.dtype == F and feat.dtype == F
    sigma_l, sigma_p = F(sigma_l), F(sigma_p)
    h, w = cv.shape[:2]
    c, v = cv[..., :3], cv[..., 3]
    n_p, p_p, z_p = feat[0][..., :3], feat[1][..., :3], feat[1][..., 3]
    bsdf = np.ascontiguousarray(feat[0]).view(np.int32)[..., 3]
    valid = v >= 0
    known = valid & (v < INF)
    hit = bsdf >= 0
    one = np.ones((h, w), F)
    with np.errstate(all="ignore"):
        # ---- variance prefilter
        sv = np.zeros((h, w), F)
        sg = np.zeros((h, w), F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g = G[abs(dx)] * G[abs(dy)]
                vq = shifted(v, dx, dy, F(-1))  # (outside the frame: as an invalid pixel)
                use = (vq >= 0) & (vq < INF)
                t = g * vq
                sv = np.where(use, sv + t, sv)
                sg = np.where(use, sg + g, sg)
        vf = sv / sg
        sd = np.sqrt(vf)
        den = sigma_l * sd
        den = den + F(1e-6)
        l_p = lum(c)
        pden = sigma_p * z_p
        # ---- taps
        sum_c = np.zeros((h, w, 3), F)
        sum_w = np.zeros((h, w), F)
        sum_v = np.zeros((h, w), F)
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                hk = K[abs(dx)] * K[abs(dy)]
                cvq = shifted(cv, dx * step, dy * step, F(-1))
                f0 = shifted(feat[0], dx * step, dy * step, F(0))
                f1 = shifted(feat[1], dx * step, dy * step, F(0))
                c_q, v_q = cvq[..., :3], cvq[..., 3]
                bsdf_q = np.ascontiguousarray(f0).view(np.int32)[..., 3]
                use = (v_q >= 0) & np.isfinite(c_q).all(-1) & (bsdf_q == bsdf)
                if dx == 0 and dy == 0:
                    wgt = np.full((h, w), hk, F)
                else:
                    cc = np.fmax(F(0), dot3(n_p, f0[..., :3]))
                    for _ in range(normal_squarings):
                        cc = cc * cc
                    d = f1[..., :3] - p_p
                    x_p = np.abs(dot3(n_p, d))
                    x_p = x_p / pden
                    w_p = F(1) - x_p
                    w_p = np.fmax(F(0), w_p)
                    w_n = np.where(hit, cc, one)
                    w_p = np.where(hit, w_p, one)
                    x_l = lum(c_q) - l_p
                    x_l = np.abs(x_l)
                    x_l = x_l / den
                    w_l = x_l * x_l
                    w_l = F(1) + w_l
                    w_l = F(1) / w_l
                    w_l = np.where(known, w_l, one)
                    wgt = hk * w_n
                    wgt = wgt * w_p
                    wgt = wgt * w_l
                vq = np.where(v_q == INF, v, v_q)
                t = wgt[..., None] * c_q
                sum_c = np.where(use[..., None], sum_c + t, sum_c)
                sum_w = np.where(use, sum_w + wgt, sum_w)
                t = wgt * wgt
                t = t * vq
                sum_v = np.where(use, sum_v + t, sum_v)
        out = np.empty_like(cv)
        out[..., :3] = sum_c / sum_w[..., None]
        t = sum_w * sum_w
        t = sum_v / t
        out[..., 3] = np.where(known, t, INF)
    through = valid & ~np.isfinite(c).all(-1)  # a non-finite centre is copied through
    out[through] = cv[through]
    out[~valid] = (F(0), F(0), F(0), F(-1))
    return out


def denoise(cv, feat, iterations, normal_squarings, sigma_l, sigma_p):
    for i in range(iterations):
        cv = iteration(cv, feat, 1 << i, normal_squarings, sigma_l, sigma_p)
    return cv


def prepare(r) -> np.ndarray:
    """The working records of a FilmRestatement (tests/film_helpers.py)."""
    h, w = r.n.shape
    cv = np.zeros((h, w, 4), F)
    cv[..., 3] = F(-1)
    m = r.n > 0
    n = r.n[m].astype(F)
    cv[m, :3] = r.sum[m] / n[:, None]
    k = r.k[m]
    q = np.fmax(r.M2[m], F(0))
    q = q / n
    with np.errstate(all="ignore"):
        q = q / (k - np.uint32(1)).astype(F)
    cv[m, 3] = np.where(k >= 2, q, INF)
    return cv


def feature_records(w, h, normal, bsdf, position, depth) -> np.ndarray:
    """A (2, h, w, 4) feature buffer from its parts."""
    feat = np.zeros((2, h, w, 4), F)
    feat[0, ..., :3] = normal
    feat[0].view(np.int32)[..., 3] = bsdf
    feat[1, ..., :3] = position
    feat[1, ..., 3] = depth
    return feat


def miss_records(w, h) -> np.ndarray:
    return feature_records(w, h, 0, -1, 0, 0)


def synthetic_case(w: int, h: int, seed: int):
    """A frame that takes every branch of the filter: three "surfaces" with
    random unit normals scattered around three axes, a miss region, two bsdf
    ids on one plane; random colours with a few inf / NaN; variances finite,
    +inf, -1 and NaN."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    region = np.where(x < w * 0.3, 0, np.where(x < w * 0.6, 1, np.where(y < h * 0.7, 2, 3)))  # 3: miss
    axes = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 0]], np.float64)
    n = axes[region] + rng.normal(0, 0.15, (h, w, 3))
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-9)
    depth = (2.0 + 0.05 * x + 0.03 * y + rng.normal(0, 0.01, (h, w))).astype(F)
    pos = np.stack([0.1 * x, 0.1 * y, -depth.astype(np.float64)], -1) + rng.normal(0, 0.002, (h, w, 3))
    bsdf = np.where(region == 0, np.where(y < h // 2, 1, 4), np.where(region == 1, 2, 3)).astype(np.int32)
    miss = region == 3
    n[miss] = 0
    pos[miss] = 0
    depth[miss] = 0
    bsdf[miss] = -1
    feat = feature_records(w, h, n.astype(F), bsdf, pos.astype(F), depth)
    cv = np.empty((h, w, 4), F)
    cv[..., :3] = rng.random((h, w, 3), F) * F(2)
    var = (rng.random((h, w), F) * F(0.05)).astype(F)
    kind = rng.random((h, w))
    var[kind < 0.25] = INF
    var[(kind >= 0.25) & (kind < 0.32)] = F(-1)
    var[(kind >= 0.32) & (kind < 0.36)] = F(np.nan)
    cv[..., 3] = var
    bad = rng.random((h, w))
    cv[bad < 0.02, 0] = INF
    cv[(bad >= 0.02) & (bad < 0.04), 1] = F(np.nan)
    cv[(bad >= 0.04) & (bad < 0.05), 2] = -INF
    return cv, feat
