"""numpy witness of eincm_preprocess_image: the four stages of the reference's preprocess_image
(NL-means, CLAHE, unsharp mask, bilateral filter), each restated from the written contract.

Borders are explicit reflect101 index maps, the integer stages run in int64, and the float stages are float32 one operation
at a time (numpy never fuses a multiply-add).  Host tables use Python's math.exp, the same libm as the library's host code."""
import math

import numpy as np

NLMEANS, CLAHE, UNSHARP, BILATERAL = 1, 2, 4, 8
ALL = NLMEANS | CLAHE | UNSHARP | BILATERAL

F = np.float32


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), iterated so that borders wider than the image fold back again."""
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def index_map(lo, hi, n):
    """reflect101 of lo .. hi-1 as an int64 array."""
    return np.array([reflect101(p, n) for p in range(lo, hi)], dtype=np.int64)


def pad101(img, top, bottom, left, right):
    """copyMakeBorder(BORDER_REFLECT_101) by index maps."""
    H, W = img.shape
    return img[np.ix_(index_map(-top, H + bottom, H), index_map(-left, W + right, W))]


def rne_u8(x):
    """cvRound (half to even) then saturate to [0, 255]."""
    return np.clip(np.rint(np.asarray(x, dtype=np.float64)), 0, 255).astype(np.uint8)


# --------------------------------------------------------------------------------------------------- a. NL-means
def nlm_shift(tw):
    s = 0
    while (1 << s) < tw * tw:
        s += 1
    return s


def nlm_table(h, tw, sw):
    """The weight table indexed by D >> shift, and (shift, fixed-point multiplier)."""
    s = nlm_shift(tw)
    fpm = (2 ** 31 - 1) // (sw * sw * 255)
    mult = float(1 << s) / (tw * tw)
    size = int(65025 / mult + 1)
    hh = float(F(h) * F(h))
    tab = np.zeros(size, dtype=np.int64)
    for a in range(size):
        w = round(fpm * math.exp(-(a * mult) / hh))       # round(): half to even, as cvRound of a double
        tab[a] = 0 if w < 0.001 * fpm else w
    return tab, s, fpm


def nlmeans(img, h=4.0, tw=3, sw=11):
    img = np.asarray(img)
    H, W = img.shape
    tr, sr = tw // 2, sw // 2
    b = tr + sr
    tab, s, _ = nlm_table(h, tw, sw)
    P = pad101(img.astype(np.int64), b, b, b, b)
    c0 = P[b - tr:b + H + tr, b - tr:b + W + tr]                   # template neighbourhood of every pixel
    est = np.zeros((H, W), np.int64)
    wsum = np.zeros((H, W), np.int64)
    for dy in range(-sr, sr + 1):
        for dx in range(-sr, sr + 1):
            c1 = P[b - tr + dy:b + H + tr + dy, b - tr + dx:b + W + tr + dx]
            sq = (c0 - c1) ** 2
            rows = sum(sq[:, k:k + W] for k in range(tw))          # tw-wide sums along x, then along y
            D = sum(rows[k:k + H, :] for k in range(tw))
            w = tab[D >> s]
            est += w * P[b + dy:b + H + dy, b + dx:b + W + dx]
            wsum += w
    assert est.max() < 2 ** 32 and wsum.max() < 2 ** 32
    return ((est + wsum // 2) // wsum).astype(np.uint8)


# --------------------------------------------------------------------------------------------------- b. CLAHE
def clahe_geometry(H, W, tiles_x, tiles_y):
    """(padded H, padded W, tile_h, tile_w): no padding only when both sides divide; otherwise the bottom gets
    tiles_y - H % tiles_y rows and the right tiles_x - W % tiles_x columns, even a side that divides (a full tile count)."""
    if W % tiles_x == 0 and H % tiles_y == 0:
        Hp, Wp = H, W
    else:
        Hp, Wp = H + tiles_y - H % tiles_y, W + tiles_x - W % tiles_x
    return Hp, Wp, Hp // tiles_y, Wp // tiles_x


def clip_histogram(hist, limit):
    """Clip every bin to limit, add clipped // 256 to every bin, then 1 to bins 0, step, 2 step, ... while the residual lasts."""
    hist = np.array(hist, dtype=np.int64)
    clipped = int(np.maximum(hist - limit, 0).sum())
    hist = np.minimum(hist, limit)
    batch = clipped // 256
    res = clipped - batch * 256
    hist += batch
    if res > 0:
        step = max(256 // res, 1)
        i = 0
        while i < 256 and res > 0:
            hist[i] += 1
            i += step
            res -= 1
    return hist


def clahe_luts(img, clip=5.0, tiles_x=10, tiles_y=10):
    """(tiles_y, tiles_x, 256) uint8 LUTs and (tile_h, tile_w)."""
    H, W = img.shape
    Hp, Wp, th, tw = clahe_geometry(H, W, tiles_x, tiles_y)
    P = pad101(np.asarray(img), 0, Hp - H, 0, Wp - W)
    total = th * tw
    scale = F(255.0) / F(total)
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            hist = np.bincount(P[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip > 0:
                hist = clip_histogram(hist, max(int(clip * total / 256), 1))
            cum = np.cumsum(hist)
            luts[ty, tx] = rne_u8(cum.astype(F) * scale)
    return luts, (th, tw)


def _interp_axis(n, tile, tiles):
    """Per coordinate: (lower tile, upper tile, fraction) in float32."""
    inv = F(1.0) / F(tile)
    f = np.arange(n).astype(F) * inv - F(0.5)
    t1 = np.floor(f).astype(np.int64)
    a = (f - t1.astype(F)).astype(F)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a


def clahe(img, clip=5.0, tiles_x=10, tiles_y=10):
    img = np.asarray(img)
    H, W = img.shape
    luts, (th, tw) = clahe_luts(img, clip, tiles_x, tiles_y)
    x1, x2, xa = _interp_axis(W, tw, tiles_x)
    y1, y2, ya = _interp_axis(H, th, tiles_y)
    v = img.astype(np.int64)
    yy1, yy2, xx1, xx2 = y1[:, None], y2[:, None], x1[None, :], x2[None, :]
    L11 = luts[yy1, xx1, v].astype(F)
    L12 = luts[yy1, xx2, v].astype(F)
    L21 = luts[yy2, xx1, v].astype(F)
    L22 = luts[yy2, xx2, v].astype(F)
    xa, ya = xa[None, :], ya[:, None]
    xa1, ya1 = F(1.0) - xa, F(1.0) - ya
    top = L11 * xa1 + L12 * xa
    bot = L21 * xa1 + L22 * xa
    return rne_u8(top * ya1 + bot * ya)


# --------------------------------------------------------------------------------------------------- c. unsharp mask
def unsharp_taps(sigma):
    """The 8-bit fixed-point Gaussian of cv.GaussianBlur(img, None, ksize=0 -> derived, sigma): ksize =
    cvRound(sigma * 6 + 1) | 1; fp64 normalised Gaussian; outer taps rounded with error diffusion from the outside in, the
    centre tap 256 minus the rest."""
    n = int(round(sigma * 3 * 2 + 1)) | 1
    half = n // 2
    scale2 = -0.125 / (sigma * sigma)
    vals = [math.exp(float(x * x) * scale2) for x in range(1 - n, 0, 2)]        # x = 2 (i - half), i < half
    total = 2.0 * sum(vals) + 1.0
    mul = 1.0 / total
    g = [v * mul for v in vals]
    k = [0] * n
    err, acc = 0.0, 0
    for i in range(half):
        adj = g[i] * 256.0 + err
        v0 = round(adj)
        err = adj - v0
        k[i] = k[n - 1 - i] = v0
        acc += v0
    k[half] = 256 - 2 * acc
    return np.array(k, dtype=np.int64)


def gaussian_blur_u8(img, sigma):
    img = np.asarray(img)
    H, W = img.shape
    k = unsharp_taps(sigma)
    r = len(k) // 2
    P = img.astype(np.int64)
    xs = index_map(-r, W + r, W)
    rows = sum(k[i] * P[:, xs[i:i + W]] for i in range(len(k)))              # exact, in 1 / 256
    ys = index_map(-r, H + r, H)
    tot = sum(k[j] * rows[ys[j:j + H], :] for j in range(len(k)))           # exact, in 1 / 65536
    return ((tot + (1 << 15)) >> 16).astype(np.uint8)


def add_weighted(a, alpha, b, beta):
    """cv.addWeighted(a, alpha, b, beta, 0) for 8-bit images: float32 a*alpha + b*beta + 0, rounded half to even."""
    t = np.asarray(a).astype(F) * F(alpha)
    u = np.asarray(b).astype(F) * F(beta)
    return rne_u8((t + u) + F(0.0))


def unsharp(img, sigma=3.0, alpha=1.5, beta=-0.5):
    return add_weighted(img, alpha, gaussian_blur_u8(img, sigma), beta)


# --------------------------------------------------------------------------------------------------- d. bilateral
def bilateral_setup(d, sc, ss):
    """(radius, colour weights (256,) float32, [(dy, dx, float32 weight)] in row-major order)."""
    sc = 1.0 if sc <= 0 else float(sc)
    ss = 1.0 if ss <= 0 else float(ss)
    r = d // 2 if d > 0 else int(round(ss * 1.5))
    r = max(r, 1)
    cc, sc2 = -0.5 / (sc * sc), -0.5 / (ss * ss)
    cw = np.array([F(math.exp(i * i * cc)) for i in range(256)], dtype=F)
    taps = []
    for i in range(-r, r + 1):
        for j in range(-r, r + 1):
            rr = math.sqrt(float(i * i) + float(j * j))
            if rr > r:
                continue
            taps.append((i, j, F(math.exp(rr * rr * sc2))))
    return r, cw, taps


def bilateral(img, d=5, sc=15.0, ss=15.0):
    img = np.asarray(img)
    H, W = img.shape
    r, cw, taps = bilateral_setup(d, sc, ss)
    P = pad101(img.astype(np.int64), r, r, r, r)
    v0 = img.astype(np.int64)
    s = np.zeros((H, W), F)
    ws = np.zeros((H, W), F)
    for dy, dx, sw in taps:
        v = P[r + dy:r + dy + H, r + dx:r + dx + W]
        w = sw * cw[np.abs(v - v0)]
        ws = ws + w
        s = s + v.astype(F) * w
    return rne_u8(s / ws)


# --------------------------------------------------------------------------------------------------- the chain
DEFAULTS = dict(h=4.0, tw=3, sw=11, clip=5.0, tiles=(10, 10), sigma=3.0, alpha=1.5, beta=-0.5, d=5, sc=15.0, ss=15.0)


def preprocess(img, stages=ALL, **kw):
    """The stages in the reference's order, each on the previous stage's uint8 output.  Keywords: DEFAULTS."""
    p = dict(DEFAULTS, **kw)
    out = np.asarray(img)
    assert out.dtype == np.uint8 and out.ndim == 2
    if stages & NLMEANS:
        out = nlmeans(out, p['h'], p['tw'], p['sw'])
    if stages & CLAHE:
        out = clahe(out, p['clip'], p['tiles'][0], p['tiles'][1])
    if stages & UNSHARP:
        out = unsharp(out, p['sigma'], p['alpha'], p['beta'])
    if stages & BILATERAL:
        out = bilateral(out, p['d'], p['sc'], p['ss'])
    return out


def preprocess_stack(imgs, stages=ALL, **kw):
    return np.stack([preprocess(im, stages, **kw) for im in imgs])
