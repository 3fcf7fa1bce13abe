"""A float32 numpy restatement of the keypoint detector of csrc/features.hip (SIFT's detection stage with cv2.SIFT_create()'s
defaults) and of the estimator's dilated interest mask.

This is the written specification the HIP kernels are tested against, bit for bit (every pyramid layer, every accept / reject
decision): the same tap order, the same float32 roundings, the same cofactor solve.  It is never called on the product path
(nav/features.py runs the kernels).  There is no OpenCV here, so neither form is compared with OpenCV's own keypoints (DESIGN.md,
"The state estimator")."""
import math

import numpy as np

N_LAYERS = 3            # nOctaveLayers
CONTRAST = 0.04         # contrastThreshold
EDGE = 10.0             # edgeThreshold
SIGMA = 1.6
BORDER = 5              # SIFT_IMG_BORDER
MAX_INTERP = 5          # SIFT_MAX_INTERP_STEPS
F = np.float32


def gray(img_rgb):
    """uint8 [H,W,3] -> uint8 [H,W]: cv2.COLOR_BGR2GRAY's fixed-point weights on channels 0, 1, 2 = R, G, B (OpenCV's SIFT takes
    the reference's RGB array for BGR, so the weights land swapped)"""
    c = img_rgb.astype(np.int32)
    return ((1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def _upsample_axis(a, axis):
    """x2 bilinear along `axis`, half-pixel centres, replicated border: out = w_lo * a[lo] + w_hi * a[lo + 1]"""
    n = a.shape[axis]
    X = np.arange(2 * n)
    lo = np.where(X & 1, X >> 1, (X >> 1) - 1)
    w_lo = np.where(X & 1, F(0.75), F(0.25)).astype(F)
    w_hi = np.where(X & 1, F(0.25), F(0.75)).astype(F)
    i0, i1 = np.clip(lo, 0, n - 1), np.clip(lo + 1, 0, n - 1)
    shape = [1] * a.ndim
    shape[axis] = -1
    return w_lo.reshape(shape) * np.take(a, i0, axis=axis) + w_hi.reshape(shape) * np.take(a, i1, axis=axis)


def base_image(img_rgb):
    """gray -> float32, x2 upsample (columns, then rows) -- before the initial blur"""
    g = gray(img_rgb).astype(F)
    return _upsample_axis(_upsample_axis(g, 1), 0)


def gaussian_taps(sigma):
    """getGaussianKernel(round(8 sigma + 1) | 1, sigma): float64 weights, normalised, cast to float32"""
    n = int(round(sigma * 8 + 1)) | 1
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    w = np.exp((-0.5 / (sigma * sigma)) * x * x)
    return (w * (1.0 / w.sum())).astype(F)


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101) on an int array"""
    p = np.asarray(p).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def blur(img, taps):
    """separable: rows (along x) then columns, each sum over the taps in order from 0.0"""
    r = len(taps) // 2
    rows, cols = img.shape
    tmp = np.zeros_like(img)
    xs = np.arange(cols)
    for k, w in enumerate(taps):
        tmp = tmp + w * img[:, reflect101(xs + k - r, cols)]
    out = np.zeros_like(img)
    ys = np.arange(rows)
    for k, w in enumerate(taps):
        out = out + w * tmp[reflect101(ys + k - r, rows), :]
    return out


def layer_sigmas():
    """the initial blur's sigma, then buildGaussianPyramid's increments"""
    sig = [math.sqrt(max(SIGMA * SIGMA - 1.0, 0.01))]
    k = 2.0 ** (1.0 / N_LAYERS)
    for i in range(1, N_LAYERS + 3):
        prev = k ** (i - 1) * SIGMA
        total = prev * k
        sig.append(math.sqrt(total * total - prev * prev))
    return sig


def n_octaves(H, W):
    return int(round(math.log(min(2 * H, 2 * W)) / math.log(2.0) - 2)) + 1


def pyramid(img_rgb):
    """-> list over octaves of (gauss [6, rows, cols], dog [5, rows, cols]) float32"""
    H, W = img_rgb.shape[:2]
    sig = layer_sigmas()
    taps = [gaussian_taps(s) for s in sig]
    out, prev3 = [], None
    for o in range(n_octaves(H, W)):
        g = [blur(base_image(img_rgb), taps[0]) if o == 0 else np.ascontiguousarray(prev3[::2, ::2][:prev3.shape[0] // 2, :prev3.shape[1] // 2])]
        for i in range(1, N_LAYERS + 3):
            g.append(blur(g[-1], taps[i]))
        g = np.stack(g)
        out.append((g, g[1:] - g[:-1]))
        prev3 = g[N_LAYERS]
    return out


def _candidates(dog):
    """(layer, r, c) of the 26-neighbourhood extrema of DoG layers 1..3 with |D| > 1, inside the border"""
    L, rows, cols = dog.shape
    if rows - 2 * BORDER <= 0 or cols - 2 * BORDER <= 0:
        return np.zeros((0, 3), np.int64)
    found = []
    for layer in range(1, N_LAYERS + 1):
        v = dog[layer, BORDER:rows - BORDER, BORDER:cols - BORDER]
        is_max, is_min = v > 0, v < 0
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl == 0 and dy == 0 and dx == 0:
                        continue
                    n = dog[layer + dl, BORDER + dy:rows - BORDER + dy, BORDER + dx:cols - BORDER + dx]
                    is_max &= v >= n
                    is_min &= v <= n
        rr, cc = np.nonzero((np.abs(v) > F(1)) & (is_max | is_min))
        found.append(np.stack([np.full_like(rr, layer), rr + BORDER, cc + BORDER], 1))
    return np.concatenate(found)


def _derivs(dog, layer, r, c):
    img_scale = F(1) / F(255)
    d1, d2, dc = img_scale * F(0.5), img_scale, img_scale * F(0.25)
    I = lambda dl, dy, dx: dog[layer + dl, r + dy, c + dx]   # noqa: E731
    dx = (I(0, 0, 1) - I(0, 0, -1)) * d1
    dy = (I(0, 1, 0) - I(0, -1, 0)) * d1
    ds = (I(1, 0, 0) - I(-1, 0, 0)) * d1
    v2 = I(0, 0, 0) * F(2)
    dxx = (I(0, 0, 1) + I(0, 0, -1) - v2) * d2
    dyy = (I(0, 1, 0) + I(0, -1, 0) - v2) * d2
    dss = (I(1, 0, 0) + I(-1, 0, 0) - v2) * d2
    dxy = (I(0, 1, 1) - I(0, 1, -1) - I(0, -1, 1) + I(0, -1, -1)) * dc
    dxs = (I(1, 0, 1) - I(1, 0, -1) - I(-1, 0, 1) + I(-1, 0, -1)) * dc
    dys = (I(1, 1, 0) - I(1, -1, 0) - I(-1, 1, 0) + I(-1, -1, 0)) * dc
    return dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys


def refine(dog, cand, octave):
    """adjustLocalExtrema for every candidate at once -> float32 keypoint positions [n, 2] (x, y) in input-image pixels"""
    L, rows, cols = dog.shape
    layer, r, c = [cand[:, i].copy() for i in range(3)]
    alive = np.ones(len(cand), bool)
    done = np.zeros(len(cand), bool)
    z = np.zeros(len(cand), F)
    xc, xr, xi, gx, gy, gs = z.copy(), z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    lim = F(2147483647 // 3)
    with np.errstate(all="ignore"):
        for _ in range(MAX_INTERP):
            a = alive & ~done
            if not a.any():
                break
            idx = np.nonzero(a)[0]
            dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys = _derivs(dog, layer[idx], r[idx], c[idx])
            c00, c01, c02 = dyy * dss - dys * dys, dys * dxs - dxy * dss, dxy * dys - dyy * dxs
            c11, c12, c22 = dxx * dss - dxs * dxs, dxy * dxs - dxx * dys, dxx * dyy - dxy * dxy
            det = dxx * c00 + dxy * c01 + dxs * c02
            sing = det == 0
            Xc = -((c00 * dx + c01 * dy + c02 * ds) / det)
            Xr = -((c01 * dx + c11 * dy + c12 * ds) / det)
            Xi = -((c02 * dx + c12 * dy + c22 * ds) / det)
            xc[idx], xr[idx], xi[idx], gx[idx], gy[idx], gs[idx] = Xc, Xr, Xi, dx, dy, ds
            conv = ~sing & (np.abs(Xi) < F(0.5)) & (np.abs(Xr) < F(0.5)) & (np.abs(Xc) < F(0.5))
            done[idx[conv]] = True
            huge = ~(np.abs(Xi) <= lim) | ~(np.abs(Xr) <= lim) | ~(np.abs(Xc) <= lim)
            dead = sing | (~conv & huge)
            alive[idx[dead]] = False
            mv = ~conv & ~dead
            j = idx[mv]
            c[j] += np.rint(Xc[mv]).astype(np.int64)
            r[j] += np.rint(Xr[mv]).astype(np.int64)
            layer[j] += np.rint(Xi[mv]).astype(np.int64)
            out = (layer[j] < 1) | (layer[j] > N_LAYERS) | (c[j] < BORDER) | (c[j] >= cols - BORDER) | (r[j] < BORDER) | (r[j] >= rows - BORDER)
            alive[j[out]] = False
        ok = np.nonzero(alive & done)[0]
        layer, r, c = layer[ok], r[ok], c[ok]
        xc, xr, xi, gx, gy, gs = xc[ok], xr[ok], xi[ok], gx[ok], gy[ok], gs[ok]
        D = dog[layer, r, c]
        t = gx * xc + gy * xr + gs * xi
        contr = D * (F(1) / F(255)) + t * F(0.5)
        keep = ~(np.abs(contr) * F(N_LAYERS) < F(CONTRAST))
        _, _, _, dxx, dyy, _, dxy, _, _ = _derivs(dog, layer, r, c)
        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
        keep &= ~((det <= 0) | (tr * tr * F(EDGE) >= F((EDGE + 1) ** 2) * det))
    scale = F(1 << octave)
    px = (c[keep].astype(F) + xc[keep]) * scale * F(0.5)
    py = (r[keep].astype(F) + xr[keep]) * scale * F(0.5)
    return np.stack([px, py], 1)


def keypoints(img_rgb, pyr=None):
    """float32 [n, 2] keypoint positions (x, y) of every accepted extremum, octave by octave (not deduplicated)"""
    pyr = pyramid(img_rgb) if pyr is None else pyr
    pts = [refine(dog, _candidates(dog), o) for o, (_, dog) in enumerate(pyr)]
    return np.concatenate(pts) if pts else np.zeros((0, 2), F)


def dilate(mask, kernel_size, iterations):
    """cv2.dilate(mask, ones((k, k)), iterations): anchor k // 2, pixels outside the array do not contribute"""
    lo, hi = (kernel_size // 2) * iterations, (kernel_size - 1 - kernel_size // 2) * iterations
    out = mask.astype(np.uint8)
    for axis in (1, 0):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for d in range(-lo, hi + 1):
            src = np.clip(np.arange(n) + d, 0, n - 1)
            valid = ((np.arange(n) + d) >= 0) & ((np.arange(n) + d) < n)
            taken = np.take(out, src, axis=axis)
            shape = [1, 1]
            shape[axis] = -1
            acc = np.maximum(acc, taken * valid.reshape(shape).astype(np.uint8))
        out = acc
    return out


def interest_mask(img_rgb, kernel_size=5, dil_iter=3):
    """-> (points uint8 [W,H], mask uint8 [W,H], keypoint count): the truncated positions set at [x, y] as
    estimate_relative_pose does (interest_regions[POI[:,0], POI[:,1]] = 1), then dilated"""
    H, W = img_rgb.shape[:2]
    kp = keypoints(img_rgb)
    xy = kp.astype(np.int64)
    pts = np.zeros((W, H), np.uint8)
    ok = (xy[:, 0] >= 0) & (xy[:, 0] < W) & (xy[:, 1] >= 0) & (xy[:, 1] < H)
    pts[xy[ok, 0], xy[ok, 1]] = 1
    return pts, dilate(pts, kernel_size, dil_iter), int(ok.sum())


def blob_frame(H, W, seed):
    """a synthetic uint8 [H, W, 3] frame of six Gaussian blobs on a flat background: keypoints at known places, for tests and
    benchmarks (the synthetic scene's smooth renders can hold none)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    v = np.full((H, W), 60.0)
    for _ in range(6):
        cy, cx, s = rng.uniform(8, H - 8), rng.uniform(8, W - 8), rng.uniform(1.5, 5)
        v += rng.uniform(-50, 150) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    img = np.clip(v, 0, 255).astype(np.uint8)
    return np.stack([img, (img * 0.7).astype(np.uint8), (img * 0.5).astype(np.uint8)], -1)
