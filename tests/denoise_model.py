"""numpy model of acn_denoise: the expressions of include/actinon_hip.h evaluated tap by tap in the header's order, vectorised
over the pixels.  numpy's elementwise + - * / are IEEE binary64 and never contracted; exp and sqrt go through the host build of
csrc/acn_detmath.h (the `detmath_cpu` fixture of conftest.py), so the device is compared with this model bit for bit."""
import numpy as np

NO_DEMODULATE, NORMAL_POWER_SET = 1, 2
DEFAULT_ITERATIONS, DEFAULT_NORMAL_POWER_LOG2, DEFAULT_SIGMA_PLANE, DEFAULT_SIGMA_LUM = 5, 7, 0.1, 4.0
MAX_ITERATIONS, MAX_NORMAL_POWER_LOG2 = 8, 10
EMITTER = 1
STRIDE = 16
K = (0.0625, 0.25, 0.375, 0.25, 0.0625)
OP_EXP, OP_SQRT = 5, 7      # op codes of tests/csrc/detmath_cpu.c


def det(lib, op, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lib.detmath_eval(op, x.ctypes.data, None, out.ctypes.data, x.size)
    return out


def lum(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def albedo(rec, demodulate=True):
    alb = rec[:, 9:12]
    return np.where(alb > 0.01, alb, 1.0) if demodulate else np.ones_like(alb)


def filterable(rec, c):
    with np.errstate(invalid="ignore"):
        kind = np.nan_to_num(rec[:, 12], nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)
    return (rec[:, 0] < np.inf) & ((kind & EMITTER) == 0) & np.isfinite(c).all(axis=1)


class Taps:
    """the pixel ( x + dx, y + dy ) of every pixel of an h x w image: clamped to the pixel itself where it is off the image"""

    def __init__(self, h, w):
        self.y, self.x = np.mgrid[0:h, 0:w]
        self.h, self.w = h, w

    def at(self, dx, dy):
        qx, qy = self.x + dx, self.y + dy
        inside = (qx >= 0) & (qx < self.w) & (qy >= 0) & (qy < self.h)
        return inside, np.where(inside, qy, self.y), np.where(inside, qx, self.x)


def denoise(lib, linear, rec, iterations=None, normal_power_log2=None, demodulate=True, sigma_plane=None, sigma_lum=None):
    """linear [h,w,3], rec [h*w,16] -> [h,w,3]; None is the default of the header"""
    linear = np.ascontiguousarray(linear, dtype=np.float64)
    h, w = linear.shape[:2]
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(h * w, STRIDE)
    iterations = DEFAULT_ITERATIONS if iterations is None else iterations
    npl = DEFAULT_NORMAL_POWER_LOG2 if normal_power_log2 is None else normal_power_log2
    sigma_plane = DEFAULT_SIGMA_PLANE if sigma_plane is None else sigma_plane
    sigma_lum = DEFAULT_SIGMA_LUM if sigma_lum is None else sigma_lum
    taps = Taps(h, w)
    with np.errstate(all="ignore"):
        a = albedo(rec, demodulate).reshape(h, w, 3)
        c = linear / a
        ok = filterable(rec, c.reshape(-1, 3)).reshape(h, w)
        key = rec[:, [7, 8, 13]].astype(np.int32).reshape(h, w, 3)
        N, P = rec[:, 4:7].reshape(h, w, 3), rec[:, 1:4].reshape(h, w, 3)

        def match(inside, qy, qx):
            return ok & inside & ok[qy, qx] & (key[qy, qx] == key).all(axis=-1)

        # 2 variance
        l = lum(c)
        n, s1, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                inside, qy, qx = taps.at(dx, dy)
                m = match(inside, qy, qx)
                lq = l[qy, qx]
                n = n + np.where(m, 1.0, 0.0)
                s1 = s1 + np.where(m, lq, 0.0)
                s2 = s2 + np.where(m, lq * lq, 0.0)
        mean = s1 / n
        v = s2 / n - mean * mean
        var = np.where(ok & (v > 0), v, 0.0)

        # 3 levels
        for i in range(iterations):
            s = 1 << i
            l = lum(c)
            den = sigma_lum * det(lib, OP_SQRT, var) + 1e-8
            sw, sd, sv = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
            for tj in range(5):
                for ti in range(5):
                    inside, qy, qx = taps.at((ti - 2) * s, (tj - 2) * s)
                    m = match(inside, qy, qx)
                    cq, vq = c[qy, qx], var[qy, qx]
                    if tj == 2 and ti == 2:
                        wt = np.full((h, w), K[2] * K[2])
                    else:
                        wn = dot(N, N[qy, qx])
                        wn = np.where(wn > 0, wn, 0.0)
                        for _ in range(npl):
                            wn = wn * wn
                        D = P[qy, qx] - P
                        ln = det(lib, OP_SQRT, dot(D, D))
                        tp = np.where(ln > 0, (np.abs(dot(N, D)) / ln) / sigma_plane, 0.0)
                        tl = np.abs(lum(cq) - l) / den
                        wt = ((K[tj] * K[ti]) * wn) * det(lib, OP_EXP, -(tp + tl))
                    sw = sw + np.where(m, wt, 0.0)
                    sd = sd + np.where(m[..., None], wt[..., None] * (cq - c), 0.0)
                    sv = sv + np.where(m, (wt * wt) * vq, 0.0)
            c = np.where(ok[..., None], c + sd / sw[..., None], c)
            var = np.where(ok, sv / (sw * sw), var)
        # 4 remodulate
        return np.where(ok[..., None], c * a, linear)


def blank(n):
    rec = np.zeros((n, STRIDE))
    rec[:, 0] = np.inf; rec[:, 7] = -1; rec[:, 8] = -1; rec[:, 14] = 1.0
    return rec


def synthetic(w, h, seed=5):
    """A hand-made frame with everything the filter tells apart: three objects in slanted bands (one seen after a hop), curved
    normals and positions, albedo channels above 0.01, below it and zero, misses, emitters, a NaN and an inf pixel.
    -> linear [h,w,3], records [h*w,16]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    obj = ((x + y // 2) * 3) // (w + h // 2 + 1)                        # 0, 1, 2
    u, v = (x + 0.5) / max(w, h), (y + 0.5) / max(w, h)
    px, py = 4 * u - 2, 4 * v - 1                                       # the surface z = f( x, y ) of each object and its normal
    pos = np.stack([px, py, 0.6 * np.sin(1.5 * px + obj) + 0.15 * py * py + obj], axis=-1)
    nrm = np.stack([-0.9 * np.cos(1.5 * px + obj), -0.3 * py, np.ones_like(px)], axis=-1)
    nrm = nrm / np.sqrt((nrm * nrm).sum(axis=-1, keepdims=True))
    colours = np.array([[0.8, 0.6, 0.3], [0.25, 0.5, 0.9], [0.005, 0.0, 0.7]])
    rec = blank(h * w).reshape(h, w, STRIDE)
    rec[..., 0] = np.sqrt((pos * pos).sum(axis=-1)) + 3
    rec[..., 1:4] = pos
    rec[..., 4:7] = nrm
    rec[..., 7] = np.where(obj == 1, -1, 3 + obj)
    rec[..., 8] = np.where(obj == 1, 9, -1)
    rec[..., 9:12] = colours[obj]
    rec[..., 12] = np.where(obj == 1, 8 + 16, 2)
    rec[..., 13] = np.where((obj == 2) & (y >= h // 2), 1, 0)
    rec[..., 14] = np.where(rec[..., 13] > 0, 0.9, 1.0)
    shade = 0.4 + 0.3 * np.sin(5 * u) * np.cos(4 * v) + 0.2 * obj
    linear = np.where(colours[obj] > 0.01, colours[obj], 1.0) * (shade[..., None] + rng.exponential(0.25, (h, w, 3)))
    linear[rng.random((h, w)) < 0.03] *= 30.0                             # fireflies
    miss = ((x * 7 + y * 3) % 23 == 0) | ((x >= w - 1 - w // 8) & (y <= h // 6))
    rec[miss] = blank(1)[0]
    linear[miss] = [0.3, 0.35, 0.4]
    emit = (x >= w // 3) & (x <= w // 3 + w // 10) & (y >= h // 3) & (y <= h // 3 + h // 8) & ~miss
    rec[emit, 12] = 1 + 32
    rec[emit, 9:12] = [1.0, 0.9, 0.8]
    linear[emit] = [25.0, 22.5, 20.0]
    linear[h // 2, w // 2, 1] = np.nan
    linear[h - 1, 0, 2] = np.inf
    return linear, rec.reshape(h * w, STRIDE)


def mse(x, ref):
    return float(np.mean((np.clip(x, 0, 1) - np.clip(ref, 0, 1)) ** 2))
