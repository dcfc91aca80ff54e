"""A numpy model of the device-resident frame, written from include/actinon_hip.h (acn_frame_*): the key, the selection, the
positions (a sequential generator: no jump), the push (a plain loop in the order of the array) and the image.  The host functions of
actinon_amd/csrc/acn_frame_host.h and the kernels of k_frame.hip are compared with it bit for bit."""
import numpy as np

A, C = 6364136223846793005, 1442695040888963407          # ACN_LCG00_A / _C of include/actinon_hip.h
MASK = 2 ** 64 - 1
A_INV = pow(A, -1, 2 ** 64)
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))     # ( dx, dy ) in the driver's order
SEED = 21943294                                           # scene.c:799


def lcg(s):
    return (s * A + C) & MASK


def lcg_steps(s, n):
    for _ in range(n):
        s = lcg(s)
    return s


def draw_double(s):
    """( double )s * 2^-64 of a uint64 draw: the conversion rounds to nearest even, the product is exact"""
    return float(s) * 2.0 ** -64


def seed_for_draw(t, nth=1):
    """The seed whose nth draw is t: ( t - C ) * A^-1 mod 2^64, nth times"""
    for _ in range(nth):
        t = ((t - C) * A_INV) & MASK
    return t


def avg(acc):
    """acc [n,6] -> [n,3]: clr * ( weight > 0 ? 1.0 / weight : 1.0 )"""
    acc = np.asarray(acc, dtype=np.float64).reshape(-1, 6)
    wgt = acc[:, 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(wgt > 0, 1.0 / np.where(wgt > 0, wgt, 1.0), 1.0)
    return acc[:, 2:5] * f[:, None]


def key(acc, w, h):
    a = avg(acc).reshape(h, w, 3)
    g = np.zeros((h, w))
    for dx, dy in NEIGHBOURS:
        sh = np.zeros_like(a)
        ok = np.zeros((h, w), dtype=bool)
        ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
        xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
        sh[yd, xd] = a[ys, xs]
        ok[yd, xd] = True
        with np.errstate(invalid="ignore", over="ignore"):
            d = a - sh
            g1 = np.where(ok, (d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1]) + (d[..., 2] * d[..., 2]), 0.0)
            g = np.where(g1 > g, g1, g)
    return g.reshape(-1)


def select(k, sqr_threshold):
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.asarray(k) > sqr_threshold).astype(np.int64)


def positions(index, samples, rval, w):
    """-> ( pos [len(index)*samples,2], rval after the draws ): one generator, two draws per entry, in the order of the array"""
    pos = np.empty((len(index) * samples, 2), dtype=np.float64)
    e = 0
    for p in index:
        i, j = int(p) % w, int(p) // w
        for _ in range(samples):
            rval = lcg(rval)
            dx = draw_double(rval)
            rval = lcg(rval)
            dy = draw_double(rval)
            pos[e] = (float(i) + dx, float(j) + dy)
            e += 1
    return pos, rval


def centres(w, h):
    idx = np.arange(w * h)
    return np.stack([(idx % w) + 0.5, (idx // w) + 0.5], axis=1)


def push(acc, w, h, pos, clr):
    """lum_image_push of every entry in the order of the array, weight 1 -> ( the new accumulator, the pixel each entry went to or -1 )"""
    acc = np.array(acc, dtype=np.float64).reshape(-1, 6)
    target = np.full(len(pos), -1, dtype=np.int64)
    for e, ((px, py), c) in enumerate(zip(pos, clr)):
        x, y = int(px), int(py)                            # ( int32_t ): truncation
        if 0 <= x < w and 0 <= y < h:
            r = acc[y * w + x]
            r[0] += px
            r[1] += py
            r[2] += c[0]
            r[3] += c[1]
            r[4] += c[2]
            r[5] += 1.0
            target[e] = y * w + x
    return acc, target


def image(acc):
    a = avg(acc)
    with np.errstate(invalid="ignore"):
        q = np.where(a > 0.0, np.where(a < 1.0, (np.where((a > 0.0) & (a < 1.0), a, 0.0) * 256).astype(np.int64), 255), 0)
    return a, q.astype(np.uint8)


def gradient_pass(acc, w, h, sqr_threshold, samples, rval, render):
    """One cycle of the driver on host arrays; render( pos ) -> colours.  -> ( acc, rval, flagged )"""
    idx = select(key(acc, w, h), sqr_threshold)
    pos, rval = positions(idx, samples, rval, w)
    if len(idx):
        acc, _ = push(acc, w, h, pos, render(pos))
    return np.array(acc, dtype=np.float64).reshape(-1, 6), rval, len(idx)


def random_frame(rng, w, h, empty=0.15, flat=0.3):
    """An accumulator as passes leave it: integer weights, some records empty (weight 0, zeros), some neighbourhoods flat"""
    n = w * h
    wgt = rng.integers(1, 6, n).astype(np.float64)
    clr = rng.uniform(0.0, 1.5, (n, 3)) * wgt[:, None]
    same = rng.random(n) < flat
    clr[same] = 0.25 * wgt[same, None]
    acc = np.zeros((n, 6))
    acc[:, 0] = rng.uniform(0, w, n) * wgt
    acc[:, 1] = rng.uniform(0, h, n) * wgt
    acc[:, 2:5] = clr
    acc[:, 5] = wgt
    acc[rng.random(n) < empty] = 0.0
    return acc
