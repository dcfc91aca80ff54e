"""numpy model of the lens sample statistics (acn_render_lens_stats, acn_lens_stats_merge, acn_lens_stats_resolve_dev,
acn_denoise_stats): the expressions of include/actinon_hip.h in the header's order, vectorised over positions.  numpy's elementwise
+ - * / are IEEE binary64 and never contracted; sqrt, exp and pow go through the host build of csrc/acn_detmath.h (the `detmath_cpu`
fixture of conftest.py, as lens_model.sqrt does), so the device is compared with this model bit for bit."""
import numpy as np

import denoise_model as D
import lens_model as M

STRIDE = 8
NOISE_FLOOR = 0.01
OP_POW = 6          # op code of tests/csrc/detmath_cpu.c
W2 = (0.2126 * 0.2126, 0.7152 * 0.7152, 0.0722 * 0.0722)


def records(L):
    """L [n, K, 3] -> records [n, 8]: n = K, the ordered mean, m2 = ( ( 0.0 + d0 * d0 ) + d1 * d1 ) + ..., dk = Lk - mean"""
    L = np.asarray(L, dtype=np.float64)
    n, K = L.shape[:2]
    mean = M.ordered_mean(L)
    m2 = np.zeros((n, 3))
    for k in range(K):
        d = L[:, k] - mean
        m2 = m2 + d * d
    rec = np.zeros((n, STRIDE))
    rec[:, 0] = float(K)
    rec[:, 1:4] = mean
    rec[:, 4:7] = m2
    return rec


def empty(rec):
    with np.errstate(invalid="ignore"):
        return ~((rec[:, 0] >= 1.0) & (rec[:, 0] < np.inf))


def merge(acc, part, index=None):
    """-> a copy of acc with part[ j ] merged into acc[ index[ j ] ] (index None: acc[ j ]); indices out of range are skipped"""
    acc = np.array(acc, dtype=np.float64)
    part = np.asarray(part, dtype=np.float64)
    idx = np.arange(len(part)) if index is None else np.asarray(index, dtype=np.int64)
    use = (idx >= 0) & (idx < len(acc))
    idx, b = idx[use], part[use]
    take = ~empty(b)
    idx, b = idx[take], b[take]
    a = acc[idx]
    ea = empty(a)
    with np.errstate(all="ignore"):
        na, nb = a[:, 0:1], b[:, 0:1]
        n = na + nb
        dl = b[:, 1:4] - a[:, 1:4]
        mean = a[:, 1:4] + dl * (nb / n)
        m2 = (a[:, 4:7] + b[:, 4:7]) + (dl * dl) * ((na * nb) / n)
    out = np.concatenate([n, mean, m2, np.zeros_like(n)], axis=1)
    out[ea] = b[ea]                                                        # bit for bit
    acc[idx] = out
    return acc


def variance_of_mean(rec):
    """( m2 / ( n - 1 ) ) / n per channel where n > 1, else NaN ("none")"""
    n = rec[:, 0:1]
    with np.errstate(all="ignore"):
        vm = (rec[:, 4:7] / (n - 1.0)) / n
        return np.where(~empty(rec)[:, None] & (n > 1.0), vm, np.nan)


def noise(lib, rec):
    vm = variance_of_mean(rec)
    with np.errstate(all="ignore"):
        has = ~empty(rec) & (rec[:, 0] > 1.0)
        v = np.where(has[:, None], vm, 0.0)
        s = (W2[0] * v[:, 0] + W2[1] * v[:, 1]) + W2[2] * v[:, 2]
        x = M.sqrt(lib, s) / (np.abs(D.lum(rec[:, 1:4])) + NOISE_FLOOR)
    return np.where(has, x, np.inf)


def cl_sat(lib, c, gamma):
    """cl_s_sat: acn_pow per channel, then the clamp x > 0 ? x < 1 ? x : 1 : 0"""
    c = np.ascontiguousarray(c, dtype=np.float64)
    g = np.full_like(c, float(gamma))
    x = np.empty_like(c)
    lib.detmath_eval(OP_POW, c.ctypes.data, g.ctypes.data, x.ctypes.data, c.size)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0.0, np.where(x < 1.0, x, 1.0), 0.0)


def resolve(lib, rec, background, gamma, linear):
    """-> ( rgb [n,3], noise [n] )"""
    rec = np.asarray(rec, dtype=np.float64)
    c = np.where(empty(rec)[:, None], np.asarray(background, dtype=np.float64)[None, :], rec[:, 1:4])
    return (c if linear else cl_sat(lib, c, gamma)), noise(lib, rec)


def var_raw(rec, a):
    """step 2 of acn_denoise_stats before the prefilter: -1.0 stands for "none" """
    vm = variance_of_mean(rec)
    with np.errstate(all="ignore"):
        has = ~empty(rec) & (rec[:, 0] > 1.0)
        v = np.where(has[:, None], vm, 0.0)
        x = (W2[0] * (v[:, 0] / (a[:, 0] * a[:, 0])) + W2[1] * (v[:, 1] / (a[:, 1] * a[:, 1]))) + W2[2] * (v[:, 2] / (a[:, 2] * a[:, 2]))
    return np.where(has, x, -1.0)


def denoise_stats(lib, stats, rec, w, h, background, iterations=None, normal_power_log2=None, demodulate=True, sigma_plane=None,
                  sigma_lum=None, detail=None):
    """stats [h*w,8], rec [h*w,16] -> [h,w,3].  detail (a dict) receives `ok`, `var_raw` and the prefiltered `var` [h,w]"""
    stats = np.ascontiguousarray(stats, dtype=np.float64).reshape(h * w, STRIDE)
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(h * w, D.STRIDE)
    iterations = D.DEFAULT_ITERATIONS if iterations is None else iterations
    npl = D.DEFAULT_NORMAL_POWER_LOG2 if normal_power_log2 is None else normal_power_log2
    sigma_plane = D.DEFAULT_SIGMA_PLANE if sigma_plane is None else sigma_plane
    sigma_lum = D.DEFAULT_SIGMA_LUM if sigma_lum is None else sigma_lum
    taps = D.Taps(h, w)
    e = empty(stats)
    linear = np.where(e[:, None], np.asarray(background, dtype=np.float64)[None, :], stats[:, 1:4]).reshape(h, w, 3)
    with np.errstate(all="ignore"):
        a2 = D.albedo(rec, demodulate)
        a = a2.reshape(h, w, 3)
        c = linear / a
        ok = (D.filterable(rec, c.reshape(-1, 3)) & ~e).reshape(h, w)
        key = rec[:, [7, 8, 13]].astype(np.int32).reshape(h, w, 3)
        N, P = rec[:, 4:7].reshape(h, w, 3), rec[:, 1:4].reshape(h, w, 3)

        def match(inside, qy, qx):
            return ok & inside & ok[qy, qx] & (key[qy, qx] == key).all(axis=-1)

        # 2 the measured variance and its 3 x 3 prefilter
        vr = var_raw(stats, a2).reshape(h, w)
        g = (0.25, 0.5, 0.25)
        sw, sv = np.zeros((h, w)), np.zeros((h, w))
        for j in range(3):
            for i in range(3):
                inside, qy, qx = taps.at(i - 1, j - 1)
                vq = vr[qy, qx]
                m = match(inside, qy, qx) & ~(vq < 0.0)
                sw = sw + np.where(m, g[j] * g[i], 0.0)
                sv = sv + np.where(m, (g[j] * g[i]) * vq, 0.0)
        var = np.where(ok & (sw > 0), sv / sw, 0.0)
        if detail is not None:
            detail.update(ok=ok, var_raw=vr, var=var.copy())

        # 3 levels: those of acn_denoise
        for it in range(iterations):
            s = 1 << it
            l = D.lum(c)
            den = sigma_lum * D.det(lib, D.OP_SQRT, var) + 1e-8
            sw, sd, sv = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
            for tj in range(5):
                for ti in range(5):
                    inside, qy, qx = taps.at((ti - 2) * s, (tj - 2) * s)
                    m = match(inside, qy, qx)
                    cq, vq = c[qy, qx], var[qy, qx]
                    if tj == 2 and ti == 2:
                        wt = np.full((h, w), D.K[2] * D.K[2])
                    else:
                        wn = D.dot(N, N[qy, qx])
                        wn = np.where(wn > 0, wn, 0.0)
                        for _ in range(npl):
                            wn = wn * wn
                        Dv = P[qy, qx] - P
                        ln = D.det(lib, D.OP_SQRT, D.dot(Dv, Dv))
                        tp = np.where(ln > 0, (np.abs(D.dot(N, Dv)) / ln) / sigma_plane, 0.0)
                        tl = np.abs(D.lum(cq) - l) / den
                        wt = ((D.K[tj] * D.K[ti]) * wn) * D.det(lib, D.OP_EXP, -(tp + tl))
                    sw = sw + np.where(m, wt, 0.0)
                    sd = sd + np.where(m[..., None], wt[..., None] * (cq - c), 0.0)
                    sv = sv + np.where(m, (wt * wt) * vq, 0.0)
            c = np.where(ok[..., None], c + sd / sw[..., None], c)
            var = np.where(ok, sv / (sw * sw), var)
        # 4 remodulate
        return np.where(ok[..., None], c * a, linear)
