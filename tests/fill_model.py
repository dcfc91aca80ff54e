"""numpy model of acn_fill_stats: the expressions of include/actinon_hip.h ("Filling") evaluated tap by tap in the header's order,
vectorised over the pixels, in the style of denoise_model.py.  numpy's elementwise + - * / are IEEE binary64 and never contracted;
exp and sqrt go through the host build of csrc/acn_detmath.h (the `detmath_cpu` fixture of conftest.py), so the device is compared
with this model bit for bit."""
import numpy as np

import denoise_model as D
import stats_model as SM

DEFAULT_RADIUS, MAX_RADIUS, DEFAULT_SIGMA_PX, DEFAULT_SIGMA_PLANE = 3, 8, 1.5, 0.1
RENDERED, BACKGROUND, FILLED, UNFILLED = 0, 1, 2, 3
CLASS_NAMES = ("rendered", "background", "filled", "unfilled")


def emitter(rec):
    with np.errstate(invalid="ignore"):
        kind = np.nan_to_num(rec[:, 12], nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)
    return (kind & D.EMITTER) != 0


def fill(lib, stats, rec, w, h, background, radius=None, normal_power_log2=None, demodulate=True, sigma_px=None, sigma_plane=None,
         detail=None):
    """stats [h*w,8], rec [h*w,16] -> ( out_stats [h*w,8], need [h,w] ); None is the default of the header.  detail (a dict)
    receives `cls` [h,w] (RENDERED .. UNFILLED), `donor`, and the sums `sw`, `sa`, `swv`, `su` [h,w(,3)] of the receivers"""
    stats = np.ascontiguousarray(stats, dtype=np.float64).reshape(h * w, SM.STRIDE)
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(h * w, D.STRIDE)
    R = DEFAULT_RADIUS if radius is None else radius
    npl = D.DEFAULT_NORMAL_POWER_LOG2 if normal_power_log2 is None else normal_power_log2
    sigma_px = DEFAULT_SIGMA_PX if sigma_px is None else sigma_px
    sigma_plane = DEFAULT_SIGMA_PLANE if sigma_plane is None else sigma_plane
    bg = np.asarray(background, dtype=np.float64)
    taps = D.Taps(h, w)
    with np.errstate(all="ignore"):
        e = SM.empty(stats)
        a2 = D.albedo(rec, demodulate)
        a = a2.reshape(h, w, 3)
        c2 = stats[:, 1:4] / a2
        hit = rec[:, 0] < np.inf
        emit = emitter(rec)
        donor = (~e & hit & ~emit & np.isfinite(c2).all(axis=1)).reshape(h, w)
        present = (~e).reshape(h, w)
        has_var = (~e & (stats[:, 0] > 1.0)).reshape(h, w)
        n1 = stats[:, 0:1]
        u = (((stats[:, 4:7] / (n1 - 1.0)) / n1) / (a2 * a2)).reshape(h, w, 3)          # vm / ( a * a )
        c = c2.reshape(h, w, 3)
        key = rec[:, [7, 8, 13]].astype(np.int32).reshape(h, w, 3)
        N, P = rec[:, 4:7].reshape(h, w, 3), rec[:, 1:4].reshape(h, w, 3)
        receiver = (e & hit & ~emit & np.isfinite(rec[:, 1:7]).all(axis=1)).reshape(h, w)

        sa, sw, swv = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        sc, su = np.zeros((h, w, 3)), np.zeros((h, w, 3))
        s2 = sigma_px * sigma_px
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                inside, qy, qx = taps.at(dx, dy)
                ts = float(dx * dx + dy * dy) / s2
                k = D.det(lib, D.OP_EXP, np.array([-ts]))[0]
                pres = receiver & inside & present[qy, qx]
                sa = sa + np.where(pres, k, 0.0)
                take = pres & donor[qy, qx] & (key[qy, qx] == key).all(axis=-1)
                wn = D.dot(N, N[qy, qx])
                wn = np.where(wn > 0, wn, 0.0)
                for _ in range(npl):
                    wn = wn * wn
                Dv = P[qy, qx] - P
                ln = D.det(lib, D.OP_SQRT, D.dot(Dv, Dv))
                tp = np.where(ln > 0, (np.abs(D.dot(N, Dv)) / ln) / sigma_plane, 0.0)
                wt = wn * D.det(lib, D.OP_EXP, -(ts + tp))
                tv = take & has_var[qy, qx]
                sw = sw + np.where(take, wt, 0.0)
                sc = sc + np.where(take[..., None], wt[..., None] * c[qy, qx], 0.0)
                swv = swv + np.where(tv, wt, 0.0)
                su = su + np.where(tv[..., None], wt[..., None] * u[qy, qx], 0.0)

        filled = receiver & (sw > 0)
        var = filled & (swv > 0)
        mean = (sc / sw[..., None]) * a
        m2 = ((su / swv[..., None]) * (a * a)) * 2.0
        out = stats.copy().reshape(h, w, SM.STRIDE)
        need = np.full((h, w), np.inf)
        need[present] = -1.0
        back = (e & ~hit).reshape(h, w)
        out[back] = np.concatenate([[1.0], bg, [0.0, 0.0, 0.0, 0.0]])
        need[back] = 0.0
        frec = np.zeros((h, w, SM.STRIDE))
        frec[..., 0] = np.where(var, 2.0, 1.0)
        frec[..., 1:4] = mean
        frec[..., 4:7] = np.where(var[..., None], m2, 0.0)
        out[filled] = frec[filled]
        need[filled] = (1.0 - sw / sa)[filled]
    cls = np.full((h, w), UNFILLED)
    cls[present], cls[back], cls[filled] = RENDERED, BACKGROUND, FILLED
    if detail is not None:
        detail.update(cls=cls, donor=donor, sw=sw, sa=sa, swv=swv, su=su, u=u, a=a)
    return out.reshape(h * w, SM.STRIDE), need


def classes(stats_in, need, rec):
    """the class of every position from the input records and the need: a FILLED position in a flat region has need 0 as a
    BACKGROUND one has, so the misses are told by their surface records"""
    e = SM.empty(np.asarray(stats_in, dtype=np.float64).reshape(-1, SM.STRIDE)).reshape(need.shape)
    cls = np.full(need.shape, FILLED)
    cls[~e] = RENDERED
    cls[e & np.isinf(need)] = UNFILLED
    cls[e & ~(np.asarray(rec)[:, 0] < np.inf).reshape(need.shape)] = BACKGROUND
    return cls


def counts(cls):
    return {name: int((cls == k).sum()) for k, name in enumerate(CLASS_NAMES)}


def lattice_mask(w, h, lattice):
    y, x = np.mgrid[0:h, 0:w]
    return (x % lattice == 0) & (y % lattice == 0)


def synthetic_sparse(w, h, lattice, seed=5):
    """The frame of denoise_model.synthetic as a sparse one: statistics records (n = 4, a few with n = 1) kept on every lattice-th
    pixel of every lattice-th row and EMPTY elsewhere; a class one pixel wide that lies between the lattice points, so that its
    receivers find no donor of their surface; the misses, the emitter, the NaN and the inf pixel of the frame.
    -> stats [h*w,8], records [h*w,16]"""
    linear, rec = D.synthetic(w, h, seed)
    rng = np.random.default_rng(seed + 100)
    y, x = np.mgrid[0:h, 0:w]
    rec = rec.reshape(h, w, D.STRIDE).copy()
    thin = (x == 5) if w > 5 else (y == 5) if h > 5 else (x == 1) & (y == 1)
    thin &= rec[..., 0] < np.inf
    rec[thin, 7] = 77
    stats = np.zeros((h, w, SM.STRIDE))
    stats[..., 0] = 4.0
    stats[..., 1:4] = linear
    stats[..., 4:7] = rng.exponential(0.05, (h, w, 3)) * np.where(np.isfinite(linear), np.abs(linear), 1.0)
    one = rng.random((h, w)) < 0.2
    stats[one, 0] = 1.0
    stats[one, 4:7] = 0.0
    stats[~lattice_mask(w, h, lattice)] = 0.0
    return stats.reshape(h * w, SM.STRIDE), rec.reshape(h * w, D.STRIDE)
