"""numpy model of the layered lens records and their filter (acn_lens_layers_reduce, acn_render_lens_layers, acn_denoise_layers): the
definitions of include/actinon_hip.h line by line -- the split one position at a time, the filter vectorised over the pixels.  numpy's
elementwise + - * / on float64 are IEEE binary64 and never contracted; sqrt and exp go through the host build of csrc/acn_detmath.h
(the `detmath_cpu` fixture of conftest.py), so the device is compared with this model bit for bit.  The one thing the header leaves
open is which NaN a NaN result is: same_bits() takes a NaN for a NaN."""
import numpy as np

import denoise_model as D
import lens_surface_model as R
import stats_model as T

SURF_PLANES, STATS_PLANES = 2, 3


def same_bits(got, want):
    """-> the indices where got and want differ in their bits, a NaN on both sides counting as equal"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    differ = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    return np.argwhere(differ)


# ---- the split ----

def parts(records):
    """records [K,16] of one position -> ( ks0, ks1, ksr ): the members of layer 0, of layer 1 (empty: absent) and of the rest, each
    in the order of k"""
    records = np.asarray(records, dtype=np.float64)
    K = len(records)
    _, ks0 = R.dominant(records)
    others = [k for k in range(K) if k not in set(ks0)]
    ks1 = []
    if others:
        _, sub = R.dominant(records[others])                # the same rule over the samples that are not in layer 0
        ks1 = [others[j] for j in sub]
    taken = set(ks0) | set(ks1)
    return list(ks0), ks1, [k for k in range(K) if k not in taken]


def layer_surface(lib, records, ks):
    """the aggregate record of acn_surface_reduce over the members ks alone, [ 15 ] = m / K; no members: the absent layer"""
    K = len(records)
    if not ks:
        out = R.miss_record(0, 0.0)
        return out
    out = R.reduce_one(lib, records[ks])                    # one class: all of them are its members, in the order of k
    out[15] = np.float64(len(ks)) / np.float64(K)
    return out


def part_stats(L, ks):
    """L [K,3] -> the record of the members ks: n, the ordered mean from +0.0, m2 in a second pass; no members: eight zeros"""
    rec = np.zeros(T.STRIDE)
    if not ks:
        return rec
    with np.errstate(all="ignore"):
        s = np.zeros(3)
        for k in ks:
            s = s + L[k]
        mean = s / np.float64(len(ks))
        m2 = np.zeros(3)
        for k in ks:
            d = L[k] - mean
            m2 = m2 + d * d
    rec[0] = float(len(ks)); rec[1:4] = mean; rec[4:7] = m2
    return rec


def split(lib, records, radiance):
    """records [n,K,16], radiance [n,K,3] -> ( surface [2,n,16], stats [3,n,8] )"""
    records = np.asarray(records, dtype=np.float64)
    radiance = np.asarray(radiance, dtype=np.float64)
    n, K = records.shape[:2]
    assert records.shape == (n, K, R.STRIDE) and radiance.shape == (n, K, 3) and K >= 1, (records.shape, radiance.shape)
    surf, st = np.zeros((SURF_PLANES, n, R.STRIDE)), np.zeros((STATS_PLANES, n, T.STRIDE))
    for i in range(n):
        ks = parts(records[i])
        for l in range(SURF_PLANES):
            surf[l, i] = layer_surface(lib, records[i], ks[l])
        for l in range(STATS_PLANES):
            st[l, i] = part_stats(radiance[i], ks[l])
    return surf, st


# hand-made inputs whose answer is known without the model: { name: ( records [n,K,16], per position ( ks0, ks1, ksr ) ) }
def hand_made():
    rng = np.random.default_rng(11)
    A_, B_, C_ = (5, -1, 0), (7, -1, 0), (-1, 5, 1)
    v = lambda c: R.varied(rng, *c)
    cases = {}
    cases["K = 1"] = (np.array([[v(A_)], [R.miss_record(1, 0.5)]]), [([0], [], []), ([0], [], [])])
    cases["all one class"] = (np.array([[v(B_) for _ in range(6)]]), [(list(range(6)), [], [])])
    cases["all misses"] = (np.array([[R.miss_record(0, 1.0) for _ in range(4)], [R.miss_record(0), R.miss_record(2, 0.5), R.miss_record(2, 0.25), R.miss_record(0)]]),
                           [([0, 1, 2, 3], [], []), ([0, 3], [1, 2], [])])
    # layer 0: A and B have two members each, A comes first; layer 1 is then B alone against C
    cases["tie for layer 0"] = (np.array([[v(A_), v(B_), v(C_), v(B_), v(A_)], [v(B_), v(A_), v(C_), v(A_), v(B_)]]),
                                [([0, 4], [1, 3], [2]), ([0, 4], [1, 3], [2])])
    # layer 0 is A (three); B and C tie with two each, C comes first among the samples outside layer 0
    cases["tie for layer 1"] = (np.array([[v(A_), v(C_), v(A_), v(B_), v(B_), v(C_), v(A_)], [v(A_), v(B_), v(C_), v(A_), v(B_), v(C_), v(A_)]]),
                                [([0, 2, 6], [1, 5], [3, 4]), ([0, 3, 6], [1, 4], [2, 5])])
    cases["three classes of one sample"] = (np.array([[v(A_), v(B_), v(C_)], [v(C_), v(B_), v(A_)]]), [([0], [1], [2]), ([0], [1], [2])])
    cases["a miss is layer 0, a miss is layer 1"] = (np.array([[R.miss_record(0), v(A_), R.miss_record(0), v(B_), R.miss_record(0)],
                                                               [v(A_), R.miss_record(0), v(A_), v(A_), R.miss_record(0)]]),
                                                     [([0, 2, 4], [1], [3]), ([0, 2, 3], [1, 4], [])])
    return cases


def synthetic_split(n, K, seed=3):
    """Records and radiances for the device test, position i on pattern i % 6 where K allows it (else the pure pattern):
    0 one class (layer 1 absent) | 1 two classes in turn (a tie for layer 0 at even K) | 2 a majority, then two classes that tie for
    layer 1 | 3 a majority of misses | 4 a minority of misses as layer 1 (a tie at K = 2) | 5 more than 8 classes: nine classes of one
    sample, THEN the first sample of layer 1 (the 8-class table has overflowed), other classes, and layer 0 last of all.
    Radiances: uniform, with -0.0, +inf and NaN samples at fixed positions.  -> records [n,K,16], radiance [n,K,3], patterns [n]"""
    rng = np.random.default_rng(seed + 1000 * n + K)
    A_, B_, C_ = (5, -1, 0), (7, 2, 1), (-1, 5, 1)
    hit = lambda c: R.varied(rng, *c)
    rec, pat = [], []
    for i in range(n):
        p = i % 6
        if (p in (1, 4) and K < 2) or (p == 2 and K < 3) or (p == 5 and K < 17):
            p = 0
        if p == 0:
            row = [hit(A_) for _ in range(K)]
        elif p == 1:
            row = [hit(A_ if k % 2 == 0 else B_) for k in range(K)]
        elif p == 2:
            t = max(1, (K - 1) // 4)
            row = [hit(A_) for _ in range(K - 2 * t)] + [hit(B_ if k % 2 == 0 else C_) for k in range(2 * t)]
        elif p == 3:
            m = K // 2 + 1
            row = [R.miss_record(0, rng.uniform(0.1, 1)) if k < m else hit(A_) for k in range(K)]
            row = [row[k] for k in rng.permutation(K)]
        elif p == 4:
            m = max(1, K // 3)
            row = [hit(A_) for _ in range(K - m)] + [R.miss_record(1, rng.uniform(0.1, 1)) for _ in range(m)]
            if K > 2:
                row = [row[0]] + [row[1 + k] for k in rng.permutation(K - 1)]
        else:
            w = (K - 9) * 3 // 8
            z = w + max(2, (K - 9) // 8)
            other = K - 9 - w - z
            assert other >= 0 and (other + 11) // 12 < w
            row = [hit((100 + j, -1, 0)) for j in range(9)] + [hit((300, -1, 0)) for _ in range(w)]
            row += [R.miss_record(2, 0.5) if j % 12 == 0 else hit((200 + j % 12, -1, 0)) for j in range(other)]
            row += [hit((400, 3, 2)) for _ in range(z)]
        assert len(row) == K
        rec.append(row); pat.append(p)
    rec = np.array(rec).reshape(n, K, R.STRIDE)
    L = rng.uniform(0.0, 2.0, (n, K, 3))
    for i in range(n):
        if i % 7 == 3:
            L[i, 0, 1] = -0.0
            L[i, K - 1, :] = -0.0
        if i % 7 == 5:
            L[i, K - 1, 0] = np.inf
        if i % 7 == 6:
            L[i, 0, 2] = np.nan
    return rec, L, np.array(pat)


# ---- the filter ----

def denoise_layers(lib, stats, rec, w, h, background, iterations=None, normal_power_log2=None, demodulate=True, sigma_plane=None,
                   sigma_lum=None, detail=None):
    """stats [3,h*w,8], rec [2,h*w,16] -> [h,w,3].  detail (a dict) receives `ok` [2,h,w] and `cross` [2]: how many taps of the levels
    the centres of layer l took from the OTHER layer of the tap pixel"""
    stats = np.ascontiguousarray(stats, dtype=np.float64).reshape(STATS_PLANES, h * w, T.STRIDE)
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(SURF_PLANES, h * w, D.STRIDE)
    iterations = D.DEFAULT_ITERATIONS if iterations is None else iterations
    npl = D.DEFAULT_NORMAL_POWER_LOG2 if normal_power_log2 is None else normal_power_log2
    sigma_plane = D.DEFAULT_SIGMA_PLANE if sigma_plane is None else sigma_plane
    sigma_lum = D.DEFAULT_SIGMA_LUM if sigma_lum is None else sigma_lum
    taps = D.Taps(h, w)
    bg = np.asarray(background, dtype=np.float64)
    cross = [0, 0]
    with np.errstate(all="ignore"):
        # steps 1 and 2 of acn_denoise_stats, per layer
        e = np.stack([T.empty(stats[l]) for l in range(STATS_PLANES)])
        a2 = np.stack([D.albedo(rec[l], demodulate) for l in range(2)])
        c = np.stack([stats[l][:, 1:4] / a2[l] for l in range(2)])
        ok = np.stack([D.filterable(rec[l], c[l]) & ~e[l] for l in range(2)]).reshape(2, h, w)
        vr = np.stack([T.var_raw(stats[l], a2[l]) for l in range(2)]).reshape(2, h, w)
        a = a2.reshape(2, h, w, 3)
        c = c.reshape(2, h, w, 3)
        key = rec[:, :, [7, 8, 13]].astype(np.int32).reshape(2, h, w, 3)
        N, P = rec[:, :, 4:7].reshape(2, h, w, 3), rec[:, :, 1:4].reshape(2, h, w, 3)

        def candidate(l, centre, inside, qy, qx):
            """-> ( taken [h,w], layer of the candidate [h,w] ) for the centres of layer l"""
            if centre:
                return ok[l].copy(), np.full((h, w), l)
            m = [ok[l] & inside & ok[k][qy, qx] & (key[k][qy, qx] == key[l]).all(axis=-1) for k in range(2)]
            return m[0] | m[1], np.where(m[0], 0, 1)

        # 2 the 3 x 3 prefilter of the measured variance
        g = (0.25, 0.5, 0.25)
        var = np.zeros((2, h, w))
        for l in range(2):
            sw, sv = np.zeros((h, w)), np.zeros((h, w))
            for j in range(3):
                for i in range(3):
                    inside, qy, qx = taps.at(i - 1, j - 1)
                    m, cl = candidate(l, i == 1 and j == 1, inside, qy, qx)
                    vq = vr[cl, qy, qx]
                    m = m & ~(vq < 0.0)
                    sw = sw + np.where(m, g[j] * g[i], 0.0)
                    sv = sv + np.where(m, (g[j] * g[i]) * vq, 0.0)
            var[l] = np.where(ok[l] & (sw > 0), sv / sw, 0.0)

        # 3 the levels of acn_denoise: both layers advance together
        for it in range(iterations):
            s = 1 << it
            c_new, var_new = c.copy(), var.copy()
            for l in range(2):
                lum = D.lum(c[l])
                den = sigma_lum * D.det(lib, D.OP_SQRT, var[l]) + 1e-8
                sw, sd, sv = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
                for tj in range(5):
                    for ti in range(5):
                        centre = tj == 2 and ti == 2
                        inside, qy, qx = taps.at((ti - 2) * s, (tj - 2) * s)
                        m, cl = candidate(l, centre, inside, qy, qx)
                        cross[l] += int((m & (cl != l)).sum())
                        cq, vq = c[cl, qy, qx], var[cl, qy, qx]
                        if centre:
                            wt = np.full((h, w), D.K[2] * D.K[2])
                        else:
                            wn = D.dot(N[l], N[cl, qy, qx])
                            wn = np.where(wn > 0, wn, 0.0)
                            for _ in range(npl):
                                wn = wn * wn
                            Dv = P[cl, qy, qx] - P[l]
                            ln = D.det(lib, D.OP_SQRT, D.dot(Dv, Dv))
                            tp = np.where(ln > 0, (np.abs(D.dot(N[l], Dv)) / ln) / sigma_plane, 0.0)
                            tl = np.abs(D.lum(cq) - lum) / den
                            wt = ((D.K[tj] * D.K[ti]) * wn) * D.det(lib, D.OP_EXP, -(tp + tl))
                        sw = sw + np.where(m, wt, 0.0)
                        sd = sd + np.where(m[..., None], wt[..., None] * (cq - c[l]), 0.0)
                        sv = sv + np.where(m, (wt * wt) * vq, 0.0)
                c_new[l] = np.where(ok[l][..., None], c[l] + sd / sw[..., None], c[l])
                var_new[l] = np.where(ok[l], sv / (sw * sw), var[l])
            c, var = c_new, var_new

        # 4 and the composite
        cnt = np.where(e, 0.0, stats[:, :, 0])
        kp = (cnt[0] + cnt[1]) + cnt[2]
        F = [np.where(ok[l].reshape(-1, 1), (c[l] * a[l]).reshape(-1, 3), stats[l][:, 1:4]) for l in range(2)] + [stats[2][:, 1:4]]
        out = np.tile(bg, (h * w, 1))
        have = np.zeros(h * w, bool)
        for l in range(STATS_PLANES):
            term = (cnt[l] / kp)[:, None] * F[l]
            present = ~e[l]
            out = np.where((present & have)[:, None], out + term, np.where(present[:, None], term, out))
            have = have | present
    if detail is not None:
        detail.update(ok=ok, cross=cross)
    return out.reshape(h, w, 3)


def synthetic_frame(w, h, K=8, seed=9):
    """A hand-made layered frame with everything the layered filter tells apart.  Two curved surfaces, objects 3 and 4, meet at a
    slanted edge; the pixels on the edge see both: the larger share is layer 0, the smaller layer 1, and the pixel next to it sees
    that smaller surface as ITS layer 0.  Some edge pixels lose a sample to a third class (the rest).  A block of emitter layers, a
    corner of sky (a miss as layer 0, and as layer 1 on its border), pixels whose three records are EMPTY, a pixel of one sample, a
    NaN mean.  -> stats [3,h*w,8], records [2,h*w,16]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    u, v = (x + 0.5) / max(w, h), (y + 0.5) / max(w, h)
    px, py = 4 * u - 2, 4 * v - 1
    colours = np.array([[0.8, 0.6, 0.3], [0.25, 0.5, 0.9]])

    def surface(obj):
        pos = np.stack([px, py, 0.6 * np.sin(1.5 * px + obj) + 0.15 * py * py + 0.2 * obj], axis=-1)
        nrm = np.stack([-0.9 * np.cos(1.5 * px + obj), -0.3 * py, np.ones_like(px)], axis=-1)
        nrm = nrm / np.sqrt((nrm * nrm).sum(axis=-1, keepdims=True))
        r = D.blank(h * w).reshape(h, w, D.STRIDE)
        r[..., 0] = np.sqrt((pos * pos).sum(axis=-1)) + 3
        r[..., 1:4] = pos; r[..., 4:7] = nrm
        r[..., 7] = 3 + obj; r[..., 8] = -1; r[..., 9:12] = colours[obj]; r[..., 12] = 2; r[..., 13] = 0; r[..., 14] = 1.0
        return r

    def stats_of(obj, m):
        shade = 0.4 + 0.3 * np.sin(5 * u) * np.cos(4 * v) + 0.25 * obj
        s = np.zeros((h, w, T.STRIDE))
        s[..., 0] = m
        s[..., 1:4] = colours[obj] * (shade[..., None] + rng.exponential(0.2, (h, w, 3)) / np.sqrt(np.maximum(m, 1))[..., None])
        s[..., 4:7] = np.where(m[..., None] > 1, rng.exponential(0.05, (h, w, 3)) * m[..., None], 0.0)
        s[m == 0] = 0.0
        return s

    # share of object 3 in a pixel: 1 on the left, 0 on the right, a band of two mixed pixels along x = edge( y )
    edge = w * 0.45 + 0.25 * y
    share = np.clip(edge - x + 1.0, 0.0, 2.0) / 2.0
    m3 = np.rint(share * K).astype(np.int64)
    third = ((x + 2 * y) % 5 == 0) & (m3 > 1) & (m3 < K - 1)                # one sample of a third class: the rest
    m4 = K - m3 - third
    rec_obj, st_obj = [surface(0), surface(1)], [stats_of(0, m3.astype(float)), stats_of(1, m4.astype(float))]
    first = np.where(m3 >= m4, 0, 1)                                          # the larger share is layer 0, object 3 on a tie
    rec = np.zeros((2, h, w, D.STRIDE)); st = np.zeros((3, h, w, T.STRIDE))
    for l in range(2):
        pick = first if l == 0 else 1 - first
        rec[l] = np.where((pick == 0)[..., None], rec_obj[0], rec_obj[1])
        st[l] = np.where((pick == 0)[..., None], st_obj[0], st_obj[1])
        rec[l][..., 15] = st[l][..., 0] / K
    absent = st[1][..., 0] == 0
    rec[1][absent] = R.miss_record(0, 0.0)
    st[2][third, 0] = 1.0
    st[2][third, 1:4] = rng.uniform(0.5, 3.0, (int(third.sum()), 3))
    # an emitter block: its layer 0 is an emitter, not filterable, copied
    emit = (x >= 3) & (x <= 6) & (y >= h // 2) & (y <= h // 2 + 3)
    rec[0][emit, 12] = 1 + 32
    st[0][emit, 1:4] = [25.0, 22.5, 20.0]
    # sky in the upper right corner: a miss as layer 0; on its border the surface is layer 0 and the miss layer 1
    sky = (x >= w - 6) & (y <= 4)
    border = (x == w - 7) & (y <= 4)
    miss = R.miss_record(0, 1.0)
    rec[0][sky] = miss; rec[0][sky, 15] = 1.0
    st[0][sky, 0] = K; st[0][sky, 1:4] = [0.3, 0.35, 0.4]; st[0][sky, 4:7] = 0.0
    rec[1][sky] = R.miss_record(0, 0.0); st[1][sky] = 0.0; st[2][sky] = 0.0
    rec[1][border] = miss; rec[1][border, 15] = 2.0 / K
    st[1][border] = 0.0; st[1][border, 0] = 2.0; st[1][border, 1:4] = [0.3, 0.35, 0.4]
    st[0][border, 0] = K - 2; rec[0][border, 15] = (K - 2.0) / K; st[2][border] = 0.0
    # pixels without a sample: three EMPTY records
    gone = ((x * 5 + y * 3) % 31 == 0) & ~sky & ~border & ~emit
    st[:, gone] = 0.0
    rec[0][gone] = R.miss_record(0, 0.0); rec[1][gone] = R.miss_record(0, 0.0)
    # a pixel of one sample (no variance of its own), and a NaN mean
    st[:, 5, 2] = 0.0; st[0, 5, 2] = st_obj[0][5, 2]; st[0, 5, 2, 0] = 1.0; st[0, 5, 2, 4:7] = 0.0
    rec[1][5, 2] = R.miss_record(0, 0.0); rec[0][5, 2, 15] = 1.0
    st[0, h - 2, 1, 2] = np.nan
    return st.reshape(3, h * w, T.STRIDE), rec.reshape(2, h * w, D.STRIDE)
