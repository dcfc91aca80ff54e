"""CPU models of the two shadow calls (acn_shadow_records, acn_shadow_limit_history; include/actinon_hip.h).

record_from_tap builds the record of one position from the oracle's tap acn_oracle_shade_point: the tap runs scene_s_lum for one hit
and records every direct-light sample -- its direction, its weight, the light's answer and the occlusion answer -- so nothing of the
sampling is restated here.  The hit's intensity is chosen so that ( uint64 )( direct_samples * diffuse_intensity ) is S for every
light; the helper asserts that it was.  limit_history restates the guard in numpy, expression by expression."""
import numpy as np

STRIDE = 16
EMITTER = 1
DEFAULT_TOLERANCE, DEFAULT_CAP = 0.25, 1.0
TAP_SURFACE, TAP_DIFFUSE, TAP_LIGHT, TAP_DIRECT = 1, 5, 6, 7
TAP_DEPTH = 25


def sampled(surface):
    """the SAMPLED rule on surface records [n,16]"""
    s = np.asarray(surface, dtype=np.float64).reshape(-1, 16)
    return (s[:, 0] < np.inf) & ((s[:, 12].astype(np.int64) & EMITTER) == 0)


def tap_hit(ray, r, intensity):
    """the hit acn_oracle_shade_point takes, of a ray [6] and its surface record r [16]"""
    return np.concatenate([ray[:6], [r[0]], r[4:7], [r[8], r[7], TAP_DEPTH, intensity]])


def tap_rows(orc, flat, ray, r, S):
    """The tap's rows of the hit at the intensity that gives S samples per light, or None where the hit has no diffuse block."""
    rows, _ = orc.shade_point(flat, tap_hit(ray, r, 1.0))
    dif = rows[rows[:, 0] == TAP_DIFFUSE]
    if len(dif) == 0:
        return None
    d1 = dif[0, 8]
    intensity = (S + 0.5) / (flat.params.direct_samples * d1)
    rows, _ = orc.shade_point(flat, tap_hit(ray, r, intensity))
    assert (rows[:, 0] == TAP_DIFFUSE).sum() == 1, "the diffuse block fell under trace_min_intensity"
    lights = rows[rows[:, 0] == TAP_LIGHT]
    assert len(lights) >= 1 and (lights[:, 6] == S).all(), (S, lights[:, 6])
    surf = rows[rows[:, 0] == TAP_SURFACE]
    assert len(surf) == 1 and np.array_equal(surf[0, 1:4], r[1:4]), "the tap's position is not the record's"
    assert np.array_equal(dif[0, 1:4], -r[4:7])
    return rows


def counts_of_rows(rows):
    """-> ( asked [L], clear [L] ) of the tap's rows: per LIGHT row, its DIRECT rows with [6] > 0 and [7] < inf, and those of them with
    [9] == 0"""
    asked, clear = [], []
    for row in rows:
        if row[0] == TAP_LIGHT:
            asked.append(0); clear.append(0)
        elif row[0] == TAP_DIRECT and row[6] > 0 and row[7] < np.inf:
            asked[-1] += 1
            if row[9] == 0:
                clear[-1] += 1
    return np.array(asked, dtype=np.int64), np.array(clear, dtype=np.int64)


def record_of_counts(S, asked, clear):
    rec = np.zeros(STRIDE)
    L = len(asked)
    rec[0], rec[1], rec[2] = 1.0, S, L
    rec[3], rec[4] = asked.sum(), clear.sum()
    rec[5] = rec[4] / rec[3] if rec[3] > 0 else 0.0
    k = min(L, 5)
    rec[6:6 + k] = clear[:k]
    rec[11:11 + k] = asked[:k]
    return rec


def record_from_tap(orc, flat, ray, surface_record, S):
    """The shadow record [16] of one SAMPLED surface record as the oracle's tap gives it, or None where the hit has no diffuse block
    (glass, mirror): the tap draws no direct-light samples there."""
    r = np.asarray(surface_record, dtype=np.float64)
    assert sampled(r)[0]
    rows = tap_rows(orc, flat, np.asarray(ray, dtype=np.float64), r, S)
    if rows is None:
        return None
    asked, clear = counts_of_rows(rows)
    assert len(asked) == flat.node(flat.c.light_root).child1
    return record_of_counts(S, asked, clear)


def records_from_tap(orc, flat, rays, surface, S):
    """-> ( records [n,16], compared [n] bool ): the tap's record of every SAMPLED row that has a diffuse block; the other rows are zeros"""
    surface = np.asarray(surface, dtype=np.float64).reshape(-1, 16)
    out = np.zeros((len(surface), STRIDE))
    compared = np.zeros(len(surface), bool)
    for i in np.flatnonzero(sampled(surface)):
        rec = record_from_tap(orc, flat, rays[i], surface[i], S)
        if rec is not None:
            out[i] = rec
            compared[i] = True
    return out, compared


def empty(n):
    """the EMPTY rule of a statistics record's [ 0 ]"""
    with np.errstate(invalid="ignore"):
        return ~((n >= 1.0) & (n < np.inf))


def limit_history(stats, motion, cur_shadow, prev_shadow, width, height, tolerance=None, changed_max_history=None, drop=False):
    """acn_shadow_limit_history in numpy -> ( stats [n,8] a limited copy, change [n] )"""
    t = np.array(stats, dtype=np.float64).reshape(-1, 8)
    m = np.asarray(motion, dtype=np.float64).reshape(-1, 2)
    c = np.asarray(cur_shadow, dtype=np.float64).reshape(-1, STRIDE)
    q = np.asarray(prev_shadow, dtype=np.float64).reshape(-1, STRIDE)
    assert len(q) == width * height and len(m) == len(t) and len(c) == len(t)
    tol = DEFAULT_TOLERANCE if not tolerance else float(tolerance)
    cap = DEFAULT_CAP if not changed_max_history else float(changed_max_history)
    n = len(t)
    change = np.full(n, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = ~empty(t[:, 0]) & ~np.isnan(m[:, 0]) & ~np.isnan(m[:, 1])
        x, y = np.floor(m[:, 0]), np.floor(m[:, 1])
        ok &= (x >= 0.0) & (x < float(width)) & (y >= 0.0) & (y < float(height))
        at = np.where(ok, y, 0.0).astype(np.int64) * int(width) + np.where(ok, x, 0.0).astype(np.int64)
        p = q[at]
        ok &= (c[:, 0] == 1.0) & (p[:, 0] == 1.0)
        mx = np.zeros(n)
        for l in range(5):
            term = np.abs(c[:, 6 + l] / c[:, 1] - p[:, 6 + l] / p[:, 1])
            mx = np.where((float(l) < c[:, 2]) & (term > mx), term, mx)
        term = np.abs(c[:, 4] / (c[:, 1] * c[:, 2]) - p[:, 4] / (p[:, 1] * p[:, 2]))
        mx = np.where(term > mx, term, mx)
        change[ok] = mx[ok]
        lim = ok & (mx > tol)
        if drop:
            t[lim] = 0.0
        else:
            lim &= t[:, 0] > cap
            f = cap / t[lim, 0]
            t[lim, 4] = t[lim, 4] * f; t[lim, 5] = t[lim, 5] * f; t[lim, 6] = t[lim, 6] * f
            t[lim, 0] = cap
    return t, change


# ---- hand-made arrays: every branch of the guard, with the answers written out ----
W_HAND, H_HAND = 4, 3


def shadow_rec(S, asked, clear, state=1.0):
    r = record_of_counts(S, np.array(asked, dtype=np.int64), np.array(clear, dtype=np.int64))
    r[0] = state
    if state != 1.0:
        r[1:] = 0.0
    return r


def hand_case():
    """-> dict( stats, motion, cur, prev, rows ): one row per case named in `rows`, a previous raster of 4 x 3.  Statistics records
    are { 8, mean ( 1, 2, 3 ), m2 ( 4, 5, 6 ), 0 } unless the case says otherwise; the previous raster is all `lit` (S 8, one light,
    8 asked, 8 clear) but for the pixels the cases name."""
    lit = shadow_rec(8, [8], [8])
    dark = shadow_rec(8, [8], [0])
    prev = np.tile(lit, (W_HAND * H_HAND, 1))
    prev[1 * W_HAND + 2] = shadow_rec(8, [8], [6])            # pixel ( 2, 1 ): 0.75 of the light
    prev[2 * W_HAND + 3] = shadow_rec(8, [0], [0], state=0.0)   # pixel ( 3, 2 ): NONE
    prev[2 * W_HAND + 0] = shadow_rec(16, [16] * 7, [16, 16, 16, 16, 16, 0, 0])   # pixel ( 0, 2 ): seven lights, the last two dark
    base = np.array([8.0, 1, 2, 3, 4, 5, 6, 0])
    rows, stats, motion, cur = [], [], [], []

    def add(name, st, mo, c):
        rows.append(name); stats.append(st); motion.append(mo); cur.append(c)

    add("empty stats", np.zeros(8), (1.5, 1.5), dark)
    add("n below 1 is empty", np.array([0.5, 1, 2, 3, 4, 5, 6, 0]), (1.5, 1.5), dark)
    add("nan motion x", base, (np.nan, 1.5), dark)
    add("nan motion y", base, (1.5, np.nan), dark)
    add("qx -0.0 is pixel 0", base, (-0.0, 0.5), dark)
    add("qx W is outside", base, (float(W_HAND), 0.5), dark)
    add("qx W - 2^-40 is the last pixel", base, (W_HAND - 2.0 ** -40, 0.5), dark)
    add("qx below 0", base, (-2.0 ** -40, 0.5), dark)
    add("qy H is outside", base, (0.5, float(H_HAND)), dark)
    add("current NONE", base, (1.5, 1.5), shadow_rec(8, [0], [0], state=0.0))
    add("previous NONE", base, (3.5, 2.5), dark)
    add("change equals the tolerance", base, (2.5, 1.5), shadow_rec(8, [8], [8]))      # 1.0 - 0.75
    add("change above the tolerance", base, (2.5, 1.5), shadow_rec(8, [8], [3]))       # 0.375
    add("n at the cap", np.array([1.0, 1, 2, 3, 4, 5, 6, 0]), (1.5, 1.5), dark)
    add("nothing changed", base, (1.5, 1.5), lit)
    add("seven lights: the sixth shows in the total only", base, (0.5, 2.5), shadow_rec(16, [16] * 7, [16] * 7))
    add("seven lights, unchanged", base, (0.5, 2.5), prev[2 * W_HAND + 0].copy())
    return dict(stats=np.array(stats), motion=np.array(motion, dtype=np.float64), cur=np.array(cur), prev=prev, rows=rows)


def hand_answers(drop=False, cap=None):
    """what the cases of hand_case give with the default tolerance 0.25 and the cap given (default 1), computed by hand -> ( stats, change )"""
    h = hand_case()
    nan = np.nan
    capv = 1.0 if cap is None else cap
    capped = np.array([capv, 1, 2, 3, 4 * (capv / 8.0), 5 * (capv / 8.0), 6 * (capv / 8.0), 0])
    limited = np.zeros(8) if drop else capped
    want = {
        "empty stats": (None, nan), "n below 1 is empty": (None, nan), "nan motion x": (None, nan), "nan motion y": (None, nan),
        "qx -0.0 is pixel 0": (limited, 1.0), "qx W is outside": (None, nan), "qx W - 2^-40 is the last pixel": (limited, 1.0),
        "qx below 0": (None, nan), "qy H is outside": (None, nan), "current NONE": (None, nan), "previous NONE": (None, nan),
        "change equals the tolerance": (None, 0.25), "change above the tolerance": (limited, 0.375),
        "n at the cap": (np.zeros(8) if drop else None, 1.0), "nothing changed": (None, 0.0),
        # lights 0 .. 4 are equal; the total: 7 * 16 / ( 16 * 7 ) - 5 * 16 / ( 16 * 7 ) = 1 - 80 / 112
        "seven lights: the sixth shows in the total only": (limited, abs(112.0 / (16.0 * 7.0) - 80.0 / (16.0 * 7.0))),
        "seven lights, unchanged": (None, 0.0),
    }
    stats = h["stats"].copy()
    change = np.zeros(len(stats))
    for i, name in enumerate(h["rows"]):
        rec, ch = want[name]
        if rec is not None:
            stats[i] = rec
        change[i] = ch
    return stats, change
