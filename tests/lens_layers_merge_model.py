"""numpy model of acn_lens_layers_merge* and acn_lens_layers_resolve_dev: the definitions of include/actinon_hip.h line by line, one
position at a time.  numpy's elementwise + - * / on float64 are IEEE binary64 and never contracted; the square root of the merged
normal and of the noise goes through the host build of csrc/acn_detmath.h (the `detmath_cpu` fixture of conftest.py), so the device
is compared with this model bit for bit (lens_layers_model.same_bits: which NaN a NaN is, the header leaves open)."""
import numpy as np

import lens_model as M
import lens_surface_model as R
import stats_model as T

SURF_PLANES, STATS_PLANES = 2, 3
MIXED = (0, 1, 2, 3, 9, 10, 11, 14)          # q = q_a + ( q_b - q_a ) * f


def empty1(rec):
    return not (rec[0] >= 1.0 and rec[0] < np.inf)


def absent_layer():
    return R.miss_record(0, 0.0), np.zeros(T.STRIDE)


def stats_pair(a, b):
    """merge( a, b ) of acn_lens_stats_merge, neither EMPTY"""
    na, nb = a[0], b[0]
    n = na + nb
    dl = b[1:4] - a[1:4]
    out = np.zeros(T.STRIDE)
    out[0] = n
    out[1:4] = a[1:4] + dl * (nb / n)
    out[4:7] = (a[4:7] + b[4:7]) + (dl * dl) * ((na * nb) / n)
    return out


def stats_fold(a, b):
    """... with its EMPTY rules: b EMPTY leaves a, an EMPTY a becomes b bit for bit"""
    if empty1(b):
        return a.copy()
    if empty1(a):
        return b.copy()
    return stats_pair(a, b)


def kind_bits(v):
    return int(np.int32(v)) & 0xFFFFFFFF


def surface_pair(lib, sa, sb, na, nb):
    """PAIR MERGE of two surface records of one key; [ 15 ] is a's here and is set by the coverage step"""
    f = nb / (na + nb)
    hit = bool(sa[0] < np.inf)
    out = np.zeros(R.STRIDE)
    out[14] = sa[14] + (sb[14] - sa[14]) * f
    out[13] = sa[13]
    out[15] = sa[15]
    if not hit:
        out[0] = np.inf
        out[7] = out[8] = -1.0
        return out
    for k in MIXED:
        out[k] = sa[k] + (sb[k] - sa[k]) * f
    g = sa[4:7] + (sb[4:7] - sa[4:7]) * f
    q = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    out[4:7] = g / M.sqrt(lib, q) if q > 0 else 0.0
    out[7], out[8] = sa[7], sa[8]
    out[12] = float(kind_bits(sa[12]) | kind_bits(sb[12]))
    return out


def merge_one(lib, a_surf, a_st, b_surf, b_st, detail=None):
    """the slots of one position: a_surf, b_surf [2,16], a_st, b_st [3,8] -> ( surf [2,16], st [3,8] ), or None: not written.
    detail (a dict) receives `demoted`: the keys of the entries whose statistics went to the rest"""
    with np.errstate(all="ignore"):
        if all(empty1(b_st[l]) for l in range(3)):
            return None
        entries = []                                                          # [ key, surface, statistics ] in the order of the list
        for l in range(2):
            if not empty1(a_st[l]):
                entries.append([R.sample_class(a_surf[l]), a_surf[l].copy(), a_st[l].copy()])
        for l in range(2):
            if empty1(b_st[l]):
                continue
            key = R.sample_class(b_surf[l])
            for e in entries:
                if e[0] == key:                                               # the first such entry
                    e[1] = surface_pair(lib, e[1], b_surf[l], e[2][0], b_st[l][0])
                    e[2] = stats_pair(e[2], b_st[l])
                    break
            else:
                entries.append([key, b_surf[l].copy(), b_st[l].copy()])
        # the ranking: descending n, the earlier entry among equals (sorted is stable)
        ranked = sorted(entries, key=lambda e: -e[2][0])
        surf, st = np.zeros((2, R.STRIDE)), np.zeros((3, T.STRIDE))
        for l in range(2):
            surf[l], st[l] = (ranked[l][1], ranked[l][2]) if l < len(ranked) else absent_layer()
        rest = stats_fold(a_st[2], b_st[2])
        for e in ranked[2:]:
            rest = stats_fold(rest, e[2])
        st[2] = np.zeros(T.STRIDE) if empty1(rest) else rest
        cnt = [0.0 if empty1(st[l]) else st[l][0] for l in range(3)]
        kp = (cnt[0] + cnt[1]) + cnt[2]
        for l in range(min(2, len(ranked))):
            surf[l][15] = st[l][0] / kp
        if detail is not None:
            detail["demoted"] = [e[0] for e in ranked[2:]]
    return surf, st


def merge(lib, acc_surf, acc_st, part_surf, part_st, index=None, detail=None):
    """-> copies of the accumulator's planes [2,n_acc,16], [3,n_acc,8] with position j of the part merged into position index[ j ]
    (index None: j); indices out of range are skipped.  detail (a dict) receives `demoted`: per accumulator position how many
    entries this merge sent to the rest"""
    acc_surf, acc_st = np.array(acc_surf, dtype=np.float64), np.array(acc_st, dtype=np.float64)
    part_surf, part_st = np.asarray(part_surf, dtype=np.float64), np.asarray(part_st, dtype=np.float64)
    n_acc, n_part = acc_st.shape[1], part_st.shape[1]
    assert acc_surf.shape == (2, n_acc, R.STRIDE) and acc_st.shape == (3, n_acc, T.STRIDE), (acc_surf.shape, acc_st.shape)
    assert part_surf.shape == (2, n_part, R.STRIDE) and part_st.shape == (3, n_part, T.STRIDE), (part_surf.shape, part_st.shape)
    idx = np.arange(n_part) if index is None else np.asarray(index, dtype=np.int64)
    demoted = np.zeros(n_acc, dtype=np.int64)
    for j in range(n_part):
        i = int(idx[j])
        if i < 0 or i >= n_acc:
            continue
        d = {}
        got = merge_one(lib, acc_surf[:, i], acc_st[:, i], part_surf[:, j], part_st[:, j], detail=d)
        if got is None:
            continue
        acc_surf[:, i], acc_st[:, i] = got
        demoted[i] = len(d["demoted"])
    if detail is not None:
        detail["demoted"] = demoted
    return acc_surf, acc_st


def pooled(st):
    """st [3,n,8] -> [n,8]: merge( merge( s0, s1 ), sr ); eight zeros where that is EMPTY"""
    st = np.asarray(st, dtype=np.float64)
    out = np.zeros((st.shape[1], T.STRIDE))
    with np.errstate(all="ignore"):
        for i in range(st.shape[1]):
            p = stats_fold(stats_fold(st[0, i], st[1, i]), st[2, i])
            out[i] = 0.0 if empty1(p) else p
    return out


def layers_resolve(lib, st, background, gamma, linear):
    """-> ( rgb [n,3], noise [n], pooled [n,8] )"""
    p = pooled(st)
    rgb, noise = T.resolve(lib, p, background, gamma, linear)
    return rgb, noise, p


# ---- hand-made positions: every rule of the definition on slots whose answer is known without the model ----

A_, B_, C_, D_ = ("hit", 5, -1, 0), ("hit", 7, 2, 1), ("hit", -1, 5, 1), ("hit", 9, -1, 2)
SKY, SKY2 = ("miss", 0), ("miss", 2)


def key_of(cls):
    """the ( hit, e, x, h ) a slot of class cls has"""
    return (True,) + tuple(cls[1:]) if cls[0] == "hit" else (False, -1, -1, cls[1])


def slot(rng, cls, n, kind=2):
    """a layer slot of class cls with n samples: ( surface record, statistics record ); cls None: the absent layer"""
    if cls is None:
        return absent_layer()
    s = R.varied(rng, *cls[1:], kind=kind) if cls[0] == "hit" else R.miss_record(cls[1], rng.uniform(0.1, 1.0))
    s[15] = rng.uniform(0.1, 1.0)                                             # (whatever it was: the merge sets it)
    t = np.zeros(T.STRIDE)
    t[0] = float(n)
    t[1:4] = rng.uniform(0.0, 2.0, 3)
    t[4:7] = rng.uniform(0.0, 1.0, 3) * (n - 1)
    return s, t


def rest_slot(rng, n):
    if not n:
        return np.zeros(T.STRIDE)
    return slot(rng, A_, n)[1]


# name: ( A0, A1, nAr, B0, B1, nBr, layers ): a slot is ( class, n ) or None; layers: the ( class, n ) of layer 0 and layer 1 of the
# result, None for an absent one, or "unwritten".  n of the rest follows from conservation
PATTERNS = {
    # presence: what a split can produce on either side
    "empty acc, L0": (None, None, 0, (A_, 4), None, 0, [(A_, 4), None]),
    "empty acc, L0 L1": (None, None, 0, (A_, 3), (B_, 1), 0, [(A_, 3), (B_, 1)]),
    "empty acc, L0 L1 r": (None, None, 0, (A_, 5), (B_, 2), 1, [(A_, 5), (B_, 2)]),
    "L0, part empty": ((A_, 4), None, 0, None, None, 0, "unwritten"),
    "L0 L1 r, part empty": ((A_, 4), (B_, 3), 1, None, None, 0, "unwritten"),
    "L0, L0 same": ((A_, 4), None, 0, (A_, 4), None, 0, [(A_, 8), None]),
    "L0, L0 other": ((A_, 4), None, 0, (B_, 3), None, 0, [(A_, 4), (B_, 3)]),
    "L0, L0 L1 r": ((A_, 4), None, 0, (A_, 2), (B_, 1), 1, [(A_, 6), (B_, 1)]),
    "L0 L1, L0": ((A_, 3), (B_, 1), 0, (B_, 4), None, 0, [(B_, 5), (A_, 3)]),
    "L0 L1 r, L0 L1 r": ((A_, 5), (B_, 2), 1, (A_, 4), (B_, 3), 1, [(A_, 9), (B_, 5)]),
    "L0 L1 r, L0": ((A_, 5), (B_, 2), 1, (C_, 8), None, 0, [(C_, 8), (A_, 5)]),
    # keys
    "B0 = A0": ((A_, 4), (B_, 2), 0, (A_, 3), (C_, 1), 0, [(A_, 7), (B_, 2)]),
    "B0 = A1": ((A_, 4), (B_, 2), 0, (B_, 3), (C_, 1), 0, [(B_, 5), (A_, 4)]),
    "B1 = A0": ((A_, 4), (B_, 2), 0, (C_, 3), (A_, 1), 0, [(A_, 5), (C_, 3)]),
    "B1 = A1": ((A_, 4), (B_, 2), 0, (C_, 3), (B_, 2), 0, [(A_, 4), (B_, 4)]),
    "crossed": ((A_, 4), (B_, 3), 1, (B_, 5), (A_, 2), 1, [(B_, 8), (A_, 6)]),
    "straight": ((A_, 4), (B_, 3), 0, (A_, 5), (B_, 2), 0, [(A_, 9), (B_, 5)]),
    "four classes": ((A_, 5), (B_, 2), 1, (C_, 4), (D_, 3), 1, [(A_, 5), (C_, 4)]),
    "four classes, the part leads": ((A_, 2), (B_, 1), 0, (C_, 6), (D_, 3), 0, [(C_, 6), (D_, 3)]),
    # ties, decided by the order of the list
    "tie at rank 1 / 2": ((A_, 4), (B_, 2), 0, (B_, 2), None, 0, [(A_, 4), (B_, 4)]),
    "tie at rank 1 / 2, the part first in n": ((A_, 3), None, 0, (B_, 3), None, 0, [(A_, 3), (B_, 3)]),
    "tie at rank 2 / 3": ((A_, 4), (B_, 2), 0, (C_, 2), None, 0, [(A_, 4), (B_, 2)]),
    "tie at rank 2 / 3 / 4": ((A_, 4), (B_, 2), 0, (C_, 2), (D_, 2), 0, [(A_, 4), (B_, 2)]),
    "all four equal": ((A_, 2), (B_, 2), 0, (C_, 2), (D_, 2), 0, [(A_, 2), (B_, 2)]),
    # a merge after which the layers swap
    "swap": ((A_, 4), (B_, 3), 0, (B_, 2), None, 0, [(B_, 5), (A_, 4)]),
    # a miss class as a layer on either side
    "miss both sides, layer 0": ((SKY, 4), (A_, 2), 0, (SKY, 3), (A_, 1), 0, [(SKY, 7), (A_, 3)]),
    "miss in the part alone": ((A_, 4), None, 0, (A_, 3), (SKY, 1), 0, [(A_, 7), (SKY, 1)]),
    "two miss classes": ((SKY, 3), (SKY2, 2), 0, (SKY2, 4), (SKY, 1), 0, [(SKY2, 6), (SKY, 4)]),
    "miss A1 = miss B0": ((A_, 4), (SKY, 2), 1, (SKY, 3), None, 0, [(SKY, 5), (A_, 4)]),
}


def hand_made(seed=5):
    """-> ( names, a_surf [2,P,16], a_st [3,P,8], b_surf [2,P,16], b_st [3,P,8], want ): position p is pattern names[ p ]; want[ p ]
    is "unwritten" or [ ( key, n ) or None ] * 2 and the n of the rest.  Further positions follow the patterns: an accumulator whose
    EMPTY records are not zeros, statistics [ 0 ] of NaN, inf and 0.5, and kind bits that differ"""
    rng = np.random.default_rng(seed)
    names, rows, want = [], [], []

    def add(name, a0, a1, ar, b0, b1, br, layers):
        names.append(name); rows.append((a0, a1, ar, b0, b1, br))
        if layers == "unwritten":
            want.append(layers)
            return
        total = sum(float(s[1][0]) for s in (a0, a1, b0, b1) if not empty1(s[1])) + sum(float(r[0]) for r in (ar, br) if not empty1(r))
        got = [None if l is None else (key_of(l[0]), float(l[1])) for l in layers]
        want.append((got, total - sum(l[1] for l in got if l is not None)))

    for name, (a0, a1, nar, b0, b1, nbr, layers) in PATTERNS.items():
        mk = lambda s: slot(rng, s[0], s[1]) if s is not None else slot(rng, None, 0)
        add(name, mk(a0), mk(a1), rest_slot(rng, nar), mk(b0), mk(b1), rest_slot(rng, nbr), layers)
    # EMPTY records that are not zeros: [ 0 ] of 0.5, NaN, inf, a negative count; the slot is not PRESENT whatever its surface record says
    for bad in (0.5, np.nan, np.inf, -3.0):
        junk = lambda cls: (slot(rng, cls, 3)[0], np.concatenate([[bad], rng.uniform(0, 1, 7)]))
        add(f"acc EMPTY by {bad}", junk(A_), junk(B_), np.concatenate([[bad], rng.uniform(0, 1, 7)]), slot(rng, A_, 3), slot(rng, C_, 2), rest_slot(rng, 1),
            [(A_, 3), (C_, 2)])
        add(f"part layer 1 EMPTY by {bad}", slot(rng, A_, 4), slot(rng, B_, 1), rest_slot(rng, 0), slot(rng, A_, 2), junk(B_), rest_slot(rng, 0),
            [(A_, 6), (B_, 1)])
        add(f"part EMPTY by {bad}", slot(rng, A_, 4), slot(rng, B_, 1), rest_slot(rng, 2), junk(A_), junk(B_), np.concatenate([[bad], rng.uniform(0, 1, 7)]),
            "unwritten")
    # kind bits are ORed, normals that cancel give a zero normal
    a, b = slot(rng, A_, 2, kind=2 | 64), slot(rng, A_, 2, kind=8 | 16)
    add("kind bits", a, slot(rng, None, 0), rest_slot(rng, 0), b, slot(rng, None, 0), rest_slot(rng, 0), [(A_, 4), None])
    a, b = slot(rng, B_, 3), slot(rng, B_, 3)
    a[0][4:7] = (0.0, 0.6, 0.8); b[0][4:7] = (0.0, -0.6, -0.8)
    add("normals cancel", a, slot(rng, None, 0), rest_slot(rng, 0), b, slot(rng, None, 0), rest_slot(rng, 0), [(B_, 6), None])
    a_surf = np.stack([np.stack([r[l][0] for r in rows]) for l in range(2)])
    b_surf = np.stack([np.stack([r[3 + l][0] for r in rows]) for l in range(2)])
    a_st = np.stack([np.stack([r[0][1] for r in rows]), np.stack([r[1][1] for r in rows]), np.stack([r[2] for r in rows])])
    b_st = np.stack([np.stack([r[3][1] for r in rows]), np.stack([r[4][1] for r in rows]), np.stack([r[5] for r in rows])])
    return names, a_surf, a_st, b_surf, b_st, want


def tiled(n, seed=5):
    """the hand-made positions repeated to n positions: position i is pattern i % P -> ( a_surf, a_st, b_surf, b_st ), [.,n,.]"""
    _, a_surf, a_st, b_surf, b_st, _ = hand_made(seed)
    pick = np.arange(n) % a_st.shape[1]
    return a_surf[:, pick].copy(), a_st[:, pick].copy(), b_surf[:, pick].copy(), b_st[:, pick].copy()
