"""numpy model of the aggregate surface record (acn_surface_reduce, acn_surface_lens): the definition of include/actinon_hip.h line by
line, one position at a time.  numpy's elementwise + * / on float64 are IEEE binary64 and never contracted; the one square root goes
through the host build of csrc/acn_detmath.h (the `detmath_cpu` fixture of conftest.py), so the device is compared with this model
bit for bit."""
import numpy as np

import lens_model as M

STRIDE = 16
MEANS = (0, 1, 2, 3, 9, 10, 11, 14)          # distance, position, albedo, weight: ordered means as they are


def sample_class(r):
    """( hit, e, x, h ) of one record: hit = r[ 0 ] < inf; r[ 7 ], r[ 8 ], r[ 13 ] converted to int32"""
    return (bool(r[0] < np.inf), int(np.int32(r[7])), int(np.int32(r[8])), int(np.int32(r[13])))


def classes(records):
    """records [K,16] of one position -> the classes in the order of their first member: [ ( class, [ k_1 < k_2 < ... ] ) ]"""
    order, members = [], {}
    for k, r in enumerate(records):
        c = sample_class(r)
        if c not in members:
            members[c] = []
            order.append(c)
        members[c].append(k)
    return [(c, members[c]) for c in order]


def dominant(records):
    """the class with the most members; among those with equally many the one whose first member has the smallest k"""
    best = None
    for c, ks in classes(records):                # in the order of the first member: only a strictly larger class takes over
        if best is None or len(ks) > len(best[1]):
            best = (c, ks)
    return best


def ordered_mean(q):
    """q [m, ...] -> s = q[ 0 ]; s = s + q[ 1 ]; ...; s / ( double )m"""
    s = q[0].copy()
    for v in q[1:]:
        s = s + v
    return s / np.float64(len(q))


def reduce_one(lib, records):
    records = np.asarray(records, dtype=np.float64)
    K = len(records)
    (hit, e, x, h), ks = dominant(records)
    mem = records[ks]
    m = len(ks)
    out = np.zeros(STRIDE)
    out[13] = float(h)
    out[14] = ordered_mean(mem[:, 14])
    out[15] = np.float64(m) / np.float64(K)
    if not hit:
        out[0] = np.inf
        out[7] = out[8] = -1.0
        return out
    for f in MEANS:
        out[f] = ordered_mean(mem[:, f])
    if m == 1:
        out[4:7] = mem[0, 4:7]
    else:
        g = ordered_mean(mem[:, 4:7])
        q = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        out[4:7] = g / M.sqrt(lib, q) if q > 0 else 0.0
    out[7], out[8] = float(e), float(x)
    kinds = 0
    for v in mem[:, 12]:
        kinds |= int(np.uint32(v))
    out[12] = float(kinds)
    return out


def reduce(lib, records):
    """records [n,K,16] -> [n,16]"""
    records = np.asarray(records, dtype=np.float64)
    assert records.ndim == 3 and records.shape[2] == STRIDE and records.shape[1] >= 1, records.shape
    return np.array([reduce_one(lib, r) for r in records]).reshape(len(records), STRIDE)


def census(records):
    """per position of records [n,K,16]: the number of classes, whether two classes share the largest size, whether the dominant
    class is a miss, and the coverage"""
    n_cls, tie, miss, cov = [], [], [], []
    for r in records:
        cl = classes(r)
        sizes = sorted((len(ks) for _, ks in cl), reverse=True)
        (hit, _, _, _), ks = dominant(r)
        n_cls.append(len(cl)); tie.append(len(sizes) > 1 and sizes[0] == sizes[1]); miss.append(not hit); cov.append(len(ks) / len(r))
    return np.array(n_cls), np.array(tie), np.array(miss), np.array(cov)


# ---- hand-made records: every rule of the definition on inputs whose answer is known without the model ----

def hit_record(dist, e, x, h, pos=(1.0, 2.0, 3.0), nor=(0.0, 0.0, 1.0), alb=(0.5, 0.25, 0.125), kind=2, weight=1.0):
    r = np.zeros(STRIDE)
    r[0] = dist; r[1:4] = pos; r[4:7] = nor; r[7] = e; r[8] = x; r[9:12] = alb; r[12] = kind; r[13] = h; r[14] = weight
    return r


def miss_record(h=0, weight=1.0):
    r = np.zeros(STRIDE)
    r[0] = np.inf; r[7] = r[8] = -1.0; r[13] = h; r[14] = weight
    return r


def varied(rng, e, x, h, kind=2):
    """a hit of class ( e, x, h ) whose other members are random: no two sums agree by accident"""
    nor = rng.normal(size=3); nor /= np.sqrt(nor @ nor)
    return hit_record(rng.uniform(1, 20), e, x, h, pos=rng.uniform(-5, 5, 3), nor=nor, alb=rng.uniform(0, 1, 3), kind=kind,
                      weight=rng.uniform(0.1, 1.0))


def hand_made():
    """{ name: ( records [n,K,16], what the dominant class must be per position as ( class, m ) or None ) }"""
    rng = np.random.default_rng(7)
    A_, B_, C_ = (5, -1, 0), (7, -1, 0), (-1, 5, 1)
    cases = {}
    cases["one class"] = (np.array([[varied(rng, *A_) for _ in range(5)]]), [((True,) + A_, 5)])
    cases["tie of two, both orders"] = (np.array([[varied(rng, *A_), varied(rng, *B_)], [varied(rng, *B_), varied(rng, *A_)]]),
                                        [((True,) + A_, 1), ((True,) + B_, 1)])
    cases["tie among three"] = (np.array([[varied(rng, *c) for c in (C_, A_, B_, B_, C_, A_)]]), [((True,) + C_, 2)])
    # misses after 0 hops and after 2 hops are two classes; the larger one wins over the hit too
    cases["dominant miss"] = (np.array([[miss_record(0, 1.0), miss_record(2, 0.25), varied(rng, *A_), miss_record(2, 0.5), miss_record(2, 0.125)]]),
                              [((False, -1, -1, 2), 3)])
    single = varied(rng, *A_)
    single[1] = -0.0; single[5] = -0.0; single[9] = -0.0
    cases["m == 1 keeps -0.0"] = (np.array([[single]]), [((True,) + A_, 1)])
    cases["normals cancel"] = (np.array([[hit_record(3.0, *A_, nor=(0.0, 0.6, 0.8)), hit_record(4.0, *A_, nor=(0.0, -0.6, -0.8))]]), [((True,) + A_, 2)])
    cases["kind bits differ"] = (np.array([[varied(rng, *A_, kind=2), varied(rng, *A_, kind=2 | 64), varied(rng, *A_, kind=8 | 16), varied(rng, *B_, kind=1)]]),
                                 [((True,) + A_, 3)])
    # K = 33: 9, 17 and 33 distinct classes; the winner is a late class (it first appears after more than 8 others), and with K
    # distinct classes the first sample wins
    def many(n_cls, winner):
        ids = list(range(n_cls)) + [winner] * (33 - n_cls)
        return [varied(rng, 100 + i, -1, 0) for i in ids]
    cases["9 / 17 / K classes at K = 33"] = (np.array([many(9, 8), many(17, 16), many(17, 3), many(33, 0)]),
                                            [((True, 108, -1, 0), 25), ((True, 116, -1, 0), 17), ((True, 103, -1, 0), 17), ((True, 100, -1, 0), 1)])
    cases["K = 4096 of one class"] = (np.array([[varied(rng, *A_) for _ in range(4096)], [varied(rng, *B_) for _ in range(4096)]]),
                                      [((True,) + A_, 4096), ((True,) + B_, 4096)])
    return cases


def edge_positions(frame_records, width, height, want=64):
    """The positions the tests take from a frame: the pixels whose class differs from the right or the lower neighbour, in row-major
    order every ( count // want )-th of them, the first `want` of those -> ( pixel indices, how many edge pixels the frame has )"""
    r = np.asarray(frame_records).reshape(height, width, STRIDE)
    key = np.stack([(r[..., 0] < np.inf).astype(np.int64), r[..., 7].astype(np.int64), r[..., 8].astype(np.int64), r[..., 13].astype(np.int64)], axis=-1)
    edge = np.zeros((height, width), bool)
    edge[:, :-1] |= (key[:, :-1] != key[:, 1:]).any(axis=-1)
    edge[:-1, :] |= (key[:-1, :] != key[1:, :]).any(axis=-1)
    idx = np.flatnonzero(edge.reshape(-1))
    return idx[:: max(1, len(idx) // want)][:want], len(idx)
