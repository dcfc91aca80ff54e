"""The sample loops of k_shade on hand-made queues (the stage seam of tests/test_gpu_stages.py): what the wide classes read once per
light and once per wave -- the light's constants in the task frame, the root positions a wave still visits, the two LCG states of a
lane, the quadrant of the cap sample's sine by selects (profiles/r22/NOTES.md says which of them the kernel kept) -- against three
references at once:

  the tap      every record is a sample of the oracle's scene_lum at that point, field for field (check_records: the record half of
               test_gpu_stages.check_against_tap, whose rule that few samples be decided in line these queues break on purpose)
  the classes  the three output queues are the same sorted byte strings on 64, 16, 4 and 1 lanes per task, with and without the
               prune programs and with the lights forced through the generic hit: the narrow classes and the PRUNE variants keep the
               root's plain loop and the cap sample's switch
  the sums     accum equals, to the last bit, the tap's terms added as the kernel adds them: per lane in the order of j, lane
               ( j - j_lo ) % LPT, then the xor butterfly of group_sum, then norm, colour, Tc and to_fixed (exact_accum below)"""
import ctypes as C

import numpy as np
import pytest

import actinon_amd as A
from actinon_amd._lib import host
import ray_sets as R
import shade_model as M
import test_gpu_stages as G

pytestmark = pytest.mark.gpu

REC = A.Handle.STAGE_RECORDS
LANES = (64, 16, 4, 1)                     # lanes per task of size class 0 .. 3
QUEUES = ("children", "hard_path", "hard_shadow")
LIGHT_AT, LIGHT_R = (0.5, -0.5, 5.0), 0.5
GLASS_AT, GLASS_ENV = (0.5, -0.5, 2.5), 0.6
LIFT = 1.0e-6                              # shading points lie this far above the floor, as the hits of a walk do: the floor is culled


def _ball(r, at, material=b"diffuse"):
    o = host.acn_obj_sphere_s_create(float(r))
    host.acn_obj_set_material(o, material)
    host.acn_obj_move(o, A.v3(*at))
    return o


def _light(kind):
    if kind in ("sphere", "sphere_env"):
        o = host.acn_obj_sphere_s_create(LIGHT_R)
        host.acn_obj_set_color(o, A.v3(1.0, 0.9, 0.7))
        host.acn_obj_set_radiance(o, 40.0)
        host.acn_obj_move(o, A.v3(*LIGHT_AT))
        if kind == "sphere_env":
            host.acn_obj_set_envelope(o, A.v3(LIGHT_AT[0] + 0.05, LIGHT_AT[1], LIGHT_AT[2]), 0.6)
        return o
    if kind == "plane":
        o = host.acn_obj_plane_s_create()
        m = host.acn_rotx(180.0)
        host.acn_obj_rotate(o, C.byref(m))                     # faces down
        host.acn_obj_set_color(o, A.v3(0.9, 1.0, 0.8))
        host.acn_obj_set_radiance(o, 300.0)
        host.acn_obj_move(o, A.v3(0.0, 0.0, 9.0))
        return o
    assert kind == "pair"                                      # no leaf: the handle runs k_shade< LEAF_LIGHTS = false >
    o = R._pair_inside(host.acn_obj_sphere_s_create(0.6), host.acn_obj_plane_s_create())
    host.acn_obj_set_color(o, A.v3(1.0, 0.8, 0.8))
    host.acn_obj_set_radiance(o, 30.0)
    host.acn_obj_move(o, A.v3(-2.0, 1.0, 4.0))
    host.acn_obj_set_envelope(o, A.v3(-2.0, 1.0, 4.0), 0.65)
    return o


def _glass():
    """a torus under the sphere light: a distance object, so a shadow ray that hits its envelope is left to k_hard_shadow"""
    t = host.acn_obj_torus_create(0.35, 0.1)
    host.acn_obj_set_material(t, b"diffuse")
    host.acn_obj_move(t, A.v3(*GLASS_AT))
    host.acn_obj_set_envelope(t, A.v3(*GLASS_AT), GLASS_ENV)
    return t


def build(lights, matter, direct_samples=200, path_samples=200, **params):
    """floor first, then `matter` ("glass", or ( radius, centre ) spheres) in the given order"""
    sc = A.Scene()
    sc.set(image_width=16, image_height=16, gamma=1.0, trace_depth=22, trace_min_intensity=0.002, direct_samples=direct_samples,
           path_samples=path_samples, max_path_length=30.0, camera_position=(0, -8, 3), camera_view_direction=(0, 8, -2.6),
           camera_top_direction=(0, 0, 1), camera_focal_length=3, background_color=(0.3, 0.35, 0.4))
    sc.set(**params)
    for kind in lights:
        o = _light(kind)
        sc.push(o)
        host.acn_obj_discard(o)
    o = host.acn_obj_plane_s_create()
    host.acn_obj_set_material(o, b"diffuse")
    host.acn_obj_set_color(o, A.v3(0.8, 0.7, 0.6))
    sc.push(o)
    host.acn_obj_discard(o)
    for m in matter:
        o = _glass() if m == "glass" else _ball(*m)
        sc.push(o)
        host.acn_obj_discard(o)
    return sc


class Queue:
    """a scene, its handle and a hand-made DTask queue with the tap's rows: what check_against_tap calls `sm` and `sm.st`"""

    def __init__(self, oracle, detmath, sc, points, seed=5):
        self.sc, self.flat = sc, sc.flatten()
        self.prm, self.oracle, self.detmath = self.flat.params, oracle, detmath
        self.h = A.Handle(self.flat, device=0)
        self.info = self.h.stage_info()
        self.st, self.expect = self, {}
        rng = np.random.default_rng(seed)
        floor = self.flat.elems_of(self.flat.c.matter_root)[0]
        hits = []
        for pos, n, depth in points:
            d = (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -1.0)
            hits.append(R._sample_point(REC["hit"], self.prm, floor, pos, (0, 0, 1), d, n, depth, rng.uniform(0.3, 1.0, 3)))
        self.hits = np.array(hits, dtype=REC["hit"])
        self.hits["pixel"] = np.arange(len(hits))
        self.labels = np.array(["p%d" % k for k in range(len(hits))], dtype=object)
        self.rows = [oracle.shade_point(self.flat, M.tap_input(r))[0] for r in self.hits]
        self.tasks = np.array([M.task_of(rw, r, REC) for r, rw in zip(self.hits, self.rows)], dtype=REC["task"])
        self.counts = [M.sample_counts(rw) for rw in self.rows]

    def run(self, **kw):
        return self.h.run_stage("shade", self.tasks, **kw)

    def close(self):
        self.h.close()


def cull_masks(q, light=0):
    """root_cone_cull of every task for light `light` of the light root, through the query seam: bit i, root position i is skipped"""
    node = q.flat.elems_of(q.flat.c.light_root)[light]
    rays = np.concatenate([q.tasks["pos"], np.tile([0.0, 0.0, 1.0], (len(q.tasks), 1))], axis=1)
    out = q.h.query_rays("cone_cull", node, rays)
    return [int(v) for v in np.ascontiguousarray(out[:, 0]).view(np.uint64)]


def butterfly(v):
    """group_sum: v += shfl_xor( v, off ) for off = LPT / 2 .. 1; every lane ends with the same sum (an IEEE add commutes)"""
    v, off = list(v), len(v) // 2
    while off:
        v = [v[i] + v[i ^ off] for i in range(len(v))]
        off //= 2
    return v[0]


def exact_accum(q, out, lpt, shard=(0, 1)):
    """accum of every task as k_shade< lpt > adds it up.  The terms are the tap's (local intensity, weights, child intensities: what
    check_against_tap compares bit for bit where a record carries them); which samples were left to the hard-ray kernels is read off
    the records, which check_against_tap has matched to samples one for one."""
    prm, n = q.prm, len(q.tasks)
    bg = np.array(list(prm.background_color))
    max_len = prm.max_path_length
    ch, hp, hs = G.by_pixel(out["children"], n), G.by_pixel(out["hard_path"], n), G.by_pixel(out["hard_shadow"], n)
    want = np.zeros((n, 3), dtype=np.int64)
    key = lambda d: G.bits(d).tobytes()                                            # noqa: E731
    for i, (t, rows) in enumerate(zip(q.tasks, q.rows)):
        lights, direct, path = M.rows_of(rows, "light"), M.rows_of(rows, "direct"), M.rows_of(rows, "path")
        hs_of = G.group(hs[i], "d")
        lum = np.zeros(3)
        for li in lights:
            nd, node = int(li[6]), q.flat.node(int(li[1]))
            lp = np.array(list(node.pos))
            lo, hi = M.shard_range(nd, *shard)
            norm = 2.0 * li[2] / nd
            rs = direct[(direct[:, 2] == li[1]) & (direct[:, 1] >= lo) & (direct[:, 1] < hi)]
            rs = rs[np.argsort(rs[:, 1], kind="stable")]
            live = rs[(rs[:, 6] > 0) & (rs[:, 7] < np.inf)]
            w = M.closed_weight(q.detmath, live[:, 6], t["theta_i"], t["on_a"], t["on_b"], live[:, 3:6], t["surface_d"], t["ray_projection"])
            part = [0.0] * lpt
            for r, wc in zip(live, w):
                if G.take(hs_of, key(r[3:6])) is not None or r[9] != 0:
                    continue
                dv = (t["pos"] + r[3:6] * r[7]) - lp
                dsq = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]
                local = node.radiance / dsq if dsq > 0 else 1e30
                part[(int(r[1]) - lo) % lpt] += local * wc * t["diffuse_intensity"]
            lum = lum + li[3:6] * (butterfly(part) * norm)
        n_path = q.counts[i][1]
        if n_path:
            lo, hi = M.shard_range(n_path, *shard)
            rs = path[(path[:, 1] >= lo) & (path[:, 1] < hi)]
            rs = rs[np.argsort(rs[:, 1], kind="stable")]
            ch_of, hp_of = G.group(ch[i], "d"), G.group(hp[i], "d")
            part = [0.0] * lpt
            for r in rs:
                k = key(r[2:5])
                if not r[5] > 0 or G.take(ch_of, k) is not None or G.take(hp_of, k) is not None or G.take(hs_of, k) is not None:
                    continue
                if not r[7] < max_len:
                    part[(int(r[1]) - lo) % lpt] += r[13]
            lum = lum + bg * (butterfly(part) * (2.0 / n_path))
        want[i] = M.to_fixed(t["Tc"] * lum)
    return want


def check_records(q, out, shard=(0, 1)):
    """Every record of every task against the tap's row of the same sample (matched through the bits of out_d), every record a sample
    of this rank's share.  Returns the counts compared; "inline" counts the direct samples only the sums show."""
    prm, n = q.prm, len(q.tasks)
    bg = np.array(list(prm.background_color))
    tmin, max_len = prm.trace_min_intensity, prm.max_path_length
    path_limit = np.nextafter(max_len, 0.0)
    ch, hp, hs = G.by_pixel(out["children"], n), G.by_pixel(out["hard_path"], n), G.by_pixel(out["hard_shadow"], n)
    tally = {"children": 0, "hard_path": 0, "hard_shadow": 0, "probes": 0, "inline": 0, "background": 0}
    key = lambda d: G.bits(d).tobytes()                                            # noqa: E731
    same = lambda a, b: np.array_equal(G.bits(a), G.bits(b))                       # noqa: E731
    for i, (t, rows) in enumerate(zip(q.tasks, q.rows)):
        lights, direct, path = M.rows_of(rows, "light"), M.rows_of(rows, "direct"), M.rows_of(rows, "path")
        hs_of = G.group(hs[i], "d")
        assert all(same(h["pos"], t["pos"]) for h in hs[i])
        for li in lights:
            nd, node = int(li[6]), q.flat.node(int(li[1]))
            lp = np.array(list(node.pos))
            lo, hi = M.shard_range(nd, *shard)
            scale = t["Tc"] * (li[3:6] * (2.0 * li[2] / nd))
            rs = direct[(direct[:, 2] == li[1]) & (direct[:, 1] >= lo) & (direct[:, 1] < hi)]
            assert len(rs) == hi - lo
            live = rs[(rs[:, 6] > 0) & (rs[:, 7] < np.inf)]
            w = M.closed_weight(q.detmath, live[:, 6], t["theta_i"], t["on_a"], t["on_b"], live[:, 3:6], t["surface_d"], t["ray_projection"])
            for r, wc in zip(live, w):
                dv = (t["pos"] + r[3:6] * r[7]) - lp
                dsq = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]
                local = node.radiance / dsq if dsq > 0 else 1e30
                if r[9] == 0:
                    assert local == r[10]                                          # the oracle's own local_intensity
                h = G.take(hs_of, key(r[3:6]))
                if h is not None:
                    assert h["limit"] == r[7] and not (h["pad"] & G.ACN_RESUME_PROBE) and h["pad"] & 2
                    assert same(h["contrib"], scale * (local * wc * t["diffuse_intensity"])), (i, int(li[1]), int(r[1]))
                    tally["hard_shadow"] += 1
                elif r[9] == 0:
                    tally["inline"] += 1
        n_path = q.counts[i][1]
        if n_path:
            lo, hi = M.shard_range(n_path, *shard)
            scale = t["Tc"] * (2.0 / n_path)
            rs = path[(path[:, 1] >= lo) & (path[:, 1] < hi)]
            assert len(rs) == hi - lo
            ch_of, hp_of = G.group(ch[i], "d"), G.group(hp[i], "d")
            assert not (set(ch_of) & set(hp_of))
            for r in rs:
                k = key(r[2:5])
                if not r[5] > 0:
                    continue
                child_i = r[13]
                dark = t["depth"] - 10 == 0 or child_i < tmin
                if k in ch_of:
                    c = G.take(ch_of, k)
                    assert not dark and r[7] < max_len
                    assert c["offs"] == r[7] and same(c["exit_nor"], r[8:11]) and c["exit_obj"] == r[11] and c["enter_obj"] == r[12]
                    assert G.bits(c["intensity"]) == G.bits(child_i) and c["depth"] == t["depth"] - 10
                    assert same(c["T"], scale) and same(c["p"], t["pos"])
                    tally["children"] += 1
                elif k in hp_of:
                    c = G.take(hp_of, k)
                    assert not dark and G.bits(c["intensity"]) == G.bits(child_i) and c["depth"] == t["depth"] - 10
                    assert same(c["T"], scale) and same(c["pos"], t["pos"]) and c["resume"] & 2
                    tally["hard_path"] += 1
                elif k in hs_of:
                    h = G.take(hs_of, k)                                           # a dark ray that needs the machine: a probe for the background term
                    assert dark and h["limit"] == path_limit and not (h["pad"] & G.ACN_RESUME_PROBE)
                    assert same(h["contrib"], scale * (bg * child_i))
                    tally["probes"] += 1
                else:
                    assert dark or not r[7] < max_len, (i, r)
                    tally["background"] += int(not r[7] < max_len)
            assert not ch_of and not hp_of, (i, len(ch_of), len(hp_of))
        assert not hs_of, (i, len(hs_of))
    return tally


def check_queue(q, classes=(0, 1, 2, 3), generic=True, need=()):
    """the three references of the module's docstring; returns check_records' tally of class 16"""
    outs = {c: q.run(cls=c) for c in classes}
    ref = outs[3] if 3 in outs else outs[classes[0]]
    for c, o in outs.items():
        assert o["flags"] == 0, (c, o["flags"])
        for name in QUEUES:
            G.same_records(o[name], list(ref[name]), (name, c))
        assert np.array_equal(o["accum"], exact_accum(q, o, LANES[c])), ("accum", c)
    if generic and q.info["leaf_lights"]:
        g = q.run(cls=1, leaf_lights=False)
        for name in QUEUES:
            G.same_records(g[name], list(outs[1][name]), (name, "generic"))
        assert np.array_equal(g["accum"], outs[1]["accum"])
    plain = q.run(cls=1, prune=False)
    for name in QUEUES:
        G.same_records(plain[name], list(outs[1][name]), (name, "no prune"))
    assert np.array_equal(plain["accum"], outs[1]["accum"])
    tally = check_records(q, outs[1])
    for k in need:
        assert tally[k] > 0, (k, tally)
    return tally, outs


# ---------------------------------------------------------------------------------------------------------------------
# the light's constants: two lights of different kinds in either order, an envelope, a light that is no leaf

FLOOR_POINTS = (((0.5, -0.5, LIFT), 200, 22), ((2.5, 1.0, LIFT), 17, 12), ((-1.5, -2.0, LIFT), 16, 22), ((0.2, 3.0, LIFT), 15, 10))
# inside the light's sphere ( cos_rs = -1 ), on the plane light's plane ( cos_rs = 0 ): the cone cull returns 0
INSIDE_POINTS = (((LIGHT_AT[0] + 0.2, LIGHT_AT[1], LIGHT_AT[2] - 0.1), 17, 12), ((0.3, 0.2, 9.0), 17, 12), (LIGHT_AT, 5, 12))


@pytest.mark.parametrize("lights", [("sphere", "plane"), ("plane", "sphere"), ("sphere_env", "plane"), ("plane", "sphere_env", "sphere"),
                                    ("sphere", "pair", "plane")], ids=lambda l: "-".join(l))
def test_light_constants_per_light(oracle, detmath_cpu, lights):
    """a constant of light 0 left in the frame shows in light 1's records (limit, contrib) and sums"""
    q = Queue(oracle, detmath_cpu, build(lights, ["glass", (0.4, (2.0, 0.6, 2.2))]), FLOOR_POINTS + INSIDE_POINTS)
    try:
        assert q.info["lights"] == len(lights) and q.info["leaf_lights"] == ("pair" not in lights)
        tally, _ = check_queue(q, need=("hard_shadow", "inline", "hard_path", "background"))
        print(lights, tally)
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------------------------------
# the root positions of a wave: mixed cull masks, the empty set, positions from 64 on

def test_mixed_cull_masks_in_one_wave(oracle, detmath_cpu):
    """four class-16 tasks fetched together: under the glass, everything culled, and two whose cones keep one sphere each"""
    matter = ["glass", (0.3, (3.0, 2.0, 2.5)), (0.3, (-2.5, -2.0, 2.5))]
    points = (((0.5, -0.5, LIFT), 40, 12), ((6.0, -6.0, LIFT), 40, 12), ((5.5, 4.5, LIFT), 40, 12), ((-5.5, -3.5, LIFT), 40, 12))
    q = Queue(oracle, detmath_cpu, build(("sphere",), matter), points)
    try:
        skips = cull_masks(q)                                  # positions: 0 floor, 1 glass, 2 and 3 the spheres
        assert skips[0] & 2 == 0 and skips[1] == 15 and skips[2] == 15 & ~4 and skips[3] == 15 & ~8, [bin(s) for s in skips]
        tally, outs = check_queue(q, need=("hard_shadow", "inline"))
        deferred = [int((outs[1]["hard_shadow"]["pixel"] == i).sum()) for i in range(4)]
        assert deferred[0] > 0 and deferred[1] == 0, deferred
        print("mixed masks:", tally, deferred, [bin(s) for s in skips])
    finally:
        q.close()


def test_every_position_culled(oracle, detmath_cpu):
    """a queue whose tasks cull every root element for the light: the waves run no root loop, and every live sample is in the sums"""
    matter = ["glass", (0.3, (3.0, 2.0, 2.5))]
    points = tuple(((6.0 + 0.1 * k, -6.0 - 0.2 * k, LIFT), n, 10) for k, n in enumerate((40, 17, 16, 15, 1, 64, 40, 40)))
    q = Queue(oracle, detmath_cpu, build(("sphere",), matter, path_samples=0), points)
    try:
        assert all(s == 7 for s in cull_masks(q))
        tally, outs = check_queue(q, need=("inline",))
        assert len(outs[1]["hard_shadow"]) == 0 and tally["inline"] == sum(c[0] for c in q.counts)
    finally:
        q.close()


def test_root_of_seventy_elements(oracle, detmath_cpu):
    """69 small spheres over the floor: positions 64 .. 69 are visited whatever the masks say, the first 64 as each task culls them"""
    rng = np.random.default_rng(9)
    balls = [(0.12, (LIGHT_AT[0] + np.cos(0.7 * k) * (0.05 + 0.012 * k), LIGHT_AT[1] + np.sin(0.7 * k) * (0.05 + 0.012 * k), 2.5 + 0.03 * k))
             for k in range(69)]                                 # a spiral under the light: a floor point's cone keeps eight to thirteen
    points = tuple(((rng.uniform(-2.5, 3.5), rng.uniform(-3.5, 2.5), LIFT), n, 12) for n in (40, 40, 40, 40, 17, 200, 40, 40))
    q = Queue(oracle, detmath_cpu, build(("sphere",), balls), points)
    try:
        assert len(q.flat.elems_of(q.flat.c.matter_root)) == 70
        skips = cull_masks(q)
        assert len(set(skips)) > 4 and all(40 < bin(s).count("1") < 64 for s in skips), [hex(s) for s in skips]
        tally, outs = check_queue(q, need=("inline", "children"))
        # some samples are occluded in line, by an element before position 64 and by one behind
        direct = np.concatenate([M.rows_of(rw, "direct") for rw in q.rows])
        assert 0 < int((direct[:, 9] != 0).sum()) < len(direct)
        print("70 elements:", tally)
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------------------------------
# sample counts and the start of a shard's LCG states

@pytest.fixture(scope="module")
def counts_queue(oracle, detmath_cpu):
    rng = np.random.default_rng(3)
    points = tuple(((rng.uniform(-2.0, 3.0), rng.uniform(-3.0, 2.0), LIFT), n, 12) for n in (1, 15, 16, 17, 200, 64, 4, 2))
    q = Queue(oracle, detmath_cpu, build(("sphere", "plane"), ["glass", (0.4, (2.0, 0.6, 2.2))]), points)
    yield q
    q.close()


def test_sample_counts(counts_queue):
    q = counts_queue
    assert [c[0] for c in q.counts] == [1, 15, 16, 17, 200, 64, 4, 2] and [c[1] for c in q.counts] == [1, 15, 16, 17, 200, 64, 4, 2]
    # in class 16, and the tasks of the other three classes in theirs (one task each, through the index list)
    tally, _ = check_queue(q, need=("children", "background", "inline"))
    for cls, task in ((0, 4), (2, 6), (3, 7)):
        one = q.run(cls=cls, index=[task])
        want = exact_accum(q, one, LANES[cls])
        assert np.array_equal(one["accum"][task], want[task]) and not np.delete(one["accum"], task, axis=0).any()
    print("counts:", tally)


def test_sample_counts_sharded(counts_queue):
    """shard_world = 3: the ranks' records partition the unsharded queues, every rank's sums are its share added as the kernel adds
    it, and the three add up to the unsharded sums: each of the four is rounded once to 2^-40 (half a unit each: 2 units), and the
    shares are the same terms in another association (the bound of test_gpu_stages.check_against_tap between two sums of m terms)"""
    q = counts_queue
    whole = q.run(cls=1)
    parts = [q.run(cls=1, shard_rank=k, shard_world=3) for k in range(3)]
    for name in QUEUES:
        G.same_records(np.concatenate([p[name] for p in parts]), list(whole[name]), name)
    for k, p in enumerate(parts):
        check_records(q, p, shard=(k, 3))
        assert np.array_equal(p["accum"], exact_accum(q, p, 16, shard=(k, 3))), k
    total = parts[0]["accum"] + parts[1]["accum"] + parts[2]["accum"]
    m = np.array([max(c) for c in q.counts])[:, None]
    bound = 2 * (m + 8) * 2.0 ** -53 * np.abs(whole["accum"]) + 2
    assert (np.abs(total - whole["accum"]) <= bound).all(), (total - whole["accum"], bound)


# ---------------------------------------------------------------------------------------------------------------------
# the COUNT variants: a frame of the mixed scene, as test_work_counters_match_oracle_exactly counts the wine glass

def test_count_variant_tallies(oracle):
    sc = build(("sphere_env", "plane"), ["glass", (0.4, (2.0, 0.6, 2.2)), (0.3, (-2.5, -2.0, 2.5))], direct_samples=40, path_samples=20)
    flat = sc.flatten()
    pos = A.main_pass_positions(flat.params.image_width, flat.params.image_height)
    h = A.Handle(flat, count_work=True)
    try:
        h.render_positions(pos)
        g = h.last_counters()
    finally:
        h.close()
    _, c = oracle.render_positions(flat, pos, counters=True)
    assert c["cap_sample"] > 30000 and c["shadow_ray"] > 20000
    assert g["lum_calls"] == c["lum"] and g["cap_samples"] == c["cap_sample"]
    assert g["shadow_rays"] == c["shadow_ray"] and g["trans_rays"] == c["trans_ray"]
    assert g["overflows"] == 0
    M.frame_work_identities(g, c)                              # transcendentals as an identity, flop from its shading part up
