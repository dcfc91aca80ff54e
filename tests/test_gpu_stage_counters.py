"""The counting kernel variants (KernelFlags::count: k_walk_count, k_walk_count_prune and the COUNT forms of k_shade_hits, k_shade,
k_hard_shadow, k_hard_path) one at a time through the stage seam (ACN_STAGE_COUNT_WORK), and the ten work counters they tally -- the
numbers bench.py turns into the achieved-FLOP figure -- against the oracle, on the queues of the per-stage tests:

  a  the counting variant writes what the plain variant writes: every queue as sorted byte strings, accum bit for bit, the flags, and
     of the counter block every word that does not depend on which wave drew which record (the exact statistics QS_*, and mark - dead
     of every queue: a mark counts the unused ends of the waves' reservations, and which wave ends where is not the launch's to decide)
  b  the ten counters do not depend on the arrangement: size class, dead index entries, grid, passes / fetch / stacks of the walk;
     shard ranks add up, with the set-up booked once per rank
  c  against the oracle: tests/shade_model.py's ledger (the tap's rows priced with acn_costs.h, the device's deliberate differences
     applied by name) predicts lum_calls, cap_samples, shadow_rays, trans_rays, transcendentals and the shading part of flop exactly;
     what is left of flop is geometry, at most what the oracle spends on the same rays, as are obj_hits, side_calls and sdf_evals
  d  every case asserts that its queue made the kernel do the thing (inline samples, deferred ones, background hits), and that the
     prediction it pins is not zero
  e  a stage call, counting or not, leaves acn_last_counters alone"""
import numpy as np
import pytest

import actinon_amd as A
import hard_queues as Q
import ray_sets as R
import shade_model as M
import walk_model as W
import test_gpu_stages as G
import test_gpu_shade_loops as L
import test_gpu_shade_batches as B
import test_gpu_stages_hard as H
from query_checks import upload
from test_gpu_shade_batches import queue33   # noqa: F401  (the fixture: 33 tasks, two lights, every fourth on the carrier ball)

pytestmark = pytest.mark.gpu

REC = A.Handle.STAGE_RECORDS
QC = A.Handle.QC
DEAD = A.Handle.STAGE_INVALID
NAMES = A.Handle.COUNTERS
STACK = A.abi.ACN_STAGE_WALK_MAX_STACK
# queue -> (mark, dead slots or None): mark - dead = records, whichever wave reserved what
MARKS = {"tasks": ("tasks", "dead_t"), "children": ("children", "dead_c"), "hard_path": ("hard_path", "dead_hp")}
STATS = ("walk_rays", "s_hard_shadow", "s_hard_path", "s_children", "s_tasks", "s_probes")


def same_output(plain, counted, queues, what):
    """a: what the two variants wrote"""
    assert plain["flags"] == counted["flags"], (what, plain["flags"], counted["flags"])
    assert np.array_equal(plain["accum"], counted["accum"]), (what, "accum")
    for name in queues:
        G.same_records(counted[name], list(plain[name]), (what, name))
    if "idx" in plain:
        G.same_records(counted["tasks"][np.concatenate(counted["idx"])], list(plain["tasks"][np.concatenate(plain["idx"])]), (what, "tasks"))
        assert [len(l) for l in plain["idx"]] == [len(l) for l in counted["idx"]], what
    p, c = plain["counts"], counted["counts"]
    for k in STATS:
        assert p[QC[k]] == c[QC[k]], (what, k, p[QC[k]], c[QC[k]])
    for name, (mark, dead) in MARKS.items():
        assert int(p[QC[mark]]) - int(p[QC[dead]]) == int(c[QC[mark]]) - int(c[QC[dead]]), (what, name)
    assert "counters" not in plain and list(counted["counters"]) == NAMES


def exact(g, m, what, geometry_transc=0):
    """c: the counters the ledger pins; geometry_transc: the roughness term of the queue's rays (rough), zero without a rough surface"""
    print(what, "device", g, "model", m)
    assert g["overflows"] == 0, what
    assert g["lum_calls"] == m["lum"], (what, "lum_calls", g["lum_calls"], m["lum"])
    assert g["cap_samples"] == m["cap_sample"], (what, "cap_samples", g["cap_samples"], m["cap_sample"])
    assert g["shadow_rays"] == m["shadow_ray"], (what, "shadow_rays", g["shadow_rays"], m["shadow_ray"])
    assert g["trans_rays"] == m["trans_ray"], (what, "trans_rays", g["trans_rays"], m["trans_ray"])
    assert g["transcendentals"] == m["transc_shade"] + geometry_transc, (what, "transcendentals", g["transcendentals"], m["transc_shade"], geometry_transc)
    assert g["flop"] >= m["flop_shade"], (what, "flop below its shading part", g["flop"], m["flop_shade"])
    return g["flop"] - m["flop_shade"]


def rough(c):
    """the transcendentals of the oracle's geometry for the same rays: ACN_T_ROUGHNESS per finite hit of a rough object whose normal is
    asked for -- the only transcendental outside scene_s_lum.  k_walk and k_hard_path test every element that can hit and want its
    normal, as compound_s_ray_trans_hit does, so they book the same number; a shadow test wants no normal and books none."""
    t = c["transc"] - c["transc_shade"]
    assert t % M.costs()["T_ROUGHNESS"] == 0
    return t


def bounded(g, remainder, c, what):
    """c: the geometry the device did is part of what the oracle does for the same rays"""
    print(what, "remainder", remainder, "oracle geometry", c["flop"] - c["flop_shade"], {k: c[k] for k in ("obj_hit", "side", "sdf_eval")})
    assert 0 <= remainder <= c["flop"] - c["flop_shade"], (what, remainder, c["flop"] - c["flop_shade"])
    assert g["obj_hits"] <= c["obj_hit"] and g["side_calls"] <= c["side"] and g["sdf_evals"] <= c["sdf_eval"], (what, g, c)


PINNED_BY_SHADE = ("cap_sample", "shadow_ray", "trans_ray", "transc_shade", "flop_shade", "direct_tail", "light_setups")


def nonzero(m, keys, what):
    """d: a prediction that is pinned is not pinned at zero"""
    for k in keys:
        assert m[k] > 0, (what, k, m)


def light_samples(oracle, flat, recs):
    """Which HardShadow records are direct-light samples, by the oracle alone: the limit of a sample is the distance at which its ray
    hits the light it was drawn for (obj_ray_hit of that light, to the bit: test_gpu_shade_loops.check_records), while a probe's limit
    is the path limit or the largest double.  Nothing of the record's word is read, nor the path limit the kernel compares with."""
    rays = H.rays_of(recs)
    is_sample = np.zeros(len(recs), dtype=bool)
    for light in flat.elems_of(flat.c.light_root):
        a, _ = oracle.obj_ray_hits(flat, light, rays)
        is_sample |= (a < np.inf) & (a == recs["limit"])
    return is_sample


def add_counters(cs):
    return {k: sum(c[k] for c in cs) for k in cs[0]}


# ---------------------------------------------------------------------------------------------------------------------
# k_shade

def shade_prediction(v, out, shard=(0, 1)):
    """the ledger of the launch: the tasks of the view v, with the samples the launch left to the hard-ray kernels read off its records
    (tests/test_gpu_shade_loops.check_records matches those to the tap's samples one for one)"""
    n = len(v.tasks)
    hs, hp = G.by_pixel(out["hard_shadow"], n), G.by_pixel(out["hard_path"], n)
    key = lambda d: G.bits(d).tobytes()                                            # noqa: E731
    return M.add_ledgers([M.ledger(v.rows[i], device=True, shard=shard, deferred={key(h["d"]) for h in hs[i]}, hard_path={key(h["d"]) for h in hp[i]})
                          for i in range(n)])


def setup_flop(v):
    """what a launch books once per task whatever its share of the samples: per light the cone and the frame, and the path loop's frame"""
    C = M.costs()
    per = [M.ledger(rw) for rw in v.rows]
    return sum(l["light_setups"] * (C["F_FOV"] + C["F_FRAME"]) + l["path_setups"] * C["F_FRAME"] for l in per)


def oracle_of_tasks(q, sel):
    return add_counters([q.oracle.shade_point_counters(q.flat, M.tap_input(q.hits[i])) for i in sel])


@pytest.fixture(scope="module")
def shade33(queue33):
    """the 33 tasks on every size class, plain and counting: [cls] = (plain, counted)"""
    v = B.view(queue33, range(33))
    runs = {c: (v.h.run_stage("shade", v.tasks, cls=c), v.h.run_stage("shade", v.tasks, cls=c, count_work=True)) for c in range(4)}
    return v, runs


def test_shade_counting_variant_writes_the_same(queue33, shade33):
    """a, for the four classes, and at class 16 without the prune programs and with the generic light hit"""
    v, runs = shade33
    for c, (plain, counted) in runs.items():
        same_output(plain, counted, L.QUEUES, ("shade", c))
    for kw in (dict(prune=False), dict(leaf_lights=False)):
        plain, counted = v.h.run_stage("shade", v.tasks, cls=1, **kw), v.h.run_stage("shade", v.tasks, cls=1, count_work=True, **kw)
        same_output(plain, counted, L.QUEUES, ("shade", kw))
        for name in L.QUEUES:
            G.same_records(counted[name], list(runs[1][1][name]), (name, kw))
        exact(counted["counters"], shade_prediction(v, counted), ("shade", kw))
    tally = L.check_records(v, runs[1][1])
    assert tally["inline"] > 0 and tally["hard_shadow"] > 0 and tally["background"] > 0 and tally["hard_path"] > 0, tally


def test_shade_counters_equal_in_every_class(queue33, shade33):
    """b: the batched set-up of class 16 books per task on the task's lane, the plain step of the other classes on one lane of the
    group: all ten words equal, the geometry remainder with them"""
    v, runs = shade33
    ref = runs[2][1]["counters"]
    assert ref["flop"] > 0 and ref["cap_samples"] > 0
    for c in range(4):
        assert runs[c][1]["counters"] == ref, (c, runs[c][1]["counters"], ref)


def test_shade_counters_against_the_oracle(queue33, shade33):
    """c and d on the 33 tasks: exact where the ledger decides, geometry within the oracle's for the same tasks"""
    v, runs = shade33
    g = runs[1][1]["counters"]
    m = shade_prediction(v, runs[1][1])
    for k in ("cap_sample", "shadow_ray", "trans_ray", "transc_shade", "flop_shade", "direct_tail", "path_tail", "light_setups", "path_setups"):
        assert m[k] > 0, (k, m)
    assert m["lum"] == 0 and m["light_setups"] == 66                               # k_shade makes no scene_s_lum call; 33 tasks, two lights
    rem = exact(g, m, "shade 33")
    c = oracle_of_tasks(queue33, range(33))
    bounded(g, rem, c, "shade 33")
    assert g["obj_hits"] > 0 and g["sdf_evals"] == 0 and rem > 0                   # (the torus is left to k_hard_shadow: no SDF step here)
    # the carrier's tasks have on_b = 0, the floor's on_b > 0: both kinds of the direct weight were priced
    assert m["oren_nayar_direct"] > 0 and (queue33.tasks["on_b"] == 0).sum() == 8


@pytest.mark.parametrize("where", list(B.DEAD_LISTS))
def test_shade_counters_with_dead_index_entries(queue33, where):
    """b: a dead entry books nothing, wherever it lies in a batch; 20 tasks reached through each list and in order"""
    v = B.view(queue33, range(20))
    ref = v.h.run_stage("shade", v.tasks, cls=2, count_work=True)
    got = v.h.run_stage("shade", v.tasks, cls=1, index=B.DEAD_LISTS[where], count_work=True)
    plain = v.h.run_stage("shade", v.tasks, cls=1, index=B.DEAD_LISTS[where])
    same_output(plain, got, L.QUEUES, ("dead", where))
    assert got["counters"] == ref["counters"], (where, got["counters"], ref["counters"])
    assert got["counters"]["overflows"] == 0
    m = shade_prediction(v, got)
    nonzero(m, PINNED_BY_SHADE, ("dead", where))
    exact(got["counters"], m, ("dead", where))
    tally = L.check_records(v, got)
    assert tally["inline"] > 0 and tally["hard_shadow"] > 0 and tally["background"] > 0, tally


def test_shade_counters_of_the_shards_add_up(queue33):
    """b, shards ( r, 3 ): every sample belongs to one rank, so what a sample books -- the cap sample, the light hit, the shadow ray,
    the tails, the path ray: cap_samples, shadow_rays, trans_rays, transcendentals, and flop but for the set-up -- adds up to the
    unsharded launch; the set-up (per light ACN_F_FOV + ACN_F_FRAME, the path loop's ACN_F_FRAME) every rank books for itself:
        sum over ranks of flop = flop of the whole + ( world - 1 ) * set-up"""
    v = B.view(queue33, range(17))
    for cls in (1, 2):
        whole = v.h.run_stage("shade", v.tasks, cls=cls, count_work=True)
        parts = [v.h.run_stage("shade", v.tasks, cls=cls, shard_rank=r, shard_world=3, count_work=True) for r in range(3)]
        for r, p in enumerate(parts):
            same_output(v.h.run_stage("shade", v.tasks, cls=cls, shard_rank=r, shard_world=3), p, L.QUEUES, ("shard", r))
            m = shade_prediction(v, p, shard=(r, 3))
            nonzero(m, PINNED_BY_SHADE, ("shard", cls, r))
            exact(p["counters"], m, ("shard", cls, r))
            tally = L.check_records(v, p, shard=(r, 3))
            assert tally["inline"] > 0, (cls, r, tally)
        total = add_counters([p["counters"] for p in parts])
        w = whole["counters"]
        for k in ("cap_samples", "shadow_rays", "trans_rays", "transcendentals", "obj_hits", "side_calls", "sdf_evals", "lum_calls", "overflows"):
            assert total[k] == w[k], (cls, k, total[k], w[k])
        setup = setup_flop(v)
        C = M.costs()
        assert setup == 17 * 2 * (C["F_FOV"] + C["F_FRAME"]) + C["F_FRAME"] * int((v.tasks["depth"] > 10).sum()) and setup > 0   # 17 tasks, two lights
        assert total["flop"] == w["flop"] + 2 * setup, (cls, total["flop"], w["flop"], setup)


def test_shade_mixed_batch_counters(oracle, detmath_cpu):
    """the 16 tasks of test_gpu_shade_batches.test_mixed_batch -- neighbours that differ in on_b, in the sample count (9 and 255), in
    having a path loop, in the cone cull, under three lights: the classes agree and the ledger holds"""
    inside = L.INSIDE_POINTS[0][0]
    rng = np.random.default_rng(23)
    rnd = lambda: (rng.uniform(-2.0, 3.0), rng.uniform(-3.0, 2.0), L.LIFT)         # noqa: E731
    points = (((0.5, -0.5, L.LIFT), 9, 12, 0), (rnd(), 255, 22, 3), (inside, 17, 12, 0), (rnd(), 17, 10, 0),
              (rnd(), 9, 10, 3), ((0.5, -0.5, L.LIFT), 255, 12, 0), (rnd(), 9, 22, 3), (inside, 40, 10, 3),
              (rnd(), 16, 12, 0), (rnd(), 255, 10, 3), (rnd(), 9, 12, 0), (rnd(), 33, 22, 3),
              (rnd(), 15, 10, 0), ((6.0, -6.0, L.LIFT), 40, 12, 3), (rnd(), 9, 12, 0), (rnd(), 255, 12, 3))
    q = B.BatchQueue(oracle, detmath_cpu, B.scene(("plane", "sphere_env", "sphere"), 256), points)
    try:
        v = B.view(q, range(16))
        outs = {c: v.h.run_stage("shade", v.tasks, cls=c, count_work=True) for c in (0, 1, 2, 3)}
        for c in (0, 1, 3):
            assert outs[c]["counters"] == outs[2]["counters"], (c, outs[c]["counters"], outs[2]["counters"])
        tally = L.check_records(v, outs[1])
        for k in ("hard_shadow", "inline", "background"):
            assert tally[k] > 0, tally
        m = shade_prediction(v, outs[1])
        assert m["oren_nayar_direct"] > 0 and m["oren_nayar_path"] > 0 and m["light_setups"] == 48
        rem = exact(outs[1]["counters"], m, "mixed batch")
        bounded(outs[1]["counters"], rem, oracle_of_tasks(q, range(16)), "mixed batch")
    finally:
        q.close()


def test_shade_geometry_flop_derived(oracle, detmath_cpu):
    """The exact case: a scene whose matter root holds the floor and one ball under a plain sphere light, tasks on the floor without a
    path loop (depth 10).  Every event of the launch can then be derived, geometry included:
      the light hit    one sphere test per sample whose weight is > 0: ACN_F_SPHERE_HIT if it is finite (the tap's row says so), else
                       ACN_F_SPHERE_MISS -- the light is a leaf, tested without a normal
      the shadow ray   the floor is culled for every task (the points lie above it, no ray of the cone can reach it), so the only
                       element a shadow ray can meet is the ball: where the task's cone cull keeps it, one sphere test without a
                       normal, finite or not by the oracle's own hit of that ball; where it is culled, nothing
    With one element left the any-hit order has nothing to decide, and the cone cull is read from the device (cull_masks) per task:
    nothing is undetermined, and flop is asserted as an equality in all four classes."""
    C = M.costs()
    ball_at = (0.5, -0.5, 2.5)
    points = (((0.5, -0.5, L.LIFT), 40, 10), ((0.7, -0.4, L.LIFT), 17, 10), ((0.3, -0.9, L.LIFT), 16, 10), ((6.0, -6.0, L.LIFT), 40, 10),
              ((-4.0, 3.0, L.LIFT), 15, 10), ((0.5, -0.2, L.LIFT), 9, 10), ((1.2, -0.5, L.LIFT), 33, 10), ((5.0, 5.0, L.LIFT), 9, 10))
    q = L.Queue(oracle, detmath_cpu, L.build(("sphere",), [(0.4, ball_at)], direct_samples=40), points)
    try:
        matter = q.flat.elems_of(q.flat.c.matter_root)
        assert len(matter) == 2 and q.info["lights"] == 1 and q.info["leaf_lights"]
        masks = L.cull_masks(q)
        assert all(m & 1 for m in masks) and any(m & 2 for m in masks) and not all(m & 2 for m in masks), [bin(m) for m in masks]
        geometry = obj_hits = occluded = 0
        for t, rows, mask in zip(q.tasks, q.rows, masks):
            d = M.rows_of(rows, "direct")
            asked = d[d[:, 6] > 0]
            hit = asked[:, 7] < np.inf
            geometry += int(hit.sum()) * C["F_SPHERE_HIT"] + int((~hit).sum()) * C["F_SPHERE_MISS"]
            obj_hits += len(asked)
            if not mask & 2:
                rays = np.concatenate([np.tile(t["pos"], (int(hit.sum()), 1)), asked[hit][:, 3:6]], axis=1)
                a, _ = oracle.obj_ray_hits(q.flat, matter[1], rays)
                geometry += int((a < np.inf).sum()) * C["F_SPHERE_HIT"] + int((~(a < np.inf)).sum()) * C["F_SPHERE_MISS"]
                obj_hits += len(rays)
                occluded += int((a < np.inf).sum())
        assert occluded > 0 and geometry > 0
        outs = {c: q.run(cls=c, count_work=True) for c in range(4)}
        m = shade_prediction(q, outs[1])
        assert len(outs[1]["hard_shadow"]) == 0 and m["trans_ray"] == 0 and m["path_setups"] == 0 and m["direct_tail"] > 0
        for c, o in outs.items():
            g = o["counters"]
            assert exact(g, m, ("derived", c)) == geometry, (c, g["flop"] - m["flop_shade"], geometry)
            assert g["obj_hits"] == obj_hits and g["side_calls"] == 0 and g["sdf_evals"] == 0, (c, g, obj_hits)
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------------------------------
# k_shade_hits

@pytest.fixture(scope="module")
def stage_a(oracle):
    s = G.Stage(oracle, False)
    yield s
    s.h.close()


def test_shade_hits_counters(stage_a):
    """The split has no geometry: every one of its events is the ledger's, so flop and transcendentals are equalities.  ~2 000 hit
    records of every kind (test_gpu_stages.split); a, and b: emit_terms off drops the probes' records, not what the kernel books --
    a dead child stands for its two compound_s_ray_trans_hit calls either way."""
    recs = R.stage_split_hits(stage_a.oracle, stage_a.flat, stage_a.node, REC["hit"])
    rows = stage_a.tap(recs)
    plain, counted = stage_a.h.run_stage("shade_hits", recs), stage_a.h.run_stage("shade_hits", recs, count_work=True)
    same_output(plain, counted, ("rays", "hard_shadow"), "shade_hits")
    m = M.add_ledgers([M.ledger_hit(rw, r["offs"], stage_a.prm, device=True) for r, rw in zip(recs, rows)])
    for k in ("lum", "trans_ray", "flop_shade", "transc_shade"):
        assert m[k] > 0, (k, m)
    assert m["trans_ray"] == 2 * len(plain["hard_shadow"]) and len(plain["rays"]) > 300 and len(np.concatenate(plain["idx"])) > 300
    g = counted["counters"]
    assert exact(g, m, "shade_hits") == 0
    assert g["obj_hits"] == 0 and g["side_calls"] == 0 and g["sdf_evals"] == 0
    quiet = stage_a.h.run_stage("shade_hits", recs, emit_terms=False, count_work=True)
    assert len(quiet["hard_shadow"]) == 0 and quiet["counters"] == g


# ---------------------------------------------------------------------------------------------------------------------
# k_hard_shadow, k_hard_path

@pytest.fixture(scope="module")
def pools(oracle):
    p = H.Pools("stage_a", oracle)
    yield p
    p.close()


def shadow_prediction(p, q, src):
    """k_hard_shadow books one event of its own: ACN_F_DIRECT_TAIL for a direct-light sample k_shade left to it that turns out not to
    be occluded (scene.c:571-574; an in-line sample books the same in k_shade).  A probe -- a dark path ray, a dead specular child, a
    seeded one -- has no tail: the oracle books nothing for the background term it stands for.  Which record is which is the
    oracle's word (light_samples), and only records k_shade wrote can be samples: the pool keeps those first."""
    live = src >= 0
    sample = np.zeros(len(q), dtype=bool)
    sample[live] = light_samples(p.oracle, p.flat, q[live])
    open_ = live & ~np.where(live, p.occluded[src], True)
    return int((sample & open_).sum()), int((~sample & open_).sum()), sample


def oracle_of_shadow(p, q, src):
    live = src >= 0
    rays, lim = H.rays_of(q[live]), q["limit"][live]
    _, c = p.oracle.query_rays(p.flat, "occluded", p.flat.c.matter_root, rays, limits=lim, counters=True)
    first = q["pad"][live] & 1 != 0
    _, cl = p.oracle.query_rays(p.flat, "occluded", p.flat.c.light_root, rays[first], limits=lim[first], counters=True)
    return add_counters([c, cl])


@pytest.mark.parametrize("case", ["live_129", "partial_last_batch", "dead_batch_between", "all_finished_in_fill"])
def test_hard_shadow_counters(pools, case):
    p = pools
    layout = Q.layout_live(129) if case == "live_129" else Q.LAYOUTS[case]
    q, src = p.queue(layout, resumed_only=case == "live_129")
    C = M.costs()
    outs = {g: p.h.run_stage("hard_shadow", q, grid=g, count_work=True) for g in (1, 2, 0)}
    plain = p.h.run_stage("hard_shadow", q, grid=1)
    same_output(plain, outs[1], (), ("hard_shadow", case))
    # the queue slot for slot.  One deliberate difference, stated in acn_k_hard.h: the counting variant has no fill phase -- it runs the
    # full loop on every record, as the oracle does -- so it leaves a probe's word as it came, where the plain variant writes the
    # resume word of its in-line pass; records that came with a resume word, and every other field, are left alike
    a, b = plain["hard_shadow"], outs[1]["hard_shadow"]
    live = src >= 0
    for f in a.dtype.names:
        if f != "pad":
            assert a[f][live].tobytes() == b[f][live].tobytes(), (case, f)
    came_resumed = live & (q["pad"] & H.RESUME_FLAG != 0)
    assert np.array_equal(a["pad"][came_resumed], b["pad"][came_resumed]) and np.array_equal(b["pad"][live], q["pad"][live]), case
    for g in (2, 0):
        assert outs[g]["counters"] == outs[1]["counters"], (case, g, outs[g]["counters"], outs[1]["counters"])
    tails, open_probes, sample = shadow_prediction(p, q, src)
    g = outs[1]["counters"]
    print(case, g, "unoccluded samples", tails, "unoccluded probes", open_probes, "samples", int(sample.sum()))
    for k in ("lum_calls", "cap_samples", "shadow_rays", "trans_rays", "transcendentals", "overflows"):
        assert g[k] == 0, (case, k, g[k])                                          # the shadow ray itself was counted where it was cast
    # d: the layouts that hold records of k_shade pin the tail on some; the one made of probes alone pins that none is booked
    if case == "all_finished_in_fill":
        assert tails == 0 and open_probes > 0 and not sample.any()
    else:
        assert tails > 0 and sample.any(), (case, tails)
    c = oracle_of_shadow(p, q, src)
    rem = g["flop"] - tails * C["F_DIRECT_TAIL"]
    bounded(g, rem, c, ("hard_shadow", case))
    if case != "all_finished_in_fill":
        assert g["obj_hits"] > 0


def test_hard_shadow_flop_derived(oracle, detmath_cpu):
    """The exact case of k_hard_shadow: the floor and the torus of test_gpu_shade_loops (a distance object in an envelope) under a
    sphere light.  k_shade leaves the rays that enter the envelope to k_hard_shadow -- direct samples, and the dark path rays of
    tasks of four or five samples (trace_min_intensity 0.02: every path ray of theirs is dark), as probes -- each with a resume word that names the torus alone, so the machine phase runs one
    obj_ray_hit of the torus per record and nothing else: the object's envelope test (ACN_F_ENV_HIT: the ray entered it), then
    distance_ray_hit: from outside the envelope its side test (ACN_F_SIDE_SPHERE), the envelope's sphere hit (finite), ACN_F_SDF_RAY, and per SDF evaluation ACN_F_SDF_TORUS, per marching step ACN_F_SDF_STEP; a
    shadow test wants no normal.  With E the launch's own sdf_evals,
        flop = n * ( ENV_HIT + SIDE_SPHERE + SPHERE_HIT + SDF_RAY - SDF_STEP ) + E * ( SDF_TORUS + SDF_STEP ) + DIRECT_TAIL * unoccluded direct samples
    and a probe that turns out unoccluded books no tail: the oracle books none for the background term it stands for."""
    C = M.costs()
    rng = np.random.default_rng(7)
    near = tuple(((L.GLASS_AT[0] + rng.uniform(-0.6, 0.6), L.GLASS_AT[1] + rng.uniform(-0.6, 0.6), L.LIFT), 40, 10) for _ in range(12))
    dim = tuple(((L.GLASS_AT[0] + rng.uniform(-1.5, 1.5), L.GLASS_AT[1] + rng.uniform(-1.5, 1.5), L.LIFT), (4, 5, 4)[k % 3], 12) for k in range(400))
    q = L.Queue(oracle, detmath_cpu, L.build(("sphere",), ["glass"], trace_min_intensity=0.02), near + dim)
    try:
        prm = q.flat.params
        path_limit = np.nextafter(prm.max_path_length, 0.0)
        recs = q.run(cls=1)["hard_shadow"].copy()
        probe = ~light_samples(oracle, q.flat, recs)
        assert np.array_equal(probe, recs["limit"] == path_limit)                  # (the oracle's word and the record's limit agree on it)
        assert (recs["pad"] & 3 == 2).all() and probe.sum() >= 8 and (~probe).sum() >= 100, (len(recs), int(probe.sum()))
        recs["pixel"] = np.arange(len(recs)) % 97
        occ = oracle.query_rays(q.flat, "occluded", q.flat.c.matter_root, H.rays_of(recs), limits=recs["limit"])[:, 5] != 0
        tails, open_probes = int((~probe & ~occ).sum()), int((probe & ~occ).sum())
        assert tails > 20 and open_probes > 0 and (~probe & occ).sum() > 20, (tails, open_probes)
        outs = {g: q.h.run_stage("hard_shadow", recs, grid=g, count_work=True) for g in (1, 2)}
        same_output(q.h.run_stage("hard_shadow", recs, grid=1), outs[1], (), "hard_shadow derived")
        g = outs[1]["counters"]
        assert outs[2]["counters"] == g
        n, E = len(recs), g["sdf_evals"]
        want = n * (C["F_ENV_HIT"] + C["F_SIDE_SPHERE"] + C["F_SPHERE_HIT"] + C["F_SDF_RAY"] - C["F_SDF_STEP"]) + E * (C["F_SDF_TORUS"] + C["F_SDF_STEP"]) + C["F_DIRECT_TAIL"] * tails
        print("hard_shadow derived:", g, "records", n, "unoccluded samples", tails, "unoccluded probes", open_probes, "flop wanted", want)
        assert g["obj_hits"] == n and E >= 2 * n
        assert g["flop"] == want, (g["flop"], want, g["flop"] - want, open_probes)
    finally:
        q.close()


@pytest.mark.parametrize("dead", [False, True])
def test_hard_path_counters(pools, dead):
    """k_hard_path books no event of its own but the compound_s_ray_trans_hit each record stands for; its flop is geometry"""
    p = pools
    q = np.concatenate([p.paths] * 3)[:150].copy()
    q["pixel"] = np.arange(len(q)) % 97
    if dead:
        q["pixel"][::3] = DEAD
    live = q["pixel"] != DEAD
    outs = {g: p.h.run_stage("hard_path", q, grid=g, count_work=True) for g in (1, 2, 0)}
    plain = p.h.run_stage("hard_path", q, grid=1)
    same_output(plain, outs[1], ("children",), ("hard_path", dead))
    for g in (2, 0):
        assert outs[g]["counters"] == outs[1]["counters"], (g, outs[g]["counters"], outs[1]["counters"])
    g = outs[1]["counters"]
    assert g["trans_rays"] == int(live.sum()) > 0 and len(plain["children"]) > 0
    for k in ("lum_calls", "cap_samples", "shadow_rays", "overflows"):
        assert g[k] == 0, (k, g[k])
    _, c = p.oracle.query_rays(p.flat, "trans_hit", p.flat.c.matter_root, H.rays_of(q[live]), counters=True)
    assert g["transcendentals"] == rough(c), (g["transcendentals"], rough(c))       # scene A has a rough surface: its term, exactly
    bounded(g, g["flop"], c, ("hard_path", dead))
    assert g["obj_hits"] > 0 and g["flop"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# k_walk

class WalkCase:
    def __init__(self, oracle, flat, handle, rays):
        self.oracle, self.flat, self.h, self.rays = oracle, flat, handle, rays
        self.ledger, self.traced = W.ledger(oracle, flat, rays, REC)
        self.room = len(self.traced) + int((rays["pixel"] == DEAD).sum())

    def run(self, **kw):
        kw.setdefault("stack_cap", STACK)
        return self.h.run_stage_walk(self.rays, room_rays=self.room, **kw)

    def oracle_counters(self):
        """the oracle's scene_s_trans_hit of every traced ray: both roots"""
        return add_counters([self.oracle.query_rays(self.flat, "trans_hit", root, self.traced, counters=True)[1]
                             for root in (self.flat.c.light_root, self.flat.c.matter_root)])


@pytest.fixture(scope="module")
def small(oracle):
    """the handle that runs k_walk< LDS, PRUNE >, and so all four units of k_walk through the seam's flags"""
    sc, flat = R.walk_small_scene()
    h = upload(flat, ACN_PRUNE_MIN=1)
    rays = R.walk_rays_small_scene(flat, REC["ray"])
    yield {"all": WalkCase(oracle, flat, h, rays), "wave": WalkCase(oracle, flat, h, rays[:64].copy())}
    h.close()


WALK_QUEUES = ("hard_shadow", "rays")


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("prune", [True, False])
def test_walk_counting_variant_writes_the_same(small, lds, prune):
    """a: k_walk_count / k_walk_count_prune against k_walk_lds / k_walk_glb with and without the prune programs; c on each"""
    c = small["all"]
    info = c.h.stage_info()
    assert info["prune"] and info["lds_nodes"]
    plain, counted = c.run(passes=1, lds=lds, prune=prune), c.run(passes=1, lds=lds, prune=prune, count_work=True)
    same_output(plain, counted, WALK_QUEUES, ("walk", lds, prune))
    assert len(plain["rays"]) == 0 and plain["counts"][QC["walk_rays"]] == len(c.traced)
    exact(counted["counters"], c.ledger, ("walk", lds, prune))


@pytest.mark.parametrize("which", ["wave", "all"])
def test_walk_counters_do_not_depend_on_the_arrangement(small, which):
    """b: one launch on private stacks, every generation in a launch of its own, one-slot stacks that spill, a fetch batch of 96, one
    and three workgroups -- one wave's worth of rays and several; c: the ledger, and the geometry within the oracle's"""
    c = small[which]
    ref = c.run(passes=1, count_work=True)
    g = ref["counters"]
    for kw in (dict(passes=14, private_limit=0), dict(passes=14, private_limit=0xFFFFFFFF, stack_use=1), dict(passes=2, fetch=96),
               dict(passes=14, private_limit=0, grid=1), dict(passes=1, grid=3), dict(passes=3, private_limit=100, fetch=512)):
        out = c.run(count_work=True, **kw)
        assert len(out["rays"]) == 0, kw
        assert out["counters"] == g, (kw, out["counters"], g)
    m = c.ledger
    for k in ("lum", "trans_ray", "flop_shade") + (("transc_shade",) if which == "all" else ()):
        assert m[k] > 0, (k, m)
    for k in ("cap_samples", "shadow_rays", "overflows"):
        assert g[k] == 0, k
    oc = c.oracle_counters()
    assert rough(oc) == 0                                                          # no rough surface in the small scene
    rem = exact(g, m, ("walk", which))
    bounded(g, rem, oc, ("walk", which))
    assert g["obj_hits"] > 0 and rem > 0 and (g["side_calls"] > 0 or which == "wave")


def test_walk_counters_stage_scene(oracle):
    """c on scene A (ray_sets.walk_rays_stage_scene: nests of water, glass and core, depths and intensities at their limits, dead
    slots), every eighth ray: the ledger and the bounds, in two arrangements.
    Scene A's torus is a machine element in an envelope and its nests hold pairs: the envelope test of such an element and the steps
    of a pair are booked once each, as the reference takes them, or the geometry exceeds the oracle's."""
    sc, node = R.shade_stage_scene()
    flat = sc.flatten()
    h = A.Handle(flat, device=0)
    try:
        rays = R.walk_rays_stage_scene(flat, node, REC["ray"])[::8].copy()
        rays["pixel"] = np.where(rays["pixel"] != DEAD, np.arange(len(rays)), DEAD)
        c = WalkCase(oracle, flat, h, rays)
        assert (rays["pixel"] == DEAD).any() and len(c.traced) > len(rays)
        a, b = c.run(passes=1, count_work=True), c.run(passes=32, private_limit=0, count_work=True)
        assert len(a["rays"]) == 0 and len(b["rays"]) == 0 and a["counters"] == b["counters"], (a["counters"], b["counters"])
        same_output(c.run(passes=1), a, WALK_QUEUES, "walk scene A")
        oc = c.oracle_counters()
        assert rough(oc) > 0                                                       # scene A has a rough surface: its term is in the model
        rem = exact(a["counters"], c.ledger, "walk scene A", geometry_transc=rough(oc))
        bounded(a["counters"], rem, oc, "walk scene A")
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# e: isolation

def test_stage_calls_leave_the_render_counters_alone(oracle):
    sc, flat = R.walk_small_scene()
    h = A.Handle(flat, count_work=True)
    try:
        h.render_positions(A.main_pass_positions(flat.params.image_width, flat.params.image_height))
        before = h.last_counters_raw(10)
        assert before[8] > 0 and before[3] > 0                                     # flop, lum calls of the frame
        rays = R.walk_rays_small_scene(flat, REC["ray"])[:200].copy()
        room = len(W.ledger(oracle, flat, rays, REC)[1]) + len(rays)
        for count_work in (True, False):
            w = h.run_stage_walk(rays, room_rays=room, stack_cap=STACK, count_work=count_work)
            assert h.last_counters_raw(10) == before
            tasks = w["tasks"][np.concatenate(w["idx"])].copy()
            tasks["pixel"] = np.arange(len(tasks))
            s = h.run_stage("shade", tasks, cls=2, count_work=count_work)
            assert h.last_counters_raw(10) == before
            assert ("counters" in s) == count_work
            if count_work:
                assert s["counters"]["cap_samples"] > 0 and w["counters"]["lum_calls"] > 0
                assert h.stage_last_counters() == s["counters"]
            else:
                assert not any(h.stage_last_counters().values())                   # a plain stage call reports zeros, not the call before
    finally:
        h.close()
