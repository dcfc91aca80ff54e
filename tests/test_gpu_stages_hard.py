"""The hard-ray kernels one at a time (acn_run_stage: the production k_hard_shadow and k_hard_path on queues the test wrote) against the
oracle, ray by ray.  The records are real: hit records of the oracle go through ACN_STAGE_SHADE_HITS, the tasks that makes through
ACN_STAGE_SHADE, and what the two kernels append -- shadow rays and path rays with k_shade's resume words, probes with none -- is
what the queues here are laid out from, with seeded probes and dead slots mixed in (tests/hard_queues.py: the layouts and the list
states they are there for).  Pixel sums are 2^-40 fixed point, so accum is compared to the word."""
import os

import numpy as np
import pytest

import actinon_amd as A
import hard_queues as Q
import ray_sets as R
import shade_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REC = A.Handle.STAGE_RECORDS
QC = A.Handle.QC
INVALID = A.Handle.STAGE_INVALID
F3_BIG = 1.7976931348623157e308
RESUME_FLAG = 2
N_PIXELS = 97               # several records per pixel: the sums are sums


def as_bytes(a):
    a = np.ascontiguousarray(a)
    return np.sort(a.view(np.dtype((np.void, a.dtype.itemsize))).reshape(-1))


def same_records(got, want, what):
    g, w = as_bytes(got), as_bytes(want)
    assert len(g) == len(w), (what, len(g), len(w))
    assert (g == w).all(), (what, int((g != w).sum()))


def rays_of(q):
    return np.concatenate([q["pos"], q["d"]], axis=1)


class Pools:
    """the records of one scene, each class with what the oracle says about every record"""

    def __init__(self, name, oracle):
        rng = np.random.default_rng(41)
        self.name, self.oracle = name, oracle
        if name == "stage_a":
            sc, node = R.shade_stage_scene(direct_samples=16, path_samples=16)
            self.flat = sc.flatten()
            hits = R.stage_base_hits(oracle, self.flat, node, REC["hit"])
        else:
            self.flat = A.Flat.load(os.path.join(HERE, "golden", "scenes", name + ".npz"), direct_samples=16, path_samples=16)
            prm = self.flat.params
            eye, view = np.array(list(prm.camera_position)), R.unit(np.array(list(prm.camera_view_direction)))
            hits = []
            balls = self.envelope_balls()
            for k in range(240):
                # half of the rays at the envelopes of the root's elements (the lamp's CSG parts): shading points whose rays are hard
                c, r = balls[k % len(balls)]
                d = R.unit(view + rng.normal(size=3) * 0.2) if k % 2 else R.unit(c + R.random_dirs(rng, 1)[0] * (r * rng.random()) - eye)
                a, nor, ex, en = oracle.trans_hit(self.flat, eye, d)
                if a < np.inf:
                    hits.append(R._hit(REC["hit"], eye, d, a, nor, ex, en, int(prm.trace_depth), 1.0, rng.uniform(0.2, 1.0, 3)))
        flat = self.flat
        self.h = A.Handle(flat, device=0)
        hits = np.array(hits, dtype=REC["hit"])
        assert len(hits) >= 24, len(hits)
        # once more at four times trace_min_intensity: the specular children of those are born dead and become probes
        dim = hits.copy()
        dim["intensity"] = 4.0 * flat.params.trace_min_intensity
        hits = np.concatenate([hits, dim])
        hits["pixel"] = np.arange(len(hits))
        split = self.h.run_stage("shade_hits", hits)
        tasks = split["tasks"][np.concatenate(split["idx"])]
        tasks = tasks[:96].copy()
        tasks["pixel"] = np.arange(len(tasks))
        assert len(tasks) >= 12, len(tasks)
        shade = self.h.run_stage("shade", tasks, cls=1)
        assert split["flags"] & ~8 == 0 and shade["flags"] & ~8 == 0
        resumed, walk_probes, self.paths = shade["hard_shadow"], split["hard_shadow"], shade["hard_path"]
        assert (resumed["pad"] & 3 == RESUME_FLAG).all() and (walk_probes["pad"] == 1).all() and (self.paths["resume"] & 3 == RESUME_FLAG).all()
        # seeded probes: from points on the objects (the hits) and off them, in random directions.  A third asks for any finite hit, as
        # the probes of the walk do (in a closed room every one of them ends at a wall, in line); the others have a short limit, so
        # that a probe that starts on a CSG object -- inside its envelope -- is left for that object's machine
        on = R.ray_pos(hits["p"], hits["d"], hits["offs"])
        centre, spread = on.mean(axis=0), on.std(axis=0).max() + 1.0
        n_seed = 900
        seeded = np.zeros(n_seed, dtype=REC["hard_shadow"])
        balls = self.envelope_balls()
        pick = rng.integers(len(balls), size=n_seed)
        inside = np.array([balls[k][0] for k in pick]) + R.random_dirs(rng, n_seed) * (np.array([balls[k][1] for k in pick]) * rng.random(n_seed))[:, None]
        where = rng.random(n_seed)[:, None]                                    # half inside an element's envelope: its pre-test passes
        seeded["pos"] = np.where(where < 0.5, inside, np.where(where < 0.8, on[rng.integers(len(on), size=n_seed)], centre + rng.normal(size=(n_seed, 3)) * spread))
        seeded["d"] = R.random_dirs(rng, n_seed)
        seeded["limit"] = np.where(rng.random(n_seed) < 0.33, F3_BIG, rng.uniform(0.02, 0.5, n_seed) * spread)
        seeded["contrib"] = rng.uniform(0.0, 1.0, (n_seed, 3))
        seeded["pad"] = 1
        shadow = np.concatenate([resumed, walk_probes, seeded])
        # what the oracle says: occluded by the matter root, or (pad bit 0) by the light root, within the record's limit
        lr, mr = flat.c.light_root, flat.c.matter_root
        rays, lim = rays_of(shadow), shadow["limit"]
        occ = oracle.query_rays(flat, "occluded", mr, rays, limits=lim)[:, 5] != 0
        occ_light = oracle.query_rays(flat, "occluded", lr, rays, limits=lim)[:, 5] != 0
        self.occluded = occ | (occ_light & (shadow["pad"] & 1 != 0))
        # which probes the fill phase finishes, by the device's own in-line pass over each root (acn_query_rays: column 1 its answer,
        # column 3 its candidate word): this only sorts the records into the layouts' classes; what is expected comes from the oracle
        fm = self.h.query_rays("occluded", mr, rays, limits=lim)
        fl = self.h.query_rays("occluded", lr, rays, limits=lim)
        probe = shadow["pad"] & RESUME_FLAG == 0
        light_first = probe & (shadow["pad"] & 1 != 0)
        untouched = light_first & (fl[:, 1] == 2)                         # a machine element of the light root: both roots in full
        finished = probe & ~untouched & ((light_first & (fl[:, 1] == 1)) | (fm[:, 1] != 2))
        self.shadow = shadow
        self.cls = np.where(finished, "f", "s")
        self.word = np.where(probe & ~finished & ~untouched, (fm[:, 3].astype(np.uint64) << np.uint64(2)) | np.uint64(RESUME_FLAG) | (shadow["pad"] & 1),
                             shadow["pad"]).astype(np.uint32)               # pad as the kernel leaves it
        self.rng = rng
        print(f"{name}: {len(resumed)} resumed records, {len(walk_probes)} probes of the split, {n_seed} seeded probes: "
              f"{int(finished.sum())} finished in the fill phase, {int((probe & ~finished).sum())} left for a machine, {int(self.occluded.sum())} occluded; "
              f"{len(self.paths)} path records")
        # every class of record is there (a queue repeats the records of its class, each time under another pixel), and the 63-element
        # root has words with the tail bit (bit 31 of the record's word: candidates at positions >= 29)
        assert (self.cls[probe] == "f").sum() >= 100 and (self.cls[probe] == "s").sum() >= 16 and len(resumed) >= 16 and len(self.paths) >= 40
        tails = int(((self.word[self.cls == "s"] >> 31) & 1).sum())
        print(f"{name}: {tails} words with the tail bit")
        assert tails > 0 or name != "hanging_lamp"

    def envelope_balls(self):
        """( centre, radius ) of the envelopes of the matter root's elements"""
        els = [e for e in self.flat.elems_of(self.flat.c.matter_root) if self.flat.node(e).flags & 1]
        return [R.node_ball(self.flat, e) for e in els]

    def queue(self, layout, resumed_only=False):
        """a hard-shadow queue of the layout's classes, records drawn in turn from the pools; returns (queue, index into the pool or -1)"""
        pick = {"s": np.flatnonzero((self.cls == "s") & ((self.shadow["pad"] & RESUME_FLAG != 0) | (not resumed_only))),
                "f": np.flatnonzero(self.cls == "f")}
        pick = {k: self.rng.permutation(v) for k, v in pick.items()}
        used = {"s": 0, "f": 0}
        src = np.full(len(layout), -1)
        for i, c in enumerate(layout):
            if c != "d":
                src[i] = pick[c][used[c] % len(pick[c])]
                used[c] += 1
        q = np.zeros(len(layout), dtype=REC["hard_shadow"])
        q[src >= 0] = self.shadow[src[src >= 0]]
        q["pixel"] = np.where(src >= 0, np.arange(len(layout)) % min(N_PIXELS, len(layout)), INVALID)
        # a dead slot holds whatever was there: nothing of it may be read
        q["pos"][src < 0] = np.nan
        q["pad"][src < 0] = 0xFFFFFFFF
        return q, src

    def close(self):
        self.h.close()


@pytest.fixture(scope="module", params=["stage_a", "hanging_lamp"])
def pools(request, oracle):
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"
    p = Pools(request.param, oracle)
    yield p
    p.close()


def check_shadow(p, layout, grid=0, resumed_only=False):
    q, src = p.queue(layout, resumed_only)
    out = p.h.run_stage("hard_shadow", q, grid=grid)
    live = src >= 0
    want = np.zeros((len(q), 3), dtype=np.int64)
    add = live & ~np.where(live, p.occluded[src], True)
    np.add.at(want, q["pixel"][add], M.to_fixed(q["contrib"][add]))
    assert out["flags"] == 0, out["flags"]
    bad = np.flatnonzero((out["accum"] != want).any(axis=1))
    assert len(bad) == 0, (p.name, len(bad), bad[:8])
    c = out["counts"]
    assert c[A.abi.QS_DEAD_HS] == int((~live).sum()) and c[QC["hard_shadow"]] == len(q)
    # the queue as the kernel leaves it: a probe left for a machine has its resume word, everything else is untouched
    after = out["hard_shadow"]
    assert np.array_equal(after["pad"][live], p.word[src[live]]), p.name
    for f in q.dtype.names:
        if f != "pad":
            assert after[f][live].tobytes() == q[f][live].tobytes(), (p.name, f)
    return int(add.sum())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129])
def test_shadow_live_records(pools, n):
    """n live records with resume words and nothing else: the wave that draws the last slots works a partly filled list off"""
    assert Q.trace(Q.layout_live(n))["machine_lanes"] == Q.machine_steps_of(n)
    check_shadow(pools, Q.layout_live(n), grid=1, resumed_only=True)


@pytest.mark.parametrize("case", list(Q.LAYOUTS))
def test_shadow_layouts(pools, case):
    """the short layouts: whichever waves draw their batches, dead slots are dropped, finished probes add their term in the fill phase
    (all_finished_in_fill: no machine phase at all) and a last batch of fewer than 64 slots ends in a partial machine phase"""
    check_shadow(pools, Q.LAYOUTS[case], grid=1)


def test_shadow_list_states_on_one_workgroup(pools):
    """32 groups of 256 slots on ONE workgroup: every wave draws whole groups (n = 8192: balanced_batch is 256), and each group takes
    its wave through 63 pending + a batch of 64 survivors (127 in the list), a batch of 64 dead slots between live ones, 63 of 64
    dead, and two full machine phases that leave nothing pending -- so the next group meets the same states"""
    t = Q.trace(Q.GROUP_256)
    assert t["max_pending"] == 127 and t["left"] == 0
    added = check_shadow(pools, Q.GROUP_256 * Q.GROUPS, grid=1)
    assert added > 0


def test_shadow_every_record_resumable_and_mixed(pools):
    """4096 + 37 slots with every second reservation half dead, on the grid the seam chooses (17 workgroups): once with k_shade's records
    alone, once with probes of every kind in the live slots"""
    layout = Q.half_dead_reservations(4096 + 37)
    check_shadow(pools, layout, resumed_only=True)
    mixed = "".join(c if c == "d" else ("f" if (7 * i) % 5 < 2 else "s") for i, c in enumerate(layout))
    check_shadow(pools, mixed)


# ---------------------------------------------------------------------------------------------------------------------
# k_hard_path

def check_path(p, layout, grid=0):
    flat, prm = p.flat, p.flat.params
    n = len(layout)
    live = np.array([c != "d" for c in layout])
    q = np.zeros(n, dtype=REC["hard_path"])
    q[live] = p.paths[np.arange(int(live.sum())) % len(p.paths)]
    q["pixel"] = np.where(live, np.arange(n) % min(N_PIXELS, n), INVALID)
    q["pos"][~live] = np.nan
    q["resume"][~live] = 0xFFFFFFFF
    out = p.h.run_stage("hard_path", q, grid=grid)
    a, nor, ex, en = p.oracle.trans_hits(flat, flat.c.matter_root, rays_of(q[live]))
    hit = a < prm.max_path_length
    src = q[live]
    want = np.zeros(int(hit.sum()), dtype=REC["hit"])
    s = src[hit]
    want["p"], want["d"], want["offs"], want["exit_nor"], want["T"], want["intensity"] = s["pos"], s["d"], a[hit], nor[hit], s["T"], s["intensity"]
    want["exit_obj"], want["enter_obj"], want["depth"], want["pixel"] = ex[hit], en[hit], s["depth"], s["pixel"]
    assert out["flags"] == 0
    same_records(out["children"], want, (p.name, "children"))
    # the miss terms: T * ( background * intensity ), one fixed-point word each
    bg = np.array(list(prm.background_color))
    acc = np.zeros((n, 3), dtype=np.int64)
    m = src[~hit]
    np.add.at(acc, m["pixel"], M.to_fixed(m["T"] * (bg[None, :] * m["intensity"][:, None])))
    assert np.array_equal(out["accum"], acc), p.name
    c = out["counts"]
    assert c[QC["s_children"]] == int(hit.sum()) and c[QC["children"]] - c[QC["dead_c"]] == int(hit.sum())
    return int(hit.sum()), int((~hit).sum())


@pytest.mark.parametrize("case", ["1", "63", "65", "129", "63_pending_then_64", "dead_batch_between", "63_of_64_dead", "partial_last_batch"])
def test_path_layouts(pools, case):
    layout = Q.layout_live(int(case)) if case.isdigit() else Q.LAYOUTS[case].replace("f", "s")
    check_path(pools, layout, grid=1)


def test_path_list_states_and_half_dead_reservations(pools):
    hits, misses = check_path(pools, Q.GROUP_256 * Q.GROUPS, grid=1)
    h2, m2 = check_path(pools, Q.half_dead_reservations(4096 + 37))
    print(f"{pools.name}: hard path {hits} + {h2} hits, {misses} + {m2} misses")
    assert hits > 0 and h2 > 0


def test_refusals_of_the_hard_stages(pools):
    q, _ = pools.queue("ssss")
    for field, value in (("pixel", 4), ("limit", 0.0), ("limit", np.nan), ("pad", 3), ("pad", 4)):
        bad = q.copy()
        bad[field][3] = value
        with pytest.raises(A.AcnError) as e:
            pools.h.run_stage("hard_shadow", bad)
        assert e.value.status == A.abi.ACN_ERR_ARG, field
    bad = q.copy()
    bad["d"][3] = np.inf
    with pytest.raises(A.AcnError):
        pools.h.run_stage("hard_shadow", bad)
    with pytest.raises(A.AcnError):
        pools.h.run_stage("hard_shadow", q, grid=65)
    hp = pools.paths[:4].copy()
    hp["pixel"] = np.arange(4)
    for field, value in (("pixel", 9), ("depth", -1), ("resume", 7)):
        bad = hp.copy()
        bad[field][3] = value
        with pytest.raises(A.AcnError) as e:
            pools.h.run_stage("hard_path", bad)
        assert e.value.status == A.abi.ACN_ERR_ARG, field
