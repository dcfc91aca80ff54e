"""The shading kernels one at a time (acn_run_stage: the production k_shade_hits and k_shade on queues the test wrote) against the
oracle's tap (acn_oracle_shade_point: scene_lum for one hit, recorded while it runs) and tests/shade_model.py (what the device does
differently: colours carried down, probes, the closed-form Oren-Nayar weight, the fixed-point sum).  Records are compared bit for bit;
what no record carries is seen through accum, exactly where a sum has one term and within a derived bound elsewhere."""
import numpy as np
import pytest

import actinon_amd as A
import ray_sets as R
import shade_model as M

pytestmark = pytest.mark.gpu

REC = A.Handle.STAGE_RECORDS
QC = A.Handle.QC
INVALID = A.Handle.STAGE_INVALID
ACN_FLAG_CLAMPED = 8
ACN_RESUME_PROBE = 1          # HardShadow.pad bit 0: a probe of a specular ray


def as_bytes(a):
    """the records of a queue as sorted raw bytes: queues are unordered, records have no padding"""
    a = np.ascontiguousarray(a)
    v = a.view(np.dtype((np.void, a.dtype.itemsize))).reshape(-1)
    return np.sort(v)


def same_records(got, want, what):
    g, w = as_bytes(got), as_bytes(np.array(want, dtype=got.dtype) if len(want) else np.zeros(0, dtype=got.dtype))
    assert len(g) == len(w), (what, len(g), len(w))
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, (what, len(bad), got[:0].dtype.names)


class Stage:
    def __init__(self, oracle, pair_light):
        self.sc, self.node = R.shade_stage_scene(pair_light=pair_light)
        self.flat = self.sc.flatten()
        self.h = A.Handle(self.flat, device=0)
        self.oracle = oracle
        self.info = self.h.stage_info()
        self.prm = self.flat.params

    def tap(self, recs):
        return [self.oracle.shade_point(self.flat, M.tap_input(r))[0] if r["pixel"] != INVALID else np.zeros((0, 16)) for r in recs]


@pytest.fixture(scope="module")
def stage_a(oracle):
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"
    s = Stage(oracle, False)
    yield s
    s.h.close()


@pytest.fixture(scope="module")
def stage_b(oracle):
    s = Stage(oracle, True)
    yield s
    s.h.close()


def test_record_layouts(stage_a, stage_b):
    """the numpy dtypes are the library's records, and the two scenes select the two light variants of k_shade"""
    for k, dt in REC.items():
        assert dt.itemsize == stage_a.info["sizeof"][k], k
    assert stage_a.info["counter_words"] == 104 and stage_a.info["lights"] == 2 and stage_b.info["lights"] == 3
    assert stage_a.info["leaf_lights"] and not stage_b.info["leaf_lights"]
    assert stage_a.info["nodes"] == stage_a.flat.n_nodes


def test_refusals_before_any_launch(stage_a):
    h = stage_a.h
    hit = np.zeros(4, dtype=REC["hit"])
    hit["pixel"] = np.arange(4); hit["enter_obj"] = -1; hit["exit_obj"] = -1
    for field, value in (("pixel", 4), ("depth", -1), ("depth", A.abi.ACN_STAGE_MAX_DEPTH + 1), ("enter_obj", stage_a.flat.n_nodes), ("exit_obj", -2)):
        bad = hit.copy()
        bad[field][3] = value
        with pytest.raises(A.AcnError) as e:
            h.run_stage("shade_hits", bad)
        assert e.value.status == A.abi.ACN_ERR_ARG, field
    task = np.zeros(4, dtype=REC["task"])
    task["pixel"] = np.arange(4); task["diffuse_intensity"] = 0.1
    for kw, field, value in (({"cls": 4}, None, None), ({"shard_rank": 2, "shard_world": 2}, None, None), ({"index": [0, 4]}, None, None),
                             ({}, "pixel", 4), ({}, "depth", -1), ({}, "diffuse_intensity", np.nan), ({}, "diffuse_intensity", 1e9)):
        bad = task.copy()
        if field:
            bad[field][3] = value
        with pytest.raises(A.AcnError) as e:
            h.run_stage("shade", bad, **kw)
        assert e.value.status == A.abi.ACN_ERR_ARG, (kw, field)
    # a dead input slot is not read further
    hit["pixel"][3] = INVALID; hit["depth"][3] = -5
    out = h.run_stage("shade_hits", hit)
    assert out["flags"] == 0 and not out["accum"].any()


# ---------------------------------------------------------------------------------------------------------------------
# the split: shade_hit as k_shade_hits launches it

@pytest.fixture(scope="module")
def split(stage_a):
    recs = R.stage_split_hits(stage_a.oracle, stage_a.flat, stage_a.node, REC["hit"])
    rows = stage_a.tap(recs)
    return recs, rows, stage_a.h.run_stage("shade_hits", recs)


def test_split_bit_for_bit(stage_a, split):
    """~2 000 hit records through k_shade_hits: the ray queue, the probes, the tasks, the class lists, the statistics and accum equal
    the tap's rows with the model's colours, to the bit"""
    recs, rows, out = split
    assert 1500 <= len(recs) <= 2600
    want_rays, want_probes, want_tasks, want_acc = [], [], [], np.zeros((len(recs), 3), dtype=np.int64)
    for i, (r, rw) in enumerate(zip(recs, rows)):
        rays, probes, task, acc = M.split_expected(rw, r, stage_a.prm, REC)
        want_rays += rays; want_probes += probes
        if task is not None:
            want_tasks.append(task)
        if r["pixel"] != INVALID:
            want_acc[r["pixel"]] = acc
    print(f"split: {len(recs)} hit records -> {len(want_rays)} rays, {len(want_probes)} probes, {len(want_tasks)} tasks, "
          f"{int((want_acc != 0).any(axis=1).sum())} emission terms, {int((recs['pixel'] == INVALID).sum())} dead slots")
    assert len(want_rays) > 300 and len(want_probes) > 100 and len(want_tasks) > 300
    same_records(out["rays"], want_rays, "rays")
    same_records(out["hard_shadow"], want_probes, "probes")
    assert (out["hard_shadow"]["pad"] == ACN_RESUME_PROBE).all()
    listed = np.concatenate(out["idx"])
    assert len(np.unique(listed)) == len(listed) == len(want_tasks)
    same_records(out["tasks"][listed], want_tasks, "tasks")
    # which class list each task is in
    def cls_of(t):
        nd = max(int(stage_a.prm.direct_samples * t["diffuse_intensity"]), 1)
        npth = max(int(stage_a.prm.path_samples * t["diffuse_intensity"]), 1) if t["depth"] > 10 else 0
        return M.size_class(max(nd, npth), stage_a.info["class0_min"])
    for k in range(4):
        assert all(cls_of(t) == k for t in out["tasks"][out["idx"][k]]), k
    want_cls = np.bincount([cls_of(t) for t in want_tasks], minlength=4)
    assert [len(l) for l in out["idx"]] == list(want_cls) and (want_cls > 0).all(), (want_cls, stage_a.info)
    # the statistics are the numbers of records; nothing overflowed, the one clamp is the point at a light's pos
    c = out["counts"]
    assert c[QC["s_probes"]] == len(want_probes) and c[QC["tasks"]] - c[QC["dead_t"]] == len(want_tasks)
    assert c[QC["s_tasks"]] == 0                                                  # (no kernel writes QS_TASKS: the tasks are mark - dead, above)
    assert c[QC["gen0"]] - c[QC["dead_r"]] == len(want_rays)
    assert out["flags"] == ACN_FLAG_CLAMPED
    assert np.array_equal(out["accum"], want_acc)
    assert (np.abs(want_acc).max(axis=1) == 16384 << 40).sum() >= 1


def test_split_without_emit_terms(stage_a, split):
    """a shard rank > 0 of a sample-sharded call (emit_terms 0) drops exactly the probes' terms: everything else is written as before"""
    recs, rows, out = split
    quiet = stage_a.h.run_stage("shade_hits", recs, emit_terms=False)
    assert len(quiet["hard_shadow"]) == 0 and quiet["counts"][QC["s_probes"]] == 0 and len(out["hard_shadow"]) > 0
    same_records(quiet["rays"], list(out["rays"]), "rays")
    same_records(quiet["tasks"][np.concatenate(quiet["idx"])], list(out["tasks"][np.concatenate(out["idx"])]), "tasks")
    assert np.array_equal(quiet["accum"], out["accum"])


# ---------------------------------------------------------------------------------------------------------------------
# the sample loops: k_shade< LPT > for every lane width

class Samples:
    """the tasks of the sample test with what the tap says about every sample"""

    def __init__(self, st, detmath):
        self.st = st
        # the hand-made shading points, then the split's own tasks; the path_limit expectations hold for scene A, whose draws they were found on
        self.hits, self.labels, self.expect = R.stage_sample_hits(st.flat, st.node, REC["hit"], oracle=st.oracle)
        if "pair_light" in st.node:
            self.expect = {}
        self.rows = st.tap(self.hits)
        self.tasks = np.array([M.task_of(rw, r, REC) for r, rw in zip(self.hits, self.rows)], dtype=REC["task"])
        self.detmath = detmath
        self.counts = [M.sample_counts(rw) for rw in self.rows]

    def run(self, **kw):
        return self.st.h.run_stage("shade", self.tasks, **kw)


@pytest.fixture(scope="module")
def samples_a(stage_a, detmath_cpu):
    return Samples(stage_a, detmath_cpu)


@pytest.fixture(scope="module")
def samples_b(stage_b, detmath_cpu):
    return Samples(stage_b, detmath_cpu)


def by_pixel(q, n):
    order = np.argsort(q["pixel"], kind="stable")
    q = q[order]
    cut = np.searchsorted(q["pixel"], np.arange(n + 1))
    return [q[cut[i]:cut[i + 1]] for i in range(n)]


def group(q, field):
    """the records of a task by the bits of a direction"""
    g = {}
    for c in q:
        g.setdefault(bits(c[field]).tobytes(), []).append(c)
    return g


def take(g, k):
    """one record of direction k, or None"""
    if k not in g:
        return None
    c = g[k].pop()
    if not g[k]:
        del g[k]
    return c


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def check_against_tap(sm, out, shard=(0, 1)):
    """Every record of every task against the tap's row of the same sample (matched through the bits of out_d), every sample of the
    sequential stream accounted for once, and accum against the sum of what no record carries.  Returns the counts compared."""
    st, prm = sm.st, sm.st.prm
    n = len(sm.tasks)
    bg = np.array(list(prm.background_color))
    tmin, max_len = prm.trace_min_intensity, prm.max_path_length
    path_limit = np.nextafter(max_len, 0.0)
    ch, hp, hs = by_pixel(out["children"], n), by_pixel(out["hard_path"], n), by_pixel(out["hard_shadow"], n)
    tally = {"children": 0, "hard_path": 0, "hard_shadow": 0, "probes": 0, "inline": 0, "background": 0, "exact_accum": 0, "plain_weight": 0,
             "limit_cases": 0}
    for i, (t, rows) in enumerate(zip(sm.tasks, sm.rows)):
        key = lambda d: bits(d).tobytes()                                          # noqa: E731
        lights, direct, path = M.rows_of(rows, "light"), M.rows_of(rows, "direct"), M.rows_of(rows, "path")
        n_direct, n_path = sm.counts[i]
        # (two samples may have the same direction to the bit -- a cone 1e6 radii away, the zero cone of a plane seen from behind --
        # and then the same fate: records are matched one for one)
        lum = np.zeros(3)
        hidden = 0
        if not t["on_b"] > 0:
            tally["plain_weight"] += 1                                             # no Oren-Nayar term: the raw weight everywhere
        hs_of = group(hs[i], "d")
        for h in hs[i]:
            assert np.array_equal(bits(h["pos"]), bits(t["pos"]))
        # -- direct samples
        for li in lights:
            nd, lp = int(li[6]), np.array(list(st.flat.node(int(li[1])).pos))
            lo, hi = M.shard_range(nd, *shard)
            norm = 2.0 * li[2] / nd
            scale = t["Tc"] * (li[3:6] * norm)
            rs = direct[(direct[:, 2] == li[1]) & (direct[:, 1] >= lo) & (direct[:, 1] < hi)]
            assert len(rs) == hi - lo
            live = rs[(rs[:, 6] > 0) & (rs[:, 7] < np.inf)]
            w = M.closed_weight(sm.detmath, live[:, 6], t["theta_i"], t["on_a"], t["on_b"], live[:, 3:6], t["surface_d"], t["ray_projection"])
            s = 0.0
            for r, wc in zip(live, w):
                ray = r[3:6]
                hit_pos = t["pos"] + ray * r[7]
                dv = hit_pos - lp
                dsq = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]
                local = st.flat.node(int(li[1])).radiance / dsq if dsq > 0 else 1e30
                if r[9] == 0:
                    assert local == r[10]                                          # the oracle's own local_intensity
                c = local * wc * t["diffuse_intensity"]
                h = take(hs_of, key(ray))
                if h is not None:
                    assert h["limit"] == r[7] and not (h["pad"] & ACN_RESUME_PROBE)
                    assert np.array_equal(bits(h["contrib"]), bits(scale * c)), (i, sm.labels[i], h["contrib"], scale * c)
                    tally["hard_shadow"] += 1
                elif r[9] == 0:
                    s += c                                                         # decided in line, unoccluded: only accum shows it
                    tally["inline"] += 1
                    hidden += 1
            # (weight <= 0 or a miss of the light: no record -- whatever is left in hs_of at the end belongs to no sample)
            lum = lum + li[3:6] * (s * norm)
        # -- path samples
        terms = 0
        if n_path:
            lo, hi = M.shard_range(n_path, *shard)
            norm = 2.0 / n_path
            scale = t["Tc"] * norm
            rs = path[(path[:, 1] >= lo) & (path[:, 1] < hi)]
            assert len(rs) == hi - lo
            ch_of, hp_of = group(ch[i], "d"), group(hp[i], "d")
            assert not (set(ch_of) & set(hp_of))
            bsum = 0.0
            for r in rs:
                k = key(r[2:5])
                if not r[5] > 0:
                    continue
                child_i = r[13]
                dark = t["depth"] - 10 == 0 or child_i < tmin
                kind = "none"
                if k in ch_of:
                    kind = "child"
                    c = take(ch_of, k)
                    assert not dark and r[7] < max_len
                    assert c["offs"] == r[7] and np.array_equal(bits(c["exit_nor"]), bits(r[8:11])) and c["exit_obj"] == r[11] and c["enter_obj"] == r[12]
                    assert bits(c["intensity"]) == bits(child_i) and c["depth"] == t["depth"] - 10
                    assert np.array_equal(bits(c["T"]), bits(scale)) and np.array_equal(bits(c["p"]), bits(t["pos"]))
                    tally["children"] += 1
                elif k in hp_of:
                    kind = "hard_path"
                    c = take(hp_of, k)
                    assert not dark
                    assert bits(c["intensity"]) == bits(child_i) and c["depth"] == t["depth"] - 10
                    assert np.array_equal(bits(c["T"]), bits(scale)) and np.array_equal(bits(c["pos"]), bits(t["pos"]))
                    tally["hard_path"] += 1
                elif k in hs_of:
                    kind = "probe"
                    h = take(hs_of, k)                                             # a dark ray that needs the machine: a probe for the background term
                    assert dark and h["limit"] == path_limit and not (h["pad"] & ACN_RESUME_PROBE)
                    assert np.array_equal(bits(h["contrib"]), bits(scale * (bg * child_i)))
                    tally["probes"] += 1
                else:
                    # decided in line: a miss adds the background term; a hit is dark (or the probe's in-line elements hit already)
                    assert dark or not r[7] < max_len, (i, sm.labels[i], r)
                    if not r[7] < max_len:
                        kind = "bsum"
                        bsum += child_i
                        terms += 1
                        tally["background"] += 1
                # a path hit at max_path_length, its predecessor, its successor (ray_sets.stage_limit_cases): what the kernel makes of it
                case = sm.expect.get((i, int(r[1])))
                if case is not None and shard == (0, 1):
                    assert r[7] == case["target"] and kind == case["kind"], (i, case["group"], case["target"], r[7], kind, case["kind"])
                    tally["limit_cases"] += 1
            assert not ch_of and not hp_of, (i, sm.labels[i], len(ch_of), len(hp_of))   # every record is a sample of this rank's share
            lum = lum + bg * (bsum * norm)
        assert not hs_of, (i, sm.labels[i], len(hs_of))                           # every deferred-shadow record is a sample of this rank's share
        # no task has more than a tenth of its direct samples where only a sum of several terms shows them (a sum of one term shows it)
        if hidden + terms > 1:
            assert hidden <= 0.1 * n_direct * len(lights), (i, sm.labels[i], hidden, n_direct)
        # -- accum: Tc * lum.  One term per sum at most: exact.  Else every sum of m terms t_k >= 0 is off by at most ( m - 1 ) 2^-53
        # sum( t_k ) in either order of adding (the lanes' partial sums, then the butterfly), the model's own sum as much again; norm, colour,
        # Tc and the three adds of lum are 8 more roundings of 2^-53 relative; to_fixed rounds once: 2^-41, and the bound is in units of 2^-40
        want = M.to_fixed(t["Tc"] * lum)
        got = out["accum"][i]
        m = max(n_direct, n_path)
        if n_direct == 1 and n_path <= 1:
            assert np.array_equal(got, want), (i, sm.labels[i], got, want)
            tally["exact_accum"] += 1
        else:
            bound = 2 * (m + 8) * 2.0 ** -53 * np.abs(t["Tc"] * lum) * 2.0 ** 40 + 1
            assert (np.abs(got - want) <= bound).all(), (i, sm.labels[i], got, want, bound)
    return tally


def test_sample_counts_cover_every_lane_width(samples_a):
    nd = {c[0] for c in samples_a.counts}
    npth = {c[1] for c in samples_a.counts}
    assert set(R.STAGE_N) <= nd and set(R.STAGE_N) <= npth and 0 in npth


@pytest.mark.parametrize("prune", [True, False], ids=["prune", "plain"])
def test_samples_identical_in_all_four_classes(samples_a, prune):
    """The same tasks on 64, 16, 4 and 1 lanes per task: the sets of HitRec, HardPath and HardShadow records are identical to the bit
    (lcg_jump_lane / lcg_stride give sample j the draw of the sequential stream), equal the tap's samples, and accum agrees."""
    outs = [samples_a.run(cls=c, prune=prune) for c in range(4)]
    for c, o in enumerate(outs):
        assert o["flags"] == 0, (c, o["flags"])                                  # nothing overflowed, nothing clamped
        for q in ("children", "hard_path", "hard_shadow"):
            assert len(o[q]) > 0, q
            same_records(o[q], list(outs[0][q]), (q, c))
        cnt = o["counts"]
        assert cnt[QC["s_children"]] == len(o["children"]) and cnt[QC["s_hard_path"]] == len(o["hard_path"]) and cnt[QC["s_hard_shadow"]] == len(o["hard_shadow"])
    tally = check_against_tap(samples_a, outs[0])
    print(f"samples (prune={prune}): {len(samples_a.tasks)} tasks x 4 classes: {tally}")
    assert all(v > 0 for v in tally.values()), tally
    assert tally["limit_cases"] == 6 and tally["plain_weight"] >= 40 and tally["plain_weight"] < len(samples_a.tasks) // 2
    for o in outs[1:]:
        # the classes add the same terms in another order: the bound of check_against_tap, between two device sums
        lim = 2 * (max(max(c) for c in samples_a.counts) + 8) * 2.0 ** -53 * np.abs(outs[0]["accum"]) + 2
        assert (np.abs(o["accum"] - outs[0]["accum"]) <= lim).all()
    light_sum = np.abs(outs[0]["accum"]).max(axis=1) / 2.0 ** 40
    assert light_sum.max() < 8000, light_sum.max()


def test_samples_sharded(samples_a):
    """shard_world = 3: the three ranks' records partition the unsharded set, each rank's records and sums are its share of the stream"""
    whole = samples_a.run(cls=1)
    parts = [samples_a.run(cls=k, shard_rank=k, shard_world=3) for k in range(3)]
    for q in ("children", "hard_path", "hard_shadow"):
        same_records(np.concatenate([p[q] for p in parts]), list(whole[q]), q)
    for k, p in enumerate(parts):
        check_against_tap(samples_a, p, shard=(k, 3))


def test_samples_generic_lights(samples_b):
    """scene B (a pair light with an envelope: k_shade< LEAF_LIGHTS = false >), and scene A's lights forced through the generic hit"""
    a = samples_b.run(cls=1)
    b = samples_b.run(cls=2)
    for q in ("children", "hard_path", "hard_shadow"):
        same_records(b[q], list(a[q]), q)
    tally = check_against_tap(samples_b, a)
    print(f"samples (pair light): {tally}")
    assert tally["hard_shadow"] > 0 and tally["children"] > 0


def test_samples_leaf_lights_forced_off(samples_a):
    a = samples_a.run(cls=1)
    b = samples_a.run(cls=1, leaf_lights=False)
    for q in ("children", "hard_path", "hard_shadow"):
        same_records(b[q], list(a[q]), q)
    assert np.array_equal(a["accum"], b["accum"])
