"""k_walk alone (acn_run_stage_walk: the passes of the production kernel in the pipeline runner's loop, on rays the test wrote) against
tests/walk_model.py, the walk as a worklist over the oracle.  The arrangement of the walk -- launches, private stacks, spills, fetch
batch, grid, kernel variant -- decides where a ray is traced, never what it produces: one expectation per scene, compared to the bit
under every arrangement, and the statistics the host planner reads wherever the model decides them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import ray_sets as R
import shade_model as M
import walk_model as W
from query_checks import upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = A.Handle.STAGE_RECORDS
QC = {**A.Handle.QC, **A.Handle.QC_WALK}
INVALID = A.Handle.STAGE_INVALID
ACN_FLAG_CLAMPED = 8
ACN_CHUNK_OVERFLOW = 1
# a private step pops at most 64 rays and pushes at most three children each, so a stack grows by at most 128 per step along a chain
# of at most trace_depth steps (25 here): 64 + 128 * 25 slots hold whatever the last pass meets, and nothing is left over
STACK = A.abi.ACN_STAGE_WALK_MAX_STACK
UNLIMITED = 0xFFFFFFFF


def as_bytes(a):
    """the records of a queue as sorted raw bytes: queues are unordered, records have no padding"""
    a = np.ascontiguousarray(a)
    return np.sort(a.view(np.dtype((np.void, a.dtype.itemsize))).reshape(-1))


def same_records(got, want, what):
    g, w = as_bytes(got), as_bytes(np.array(want, dtype=got.dtype) if len(want) else np.zeros(0, dtype=got.dtype))
    assert len(g) == len(w), (what, len(g), len(w))
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, (what, len(bad), got[:0].dtype.names)


class Case:
    """a scene, its handle, the input rays and the model's expectation, made once"""

    def __init__(self, name, oracle, flat, handle, rays):
        self.name, self.oracle, self.flat, self.h, self.rays = name, oracle, flat, handle, rays
        self.n = len(rays)
        self.live_in = int((rays["pixel"] != INVALID).sum())
        self.dead_in = self.n - self.live_in
        self.memo = {}
        self.model = W.walk(oracle, flat, rays, REC, memo=self.memo)
        self.room = self.model.rays + self.dead_in
        self.info = handle.stage_info()
        self.prm = flat.params
        print(f"{name}: {self.n} records ({self.dead_in} dead) -> {self.model.totals()}")

    def run(self, **kw):
        kw.setdefault("stack_cap", STACK)
        return self.h.run_stage_walk(self.rays, room_rays=self.room, **kw)

    def cls_of(self, t):
        nd = max(int(self.prm.direct_samples * t["diffuse_intensity"]), 1) if self.info["lights"] else 0
        npth = max(int(self.prm.path_samples * t["diffuse_intensity"]), 1) if self.prm.path_samples and t["depth"] > 10 else 0
        return M.size_class(max(nd, npth), self.info["class0_min"])


@pytest.fixture(scope="module")
def case_a(oracle):
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"
    sc, node = R.shade_stage_scene()
    flat = sc.flatten()
    c = Case("scene A", oracle, flat, A.Handle(flat, device=0), R.walk_rays_stage_scene(flat, node, REC["ray"]))
    yield c
    c.h.close()


@pytest.fixture(scope="module")
def case_w(oracle):
    sc, flat = R.walk_scene_wine_glass()
    c = Case("wine glass", oracle, flat, A.Handle(flat, device=0), R.walk_rays_wine_glass(flat, REC["ray"]))
    yield c
    c.h.close()


@pytest.fixture(scope="module")
def case_v(oracle):
    """the small scene, uploaded so that its handle runs k_walk< LDS, PRUNE >"""
    sc, flat = R.walk_small_scene()
    c = Case("small scene", oracle, flat, upload(flat, ACN_PRUNE_MIN=1), R.walk_rays_small_scene(flat, REC["ray"]))
    yield c
    c.h.close()


@pytest.fixture(scope="module", params=["scene A", "wine glass"])
def case(request, case_a, case_w):
    return case_a if request.param == "scene A" else case_w


def check(c, out, emit_terms=True, leftovers=False):
    """Everything a run wrote against the model.  What the last pass left over (out["rays"]) is continued by the model: the run's
    records and sums plus the continuation's are the full expectation, so no ray is lost and none is traced twice.  Returns the
    continuation."""
    m = c.model
    assert leftovers == (len(out["rays"]) > 0), (len(out["rays"]), out["gen"])
    rest = W.walk(c.oracle, c.flat, out["rays"], REC, n=c.n, emit_terms=emit_terms, memo=c.memo)
    listed = np.concatenate(out["idx"])
    assert len(np.unique(listed)) == len(listed) and (listed < len(out["tasks"])).all()
    tasks = out["tasks"][listed]
    same_records(np.concatenate([tasks, np.array(rest.tasks, dtype=REC["task"])]) if rest.tasks else tasks, m.tasks, "tasks")
    for k in range(4):
        assert all(c.cls_of(t) == k for t in out["tasks"][out["idx"][k]]), k
    c_ = out["counts"]
    assert c_[QC["tasks"]] - c_[QC["dead_t"]] == len(tasks)
    if emit_terms:
        probes = out["hard_shadow"]
        assert (probes["pad"] == 1).all() and (probes["limit"] == M.F3_BIG).all()
        same_records(np.concatenate([probes, np.array(rest.probes, dtype=REC["hard_shadow"])]) if rest.probes else probes, m.probes, "probes")
        assert np.array_equal(out["accum"] + rest.accum, m.accum)
        assert c_[QC["s_probes"]] == len(probes)
    else:
        assert len(out["hard_shadow"]) == 0 and c_[QC["s_probes"]] == 0 and c_[QC["hard_shadow"]] == 0 and not out["accum"].any()
    assert out["flags"] == (ACN_FLAG_CLAMPED if m.clamped and emit_terms else 0)
    assert c_[QC["walk_rays"]] + rest.rays == m.rays
    assert int(c_[QC["walk_steps"]]) * 64 >= int(c_[QC["walk_rays"]]) + c.dead_in
    return rest


# ---------------------------------------------------------------------------------------------------------------------

def test_layouts_and_kernel_variants(case_a, case_w, case_v):
    for c in (case_a, case_w, case_v):
        for k, dt in REC.items():
            assert dt.itemsize == c.info["sizeof"][k], k
        assert c.info["counter_words"] == 104
        assert c.n <= 2600 and c.n % 64 and c.model.generations + 1 <= A.abi.ACN_MAX_WALK_PASSES
    assert case_v.info["prune"] and case_v.info["lds_nodes"]
    assert not case_a.info["lds_nodes"] and not case_w.info["lds_nodes"]
    assert case_a.model.misses == 0 and case_w.model.misses >= 100 and case_a.model.emissions >= 300


def test_one_pass_all_private(case):
    """one launch: everything on the private stacks, default grid and fetch"""
    out = case.run(passes=1)
    check(case, out)
    c = out["counts"]
    assert c[QC["private_rays"]] == c[QC["walk_rays"]] == case.model.rays
    assert (out["gen"][1:] == 0).all()
    # the production stack of 512 slots: whatever it spills is left over, nothing is lost
    out = case.run(passes=1, stack_cap=512)
    check(case, out, leftovers=len(out["rays"]) > 0)


def test_every_generation_in_a_launch_of_its_own(case):
    """passes = generations + 1, private_limit 0: every generation goes through the global queues; the last launch has no input.  The
    generation marks are what acn_read_chunk and acn_walk_passes_seen read"""
    m = case.model
    g_n = m.generations
    out = case.run(passes=g_n + 1, private_limit=0)
    check(case, out)
    c, gen = out["counts"], out["gen"]
    assert gen[0] == case.n
    assert int(gen[1:].sum()) - int(c[QC["dead_r"]]) == m.rays - len(m.gens[0])
    for g in range(1, g_n + 2):
        want = len(m.gens[g]) if g < g_n else 0
        assert gen[g] >= want and (gen[g] == 0) == (want == 0), (g, gen[g], want)
    assert c[QC["private_rays"]] == 0 and c[QC["walk_rays"]] == m.rays
    # every launch worked its generation off: the cursor of a pass passed its mark
    for g in range(g_n):
        assert c[QC["cur_gen0"] + g] >= gen[g], g


@pytest.mark.parametrize("kw", [dict(passes=3, private_limit=1000, fetch=512), dict(passes=2, fetch=96), dict(passes=1, fetch=96),
                                dict(passes=2, private_limit=0, grid=1), dict(passes=2, private_limit=0, grid=3), dict(passes=1, grid=3)],
                         ids=["3_passes_limit_1000_fetch_512", "fetch_96", "fetch_96_private", "grid_1", "grid_3", "grid_3_private"])
def test_arrangements(case, kw):
    """three passes with a private limit in the middle of the generations' sizes; a fetch batch of 96, which leaves half-filled fetch
    ranges (steps mix a partial top-up with popped rays); one and three workgroups"""
    out = case.run(**kw)
    check(case, out)
    assert out["counts"][QC["walk_rays"]] == case.model.rays


def test_one_slot_stacks_spill(case):
    """stack_use 1 with an unlimited private limit: every pass but the last runs in private mode on stacks of one slot, so of the
    children of a step all but one spill into the next generation's queue.  A lineage whose ray stays on the stack is followed to its
    end within the pass, so the late generations of the model are finished early and their marks may be zero.  What a correct kernel
    must show: a step keeps at most one child on the stack, so all other rays beyond the input went through the spill queues; a pass
    without input spills nothing, so the non-zero marks have no gap; and generation 1 is not empty."""
    m = case.model
    g_n = m.generations
    out = case.run(passes=g_n + 1, private_limit=UNLIMITED, stack_use=1)
    check(case, out)
    c, gen = out["counts"], out["gen"]
    spilled = int(gen[1:].sum()) - int(c[QC["dead_r"]])
    print(f"{case.name}: marks with one-slot stacks {[int(v) for v in gen]}, {spilled} rays spilled of {m.rays - case.live_in}, {int(c[QC['walk_steps']])} steps")
    used = int(np.max(np.nonzero(gen)[0]))
    assert used >= 1 and (gen[:used + 1] > 0).all() and gen[g_n + 1] == 0
    assert m.rays - case.live_in >= spilled >= m.rays - case.live_in - int(c[QC["walk_steps"]]) and spilled > 0
    assert c[QC["private_rays"]] == c[QC["walk_rays"]] == m.rays


def test_private_limit_edge(case):
    """n_in <= private_limit: with the limit at the number of input slots pass 0 runs on the private stacks, one below it is a
    generation pass"""
    out = case.run(passes=2, private_limit=case.n)
    check(case, out)
    c = out["counts"]
    assert c[QC["private_rays"]] == c[QC["walk_rays"]] == case.model.rays and out["gen"][1] == 0
    out = case.run(passes=2, private_limit=case.n - 1)
    check(case, out)
    c = out["counts"]
    assert c[QC["walk_rays"]] == case.model.rays and c[QC["private_rays"]] == case.model.rays - case.live_in and out["gen"][1] > 0


def test_without_emit_terms(case):
    """emit_terms 0 (a shard rank > 0 of a sample-sharded call): no probes, no terms of the walk; tasks and lists as before"""
    for kw in (dict(passes=1), dict(passes=3, private_limit=200)):
        out = case.run(emit_terms=False, **kw)
        check(case, out, emit_terms=False)
        assert out["counts"][QC["walk_rays"]] == case.model.rays


@pytest.fixture(scope="module")
def read_chunk(tmp_path_factory):
    """acn_read_chunk of the host planner through the shim of tests/csrc/queueplan_cpu.cpp"""
    out = tmp_path_factory.mktemp("queueplan") / "libqueueplan_cpu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "actinon_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "queueplan_cpu.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.qp_read_chunk.restype, lib.qp_read_chunk.argtypes = None, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

    def read(counts, passes):
        c = np.array(counts, dtype=np.uint32)
        words, dead, p = np.zeros(32, dtype=np.uint64), C.c_double(0), np.array([passes], dtype=np.uint32)
        lib.qp_read_chunk(c.ctypes.data, 1, p.ctypes.data, 0, words.ctypes.data, C.byref(dead))
        return int(words[0]), int(words[1])
    return read


def test_leftovers_of_the_last_pass(case, read_chunk):
    """one workgroup, stacks of 16 slots: the last pass's stacks overflow into the queue of a generation no launch reads.  No ray is
    lost and none traced twice -- the run plus the model continued from the rays it left equals the full expectation -- the device
    flags stay 0, and the host's reader declares the chunk lost from the mark QC_GEN + passes"""
    out = case.run(passes=1, grid=1, stack_cap=16)
    rest = check(case, out, leftovers=True)
    assert out["gen"][1] >= len(out["rays"]) > 0 and rest.rays > 0
    assert out["flags"] == 0
    flags, verdict = read_chunk(out["counts"], 1)
    assert verdict == ACN_CHUNK_OVERFLOW and flags & 2
    # the same block read as a chunk of two launches has nothing left over
    assert read_chunk(out["counts"], 2)[1] == 0


def test_kernel_variants(case_v):
    """nodes in LDS or global memory, with or without prune programs: the four non-counting instantiations of k_walk on a handle that
    reports both, each against the same expectation"""
    assert case_v.info["prune"] and case_v.info["lds_nodes"]
    for prune in (True, False):
        for lds in (True, False):
            for kw in (dict(passes=1), dict(passes=3, private_limit=100, fetch=96)):
                out = case_v.run(prune=prune, lds=lds, **kw)
                check(case_v, out)
                assert out["counts"][QC["walk_rays"]] == case_v.model.rays


# ---------------------------------------------------------------------------------------------------------------------
# the camera form

def test_camera_form(case):
    """300 positions -- two tiles, the second one short -- at jittered positions and on the raster from a first pixel: each equals, to
    the bit in every queue and in accum, the run on Handle.camera_rays of the same positions with what k_walk gives a camera ray"""
    h, prm = case.h, case.prm
    rng = np.random.default_rng(5)
    n, first = 300, 37
    raster = A.main_pass_positions(prm.image_width, prm.image_height, first=first, count=n)
    jittered = raster + rng.uniform(-0.5, 0.5, raster.shape)
    room = 40 * n
    for pos, kw in ((jittered, dict(pos_xy=jittered)), (raster, dict(n=n, first_pixel=first))):
        rays = np.zeros(n, dtype=REC["ray"])
        cr = h.camera_rays(pos)
        rays["p"], rays["d"], rays["T"], rays["intensity"], rays["depth"], rays["pixel"] = cr[:, :3], cr[:, 3:], 1.0, 1.0, prm.trace_depth, np.arange(n)
        for arr in (dict(passes=1), dict(passes=4, private_limit=100)):
            want = h.run_stage_walk(rays, room_rays=room, stack_cap=STACK, **arr)
            got = h.run_stage_walk(room_rays=room, stack_cap=STACK, **kw, **arr)
            assert want["flags"] == got["flags"] == 0 and len(want["rays"]) == len(got["rays"]) == 0
            for q in ("hard_shadow",):
                same_records(got[q], list(want[q]), q)
            same_records(got["tasks"][np.concatenate(got["idx"])], list(want["tasks"][np.concatenate(want["idx"])]), "tasks")
            for k in range(4):
                same_records(got["tasks"][got["idx"][k]], list(want["tasks"][want["idx"][k]]), ("class", k))
            assert np.array_equal(got["accum"], want["accum"]) and want["accum"].any()
            cg, cw = got["counts"], want["counts"]
            for key in ("walk_rays", "s_probes"):
                assert cg[QC[key]] == cw[QC[key]] > 0, key
            # the launch covered the 512 slots of two tiles: the 212 past the last position are stepped over as dead input
            assert int(cg[QC["walk_steps"]]) * 64 >= int(cg[QC["walk_rays"]]) + 212
            assert cg[QC["cur_gen0"]] >= 512


# ---------------------------------------------------------------------------------------------------------------------
# refusals

def test_refusals_before_any_launch(case_a):
    h = case_a.h
    rays = case_a.rays[case_a.rays["pixel"] != INVALID][:8].copy()
    rays["pixel"] = np.arange(8)
    tmin = case_a.prm.trace_min_intensity
    ok = dict(room_rays=100, passes=1)

    def refused(r=rays, **kw):
        with pytest.raises(A.AcnError) as e:
            h.run_stage_walk(r, **{**ok, **kw})
        return e.value.status == A.abi.ACN_ERR_ARG

    for field, value in (("pixel", 8), ("depth", 0), ("depth", -1), ("depth", A.abi.ACN_STAGE_MAX_DEPTH + 1), ("intensity", np.nan), ("intensity", np.inf),
                         ("intensity", np.nextafter(tmin, 0.0)), ("intensity", 0.0), ("p", (np.nan, 0, 0)), ("d", (0, np.inf, 0)), ("d", (0, 0, 0)),
                         ("T", (1, np.nan, 1)), ("T", (np.inf, 1, 1))):
        bad = rays.copy()
        bad[field][7] = value
        assert refused(bad), (field, value)
    for kw in (dict(passes=0), dict(passes=A.abi.ACN_MAX_WALK_PASSES + 1), dict(stack_cap=0), dict(stack_cap=A.abi.ACN_STAGE_WALK_MAX_STACK + 1),
               dict(stack_cap=64, stack_use=65), dict(fetch=63), dict(fetch=(1 << 20) + 1), dict(grid=65), dict(room_rays=7), dict(room_rays=1 << 26),
               dict(flags=32), dict(flags=A.abi.ACN_STAGE_COUNT_WORK | A.abi.ACN_STAGE_NO_LEAF_LIGHTS), dict(flags=A.abi.ACN_STAGE_NO_LEAF_LIGHTS), dict(pos_xy=np.zeros((8, 2))), dict(n=8)):
        assert refused(**kw), kw
    # neither form, and the raw entry points with null arguments
    a, caps, o = A.abi.StageWalkArgs(), A.abi.StageCaps(), A.abi.StageOut()
    a.stage, a.n, a.passes, a.stack_cap, a.fetch, a.room_rays = A.abi.ACN_STAGE_WALK, 8, 1, 64, 64, 100
    from actinon_amd._lib import hip
    assert hip.acn_stage_walk_plan(h.h, C.byref(a), C.byref(caps)) == A.abi.ACN_ERR_ARG              # neither input form
    a.input = rays.ctypes.data
    assert hip.acn_stage_walk_plan(h.h, C.byref(a), C.byref(caps)) == A.abi.ACN_OK
    assert hip.acn_stage_walk_plan(None, C.byref(a), C.byref(caps)) == A.abi.ACN_ERR_ARG
    assert hip.acn_stage_walk_plan(h.h, None, C.byref(caps)) == A.abi.ACN_ERR_ARG
    assert hip.acn_stage_walk_plan(h.h, C.byref(a), None) == A.abi.ACN_ERR_ARG
    assert hip.acn_run_stage_walk(h.h, C.byref(a), None) == A.abi.ACN_ERR_ARG
    a.stage = A.abi.ACN_STAGE_SHADE_HITS
    assert hip.acn_run_stage_walk(h.h, C.byref(a), C.byref(o)) == A.abi.ACN_ERR_ARG
    # a dead slot is not read further, and an accepted call of eight rays runs
    rays["pixel"][3], rays["depth"][3], rays["intensity"][3] = INVALID, -5, np.nan
    out = h.run_stage_walk(rays, room_rays=8 * 100, passes=2, private_limit=0)
    assert out["flags"] == 0 and out["counts"][QC["walk_rays"]] >= 7 and out["gen"][0] == 8
