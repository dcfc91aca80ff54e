"""The CPU side of the walk stage test (tests/test_gpu_stage_walk.py): the argument checks and the plan of acn_run_stage_walk in a
sanitized program, the model of the walk (tests/walk_model.py) against the oracle's own recursion, what the inputs of the GPU test
contain by the oracle alone, and the binding's names."""
import os
import re
import subprocess

import numpy as np

import actinon_amd as A
import ray_sets as R
import shade_model as M
import walk_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = A.Handle.STAGE_RECORDS
QC = {**A.Handle.QC, **A.Handle.QC_WALK}


def test_walk_stage_checks_in_a_sanitized_program(tmp_path):
    """acn_stage_host.h compiled with tests/csrc/stage_walk_cpu.cpp into a program of its own with -fsanitize=address,undefined: every
    refusal of the walk stage and the plan of an accepted call, rays in heap blocks of exactly their size; nothing sanitized is
    loaded here"""
    exe = tmp_path / "stage_walk_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "stage_walk_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_binding_names_the_walk_stage_as_the_header_does():
    with open(os.path.join(ROOT, "include", "actinon_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "actinon_amd", "csrc", "acn_counts.h")) as f:
        counts = f.read()
    for name in ("ACN_STAGE_WALK", "ACN_STAGE_GLOBAL_NODES", "ACN_STAGE_WALK_MAX_STACK"):
        m = re.search(r"#define %s\s+(\d+)u" % name, header)
        assert m and int(m.group(1)) == getattr(A.abi, name), name
    assert re.search(r"#define ACN_MAX_WALK_PASSES (\d+)", counts).group(1) == str(A.abi.ACN_MAX_WALK_PASSES)
    # the flags of the walk are distinct bits beside the stage runner's
    bits = (A.abi.ACN_STAGE_NO_PRUNE, A.abi.ACN_STAGE_NO_LEAF_LIGHTS, A.abi.ACN_STAGE_NO_EMIT_TERMS, A.abi.ACN_STAGE_GLOBAL_NODES,
            A.abi.ACN_STAGE_COUNT_WORK)
    assert sorted(bits) == [1, 2, 4, 8, 16]
    m = re.search(r"#define ACN_STAGE_COUNT_WORK\s+(\d+)u", header)
    assert m and int(m.group(1)) == A.abi.ACN_STAGE_COUNT_WORK
    assert "int acn_stage_last_counters( acn_scene_handle* h, uint64_t* out, int n );" in header
    # the struct, field for field in the header's order
    body = re.search(r"typedef struct acn_stage_walk_args\s*\{(.*?)\}\s*acn_stage_walk_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip().lstrip("*") for n in decl.split(" ", 2 if decl.startswith("const") else 1)[-1].split(",")]
    ours = [n for n, _ in A.abi.StageWalkArgs._fields_]
    assert [{"in": "input"}.get(n, n) for n in fields] == ours, (fields, ours)
    # the words of the counter block the walk test reads
    for key, word in (("walk_rays", "QS_WALK_RAYS"), ("walk_steps", "QS_WALK_STEPS"), ("private_rays", "QS_PRIVATE_RAYS"), ("s_probes", "QS_PROBES"),
                      ("dead_r", "QS_DEAD_R"), ("dead_t", "QS_DEAD_T"), ("gen0", "QC_GEN")):
        assert re.search(r"\b%s = %d\b" % (word, QC[key]), counts), word
    assert QC["cur_gen0"] == QC["gen0"] + A.abi.ACN_MAX_WALK_PASSES + 1 and "QC_CUR_GEN = QC_GEN + ACN_MAX_WALK_PASSES + 1" in counts


# ---------------------------------------------------------------------------------------------------------------------
# the model against the oracle's own recursion

def _axis_camera_rays(prm, pos):
    """camera_ray for a camera that looks along +y with +z up: the rotation is the identity, so the ray is stated here exactly"""
    unit_f = 1.0 / (prm.image_height >> 1)
    out = np.zeros((len(pos), 6))
    for k, p in enumerate(pos):
        d = np.array([unit_f * (p[0] - (prm.image_width >> 1)), prm.camera_focal_length, unit_f * ((prm.image_height >> 1) - p[1])])
        r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        assert abs(r2 - 1.0) >= 1e-8
        out[k, :3], out[k, 3:] = list(prm.camera_position), d * (1.0 / np.sqrt(r2))
    return out


def test_model_sums_to_the_oracles_picture(oracle):
    """A scene without a diffuse surface -- a glass lens, mirrors, water, a light, the sky: scene_lum's picture is then the sum of the
    walk's own terms (emission, the background of a miss) and of the probes' (the background where a dead child hits nothing).  The
    model's accum * 2^-40 per pixel against Oracle.render_positions( linear ), within terms * 2^-41 (one rounding to the 2^-40 grid
    per term) + 64 * eps * |lum| (the oracle multiplies the colours onto what the recursion returns, the walk carries them down:
    the reassociation of the sum)."""
    sc, flat = R.walk_small_scene(diffuse_floor=False, camera_position=(-0.3, -7.0, 2.0), camera_view_direction=(0, 1, 0), camera_top_direction=(0, 0, 1),
                                   image_width=36, image_height=24, trace_min_intensity=0.04, camera_focal_length=3.0)
    prm = flat.params
    pos = A.main_pass_positions(prm.image_width, prm.image_height)
    want = oracle.render_positions(flat, pos, linear=True)
    rays = R._walk_records(REC["ray"], _axis_camera_rays(prm, pos), 1.0, 1.0, int(prm.trace_depth))
    rays["pixel"] = np.arange(len(rays))
    w = W.walk(oracle, flat, rays, REC)
    acc, terms = w.accum.copy(), w.terms.copy()
    for p in w.probes:                                        # k_hard_shadow: the probe's term where nothing is hit
        assert p["pad"] == 1 and p["limit"] == M.F3_BIG
        if not oracle.trans_hit(flat, p["pos"], p["d"])[0] < np.inf:
            acc[p["pixel"]] += M.to_fixed(p["contrib"])
            terms[p["pixel"]] += 1
    assert len(w.tasks) == 0 and w.misses > 100 and w.emissions >= 10 and len(w.probes) > 50 and w.generations == prm.trace_depth, w.totals()
    got = acc * 2.0 ** -40
    bound = terms[:, None] * 2.0 ** -41 + 64 * np.finfo(np.float64).eps * np.abs(want)
    err = np.abs(got - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"walk model against the oracle: {len(pos)} pixels, {w.totals()}, {int(terms.sum())} terms (at most {int(terms.max())} per pixel), "
          f"worst error / bound {ratio.max():.3f}")
    assert (err <= bound).all(), (ratio.max(), np.argmax(ratio))
    assert (terms > 1).sum() >= 40 and (np.abs(want).max(axis=1) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU test, by the oracle alone

def _check_input(rays):
    n = len(rays)
    dead = rays["pixel"] == M.INVALID
    assert n % 64 != 0 and n % 256 != 0
    assert abs(int(dead.sum()) - n // 20) <= n // 200 + 2 and (rays["pixel"][~dead] == np.nonzero(~dead)[0]).all()
    return int(dead.sum())


def test_walk_inputs_contain_what_the_gpu_test_relies_on(oracle):
    sc, node = R.shade_stage_scene()
    flat = sc.flatten()
    prm = flat.params
    rays = R.walk_rays_stage_scene(flat, node, REC["ray"])
    dead = _check_input(rays)
    live = rays[rays["pixel"] != M.INVALID]
    tmin = prm.trace_min_intensity
    for d in R.WALK_DEPTHS:
        assert (live["depth"] == d).sum() >= 150, d
    for i in (tmin, np.nextafter(tmin, 1.0), 0.5):
        assert (live["intensity"] == i).sum() >= 150, i
    assert (live["T"] >= 0.2).all() and (live["T"] <= 1.0).all() and (live["intensity"] >= tmin).all()
    a = W.walk(oracle, flat, rays, REC)
    print(f"scene A: {len(rays)} records ({dead} dead) -> {a.totals()}, rays at the added depths {[a.rays_at_depth(d) for d in R.WALK_DEPTHS]}")
    assert a.generations >= 20 and len(a.tasks) >= 1500 and len(a.probes) >= 1500 and a.emissions >= 300
    for d in R.WALK_DEPTHS:
        assert a.rays_at_depth(d) >= 200, d
    assert a.generations + 1 <= A.abi.ACN_MAX_WALK_PASSES and a.clamped == 0
    # classes: the tasks of the walk reach every index list but need not fill each
    sw, fw = R.walk_scene_wine_glass()
    rw = R.walk_rays_wine_glass(fw, REC["ray"])
    dead = _check_input(rw)
    memo = {}
    g = W.walk(oracle, fw, rw, REC, memo=memo)
    # continued from a generation the model is the rest of itself; without emit_terms it keeps the rays and the tasks and drops the rest
    rest = W.walk(oracle, fw, g.gens[3], REC, n=len(rw), memo=memo)
    assert rest.generations == g.generations - 3 and rest.rays == sum(len(x) for x in g.gens[3:]) and len(memo) == g.rays
    head = W.walk(oracle, fw, rw, REC)
    assert np.array_equal(head.accum, g.accum) and len(head.probes) == len(g.probes)
    quiet = W.walk(oracle, fw, rw, REC, emit_terms=False)
    assert quiet.rays == g.rays and len(quiet.tasks) == len(g.tasks) and not quiet.probes and not quiet.accum.any() and g.accum.any()
    print(f"wine glass: {len(rw)} records ({dead} dead) -> {g.totals()}")
    assert g.misses >= 100 and g.generations + 1 <= A.abi.ACN_MAX_WALK_PASSES and len(g.tasks) > 500
    assert a.rays + g.rays <= 20000
    # every queued ray of the model is one the seam accepts: depth >= 1, intensity >= trace_min_intensity
    for w, f in ((a, flat), (g, fw)):
        for gen in w.gens:
            assert (gen["depth"] >= 1).all() and (gen["intensity"] >= f.params.trace_min_intensity).all()
    # the small scene of the kernel variants
    sv, fv = R.walk_small_scene()
    rv = R.walk_rays_small_scene(fv, REC["ray"])
    _check_input(rv)
    v = W.walk(oracle, fv, rv, REC)
    print(f"small scene: {len(rv)} records -> {v.totals()}")
    assert v.rays >= 1500 and len(v.tasks) >= 300 and len(v.probes) >= 100 and v.misses >= 100 and v.generations >= 10
