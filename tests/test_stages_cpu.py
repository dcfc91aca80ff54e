"""The CPU side of the stage tests (tests/test_gpu_stages.py): the argument checks of the stage runner in a sanitized program, the
oracle's tap against the oracle itself, the geometry of the test scene, and the contract of the closed-form Oren-Nayar weight."""
import os
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import ray_sets as R
import shade_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = A.Handle.STAGE_RECORDS
T = M.T


def test_stage_checks_in_a_sanitized_program(tmp_path):
    """acn_stage_host.h compiled with tests/csrc/stage_cpu.cpp into a program of its own with -fsanitize=address,undefined: every
    refusal of acn_run_stage and the capacities of an accepted call, records and index list in heap blocks of exactly their size;
    nothing sanitized is loaded here"""
    exe = tmp_path / "stage_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "stage_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_model_to_fixed_and_classes():
    x = np.array([0.0, 2.0 ** -41, 3 * 2.0 ** -41, -2.0 ** -41, 2.0 ** -41 + 2.0 ** -60, 1.0, 16384.0, 16385.0, -1e30, np.nan, np.inf])
    assert list(M.to_fixed(x)) == [0, 0, 2, 0, 1, 1 << 40, 16384 << 40, 16384 << 40, -(16384 << 40), 0, 16384 << 40]
    assert [M.size_class(n, 40) for n in (1, 2, 3, 8, 9, 40, 41, 200)] == [3, 3, 2, 2, 1, 1, 0, 0]
    for n in (1, 2, 3, 7, 200):
        parts = [M.shard_range(n, k, 3) for k in range(3)]
        assert parts[0][0] == 0 and parts[-1][1] == n and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))


# ---------------------------------------------------------------------------------------------------------------------
# the tap against the oracle: its rows, summed in scene_lum's own order, are the oracle's image

def _lum(oracle, flat, hit, bg):
    """scene_lum of the oracle from the tap's rows: the recursion and the sums are made here, in the order of scene_lum"""
    rows, _ = oracle.shade_point(flat, hit)
    lum = np.zeros(3)
    if len(rows) == 0:
        return lum
    if rows[0, 0] == T["emission"]:
        return rows[0, 1:4].copy()
    enter_color = M.rows_of(rows, "surface")[0, 4:7]
    depth = hit[12]
    k = 0
    while k < len(rows):
        r = rows[k]
        kind = int(r[0])
        if kind in (T["fresnel"], T["chromatic"], T["refraction"]):
            a, nor, ex, en = oracle.trans_hit(flat, r[1:4], r[4:7])
            if a < np.inf:
                l = _lum(oracle, flat, np.concatenate([r[1:4], r[4:7], [a], nor, [ex, en, r[8], r[7]]]), bg)
            else:
                l = bg * r[7]
            lum = lum + l * r[9:12]
        elif kind == T["diffuse"]:
            lum_l = np.zeros(3)
            k += 1
            while k < len(rows) and int(rows[k, 0]) in (T["light"], T["direct"], T["paths"], T["path"]):
                r = rows[k]
                kind = int(r[0])
                if kind == T["light"]:
                    color, norm, cl = r[3:6], 2.0 * r[2] / r[6], np.zeros(3)
                    k += 1
                    while k < len(rows) and int(rows[k, 0]) == T["direct"]:
                        d = rows[k]
                        if d[6] > 0 and d[7] < np.inf and d[9] == 0:
                            cl = cl + color * d[11]
                        k += 1
                    lum_l = lum_l + cl * norm
                elif kind == T["paths"]:
                    norm, cl = 2.0 / r[1], np.zeros(3)
                    k += 1
                    while k < len(rows) and int(rows[k, 0]) == T["path"]:
                        p = rows[k]
                        if p[5] > 0:
                            if p[14]:
                                pos = M.rows_of(rows, "surface")[0, 1:4]
                                cl = cl + _lum(oracle, flat, np.concatenate([pos, p[2:5], [p[7]], p[8:11], [p[11], p[12], depth - 10, p[13]]]), bg)
                            else:
                                cl = cl + bg * p[13]
                        k += 1
                    lum_l = lum_l + cl * norm
                else:
                    raise AssertionError("a sample row outside its loop")
            lum = lum + lum_l * enter_color
            continue
        elif kind == T["absorb"]:
            lum = lum * r[1:4]
        k += 1
    return lum


def test_tap_rows_reproduce_the_oracle_image(oracle):
    """Scene A cut to trace_depth 11 (one level of path samples), black background: the tap's rows, added up in scene_lum's own
    order with the recursion made here, are acn_oracle_render_positions on the same rays bit for bit.  The camera looks along +y,
    so its rotation is the identity and the ray of a position is stated here exactly."""
    for bgc in ((0.0, 0.0, 0.0), (0.3, 0.35, 0.4)):
        sc, node = R.shade_stage_scene(direct_samples=6, path_samples=5, trace_depth=11, image_width=24, image_height=24, background_color=bgc,
                                       camera_position=(0.5, -7.0, 2.5), camera_view_direction=(0, 1, 0), camera_top_direction=(0, 0, 1),
                                       camera_focal_length=1.2, trace_min_intensity=0.03)
        flat = sc.flatten()
        prm = flat.params
        pos = np.array([[x + 0.5, y + 0.5] for y in range(0, 24, 2) for x in range(0, 24, 2)])
        want = oracle.render_positions(flat, pos, linear=True)
        bg = np.array(bgc)
        unit_f = 1.0 / (prm.image_height >> 1)
        hits = 0
        for p, w in zip(pos, want):
            d = np.array([unit_f * (p[0] - (prm.image_width >> 1)), prm.camera_focal_length, unit_f * ((prm.image_height >> 1) - p[1])])
            r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            assert abs(r2 - 1.0) >= 1e-8
            d = d * (1.0 / np.sqrt(r2))
            o = np.array(list(prm.camera_position))
            a, nor, ex, en = oracle.trans_hit(flat, o, d)
            got = bg
            if a < np.inf:
                hits += 1
                got = _lum(oracle, flat, np.concatenate([o, d, [a], nor, [ex, en, prm.trace_depth, 1.0]]), bg)
            assert np.array_equal(got.view(np.uint64), w.view(np.uint64)), (p, got, w)
        assert hits > 100


# ---------------------------------------------------------------------------------------------------------------------
# the geometry of the sample test, from the oracle alone

def _sample_rows(oracle, flat, node):
    hits, labels, expect = R.stage_sample_hits(flat, node, REC["hit"], oracle=oracle)
    return hits, labels, [oracle.shade_point(flat, M.tap_input(r))[0] for r in hits], expect


def test_sample_tasks_shadow_rays_enter_the_envelope(oracle):
    """A shadow ray that enters the torus' envelope cannot be decided by k_shade in line: the sample leaves it as a HardShadow record.
    For EVERY task of the sample test, from the oracle's rows alone: the unoccluded direct samples whose ray misses the envelope -- what
    only accum shows -- are at most a tenth of the task's direct samples, unless accum holds that one term alone.  The tasks cover
    every sample count, tasks with and without the Oren-Nayar term, and the sums stay below the fixed point's clamp."""
    sc, node = R.shade_stage_scene()
    flat = sc.flatten()
    hits, labels, rows, expect = _sample_rows(oracle, flat, node)
    c, rad = np.array(R.STAGE_ENVELOPE[0]), R.STAGE_ENVELOPE[1]

    def misses(pos, dirs):
        """the rays pos + t * dir, t > 0, that do not meet the envelope's ball (the device's test has no limit either)"""
        tca = ((c - pos) * dirs).sum(axis=1)
        off2 = ((c - pos) ** 2).sum() - tca * tca
        return ~((off2 < rad * rad) & ((tca > 0) | (((c - pos) ** 2).sum() < rad * rad)))

    seen = {n: 0 for n in R.STAGE_N}
    in_line = 0
    for r, l, rw in zip(hits, labels, rows):
        d, p = M.rows_of(rw, "direct"), M.rows_of(rw, "path")
        nd, npth = M.sample_counts(rw)
        seen[nd] = seen.get(nd, 0) + 1
        pos = M.rows_of(rw, "surface")[0, 1:4]
        open_ = d[(d[:, 6] > 0) & (d[:, 7] < np.inf) & (d[:, 9] == 0)]
        hidden = int(misses(pos, open_[:, 3:6]).sum())
        back = p[(p[:, 5] > 0) & ~(p[:, 7] < flat.params.max_path_length)]
        terms = int(misses(pos, back[:, 2:5]).sum())
        in_line += hidden
        if hidden + terms > 1:
            assert hidden <= 0.1 * len(d), (l, hidden, terms, len(d))
    assert in_line >= 8                                    # ("outside_one": a single term each, which accum shows exactly)
    assert all(v > 0 for v in seen.values()), seen
    on_b = np.array([M.rows_of(rw, "surface")[0, 9] for rw in rows])
    assert (on_b == 0).sum() >= 40 and (on_b > 0).sum() >= 200 and 250 <= len(hits) <= 350
    lum = np.array([np.abs(oracle.shade_point(flat, M.tap_input(r))[1]).max() for r in hits])
    # (a task of one sample at intensity 1.5 / 200 sums to ~1e-3, where 2^-40 is 1e-9 relative: the absolute term of the GPU test's bound)
    assert lum.max() < 8000 and np.median(lum[labels == "inside"]) > 0.1


def test_sample_tasks_sit_on_the_named_edges(oracle):
    """the edges the sample test names are there to the bit, by the oracle's own numbers"""
    sc, node = R.shade_stage_scene()
    flat = sc.flatten()
    hits, labels, rows, expect = _sample_rows(oracle, flat, node)
    # on the light's sphere: diff_sqr == radius_sqr, the double below and the double above (sphere_fov: diff_sqr > radius_sqr)
    lp, lr = np.array(list(flat.node(node["sphere_light"]).pos)), flat.node(node["sphere_light"]).prm[0]
    want = {"on_light": lr * lr, "in_light": np.nextafter(lr * lr, 0.0), "off_light": np.nextafter(lr * lr, 1.0)}
    for label, v in want.items():
        sel = np.nonzero(labels == label)[0]
        assert len(sel) == 4
        for i in sel:
            df = lp - M.rows_of(rows[i], "surface")[0, 1:4]
            assert (df[0] * df[0] + df[1] * df[1]) + df[2] * df[2] == v, label
            li = M.rows_of(rows[i], "light")
            li = li[li[:, 1] == node["sphere_light"]][0]
            assert (li[2] == 2.0) == (label != "off_light")          # cos_rs = -1 (the whole sphere of directions) unless outside
    # path hits at max_path_length, its predecessor and its successor: one bright and one dark sample each
    lim = flat.params.max_path_length
    got = set()
    for (i, j), case in expect.items():
        p = M.rows_of(rows[i], "path")
        r = p[p[:, 1] == j][0]
        assert r[7] == case["target"] and r[5] > 0 and r[12] >= node["limit0"], (case["group"], r)
        dark = r[13] < flat.params.trace_min_intensity
        assert dark == (case["group"] == "probe") and bool(r[14]) == (r[7] < lim)
        got.add((case["group"], float(r[7] - lim) > 0, float(r[7] - lim) < 0))
    assert len(expect) == 6 and len(got) == 6


# ---------------------------------------------------------------------------------------------------------------------
# the closed form's contract: oren_nayar_weight_direct (the model's, which the GPU test pins to the device bit for bit) against the
# oracle's exact form

# |closed - exact| <= K * 2^-53 * on_b / min( sr, cos_i, 1 ), sr = |out_d - nor * w|, per region.  The form is what the conditioning
# predicts: acos( w ) near w = 1 loses the digits of sr ( theta_r ~ sr, rounded against pi / 2 - scale constants ), and cos( acos x )
# near x = 0 those of cos_i.  K is 4 x the largest quotient measured on the sample test's tasks and 10^5 random ones (the factor covers
# draws this set did not make); DESIGN.md section 5 lists the measured values
# measured maxima of the quotient: general 8.615, sr < 1e-3 3.500, cos_i < 1e-3 0.190.  Where w < 1e-4 the form does not describe the
# difference: there the two differ by up to 4.4e-9 relative, the EXACT form's deviation (v_of_length hands it an unscaled vector), and
# the test takes 5.0000001e-9 * addend out before it applies the form.  Nothing measurable is left after that (quotient 0), so in that
# region the assertion is in effect "within 5e-9 of the Oren-Nayar addend" -- the bound the kernel's comment has always stated, not one
# of the form above; the K it keeps is the general one and binds nothing there
CLOSED_FORM_K = {"general": 34.5, "w<1e-4": 34.5, "sr<1e-3": 14.0, "cos_i<1e-3": 0.76}


def _closed_form_errors(oracle, detmath, flat, hits):
    out = []
    for r in hits:
        rows = oracle.shade_point(flat, M.tap_input(r))[0]
        if not len(M.rows_of(rows, "diffuse")):
            continue
        t = M.task_of(rows, r, REC)
        d = M.rows_of(rows, "direct")
        live = d[(d[:, 6] > 0) & (d[:, 7] < np.inf)]
        if not len(live) or not t["on_b"] > 0 or not np.isfinite(t["theta_i"]):
            continue
        w = live[:, 6]
        closed = M.closed_weight(detmath, w, t["theta_i"], t["on_a"], t["on_b"], live[:, 3:6], t["surface_d"], t["ray_projection"])
        prj = live[:, 3:6] - t["surface_d"][None, :] * w[:, None]
        sr = np.sqrt((prj * prj).sum(axis=1))
        cos_i = abs(np.cos(t["theta_i"]))
        out.append(np.stack([np.abs(closed - live[:, 8]), w, sr, np.full(len(w), cos_i), np.full(len(w), t["on_b"]), live[:, 8],
                             np.abs(live[:, 8] - w * t["on_a"])], axis=1))
    return np.concatenate(out)


def test_closed_form_weight_contract(oracle, detmath_cpu):
    sc, node = R.shade_stage_scene()
    flat = sc.flatten()
    hits, labels, _ = R.stage_sample_hits(flat, node, REC["hit"])
    rng = np.random.default_rng(31)
    lp = np.array(list(flat.node(node["sphere_light"]).pos))
    rnd = []
    for k in range(520):                                                           # x 200 samples: 10^5 samples that reach the light
        pos = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0, 3)])
        if k % 4 in (1, 2):
            pos = lp + R.unit(pos - lp) * 10.0 ** rng.uniform(2, 6)                # a narrow cone: its samples graze the surface / lie at the normal together
        ax = R.unit(lp - pos)
        side = R.unit(np.cross(ax, rng.normal(size=3)))
        mode = k % 4
        if mode == 0:
            nor = R.unit(ax + rng.normal(size=3) * 0.8)                            # general
        elif mode == 1:
            nor = R.unit(side + ax * 10.0 ** rng.uniform(-6, -4))                  # the light at the horizon: w down to 1e-6 and below
        elif mode == 2:
            nor = R.unit(ax + side * 10.0 ** rng.uniform(-9, -2))                  # out_d at the normal
        else:
            nor = R.unit(ax + rng.normal(size=3) * 0.5)
        view = R.unit(rng.normal(size=3))
        view = view - nor * min(view @ nor, 0.0) * 2 if view @ nor > 0 else view   # arrives from the side the normal faces
        if mode == 3:
            tang = R.unit(np.cross(nor, rng.normal(size=3)))
            view = R.unit(tang - nor * 10.0 ** rng.uniform(-8, -1))               # theta_i at pi / 2
        if view @ nor > 0:
            view = view - 2 * nor * (view @ nor)
        rnd.append(R._hit(REC["hit"], pos - view, view, 1.0, -nor, -1, node["floor"], 12, 1.0, (1, 1, 1)))
    e = _closed_form_errors(oracle, detmath_cpu, flat, list(hits) + rnd)
    assert len(e) >= 100000, len(e)
    err, w, sr, cos_i, on_b, exact, addend = e.T
    # w < 1e-4 is where 1 - sr^2 = w^2 < 1e-8: there v_of_length (vectors.h:151) hands the EXACT form its argument back unscaled, a
    # vector of length sr, not 1, so the exact form's addend on_b * cos_phi * sin * tan is short by the factor sr >= 1 - 5.0000001e-9.
    # That share is the reference's, not the closed form's; what is left is held to the same form as elsewhere
    raw = err
    err = np.where(w < 1e-4, np.maximum(err - 5.0000001e-9 * addend, 0.0), err)
    quot = err / (2.0 ** -53 * on_b / np.minimum(np.minimum(sr, cos_i), 1.0))
    regions = {"w<1e-4": w < 1e-4, "sr<1e-3": (sr < 1e-3) & (w >= 1e-4), "cos_i<1e-3": (cos_i < 1e-3) & (w >= 1e-4) & (sr >= 1e-3)}
    regions["general"] = ~(regions["w<1e-4"] | regions["sr<1e-3"] | regions["cos_i<1e-3"])
    for name, sel in regions.items():
        rel = (raw[sel] / np.maximum(np.abs(exact[sel]), 1e-300)).max()
        print(f"closed form, {name}: {int(sel.sum())} samples, max |closed - exact| {raw[sel].max():.3e} (relative {rel:.3e}), "
              f"max quotient {quot[sel].max():.3f}")
    for name, sel in regions.items():
        assert sel.sum() > 500, (name, sel.sum())
        assert quot[sel].max() <= CLOSED_FORM_K[name], (name, quot[sel].max())


# ---------------------------------------------------------------------------------------------------------------------
# the work ledger (shade_model.ledger, ledger_hit): the model of what a scene_s_lum call books, against the oracle's own books

@pytest.mark.parametrize("name", ["primitives_path", "wine_glass_c2"])
def test_ledger_sums_to_the_oracles_counters(oracle, name):
    """The ledgers of every tap of a small frame, with scene_lum's recursion made from the rows (shade_model.frame_ledger), add up to
    the counters Oracle.render_positions returns for the same positions.  Before the device's differences are applied the model is
    the oracle's own bookkeeping read off its rows, so this is an identity: no tolerance.  The costs come from acn_costs.h."""
    import scenes_util as S
    sc, flat = S.build(name)
    pos = S.positions(flat)
    pos = pos[::-(-len(pos) // 200)]
    assert 150 <= len(pos) <= 200
    _, c = oracle.render_positions(flat, pos, counters=True)
    m = M.frame_ledger(oracle, flat, pos)
    assert c["flop_shade"] > 100000 and c["transc_shade"] > 10000 and c["oren_nayar_direct"] > 0 and c["oren_nayar_path"] > 0
    for ours, theirs in (("flop_shade", "flop_shade"), ("transc_shade", "transc_shade"), ("cap_sample", "cap_sample"), ("shadow_ray", "shadow_ray"),
                         ("lum", "lum"), ("trans_ray", "trans_ray"), ("oren_nayar_direct", "oren_nayar_direct"), ("oren_nayar_path", "oren_nayar_path")):
        assert m[ours] == c[theirs], (ours, m[ours], c[theirs])
    # the split itself: the two loops add up, and the shading part is a part
    assert c["oren_nayar_direct"] + c["oren_nayar_path"] == c["oren_nayar"]
    assert c["flop_shade"] < c["flop"] and c["transc_shade"] <= c["transc"]


def test_ledger_reads_the_cost_table():
    """the numbers are the header's: every event the ledger prices is a line of acn_costs.h"""
    C = M.costs()
    for k in ("F_LUM_FIXED", "F_EMISSION", "F_ABSORB", "T_ABSORB", "F_FRESNEL_REFL", "F_FRESNEL_REFR", "F_REFLECTION", "F_SHADE_DIFFUSE", "T_SHADE_DIFFUSE",
              "F_SEED", "T_SEED", "F_FOV", "F_FRAME", "F_CAP_SAMPLE", "T_CAP_SAMPLE", "F_OREN_NAYAR", "T_OREN_NAYAR", "F_OREN_NAYAR_DIRECT", "F_DIRECT_TAIL",
              "F_PATH_TAIL", "F_CAMERA_RAY"):
        assert C[k] > 0, k
    assert "T_OREN_NAYAR_DIRECT" not in C           # the closed form has no transcendental: DEVICE_DIRECT_WEIGHT
