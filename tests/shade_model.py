"""What the shading kernels (acn_queues.h: shade_hit; acn_k_shade.h: k_shade) do differently from the oracle, restated in numpy one IEEE operation
at a time, so that every intermediate is rounded as on the device.  The oracle's own arithmetic is NOT restated: it comes from the rows
of acn_oracle_shade_point (oracle_binding.Oracle.shade_point), which scene_lum writes while it runs.

  colours     the oracle multiplies colours onto what the recursion returns; the device carries them down: T after absorption for the
              Fresnel and the refracted child, T * enter_color for the chromatic child and for the task (Tc)
  probes      a child scene_s_lum would return zero for (depth 0 or intensity below trace_min_intensity) is an any-hit probe whose
              contrib is T * ( background * intensity )
  closed form oren_nayar_weight_direct from sin_i, cos_i, tan_i (detmath through the detmath_cpu fixture)
  HardShadow  c = local_intensity * weight * diffuse_intensity, scale = Tc * ( light_color * norm ), contrib = scale * c
  to_fixed    clamp to +-16384, round to nearest even at 2^-40
  classes     size_class and the shard ranges j_lo / j_hi"""
import numpy as np

from oracle_binding import Oracle
from test_detmath import cpu_eval

T = Oracle.TAP
INVALID = 0xFFFFFFFF
F3_BIG = 1.7976931348623157e308
FIX_SCALE, FIX_CLAMP = 2.0 ** 40, 16384.0
CLASS1_MIN = 8


def to_fixed(x):
    """acn_records.h to_fixed: int64 per component"""
    x = np.asarray(x, dtype=np.float64)
    c = np.where(x < FIX_CLAMP, x, FIX_CLAMP)
    c = np.where(c > -FIX_CLAMP, c, -FIX_CLAMP)
    return np.where(np.isnan(x), 0, np.rint(np.nan_to_num(c) * FIX_SCALE)).astype(np.int64)


def size_class(n, class0_min):
    return 0 if n > class0_min else 1 if n > CLASS1_MIN else 2 if n > 2 else 3


def shard_range(n, rank, world):
    return (0, n) if world <= 1 else (n * rank // world, n * (rank + 1) // world)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def rows_of(rows, kind):
    return rows[rows[:, 0] == T[kind]]


def tap_input(r):
    """the [14] argument of Oracle.shade_point for a hit record"""
    return np.concatenate([r["p"], r["d"], [r["offs"]], r["exit_nor"], [r["exit_obj"], r["enter_obj"], r["depth"], r["intensity"]]])


def carried(rows, Tin):
    """T as shade_hit carries it past the absorption of the exit object (T *= pow( transparency, offs ) where offs > 0)"""
    ab = rows_of(rows, "absorb")
    Tin = np.asarray(Tin, dtype=np.float64)
    return Tin * ab[0, 1:4] if len(ab) else Tin


def split_expected(rows, rec, prm, records, emit_terms=True):
    """What k_shade_hits writes for hit record `rec` whose tap rows are `rows`: (rays, probes, task or None, accum int64 [3])"""
    tmin, bg = prm.trace_min_intensity, np.array(list(prm.background_color))
    rays, probes, task, acc = [], [], None, np.zeros(3, dtype=np.int64)
    if rec["pixel"] == INVALID or rec["depth"] == 0 or rec["intensity"] < tmin:
        assert len(rows) == 0
        return rays, probes, task, acc
    em = rows_of(rows, "emission")
    if len(em):
        return rays, probes, task, to_fixed(rec["T"] * em[0, 1:4])
    Ta = carried(rows, rec["T"])
    for r in rows:
        kind = int(r[0])
        if kind not in (T["fresnel"], T["chromatic"], T["refraction"]):
            continue
        Tc = Ta * r[9:12] if kind == T["chromatic"] else Ta
        depth, inten = int(r[8]), r[7]
        if depth == 0 or inten < tmin:
            if emit_terms:
                h = np.zeros((), dtype=records["hard_shadow"])
                h["pos"], h["d"], h["limit"], h["contrib"], h["pixel"], h["pad"] = r[1:4], r[4:7], F3_BIG, Tc * (bg * inten), rec["pixel"], 1
                probes.append(h)
        else:
            q = np.zeros((), dtype=records["ray"])
            q["p"], q["d"], q["T"], q["intensity"], q["depth"], q["pixel"] = r[1:4], r[4:7], Tc, inten, depth, rec["pixel"]
            rays.append(q)
    df = rows_of(rows, "diffuse")
    if len(df):
        task = task_of(rows, rec, records)
    return rays, probes, task, acc


def task_of(rows, rec, records):
    """the DTask of a hit with a diffuse block"""
    df, sf = rows_of(rows, "diffuse")[0], rows_of(rows, "surface")[0]
    t = np.zeros((), dtype=records["task"])
    t["pos"], t["surface_d"], t["theta_i"], t["ray_projection"], t["diffuse_intensity"] = sf[1:4], df[1:4], df[4], df[5:8], df[8]
    t["on_a"], t["on_b"], t["Tc"] = sf[8], sf[9], carried(rows, rec["T"]) * sf[4:7]
    t["rv"] = df[9:10].view(np.uint64)[0]
    t["depth"], t["pixel"] = rec["depth"], rec["pixel"]
    return t


def sample_counts(rows):
    li, pa = rows_of(rows, "light"), rows_of(rows, "paths")
    return (int(li[0, 6]) if len(li) else 0), (int(pa[0, 1]) if len(pa) else 0)


def closed_weight(detmath, w, theta_i, on_a, on_b, out_d, nor, ray_prj):
    """oren_nayar_weight_direct with k_shade's sin_i, cos_i, tan_i (TF_TAN_I = cos_i > 0 ? sin_i / cos_i : 0); arrays of samples"""
    w = np.asarray(w, dtype=np.float64)
    if not on_b > 0:
        return w
    th = np.array([theta_i])
    sin_i, cos_i = cpu_eval(detmath, "sin", th)[0], cpu_eval(detmath, "cos", th)[0]
    tan_i = sin_i / cos_i if cos_i > 0 else 0.0
    o = np.asarray(out_d, dtype=np.float64).T
    f = dot(o, nor)
    prj = [o[0] - nor[0] * f, o[1] - nor[1] * f, o[2] - nor[2] * f]
    m = -dot(prj, ray_prj)
    m = np.where(m > 0, m, 0.0)
    return w * on_a + on_b * m * np.where(cos_i <= w, sin_i, w * tan_i)


# ---------------------------------------------------------------------------------------------------------------------
# The work ledger: what the oracle, and what the counting kernels, book per event (acn_costs.h) for ONE scene_s_lum call, from the
# rows of its tap.  Two halves, as the device splits the call: ledger_hit is everything outside the two sample loops (shade_hit of
# acn_queues.h, run by k_shade_hits and k_walk), ledger the loops themselves (k_shade).  With device=False the two add up to what
# scene_lum of the oracle books for the call -- an identity, tests/test_stages_cpu.py sums it over a frame.  device=True applies the
# differences the kernels make on purpose, each by name:
DEVICE_DIRECT_WEIGHT = "ACN_F_OREN_NAYAR_DIRECT"   # the direct loop's weight in closed form: 17 flop and NO transcendental, and only
#                                                    for a sample no in-line element occluded (acn_k_shade_direct_loop.h)
DEVICE_DEFERRED_TAIL = "ACN_F_DIRECT_TAIL"         # a sample left to k_hard_shadow books its tail there, not in k_shade
DEVICE_HARD_PATH_TRANS = "trans_ray"               # a path ray left to k_hard_path books its compound_s_ray_trans_hit there
DEVICE_SHARD_SHARE = "cap_sample"                  # a shard rank draws its share of a loop alone (the oracle draws all, to stay in step)
DEVICE_DEAD_CHILD = "trans_ray"                    # a specular child scene_s_lum returns zero for is never traced: the probe, or the
#                                                    dropped ray, stands for the two compound_s_ray_trans_hit calls of scene_s_trans_hit

_COSTS = None


def costs():
    """{ "F_NAME": flop, "T_NAME": transcendentals } parsed from actinon_amd/csrc/acn_costs.h: the numbers are not restated here"""
    global _COSTS
    if _COSTS is None:
        import os
        import re
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "actinon_amd", "csrc", "acn_costs.h")
        with open(path) as f:
            _COSTS = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define ACN_([FT]_[A-Z_]+)\s+(\d+)", f.read(), re.M)}
        assert len(_COSTS) > 40 and _COSTS["F_FOV"] == 20 and _COSTS["T_CAP_SAMPLE"] == 2, _COSTS
    return _COSTS


LEDGER_KEYS = ("lum", "trans_ray", "shadow_ray", "cap_sample", "oren_nayar_direct", "oren_nayar_path", "direct_tail", "path_tail",
               "light_setups", "path_setups", "flop_shade", "transc_shade")


def _priced(ev, flop, transc):
    out = {k: int(ev.get(k, 0)) for k in LEDGER_KEYS}
    out["flop_shade"], out["transc_shade"] = int(flop), int(transc)
    return out


def add_ledgers(ledgers):
    out = {k: 0 for k in LEDGER_KEYS}
    for l in ledgers:
        for k in LEDGER_KEYS:
            out[k] += l[k]
    return out


def ledger(rows, lights_culled=0, device=False, shard=(0, 1), deferred=(), hard_path=()):
    """The sample loops of one task (rows: its tap) as event counts and flop_shade / transc_shade.
    device=False: what scene_lum books for the loops.  device=True: what k_shade books for the task, given
      lights_culled  lights whose set-up the kernel leaves out (it leaves out none today: the cone cull drops root elements, never a light)
      shard          (rank, world): the rank's share of each loop
      deferred       bits of out_d (bytes) of the direct samples the launch left to k_hard_shadow (its HardShadow records)
      hard_path      the same for the path rays it left to k_hard_path"""
    C = costs()
    sf, li, di, pa, ps = rows_of(rows, "surface"), rows_of(rows, "light"), rows_of(rows, "direct"), rows_of(rows, "paths"), rows_of(rows, "path")
    if not len(rows_of(rows, "diffuse")):
        return _priced({}, 0, 0)
    rough = sf[0, 9] > 0
    deferred, hard_path = set(deferred), set(hard_path)
    key = lambda d: np.ascontiguousarray(d, dtype=np.float64).tobytes()           # noqa: E731
    ev = {k: 0 for k in LEDGER_KEYS}
    flop = transc = 0
    ev["light_setups"] = len(li) - (lights_culled if device else 0)
    flop += ev["light_setups"] * (C["F_FOV"] + C["F_FRAME"])
    for l in li:
        n = int(l[6])
        lo, hi = shard_range(n, *shard) if device else (0, n)
        rs = di[(di[:, 2] == l[1]) & (di[:, 1] >= lo) & (di[:, 1] < hi)]
        assert len(rs) == hi - lo
        ev["cap_sample"] += (hi - lo) if device else n                             # DEVICE_SHARD_SHARE
        live = rs[(rs[:, 6] > 0) & (rs[:, 7] < np.inf)]
        ev["shadow_ray"] += len(live)
        later = np.array([key(r[3:6]) in deferred for r in live], dtype=bool) if device and deferred else np.zeros(len(live), dtype=bool)
        open_ = live[:, 9] == 0
        if device and rough:                                                        # DEVICE_DIRECT_WEIGHT
            k = int((open_ | later).sum())
            ev["oren_nayar_direct"] += k
            flop += k * C["F_OREN_NAYAR_DIRECT"]
        elif rough:
            ev["oren_nayar_direct"] += len(live)
            flop += len(live) * C["F_OREN_NAYAR"]
            transc += len(live) * C["T_OREN_NAYAR"]
        k = int((open_ & ~later).sum())                                             # DEVICE_DEFERRED_TAIL
        ev["direct_tail"] += k
        flop += k * C["F_DIRECT_TAIL"]
    if len(pa):
        n = int(pa[0, 1])
        ev["path_setups"] = 1
        flop += C["F_FRAME"]
        lo, hi = shard_range(n, *shard) if device else (0, n)
        rs = ps[(ps[:, 1] >= lo) & (ps[:, 1] < hi)]
        assert len(rs) == hi - lo
        ev["cap_sample"] += (hi - lo) if device else n
        live = rs[rs[:, 5] > 0]
        ev["path_tail"] = len(live)
        flop += len(live) * C["F_PATH_TAIL"]
        if rough:
            ev["oren_nayar_path"] = len(live)
            flop += len(live) * C["F_OREN_NAYAR"]
            transc += len(live) * C["T_OREN_NAYAR"]
        ev["trans_ray"] = len(live) - (sum(1 for r in live if key(r[2:5]) in hard_path) if device else 0)   # DEVICE_HARD_PATH_TRANS
    flop += ev["cap_sample"] * C["F_CAP_SAMPLE"]
    transc += ev["cap_sample"] * C["T_CAP_SAMPLE"]
    return _priced(ev, flop, transc)


def ledger_hit(rows, offs, prm=None, device=False):
    """scene_s_lum for one hit outside its sample loops (rows: the tap of the hit; offs: the hit's distance, which decides whether the
    exit object absorbs).  A hit record or a walk ray's hit; device=True: what shade_hit books, which needs prm for DEVICE_DEAD_CHILD."""
    C = costs()
    ev = {k: 0 for k in LEDGER_KEYS}
    if not len(rows):
        return _priced(ev, 0, 0)                                                    # depth 0 or too little intensity: no call
    ev["lum"] = 1
    flop, transc = C["F_LUM_FIXED"], 0
    if len(rows_of(rows, "emission")):
        return _priced(ev, flop + C["F_EMISSION"], 0)
    for r in rows:
        kind = int(r[0])
        if kind == T["fresnel"]:
            flop += C["F_FRESNEL_REFL"]
        elif kind == T["chromatic"]:
            flop += C["F_REFLECTION"]
        elif kind == T["refraction"]:
            flop += C["F_FRESNEL_REFR"]
        elif kind == T["diffuse"]:
            flop += C["F_SHADE_DIFFUSE"] + C["F_SEED"]
            transc += C["T_SHADE_DIFFUSE"] + C["T_SEED"]
        elif kind == T["absorb"] and offs > 0:
            flop += C["F_ABSORB"]
            transc += C["T_ABSORB"]
        if device and kind in (T["fresnel"], T["chromatic"], T["refraction"]) and (int(r[8]) == 0 or r[7] < prm.trace_min_intensity):
            ev["trans_ray"] += 2                                                    # DEVICE_DEAD_CHILD
    return _priced(ev, flop, transc)


def ledger_camera(n):
    """the camera rays of n positions (sample_position of the oracle, the camera form of k_walk)"""
    return _priced({}, n * costs()["F_CAMERA_RAY"], 0)


def camera_ray(prm, p):
    """sample_position of the oracle for position p, one IEEE operation at a time: the ray [6] to the bit (camera_setup, v3_of_length,
    v3_von, m3_mlv of oracle/acn_oracle.c)"""
    import math

    def of_length(v):
        r = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        if abs(r - 1.0) < 1e-8:
            return list(v)
        f = 1.0 / math.sqrt(r) if r > 0 else 0.0
        return [v[0] * f, v[1] * f, v[2] * f]

    W, H = int(prm.image_width), int(prm.image_height)
    unit_f = 1.0 / (H >> 1)
    ry = of_length([float(x) for x in prm.camera_view_direction])
    rz = of_length([float(x) for x in prm.camera_top_direction])
    o_n = of_length(ry)
    f = (o_n[0] * rz[0] + o_n[1] * rz[1]) + o_n[2] * rz[2]
    rz = of_length([rz[0] - o_n[0] * f, rz[1] - o_n[1] * f, rz[2] - o_n[2] * f])
    rx = [ry[1] * rz[2] - ry[2] * rz[1], ry[2] * rz[0] - ry[0] * rz[2], ry[0] * rz[1] - ry[1] * rz[0]]
    z, x = unit_f * ((H >> 1) - float(p[1])), unit_f * (float(p[0]) - (W >> 1))
    d = of_length([x, float(prm.camera_focal_length), z])
    rot = [[rx[k], ry[k], rz[k]] for k in range(3)]                                # the transposed of { rx, ry, rz }
    D = [rot[k][0] * d[0] + rot[k][1] * d[1] + rot[k][2] * d[2] for k in range(3)]
    return np.array([float(x) for x in prm.camera_position] + D)


def frame_ledger(oracle, flat, pos):
    """the ledgers of every scene_s_lum call of the frame `pos`, added up, with the recursion of scene_lum made here from the tap's
    rows: the oracle's own books (device=False), to be compared with the counters of Oracle.render_positions"""
    total = [ledger_camera(len(pos))]
    trans = 0

    def lum(hit):
        nonlocal trans
        rows = oracle.shade_point(flat, hit)[0]
        if not len(rows):
            return
        total.append(ledger_hit(rows, hit[6]))
        total.append(ledger(rows))
        sf = rows_of(rows, "surface")
        for r in rows:
            kind = int(r[0])
            if kind in (T["fresnel"], T["chromatic"], T["refraction"]):
                trans += 2                                                          # scene_s_trans_hit: the light root and the matter root
                a, nor, ex, en = oracle.trans_hit(flat, r[1:4], r[4:7])
                if a < np.inf:
                    lum(np.concatenate([r[1:4], r[4:7], [a], nor, [ex, en, r[8], r[7]]]))
            elif kind == T["path"] and r[5] > 0 and r[14]:
                lum(np.concatenate([sf[0, 1:4], r[2:5], [r[7]], r[8:11], [r[11], r[12], hit[12] - 10, r[13]]]))

    for p in pos:
        ray = camera_ray(flat.params, p)
        trans += 2
        a, nor, ex, en = oracle.trans_hit(flat, ray[:3], ray[3:])
        if a < np.inf:
            lum(np.concatenate([ray, [a], nor, [ex, en, flat.params.trace_depth, 1.0]]))
    out = add_ledgers(total)
    out["trans_ray"] += trans
    return out


def frame_work_identities(g, c):
    """fp64 work by the cost table of SURVEY.md App. B (actinon_amd/csrc/acn_costs.h): the oracle tallies the reference's algorithm,
    the device what it executed.  The oracle keeps the part scene_s_lum and the camera ray book themselves apart (flop_shade,
    transc_shade: oracle/acn_oracle.h); the device can skip none of those events, only geometry -- any-hit shadow tests, envelope
    pruning, the cone cull.  g: Handle.last_counters of a frame, c: the oracle's counters of the same positions."""
    C = costs()
    assert c["oren_nayar_direct"] + c["oren_nayar_path"] == c["oren_nayar"] and c["oren_nayar_direct"] > 0 and c["oren_nayar_path"] > 0
    # transcendentals, every difference by name:
    #   the direct-light loop's weight is a closed form without a transcendental (oren_nayar_weight_direct: that weight only scales a
    #   colour), where the oracle books ACN_T_OREN_NAYAR per sample that reaches the light; the path loop keeps the exact form
    #   (ACN_T_SAT: neither side books the gamma curve: the device resolves in a kernel of its own, the oracle's cl_sat is not tallied)
    #   geometry: ACN_T_ROUGHNESS per perturbed normal is the only transcendental outside scene_s_lum -- this scene has no rough surface
    assert c["transc"] == c["transc_shade"], "the scene has a rough surface: its term belongs into the identity below"
    assert g["transcendentals"] == c["transc_shade"] - C["T_OREN_NAYAR"] * c["oren_nayar_direct"], (g["transcendentals"], c["transc_shade"], c["oren_nayar_direct"])
    # flop: at least the shading part, less the exact weight of the direct loop (the device books ACN_F_OREN_NAYAR_DIRECT instead, and
    # only for a sample no in-line element occluded: not counted here, so this bound leaves them out), at most the oracle's all
    assert c["flop_shade"] - C["F_OREN_NAYAR"] * c["oren_nayar_direct"] <= g["flop"] <= c["flop"], (g["flop"], c["flop_shade"], c["flop"], c["oren_nayar_direct"])
