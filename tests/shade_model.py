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
