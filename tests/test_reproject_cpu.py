"""acn_project_points and acn_reproject (include/actinon_hip.h) without a GPU: the numpy model of tests/reproject_model.py on hand-made
records whose answers are written down here, the constants against the header, the projection against the oracle's first hits, and
the host-side checks of csrc/acn_reproject_host.h in a stand-alone program built with the address and undefined-behaviour
sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import actinon_amd as A
import lens_model as M
import reproject_model as R
import scenes_util as S
import stats_model as T
import surface_model as F
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["acn_project_points", "acn_project_points_dev", "acn_reproject", "acn_reproject_dev"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def flat_raster(rng, w=R.PW, h=R.PH, n=4.0):
    """a previous raster without special pixels: the surface points of the pixel centres, records of n samples"""
    surf = np.stack([R.surface_record(x + 0.5, y + 0.5, width=w, height=h) for y in range(h) for x in range(w)])
    st = np.zeros((w * h, 8))
    st[:, 0] = n
    st[:, 1:4] = rng.uniform(0.0, 2.0, (w * h, 3))
    st[:, 4:7] = rng.uniform(0.0, 1.0, (w * h, 3))
    return surf, st


# ---- the header, the mirror, the documents ----
def test_symbols_and_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\s*\(", text, re.M), name
        assert hasattr(hip, name)
    for method in ("project_points", "project_points_dev", "reproject", "reproject_dev", "reproject_params"):
        assert callable(getattr(A.Handle, method))
    define = lambda name: re.search(r"^#define " + name + r"\s+(.+?)\s*(/\*.*)?$", text, re.M).group(1)
    assert int(define("ACN_REPROJECT_KINDS_SET").rstrip("u")) == abi.ACN_REPROJECT_KINDS_SET == R.KINDS_SET
    assert int(define("ACN_REPROJECT_HOPS_SET").rstrip("u")) == abi.ACN_REPROJECT_HOPS_SET == R.HOPS_SET
    assert define("ACN_REPROJECT_DEFAULT_REJECT_KINDS") == "( ACN_SURF_CHROMATIC | ACN_SURF_FRESNEL | ACN_SURF_TRANSPARENT | ACN_SURF_CUT )"
    assert (abi.ACN_SURF_CHROMATIC | abi.ACN_SURF_FRESNEL | abi.ACN_SURF_TRANSPARENT | abi.ACN_SURF_CUT) == abi.ACN_REPROJECT_DEFAULT_REJECT_KINDS == R.DEFAULT_REJECT_KINDS
    assert int(define("ACN_REPROJECT_DEFAULT_MAX_HOPS")) == abi.ACN_REPROJECT_DEFAULT_MAX_HOPS == R.DEFAULT_MAX_HOPS
    assert float(define("ACN_REPROJECT_DEFAULT_NORMAL_MIN")) == abi.ACN_REPROJECT_DEFAULT_NORMAL_MIN == R.DEFAULT_NORMAL_MIN == 0.9
    assert float(define("ACN_REPROJECT_DEFAULT_PLANE_TOLERANCE")) == abi.ACN_REPROJECT_DEFAULT_PLANE_TOLERANCE == R.DEFAULT_PLANE_TOLERANCE == 0.01
    assert float(define("ACN_REPROJECT_DEFAULT_MAX_HISTORY")) == abi.ACN_REPROJECT_DEFAULT_MAX_HISTORY == R.DEFAULT_MAX_HISTORY == 32.0
    # the struct: the members in the header's order, 40 bytes
    body = re.search(r"typedef struct acn_reproject_params\s*\{(.*?)\}\s*acn_reproject_params;", text, re.S).group(1)
    members = re.findall(r"^\s*(?:uint32_t|int32_t|double)\s+(\w+);", body, re.M)
    assert members == [f[0] for f in abi.ReprojectParams._fields_] and C.sizeof(abi.ReprojectParams) == 40
    p = A.Handle.reproject_params()
    assert (p.struct_size, p.flags, p.reject_kinds, p.max_hops, p.normal_min, p.plane_tolerance, p.max_history) == (40, 0, 0, 0, 0.0, 0.0, 0.0)
    p = A.Handle.reproject_params(reject_kinds=0, max_hops=0)
    assert p.flags == abi.ACN_REPROJECT_KINDS_SET | abi.ACN_REPROJECT_HOPS_SET


def test_the_documents_state_the_call():
    header = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for word in ("PROJECTED", "ELIGIBLE", "VALID", "GATHER", "n >= 1 holds", "WORLD IS TAKEN TO BE AT REST", "rounding is monotone"):
        assert word in header, word
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "acn_reproject" in open(os.path.join(ROOT, doc)).read(), doc
    assert "3e" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"k_reproject\b", open(os.path.join(ROOT, "Makefile")).read())


def test_entry_points_refuse_a_null_handle():
    buf = np.full((4, 16), 7.25)
    prm = R.axis_params()
    assert hip.acn_project_points(None, buf.ctypes.data, 4, buf.ctypes.data, None) == abi.ACN_ERR_ARG
    assert hip.acn_project_points_dev(None, buf.ctypes.data, 4, buf.ctypes.data, None, None) == abi.ACN_ERR_ARG
    for f in (hip.acn_reproject, hip.acn_reproject_dev):
        assert f(None, buf.ctypes.data, 4, C.byref(prm), buf.ctypes.data, buf.ctypes.data, None, buf.ctypes.data, None, None) == abi.ACN_ERR_ARG
        assert "handle" in hip.acn_last_error().decode()
    assert (buf == 7.25).all()


# ---- the projection ----
def test_the_axis_camera_is_exact(detmath_cpu):
    cam = M.Camera(detmath_cpu, R.axis_params())
    assert np.array_equal(cam.R, [1, 0, 0]) and np.array_equal(cam.V, [0, 1, 0]) and np.array_equal(cam.T, [0, 0, 1])
    pts = np.stack([R.point_at(x, y) for x, y in ((3.5, 2.5), (0.25, 4.75), (-5.0, 9.0))] + [np.array([0.0, -2.0, 0.0]), np.array([0.0, 0.0, 0.0])])
    q, depth, ok = R.project(cam, pts)
    assert np.array_equal(q[:3], [[3.5, 2.5], [0.25, 4.75], [-5.0, 9.0]]) and ok[:3].all()
    assert np.isnan(q[3:]).all() and not ok[3:].any() and np.array_equal(depth, [2, 2, 2, -2, 0])


def test_projection_inverts_the_oracles_camera_rays(oracle, detmath_cpu):
    """the oracle's first hits on wine_glass_c2, 96 x 54, projected with the same camera: | q - pos | <= 1e-12 on every hit (measured
    when the model was written: 2.9e-14).  The bound: the ray direction is unit to 1e-16, the hit point pos + d * t carries relative
    1e-16 errors of coordinates of order 10, and the projection scales the sum by hh / ly * focal of order 10: 1e-14, a hundredfold margin."""
    _, flat = S.build("wine_glass_c2")
    pos = S.positions(flat)
    rec, _ = F.first_hit(oracle, flat, F.camera_rays(flat.params, pos))
    hit = rec[:, 0] < np.inf
    assert hit.sum() >= 4000
    q, depth, ok = R.project(M.Camera(detmath_cpu, flat.params), rec[hit, 1:4])
    assert ok.all() and (depth > 0).all()
    err = float(np.abs(q - pos[hit]).max())
    print(f"wine_glass_c2 96x54: {int(hit.sum())} first hits, max | q - pos | = {err:.2e}")
    assert err <= 1e-12


# ---- the model on hand-made records, answers written down here ----
def test_a_pixel_centre_returns_the_record_bit_for_bit(detmath_cpu):
    rng = np.random.default_rng(1)
    surf, st = flat_raster(rng)
    cur = np.stack([R.surface_record(x + 0.5, y + 0.5) for y in range(R.PH) for x in range(R.PW)])
    detail = {}
    out, motion = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st, detail=detail)
    assert (bits(out) == bits(st)).all()
    assert (detail["valid"].sum(axis=1) == 1).all() and detail["valid"][:, 0].all()   # one tap, the first, of weight 1
    assert np.array_equal(motion, A.main_pass_positions(R.PW, R.PH))


def test_halfway_between_four_equal_records_is_that_record(detmath_cpu):
    rng = np.random.default_rng(2)
    surf, st = flat_raster(rng)
    st[:] = np.round(st[0] * 64.0) / 64.0                                     # (dyadic: three quarters of each number are exact)
    cur = np.stack([R.surface_record(x, y) for y in range(1, R.PH) for x in range(1, R.PW)])   # the corners shared by four pixels
    detail = {}
    out, _ = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st, detail=detail)
    assert detail["valid"].all()
    assert (bits(out) == bits(np.broadcast_to(st[0], out.shape))).all()       # four weights of 1 / 4: every sum and quotient is exact


def test_weights_are_bilinear(detmath_cpu):
    """a point a quarter of the way: 9/16, 3/16, 3/16, 1/16 of a quantity that is 16 x the pixel's index"""
    rng = np.random.default_rng(3)
    surf, st = flat_raster(rng)
    st[:, 1] = 16.0 * np.arange(R.PW * R.PH)
    out, motion = R.reproject(detmath_cpu, [R.surface_record(2.75, 1.75)], R.axis_params(), surf, st)
    a = 1 * R.PW + 2
    assert out[0, 1] == 9 * a + 3 * (a + 1) + 3 * (a + R.PW) + 1 * (a + R.PW + 1) and out[0, 0] == 4.0
    assert np.array_equal(motion[0], [2.75, 1.75])


def test_history_is_capped(detmath_cpu):
    rng = np.random.default_rng(4)
    surf, st = flat_raster(rng, n=128.0)
    cur = [R.surface_record(3.5, 2.5), R.surface_record(4.0, 3.0)]
    out, _ = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st)
    p = 2 * R.PW + 3
    assert (out[:, 0] == 32.0).all()
    assert np.array_equal(out[0, 1:4], st[p, 1:4]) and np.array_equal(out[0, 4:7], st[p, 4:7] * 0.25)   # m2 scaled by 32 / 128: the variance of the mean stays
    out, _ = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st, max_history=1000.0)
    assert (out[:, 0] == 128.0).all() and np.array_equal(out[0, 4:7], st[p, 4:7])
    out, _ = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st, max_history=1.0)
    assert (out[:, 0] == 1.0).all()


def test_the_history_merged_with_new_samples_is_the_pooled_mean(detmath_cpu):
    """the model's output as the accumulator of stats_model.merge: ( n_h * mean_h + K * mean_new ) / ( n_h + K ) to rounding"""
    rng = np.random.default_rng(5)
    surf, st = flat_raster(rng, n=12.0)
    cur = np.stack([R.surface_record(float(x), float(y)) for x, y in rng.uniform(1.0, 4.0, (40, 2))])
    hist, _ = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st)
    nh = hist[:, 0:1]
    assert np.allclose(nh, 12.0, rtol=1e-15, atol=0)                          # equal n on every tap: 12 to the rounding of the weighted sums
    new = np.zeros((40, 8)); new[:, 0] = 4.0; new[:, 1:4] = rng.uniform(0.0, 2.0, (40, 3)); new[:, 4:7] = rng.uniform(0.0, 1.0, (40, 3))
    merged = T.merge(hist, new)
    assert np.array_equal(merged[:, 0:1], nh + 4.0)
    assert np.allclose(merged[:, 1:4], (nh * hist[:, 1:4] + 4.0 * new[:, 1:4]) / (nh + 4.0), rtol=1e-14, atol=0)
    lo, hi = st[:, 1:4].min(axis=0), st[:, 1:4].max(axis=0)
    assert ((hist[:, 1:4] >= lo) & (hist[:, 1:4] <= hi)).all()                # a weighted mean lies between its taps


def test_the_hand_made_patterns(detmath_cpu):
    """every pattern of reproject_model.patterns under the three parameter sets: which records are EMPTY, which motions NaN"""
    names, cur = R.patterns()
    surf, st = R.prev_raster()
    at = lambda name: names.index(name)
    res = {}
    for key, params in R.PARAM_SETS.items():
        detail = {}
        out, motion = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st, detail=detail, **params)
        res[key] = (out, motion, detail)
        empty = T.empty(out)
        assert (out[empty] == 0).all() and (out[~empty, 0] >= 1.0).all() and (out[:, 7] == 0).all()
        assert np.array_equal(np.isnan(motion[:, 0]), ~detail["projected"]) and np.array_equal(np.isnan(motion[:, 0]), np.isnan(motion[:, 1]))
        assert (empty[~detail["eligible"]]).all()
    out, motion, detail = res["defaults"]
    empty = T.empty(out)
    for name in ("behind the camera", "ly == 0", "ly == -0", "a NaN in P", "an inf in P", "an infinite depth", "a miss"):
        assert np.isnan(motion[at(name)]).all() and empty[at(name)], name
    assert 1e300 < motion[at("qx of 1e300"), 0] < np.inf and motion[at("qx of 1e300"), 1] == 2.0 and empty[at("qx of 1e300")]
    assert 1e300 < motion[at("qy of 1e300"), 1] < np.inf and empty[at("qy of 1e300")]
    for name in ("left of the image", "below the image", "another enter object", "another exit object", "hops 1 on a tap of hops 0",
                 "hops 1 on a tap of hops 1", "hops 0 on a tap of hops 1", "an EMPTY tap alone", "two EMPTY taps: all invalid",
                 "EMPTY by a NaN n and by an infinite n", "a miss tap alone", "enter and exit differ on both taps", "the normal one ulp beyond",
                 "the plane at the threshold of TOL_AT", "the plane one ulp beyond", "kind bits 4", "kind bits 8", "kind bits 16", "kind bits 64",
                 "kind bits 26"):
        assert empty[at(name)] and not np.isnan(motion[at(name)]).any(), name
    for name, taps in (("a pixel centre: one tap of weight 1", [1, 0, 0, 0]), ("halfway between four", [1, 1, 1, 1]), ("halfway, one EMPTY tap", [0, 1, 1, 1]),
                       ("tx == 0", [1, 0, 1, 0]), ("ty == 0", [1, 1, 0, 0]), ("x0 == -1", [0, 1, 0, 1]), ("x0 == W' - 1", [1, 0, 0, 0]),
                       ("y0 == -1", [0, 0, 1, 1]), ("y0 == H' - 1", [1, 1, 0, 0]), ("the corner x0 == -1, y0 == -1", [0, 0, 0, 1]),
                       ("the corner beyond W', H'", [1, 0, 0, 0]), ("a miss tap among four", [1, 0, 1, 1]), ("one tap of two matches", [0, 1, 0, 0]),
                       ("classes differ on two of four", [0, 0, 1, 1]), ("the normal at the threshold", [1, 0, 0, 0]),
                       ("the normal: one of two taps", [1, 0, 0, 0]), ("kind bits 1", [1, 0, 0, 0]), ("kind bits 2", [1, 0, 0, 0]),
                       ("kind bits 32", [1, 0, 0, 0]), ("kind bits 35", [1, 0, 0, 0])):
        assert list(detail["valid"][at(name)].astype(int)) == taps, (name, detail["valid"][at(name)])
    p = lambda x, y: y * R.PW + x
    assert out[at("n == 1"), 0] == 1.0 and out[at("n at max_history"), 0] == 32.0
    assert out[at("n above max_history"), 0] == 32.0 and np.array_equal(out[at("n above max_history"), 4:7], st[p(1, 4), 4:7] * (32.0 / 40.0))
    assert out[at("n one ulp above max_history"), 0] == 32.0
    assert out[at("n of 1 and 40 mixed"), 0] == 20.5                          # ( 0.5 * 1 + 0.5 * 40 ) / 1
    assert (bits(out[at("n at max_history")]) == bits(st[p(2, 4)])).all()
    assert out[at("a mean of -0.0"), 1] == 0.0 and not np.signbit(out[at("a mean of -0.0"), 1])
    # exact thresholds, hops allowed, only emitters rejected
    out, motion, detail = res["exact"]
    empty = T.empty(out)
    for name in ("the plane at the threshold of TOL_AT", "hops 1 on a tap of hops 1", "kind bits 4", "kind bits 8", "kind bits 16", "kind bits 64", "kind bits 26"):
        assert not empty[at(name)], name
    for name in ("the plane one ulp beyond", "hops 1 on a tap of hops 0", "hops 0 on a tap of hops 1", "kind bits 1", "kind bits 35"):
        assert empty[at(name)], name
    assert (out[~empty, 0] <= 8.0).all() and (out[~empty, 0] >= 1.0).all()
    # no normal test, every kind, a cap of 1
    out, motion, detail = res["all kinds, no normal test"]
    empty = T.empty(out)
    for name in ("the normal one ulp beyond", "the plane one ulp beyond", "kind bits 1", "kind bits 64"):
        assert not empty[at(name)], name
    assert (out[~empty, 0] == 1.0).all()


def test_tiled_positions_repeat_the_patterns(detmath_cpu):
    names, cur = R.patterns()
    tiled = R.tiled(64 * 2 + 3)
    assert len(tiled) == 131 and len(names) < 128                             # every pattern is there, and meets more than one lane
    surf, st = R.prev_raster()
    a, _ = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st)
    b, _ = R.reproject(detmath_cpu, tiled, R.axis_params(), surf, st)
    assert (bits(b) == bits(a[np.arange(131) % len(cur)])).all()


# ---- the host-side checks under the sanitizers ----
def test_host_checks_in_a_sanitized_program(tmp_path):
    """the checks of acn_reproject_host.h compiled with tests/csrc/reproject_cpu.cpp into a program of its own with
    -fsanitize=address,undefined; nothing sanitized is loaded here"""
    exe = tmp_path / "reproject_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "reproject_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
