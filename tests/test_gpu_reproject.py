"""acn_project_points* and acn_reproject* on the GPU (include/actinon_hip.h) against the numpy model of tests/reproject_model.py, bit for
bit (test_reproject_cpu.py checks the model against answers known without it): hand-made records, rendered frames of an orbiting
camera, the projection as the inverse of the camera rays, a sequence of four frames, tools/render_turntable.py --temporal, and the
calls' contracts: streams, refusals, the renderer left alone.  Bit for bit means lens_layers_model.same_bits: which NaN a NaN is, the
header leaves open."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

import actinon_amd as A
import lens_layers_model as Y
import reproject_model as R
import scenes_util as S
import stats_model as T
from actinon_amd import abi
from actinon_amd._lib import hip
from actinon_amd.cameras import orbit_camera

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4
LENS = dict(samples=K, jitter=True)                                           # the samples of tools/render_turntable.py --temporal
N_HAND = 64 * 2 + 3                                                           # a wavefront boundary and a tail
# sha256 over the two files `render_turntable.py SCENE OUT_%d.pnm --frames 2 --orbit-deg 2` writes for wine_glass_c2 96 x 54, frame 0
# then frame 1, taken on the commit before --temporal existed
PLAIN_SHA256 = "649bbdc3d444acf0f2e37407a68b5a544f388a11b8593fbb4c3cc426654816bb"


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def flat():
    return S.build("wine_glass_c2")[1]


@pytest.fixture(scope="module")
def h(flat):
    handle = A.Handle(flat)
    yield handle
    handle.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want):
    bad = Y.same_bits(got, want)
    got, want = np.asarray(got), np.asarray(want)
    assert len(bad) == 0, (len(bad), bad[:5], [got[tuple(i)] for i in bad[:5]], [want[tuple(i)] for i in bad[:5]])


def copy_params(p):
    q = abi.Params()
    C.memmove(C.addressof(q), C.addressof(p), C.sizeof(abi.Params))
    return q


def moved(params, degrees):
    """a copy of params with the camera orbit_camera gives"""
    q = copy_params(params)
    for k, v in orbit_camera(params, degrees).items():
        getattr(q, k)[:] = v
    return q


def reproject_dev(h, cur, prev_params, prev_surf, prev_stats, stream=None, **params):
    """the _dev form on torch buffers with a NaN record behind every buffer -> ( stats, motion ) read back; the inputs stay"""
    import torch
    n = len(cur)
    up = lambda a, stride: torch.cat([torch.from_numpy(np.ascontiguousarray(a)).reshape(-1, stride),
                                      torch.full((1, stride), float("nan"), dtype=torch.float64)]).to("cuda")
    d_cur, d_ps, d_pt = up(cur, 16), up(prev_surf, 16), up(prev_stats, 8)
    d_out = torch.full((n + 1, 8), float("nan"), dtype=torch.float64, device="cuda")
    d_motion = torch.full((n + 1, 2), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    h.reproject_dev(d_cur.data_ptr(), n, prev_params, d_ps.data_ptr(), d_pt.data_ptr(), d_out.data_ptr(), d_motion.data_ptr(), stream=stream, **params)
    torch.cuda.synchronize()
    out, motion = d_out.cpu().numpy(), d_motion.cpu().numpy()
    assert np.isnan(out[-1]).all() and np.isnan(motion[-1]).all()
    assert_same_bits(d_cur.cpu().numpy()[:-1], cur)
    assert_same_bits(d_ps.cpu().numpy()[:-1], prev_surf)
    assert_same_bits(d_pt.cpu().numpy()[:-1], prev_stats)
    return out[:-1], motion[:-1]


# ---- hand-made records against the model ----
@pytest.mark.parametrize("key", list(R.PARAM_SETS))
def test_hand_made_records_against_the_model(h, detmath_cpu, key):
    """position i is pattern i % P of reproject_model.patterns against a previous raster of 7 x 5: zero weights, taps off every edge,
    points that do not project, misses, classes, EMPTY taps, both thresholds at and one ulp beyond, the cap, every kind bit, hops.
    The host form and the _dev form; the handle's own scene (the wine glass) and camera play no part"""
    params = R.PARAM_SETS[key]
    cur = R.tiled(N_HAND)
    surf, st = R.prev_raster()
    prm = R.axis_params()
    detail = {}
    want, want_motion = R.reproject(detmath_cpu, cur, prm, surf, st, detail=detail, **params)
    assert 0 < T.empty(want).sum() < N_HAND and detail["valid"].any(axis=0).all() and not detail["valid"].all(axis=0).any()
    got, motion = h.reproject(cur, prm, surf, st, **params)
    assert_same_bits(got.raw, want)
    assert_same_bits(motion, want_motion)
    got, motion = reproject_dev(h, cur, prm, surf, st, **params)
    assert_same_bits(got, want)
    assert_same_bits(motion, want_motion)
    assert (got[~T.empty(got), 0] >= 1.0).all() and (got[T.empty(got)] == 0).all()


def test_a_position_does_not_depend_on_its_neighbours(h):
    cur = R.tiled(N_HAND)
    surf, st = R.prev_raster()
    prm = R.axis_params()
    out, motion = reproject_dev(h, cur, prm, surf, st)
    sel = np.array([0, 7, 63, 64, 130])
    few, few_motion = reproject_dev(h, cur[sel], prm, surf, st)
    assert_same_bits(few, out[sel])
    assert_same_bits(few_motion, motion[sel])
    perm = np.random.default_rng(1).permutation(N_HAND)
    p_out, p_motion = reproject_dev(h, cur[perm], prm, surf, st)
    assert_same_bits(p_out, out[perm])
    assert_same_bits(p_motion, motion[perm])


def test_on_a_callers_stream_and_without_a_motion_plane(h, detmath_cpu):
    """behind copies that fill the inputs on that stream; the call does not synchronise: the result is right only if it ran in stream order"""
    import torch
    cur = R.tiled(N_HAND)
    surf, st = R.prev_raster()
    prm = R.axis_params()
    want, _ = R.reproject(detmath_cpu, cur, prm, surf, st)
    src = [torch.from_numpy(a).to("cuda") for a in (cur, surf, st)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_cur, d_ps, d_pt = [torch.zeros_like(a) for a in src]
        for d, a in zip((d_cur, d_ps, d_pt), src):
            d.copy_(a)                                                        # kernels on s: the inputs are not there before them
        d_out = torch.full((N_HAND, 8), float("nan"), dtype=torch.float64, device="cuda")
        h.reproject_dev(d_cur.data_ptr(), N_HAND, prm, d_ps.data_ptr(), d_pt.data_ptr(), d_out.data_ptr(), None, stream=s.cuda_stream)
    s.synchronize()
    assert_same_bits(d_out.cpu().numpy(), want)


# ---- rendered frames ----
def frame_records(hd, params, pos):
    """first-hit surface records and K jittered samples' statistics of the positions under `params`"""
    hd.set_params(camera_position=params.camera_position[:], camera_view_direction=params.camera_view_direction[:])
    surf = hd.surface_positions(pos).raw
    st = hd.render_lens_stats(pos, linear=True, **LENS)[1].raw
    return surf, st


@pytest.mark.parametrize("scene,degrees,allow_fresnel,seen", [("wine_glass_c2", 1.0, False, 0.998), ("wine_glass_c2", 3.0, False, 0.982),
                                                              ("primitives_path", 1.0, True, 0.983), ("textured", 1.0, True, 0.994)])
def test_rendered_frames_against_the_model(detmath_cpu, scene, degrees, allow_fresnel, seen):
    """the previous frame at the scene's camera, the current one `degrees` further on its orbit.  Both planes equal the model bit for
    bit; the motion plane equals acn_project_points on a handle set to the previous params; n >= 1 on every record that is not EMPTY;
    and at least 0.95 of the ELIGIBLE positions get a history (`seen`: the share a CPU prototype on the oracle's records gave)."""
    flat = S.build(scene)[1]
    pos = S.positions(flat)
    params = dict(reject_kinds=abi.ACN_REPROJECT_DEFAULT_REJECT_KINDS & ~abi.ACN_SURF_FRESNEL) if allow_fresnel else {}
    hd = A.Handle(flat)
    prev_params = copy_params(flat.params)
    cur_params = moved(flat.params, degrees)
    prev_surf, prev_st = frame_records(hd, prev_params, pos)
    hd.set_params(camera_position=cur_params.camera_position[:], camera_view_direction=cur_params.camera_view_direction[:])
    cur = hd.surface_positions(pos).raw                                       # the handle's camera is the CURRENT one during the call
    got, motion = hd.reproject(cur, prev_params, prev_surf, prev_st, **params)
    detail = {}
    want, want_motion = R.reproject(detmath_cpu, cur, prev_params, prev_surf, prev_st, detail=detail, **params)
    assert_same_bits(got.raw, want)
    assert_same_bits(motion, want_motion)
    hd.set_params(camera_position=prev_params.camera_position[:], camera_view_direction=prev_params.camera_view_direction[:])
    q, depth = hd.project_points(cur[:, 1:4])
    hd.close()
    hit = detail["hit"]
    assert_same_bits(motion[hit], q[hit])
    assert np.isnan(motion[~hit]).all() and (depth[hit & ~np.isnan(q[:, 0])] > 0).all()
    has = ~T.empty(got.raw)
    assert (got.raw[has, 0] >= 1.0).all() and (got.raw[has, 0] <= 32.0).all() and (got.raw[~has] == 0).all()
    eligible = detail["eligible"]
    share = has[eligible].mean()
    print(f"{scene} {flat.params.image_width}x{flat.params.image_height}, {degrees} degrees: {int(eligible.sum())} of {len(pos)} positions ELIGIBLE, "
          f"{share:.4f} of them with a history (CPU prototype: {seen}); mean n of a history {got.raw[has, 0].mean():.3f}")
    assert eligible.sum() >= len(pos) // 4 and not has[~eligible].any()
    assert share >= 0.95


# ---- acn_project_points ----
def test_projection_inverts_the_camera_rays(h, detmath_cpu, flat):
    """acn_project_points( origin + direction * t of acn_camera_rays( pos ) ) is pos within 1e-9 for t in { 0.5, 7, 300 }; the call equals
    the model bit for bit; points behind the camera and at its depth 0 give NaN and their depth"""
    import lens_model as M
    rng = np.random.default_rng(3)
    pos = np.concatenate([S.positions(flat)[::11], rng.uniform(-20.0, 120.0, (200, 2))])
    rays = h.camera_rays(pos)
    cam = M.Camera(detmath_cpu, h.params)
    for t in (0.5, 7.0, 300.0):
        pts = rays[:, :3] + rays[:, 3:] * t
        q, depth = h.project_points(pts)
        err = float(np.abs(q - pos).max())
        print(f"t = {t}: max | project( camera_ray( pos )( t ) ) - pos | = {err:.2e}")
        assert err <= 1e-9
        want_q, want_depth, _ = R.project(cam, pts)
        assert_same_bits(q, want_q)
        assert_same_bits(depth, want_depth)
    o = rays[0, :3]
    pts = np.stack([o - rays[0, 3:] * 2.0, o, o + np.array([np.nan, 0, 0]), o + rays[5, 3:] * np.inf, o + cam.V * 3.0])
    q, depth = h.project_points(pts)
    want_q, want_depth, ok = R.project(cam, pts)
    assert_same_bits(q, want_q)
    assert_same_bits(depth, want_depth)
    assert list(ok) == [False, False, False, False, True] and np.isnan(q[:4]).all() and depth[0] < 0 and depth[1] == 0


def test_project_points_dev_on_a_stream(h):
    import torch
    pts = np.random.default_rng(4).uniform(-5.0, 5.0, (N_HAND, 3))
    q, depth = h.project_points(pts)
    src = torch.from_numpy(pts).to("cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_pts = torch.zeros_like(src)
        d_pts.copy_(src)
        d_q = torch.full((N_HAND + 1, 2), float("nan"), dtype=torch.float64, device="cuda")
        d_depth = torch.full((N_HAND + 1,), float("nan"), dtype=torch.float64, device="cuda")
        h.project_points_dev(d_pts.data_ptr(), N_HAND, d_q.data_ptr(), d_depth.data_ptr(), stream=s.cuda_stream)
        d_q2 = torch.full((N_HAND + 1, 2), float("nan"), dtype=torch.float64, device="cuda")
        h.project_points_dev(d_pts.data_ptr(), N_HAND, d_q2.data_ptr(), None, stream=s.cuda_stream)       # the depth is optional
    s.synchronize()
    assert_same_bits(d_q.cpu().numpy()[:-1], q)
    assert_same_bits(d_q2.cpu().numpy()[:-1], q)
    assert_same_bits(d_depth.cpu().numpy()[:-1], depth)
    assert np.isnan(d_q.cpu().numpy()[-1]).all() and np.isnan(d_depth.cpu().numpy()[-1])


# ---- a sequence of frames ----
def test_a_sequence_accumulates(flat):
    """Four frames, 1 degree of orbit per frame, K = 4 jittered samples each: reproject against the frame before, then merge, all on the
    device.  Over the positions whose merged n is at least 2 K the linear RMSE of the last frame's accumulated mean against a converged
    frame of the last camera (K = 64, another seed) is below that of its own K = 4 mean.  The ratio is printed, no value is fixed for it."""
    import torch
    n = int(flat.params.image_width * flat.params.image_height)
    hd = A.Handle(flat)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    d_pos = torch.from_numpy(S.positions(flat)).to("cuda")
    d_surf, d_prev_surf, d_cur, d_acc, d_prev = new(n, 16), new(n, 16), new(n, 8), new(n, 8), new(n, 8)
    torch.cuda.synchronize()
    prev_params = None
    for f in range(4):
        prm = moved(flat.params, 1.0 * f)
        hd.set_params(camera_position=prm.camera_position[:], camera_view_direction=prm.camera_view_direction[:])
        hd.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr())
        hd.render_lens_stats_main_pass_dev(0, n, None, d_cur.data_ptr(), linear=True, seed=f, **LENS)
        if f:
            hd.reproject_dev(d_surf.data_ptr(), n, prev_params, d_prev_surf.data_ptr(), d_prev.data_ptr(), d_acc.data_ptr())
            hd.lens_stats_merge_dev(d_acc.data_ptr(), n, d_cur.data_ptr(), n)
        else:
            d_acc.copy_(d_cur)
            torch.cuda.synchronize()
        if f < 3:
            d_surf, d_prev_surf = d_prev_surf, d_surf
            d_acc, d_prev = d_prev, d_acc
        prev_params = prm
    acc, raw = d_acc.cpu().numpy(), d_cur.cpu().numpy()
    ref = hd.render_lens(S.positions(flat), linear=True, samples=64, jitter=True, seed=99)
    assert hd.info()["learning_passes"] == 1
    hd.close()
    assert (raw[:, 0] == K).all() and (acc[:, 0] >= K).all() and acc[:, 0].max() <= 32.0 + K
    sel = acc[:, 0] >= 2 * K
    assert sel.mean() > 0.5
    rmse = lambda x: float(np.sqrt(np.mean((x[sel] - ref[sel]) ** 2)))
    e_acc, e_raw = rmse(acc[:, 1:4]), rmse(raw[:, 1:4])
    print(f"wine_glass_c2 96x54, 4 frames of K={K} at 1 degree: {int(sel.sum())} of {n} positions with n >= {2 * K} (mean n {acc[sel, 0].mean():.2f}); "
          f"linear RMSE vs K=64: raw {e_raw:.4e}  accumulated {e_acc:.4e}  ratio {e_acc / e_raw:.3f}")
    assert e_acc < e_raw


# ---- the tool ----
def test_the_turntable_tool(tmp_path, flat):
    """--temporal writes its frames on one handle with one learning pass; without it the command writes the bytes it wrote before the
    option existed"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_turntable as tool
    scene = tmp_path / "scene.npz"
    flat.save(str(scene))
    tool.main([str(scene), str(tmp_path / "plain_%d.pnm"), "--frames", "2", "--orbit-deg", "2"])
    plain = [open(tmp_path / f"plain_{f}.pnm", "rb").read() for f in range(2)]
    assert hashlib.sha256(plain[0] + plain[1]).hexdigest() == PLAIN_SHA256
    frames = {}
    info, report = tool.render_temporal(flat, 3, 3.0, lambda f, rgb8: frames.__setitem__(f, rgb8.copy()), samples=K, denoise=True, max_history=16.0)
    assert info["learning_passes"] == 1 and info["param_sets"] == 2
    assert sorted(frames) == [0, 1, 2] and all(v.shape == (54, 96, 3) and v.dtype == np.uint8 for v in frames.values())
    assert report[0] == (0.0, float(K)) and all(took > 0.5 and K < mean_n <= 16.0 + K for took, mean_n in report[1:])
    tool.main([str(scene), str(tmp_path / "temporal_%d.pnm"), "--frames", "2", "--orbit-deg", "2", "--temporal", "--samples", str(K), "--allow-fresnel"])
    for f in range(2):
        data = open(tmp_path / f"temporal_{f}.pnm", "rb").read()
        assert data.startswith(b"P6") and len(data) == len(plain[f]) and data != plain[f]
    for bad in (["--samples", "4"], ["--temporal"], ["--temporal", "--samples", "0"], ["--denoise"], ["--temporal", "--samples", "4", "--max-history", "0.5"]):
        with pytest.raises(SystemExit):
            tool.main([str(scene), str(tmp_path / "x_%d.pnm"), "--frames", "2", "--orbit-deg", "2"] + bad)


# ---- isolation ----
def test_the_calls_leave_the_renderer_alone(flat):
    pos = S.positions(flat)[::7]
    hd = A.Handle(flat)
    hd.render_positions(pos, linear=True)                                   # a warm handle
    before = hd.render_positions(pos, linear=True)
    assert hd.last_stages()["retries"] == 0
    raw = (C.c_double * 25)()
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    raw_before = list(raw)
    counters = hd.last_counters_raw(10)
    kernel_ms = hd.last_kernel_ms()
    info = hd.info()
    cur = R.tiled(N_HAND)
    surf, st = R.prev_raster()
    out, motion = hd.reproject(cur, R.axis_params(), surf, st)
    q, depth = hd.project_points(cur[:, 1:4])
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    assert list(raw) == raw_before                                          # [ 23 ], [ 24 ] included: nothing of the workspace moved
    assert list(hd.last_counters_raw(10)) == list(counters) and hd.last_kernel_ms() == kernel_ms and hd.info() == info
    after = hd.render_positions(pos, linear=True)
    assert hd.last_stages()["retries"] == 0
    assert np.array_equal(before, after)
    again, again_motion = hd.reproject(cur, R.axis_params(), surf, st)
    assert_same_bits(again.raw, out.raw)
    assert_same_bits(again_motion, motion)
    hd.close()


# ---- errors ----
def test_refusals_leave_the_output_untouched(flat):
    """Every ACN_ERR_ARG of the four calls: the status, acn_last_error, and not one word written, on host and device buffers; then the
    handle still works"""
    import torch
    n = 40
    h = A.Handle(flat)
    o = h._plain_opts(False, None)
    cur = R.tiled(n)
    surf, st = R.prev_raster()
    prm = R.axis_params()
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    d_out, d_motion, d_q, d_depth = nan(n + 1, 8), nan(n + 1, 2), nan(n, 2), nan(n)
    d_cur, d_ps, d_pt = [torch.from_numpy(a).to("cuda") for a in (cur, surf, st)]
    h_out, h_motion, h_q = np.full((n + 1, 8), np.nan), np.full((n + 1, 2), np.nan), np.full((n, 2), np.nan)
    rp = A.Handle.reproject_params()
    torch.cuda.synchronize()

    def refused(table, word):
        for name, call in table.items():
            hip.acn_render_positions(None, None, 0, None, None)            # (sets another message)
            assert call() == abi.ACN_ERR_ARG, name
            msg = hip.acn_last_error().decode()
            assert msg and word in msg, (name, msg)
            torch.cuda.synchronize()
            assert np.isnan(h_out).all() and np.isnan(h_motion).all() and np.isnan(h_q).all(), name
            assert all(bool(torch.isnan(a).all()) for a in (d_out, d_motion, d_q, d_depth)), name

    def calls(handle, opts, count=n, prev=prm, p=rp, dc=d_cur.data_ptr(), dps=d_ps.data_ptr(), dpt=d_pt.data_ptr(), do=d_out.data_ptr(), dm=d_motion.data_ptr(),
              hc=cur.ctypes.data, hps=surf.ctypes.data, hpt=st.ctypes.data, ho=h_out.ctypes.data, hm=h_motion.ctypes.data):
        ref = lambda x: None if x is None else C.byref(x)
        return {"host": lambda: hip.acn_reproject(handle, hc, count, ref(prev), hps, hpt, ref(p), ho, hm, C.byref(opts)),
                "dev": lambda: hip.acn_reproject_dev(handle, dc, count, ref(prev), dps, dpt, ref(p), do, dm, C.byref(opts))}

    only = lambda table, *names: {k: v for k, v in table.items() if k in names}
    refused(calls(None, o), "handle")
    refused(calls(h.h, o, prev=None), "prev_params")
    for kw in ("hc", "hps", "hpt", "ho"):
        refused(only(calls(h.h, o, **{kw: None}), "host"), "null")
    for kw in ("dc", "dps", "dpt", "do"):
        refused(only(calls(h.h, o, **{kw: None}), "dev"), "null")
    refused(calls(h.h, o, count=(1 << 31) + 1), "2^31")
    for field, value, word in (("image_height", 1, "raster"), ("image_width", 0, "raster"), ("image_width", 1 << 31, "2^31"), ("experimental_level", 1, "prev_params")):
        bad = R.axis_params()
        setattr(bad, field, value)
        refused(calls(h.h, o, prev=bad), word)
    for kw, buf in (("dc", d_cur), ("dps", d_ps), ("dpt", d_pt), ("do", d_out)):
        refused(only(calls(h.h, o, **{kw: buf.data_ptr() + 8}), "dev"), "align")
    refused(only(calls(h.h, o, ho=h_out.ctypes.data + 8), "host"), "align")
    refused(only(calls(h.h, o, dm=d_motion.data_ptr() + 4), "dev"), "out_motion")
    for field, value, word in (("struct_size", 3, "struct_size"), ("flags", 4, "flags"), ("normal_min", 1.5, "normal_min"), ("normal_min", float("nan"), "normal_min"),
                               ("plane_tolerance", -1.0, "plane_tolerance"), ("plane_tolerance", float("inf"), "plane_tolerance"),
                               ("max_history", 0.5, "max_history"), ("max_history", float("inf"), "max_history"), ("max_history", float("nan"), "max_history")):
        bad = A.Handle.reproject_params()
        setattr(bad, field, value)
        refused(calls(h.h, o, p=bad), word)
    world2 = h._plain_opts(False, None)
    world2.shard_world = 2
    refused(calls(h.h, world2), "sharded")
    # acn_project_points*: the refusals of acn_camera_rays*
    pts = np.zeros((n, 3))
    d_pts = torch.from_numpy(pts).to("cuda")
    refused({"null handle": lambda: hip.acn_project_points(None, pts.ctypes.data, n, h_q.ctypes.data, None),
             "null handle, dev": lambda: hip.acn_project_points_dev(None, d_pts.data_ptr(), n, d_q.data_ptr(), d_depth.data_ptr(), C.byref(o)),
             "null points": lambda: hip.acn_project_points(h.h, None, n, h_q.ctypes.data, None),
             "null out": lambda: hip.acn_project_points_dev(h.h, d_pts.data_ptr(), n, None, d_depth.data_ptr(), C.byref(o)),
             "too many": lambda: hip.acn_project_points_dev(h.h, d_pts.data_ptr(), 0xFFFFFF01, d_q.data_ptr(), d_depth.data_ptr(), C.byref(o))}, "")
    # nothing to do is ACN_OK and writes nothing, null buffers included
    for call in (lambda: hip.acn_reproject_dev(h.h, None, 0, C.byref(prm), None, None, None, None, None, C.byref(o)),
                 lambda: hip.acn_reproject(h.h, None, 0, C.byref(prm), None, None, None, None, None, None),
                 lambda: hip.acn_project_points_dev(h.h, None, 0, None, None, C.byref(o)),
                 lambda: hip.acn_project_points(h.h, None, 0, None, None)):
        assert call() == abi.ACN_OK
    torch.cuda.synchronize()
    assert np.isnan(h_out).all() and all(bool(torch.isnan(a).all()) for a in (d_out, d_motion, d_q, d_depth))
    # and the handle works, with null parameters too
    assert hip.acn_reproject_dev(h.h, d_cur.data_ptr(), n, C.byref(prm), d_ps.data_ptr(), d_pt.data_ptr(), None, d_out.data_ptr(), d_motion.data_ptr(), C.byref(o)) == abi.ACN_OK
    got, _ = h.reproject(cur, prm, surf, st)
    assert_same_bits(d_out.cpu().numpy()[:n], got.raw)
    assert np.isnan(d_out.cpu().numpy()[n]).all()
    h.close()
