"""acn_reproject_moving* on the GPU (include/actinon_hip.h) against the numpy model of tests/motion_model.py, bit for bit
(test_motion_cpu.py checks the model against answers known without it): an all-REST table against acn_reproject*, the hand-made
table of eight rows, independence of the positions, a caller's stream, every refusal, two rendered frames between which an object
and the camera move, and tools/render_turntable.py --spin.  The shapes: 131 positions (a wavefront boundary and a tail), the 7 x 5
previous raster, a table of 8 rows.  Bit for bit means lens_layers_model.same_bits: which NaN a NaN is, the header leaves open."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

import actinon_amd as A
import lens_layers_model as Y
import motion_model as MM
import reproject_model as R
import stats_model as T
from actinon_amd import abi
from actinon_amd._lib import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_HAND = MM.N_HAND


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def frames():
    return MM.two_frames()


@pytest.fixture(scope="module")
def h(frames):
    handle = A.Handle(frames["prev_flat"])
    yield handle
    handle.close()


def assert_same_bits(got, want):
    bad = Y.same_bits(got, want)
    got, want = np.asarray(got), np.asarray(want)
    assert len(bad) == 0, (len(bad), bad[:5], [got[tuple(i)] for i in bad[:5]], [want[tuple(i)] for i in bad[:5]])


def moving_dev(h, cur, prev_params, prev_surf, prev_stats, table, stream=None, **params):
    """the _dev form on torch buffers with a NaN record behind every buffer, the table included -> ( stats, motion ) read back; the
    inputs stay and the NaN records stay NaN"""
    import torch
    n = len(cur)
    up = lambda a, stride: torch.cat([torch.from_numpy(np.ascontiguousarray(a)).reshape(-1, stride),
                                      torch.full((1, stride), float("nan"), dtype=torch.float64)]).to("cuda")
    d_cur, d_ps, d_pt, d_table = up(cur, 16), up(prev_surf, 16), up(prev_stats, 8), up(table, 16)
    d_out = torch.full((n + 1, 8), float("nan"), dtype=torch.float64, device="cuda")
    d_motion = torch.full((n + 1, 2), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    h.reproject_moving_dev(d_cur.data_ptr(), n, prev_params, d_ps.data_ptr(), d_pt.data_ptr(), d_table.data_ptr(), len(table), d_out.data_ptr(),
                           d_motion.data_ptr(), stream=stream, **params)
    torch.cuda.synchronize()
    out, motion = d_out.cpu().numpy(), d_motion.cpu().numpy()
    assert np.isnan(out[-1]).all() and np.isnan(motion[-1]).all()
    for d, a in ((d_cur, cur), (d_ps, prev_surf), (d_pt, prev_stats), (d_table, table)):
        back = d.cpu().numpy()
        assert_same_bits(back[:-1], a)
        assert np.isnan(back[-1]).all()
    return out[:-1], motion[:-1]


# ---- an all-REST table is acn_reproject ----
@pytest.mark.parametrize("key", list(R.PARAM_SETS))
def test_an_all_rest_table_gives_the_bits_of_acn_reproject(h, key):
    """the host form and the _dev form, statistics and motion, against Handle.reproject on the same inputs; rows 3, 4 and 5 are read"""
    params = R.PARAM_SETS[key]
    cur = R.tiled(N_HAND)
    cur[::3, 7] = np.where(cur[::3, 7] == 3, 5, cur[::3, 7])
    surf, st = R.prev_raster()
    surf[::2, 7] = np.where(surf[::2, 7] == 3, 5, surf[::2, 7])
    prm = R.axis_params()
    want, want_motion = h.reproject(cur, prm, surf, st, **params)
    assert 0 < T.empty(want.raw).sum() < N_HAND
    got, motion = h.reproject_moving(cur, prm, surf, st, MM.rest_table(8), **params)
    assert_same_bits(got.raw, want.raw)
    assert_same_bits(motion, want_motion)
    got, motion = moving_dev(h, cur, prm, surf, st, MM.rest_table(8), **params)
    assert_same_bits(got, want.raw)
    assert_same_bits(motion, want_motion)


# ---- the hand-made table against the model ----
@pytest.mark.parametrize("key", list(R.PARAM_SETS))
def test_hand_made_motion_against_the_model(h, detmath_cpu, key):
    """the cases of motion_model.hand_cases with the table of eight rows: REST, the exact shift, the exact quarter turn, the tilt with
    previous normals at normal_min and one ulp beyond, NONE, a NaN state, the caps 4 and 64; exit objects, an id of 8 and of -1.  The
    host form and the _dev form.  The model's detail shows every state and both outcomes of every VALID term"""
    params = R.PARAM_SETS[key]
    prm = R.axis_params()
    table = MM.hand_table()
    details = []
    for name, cur, surf, st in MM.hand_cases():
        detail = {}
        want, want_motion = MM.reproject_moving(detmath_cpu, cur, prm, surf, st, table, detail=detail, **params)
        details.append(detail)
        got, motion = h.reproject_moving(cur, prm, surf, st, table, **params)
        assert_same_bits(got.raw, want)
        assert_same_bits(motion, want_motion)
        got, motion = moving_dev(h, cur, prm, surf, st, table, **params)
        assert_same_bits(got, want)
        assert_same_bits(motion, want_motion)
        assert (got[~T.empty(got), 0] >= 1.0).all() and (got[T.empty(got)] == 0).all(), name
        assert 0 < T.empty(want).sum()
    decided = MM.TERMS if key != "all kinds, no normal test" else tuple(t for t in MM.TERMS if t not in ("normal", "plane"))
    assert MM.coverage(details, decided) == []


def test_a_position_does_not_depend_on_its_neighbours(h):
    name, cur, surf, st = MM.hand_cases()[-1]                                 # the rows mixed over the lanes
    prm, table = R.axis_params(), MM.hand_table()
    out, motion = moving_dev(h, cur, prm, surf, st, table)
    sel = np.array([0, 7, 63, 64, 130])
    few, few_motion = moving_dev(h, cur[sel], prm, surf, st, table)
    assert_same_bits(few, out[sel])
    assert_same_bits(few_motion, motion[sel])
    perm = np.random.default_rng(1).permutation(len(cur))
    p_out, p_motion = moving_dev(h, cur[perm], prm, surf, st, table)
    assert_same_bits(p_out, out[perm])
    assert_same_bits(p_motion, motion[perm])


def test_on_a_callers_stream_and_without_a_motion_plane(h, detmath_cpu):
    """behind copies that fill the inputs, the table among them, on that stream; the call does not synchronise: the result is right
    only if it ran in stream order"""
    import torch
    name, cur, surf, st = MM.hand_cases()[MM.ROW_SHIFT]
    prm, table = R.axis_params(), MM.hand_table()
    want, _ = MM.reproject_moving(detmath_cpu, cur, prm, surf, st, table)
    src = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (cur, surf, st, table)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_cur, d_ps, d_pt, d_table = [torch.zeros_like(a) for a in src]
        for d, a in zip((d_cur, d_ps, d_pt, d_table), src):
            d.copy_(a)                                                        # kernels on s: the inputs are not there before them
        d_out = torch.full((len(cur), 8), float("nan"), dtype=torch.float64, device="cuda")
        h.reproject_moving_dev(d_cur.data_ptr(), len(cur), prm, d_ps.data_ptr(), d_pt.data_ptr(), d_table.data_ptr(), len(table), d_out.data_ptr(), None,
                               stream=s.cuda_stream)
    s.synchronize()
    assert_same_bits(d_out.cpu().numpy(), want)


# ---- errors ----
def test_refusals_leave_the_output_untouched(h):
    """Every ACN_ERR_ARG of the two calls: the status, acn_last_error naming the argument, and not one word written, on host and device
    buffers; then the handle still works"""
    import torch
    n = 40
    o = h._plain_opts(False, None)
    name, cur, surf, st = MM.hand_cases()[-1]
    cur = np.ascontiguousarray(cur[:n])
    prm, table = R.axis_params(), MM.hand_table()
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    d_out, d_motion = nan(n + 1, 8), nan(n + 1, 2)
    d_cur, d_ps, d_pt, d_table = [torch.from_numpy(a).to("cuda") for a in (cur, surf, st, table)]
    h_out, h_motion = np.full((n + 1, 8), np.nan), np.full((n + 1, 2), np.nan)
    rp = A.Handle.reproject_params()
    torch.cuda.synchronize()

    def refused(calls, word):
        for name, call in calls.items():
            hip.acn_render_positions(None, None, 0, None, None)            # (sets another message)
            assert call() == abi.ACN_ERR_ARG, name
            msg = hip.acn_last_error().decode()
            assert msg and word in msg, (name, msg)
            torch.cuda.synchronize()
            assert np.isnan(h_out).all() and np.isnan(h_motion).all(), name
            assert bool(torch.isnan(d_out).all()) and bool(torch.isnan(d_motion).all()), name

    def calls(handle, opts, count=n, prev=prm, p=rp, dc=d_cur.data_ptr(), dps=d_ps.data_ptr(), dpt=d_pt.data_ptr(), dt=d_table.data_ptr(), nt=len(table),
              do=d_out.data_ptr(), dm=d_motion.data_ptr(), hc=cur.ctypes.data, hps=surf.ctypes.data, hpt=st.ctypes.data, ht=table.ctypes.data,
              ho=h_out.ctypes.data, hm=h_motion.ctypes.data):
        ref = lambda x: None if x is None else C.byref(x)
        return {"host": lambda: hip.acn_reproject_moving(handle, hc, count, ref(prev), hps, hpt, ht, nt, ref(p), ho, hm, C.byref(opts)),
                "dev": lambda: hip.acn_reproject_moving_dev(handle, dc, count, ref(prev), dps, dpt, dt, nt, ref(p), do, dm, C.byref(opts))}

    only = lambda table_, *names: {k: v for k, v in table_.items() if k in names}
    # those of acn_reproject*
    refused(calls(None, o), "handle")
    refused(calls(h.h, o, prev=None), "prev_params")
    for kw, word in (("hc", "cur_surface"), ("hps", "prev_surface"), ("hpt", "prev_stats"), ("ho", "out_stats")):
        refused(only(calls(h.h, o, **{kw: None}), "host"), word)
    for kw, word in (("dc", "cur_surface"), ("dps", "prev_surface"), ("dpt", "prev_stats"), ("do", "out_stats")):
        refused(only(calls(h.h, o, **{kw: None}), "dev"), word)
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
    # those of the table
    refused(only(calls(h.h, o, ht=None), "host"), "motion")
    refused(only(calls(h.h, o, dt=None), "dev"), "motion")
    refused(calls(h.h, o, nt=0), "n_motion")
    refused(only(calls(h.h, o, dt=d_table.data_ptr() + 8), "dev"), "motion table")
    refused(only(calls(h.h, o, ht=table.ctypes.data + 8), "host"), "motion table")
    refused(calls(h.h, o, nt=(1 << 31) + 1), "n_motion")
    # nothing to do is ACN_OK and writes nothing, null buffers and no table included
    for call in (lambda: hip.acn_reproject_moving_dev(h.h, None, 0, C.byref(prm), None, None, None, 0, None, None, None, C.byref(o)),
                 lambda: hip.acn_reproject_moving(h.h, None, 0, C.byref(prm), None, None, None, 0, None, None, None, None)):
        assert call() == abi.ACN_OK
    torch.cuda.synchronize()
    assert np.isnan(h_out).all() and bool(torch.isnan(d_out).all()) and bool(torch.isnan(d_motion).all())
    # and the handle works, with null parameters too
    assert hip.acn_reproject_moving_dev(h.h, d_cur.data_ptr(), n, C.byref(prm), d_ps.data_ptr(), d_pt.data_ptr(), d_table.data_ptr(), len(table), None,
                                        d_out.data_ptr(), d_motion.data_ptr(), C.byref(o)) == abi.ACN_OK
    got, _ = h.reproject_moving(cur, prm, surf, st, table)
    assert_same_bits(d_out.cpu().numpy()[:n], got.raw)
    assert np.isnan(d_out.cpu().numpy()[n]).all()


# ---- two rendered frames: an object and the camera move ----
@pytest.fixture(scope="module")
def rendered(frames):
    """first-hit surface records of both frames, frame B reached by Handle.replace; synthetic previous statistics; the table"""
    pos = A.main_pass_positions(96, 72)
    hd = A.Handle(frames["prev_flat"])
    prev_surf = hd.surface_positions(pos).raw
    hd.replace(frames["cur_flat"])
    cp = frames["cur_params"]
    hd.set_params(camera_position=cp.camera_position[:], camera_view_direction=cp.camera_view_direction[:])
    cur = hd.surface_positions(pos).raw
    table, report = A.motion_from_scenes(frames["prev_flat"], frames["cur_flat"])
    yield dict(hd=hd, cur=cur, prev_surf=prev_surf, prev_st=MM.synthetic_stats(len(pos)), table=table, report=report)
    hd.close()


def test_rendered_frames_against_the_model(frames, rendered, detmath_cpu):
    """the pose scene at 96 x 72; frame B has the ball turned 10 degrees about z through its centre, shifted by ( 0.15, 0, 0 ), and the
    camera orbited by 2 degrees.  Statistics and motion of the device equal the model bit for bit"""
    r = rendered
    assert r["report"] == dict(rest=frames["cur_flat"].c.n_nodes - 1, moved=1, none=0, same_shape=True)
    want, want_motion = MM.reproject_moving(detmath_cpu, r["cur"], frames["prev_params"], r["prev_surf"], r["prev_st"], r["table"])
    got, motion = r["hd"].reproject_moving(r["cur"], frames["prev_params"], r["prev_surf"], r["prev_st"], r["table"])
    assert_same_bits(got.raw, want)
    assert_same_bits(motion, want_motion)
    has = ~T.empty(got.raw)
    assert (got.raw[has, 0] >= 1.0).all() and (got.raw[has, 0] <= 9.0 + 1e-12).all() and (got.raw[~has] == 0).all()


def test_the_moved_ball_takes_its_history_through_the_table(frames, rendered, detmath_cpu):
    """independent of the model's gather: of the ELIGIBLE current positions on the ball more than half take a history under
    acn_reproject_moving, and strictly more than under acn_reproject (test_motion_cpu.py confirms the pose on the oracle's records:
    1.000 against 0.709 of 443 positions)"""
    r = rendered
    ball = MM.ball_node(frames["cur_flat"])
    cur = r["cur"]
    kinds = cur[:, 12].astype(np.int64)
    on_ball = (cur[:, 0] < np.inf) & (cur[:, 7] == ball) & ((kinds & abi.ACN_REPROJECT_DEFAULT_REJECT_KINDS) == 0) & (cur[:, 13] <= 0)
    moving, _ = r["hd"].reproject_moving(cur, frames["prev_params"], r["prev_surf"], r["prev_st"], r["table"])
    at_rest, _ = r["hd"].reproject(cur, frames["prev_params"], r["prev_surf"], r["prev_st"])
    share, share_rest = float((~T.empty(moving.raw))[on_ball].mean()), float((~T.empty(at_rest.raw))[on_ball].mean())
    print(f"{int(on_ball.sum())} ELIGIBLE positions on the ball: {share:.3f} take a history through the table, {share_rest:.3f} with the world at rest")
    assert on_ball.sum() >= 100
    assert share > 0.5 and share > share_rest
    off_ball = (cur[:, 7] != ball) | ~(cur[:, 0] < np.inf)
    assert_same_bits(moving.raw[off_ball], at_rest.raw[off_ball])             # everything else is at rest


# ---- the tool ----
def test_the_turntable_tool_spins_an_object(tmp_path, frames, capsys):
    """--spin with --temporal writes its frames and reports a history on frame 1; without --spin and --temporal the command still
    writes the bytes test_gpu_reproject.py pins"""
    import re
    import scenes_util as S
    from test_gpu_reproject import PLAIN_SHA256
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_turntable as tool
    scene = tmp_path / "pose.npz"
    frames["prev_flat"].save(str(scene))
    capsys.readouterr()
    tool.main([str(scene), str(tmp_path / "spin_%d.pnm"), "--frames", "2", "--orbit-deg", "10", "--spin", str(MM.BALL_ELEM), "--temporal", "--samples", "2",
               "--moved-max-history", "8"])
    said = capsys.readouterr().out
    data = [open(tmp_path / f"spin_{f}.pnm", "rb").read() for f in range(2)]
    assert all(d.startswith(b"P6") for d in data) and len(data[0]) == len(data[1]) and data[0] != data[1]
    took = [float(v) for v in re.findall(r"^frame \d+: ([0-9.]+) of the pixels took a history", said, re.M)]
    assert len(took) == 2 and took[0] == 0.0 and took[1] > 0.0, said
    assert "1 scene changes" in said, said                                    # one handle: frame 1 came by acn_scene_replace
    tool.main([str(scene), str(tmp_path / "turn_%d.pnm"), "--frames", "2", "--orbit-deg", "10", "--spin", str(MM.TORUS_ELEM), "--spin-axis", "1,0,0"])
    turn = [open(tmp_path / f"turn_{f}.pnm", "rb").read() for f in range(2)]
    assert turn[0] != turn[1]
    for bad in (["--spin", "9"], ["--spin", "1", "--spin-axis", "0,0,0"], ["--spin-axis", "0,0,1"], ["--spin", "1", "--moved-max-history", "8"],
                ["--spin", "1", "--temporal", "--samples", "2", "--moved-max-history", "0.5"]):
        with pytest.raises(SystemExit):
            tool.main([str(scene), str(tmp_path / "x_%d.pnm"), "--frames", "2", "--orbit-deg", "10"] + bad)
    plain_scene = tmp_path / "scene.npz"
    S.build("wine_glass_c2")[1].save(str(plain_scene))
    tool.main([str(plain_scene), str(tmp_path / "plain_%d.pnm"), "--frames", "2", "--orbit-deg", "2"])
    plain = [open(tmp_path / f"plain_{f}.pnm", "rb").read() for f in range(2)]
    assert hashlib.sha256(plain[0] + plain[1]).hexdigest() == PLAIN_SHA256
