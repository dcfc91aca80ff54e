"""The thin-lens camera without a GPU: tests/lens_model.py is the contract of include/actinon_hip.h restated in numpy, and these
tests pin what that contract promises -- the rays of a position meet in the plane in focus, the lens samples lie in the aperture
disc, jitter stays inside the pixel, samples differ by k and by seed, a closed aperture without jitter is the pinhole, and the
32-round fallback of the disc sample is reached by construction only.  The entry points refuse a null handle."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import actinon_amd as A
import lens_model as M
import scenes_util as S
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def flat():
    return S.build("primitives_c1")[1]


@pytest.fixture(scope="module")
def prm(flat):
    return flat.params


@pytest.fixture(scope="module")
def pos(flat):
    p = S.positions(flat)
    return p[:: len(p) // 23][:24].copy()                           # 24 pixel centres over the raster


def line_distance(point, rays):
    """distance of `point` [...,3] from the lines of rays [...,6]"""
    o, d = rays[..., :3], rays[..., 3:]
    w = point - o
    along = (w * d).sum(axis=-1, keepdims=True)
    return np.sqrt(((w - d * along) ** 2).sum(axis=-1))


def test_the_rays_of_a_position_meet_in_the_plane_in_focus(detmath_cpu, oracle, prm, pos):
    cam = M.Camera(detmath_cpu, prm)
    for focus, aperture, jitter in ((7.5, 0.2, False), (2.0, 0.05, False), (40.0, 1.5, False), (7.5, 0.2, True)):
        det = {}
        rays = M.lens_rays(detmath_cpu, oracle, prm, pos, samples=8, aperture=aperture, focus=focus, jitter=jitter, detail=det)
        assert rays.shape == (len(pos), 8, 6)
        # each ray passes through the point F its pinhole ray has in the plane at view depth `focus`
        assert line_distance(det["F"], rays).max() <= 1e-12 * focus
        depth = ((det["F"] - cam.position) * cam.V).sum(axis=-1)
        assert np.abs(depth - focus).max() <= 1e-12 * focus
        assert np.abs((rays[..., 3:] ** 2).sum(axis=-1) - 1.0).max() <= 1e-12
        if not jitter:      # one position, one pinhole ray, one F: all K rays of a position meet there
            assert (det["F"] == det["F"][:, :1]).all()
            assert line_distance(det["F"][:, :1], rays).max() <= 1e-12 * focus


def test_lens_samples_lie_in_the_aperture_disc(detmath_cpu, oracle, prm, pos):
    cam = M.Camera(detmath_cpu, prm)
    aperture = 0.3
    det = {}
    rays = M.lens_rays(detmath_cpu, oracle, prm, pos, samples=64, aperture=aperture, focus=5.0, detail=det)
    u, v = det["uv"][..., 0], det["uv"][..., 1]
    assert (u * u + v * v <= 1.0).all()
    off = rays[..., :3] - cam.position
    assert np.sqrt((off ** 2).sum(axis=-1)).max() <= aperture * (1 + 1e-12)
    assert np.abs((off * cam.V).sum(axis=-1)).max() <= 1e-12          # the lens lies in the plane through the camera position
    assert np.abs((off * cam.R).sum(axis=-1) - aperture * u).max() <= 1e-12
    assert np.abs((off * cam.T).sum(axis=-1) - aperture * v).max() <= 1e-12
    # a uniform disc: both signs of both coordinates, and radii beyond 0.9
    assert (u > 0).any() and (u < 0).any() and (v > 0).any() and (v < 0).any() and (u * u + v * v > 0.81).any()
    assert 0.45 < (u * u + v * v <= 0.5).mean() < 0.55                    # half of the area lies within radius sqrt( 1/2 )


def test_jitter_stays_inside_the_pixel(detmath_cpu, oracle, prm, pos):
    det = {}
    M.lens_rays(detmath_cpu, oracle, prm, pos, samples=64, jitter=True, detail=det)
    j = det["q"] - pos[:, None, :]
    assert np.abs(j).max() <= 0.5
    assert j.min() < -0.4 and j.max() > 0.4 and abs(j.mean()) < 0.05
    # without jitter nothing moves
    M.lens_rays(detmath_cpu, oracle, prm, pos, samples=4, detail=det)
    assert (det["q"] == pos[:, None, :]).all()


def test_samples_differ_by_k_and_by_seed(detmath_cpu, oracle, prm, pos):
    kw = dict(samples=16, aperture=0.2, focus=6.0, jitter=True)
    a = M.lens_rays(detmath_cpu, oracle, prm, pos, seed=0, **kw)
    b = M.lens_rays(detmath_cpu, oracle, prm, pos, seed=1, **kw)
    for i in range(len(pos)):
        assert len({r.tobytes() for r in a[i]}) == 16                      # the 16 samples of a position are 16 rays
    assert not (a == b).all(axis=-1).any()
    assert (a == M.lens_rays(detmath_cpu, oracle, prm, pos, seed=0, **kw)).all()    # and the generator is a function
    # a window of samples is that slice of the whole set
    w = M.lens_rays(detmath_cpu, oracle, prm, pos, seed=0, first_sample=5, n_samples=3, **kw)
    assert np.array_equal(w, a[:, 5:8])
    # positions differ too
    assert len({r.tobytes() for r in a[:, 0]}) == len(pos)


def test_closed_aperture_without_jitter_is_the_pinhole(detmath_cpu, oracle, prm, pos, monkeypatch):
    cam = M.Camera(detmath_cpu, prm)
    o, d = cam.rays(pos[:, 0], pos[:, 1])
    want = np.concatenate([o, d], axis=-1)

    def no_draw(rv):
        raise AssertionError("a pinhole ray draws nothing")
    monkeypatch.setattr(M, "rnd0", no_draw)
    monkeypatch.setattr(M, "rnd1", no_draw)
    got = M.lens_rays(detmath_cpu, oracle, prm, pos, samples=3, aperture=0.0, focus=0.0)
    assert got.shape == (len(pos), 3, 6)
    for k in range(3):
        assert np.array_equal(got[:, k], want)
    # the camera model itself: unit directions, the view direction in the raster's centre, x to the right and y downwards
    assert np.abs((d * d).sum(axis=-1) - 1.0).max() <= 1e-15
    _, c = cam.rays(np.array([float(cam.width >> 1)]), np.array([float(cam.height >> 1)]))
    assert np.abs(c[0] - cam.V).max() <= 1e-15
    _, e = cam.rays(np.array([float(cam.width >> 1) + 10]), np.array([float(cam.height >> 1) + 10]))
    assert (e[0] * cam.R).sum() > 0 and (e[0] * cam.T).sum() < 0


def test_the_fallback_of_the_disc_sample_is_reached_by_construction_only(detmath_cpu, oracle, prm, pos, monkeypatch):
    det = {}
    M.lens_rays(detmath_cpu, oracle, prm, pos, samples=256, aperture=0.2, focus=6.0, jitter=True, detail=det)
    assert det["taken"].all() and 1 <= det["rounds"].min() and det["rounds"].max() < M.ROUNDS // 2
    assert (det["rounds"] > 1).any()                                      # the rejection loop does reject
    # a draw that never lands in the disc: 32 rounds, then the centre of the lens
    calls = []

    def corner(rv):
        calls.append(1)
        return M.lcg(rv), np.ones(rv.shape)
    monkeypatch.setattr(M, "rnd0", corner)
    rays = M.lens_rays(detmath_cpu, oracle, prm, pos, samples=2, aperture=0.2, focus=6.0, detail=det)
    assert len(calls) == 2 * M.ROUNDS
    assert not det["taken"].any() and (det["rounds"] == M.ROUNDS).all() and (det["uv"] == 0).all()
    cam = M.Camera(detmath_cpu, prm)
    assert (rays[..., :3] == cam.position).all()
    assert np.abs(rays[..., 3:] - det["pinhole"][..., 3:]).max() <= 1e-15   # through F from the lens centre: the pinhole ray again


def test_ordered_mean():
    L = np.array([[[-0.0, 1.0, 1e16], [-0.0, 2.0, 1.0], [-0.0, 4.0, -1e16]]])
    m = M.ordered_mean(L)
    assert np.array_equal(m, [[0.0, 7.0 / 3.0, 0.0]]) and not np.signbit(m[0, 0])     # 0.0 + -0.0 is +0.0; the order is k's
    assert np.array_equal(M.ordered_mean(L[:, :1]), 0.0 + L[:, 0])


def test_lens_entry_points_refuse_a_null_handle_and_the_params_mirror_the_header():
    pos, out = np.zeros((1, 2)), np.zeros((1, 16 * 6))
    o = abi.RenderOpts()
    o.struct_size = C.sizeof(abi.RenderOpts)
    p = A.Handle.lens_params()
    assert (p.struct_size, p.samples, p.flags, p.seed, p.aperture_radius, p.focus_distance) == (32, 0, 0, 0, 0.0, 0.0)
    q = A.Handle.lens_params(samples=5, aperture=0.25, focus=3.0, jitter=True, seed=9)
    assert (q.samples, q.flags, q.seed, q.aperture_radius, q.focus_distance) == (5, abi.ACN_LENS_JITTER, 9, 0.25, 3.0)
    assert hip.acn_lens_rays(None, pos.ctypes.data, 1, C.byref(p), 0, 1, out.ctypes.data) == abi.ACN_ERR_ARG
    assert hip.acn_lens_rays_dev(None, pos.ctypes.data, 1, C.byref(p), 0, 1, out.ctypes.data, C.byref(o)) == abi.ACN_ERR_ARG
    assert hip.acn_render_lens(None, pos.ctypes.data, 1, C.byref(p), out.ctypes.data, C.byref(o)) == abi.ACN_ERR_ARG
    assert hip.acn_render_lens_dev(None, pos.ctypes.data, 1, C.byref(p), out.ctypes.data, C.byref(o)) == abi.ACN_ERR_ARG
    assert hip.acn_render_lens_main_pass_dev(None, 0, 1, C.byref(p), out.ctypes.data, C.byref(o)) == abi.ACN_ERR_ARG
    assert b"null" in hip.acn_last_error()
    # the constants of the header
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for name, value in (("ACN_LENS_JITTER", "1u"), ("ACN_LENS_DEFAULT_SAMPLES", "16"), ("ACN_LENS_MAX_SAMPLES", "4096"),
                        ("ACN_LENS_SEED", "2718281828ull")):
        assert f"#define {name} " in text and text.split(f"#define {name} ")[1].split()[0] == value, name
    assert (abi.ACN_LENS_JITTER, abi.ACN_LENS_DEFAULT_SAMPLES, abi.ACN_LENS_MAX_SAMPLES, abi.ACN_LENS_SEED) == (
        M.JITTER, M.DEFAULT_SAMPLES, M.MAX_SAMPLES, M.SEED) == (1, 16, 4096, 2718281828)


def test_dof_tool_focus_depth_and_arguments():
    """tools/render_dof.py: the view depth of a picked point, and the scene of a script (nothing rendered)."""
    spec = importlib.util.spec_from_file_location("render_dof", os.path.join(ROOT, "tools", "render_dof.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    script = os.path.join(ROOT, "tests", "scripts", "csg.acn")
    got = tool.load_scene(script)
    want = A.Scene.from_script(script, A.Scene.AUTOENV_SKIP).flatten()
    assert got.nodes_bytes() == want.nodes_bytes()
    prm = got.params
    p = np.array(prm.camera_position[:])
    view = np.array(prm.camera_view_direction[:])
    view = view / np.sqrt(view @ view)
    side = np.cross(view, [0.3, 0.2, 0.9])
    assert abs(tool.focus_depth(prm, p + 4.5 * view + 2.0 * side) - 4.5) <= 1e-12
    a = tool.parse_args(["s.acn", "o.pnm", "--aperture", "0.1", "--focus-at", "12.5,7"])
    assert a.focus is None and a.focus_at == (12.5, 7.0) and a.samples is None and not a.jitter
    with pytest.raises(SystemExit):
        tool.parse_args(["s.acn", "o.pnm", "--aperture", "0.1"])                      # neither --focus nor --focus-at
    with pytest.raises(SystemExit):
        tool.parse_args(["s.acn", "o.pnm", "--aperture", "0.1", "--focus", "3", "--focus-at", "1,2"])
