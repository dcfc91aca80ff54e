"""Caller-supplied primary rays on the GPU (acn_render_rays / acn_camera_rays, include/actinon_hip.h): against the pipeline's
own camera rays and against the CPU oracle.

The oracle has no ray entry.  Any ray (p, u) with | |u|^2 - 1 | < 1e-8 is the central ray of a pinhole at p looking along u
with focal length 1, at the position ( W >> 1, H >> 1 ) of any raster with H >= 2: there x = z = 0, ( 0, 1, 0 ) passes
v3d_s_of_length unchanged, and the rotation maps it onto u exactly (each component is +-0 + u_i + +-0; u has no zero
component).  That is how arbitrary rays are checked here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import actinon_amd as A
import scenes_util as S
from actinon_amd.cameras import panorama_rays

pytestmark = pytest.mark.gpu
TOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACN_F_CAMERA_RAY = 35   # actinon_amd/csrc/acn_costs.h


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


def matter_side(oracle, flat, p):
    """-1 if p lies inside some element of the matter root (oracle OBJ_SIDE), else 1"""
    return min(oracle.obj_side(flat, e, p) for e in flat.elems_of(flat.c.matter_root))


@pytest.mark.parametrize("name", list(S.SMALL))
def test_camera_rays_render_as_the_pipelines_own(name):
    """render_rays( camera_rays( pos ) ) is render_positions( pos ) bit for bit: on host buffers, and through the device
    entry points on a torch stream of the caller's."""
    import torch
    sc, flat = S.build(name)
    pos = S.positions(flat)
    n = len(pos)
    h = A.Handle(flat)
    rays = h.camera_rays(pos)
    for linear in (True, False):
        assert np.array_equal(h.render_rays(rays, linear=linear), h.render_positions(pos, linear=linear)), linear
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_pos = torch.from_numpy(pos).to("cuda")
        d_rays = torch.full((n, 6), float("nan"), dtype=torch.float64, device="cuda")
        d_ray_out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        d_pos_out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        h.camera_rays_dev(d_pos.data_ptr(), n, d_rays.data_ptr(), stream=s.cuda_stream)
        for linear in (True, False):
            h.render_rays_dev(d_rays.data_ptr(), n, d_ray_out.data_ptr(), linear=linear, stream=s.cuda_stream)
            h.render_positions_dev(d_pos.data_ptr(), n, d_pos_out.data_ptr(), linear=linear, stream=s.cuda_stream)
            assert torch.equal(d_ray_out, d_pos_out), linear
    s.synchronize()
    assert np.array_equal(d_rays.cpu().numpy(), rays)
    h.close()


# cameras other than the scene's own: (position, look-at point, top, focal length, width, height).  Per scene one looks up
# from below the objects and one sits inside an object (checked with the oracle's OBJ_SIDE)
FOREIGN = {
    "wine_glass_c2": [((4.0, -6.0, 3.0), (0.0, 0.0, 0.8), (0, 0, 1), 3.0, 40, 24),
                      ((0.3, -3.0, -0.8), (0.0, 0.0, 1.5), (0, 1, 0), 2.0, 40, 24),             # below the bowl, looking up
                      ((0.05, -0.1, 0.45), (1.0, 2.0, 0.2), (0, 0, 1), 1.5, 32, 20),             # inside the wine
                      ((-3.0, 2.0, 6.0), (0.0, 0.0, 0.0), (1, 1, 0.3), 1.0, 36, 36)],
    "diamond_c4": [((0.2, 0.3, 0.05), (0.0, 0.0, -0.04), (0, 0, 1), 4.0, 40, 24),
                   ((0.05, -0.15, -0.074), (0.0, 0.0, -0.02), (0, 1, 0), 2.0, 40, 24),         # on the floor, looking up
                   ((0.002, -0.001, -0.022), (0.3, 1.0, 0.1), (0, 0, 1), 1.0, 32, 20),        # inside the stone
                   ((0.0, 0.0, 0.3), (0.0, 0.0, -0.05), (0, 1, 0), 3.0, 30, 30)],
    "textured": [((5.0, -5.0, 3.0), (0.0, 0.0, 0.0), (0, 0, 1), 3.0, 40, 24),
                 ((0.5, -3.0, -0.9), (0.0, 0.0, 1.0), (0, 1, 0), 1.5, 40, 24),                   # above the floor, looking up
                 ((-1.2, 0.1, 0.1), (1.0, 0.5, -0.3), (0, 0, 1), 1.0, 32, 20),                 # inside the chess ball
                 ((-4.0, 4.0, 1.0), (0.6, 0.5, -0.2), (0.2, 0, 1), 2.5, 36, 30)],
}


@pytest.mark.parametrize("name", sorted(FOREIGN))
def test_foreign_cameras_in_one_shuffled_call(oracle, name):
    """The rays of four other cameras, each taken from that camera's own handle over its raster, concatenated and shuffled,
    rendered in ONE call on the handle of the scene's own camera: every ray comes out as its camera renders it, bit for bit,
    and as the oracle renders it with that camera."""
    sc, flat = S.build(name)
    own = A.Handle(flat)
    rays, cams = [], []
    inside = 0
    for p, tgt, top, focal, w, hh in FOREIGN[name]:
        sc.set(camera_position=p, camera_view_direction=np.subtract(tgt, p), camera_top_direction=top,
               camera_focal_length=focal, image_width=w, image_height=hh)
        cam = sc.flatten()
        inside += matter_side(oracle, cam, p) == -1
        pos = S.positions(cam)
        hc = A.Handle(cam)
        rays.append(hc.camera_rays(pos))
        cams.append((cam, pos, hc.render_positions(pos)))
        hc.close()
    assert inside >= 1
    looks_up = [np.subtract(tgt, p)[2] > 0 and p[2] < tgt[2] for p, tgt, *_ in FOREIGN[name]]
    assert any(looks_up)
    all_rays = np.concatenate(rays)
    perm = np.random.default_rng(11).permutation(len(all_rays))
    got = np.empty((len(all_rays), 3))
    got[perm] = own.render_rays(all_rays[perm])
    own.close()
    k = 0
    for cam, pos, ref in cams:
        g = got[k:k + len(pos)]
        k += len(pos)
        assert np.array_equal(g, ref)
        cpu = oracle.render_positions(cam, pos)
        assert np.abs(g - cpu).max() <= TOL
        assert np.array_equal(A.cps_from_cl(g), A.cps_from_cl(cpu))


# scene -> centre and half size of the box the origins are drawn from, origins inside objects
ARBITRARY = {"wine_glass_c2": ((0.0, 0.0, 1.0), 3.0, [(0.05, -0.1, 0.45), (0.0, 0.0, -1.5)]),
             "diamond_c4": ((0.0, 0.0, -0.03), 0.08, [(0.002, -0.001, -0.022), (0.0, 0.0, -0.09)]),
             "primitives_path": ((0.0, 0.0, 0.2), 2.5, [(2.0, 0.1, 0.0), (0.0, 0.0, -1.5)])}


def pinhole_of_ray(flat, p, u):
    """Sets flat's camera to the pinhole whose central ray is (p, u) (module docstring); returns that sample position."""
    prm = flat.c.params
    prm.image_width, prm.image_height, prm.camera_focal_length = 3, 2, 1.0
    top = np.zeros(3)
    top[np.argmin(np.abs(u))] = 1.0                    # the axis least parallel to u
    for k in range(3):
        prm.camera_position[k], prm.camera_view_direction[k], prm.camera_top_direction[k] = p[k], u[k], top[k]
    return np.array([[3 >> 1, 2 >> 1]], dtype=np.float64)


@pytest.mark.parametrize("name", sorted(ARBITRARY))
def test_arbitrary_rays_against_the_oracle(oracle, name):
    centre, half, inside_pts = ARBITRARY[name]
    sc, flat = S.build(name)
    rng = np.random.default_rng(5)
    n = 128
    org = np.asarray(centre) + rng.uniform(-half, half, (n, 3))
    org[:len(inside_pts)] = inside_pts
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    assert (d != 0).all() and (np.abs((d * d).sum(axis=1) - 1) < 1e-8).all()
    h = A.Handle(flat)
    gpu = h.render_rays(np.concatenate([org, d], axis=1), linear=True)
    h.close()
    bg = np.array(flat.params.background_color[:])
    sides = [matter_side(oracle, flat, o) for o in org]
    cpu = np.empty_like(gpu)
    for i in range(n):
        cpu[i] = oracle.render_positions(flat, pinhole_of_ray(flat, org[i], d[i]), linear=True, threads=1)[0]
    assert sides.count(-1) >= 2, sides
    assert (np.abs(cpu - bg).max(axis=1) == 0).sum() >= 8      # rays that miss everything return the background
    err = np.abs(gpu - cpu).max(axis=1)
    assert err.max() <= TOL, (np.flatnonzero(err > TOL), err.max())


def test_bench_frame_as_rays_cold_and_between_position_calls(monkeypatch):
    """The bench frame (wine_glass 1920x1080 p64 d200): a cold handle's first call is render_rays_dev of the frame's camera
    rays and equals render_main_pass_dev bit for bit, on the default lanes and on one; position and ray calls alternate on
    the handle without a redone chunk."""
    import torch
    sc = A.Scene.build("wine_glass", image_width=1920, image_height=1080, path_samples=64, direct_samples=200)
    flat = sc.flatten()
    n = 1920 * 1080
    stream = torch.cuda.current_stream().cuda_stream
    d_pos = torch.from_numpy(S.positions(flat)).to("cuda")
    d_rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    frame = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    out = torch.empty_like(frame)
    for lanes in (None, "1"):
        if lanes:
            monkeypatch.setenv("ACN_LANES", lanes)
        else:
            monkeypatch.delenv("ACN_LANES", raising=False)
        h = A.Handle(flat)
        h.camera_rays_dev(d_pos.data_ptr(), n, d_rays.data_ptr(), stream=stream)
        h.render_rays_dev(d_rays.data_ptr(), n, out.data_ptr(), linear=True, stream=stream)    # the first render call
        assert h.last_stages()["retries"] == 0, lanes
        h.render_main_pass_dev(0, n, frame.data_ptr(), linear=True, stream=stream)
        assert h.last_stages()["retries"] == 0, lanes
        assert torch.equal(out, frame), lanes
        for call in ("positions", "rays", "positions"):
            out.fill_(-1.0)
            if call == "rays":
                h.render_rays_dev(d_rays.data_ptr(), n, out.data_ptr(), linear=True, stream=stream)
            else:
                h.render_positions_dev(d_pos.data_ptr(), n, out.data_ptr(), linear=True, stream=stream)
            assert h.last_stages()["retries"] == 0, (lanes, call)
            assert torch.equal(out, frame), (lanes, call)
        h.close()
    monkeypatch.delenv("ACN_LANES", raising=False)


def test_work_counters_of_a_ray_call():
    """The same rays, the same work -- less the camera rays the call did not compute."""
    sc, flat = S.build("wine_glass_c2")
    pos = S.positions(flat)
    h = A.Handle(flat, count_work=True)
    rays = h.camera_rays(pos)
    h.render_positions(pos)
    cp = h.last_counters()
    h.render_rays(rays)
    cr = h.last_counters()
    h.close()
    for k in ("trans_rays", "shadow_rays", "obj_hits", "lum_calls", "cap_samples", "side_calls", "sdf_evals", "transcendentals"):
        assert cr[k] == cp[k], (k, cr[k], cp[k])
    assert cp["flop"] - cr["flop"] == len(pos) * ACN_F_CAMERA_RAY, (cp["flop"], cr["flop"])


def test_sample_shards_of_a_ray_call():
    sc, flat = S.build("wine_glass_c2")
    pos = S.positions(flat)
    h = A.Handle(flat)
    rays = h.camera_rays(pos)
    full = h.render_rays(rays, linear=True)
    for world in (2, 3):
        total = np.zeros_like(full)
        for rank in range(world):
            h.sample_shard = (rank, world)
            part = h.render_rays(rays, linear=True)
            assert np.array_equal(part, h.render_positions(pos, linear=True)), (rank, world)
            total += part
        h.sample_shard = None
        assert np.abs(total - full).max() <= 1e-10, (world, np.abs(total - full).max())
    h.close()


def test_contract_of_a_ray_call(monkeypatch):
    """n = 0; refused rays (the first one named, the output untouched); the normalisation rule; the cancel flag."""
    import torch
    sc, flat = S.build("wine_glass_c2")
    pos = S.positions(flat)[::7]
    h = A.Handle(flat)
    rays = h.camera_rays(pos)
    n = len(rays)
    stream = torch.cuda.current_stream().cuda_stream
    assert h.render_rays(np.zeros((0, 6))).shape == (0, 3)
    sentinel = torch.full((n, 3), 7.25, dtype=torch.float64, device="cuda")
    h.render_rays_dev(0, 0, sentinel.data_ptr(), stream=stream)
    d_bad = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    for i, j, v in ((37, 3, np.nan), (5, 0, np.inf), (n - 2, 5, -np.inf), (12, None, 0.0), (20, 1, np.nan)):
        bad = rays.copy()
        if j is None:
            bad[i, 3:] = 0.0
        else:
            bad[i, j] = v
        bad[n - 1, 4] = np.nan                           # a second refused ray: the first one is named
        with pytest.raises(A.AcnError) as e:
            h.render_rays(bad)
        assert e.value.status == A.abi.ACN_ERR_ARG and f"ray {i}:" in str(e.value), str(e.value)
        d_bad.copy_(torch.from_numpy(bad))
        with pytest.raises(A.AcnError) as e:
            h.render_rays_dev(d_bad.data_ptr(), n, sentinel.data_ptr(), stream=stream)
        assert e.value.status == A.abi.ACN_ERR_ARG and f"ray {i}:" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert (sentinel == 7.25).all()
    # directions of any length are scaled by 1 / sqrt( x*x + y*y + z*z ) (v3d_s_of_length)
    long = rays.copy()
    long[:, 3:] *= 2.5
    x, y, z = long[:, 3], long[:, 4], long[:, 5]
    unit = long.copy()
    unit[:, 3:] = long[:, 3:] * (1 / np.sqrt(x * x + y * y + z * z))[:, None]
    assert np.array_equal(h.render_rays(long, linear=True), h.render_rays(unit, linear=True))
    # a cancel flag set before the call: on one lane, and on the concurrent lanes of a larger call
    h.cancel = C.c_int(1)
    with pytest.raises(A.AcnError) as e:
        h.render_rays(rays)
    assert e.value.status == A.abi.ACN_ERR_CANCELLED
    h.close()
    monkeypatch.setenv("ACN_LANES", "4")
    h = A.Handle(flat)
    many = np.tile(h.camera_rays(S.positions(flat)), (8, 1))
    h.cancel = C.c_int(1)
    with pytest.raises(A.AcnError) as e:
        h.render_rays(many)
    assert e.value.status == A.abi.ACN_ERR_CANCELLED
    h.cancel = None
    assert np.isfinite(h.render_rays(many[:1000])).all()
    h.close()
    monkeypatch.delenv("ACN_LANES", raising=False)


def test_render_panorama_tool(tmp_path):
    """tools/render_panorama.py in a child process: a P6 image of the requested size whose pixels are cps_from_cl of
    render_rays( panorama_rays( ... ) )."""
    sc, flat = S.build("wine_glass_c2")
    path = str(tmp_path / "scene.npz")
    flat.save(path)
    out = tmp_path / "pano.pnm"
    w, hh, origin = 64, 32, (0.5, -3.0, 1.5)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_panorama.py"), path, str(out), "--width", str(w),
                        "--height", str(hh), "--origin", ",".join(str(v) for v in origin)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    data = out.read_bytes()
    head = b"P6\n%d %d\n255\n" % (w, hh)
    assert data.startswith(head) and len(data) == len(head) + w * hh * 3
    prm = flat.params
    h = A.Handle(A.Flat.load(path))
    rgb = h.render_rays(panorama_rays(origin, prm.camera_view_direction[:], prm.camera_top_direction[:], w, hh))
    h.close()
    assert data[len(head):] == A.cps_from_cl(rgb).tobytes()
