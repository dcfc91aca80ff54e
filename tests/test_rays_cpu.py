"""Caller-supplied primary rays without a GPU: the four entry points of include/actinon_hip.h refuse a null handle, and
actinon_amd.cameras.panorama_rays builds the equirectangular rays tools/render_panorama.py renders."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import actinon_amd as A
from actinon_amd import abi
from actinon_amd._lib import hip
from actinon_amd.cameras import panorama_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ray_entry_points_refuse_a_null_handle():
    rays, pos, out = np.zeros((1, 6)), np.zeros((1, 2)), np.zeros((1, 6))
    o = abi.RenderOpts()
    o.struct_size = C.sizeof(abi.RenderOpts)
    assert hip.acn_render_rays(None, rays.ctypes.data, 1, out.ctypes.data, C.byref(o)) == abi.ACN_ERR_ARG
    assert hip.acn_render_rays_dev(None, rays.ctypes.data, 1, out.ctypes.data, C.byref(o)) == abi.ACN_ERR_ARG
    assert hip.acn_camera_rays(None, pos.ctypes.data, 1, out.ctypes.data) == abi.ACN_ERR_ARG
    assert hip.acn_camera_rays_dev(None, pos.ctypes.data, 1, out.ctypes.data, C.byref(o)) == abi.ACN_ERR_ARG
    assert b"null" in hip.acn_last_error()


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(v @ v)


def test_panorama_rays_layout_and_directions():
    origin, view, top = (1.0, -2.0, 0.5), (0.3, 2.0, -0.4), (0.1, 0.0, 1.0)
    w, h = 33, 17                                    # odd: a centre column and an equator row exist
    r = panorama_rays(origin, view, top, w, h)
    assert r.shape == (h * w, 6) and r.dtype == np.float64
    assert (r[:, :3] == np.asarray(origin)).all()
    d = r[:, 3:]
    assert np.abs((d * d).sum(axis=1) - 1.0).max() <= 1e-15
    fwd = unit(view)
    t = np.asarray(top) - (np.asarray(top) @ fwd) * fwd
    up = unit(t)
    right = np.cross(fwd, up)
    grid = d.reshape(h, w, 3)                        # row-major: row j, column i is ray j * w + i
    assert np.allclose(grid[h // 2, w // 2], fwd, rtol=0, atol=1e-15)
    lat = np.arcsin(np.clip(grid @ up, -1, 1))
    lon = np.arctan2(grid @ right, grid @ fwd)
    assert np.allclose(lat, ((0.5 - (np.arange(h) + 0.5) / h) * np.pi)[:, None], rtol=0, atol=1e-12)
    assert np.allclose(lon[h // 2], ((np.arange(w) + 0.5) / w - 0.5) * 2 * np.pi, rtol=0, atol=1e-12)
    # the top row lies within one pixel's angle of top; longitude grows to the right, latitude falls downwards
    assert (np.arccos(np.clip(grid[0] @ up, -1, 1)) <= np.pi / h).all()
    assert (np.diff(lon[h // 2]) > 0).all() and (np.diff(lat[:, 0]) < 0).all()
    with pytest.raises(ValueError):
        panorama_rays(origin, view, view, w, h)


def test_panorama_tool_reads_the_scene_of_a_script():
    """tools/render_panorama.py: an .acn script gives the scene of its first create_image (nothing rendered)."""
    spec = importlib.util.spec_from_file_location("render_panorama", os.path.join(ROOT, "tools", "render_panorama.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    script = os.path.join(ROOT, "tests", "scripts", "csg.acn")
    got = tool.load_scene(script)
    want = A.Scene.from_script(script, A.Scene.AUTOENV_SKIP).flatten()
    assert got.nodes_bytes() == want.nodes_bytes()
    assert C.string_at(C.addressof(got.c.params), C.sizeof(abi.Params)) == C.string_at(C.addressof(want.c.params), C.sizeof(abi.Params))
