"""Replacing the scene of a live handle (acn_scene_replace, acn_scene_set_params, acn_scene_info): a handle whose scene or parameters
were changed renders the bits of a fresh handle of that scene, keeps its streams and lanes, learns again exactly when the kind of
the scene changed (or it is told to forget), refuses what an upload refuses without changing, and accumulates nothing on the device.
ACN_LANES=3 and wine_glass 320 x 180 p64 d50: the smallest shape at which three lanes run (tests/test_queueplan_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import scenes_util as S
from actinon_amd import abi
from actinon_amd._lib import host
from actinon_amd.cameras import orbit_camera

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "actinon_amd", "bin", "actinon_hip")
WINE = dict(image_width=320, image_height=180, path_samples=64, direct_samples=50)
LENS = dict(samples=3, aperture=0.15, focus=12.0)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(autouse=True)
def three_lanes(monkeypatch):
    monkeypatch.setenv("ACN_LANES", "3")                            # (tunables are read at the upload)


def wine(**kw):
    return A.Scene.build("wine_glass", **dict(WINE, **kw)).flatten()


def frame(h, flat=None):
    p = h.params if flat is None else flat.params
    return h.render_positions(A.main_pass_positions(p.image_width, p.image_height), linear=True)


def everything(h, flat):
    """the frame, the followed surface records and the lens statistics of 37 positions"""
    few = S.positions(flat)[::max(1, len(S.positions(flat)) // 37)][:37]
    rgb, stats = h.render_lens_stats(few, linear=True, **LENS)
    return frame(h, flat), h.surface_positions(few, follow=True).raw, rgb, stats.raw


def fresh(flat, what=frame):
    h = A.Handle(flat)
    try:
        return what(h, flat)
    finally:
        h.close()


_REF = {}


def wine_reference():
    """the frame of a fresh handle of the unmoved wine glass: computed once, shared, never changed"""
    if "wine" not in _REF:
        _REF["wine"] = fresh(wine())
        _REF["wine"].setflags(write=False)
    return _REF["wine"]


def test_a_replaced_handle_renders_the_fresh_handles_bits():
    """One handle through wine_glass (three lanes), diamond (prune programs, class0_min 32, the own run), many_spheres (the
    simple-compound and sphere tables appear and grow), the textured scene and wine_glass again: after each step the frame, the
    surface records and the lens statistics are those of a fresh handle of that scene."""
    steps = [wine(), S.build("diamond_c4")[1], S.build("many_spheres_c3")[1], S.build("textured")[1], wine()]
    h, first = None, None
    try:
        for i, flat in enumerate(steps):
            if h is None:
                h = A.Handle(flat)
            else:
                h.replace(flat)
            got = everything(h, flat)
            assert h.info()["nodes"] == flat.n_nodes
            want = fresh(flat, everything)
            for name, g, w in zip(("frame", "surface", "lens rgb", "lens stats"), got, want):
                assert np.array_equal(g, w), f"step {i}: {name} differs from a fresh handle's"
            if i == 0:
                first = got[0]
                assert h.last_stages()["finalize_launches"] == 3    # (the last render call of a step is the frame: on three lanes)
        assert np.array_equal(got[0], first) and np.array_equal(first, wine_reference())
        assert h.info()["replaces"] == len(steps) - 1
    finally:
        h.close()


def animation(change):
    """five frames on one handle, change( h, f ) between them -> the handle, the infos after each frame, the workspace allocations"""
    h = A.Handle(wine())
    infos, allocs = [], []
    for f in range(5):
        flat = wine(**orbit_camera(wine().params, 9.0 * f)) if f else wine()
        if f:
            change(h, f, flat)
        got = frame(h, flat)
        st = h.last_stages()
        assert st["finalize_launches"] == 3, st                     # three lanes ran
        assert np.array_equal(got, fresh(flat) if f else wine_reference()), f"frame {f + 1}"
        infos.append(h.info())
        allocs.append(st["workspace_allocs"])
    return h, infos, allocs


@pytest.mark.parametrize("how", ["set_params", "replace"])
def test_animation_stays_warm(how):
    """Five frames of an orbiting camera, by set_params or by replace with re-flattened scenes of the same kind: each has a fresh
    handle's bits, and the handle made no stream, no lane and no learning pass after its first frame; its queues are allocated for
    the first frame and trimmed once, by the second call."""
    def change(h, f, flat):
        if how == "replace":
            h.replace(flat)
        else:
            h.set_params(**orbit_camera(wine().params, 9.0 * f))
    h, infos, allocs = animation(change)
    try:
        print(how, infos, allocs)
        for key in ("streams", "lanes", "learning_passes"):
            assert infos[0][key] == infos[4][key], (key, infos)
        assert infos[0]["learning_passes"] == 1 and infos[0]["lanes"] == 3 and infos[0]["streams"] == 4
        assert all(i["rates_known"] == 1 for i in infos)
        assert infos[4]["replaces" if how == "replace" else "param_sets"] == 4
        assert allocs[3] == allocs[2] and allocs[4] == allocs[2], allocs
    finally:
        h.close()


def test_another_kind_learns_again_on_the_same_lanes():
    """path_samples 64 -> 16 changes the kind: the next frame runs a second learning pass, on the streams and lanes that exist, and has a
    fresh handle's bits.  A replace with a scene of that kind forgets nothing; with forget=True the handle learns a third time."""
    h = A.Handle(wine())
    try:
        frame(h)
        before = h.info()
        assert before["learning_passes"] == 1
        h.set_params(path_samples=16)
        assert h.info()["rates_known"] == 0
        p16 = wine(path_samples=16)
        assert np.array_equal(frame(h), fresh(p16))
        after = h.info()
        assert after["learning_passes"] == 2 and after["streams"] == before["streams"] and after["lanes"] == before["lanes"]
        h.replace(p16)                                              # the same kind: nothing is forgotten
        assert h.info()["rates_known"] == 1
        frame(h)
        assert h.info()["learning_passes"] == 2
        h.replace(p16, forget=True)
        assert h.info()["rates_known"] == 0
        assert np.array_equal(frame(h), fresh(p16))
        last = h.info()
        assert last["learning_passes"] == 3 and last["streams"] == before["streams"] and last["lanes"] == before["lanes"]
    finally:
        h.close()


def refused_scenes():
    unsupported = A.Scene.build("wine_glass", **dict(WINE, experimental_level=1)).flatten()
    sc = A.Scene()                                                  # a light without fov function: a radiant ellipsoid
    el = host.acn_obj_squaroid_s_create_ellipsoid(1, 1, 1)
    host.acn_obj_set_radiance(el, 5.0)
    sc.push(el)
    host.acn_obj_discard(el)
    no_fov = sc.flatten()
    bad_child = wine()
    bad_child.c.elems[bad_child.c.nodes[bad_child.c.matter_root].child0] = bad_child.c.n_nodes
    return [(unsupported, abi.ACN_ERR_UNSUPPORTED), (no_fov, abi.ACN_ERR_NO_FOV), (bad_child, abi.ACN_ERR_ARG)]


def test_a_refused_replace_changes_nothing():
    """experimental_level 1, a light without fov and an element index out of range each raise with the status an upload gives; so does
    set_params( image_height=1 ).  After each the handle renders the old scene's bits and its counters have not moved."""
    small = dict(image_width=64, image_height=36, path_samples=16)
    flat = wine(**small)
    want = fresh(flat)
    h = A.Handle(flat)
    try:
        assert np.array_equal(frame(h), want)
        for scene, status in refused_scenes():
            with pytest.raises(A.AcnError) as e:
                h.replace(scene)
            assert e.value.status == status
            assert h.flat is flat and np.array_equal(frame(h), want)
            assert h.info()["replaces"] == 0 and h.info()["nodes"] == flat.n_nodes
        with pytest.raises(A.AcnError) as e:
            h.set_params(image_height=1)
        assert e.value.status == abi.ACN_ERR_ARG
        assert h.params.image_height == 36 and np.array_equal(frame(h), want)
        assert h.info()["param_sets"] == 0
    finally:
        h.close()


def test_raster_follows_the_params():
    """After set_params( image_width=48, image_height=20 ) the main pass takes 960 pixels and refuses 961, and the frame and the camera
    rays are those of a fresh handle with that raster."""
    import torch
    flat = wine(image_width=64, image_height=36, path_samples=16)
    h = A.Handle(flat)
    try:
        h.set_params(image_width=48, image_height=20)
        small = wine(image_width=48, image_height=20, path_samples=16)
        out = torch.empty((961, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        h.render_main_pass_dev(0, 960, out.data_ptr(), linear=True)
        assert np.array_equal(out[:960].cpu().numpy(), fresh(small))
        with pytest.raises(A.AcnError) as e:
            h.render_main_pass_dev(0, 961, out.data_ptr(), linear=True)
        assert e.value.status == abi.ACN_ERR_ARG
        pos = S.positions(small)
        assert np.array_equal(h.camera_rays(pos), fresh(small, lambda f, _: f.camera_rays(pos)))
    finally:
        h.close()


def test_nothing_accumulates():
    """Eight replaces alternating wine_glass and diamond, a frame after each.  The free device memory after rounds 2 - 4 (a round: both
    scenes) is not below the value after round 1 by more than W / 4, W the queue workspace of the first call: round 1 pays for code
    objects and whatever the runtime keeps; a scene or a workspace that is not released costs at least W per round
    (tests/test_gpu_handle_lifecycle.py).  close() gives the device back what the handle holds."""
    import torch
    glass, diamond = wine(), S.build("diamond_c4")[1]
    h = A.Handle(glass)
    try:
        frame(h)
        w = h.last_stages()["workspace_bytes"]
        free = []
        for rnd in range(4):
            for flat in (diamond, glass):                           # every round ends as the handle began: on the wine glass, on three lanes
                h.replace(flat)
                frame(h)
            torch.cuda.empty_cache()
            free.append(torch.cuda.mem_get_info(0)[0])
        held = h.last_stages()["workspace_bytes"]
        assert h.info()["replaces"] == 8
    finally:
        h.close()
    torch.cuda.empty_cache()
    closed = torch.cuda.mem_get_info(0)[0]
    drops = [free[0] - f for f in free[1:]]
    print(f"W = {w:.0f} bytes; free after each round {free}; drops against round 1 {drops}; held {held:.0f}; free after close {closed}")
    assert w > 0 and held > 0
    assert max(drops) <= w / 4, (drops, w)
    assert closed - free[-1] >= held / 2, (closed, free[-1], held)


def test_driver_keeps_one_handle_over_two_images(tmp_path):
    """tests/scripts/two_images.acn -- two different scenes, two gradient cycles each -- through create_image_file( keep=... ) on one
    kept handle, and through the built command line tool in a child process, writes the bytes the plain create_image_file writes."""
    script = os.path.join(ROOT, "tests", "scripts", "two_images.acn")

    def names(tag):
        return [str(tmp_path / f"{tag}_{k}.pnm") for k in (1, 2)]

    plain, kept, cli = names("plain"), names("kept"), names("cli")
    A.run_script(script, args=("actinon", script, *plain))
    with A.KeptHandle() as keep:
        A.run_script(script, on_create_image=lambda sc, file: sc.create_image_file(file, keep=keep), args=("actinon", script, *kept))
        info = keep.info()
    assert info["replaces"] == 1 and info["streams"] >= 1, info
    r = subprocess.run([CLI, script, *cli, "-f"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = [open(p, "rb").read() for p in plain]
    assert len(want[0]) > 64 * 48 * 3 and len(want[1]) > 80 * 40 * 3 and want[0] != want[1]
    for tag, files in (("kept handle", kept), ("command line tool", cli)):
        for p, w in zip(files, want):
            assert open(p, "rb").read() == w, f"{tag}: {os.path.basename(p)}"
