"""The device-resident frame on the GPU (include/actinon_hip.h: acn_frame_*) against the numpy model tests/frame_model.py, bit for bit.
The bit-level tests render nothing: they upload a synthetic accumulator, plan, write synthetic colours into the colour buffer of
view() and push; accumulator, key, index list, positions, rval, image and download are compared with the model.  The driver tests
render tests/scripts/cycles3.acn and cycles24.acn on both loops of the render driver and hand a recovery file from each to the other."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import actinon_amd as A
import frame_model as FM
from actinon_amd import abi
from actinon_amd._lib import host

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = os.path.join(HERE, "scripts")
RASTERS = [(1, 1), (1, 5), (5, 1), (64, 4), (37, 19), (67, 41)]
_rt = C.CDLL(None)                                                              # the HIP runtime the library brought along
_rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
_rt.hipPointerGetAttributes.argtypes = [C.c_void_p, C.c_void_p]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if A.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests need one")


def d_read(ptr, shape, dtype=np.float64):
    out = np.empty(shape, dtype=dtype)
    if out.nbytes:
        assert ptr and _rt.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def d_write(ptr, arr):
    arr = np.ascontiguousarray(arr)
    if arr.nbytes:
        assert ptr and _rt.hipMemcpy(ptr, arr.ctypes.data, arr.nbytes, 1) == 0


def memory_type(ptr):
    """hipPointerAttribute_t.type of a pointer; 0 when the runtime does not know it"""
    attr = (C.c_int * 64)()
    return attr[0] if _rt.hipPointerGetAttributes(attr, C.c_void_p(ptr)) == 0 else 0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def script_flat(name="cycles3.acn"):
    sc = A.Scene.from_script(os.path.join(SCRIPTS, name), A.Scene.AUTOENV_GPU)
    return sc, sc.flatten()


@pytest.fixture(scope="module")
def handle():
    sc, flat = script_flat()
    h = A.Handle(flat)
    h.scene = sc
    yield h
    h.close()


def handle_with(monkeypatch, **env):
    """a handle whose tunables (read at upload) are the test's"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    h = A.Handle(script_flat()[1])
    for k in env:
        monkeypatch.delenv(k)
    return h


def synthetic_pass(h, w, hh, acc, thr, K, rval, clr_seed=1):
    """upload, plan, synthetic colours, push on the device; the same on the model; everything compared.  -> ( flagged, targets )"""
    n = w * hh
    with h.frame(w, hh) as f:
        assert same_bits(f.download(), np.zeros((n, 6)))                        # the empty lum_image
        f.upload(acc)
        flagged, rv = f.plan(thr, K, rval)
        want_key = FM.key(acc, w, hh)
        idx = FM.select(want_key, thr)
        want_pos, want_rv = FM.positions(idx, K, rval, w)
        v = f.view()
        assert (v.planned, v.width, v.height, v.flagged, v.samples) == (1, w, hh, len(idx), K)
        assert flagged == len(idx) and rv == want_rv == A.lcg00_jump(rval, 2 * K * flagged)
        assert same_bits(d_read(v.d_key, n), want_key)
        assert np.array_equal(d_read(v.d_index, flagged, np.int64), idx)
        assert same_bits(d_read(v.d_positions, (flagged * K, 2)), want_pos)
        clr = np.random.default_rng(clr_seed).uniform(0, 2, (flagged * K, 3))
        d_write(v.d_colours, clr)
        assert same_bits(f.download(), acc)                                     # a plan writes nothing into the accumulator
        f.push()
        assert f.view().planned == 0
        want, target = FM.push(acc, w, hh, want_pos, clr)
        got = f.download()
        assert same_bits(got, want), np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))[:5]
        rgb, rgb8 = f.image()
        want_rgb, want_rgb8 = FM.image(want)
        assert same_bits(rgb, want_rgb) and np.array_equal(rgb8, want_rgb8)
        assert f.image(rgb=False)[0] is None and np.array_equal(f.image(rgb=False)[1], want_rgb8)
        with pytest.raises(A.AcnError, match="push without a plan"):
            f.push()
        return idx, target


@pytest.mark.parametrize("w,hh", RASTERS)
def test_synthetic_passes_are_the_models_bits(handle, w, hh):
    rng = np.random.default_rng(100 * w + hh)
    n = w * hh
    acc = FM.random_frame(rng, w, hh)
    if n >= 5:
        acc[rng.integers(0, n)] = 0.0
    keys = FM.key(acc, w, hh)
    third = float(np.sort(keys)[(2 * n) // 3]) if n > 2 else 0.0
    seen = set()
    for K in (1, 2, 3):
        for thr in (np.inf, -np.inf, third):
            idx, _ = synthetic_pass(handle, w, hh, acc, thr, K, FM.SEED + 7 * K, clr_seed=K)
            seen.add(len(idx))
            assert len(idx) == (0 if thr == np.inf else n if thr == -np.inf else len(idx))
    if n == 1:
        assert seen == {0, 1}                                                   # no neighbour: the key is 0.0, above -inf alone
    if n > 100:
        assert any(n // 5 < s < n // 2 for s in seen), seen                     # about a third


def spot(w, hh, bright, dim=()):
    """weight 1 everywhere, red 1.0 in the `bright` pixels ( x, y ) and 0.6 in the `dim` ones: with a threshold of 0.5 a pixel is
    flagged iff it is bright or touches a bright one and is not dim"""
    acc = np.zeros((w * hh, 6))
    acc[:, 5] = 1.0
    for x, y in bright:
        acc[y * w + x, 2] = 1.0
    for x, y in dim:
        acc[y * w + x, 2] = 0.6
    return acc


# ( name, w, h, accumulator, which draw is 2^64 - 1, the first flagged pixel, where its first entry lands (-1: dropped), that pixel flagged? )
FOREIGN = [
    ("dx, neighbour flagged", 6, 5, spot(6, 5, [(2, 2)]), 1, 1 * 6 + 1, 1 * 6 + 2, True),
    ("dy, neighbour flagged", 6, 5, spot(6, 5, [(2, 2)]), 2, 1 * 6 + 1, 2 * 6 + 1, True),
    ("dx, neighbour not flagged", 6, 5, spot(6, 5, [(0, 0)], [(1, 0)]), 1, 0, 1, False),
    ("dx, last column", 6, 5, spot(6, 5, [(5, 0)], [(4, 0)]), 1, 5, -1, False),
    ("dx, one column", 1, 5, spot(1, 5, [(0, 2)]), 1, 1, -1, False),
    ("dy, last row", 6, 5, spot(6, 5, [(0, 4)], [(0, 3), (1, 3)]), 2, 4 * 6, -1, False),
    ("dy, one row", 5, 1, spot(5, 1, [(2, 0)]), 2, 1, -1, False),
]


@pytest.mark.parametrize("slots", [None, 0])
@pytest.mark.parametrize("case", FOREIGN, ids=[c[0] for c in FOREIGN])
def test_foreign_entries_are_added_before_the_targets_own(handle, monkeypatch, case, slots):
    """slots 0: the list holds nothing, so one lane walks the whole plan"""
    name, w, hh, acc, nth, first, lands, lands_flagged = case
    h = handle if slots is None else handle_with(monkeypatch, ACN_FRAME_FOREIGN_SLOTS=slots)
    try:
        for K in (1, 2):
            idx, target = synthetic_pass(h, w, hh, acc, 0.5, K, FM.seed_for_draw(2 ** 64 - 1, nth))
            assert idx[0] == first and target[0] == lands and (lands in idx) == lands_flagged, (name, idx, target[:4])
            assert (target[1:] >= 0).all() and (np.repeat(idx, K)[1:] == target[1:]).all()    # every other entry is its own pixel's
    finally:
        if h is not handle:
            h.close()


def test_slices_give_the_bits_of_one(handle, monkeypatch):
    w, hh, K = 37, 19, 3
    acc = FM.random_frame(np.random.default_rng(9), w, hh)
    h = handle_with(monkeypatch, ACN_FRAME_SLICE=900)                           # 300 pixels of 3 positions: 703 pixels in three slices
    try:
        idx, _ = synthetic_pass(h, w, hh, acc, -np.inf, K, FM.SEED)
        assert len(idx) == 703
        synthetic_pass(h, w, hh, acc, float(np.median(FM.key(acc, w, hh))), 2, FM.SEED)
        synthetic_pass(h, w, hh, acc, -np.inf, 1, FM.seed_for_draw(2 ** 64 - 1))  # a foreign entry, with slices
        # ... and a rendered pass: the main pass in seven slices, the gradient pass in several
        out = []
        for hx in (h, handle):
            with hx.frame() as f:
                f.main_pass()
                flagged, rv = f.gradient_pass(0.05 ** 2, 3, FM.SEED)
                assert flagged > 0
                out.append((f.download(), rv))
        assert same_bits(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    finally:
        h.close()


def read_pnm_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_whole_driver_on_cycles3(handle, tmp_path):
    sc = handle.scene
    w, hh = int(sc.s.prm.image_width), int(sc.s.prm.image_height)
    cycles, K, thr = int(sc.s.gradient_cycles), int(sc.s.gradient_samples), sc.s.gradient_threshold * sc.s.gradient_threshold
    assert (w, hh, cycles, K) == (96, 64, 3, 3)
    with handle.frame() as f:
        f.main_pass()
        centres = FM.centres(w, hh)
        acc, _ = FM.push(np.zeros((w * hh, 6)), w, hh, centres, handle.render_positions(centres))
        assert same_bits(f.download(), acc)
        rval = want_rval = FM.SEED
        counts = []
        for c in range(cycles):
            flagged, rval = f.gradient_pass(thr, K, rval)
            acc, want_rval, want_flagged = FM.gradient_pass(acc, w, hh, thr, K, want_rval, handle.render_positions)
            assert (flagged, rval) == (want_flagged, want_rval)
            assert same_bits(f.download(), acc), c                              # every word
            counts.append(flagged)
        assert any(0 < c < w * hh for c in counts), counts
        frame_rgb8 = f.image(rgb=False)[1]
    files = {}
    for host_cycles in (False, True):
        script = tmp_path / ("host" if host_cycles else "frame") / "cycles3.acn"
        script.parent.mkdir()
        script.write_text(open(os.path.join(SCRIPTS, "cycles3.acn")).read())
        A.run_script(script, host_cycles=host_cycles)
        files[host_cycles] = read_pnm_bytes(str(script) + ".pnm")
    assert files[False] == files[True]
    assert files[False] == b"P6\n96 64\n255\n" + frame_rgb8.tobytes()
    assert C.c_int.in_dll(host, "acn_scene_s_host_cycles_g").value == 0         # the default, and run_script put it back


def write_recovery(path, w, hh, cycle, rval, acc):
    """the layout of acn_driver.c's recovery_save"""
    with open(path, "wb") as f:
        f.write(struct.pack("<8sQQQQ", b"ACNLUM1", w, hh, cycle, rval))
        f.write(np.ascontiguousarray(acc, dtype=np.float64).tobytes())


@pytest.mark.parametrize("first", ["frame", "host"])
def test_recovery_file_of_one_path_resumes_under_the_other(tmp_path, capfd, first):
    """Three cycles on one implementation, its accumulator in the driver's recovery layout, cycles 4 - 6 on the other: the bytes of an
    uninterrupted run.  `host` drives the loop on host arrays through the model and render_positions."""
    text = open(os.path.join(SCRIPTS, "cycles24.acn")).read()
    assert "scene.gradient_cycles    = 24;" in text
    script = tmp_path / "cycles6.acn"
    script.write_text(text.replace("scene.gradient_cycles    = 24;", "scene.gradient_cycles    = 6;"))
    full, part = str(tmp_path / "full.pnm"), str(tmp_path / "part.pnm")
    A.run_script(script, args=("actinon_hip", str(script), full), host_cycles=first == "host")

    def three_cycles(scene, file):
        w, hh = int(scene.s.prm.image_width), int(scene.s.prm.image_height)
        K, thr = int(scene.s.gradient_samples), scene.s.gradient_threshold * scene.s.gradient_threshold
        assert int(scene.s.gradient_cycles) == 6
        h = A.Handle(scene.flatten())
        try:
            rval = FM.SEED
            if first == "frame":
                with h.frame() as f:
                    f.main_pass()
                    for _ in range(3):
                        _, rval = f.gradient_pass(thr, K, rval)
                    acc = f.download()
            else:
                centres = FM.centres(w, hh)
                acc, _ = FM.push(np.zeros((w * hh, 6)), w, hh, centres, h.render_positions(centres))
                for _ in range(3):
                    acc, rval, _ = FM.gradient_pass(acc, w, hh, thr, K, rval, h.render_positions)
        finally:
            h.close()
        write_recovery(file + ".tmp.lum_image", w, hh, 4, rval, acc)

    A.run_script(script, on_create_image=three_cycles, args=("actinon_hip", str(script), part))
    assert os.path.exists(part + ".tmp.lum_image") and not os.path.exists(part)
    recover = C.c_int.in_dll(host, "acn_scene_s_automatic_recover_g")
    recover.value = 1
    try:
        capfd.readouterr()
        A.run_script(script, args=("actinon_hip", str(script), part), host_cycles=first == "frame")
        out = capfd.readouterr().out
    finally:
        recover.value = 0
    assert "resuming at gradient cycle 4" in out and "main image" not in out and "gradient pass   6" in out, out
    assert "gradient pass   3" not in out
    assert read_pnm_bytes(part) == read_pnm_bytes(full)


def test_cancel_leaves_the_accumulator(handle):
    with handle.frame() as f:
        f.main_pass()
        before = f.download()
        handle.cancel = C.c_int(1)
        try:
            with pytest.raises(A.AcnError) as e:
                f.gradient_pass(0.05 ** 2, 3, FM.SEED)
            assert e.value.status == abi.ACN_ERR_CANCELLED
            with pytest.raises(A.AcnError) as e:
                f.main_pass()
            assert e.value.status == abi.ACN_ERR_CANCELLED
        finally:
            handle.cancel = None
        assert same_bits(f.download(), before) and f.view().planned == 0        # the pass dropped its plan
        flagged, _ = f.gradient_pass(0.05 ** 2, 3, FM.SEED)
        assert flagged > 0 and not same_bits(f.download(), before)


def test_plan_push_and_image_leave_the_render_statistics(handle):
    pos = FM.centres(96, 64)[:500]
    handle.count_work = True
    try:
        handle.render_positions(pos)
    finally:
        handle.count_work = False
    counters, stages = handle.last_counters_raw(10), handle.last_stages()
    assert counters[0] > 0
    acc = FM.random_frame(np.random.default_rng(3), 37, 19)
    synthetic_pass(handle, 37, 19, acc, -np.inf, 2, FM.SEED)
    assert handle.last_counters_raw(10) == counters and handle.last_stages() == stages
    with handle.frame(37, 19) as f:                                             # plan on plan, render of another raster: refused, nothing changes
        f.upload(acc)
        f.plan(0.0, 1, 5)
        with pytest.raises(A.AcnError, match="consumed"):
            f.plan(0.0, 1, 5)
        with pytest.raises(A.AcnError, match="the frame is 37 x 19, the raster of the resident scene 96 x 64"):
            f.render()
        for bad, word in ((dict(samples=0), "samples"), (dict(sqr_threshold=float("nan")), "NaN")):
            with pytest.raises(A.AcnError, match=word):
                f.plan(**{**dict(sqr_threshold=0.0, samples=1, rval=5), **bad})
        f.upload(acc)                                                           # drops the plan
        assert f.view().planned == 0 and same_bits(f.download(), acc)
    assert handle.last_counters_raw(10) == counters


def test_lifetime_and_raster_changes():
    sc, flat = script_flat()
    h = A.Handle(flat)
    f = h.frame()
    f.main_pass()
    before = f.download()
    h.set_params(image_width=48)
    for call in (f.main_pass, lambda: f.gradient_pass(0.0025, 3, FM.SEED), lambda: (f.plan(0.0025, 3, FM.SEED), f.render())):
        with pytest.raises(A.AcnError, match="the frame is 96 x 64, the raster of the resident scene 48 x 64") as e:
            call()
        assert e.value.status == abi.ACN_ERR_ARG
    h.set_params(image_width=96)
    f.upload(before)                                                            # (drops the plan the last call left)
    assert f.gradient_pass(0.0025, 3, FM.SEED)[0] > 0
    # a frame the caller never frees goes with its handle: its accumulator is no device allocation any more
    d_acc = f.view().d_accumulator
    assert memory_type(d_acc) == 2                                              # hipMemoryTypeDevice
    h.close()
    assert memory_type(d_acc) == 0                                              # hipMemoryTypeUnregistered (or no pointer the runtime knows)
    f.close()                                                                   # the handle took it along: nothing left to free
    h = A.Handle(flat)
    try:
        with pytest.raises(A.AcnError, match="2\\^31"):
            h.frame(2 ** 31, 1)
        with pytest.raises(A.AcnError, match="width"):
            h.frame(0, 4)
        g = h.frame(5, 3)
        g.close()
        g.close()
    finally:
        h.close()
