"""acn_denoise on the GPU against the numpy model of tests/denoise_model.py, bit for bit (the header states every expression
and its order; test_denoise_cpu.py checks the model's properties), the call's contract (streams, in place, the renderer left
alone), what the filter buys against converged frames rendered on the device, and tools/render_denoised.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import actinon_amd as A
import denoise_model as D
import scenes_util as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 23
PARAMS = {"defaults": dict(), "other": dict(iterations=2, normal_power_log2=3, demodulate=False)}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def h():
    """the filter does not consult the scene: any handle serves"""
    handle = A.Handle(S.build("wine_glass_c2")[1])
    yield handle
    handle.close()


@pytest.fixture(scope="module")
def glass():
    """wine_glass 96 x 54 at p8 / d16: the device's linear frame and its FIRST_HIT and FOLLOW records"""
    sc = A.Scene.build("wine_glass", image_width=96, image_height=54, path_samples=8, direct_samples=16)
    flat = sc.flatten()
    pos = S.positions(flat)
    hd = A.Handle(flat)
    lin = hd.render_positions(pos, linear=True).reshape(54, 96, 3)
    rec = {follow: hd.surface_positions(pos, follow=follow).raw for follow in (False, True)}
    hd.close()
    for a in (lin, rec[False], rec[True]):
        a.setflags(write=False)
    return lin, rec


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same_bits(got, want):
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:5], [got[tuple(i)] for i in bad[:5]], [want[tuple(i)] for i in bad[:5]])


@pytest.mark.parametrize("params", list(PARAMS))
@pytest.mark.parametrize("shape", [(W, H), (1, 64), (64, 1), (5, 5)])
def test_synthetic_frames_have_the_models_bits(h, detmath_cpu, shape, params):
    lin, rec = D.synthetic(*shape)
    got = h.denoise(lin, rec, **PARAMS[params])
    assert got.shape == (shape[1], shape[0], 3)
    assert_same_bits(got, D.denoise(detmath_cpu, lin, rec, **PARAMS[params]))
    passed = ~np.isfinite(lin).all(axis=-1) | ~(rec[:, 0] < np.inf).reshape(lin.shape[:2])
    assert passed.any() and same_bits(got[passed], lin[passed])


def test_normal_power_zero_is_expressible(h, detmath_cpu):
    """k = 0 needs ACN_DENOISE_NORMAL_POWER_SET; without the flag a 0 is the default 7"""
    lin, rec = D.synthetic(W, H)
    want = {k: D.denoise(detmath_cpu, lin, rec, normal_power_log2=k) for k in (0, 7)}
    assert not same_bits(want[0], want[7])
    assert_same_bits(h.denoise(lin, rec, normal_power_log2=0), want[0])
    out = np.empty_like(lin)
    p = A.abi.DenoiseParams()
    p.struct_size = C.sizeof(A.abi.DenoiseParams)
    for prm in (None, C.byref(p)):
        A.check(A.hip.acn_denoise(h.h, lin.ctypes.data, rec.ctypes.data, W, H, prm, out.ctypes.data, None), "acn_denoise")
        assert_same_bits(out, want[7])
    p.struct_size = 8                                  # a caller that knows the first two members only
    p.iterations, p.normal_power_log2, p.flags = 3, 9, 1
    A.check(A.hip.acn_denoise(h.h, lin.ctypes.data, rec.ctypes.data, W, H, C.byref(p), out.ctypes.data, None), "acn_denoise")
    assert_same_bits(out, D.denoise(detmath_cpu, lin, rec, iterations=3))


@pytest.mark.parametrize("params", list(PARAMS))
@pytest.mark.parametrize("follow", [False, True])
def test_wine_glass_has_the_models_bits(h, detmath_cpu, glass, follow, params):
    lin, rec = glass
    got = h.denoise(lin, rec[follow], **PARAMS[params])
    assert_same_bits(got, D.denoise(detmath_cpu, lin, rec[follow], **PARAMS[params]))
    assert (got != lin).any(axis=-1).mean() > 0.5


def test_results_do_not_depend_on_wave_neighbours(h):
    """the frame inside a larger one whose other pixels are misses: other tiles, other waves, the same bits"""
    lin, rec = D.synthetic(W, H)
    plain = h.denoise(lin, rec)
    for (bw, bh, x0, y0) in ((W + 30, H + 19, 19, 9), (W + 1, H + 1, 1, 0), (W + 64, H, 64, 0)):
        big_lin = np.full((bh, bw, 3), 0.125)
        big_rec = D.blank(bh * bw).reshape(bh, bw, 16)
        big_lin[y0:y0 + H, x0:x0 + W] = lin
        big_rec[y0:y0 + H, x0:x0 + W] = rec.reshape(H, W, 16)
        got = h.denoise(big_lin, big_rec.reshape(-1, 16))
        assert_same_bits(np.ascontiguousarray(got[y0:y0 + H, x0:x0 + W]), plain)
        outside = np.ones((bh, bw), bool)
        outside[y0:y0 + H, x0:x0 + W] = False
        assert (got[outside] == 0.125).all()


def test_device_buffers_streams_and_in_place(h, glass):
    import torch
    lin, rec = glass
    hh, w = lin.shape[:2]
    n = w * hh
    for params in PARAMS.values():
        host = h.denoise(lin, rec[True], **params)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_lin = torch.from_numpy(lin.reshape(n, 3).copy()).to("cuda")
            d_rec = torch.from_numpy(rec[True].copy()).to("cuda")
            d_out = torch.full((n + 1, 3), float("nan"), dtype=torch.float64, device="cuda")
            h.denoise_dev(d_lin.data_ptr(), d_rec.data_ptr(), w, hh, d_out.data_ptr(), stream=s.cuda_stream, **params)
            d_same = d_lin.clone()
            h.denoise_dev(d_same.data_ptr(), d_rec.data_ptr(), w, hh, d_same.data_ptr(), stream=s.cuda_stream, **params)
        s.synchronize()
        out = d_out.cpu().numpy()
        assert_same_bits(out[:n].reshape(hh, w, 3), host)
        assert np.isnan(out[n]).all()                                  # nothing behind the frame
        assert_same_bits(d_same.cpu().numpy().reshape(hh, w, 3), host)
        assert same_bits(d_lin.cpu().numpy().reshape(hh, w, 3), lin)   # out of place: the input stays
        d_sync = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        h.denoise_dev(d_lin.data_ptr(), d_rec.data_ptr(), w, hh, d_sync.data_ptr(), **params)   # the handle's stream: the call waits
        assert_same_bits(d_sync.cpu().numpy().reshape(hh, w, 3), host)
    # refusals with a real handle write nothing either; an unaligned record buffer is one of them
    d_out.fill_(7.25)
    torch.cuda.synchronize()
    with pytest.raises(A.AcnError) as e:
        h.denoise_dev(d_lin.data_ptr(), d_rec.data_ptr() + 8, w, hh - 1, d_out.data_ptr())
    assert e.value.status == A.abi.ACN_ERR_ARG and "align" in str(e.value)
    with pytest.raises(A.AcnError) as e:
        h.denoise_dev(d_lin.data_ptr(), d_rec.data_ptr(), w, hh, d_out.data_ptr(), iterations=9)
    assert e.value.status == A.abi.ACN_ERR_ARG
    torch.cuda.synchronize()
    assert (d_out == 7.25).all()


def test_a_denoise_call_leaves_the_renderer_alone(glass):
    lin, rec = glass
    sc, flat = S.build("wine_glass_c2")
    pos = S.positions(flat)
    hd = A.Handle(flat)
    before = hd.render_positions(pos, linear=True)
    st0 = hd.last_stages()
    first = hd.denoise(lin, rec[True])
    big = hd.denoise(np.tile(lin, (3, 2, 1)), np.tile(rec[True].reshape(54, 96, 16), (3, 2, 1)).reshape(-1, 16))   # the scratch grows
    again = hd.denoise(lin, rec[True])
    after = hd.render_positions(pos, linear=True)
    st1 = hd.last_stages()
    hd.close()
    assert big.shape == (162, 192, 3) and same_bits(first, again)
    assert np.array_equal(before, after)
    assert st1["retries"] == 0
    assert st1["workspace_bytes"] == st0["workspace_bytes"] and st1["workspace_allocs"] == st0["workspace_allocs"], (st0, st1)


QUALITY = {
    # scene -> builder, width, height, the reference's sampling
    "wine_glass": ("wine_glass", 160, 90, (4096, 12800)),
    "many_spheres": ("many_spheres:3:1", 128, 72, (512, 1600)),
}


@pytest.mark.parametrize("name", list(QUALITY))
def test_quality_against_a_converged_frame(name):
    """the filtered p8 / d16 frame has at most half the MSE of the raw p8 / d16 frame and at most the MSE of the raw p64 / d200
    frame, eight times its samples; MSE of clip( x, 0, 1 ) against a reference rendered on the device"""
    builder, w, hh, ref_samples = QUALITY[name]
    sc = A.Scene.build(builder, image_width=w, image_height=hh)
    frames = {}
    for p, d in ((8, 16), (64, 200), ref_samples):
        sc.set(path_samples=p, direct_samples=d)
        flat = sc.flatten()
        pos = S.positions(flat)
        hd = A.Handle(flat)
        frames[p] = hd.render_positions(pos, linear=True).reshape(hh, w, 3)
        if p == 8:
            rec = hd.surface_positions(pos, follow=True)
            frames["filtered"] = hd.denoise(frames[8], rec)
        hd.close()
    ref = frames[ref_samples[0]]
    e8, e64, ef = D.mse(frames[8], ref), D.mse(frames[64], ref), D.mse(frames["filtered"], ref)
    print(f"{name} {w}x{hh}: mse raw p8/d16 {e8:.4e}  raw p64/d200 {e64:.4e}  filtered p8/d16 {ef:.4e}  ({ef / e8:.3f} of raw, {ef / e64:.3f} of p64)")
    assert ef <= 0.5 * e8, (ef, e8)
    assert ef <= e64, (ef, e64)


def test_the_tool_writes_the_resolved_filtered_frame(tmp_path, monkeypatch):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from render_aovs import read_pnm
    from render_panorama import load_scene
    script = os.path.join(ROOT, "tests", "scripts", "textured.acn")
    out, raw = tmp_path / "out.pnm", tmp_path / "raw.pnm"
    args = ["--path-samples", "4", "--direct-samples", "8", "--width", "80", "--height", "50"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_denoised.py"), script, str(out), "--raw", str(raw)] + args,
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    monkeypatch.chdir(tmp_path)
    flat = load_scene(script)
    prm = flat.params
    prm.path_samples, prm.direct_samples, prm.image_width, prm.image_height = 4, 8, 80, 50
    pos = A.main_pass_positions(80, 50)
    hd = A.Handle(flat)
    lin = hd.render_positions(pos, linear=True).reshape(50, 80, 3)
    filtered = hd.denoise(lin, hd.surface_positions(pos, follow=True))
    d_rgb8 = torch.empty((2, 4000, 3), dtype=torch.uint8, device="cuda")
    for k, frame in enumerate((filtered, lin)):
        d = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1, 3)).to("cuda")
        hd.resolve_dev(d.data_ptr(), 4000, None, d_rgb8[k].data_ptr())
    hd.close()
    want = d_rgb8.cpu().numpy().reshape(2, 50, 80, 3)
    assert np.array_equal(read_pnm(out), want[0])
    assert np.array_equal(read_pnm(raw), want[1])
    assert (want[0] != want[1]).any(axis=-1).mean() > 0.2
