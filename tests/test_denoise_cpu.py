"""acn_denoise without a GPU: the refusals (all made on the host, before the handle is touched), the constants of the header,
properties of the numpy model of tests/denoise_model.py (which test_gpu_denoise.py compares the device with, bit for bit), and
what the filter buys on an oracle frame."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import actinon_amd as A
import denoise_model as D
import scenes_util as S
import surface_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 23


def opts_struct(**kw):
    o = A.abi.RenderOpts()
    o.struct_size = C.sizeof(A.abi.RenderOpts)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def params_struct(**kw):
    p = A.abi.DenoiseParams()
    p.struct_size = C.sizeof(A.abi.DenoiseParams)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("fn", ["acn_denoise", "acn_denoise_dev"])
def test_null_handle_is_refused(fn):
    lin, rec, out = np.full((4, 3), 0.5), np.zeros((4, 16)), np.full((4, 3), 7.25)
    o, p = opts_struct(), params_struct()
    for opts in (None, C.byref(o)):
        for prm in (None, C.byref(p)):
            st = getattr(A.hip, fn)(None, lin.ctypes.data, rec.ctypes.data, 2, 2, prm, out.ctypes.data, opts)
            assert st == A.abi.ACN_ERR_ARG
            assert b"null" in A.hip.acn_last_error()
    assert (out == 7.25).all() and (lin == 0.5).all()


BAD = {
    "null linear": dict(lin=None),
    "null surface": dict(rec=None),
    "null out": dict(out=None),
    "zero width": dict(w=0),
    "zero height": dict(h=0),
    "too many pixels": dict(w=65536, h=32769),
    "product overflows": dict(w=2 ** 33, h=2 ** 33),
    "iterations": dict(prm=dict(iterations=9)),
    "normal power": dict(prm=dict(normal_power_log2=11)),
    "negative sigma_plane": dict(prm=dict(sigma_plane=-0.1)),
    "nan sigma_plane": dict(prm=dict(sigma_plane=np.nan)),
    "inf sigma_lum": dict(prm=dict(sigma_lum=np.inf)),
    "negative sigma_lum": dict(prm=dict(sigma_lum=-4.0)),
    "struct_size 0": dict(prm=dict(struct_size=0)),
    "struct_size 3": dict(prm=dict(struct_size=3)),
    "unknown flag": dict(prm=dict(flags=4)),
    "sharded": dict(opts=dict(shard_mode=A.abi.ACN_SHARD_SAMPLES, shard_rank=0, shard_world=2)),
}


@pytest.mark.parametrize("fn", ["acn_denoise", "acn_denoise_dev"])
@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_refused_before_the_handle_is_used(fn, case):
    """every check is on the host and comes before the first use of the handle: a block of zeroes stands in for one here"""
    bad = BAD[case]
    handle = C.create_string_buffer(1 << 16)
    lin, rec, out = np.full((4, 3), 0.5), D.blank(4), np.full((4, 3), 7.25)
    ptr = {k: (None if k in bad and bad[k] is None else arr.ctypes.data) for k, arr in (("lin", lin), ("rec", rec), ("out", out))}
    p, o = params_struct(**bad.get("prm", {})), opts_struct(**bad.get("opts", {}))
    st = getattr(A.hip, fn)(C.addressof(handle), ptr["lin"], ptr["rec"], bad.get("w", 2), bad.get("h", 2), C.byref(p), ptr["out"], C.byref(o))
    assert st == A.abi.ACN_ERR_ARG, case
    assert A.hip.acn_last_error()
    assert (out == 7.25).all() and (lin == 0.5).all() and np.array_equal(rec, D.blank(4))
    assert handle.raw == bytes(1 << 16)


def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    defs = dict(re.findall(r"^#define ACN_DENOISE_(\w+)\s+([0-9.]+)u?\s", text, re.M))
    assert set(defs) == {"NO_DEMODULATE", "NORMAL_POWER_SET", "DEFAULT_ITERATIONS", "DEFAULT_NORMAL_POWER_LOG2", "DEFAULT_SIGMA_PLANE",
                         "DEFAULT_SIGMA_LUM", "MAX_ITERATIONS", "MAX_NORMAL_POWER_LOG2"}
    for name, value in defs.items():
        assert float(value) == getattr(A.abi, "ACN_DENOISE_" + name) == getattr(D, name), name
    assert (D.EMITTER, D.STRIDE) == (A.abi.ACN_SURF_EMITTER, A.abi.ACN_SURF_STRIDE)
    assert "#define ACN_DENOISE_PARAMS_INIT { ( uint32_t )sizeof( acn_denoise_params ), 0u, 0u, 0u, 0.0, 0.0 }" in text
    body = text[text.index("typedef struct acn_denoise_params"):text.index("} acn_denoise_params;")]
    members = re.findall(r"^\s+(uint32_t|double)\s+(\w+);", body, re.M)
    assert members == [({C.c_uint32: "uint32_t", C.c_double: "double"}[t], n) for n, t in A.abi.DenoiseParams._fields_]
    assert C.sizeof(A.abi.DenoiseParams) == 32
    p = A.Handle.denoise_params()
    assert (p.struct_size, p.iterations, p.normal_power_log2, p.flags, p.sigma_plane, p.sigma_lum) == (32, 0, 0, 0, 0.0, 0.0)
    p = A.Handle.denoise_params(iterations=2, normal_power_log2=0, demodulate=False, sigma_plane=0.5, sigma_lum=2.0)
    assert (p.iterations, p.normal_power_log2, p.flags, p.sigma_plane, p.sigma_lum) == (2, 0, 3, 0.5, 2.0)


# ---- properties of the model ----
@pytest.fixture(scope="module")
def frame():
    lin, rec = D.synthetic(W, H)
    lin.setflags(write=False); rec.setflags(write=False)
    return lin, rec


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_model_passes_what_it_cannot_filter(detmath_cpu, frame):
    lin, rec = frame
    out = D.denoise(detmath_cpu, lin, rec)
    c = (lin / D.albedo(rec).reshape(H, W, 3)).reshape(-1, 3)
    ok = D.filterable(rec, c).reshape(H, W)
    miss, emit = ~(rec[:, 0] < np.inf).reshape(H, W), (rec[:, 12].astype(int) & D.EMITTER).reshape(H, W) != 0
    assert miss.sum() >= 30 and emit.sum() >= 4 and not ok[H // 2, W // 2] and not ok[H - 1, 0]
    assert np.array_equal(~ok, miss | emit | ~np.isfinite(lin).all(axis=-1))
    assert same_bits(out[~ok], lin[~ok])
    assert np.isfinite(out[ok]).all() and (out[ok] != lin[ok]).any(axis=-1).mean() > 0.9
    # and the filter filters: neighbours on one object differ by less than they did (medians: fireflies apart)
    pair = ok[:, 1:] & ok[:, :-1] & (rec[:, 7].reshape(H, W)[:, 1:] == rec[:, 7].reshape(H, W)[:, :-1])
    step = lambda img: np.median(np.abs(D.lum(img)[:, 1:] - D.lum(img)[:, :-1])[pair])
    assert step(out) < step(lin), (step(out), step(lin))


def test_model_keeps_a_constant_image(detmath_cpu, frame):
    _, rec = frame
    value = np.array([0.3, 0.6, 0.9])
    lin = np.broadcast_to(value, (H, W, 3)).copy()
    rec = rec.copy()
    rec[:, 9:12] = [0.7, 0.2, 1.0]                     # one albedo: the image and the demodulated image are constant
    for demodulate in (True, False):
        out = D.denoise(detmath_cpu, lin, rec, demodulate=demodulate)
        assert np.abs(out / value - 1).max() <= 1e-15, demodulate


def test_model_never_crosses_a_key_boundary(detmath_cpu):
    """two objects, a constant each, same normal and plane, nothing else to stop the filter: both constants survive"""
    rec = D.blank(H * W).reshape(H, W, 16)
    y, x = np.mgrid[0:H, 0:W]
    left = x < W // 2 + (y % 3)
    rec[..., 0] = 5.0
    rec[..., 1], rec[..., 2] = x * 0.1, y * 0.1
    rec[..., 6] = -1.0
    rec[..., 7] = np.where(left, 2, 3)
    rec[..., 9:12] = 1.0
    rec[..., 12] = 2
    lin = np.where(left[..., None], [0.3, 0.6, 0.9], [4.1, 2.2, 1.3])
    for key_slot, other in ((7, (2, 3)), (8, (-1, 6)), (13, (0, 1))):
        r = rec.copy()
        r[..., 7] = 2
        r[..., key_slot] = np.where(left, *other)
        out = D.denoise(detmath_cpu, lin, r.reshape(-1, 16), sigma_lum=1e9)
        assert np.abs(out / lin - 1).max() <= 1e-15, key_slot      # (a weighted mean of equal numbers, roundings apart)
    r = rec.copy()
    r[..., 7] = 2                                          # one object: now the constants mix
    out = D.denoise(detmath_cpu, lin, r.reshape(-1, 16), sigma_lum=1e9)
    assert (np.abs(out / lin - 1) > 1e-3).any(axis=-1).mean() > 0.5


def test_model_takes_strides_larger_than_the_image(detmath_cpu, frame):
    """iterations = 5 at height 23: stride 16 leaves most taps off the image; strides 64 and 128 leave the centre tap alone"""
    lin, rec = frame
    out = {it: D.denoise(detmath_cpu, lin, rec, iterations=it) for it in (4, 5, 6, 8)}
    ok = np.isfinite(lin).all(axis=-1)
    for it in out:
        assert np.isfinite(out[it][ok]).all(), it
    assert not np.array_equal(out[5][ok], out[4][ok])          # stride 16 still has taps on 37 x 23
    # levels 7 and 8 have the centre tap only: ( k22 * c ) / k22 and ( c / a ) * a roundings apart, the frame of level 6
    assert np.abs(out[8][ok] / out[6][ok] - 1).max() <= 1e-15


def test_model_a_nan_pixel_changes_no_other(detmath_cpu, frame):
    lin, rec = frame
    y, x = H // 2, W // 2
    assert np.isnan(lin[y, x, 1]) and rec[y * W + x, 0] < np.inf and not int(rec[y * W + x, 12]) & D.EMITTER
    a = D.denoise(detmath_cpu, lin, rec)
    assert np.isnan(a).sum() == 1 and same_bits(a[y, x], lin[y, x])
    other = lin.copy()
    other[y, x] = [100.0, np.nan, -3.0]                    # whatever else the pixel holds
    b = D.denoise(detmath_cpu, other, rec)
    miss = rec.copy()
    miss[y * W + x] = D.blank(1)[0]                        # the pixel as a miss: never a tap either
    c = D.denoise(detmath_cpu, lin, miss)
    rest = np.ones((H, W), bool)
    rest[y, x] = False
    assert same_bits(a[rest], b[rest]) and same_bits(a[rest], c[rest])
    number = lin.copy()
    number[y, x, 1] = 0.5                                  # (with a number there it is a tap, and its neighbours do change)
    assert not same_bits(a[rest], D.denoise(detmath_cpu, number, rec)[rest])


# ---- what it buys ----
def test_quality_against_the_oracle(oracle, detmath_cpu):
    """wine_glass 160 x 90, p8 / d16, filtered with the model's FOLLOW records, against the oracle's frame at p1024 / d3200:
    at most half the raw frame's MSE of clip( x, 0, 1 )"""
    w, h = 160, 90
    sc = A.Scene.build("wine_glass", image_width=w, image_height=h, path_samples=8, direct_samples=16)
    flat = sc.flatten()
    pos = S.positions(flat)
    raw = oracle.render_positions(flat, pos, linear=True).reshape(h, w, 3)
    rec, _ = M.follow(oracle, flat, M.camera_rays(flat.params, pos))
    sc.set(path_samples=1024, direct_samples=3200)
    ref = oracle.render_positions(sc.flatten(), pos, linear=True).reshape(h, w, 3)
    out = D.denoise(detmath_cpu, raw, rec)
    e_raw, e_out = D.mse(raw, ref), D.mse(out, ref)
    print(f"wine_glass 160x90 p8/d16 vs p1024/d3200: mse raw {e_raw:.4e} filtered {e_out:.4e} ratio {e_out / e_raw:.3f}")
    assert e_out <= 0.5 * e_raw, (e_out, e_raw)
