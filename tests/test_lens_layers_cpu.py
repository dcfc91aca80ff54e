"""The layered lens records and their filter (acn_lens_layers_reduce*, acn_render_lens_layers*, acn_denoise_layers*;
include/actinon_hip.h) without a GPU: the numpy model of tests/lens_layers_model.py on hand-made inputs whose answers are known,
the inputs of the device tests (they must contain what they are there for), the model of the filter against the model of
acn_denoise_stats, and the host-side checks of csrc/acn_layers_host.h in a stand-alone program built with the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import denoise_model as D
import lens_layers_model as Y
import lens_surface_model as R
import stats_model as T
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acn_lens_layers_reduce_dev", "acn_lens_layers_reduce", "acn_render_lens_layers_dev", "acn_render_lens_layers_main_pass_dev",
         "acn_render_lens_layers", "acn_denoise_layers_dev", "acn_denoise_layers")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_and_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\s*\(", text, re.M), name
        assert name in A._lib.HIP_SYMBOLS and getattr(hip, name).argtypes, name
    assert "#define ACN_ABI_VERSION 2\n" in text and abi.ACN_ABI_VERSION == 2
    defs = dict(re.findall(r"^#define ACN_LAYERS_(\w+)_PLANES\s+([0-9]+)\s", text, re.M))
    assert defs == {"SURFACE": "2", "STATS": "3"}
    assert (abi.ACN_LAYERS_SURFACE_PLANES, abi.ACN_LAYERS_STATS_PLANES) == (Y.SURF_PLANES, Y.STATS_PLANES) == (2, 3)
    for method in ("render_lens_layers", "lens_layers_reduce", "denoise_layers"):
        assert callable(getattr(A.Handle, method))


def test_entry_points_refuse_a_null_handle():
    rec, rad, pos = np.zeros((4, 2, 16)), np.zeros((4, 2, 3)), np.zeros((4, 2))
    surf, st, rgb = np.full((2, 4, 16), 7.25), np.full((3, 4, 8), 7.25), np.full((4, 3), 7.25)
    p = A.Handle.lens_params(samples=2)
    dp = A.Handle.denoise_params()
    calls = {
        "acn_lens_layers_reduce": lambda: hip.acn_lens_layers_reduce(None, rec.ctypes.data, rad.ctypes.data, 4, 2, surf.ctypes.data, st.ctypes.data, None),
        "acn_lens_layers_reduce_dev": lambda: hip.acn_lens_layers_reduce_dev(None, rec.ctypes.data, rad.ctypes.data, 4, 2, surf.ctypes.data, st.ctypes.data, None),
        "acn_render_lens_layers": lambda: hip.acn_render_lens_layers(None, pos.ctypes.data, 4, p, 0, rgb.ctypes.data, surf.ctypes.data, st.ctypes.data, None),
        "acn_render_lens_layers_dev": lambda: hip.acn_render_lens_layers_dev(None, pos.ctypes.data, 4, p, 0, rgb.ctypes.data, surf.ctypes.data, st.ctypes.data, None),
        "acn_render_lens_layers_main_pass_dev": lambda: hip.acn_render_lens_layers_main_pass_dev(None, 0, 4, p, 0, rgb.ctypes.data, surf.ctypes.data, st.ctypes.data, None),
        "acn_denoise_layers": lambda: hip.acn_denoise_layers(None, st.ctypes.data, surf.ctypes.data, 2, 2, C.byref(dp), rgb.ctypes.data, None),
        "acn_denoise_layers_dev": lambda: hip.acn_denoise_layers_dev(None, st.ctypes.data, surf.ctypes.data, 2, 2, C.byref(dp), rgb.ctypes.data, None),
    }
    assert set(calls) == set(NAMES)
    for name, call in calls.items():
        hip.acn_scene_upload(None, 0, None)                                  # (sets another message, or none)
        assert call() == abi.ACN_ERR_ARG, name
        assert b"null" in hip.acn_last_error(), (name, hip.acn_last_error())
    assert (surf == 7.25).all() and (st == 7.25).all() and (rgb == 7.25).all()


def radiances(rec, seed=1):
    return np.random.default_rng(seed).uniform(0.0, 2.0, rec.shape[:2] + (3,))


def check_split(lib, rec, L, surf, st):
    """what every split satisfies, whatever the input"""
    n, K = rec.shape[:2]
    assert surf.shape == (2, n, 16) and st.shape == (3, n, 8)
    assert (st[:, :, 0].sum(axis=0) == K).all()                               # m0 + m1 + mr = K
    assert (bits(surf[0]) == bits(R.reduce(lib, rec))).all()                  # plane 0 is acn_surface_reduce, all 16 doubles
    assert (surf[0][:, 15] == st[0][:, 0] / K).all() and (surf[1][:, 15] == st[1][:, 0] / K).all()
    assert (st[0][:, 0] >= st[1][:, 0]).all() and (st[0][:, 0] >= 1).all()
    absent = st[1][:, 0] == 0
    blank = R.miss_record(0, 0.0)
    assert (bits(surf[1][absent]) == bits(blank)).all() and (st[1][absent] == 0).all() and (st[2][absent] == 0).all()
    assert (st[:, :, 7] == 0).all()
    pure = st[0][:, 0] == K
    if pure.any():                                                            # one class: the record of acn_render_lens_stats
        with np.errstate(all="ignore"):
            assert Y.same_bits(st[0][pure], T.records(L[pure])).size == 0


@pytest.mark.parametrize("name", list(Y.hand_made()))
def test_the_split_on_hand_made_inputs(detmath_cpu, name):
    rec, want = Y.hand_made()[name]
    L = radiances(rec)
    surf, st = Y.split(detmath_cpu, rec, L)
    check_split(detmath_cpu, rec, L, surf, st)
    K = rec.shape[1]
    for i, ks in enumerate(want):
        assert tuple(Y.parts(rec[i])) == tuple(ks), (name, i, Y.parts(rec[i]))
        assert sum(len(k) for k in ks) == K
        for l in range(3):
            m = len(ks[l])
            assert st[l, i, 0] == m
            if m == 0:
                assert (bits(st[l, i]) == 0).all()
                continue
            mem = L[i][ks[l]]
            s = np.zeros(3)
            for v in mem:
                s = s + v
            assert (bits(st[l, i, 1:4]) == bits(s / float(m))).all()
            d = mem - st[l, i, 1:4]
            assert np.allclose(st[l, i, 4:7], (d * d).sum(axis=0), rtol=1e-12, atol=0)
            if l < 2:                                                          # the layer's own aggregate: of its members alone
                one = R.reduce_one(detmath_cpu, rec[i][ks[l]])
                assert (bits(surf[l, i, :15]) == bits(one[:15])).all() and surf[l, i, 15] == m / K
                assert R.sample_class(surf[l, i]) == R.sample_class(rec[i][ks[l][0]])


def test_a_mean_starts_at_plus_zero():
    """( 0.0 + -0.0 ) / 1 is +0.0: the statistics start their sums at +0.0, as acn_render_lens_stats does; the surface record of the
    same sample keeps its -0.0"""
    r = R.hit_record(2.0, 5, -1, 0, alb=(-0.0, 0.5, 0.5))
    st = Y.part_stats(np.array([[-0.0, 1.0, -0.0]]), [0])
    assert not np.signbit(st[1]) and not np.signbit(st[3]) and st[2] == 1.0
    assert np.signbit(Y.layer_surface(None, np.array([r]), [0])[9])


@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 33, 100])
def test_the_inputs_of_the_device_test(detmath_cpu, K):
    """synthetic_split must contain what test_gpu_lens_layers.py is to cover: ties for either layer, a miss class as layer 0 and as
    layer 1, layer 1 absent, more than 8 classes with a layer 1 that first appears after the 8-class table has overflowed, and
    radiances with -0.0, inf and NaN"""
    rec, L, pat = Y.synthetic_split(33, K)
    with np.errstate(all="ignore"):
        surf, st = Y.split(detmath_cpu, rec, L)
        check_split(detmath_cpu, rec, L, surf, st)
    assert np.signbit(L[L == 0]).any() and np.isinf(L).any() and np.isnan(L).any()
    assert np.isnan(st).any()
    assert (st[1][:, 0] == 0).any()                                           # layer 1 absent
    miss0, miss1 = ~(surf[0][:, 0] < np.inf), ~(surf[1][:, 0] < np.inf) & (st[1][:, 0] > 0)
    assert miss0.any()
    if K >= 2:
        assert miss1.any()
        assert ((st[0][:, 0] == st[1][:, 0])).any() or K % 2                 # a tie for layer 0 (two classes in turn, even K)
    if K >= 3:
        tie1 = [i for i in range(33) if pat[i] == 2]
        assert tie1 and all(st[1][i, 0] == st[2][i, 0] > 0 for i in tie1)     # layer 1 and the rest tie: the first of them wins
        assert all(surf[1][i, 7] == 7 for i in tie1)
    if K >= 17:
        many = [i for i in range(33) if pat[i] == 5]
        assert many
        for i in many:
            cl = R.classes(rec[i])
            assert len(cl) > 8
            order = [c for c, _ in cl]
            assert order.index(R.sample_class(surf[1][i])) >= 8               # layer 1 first appears after eight other classes
            assert order.index(R.sample_class(surf[0][i])) > order.index(R.sample_class(surf[1][i]))
            assert st[2][i, 0] >= 9


@pytest.fixture(scope="module")
def frame():
    st, rec = Y.synthetic_frame(37, 29)
    st.setflags(write=False); rec.setflags(write=False)
    return st, rec


def test_the_synthetic_frame_has_what_the_filter_tells_apart(detmath_cpu, frame):
    st, rec = frame
    w, h = 37, 29
    bg = np.array([0.3, 0.35, 0.4])
    detail = {}
    out = Y.denoise_layers(detmath_cpu, st, rec, w, h, bg, iterations=3, detail=detail)
    ok, cross = detail["ok"], detail["cross"]
    e = np.stack([T.empty(st[l]) for l in range(3)])
    assert ok[0].any() and ok[1].any() and (ok[0] & ok[1]).sum() >= 20        # the two-surface edge
    assert cross[0] > 0 and cross[1] > 0                                      # a minority layer finds its neighbour's majority, and back
    emit = (rec[0][:, 12].astype(int) & 1) == 1
    assert emit.sum() >= 8 and not ok[0].reshape(-1)[emit].any()
    miss0 = ~(rec[0][:, 0] < np.inf) & ~e[0]
    miss1 = ~(rec[1][:, 0] < np.inf) & ~e[1]
    assert miss0.any() and miss1.any()
    gone = e.all(axis=0)
    assert gone.sum() >= 10 and (bits(out.reshape(-1, 3)[gone]) == bits(np.tile(bg, (int(gone.sum()), 1)))).all()
    assert ((st[0][:, 0] == 1) & e[1] & e[2]).any()                           # the pixel of one sample
    assert (~e[2]).sum() >= 3                                                 # a rest
    assert np.isnan(out).sum() == 1                                           # the NaN channel of one mean: its layer is copied, never a tap
    # a pixel whose only record is a sky layer 0 keeps its mean
    only_sky = miss0 & e[1] & e[2]
    assert only_sky.any() and (bits(out.reshape(-1, 3)[only_sky]) == bits(st[0][only_sky, 1:4])).all()
    # the emitter pixels with nothing else: the mean, bit for bit
    only_emit = emit & e[1] & e[2]
    assert only_emit.any() and (bits(out.reshape(-1, 3)[only_emit]) == bits(st[0][only_emit, 1:4])).all()


@pytest.mark.parametrize("params", [dict(iterations=3), dict(iterations=2, normal_power_log2=3, demodulate=False)])
def test_one_plane_is_denoise_stats(detmath_cpu, frame, params):
    """with plane 1 and the rest EMPTY the model of the layered filter is the model of acn_denoise_stats on plane 0, bit for bit"""
    st, rec = frame
    w, h = 37, 29
    bg = np.array([0.3, 0.35, 0.4])
    st1 = np.zeros_like(st); st1[0] = st[0]
    rec1 = rec.copy(); rec1[1] = R.miss_record(0, 0.0)
    got = Y.denoise_layers(detmath_cpu, st1, rec1, w, h, bg, **params)
    want = T.denoise_stats(detmath_cpu, st[0], rec[0], w, h, bg, **params)
    assert Y.same_bits(got, want).size == 0


# ---- the host-side checks under the sanitizers ----
def test_host_checks_in_a_sanitized_program(tmp_path):
    """acn_layers_host.h compiled with tests/csrc/layers_cpu.cpp into a program of its own with -fsanitize=address,undefined;
    nothing sanitized is loaded here"""
    exe = tmp_path / "layers_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "layers_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
