"""acn_fill_stats without a GPU (include/actinon_hip.h, "Filling"): the properties of the numpy model tests/fill_model.py that the
device is compared with bit for bit in test_gpu_fill.py -- the four classes and their `need`, the frames the fill must leave alone,
what a filled record is to the calls that read it -- the constants of the three restatements, and the one host-side check of the
entry points (actinon_amd/csrc/acn_fill_host.h) behind the shim tests/csrc/fill_cpu.cpp: the versioned parameter block, the
defaults, every refusal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_model as D
import fill_model as F
import stats_model as SM
from actinon_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 23
BG = (0.3, 0.35, 0.4)
CASES = [(2, dict()), (4, dict()), (2, dict(radius=1)), (4, dict(radius=8, normal_power_log2=0)), (2, dict(demodulate=False))]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def filled(detmath_cpu):
    """every case once: ( stats, rec, out, need, detail )"""
    res = []
    for lattice, params in CASES:
        stats, rec = F.synthetic_sparse(W, H, lattice)
        detail = {}
        out, need = F.fill(detmath_cpu, stats, rec, W, H, BG, detail=detail, **params)
        res.append((stats, rec, out, need, detail))
    return res


def test_every_class_occurs_and_need_tells_them_apart(filled):
    for (lattice, params), (stats, rec, out, need, detail) in zip(CASES, filled):
        cls = detail["cls"]
        n = F.counts(cls)
        print(lattice, params, n)
        assert all(n[name] > 0 for name in F.CLASS_NAMES), n
        assert sum(n.values()) == W * H
        assert (need[cls == F.RENDERED] == -1.0).all()
        assert (need[cls == F.BACKGROUND] == 0.0).all()
        nf = need[cls == F.FILLED]
        print("need of the filled positions: min", nf.min(), "max", nf.max())
        assert ((nf >= 0.0) & (nf < 1.0)).all(), (nf.min(), nf.max())
        assert np.isposinf(need[cls == F.UNFILLED]).all()
        assert np.array_equal(F.classes(stats, need, rec), cls)
        e = SM.empty(stats).reshape(H, W)
        assert same_bits(out.reshape(H, W, 8)[~e], stats.reshape(H, W, 8)[~e])                        # RENDERED: bit for bit
        assert same_bits(out.reshape(H, W, 8)[cls == F.UNFILLED], stats.reshape(H, W, 8)[cls == F.UNFILLED])
        assert (out.reshape(H, W, 8)[cls == F.BACKGROUND] == np.array([1.0, *BG, 0, 0, 0, 0])).all()
        # the thin class has no donor on the lattice: where it is a receiver it stays UNFILLED; emitters are never filled
        thin = (rec[:, 7] == 77).reshape(H, W)
        assert thin.any() and (cls[thin & e] == F.UNFILLED).all()
        emit = F.emitter(rec).reshape(H, W)
        assert (cls[emit & e] == F.UNFILLED).all() and (emit & e).any()


def test_a_frame_with_no_empty_record_comes_back_bit_for_bit(detmath_cpu):
    stats, rec = F.synthetic_sparse(W, H, 1)
    assert not SM.empty(stats).any()
    out, need = F.fill(detmath_cpu, stats, rec, W, H, BG)
    assert same_bits(out, stats) and (need == -1.0).all()


def test_an_all_empty_frame_is_background_or_unfilled(detmath_cpu):
    stats, rec = F.synthetic_sparse(W, H, 2)
    detail = {}
    out, need = F.fill(detmath_cpu, np.zeros_like(stats), rec, W, H, BG, detail=detail)
    cls = detail["cls"]
    assert set(np.unique(cls)) == {F.BACKGROUND, F.UNFILLED}
    assert np.array_equal(cls == F.BACKGROUND, ~(rec[:, 0] < np.inf).reshape(H, W))
    assert (out[(cls == F.UNFILLED).ravel()] == 0.0).all()


def test_a_filled_record_is_a_record_to_its_readers(filled, detmath_cpu):
    """not EMPTY, finite, resolved to its mean with a finite or infinite noise, never NaN; its variance of the mean is the weighted
    mean of its donors' demodulated variances, remodulated"""
    for (stats, rec, out, need, detail) in filled:
        f = (detail["cls"] == F.FILLED).ravel()
        r = out[f]
        assert not SM.empty(r).any() and np.isfinite(r).all() and (r[:, 7] == 0).all()
        assert set(np.unique(r[:, 0])) <= {1.0, 2.0} and (r[r[:, 0] == 1.0, 4:7] == 0).all() and (r[:, 4:7] >= 0).all()
        rgb, noise = SM.resolve(detmath_cpu, r, BG, 2.2, True)
        assert same_bits(rgb, r[:, 1:4]) and not np.isnan(noise).any()
        assert np.isposinf(noise[r[:, 0] == 1.0]).all() and np.isfinite(noise[r[:, 0] == 2.0]).all()
        two = f & (out[:, 0] == 2.0)
        assert two.any()
        with np.errstate(all="ignore"):
            want = (detail["su"] / detail["swv"][..., None]) * (detail["a"] * detail["a"])
        assert same_bits(SM.variance_of_mean(out)[two], want.reshape(-1, 3)[two])
        # and the donors' u is their own vm over a * a
        d = detail["donor"].ravel() & (stats[:, 0] > 1.0)
        with np.errstate(all="ignore"):
            assert same_bits(detail["u"].reshape(-1, 3)[d], SM.variance_of_mean(stats)[d] / (detail["a"] * detail["a"]).reshape(-1, 3)[d])


def test_a_receiver_borrows_from_its_own_surface_only(detmath_cpu):
    """two flat half planes of different objects and colours: every filled mean is its own side's colour, and need is 0 deep inside
    a side and grows towards the edge"""
    w, h = 24, 12
    rec = D.blank(h * w).reshape(h, w, 16)
    y, x = np.mgrid[0:h, 0:w]
    left = x < 12
    rec[..., 0] = 5.0
    rec[..., 1], rec[..., 2], rec[..., 3] = x * 0.1, y * 0.1, 0.0
    rec[..., 4:7] = [0.0, 0.0, 1.0]
    rec[..., 7] = np.where(left, 3, 4)
    rec[..., 9:12] = np.where(left[..., None], [0.5, 0.5, 0.5], [0.25, 0.5, 1.0])
    rec[..., 12] = 2
    stats = np.zeros((h, w, 8))
    stats[..., 0] = 4.0
    stats[..., 1:4] = np.where(left[..., None], [0.25, 0.25, 0.25], [0.5, 1.0, 2.0])
    stats[..., 4:7] = 0.01
    stats[~F.lattice_mask(w, h, 2)] = 0.0
    out, need = F.fill(detmath_cpu, stats.reshape(-1, 8), rec.reshape(-1, 16), w, h, BG)
    out = out.reshape(h, w, 8)
    assert (need != np.inf).all()
    assert (out[left][:, 1:4] == 0.25).all() and (out[~left][:, 1:4] == [0.5, 1.0, 2.0]).all()
    e = SM.empty(stats.reshape(-1, 8)).reshape(h, w)
    inner = e & ((x < 8) | (x > 15))
    assert (need[inner] == 0.0).all()
    assert (need[e & ((x == 11) | (x == 12))] > need[e & ((x == 9) | (x == 14))].max()).all()


def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    d = dict(re.findall(r"^#define ACN_FILL_(\w+)\s+([0-9.]+)\s", text, re.M))
    assert d == {"DEFAULT_RADIUS": "3", "MAX_RADIUS": "8", "DEFAULT_SIGMA_PX": "1.5", "DEFAULT_SIGMA_PLANE": "0.1"}
    assert (abi.ACN_FILL_DEFAULT_RADIUS, abi.ACN_FILL_MAX_RADIUS, abi.ACN_FILL_DEFAULT_SIGMA_PX, abi.ACN_FILL_DEFAULT_SIGMA_PLANE) \
        == (F.DEFAULT_RADIUS, F.MAX_RADIUS, F.DEFAULT_SIGMA_PX, F.DEFAULT_SIGMA_PLANE) == (3, 8, 1.5, 0.1)
    assert C.sizeof(abi.FillParams) == 32 and [f[0] for f in abi.FillParams._fields_] == \
        re.findall(r"^\s+(?:uint32_t|double)\s+(\w+);", text[text.index("typedef struct acn_fill_params"):text.index("} acn_fill_params;")], re.M)
    for name in ("acn_fill_stats_dev", "acn_fill_stats"):
        assert re.search(r"^int " + name + r"\s*\(", text, re.M), name
    assert "actinon_hip.h" in F.__doc__
    for word in ("DONOR", "RENDERED", "BACKGROUND", "RECEIVER", "FILLED", "UNFILLED", "need = 1.0 - sw / sa", "acn_select_above_dev"):
        assert word in text, word


# ---- the host-side check ----
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """acn_fill_host.h compiled for the host behind tests/csrc/fill_cpu.cpp"""
    out = tmp_path_factory.mktemp("fill") / "libfill_cpu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "actinon_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "fill_cpu.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.fill_check.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                               C.c_void_p, C.c_char_p, C.c_size_t]
    return lib


BASE = 1 << 20          # addresses are compared, never followed


def run_check(shim, prm=None, stats=BASE, surface=BASE * 2, w=8, h=4, out=BASE * 3, need=BASE * 4, world=1, handle=1):
    setup = np.full(5, -1.0)
    msg = C.create_string_buffer(256)
    st = shim.fill_check(handle, stats, surface, w, h, None if prm is None else C.addressof(prm), out, need, world, setup.ctypes.data, msg, 256)
    return st, tuple(setup), msg.value.decode()


def test_parameter_block_versions_and_defaults(shim):
    defaults = (3.0, 7.0, 0.0, 1.5, 0.1)
    assert run_check(shim)[:2] == (abi.ACN_OK, defaults)
    p = abi.FillParams()
    p.struct_size = C.sizeof(p)
    assert run_check(shim, p)[:2] == (abi.ACN_OK, defaults)
    p.radius, p.normal_power_log2, p.flags, p.sigma_px, p.sigma_plane = 5, 2, abi.ACN_DENOISE_NO_DEMODULATE, 0.75, 0.5
    want = {32: (5.0, 2.0, 1.0, 0.75, 0.5), 24: (5.0, 2.0, 1.0, 0.75, 0.1), 16: (5.0, 2.0, 1.0, 1.5, 0.1), 12: (5.0, 2.0, 0.0, 1.5, 0.1),
            8: (5.0, 7.0, 0.0, 1.5, 0.1), 4: defaults, 40: (5.0, 2.0, 1.0, 0.75, 0.5), 1 << 20: (5.0, 2.0, 1.0, 0.75, 0.5)}
    for size, setup in want.items():           # every layout a caller may have been compiled with; nothing beyond sizeof is read
        p.struct_size = size
        assert run_check(shim, p)[:2] == (abi.ACN_OK, setup), size
    for size in (0, 1, 3):
        p.struct_size = size
        st, _, msg = run_check(shim, p)
        assert st == abi.ACN_ERR_ARG and "struct_size" in msg
    # normal_power_log2 = 0 is expressible with the flag only
    q = abi.FillParams()
    q.struct_size = C.sizeof(q)
    q.flags = abi.ACN_DENOISE_NORMAL_POWER_SET
    assert run_check(shim, q)[1][1] == 0.0
    q.radius = 8
    assert run_check(shim, q)[1][0] == 8.0


def test_refusals(shim):
    def bad(word, prm=None, **kw):
        st, setup, msg = run_check(shim, prm, **kw)
        assert st == abi.ACN_ERR_ARG and word in msg and setup == (-1.0,) * 5, (word, st, msg)

    def params(**kw):
        p = abi.FillParams()
        p.struct_size = C.sizeof(p)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad("null", handle=0)
    bad("null", stats=None)
    bad("null", surface=None)
    bad("null", out=None)
    assert run_check(shim, need=None)[0] == abi.ACN_OK
    bad("width", w=0)
    bad("width", h=0)
    bad("2^31", w=1 << 16, h=(1 << 15) + 1)
    bad("2^31", w=1 << 40, h=1 << 40)
    bad("radius", params(radius=9))
    bad("normal_power_log2", params(normal_power_log2=11))
    bad("flags", params(flags=4))
    for s in (-0.5, float("inf"), float("nan")):
        bad("sigma", params(sigma_px=s))
        bad("sigma", params(sigma_plane=s))
    bad("sharded", world=2)
    bad("align", stats=BASE + 8)
    bad("align", out=BASE * 3 + 8)
    bad("align", surface=BASE * 2 + 8)
    bad("align", need=BASE * 4 + 4)
    n_bytes = 8 * 4 * 64
    bad("overlaps", out=BASE)                                  # in place
    bad("overlaps", out=BASE + n_bytes - 16)                   # the last record of stats
    bad("overlaps", out=BASE - n_bytes + 16)
    assert run_check(shim, out=BASE + n_bytes)[0] == abi.ACN_OK    # behind it
    bad("overlaps", need=BASE + 64)
    bad("overlaps", need=BASE * 3 + n_bytes - 8)
    assert run_check(shim, need=BASE * 3 + n_bytes)[0] == abi.ACN_OK
