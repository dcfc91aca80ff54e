"""The aggregate surface record (acn_surface_reduce*, acn_surface_lens*; include/actinon_hip.h) without a GPU: the numpy model of
tests/lens_surface_model.py on hand-made records whose answers are known, and on real records -- the oracle's FOLLOW records of the
model's lens rays at the class edges of a wine_glass_c2 frame; the pinhole identity; and the host-side checks of
csrc/acn_lenssurf_host.h in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import lens_model as M
import lens_surface_model as R
import scenes_util as S
import surface_model as SM
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = dict(aperture=0.15, focus=12.0, jitter=True)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_and_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for name in ("acn_surface_reduce", "acn_surface_reduce_dev", "acn_surface_lens", "acn_surface_lens_dev", "acn_surface_lens_main_pass_dev"):
        assert re.search(r"^int " + name + r"\s*\(", text, re.M), name
        assert hasattr(hip, name), name
    assert R.STRIDE == abi.ACN_SURF_STRIDE == 16
    assert A.Surface(np.arange(32.0).reshape(2, 16)).coverage.tolist() == [15.0, 31.0]


def test_entry_points_refuse_a_null_handle():
    rec, out, pos = np.zeros((4, 2, 16)), np.full((4, 16), 7.25), np.zeros((4, 2))
    p = A.Handle.lens_params(samples=2)
    assert hip.acn_surface_reduce(None, rec.ctypes.data, 4, 2, out.ctypes.data, None) == abi.ACN_ERR_ARG
    assert b"handle" in hip.acn_last_error()
    assert hip.acn_surface_reduce_dev(None, rec.ctypes.data, 4, 2, out.ctypes.data, None) == abi.ACN_ERR_ARG
    assert hip.acn_surface_lens(None, pos.ctypes.data, 4, p, 0, out.ctypes.data, None) == abi.ACN_ERR_ARG
    assert hip.acn_surface_lens_dev(None, pos.ctypes.data, 4, p, 0, out.ctypes.data, None) == abi.ACN_ERR_ARG
    assert hip.acn_surface_lens_main_pass_dev(None, 0, 4, p, 0, out.ctypes.data, None) == abi.ACN_ERR_ARG
    assert b"handle" in hip.acn_last_error()
    assert (out == 7.25).all()


@pytest.mark.parametrize("name", list(R.hand_made()))
def test_the_model_on_hand_made_records(detmath_cpu, name):
    rec, want = R.hand_made()[name]
    out = R.reduce(detmath_cpu, rec)
    K = rec.shape[1]
    for i, ((hit, e, x, h), m) in enumerate(want):
        o = out[i]
        assert R.dominant(rec[i])[0] == (hit, e, x, h) and len(R.dominant(rec[i])[1]) == m, (name, i)
        assert o[15] == m / K and o[15] > 0 and o[13] == h
        mem = [r for r in rec[i] if R.sample_class(r) == (hit, e, x, h)]
        assert len(mem) == m
        if not hit:
            blank = SM.blank(1)[0]
            blank[13], blank[14], blank[15] = o[13], o[14], o[15]
            assert (bits(o) == bits(blank)).all()
        else:
            assert (o[7], o[8]) == (e, x) and np.isfinite(o[:15]).all()
            # a mean lies between the least and the largest member (to rounding), and is none of the other classes' values
            lo, hi = np.min(mem, axis=0), np.max(mem, axis=0)
            for f in R.MEANS:
                assert lo[f] - 1e-12 <= o[f] <= hi[f] + 1e-12, (name, i, f)
            kinds = 0
            for r in mem:
                kinds |= int(r[12])
            assert o[12] == kinds
            nn = (o[4] * o[4] + o[5] * o[5]) + o[6] * o[6]
            assert m == 1 or nn == 0 or abs(nn - 1) < 1e-12                  # (m == 1: the sample's normal as it came)
        w = [r[14] for r in mem]
        assert min(w) - 1e-15 <= o[14] <= max(w) + 1e-15
    # what each case is there for
    if name == "m == 1 keeps -0.0":
        assert (bits(out[0, :15]) == bits(rec[0, 0, :15])).all()
        assert np.signbit(out[0, [1, 5, 9]]).all()
    if name == "normals cancel":
        assert (bits(out[0, 4:7]) == 0).all() and out[0, 0] == 3.5 and out[0, 15] == 1.0
    if name == "kind bits differ":
        assert out[0, 12] == (2 | 64 | 8 | 16) and out[0, 15] == 0.75
    if name == "dominant miss":
        assert out[0, 14] == ((0.25 + 0.5) + 0.125) / 3.0 and out[0, 15] == 0.6
    if name == "tie of two, both orders":
        assert (bits(out[0, :15]) == bits(rec[0, 0, :15])).all() and (bits(out[1, :15]) == bits(rec[1, 0, :15])).all()
        assert (out[:, 15] == 0.5).all()
    if name == "K = 4096 of one class":
        assert (out[:, 15] == 1.0).all()
        s = rec[0, 0, 0]
        for v in rec[0, 1:, 0]:
            s = s + v
        assert out[0, 0] == s / 4096.0


def test_a_sum_starts_at_its_first_member():
    """-0.0 alone stays -0.0; 0.0 + -0.0 would be +0.0"""
    r = R.hit_record(2.0, 5, -1, 0, alb=(-0.0, 0.5, 0.5))
    assert np.signbit(R.ordered_mean(np.array([r[9]])))
    assert not np.signbit(np.float64(0.0) + r[9])


@pytest.fixture(scope="module")
def flat():
    sc = A.Scene.build("wine_glass", **dict(S.SMALL["wine_glass_c2"][1], image_width=96, image_height=54))
    return sc.flatten()


@pytest.fixture(scope="module")
def edges(oracle, flat):
    """the 64 edge positions of the pinhole FOLLOW frame"""
    pos = S.positions(flat)
    frame, _ = SM.follow(oracle, flat, SM.camera_rays(flat.params, pos))
    idx, count = R.edge_positions(frame, 96, 54)
    assert count >= 128 and len(idx) == 64, (count, len(idx))
    return pos[idx].copy(), frame


def lens_records(oracle, lib, flat, pos, K, **lens):
    rays = M.lens_rays(lib, oracle, flat.params, pos, samples=K, seed=0, **lens)
    rec, _ = SM.follow(oracle, flat, rays.reshape(-1, 6))
    return rec.reshape(len(pos), K, 16)


def test_the_model_on_real_records(oracle, detmath_cpu, flat, edges):
    """Conditions on the inputs, from a run of this rule with the oracle (208 edge pixels; K = 2: 24 mixed positions, all ties;
    K = 5: 36 mixed, 2 ties, 20 with three or more classes; K = 16: 49 mixed, 4 ties, 35 with three or more), with margin; then what
    every aggregate of real records must satisfy."""
    pos, frame = edges
    seen_miss = 0
    for K, need in ((2, dict(ties=8)), (5, dict(mixed=16, three=8)), (16, dict(ties=1))):
        rec = lens_records(oracle, detmath_cpu, flat, pos, K, **LENS)
        n_cls, tie, miss, cov = R.census(rec)
        print(f"K = {K}: {int((n_cls > 1).sum())} mixed, {int(tie.sum())} ties, {int((n_cls >= 3).sum())} with three or more classes, "
              f"{int(miss.sum())} dominant misses, least coverage {cov.min()}")
        assert tie.sum() >= need.get("ties", 0) and (n_cls > 1).sum() >= need.get("mixed", 0) and (n_cls >= 3).sum() >= need.get("three", 0)
        seen_miss += int(miss.sum())
        out = R.reduce(detmath_cpu, rec)
        assert (out[:, 15] == cov).all() and (out[:, 15] > 0).all()
        pure = n_cls == 1
        assert pure.any() and (out[pure, 15] == 1.0).all()
        hit = out[:, 0] < np.inf
        nn = (out[hit, 4:7] ** 2).sum(axis=1)
        assert (np.abs(nn - 1) < 1e-12).all()
        for i in range(len(pos)):
            mem = rec[i][[R.sample_class(r) == R.dominant(rec[i])[0] for r in rec[i]]]
            assert (out[i, [7, 8, 13]] == mem[0, [7, 8, 13]]).all()
            if hit[i]:
                assert mem[:, 0].min() - 1e-9 <= out[i, 0] <= mem[:, 0].max() + 1e-9
    # positions whose dominant class is a miss: some of the 64, or four sky pixels of the frame's border are added
    if seen_miss == 0:
        sky = np.flatnonzero(~(frame[:, 0] < np.inf))
        border = [i for i in sky if i % 96 in (0, 95) or i // 96 in (0, 53)][:4]
        assert len(border) == 4
        rec = lens_records(oracle, detmath_cpu, flat, S.positions(flat)[border], 5, **LENS)
        seen_miss = int(R.census(rec)[2].sum())
        out = R.reduce(detmath_cpu, rec)
        assert (out[R.census(rec)[2], 0] == np.inf).all()
    assert seen_miss >= 1


def test_jitter_alone_gives_ties(oracle, detmath_cpu, flat, edges):
    """a closed aperture: the anti-aliased silhouettes alone (22 ties at K = 2 in the run the conditions come from)"""
    rec = lens_records(oracle, detmath_cpu, flat, edges[0], 2, jitter=True)
    assert R.census(rec)[1].sum() >= 8


def test_pinhole_identity(oracle, detmath_cpu, flat, edges):
    """K = 1 without jitter and with aperture 0 is the surface record of the pixel centre in doubles 0 .. 14, bit for bit"""
    pos = edges[0]
    rays = M.lens_rays(detmath_cpu, oracle, flat.params, pos, samples=1)
    centre = np.concatenate(M.Camera(detmath_cpu, flat.params).rays(pos[:, 0], pos[:, 1]), axis=-1)
    for fn in (SM.follow, SM.first_hit):
        rec, _ = fn(oracle, flat, centre)
        out = R.reduce(detmath_cpu, fn(oracle, flat, rays.reshape(-1, 6))[0].reshape(len(pos), 1, 16))
        assert (bits(out[:, :15]) == bits(rec[:, :15])).all()
        assert (rec[:, 15] == 0).all() and (out[:, 15] == 1.0).all()


# ---- the host-side checks under the sanitizers ----
def test_host_checks_in_a_sanitized_program(tmp_path):
    """acn_lenssurf_host.h compiled with tests/csrc/lenssurf_cpu.cpp into a program of its own with -fsanitize=address,undefined;
    nothing sanitized is loaded here"""
    exe = tmp_path / "lenssurf_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "lenssurf_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
