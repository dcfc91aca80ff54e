"""Shadow records and the history guard without a GPU: the model of tests/shadow_model.py against two independent routes of the
oracle, the numpy guard against answers computed by hand, the refusals that need no device, the constants against the header."""
import ctypes as C
import os

import numpy as np
import pytest

import actinon_amd as A
import scenes_util as S
import shadow_model as SM
import surface_model as M
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for name, value in (("ACN_SHADOW_STRIDE", abi.ACN_SHADOW_STRIDE), ("ACN_SHADOW_NONE", abi.ACN_SHADOW_NONE), ("ACN_SHADOW_SAMPLED", abi.ACN_SHADOW_SAMPLED),
                        ("ACN_SHADOW_DEFAULT_SAMPLES", abi.ACN_SHADOW_DEFAULT_SAMPLES), ("ACN_SHADOW_MAX_SAMPLES", abi.ACN_SHADOW_MAX_SAMPLES),
                        ("ACN_SHADOW_HISTORY_DROP", abi.ACN_SHADOW_HISTORY_DROP),
                        ("ACN_SHADOW_HISTORY_DEFAULT_TOLERANCE", abi.ACN_SHADOW_HISTORY_DEFAULT_TOLERANCE),
                        ("ACN_SHADOW_HISTORY_DEFAULT_MAX_HISTORY", abi.ACN_SHADOW_HISTORY_DEFAULT_MAX_HISTORY)):
        line = [ln for ln in text.splitlines() if ln.startswith(f"#define {name} ")]
        assert len(line) == 1, name
        assert float(line[0].split()[2].rstrip("u")) == value, name
    assert (SM.STRIDE, SM.EMITTER, SM.DEFAULT_TOLERANCE, SM.DEFAULT_CAP) == (
        abi.ACN_SHADOW_STRIDE, abi.ACN_SURF_EMITTER, abi.ACN_SHADOW_HISTORY_DEFAULT_TOLERANCE, abi.ACN_SHADOW_HISTORY_DEFAULT_MAX_HISTORY)
    assert (SM.TAP_SURFACE, SM.TAP_DIFFUSE, SM.TAP_LIGHT, SM.TAP_DIRECT) == tuple(
        __import__("oracle_binding").Oracle.TAP[k] for k in ("surface", "diffuse", "light", "direct"))


@pytest.mark.parametrize("fn", ["acn_shadow_records", "acn_shadow_records_dev"])
def test_records_refusals_without_a_device(fn):
    """a null handle comes first; nothing is written"""
    buf = np.full((4, 16), 7.0)
    st = getattr(hip, fn)(None, buf.ctypes.data, 2, None, buf.ctypes.data, None)
    assert st == abi.ACN_ERR_ARG and b"handle" in hip.acn_last_error()
    assert (buf == 7.0).all()


@pytest.mark.parametrize("fn", ["acn_shadow_limit_history", "acn_shadow_limit_history_dev"])
def test_guard_refusals_without_a_device(fn):
    buf = np.full((4, 16), 7.0)
    st = getattr(hip, fn)(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 2, 2, 1, None, buf.ctypes.data, None)
    assert st == abi.ACN_ERR_ARG and b"handle" in hip.acn_last_error()
    assert (buf == 7.0).all()


@pytest.mark.parametrize("name,S_", [("primitives_c1", 8), ("textured", 8), ("wine_glass_c2", 8), ("diamond_c4", 8), ("primitives_c1", 1), ("textured", 64)])
def test_the_tap_is_reproduced_by_two_one_ray_queries(oracle, name, S_):
    """The tap's light answer [ 7 ] and occlusion answer [ 9 ] of every direct-light sample, against obj_ray_hit of the light and the
    `occluded` query of the matter root on the tap's own out_d: the model rests on two routes through the oracle.  Every hit with a
    diffuse block gets exactly S samples per light (record_from_tap asserts it)."""
    sc, flat = S.build(name)
    pos = S.positions(flat)
    pos = pos[::max(1, len(pos) // 150)]
    rays = M.camera_rays(flat.params, pos)
    surf, _ = M.first_hit(oracle, flat, rays)
    rays = rays.copy()
    rays[:, 3:] = M.of_length_1(rays[:, 3:])
    # the model's position is origin + direction * a in numpy, the tap's is ray_pos: the same expression; keep the rows where they agree
    n_lights = flat.node(flat.c.light_root).child1
    light_elems = [flat.c.elems[flat.node(flat.c.light_root).child0 + k] for k in range(n_lights)]
    compared = samples = asked_all = occluded_all = 0
    for i in np.flatnonzero(SM.sampled(surf)):
        rows = SM.tap_rows(oracle, flat, rays[i], surf[i], S_)
        if rows is None:
            continue
        compared += 1
        direct = rows[rows[:, 0] == SM.TAP_DIRECT]
        assert len(direct) == S_ * n_lights
        assert np.array_equal(direct[:, 1], np.tile(np.arange(S_), n_lights))
        assert np.array_equal(direct[:, 2], np.repeat(light_elems, S_))
        P = np.tile(surf[i, 1:4], (len(direct), 1))
        q = np.concatenate([P, direct[:, 3:6]], axis=1)
        facing = direct[:, 6] > 0
        assert np.isinf(direct[~facing, 7]).all()
        for e in light_elems:
            sel = facing & (direct[:, 2] == e)
            if sel.any():
                assert np.array_equal(oracle.query_rays(flat, "obj_ray_hit", e, q[sel])[:, 0], direct[sel, 7])
        ask = facing & (direct[:, 7] < np.inf)
        if ask.any():
            occ = oracle.query_rays(flat, "occluded", flat.c.matter_root, q[ask], limits=direct[ask, 7])[:, 5]
            assert np.array_equal(occ, direct[ask, 9])
        rec = SM.record_from_tap(oracle, flat, rays[i], surf[i], S_)
        assert rec[3] == ask.sum() and rec[4] == (ask & (direct[:, 9] == 0)).sum() and rec[1] == S_ and rec[2] == n_lights
        samples += len(direct); asked_all += int(ask.sum()); occluded_all += int((ask & (direct[:, 9] == 1)).sum())
    hits = int((surf[:, 0] < np.inf).sum())
    print(f"{name} S={S_}: {compared} of {hits} hits compared, {samples} samples, {asked_all} asked, {occluded_all} occluded")
    assert compared >= 0.5 * hits and compared >= 20 and asked_all >= compared


def test_a_record_of_counts():
    r = SM.record_of_counts(4, np.array([4, 3, 0, 1, 2, 4, 4]), np.array([4, 0, 0, 1, 1, 2, 0]))
    assert r.tolist() == [1, 4, 7, 18, 8, 8 / 18, 4, 0, 0, 1, 1, 4, 3, 0, 1, 2]
    r = SM.record_of_counts(2, np.array([0]), np.array([0]))
    assert r.tolist() == [1, 2, 1, 0, 0, 0] + [0] * 10


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("cap", [None, 4.0])
def test_the_numpy_guard_against_hand_computed_answers(drop, cap):
    h = SM.hand_case()
    got, change = SM.limit_history(h["stats"], h["motion"], h["cur"], h["prev"], SM.W_HAND, SM.H_HAND, changed_max_history=cap, drop=drop)
    want, want_change = SM.hand_answers(drop=drop, cap=cap)
    for i, name in enumerate(h["rows"]):
        assert np.array_equal(got[i], want[i]), (name, got[i], want[i])
        assert (np.isnan(change[i]) and np.isnan(want_change[i])) or change[i] == want_change[i], (name, change[i], want_change[i])
    assert np.isnan(change).sum() == 9 and (change == 0.25).sum() == 1
    # the input is not written
    assert np.array_equal(h["stats"], SM.hand_case()["stats"])


def test_the_guard_with_another_tolerance():
    h = SM.hand_case()
    i = h["rows"].index("change equals the tolerance")
    got, change = SM.limit_history(h["stats"], h["motion"], h["cur"], h["prev"], SM.W_HAND, SM.H_HAND, tolerance=0.2499)
    assert change[i] == 0.25 and got[i].tolist() == [1.0, 1, 2, 3, 0.5, 0.625, 0.75, 0]
    got, _ = SM.limit_history(h["stats"], h["motion"], h["cur"], h["prev"], SM.W_HAND, SM.H_HAND, tolerance=0.5)
    j = h["rows"].index("change above the tolerance")
    assert np.array_equal(got[j], h["stats"][j])


def test_params_of_keyword_arguments():
    p = A.Handle.shadow_params(8)
    assert (p.struct_size, p.flags, p.samples) == (12, 0, 8)
    q = A.Handle.shadow_history_params(tolerance=0.5, drop=True)
    assert (q.struct_size, q.flags, q.tolerance, q.changed_max_history) == (24, abi.ACN_SHADOW_HISTORY_DROP, 0.5, 0.0)
    assert C.sizeof(abi.ShadowParams) == 12 and C.sizeof(abi.ShadowHistoryParams) == 24
