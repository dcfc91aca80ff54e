"""Layered records merged across passes and resolved (acn_lens_layers_merge*, acn_lens_layers_resolve_dev; include/actinon_hip.h) without
a GPU: the numpy model of tests/lens_layers_merge_model.py on hand-made positions whose answers are known without it, conservation,
agreement with one call of all the samples, the identities the header states, and the host-side checks of csrc/acn_layers_host.h in a
stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import lens_layers_merge_model as G
import lens_layers_model as Y
import lens_surface_model as R
import stats_model as T
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acn_lens_layers_merge_dev", "acn_lens_layers_merge", "acn_lens_layers_resolve_dev")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\s*\(", text, re.M), name
        assert name in A._lib.HIP_SYMBOLS and getattr(hip, name).argtypes, name
    for method in ("lens_layers_merge", "lens_layers_merge_dev", "lens_layers_resolve", "lens_layers_resolve_dev"):
        assert callable(getattr(A.Handle, method))


def test_the_documents_define_the_merge():
    """the three sentences that left the merge out of scope are gone, and the header defines every step"""
    for doc in (os.path.join("include", "actinon_hip.h"), "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "Out of scope: merging layered records" not in text, doc
        assert "acn_lens_layers_merge" in text and "acn_lens_layers_resolve_dev" in text, doc
    header = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for word in ("CLASS LIST", "PAIR MERGE", "RANKING", "REST", "COVERAGE"):
        assert word in header, word


def test_entry_points_refuse_a_null_handle():
    surf, st = np.full((2, 4, 16), 7.25), np.full((3, 4, 8), 7.25)
    psurf, pst = np.zeros((2, 4, 16)), np.zeros((3, 4, 8))
    rgb, noise, pooled = np.full((4, 3), 7.25), np.full(4, 7.25), np.full((4, 8), 7.25)
    calls = {
        "acn_lens_layers_merge": lambda: hip.acn_lens_layers_merge(None, surf.ctypes.data, st.ctypes.data, 4, psurf.ctypes.data, pst.ctypes.data, 4, None, None),
        "acn_lens_layers_merge_dev": lambda: hip.acn_lens_layers_merge_dev(None, surf.ctypes.data, st.ctypes.data, 4, psurf.ctypes.data, pst.ctypes.data, 4, None, None),
        "acn_lens_layers_resolve_dev": lambda: hip.acn_lens_layers_resolve_dev(None, st.ctypes.data, 4, rgb.ctypes.data, noise.ctypes.data, pooled.ctypes.data, None),
    }
    assert set(calls) == set(NAMES)
    for name, call in calls.items():
        hip.acn_scene_upload(None, 0, None)                                  # (sets another message, or none)
        assert call() == abi.ACN_ERR_ARG, name
        assert b"null" in hip.acn_last_error(), (name, hip.acn_last_error())
    assert all((a == 7.25).all() for a in (surf, st, rgb, noise, pooled))


# ---- hand-made positions ----
@pytest.fixture(scope="module")
def hand():
    out = G.hand_made()
    for a in out[1:5]:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def merged(detmath_cpu, hand):
    _, a_surf, a_st, b_surf, b_st, _ = hand
    return G.merge(detmath_cpu, a_surf, a_st, b_surf, b_st)


def test_the_patterns_are_all_there(hand):
    names = hand[0]
    assert len(names) == len(set(names)) >= len(G.PATTERNS) + 14
    for word in ("empty acc", "part empty", "B0 = A0", "B0 = A1", "B1 = A0", "B1 = A1", "crossed", "four classes", "tie at rank 1 / 2",
                 "tie at rank 2 / 3", "swap", "miss", "EMPTY by nan", "EMPTY by inf", "EMPTY by 0.5"):
        assert any(word in n for n in names), word


@pytest.mark.parametrize("p", range(len(G.hand_made()[0])))
def test_hand_made_positions(hand, merged, p):
    """the layers' classes and counts as written down beside the pattern; exact conservation; a single contributor bit for bit; a
    merged pair against the weighted means computed here"""
    names, a_surf, a_st, b_surf, b_st, want = hand
    surf, st = merged[0][:, p], merged[1][:, p]
    if want[p] == "unwritten":
        assert (bits(surf) == bits(a_surf[:, p])).all() and (bits(st) == bits(a_st[:, p])).all(), names[p]
        return
    layers, n_rest = want[p]
    slots = [(a_surf[l, p], a_st[l, p]) for l in range(2)] + [(b_surf[l, p], b_st[l, p]) for l in range(2)]
    present = [s for s in slots if not G.empty1(s[1])]
    put_in = sum(s[1][0] for s in present) + sum(r[0] for r in (a_st[2, p], b_st[2, p]) if not G.empty1(r))
    assert (st[0, 0] + st[1, 0]) + st[2, 0] == put_in, names[p]               # conservation, exact
    assert st[2, 0] == n_rest and (st[:, 7] == 0).all(), names[p]
    for l in range(2):
        if layers[l] is None:
            blank = G.absent_layer()
            assert (bits(surf[l]) == bits(blank[0])).all() and (bits(st[l]) == 0).all(), (names[p], l)
            continue
        key, n = layers[l]
        assert R.sample_class(surf[l]) == key and st[l, 0] == n, (names[p], l, R.sample_class(surf[l]), st[l, 0])
        assert surf[l, 15] == n / put_in, (names[p], l)                       # coverage: n_l / K_p
        mine = [s for s in present if R.sample_class(s[0]) == key]
        if len(mine) == 1:                                                    # a single contributor: 15 doubles and the record, bit for bit
            assert (bits(surf[l, :15]) == bits(mine[0][0][:15])).all() and (bits(st[l]) == bits(mine[0][1])).all(), (names[p], l)
            continue
        assert len(mine) == 2
        (sa, ta), (sb, tb) = mine
        w = np.array([ta[0], tb[0]]) / (ta[0] + tb[0])
        assert np.allclose(st[l, 1:4], w[0] * ta[1:4] + w[1] * tb[1:4], rtol=1e-14, atol=0)
        d = tb[1:4] - ta[1:4]
        assert np.allclose(st[l, 4:7], ta[4:7] + tb[4:7] + d * d * (ta[0] * tb[0] / (ta[0] + tb[0])), rtol=1e-13, atol=0)
        assert surf[l, 13] == sa[13] and surf[l, 7] == sa[7] and surf[l, 8] == sa[8]
        assert np.isclose(surf[l, 14], w[0] * sa[14] + w[1] * sb[14], rtol=1e-14, atol=0)
        if key[0]:
            for f in (0, 1, 2, 3, 9, 10, 11):
                assert np.isclose(surf[l, f], w[0] * sa[f] + w[1] * sb[f], rtol=1e-13, atol=1e-15), (names[p], l, f)
            g = w[0] * sa[4:7] + w[1] * sb[4:7]
            if "cancel" in names[p]:
                assert (bits(surf[l, 4:7]) == 0).all()
            else:
                assert np.allclose(surf[l, 4:7], g / np.sqrt(g @ g), rtol=1e-13, atol=1e-15)
            assert surf[l, 12] == float(int(sa[12]) | int(sb[12]))
        else:
            assert surf[l, 0] == np.inf and (surf[l, 1:7] == 0).all() and (surf[l, 9:13] == 0).all() and surf[l, 7] == surf[l, 8] == -1


def test_demoted_statistics_are_folded_in_ranked_order(detmath_cpu, hand):
    """four distinct classes: the rest is ( ( Ar + Br ) + third ) + fourth of the ranking, and their surface records are gone"""
    names, a_surf, a_st, b_surf, b_st, _ = hand
    p = names.index("four classes")
    detail = {}
    surf, st = G.merge_one(detmath_cpu, a_surf[:, p], a_st[:, p], b_surf[:, p], b_st[:, p], detail=detail)
    assert detail["demoted"] == [G.key_of(G.D_), G.key_of(G.B_)]               # D has 3 samples, B has 2
    want = T.merge(T.merge(T.merge(a_st[2, p][None], b_st[2, p][None]), b_st[1, p][None]), a_st[1, p][None])[0]
    assert (bits(st[2]) == bits(want)).all()
    kind = names.index("kind bits")
    surf, _ = G.merge_one(detmath_cpu, a_surf[:, kind], a_st[:, kind], b_surf[:, kind], b_st[:, kind])
    assert surf[0, 12] == float(2 | 64 | 8 | 16)


# ---- the identities the header states ----
def test_an_empty_accumulator_becomes_the_part(detmath_cpu):
    """zero-filled, and EMPTY by other values: all five planes of a part that the split wrote, bit for bit"""
    rec, L, _ = Y.synthetic_split(42, 17)
    with np.errstate(all="ignore"):
        surf, st = Y.split(detmath_cpu, rec, L)
    n = st.shape[1]
    got_surf, got_st = G.merge(detmath_cpu, np.zeros_like(surf), np.zeros_like(st), surf, st)
    assert Y.same_bits(got_surf, surf).size == 0 and Y.same_bits(got_st, st).size == 0
    junk_surf = np.random.default_rng(2).uniform(-1, 1, surf.shape)
    junk_st = np.random.default_rng(3).uniform(0, 1, st.shape)
    junk_st[:, :, 0] = np.array([0.5, np.nan, np.inf, -1.0, 0.0, 0.999])[np.arange(n) % 6]
    got_surf, got_st = G.merge(detmath_cpu, junk_surf, junk_st, surf, st)
    assert Y.same_bits(got_surf, surf).size == 0 and Y.same_bits(got_st, st).size == 0
    # and a part whose three records are EMPTY leaves the accumulator's bytes
    got_surf, got_st = G.merge(detmath_cpu, surf, st, junk_surf, junk_st)
    assert (bits(got_surf) == bits(surf)).all() and (bits(got_st) == bits(st)).all()


def test_plane_0_alone_is_the_statistics_merge(detmath_cpu):
    """plane 1 and the rest EMPTY on both sides, the keys of A0 and B0 equal (hits and misses): statistics plane 0 is stats_model's merge"""
    rng = np.random.default_rng(8)
    n = 24
    cls = [G.A_ if i % 3 else G.SKY for i in range(n)]
    blank = G.absent_layer()
    planes = lambda side: (np.stack([np.stack([s[0] for s in side]), np.stack([blank[0]] * n)]),
                           np.stack([np.stack([s[1] for s in side]), np.zeros((n, 8)), np.zeros((n, 8))]))
    a_surf, a_st = planes([G.slot(rng, cls[i], 1 + i % 5) for i in range(n)])
    for index in (None, rng.permutation(n)):
        target = np.arange(n) if index is None else index
        b_surf, b_st = planes([G.slot(rng, cls[target[j]], 1 + j % 4) for j in range(n)])
        _, got = G.merge(detmath_cpu, a_surf, a_st, b_surf, b_st, index=index)
        assert (bits(got[0]) == bits(T.merge(a_st[0], b_st[0], index=index))).all()
        assert (got[0][:, 0] == a_st[0][:, 0] + b_st[0][target.argsort() if index is not None else target][:, 0]).all()
        assert (got[1:] == 0).all()


def test_indices_out_of_range_are_skipped(detmath_cpu, hand):
    _, a_surf, a_st, b_surf, b_st, _ = hand
    n = a_st.shape[1]
    idx = np.array([-1, n, 2, 0, 1 << 40, -(1 << 40)])
    surf, st = G.merge(detmath_cpu, a_surf, a_st, b_surf[:, :6], b_st[:, :6], index=idx)
    keep = np.ones(n, bool); keep[[2, 0]] = False
    assert (bits(surf[:, keep]) == bits(a_surf[:, keep])).all() and (bits(st[:, keep]) == bits(a_st[:, keep])).all()
    one = G.merge_one(detmath_cpu, a_surf[:, 2], a_st[:, 2], b_surf[:, 2], b_st[:, 2])
    assert (bits(surf[:, 2]) == bits(one[0])).all() and (bits(st[:, 2]) == bits(one[1])).all()


# ---- two halves of 2 K samples against one call of all of them ----
@pytest.mark.parametrize("K", [4, 8, 17])
def test_two_halves_agree_with_one_call(detmath_cpu, K):
    """synthetic_split( n, 2 K ) cut into the samples [ 0, K ) and [ K, 2 K ), each split, the two merged.  The pooled record against the
    record of all 2 K samples: the mean to 1e-12, m2 to 1e-9 (both are few-ulp rearrangements of the same sums on data of order 1;
    measured here: 4.5e-16 and 6.7e-16 at the most).  Where the two halves hold at most two classes in total a layer's n is that of the
    split of all 2 K samples and its mean agrees to 1e-12"""
    n = 42
    rec, L, _ = Y.synthetic_split(n, 2 * K)
    with np.errstate(all="ignore"):
        halves = [Y.split(detmath_cpu, rec[:, h * K:(h + 1) * K], L[:, h * K:(h + 1) * K]) for h in range(2)]
        whole_surf, whole_st = Y.split(detmath_cpu, rec, L)
        surf, st = G.merge(detmath_cpu, halves[0][0], halves[0][1], halves[1][0], halves[1][1])
        assert ((st[0][:, 0] + st[1][:, 0]) + st[2][:, 0] == 2 * K).all()     # conservation, exact
        pooled = G.pooled(st)
        want = np.stack([Y.part_stats(L[i], list(range(2 * K))) for i in range(n)])
        assert (pooled[:, 0] == 2 * K).all()
        finite = np.isfinite(L).all(axis=(1, 2))
        assert finite.sum() >= n // 2
        err_mean = np.abs(pooled[finite, 1:4] / want[finite, 1:4] - 1).max()
        err_m2 = np.abs(pooled[finite, 4:7] / want[finite, 4:7] - 1).max()
        print(f"K = {K}: pooled mean off by {err_mean:.3g}, m2 by {err_m2:.3g} (relative)")
        assert np.allclose(pooled[finite, 1:4], want[finite, 1:4], rtol=1e-12, atol=0)
        assert np.allclose(pooled[finite, 4:7], want[finite, 4:7], rtol=1e-9, atol=0)
        # a channel with an infinite or NaN radiance has no finite mean either way (inf - inf in the merge's dl * f is a NaN, not the
        # inf of the one sum): it is not finite on both sides, and the other channels of the position agree as above
        ch = np.isfinite(L).all(axis=1)
        assert not np.isfinite(pooled[:, 1:4][~ch]).any() and not np.isfinite(want[:, 1:4][~ch]).any()
        assert np.allclose(pooled[:, 1:4][ch], want[:, 1:4][ch], rtol=1e-12, atol=0)
        assert np.allclose(pooled[:, 4:7][ch], want[:, 4:7][ch], rtol=1e-9, atol=0)
        few = np.array([len(R.classes(rec[i])) <= 2 for i in range(n)])
        assert few.sum() >= n // 2
        for l in range(2):
            assert (st[l][few, 0] == whole_st[l][few, 0]).all()
            fin = few & finite
            assert np.allclose(st[l][fin, 1:4], whole_st[l][fin, 1:4], rtol=1e-12, atol=0)
            assert [R.sample_class(r) for r in surf[l][few]] == [R.sample_class(r) for r in whole_surf[l][few]]
            cols = [0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14]                      # (the normal of two halves is the normalised mean of two
            assert np.allclose(surf[l][few][:, cols], whole_surf[l][few][:, cols], rtol=1e-12, atol=1e-15)   # unit normals: another vector)
            assert (surf[l][few, 15] == whole_surf[l][few, 15]).all()
            length = np.sqrt((surf[l][few, 4:7] ** 2).sum(axis=1))
            hit = surf[l][few, 0] < np.inf
            assert np.allclose(length[hit], 1.0, rtol=1e-14) and (length[~hit] == 0).all()


def test_the_resolve_model(detmath_cpu):
    """three EMPTY records give the background and +inf; n = 1 gives +inf; else the resolve of the pooled record"""
    st = np.zeros((3, 4, 8))
    rng = np.random.default_rng(4)
    st[0, 1] = G.slot(rng, G.A_, 1)[1]
    st[0, 2], st[1, 2], st[2, 2] = G.slot(rng, G.A_, 5)[1], G.slot(rng, G.B_, 2)[1], G.slot(rng, G.C_, 1)[1]
    st[2, 3] = G.slot(rng, G.A_, 3)[1]                                       # only a rest
    bg = np.array([0.3, 0.35, 0.4])
    rgb, noise, pooled = G.layers_resolve(detmath_cpu, st, bg, 2.2, True)
    assert (bits(rgb[0]) == bits(bg)).all() and noise[0] == np.inf and (bits(pooled[0]) == 0).all()
    assert noise[1] == np.inf and (bits(pooled[1]) == bits(st[0, 1])).all()
    assert pooled[2, 0] == 8 and np.isfinite(noise[2]) and noise[2] > 0
    assert np.allclose(pooled[2, 1:4], (5 * st[0, 2, 1:4] + 2 * st[1, 2, 1:4] + st[2, 2, 1:4]) / 8, rtol=1e-14)
    assert (bits(pooled[3]) == bits(st[2, 3])).all() and (bits(rgb[3]) == bits(st[2, 3, 1:4])).all()


# ---- the host-side checks under the sanitizers ----
def test_host_checks_in_a_sanitized_program(tmp_path):
    """the merge and resolve checks of acn_layers_host.h compiled with tests/csrc/layers_merge_cpu.cpp into a program of its own with
    -fsanitize=address,undefined; nothing sanitized is loaded here"""
    exe = tmp_path / "layers_merge_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "layers_merge_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
