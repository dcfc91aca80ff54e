"""The planning arithmetic of the pipeline runner (actinon_amd/csrc/acn_queueplan.h) without a GPU: queue capacities, chunk sizes,
learned rates, the reading of a chunk's counter blocks, walk passes, lanes and the tile order behind the shim tests/csrc/queueplan_cpu.cpp.  Every function is compared with
a short Python model of the expressions launch_render, ensure_workspace, learn_rates, render_chunk, render_lanes and render_dispatch
had in line before the header existed: integers with ==, doubles bit for bit (Python floats are the same IEEE doubles; the shim is
built with -ffp-contract=off, as the library is).  The same file with its own main runs under the address and undefined-behaviour
sanitizers.  And the lane counts the GPU tests that say they run on concurrent lanes rely on."""
import ctypes as C
import os
import re
import struct
import subprocess
from math import gcd

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "csrc", "queueplan_cpu.cpp")
T, CH, HS, HP, R = range(5)                      # WQ_*
REC = [112 + 16, 48, 64, 96, 2 * 80]              # bytes per record of the five queues: any five will do, the header is handed them
MAXCAP = 0xFFFFFF00


# the counter block of a path level as it is today (actinon_amd/csrc/acn_counts.h): pinned, the device writes these words
LAYOUT = {"QC_TASKS": 0, "QC_CLASS0": 1, "QC_CHILDREN": 5, "QC_FLAGS": 6, "QC_HARD_SHADOW": 7, "QC_HARD_PATH": 8, "QS_WALK_RAYS": 12,
          "QS_HARD_SHADOW": 13, "QS_HARD_PATH": 14, "QS_CHILDREN": 15, "QS_TASKS": 16, "QS_WALK_STEPS": 17, "QS_PRIVATE_RAYS": 18, "QS_PROBES": 19,
          "QS_DEAD_T": 28, "QS_DEAD_C": 29, "QS_DEAD_HP": 30, "QS_DEAD_R": 31, "QC_GEN": 32, "QC_N": 104, "ACN_QCHUNK": 64}
QC_N, GEN, GENS, LEVEL_BLOCKS = LAYOUT["QC_N"], LAYOUT["QC_GEN"], 33, 6         # ACN_MAX_WALK_PASSES + 1 generation words; ACN_MAX_PATH_LEVELS + 1 levels
TASK_OVERFLOW, CHILD_OVERFLOW, STACK_OVERFLOW, CLAMPED = 1, 2, 4, 8            # ACN_FLAG_*
FITS, OVERFLOW, FAILS = 0, 1, 2                                                 # ACN_CHUNK_*


def dbl(v):
    return (C.c_double * len(v))(*v)


def u32(v):
    return (C.c_uint32 * len(v))(*v)


def u64(v):
    return (C.c_uint64 * len(v))(*v)


def same_bits(a, b):
    return struct.pack(f"{len(a)}d", *a) == struct.pack(f"{len(b)}d", *b)


@pytest.fixture(scope="module")
def qp(tmp_path_factory):
    out = tmp_path_factory.mktemp("queueplan") / "libqueueplan_cpu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared"] + INCLUDES + [SOURCE, "-o", str(out)])
    lib = C.CDLL(str(out))
    u, i, d, p = C.c_uint64, C.c_int, C.c_double, C.c_void_p
    for name, res, args in (("qp_first_chunk_guess", u, [C.c_uint32, C.c_uint32, u, u, u, u]), ("qp_sample_positions", u, [C.c_uint32, C.c_uint32, u, u, u, u]),
                            ("qp_wanted_caps", None, [p, i, u, u, u, u, u, u, p, p]), ("qp_keep_caps", i, [p, u, u, p, p, i, C.c_uint32, i, p, p]),
                            ("qp_halve_caps", i, [p]), ("qp_rates_known", i, [p]), ("qp_queue_demand", d, [p, i, i]), ("qp_chunk_for_caps", u, [p, i, d, p]),
                            ("qp_set_rates", None, [p, p, C.c_uint32, p, d]), ("qp_learn_rates", None, [p, p, C.c_uint32, p, d]),
                            ("qp_overflow_rates", None, [p, C.c_uint32, p]), ("qp_sample_rates", None, [p, i, C.c_uint32, u, C.c_uint, p]),
                            ("qp_read_chunk", None, [p, i, p, i, p, p]), ("qp_constant", C.c_int64, [C.c_char_p]),
                            ("qp_walk_passes", C.c_uint32, [u, i, C.c_uint32, C.c_uint32]), ("qp_walk_passes_seen", C.c_uint32, [p, C.c_uint32]),
                            ("qp_lane_count", u, [u, i, i]), ("qp_lanes_for_counts", i, [i, u, u]), ("qp_one_lane", i, [p, i, u, p, u, i]),
                            ("qp_tile_order", C.c_uint32, [u, i, p])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


# ---- the models: the expressions as they stood in actinon_hip.hip ----
def m_known(rate):
    return rate[T] > 0 or rate[R] > 0 or rate[HS] > 0


def m_demand(rate, q, seeded):
    return 1.0 if seeded and q == R and rate[q] < 1.0 else rate[q]


def m_chunk_for_caps(rate, seeded, fill_target, cap):
    chunk = 2.0e9
    for q in range(5):
        r = m_demand(rate, q, seeded) if m_demand(rate, q, seeded) > 1e-3 else 1e-3
        c = fill_target * float(cap[q]) / r
        if c < chunk:
            chunk = c
    return 64 if chunk < 64 else int(chunk)


def m_first_guess(cap_children, cap_hs, ps, ds, n_lights, most):
    s = ps if ps else 1
    want = int(float(cap_children) / (float(s + 2) * (float(s) / 64.0 if s > 64 else 1.0)))
    by_shadow = int(float(cap_hs) / (0.25 * float(ds * n_lights + s) + 4.0))
    if want > by_shadow:
        want = by_shadow
    if want > most:
        want = most
    return want


def m_sample_positions(cap_children, cap_hs, ps, ds, n_lights, n):
    want = m_first_guess(cap_children, cap_hs, ps, ds, n_lights, 4096)
    if want < 256:
        want = 256
    if want > n // 4:
        want = n // 4
    return want


def m_wanted_caps(rate, seeded, n, ps, ds, n_lights, budget, stack_bytes, rec=REC):
    want = [0] * 5
    if not m_known(rate):
        s = ps if ps else 1
        per_pos = (s + 2) * (s // 16 if s > 16 else 1) + ds * n_lights
        recs = min(n * per_pos + 65536, 1 << 20)
        per_rec = rec[HS] + sum(rec)
        max_recs = (budget - stack_bytes) // per_rec if budget > stack_bytes else 0
        recs = min(recs, max_recs)
        want = [recs] * 5
        want[HS] = 2 * recs
    else:
        positions = float(n if n < (1 << 22) else (1 << 22))
        nbytes = 0.0
        slack = 1.4
        for q in range(5):
            nbytes += (slack * m_demand(rate, q, seeded) * positions / 0.7 + 65536.0) * float(rec[q])
        room = float(budget - stack_bytes) if budget > stack_bytes else 0.0
        if nbytes > room:
            positions *= room / nbytes
        for q in range(5):
            c = slack * m_demand(rate, q, seeded) * positions / 0.7 + 65536.0
            want[q] = MAXCAP if c > 4.0e9 else int(c)
    return [min(max(w, 65536), MAXCAP) for w in want]


def m_keep_caps(cap, have_waves, waves, want, known, rate_cnt, trimmed, sized_calls, rec=REC):
    """-> fits, trim, sized_calls"""
    fits = have_waves >= waves
    for q in range(5):
        if float(cap[q]) < float(want[q]) / 1.4:
            fits = False
    if known and rate_cnt >= 32768:
        sized_calls += 1
    trim = False
    if fits and known and rate_cnt >= 32768 and not trimmed and sized_calls <= 3:
        have = sum(cap[q] * rec[q] for q in range(5))
        need = sum(want[q] * rec[q] for q in range(5))
        if float(have) > 1.25 * float(need) and have - need > (1 << 29):
            fits, trim = False, True
    return fits, trim, sized_calls


def m_set_rates(cnt, fill, dead_share):
    live = 1.0 - dead_share if cnt <= 4096 and 0 < dead_share < 0.95 else 1.0
    return [max(live * float(fill[q]) / float(cnt), 1e-3) for q in range(5)], cnt


def m_learn_rates(rate, rate_cnt, cnt, fill, dead_share):
    if not m_known(rate) or cnt >= (4 * rate_cnt) % (1 << 32):
        return m_set_rates(cnt, fill, dead_share)
    return [max(max(float(fill[q]) / float(cnt), 0.85 * rate[q]), 1e-3) for q in range(5)], max(cnt, rate_cnt)


def m_sample_rates(counts, levels, cnt, plan_positions, plan_grid):
    w = LAYOUT
    live = [0.0] * 5
    for level in range(levels):
        c = counts[level * QC_N:(level + 1) * QC_N]
        gens = [c[GEN + g] for g in range(GENS)]
        s = 0.0
        for g in gens:
            s += g
        s -= float(c[w["QS_DEAD_R"]])
        top = float(max(gens))
        for q, v in ((T, float(c[w["QC_TASKS"]]) - float(c[w["QS_DEAD_T"]])), (CH, float(c[w["QC_CHILDREN"]]) - float(c[w["QS_DEAD_C"]])),
                     (HS, float(c[w["QS_HARD_SHADOW"]]) + float(c[w["QS_PROBES"]])), (HP, float(c[w["QC_HARD_PATH"]]) - float(c[w["QS_DEAD_HP"]])),
                     (R, s if s < top else top)):
            if v > live[q]:
                live[q] = v
    per_launch = float(w["ACN_QCHUNK"]) * 4.0 * float(plan_grid)
    walkers, shaders = 3.0 * per_launch, 3.0 * per_launch
    dead = [walkers, shaders, walkers + shaders, shaders, walkers]
    pp = float(min(plan_positions, 1 << 22))
    ray_bound = 2.0 * live[CH] + live[T]
    if live[R] > ray_bound and ray_bound > 0:
        live[R] = ray_bound
    return [max(1.2 * live[q] / float(cnt) + dead[q] / pp, 1e-3) for q in range(5)]


def m_walk_passes(trace_depth, level, tun_passes, seen):
    depth_left = trace_depth - 10 * level if trace_depth > 10 * level else 1
    passes = tun_passes
    if passes > depth_left + 1:
        passes = depth_left + 1
    if seen and seen + 1 < passes:
        passes = seen + 1
    return passes


def m_walk_passes_seen(gen, launched):
    used = 1
    for g in range(launched):
        if gen[g]:
            used = g + 1
    return used + 2 if used == launched and launched > 1 else used


STATS = ("levels", "walk_rays", "walk_steps", "hard_rays", "shade_hit_recs", "private_rays", "probe_rays", "peak_tasks", "peak_children")


def m_read_chunk(counts, levels, passes, seeded):
    """What render_chunk did between its synchronisation and its return -> the report, and the words as it left them"""
    w = LAYOUT
    h = list(counts)
    if seeded:
        h[GEN + 0] = 0
    blocks = [h[level * QC_N:(level + 1) * QC_N] for level in range(levels)]
    flags = 0
    for level, c in enumerate(blocks):
        flags |= c[w["QC_FLAGS"]]
        if c[GEN + passes[level]]:
            flags |= CHILD_OVERFLOW
    fill = [0] * 5
    for c in blocks:
        for q, v in [(T, c[w["QC_TASKS"]])] + [(T, c[w["QC_CLASS0"] + k]) for k in range(4)] + [(CH, c[w["QC_CHILDREN"]]), (HS, c[w["QC_HARD_SHADOW"]]),
                                                                                               (HP, c[w["QC_HARD_PATH"]])] + [(R, c[GEN + g]) for g in range(GENS)]:
            if v > fill[q]:
                fill[q] = v
    mark = recs = 0
    for c in blocks:
        if c[w["QC_HARD_SHADOW"]] > mark:
            mark, recs = c[w["QC_HARD_SHADOW"]], (c[w["QS_HARD_SHADOW"]] + c[w["QS_PROBES"]]) % (1 << 32)
    dead_share = float(mark - recs) / float(mark) if mark > 0 and recs < mark else 0.0
    rep = dict(flags=flags, fill=fill, dead_share=dead_share, passes_seen=[0] * LEVEL_BLOCKS, **{k: 0 for k in STATS})
    rep["verdict"] = OVERFLOW if flags & (TASK_OVERFLOW | CHILD_OVERFLOW) else FAILS if flags & STACK_OVERFLOW else FITS
    if rep["verdict"] != FITS:
        return rep, h
    for c in blocks:
        if c[w["QC_TASKS"]] == 0 and c[w["QS_WALK_RAYS"]] == 0:
            break
        rep["levels"] += 1
        rep["walk_rays"] += c[w["QS_WALK_RAYS"]]
        rep["walk_steps"] += c[w["QS_WALK_STEPS"]]
        rep["hard_rays"] += c[w["QS_HARD_SHADOW"]] + c[w["QS_HARD_PATH"]]
        rep["shade_hit_recs"] += c[w["QS_CHILDREN"]]
        rep["peak_tasks"] = max(rep["peak_tasks"], c[w["QC_TASKS"]])
        rep["peak_children"] = max(rep["peak_children"], c[w["QC_CHILDREN"]])
        rep["private_rays"] += c[w["QS_PRIVATE_RAYS"]]
        rep["probe_rays"] += c[w["QS_PROBES"]]
    for level, c in enumerate(blocks):
        rep["passes_seen"][level] = m_walk_passes_seen(c[GEN:GEN + GENS], passes[level])
    return rep, h


def m_lane_count(n, lanes, lane):
    tiles = (n + 255) // 256
    if tiles == 0:
        return 0
    cnt = (tiles // lanes + (1 if lane < tiles % lanes else 0)) * 256
    if (tiles - 1) % lanes == lane:
        cnt -= tiles * 256 - n
    return cnt


def m_lanes_for_counts(tun_lanes, n, ps):
    lanes = tun_lanes
    work = n * (ps + 1)
    while lanes > 1 and (n < lanes * 32 * 256 or work < lanes << 20):
        lanes -= 1
    return lanes


def m_one_lane(rate, seeded, n, budget, was_one_lane, rec=REC):
    need = 0.0
    for q in range(5):
        need += m_demand(rate, q, seeded) * float(n) / 0.7 * float(rec[q])
    return need > (0.7 if was_one_lane else 1.0) * float(budget)


def m_tile_order(n, shift=8):
    n_tiles = (n + (1 << shift) - 1) >> shift
    mul = 1
    if n_tiles > 2:
        m = int(0.6180339887 * n_tiles) | 1
        while gcd(m, n_tiles) != 1:
            m += 2
        mul = m % n_tiles
    return n_tiles, mul


# ---- the comparisons ----
STARTER = (1 << 20, 2 << 20)                    # capacities of the starter set: path-sample hits, deferred shadow rays


@pytest.mark.parametrize("ps", [0, 16, 64, 1024])
def test_first_chunk_guess_and_sample(qp, ps):
    """One guess with two caps: 32 768 positions for a first chunk, 4096 for the learning sample, which has a floor of 256 and n / 4.
    At path_samples 1024 the guess is 63 positions, below the 64 a sample needs: the floor is what makes the handle learn at all."""
    for ds, lights in ((0, 1), (50, 1), (200, 3), (30, 17)):
        for caps in (STARTER, (65536, 131072), (MAXCAP, MAXCAP)):
            for most in (4096, 32768):
                assert qp.qp_first_chunk_guess(*caps, ps, ds, lights, most) == m_first_guess(*caps, ps, ds, lights, most)
            for n in (0, 3, 63, 255, 1024, 16384, 57600, 2073600):
                assert qp.qp_sample_positions(*caps, ps, ds, lights, n) == m_sample_positions(*caps, ps, ds, lights, n)
    if ps == 1024:
        assert qp.qp_first_chunk_guess(*STARTER, ps, 30, 17, 4096) == 63
        assert qp.qp_sample_positions(*STARTER, ps, 30, 17, 2073600) == 256
    if ps == 64:
        assert qp.qp_sample_positions(*STARTER, ps, 200, 1, 2073600) == 4096


def wanted(qp, rate, seeded, n, ps, ds, lights, budget, stack):
    out = u64([0] * 5)
    qp.qp_wanted_caps(dbl(rate), seeded, n, ps, ds, lights, budget, stack, u64(REC), out)
    return list(out)


def test_wanted_capacities(qp):
    """Both branches of ensure_workspace: the starter set and the learned rates with slack 1.4 at 1 / 0.7, scaled to the budget less
    the stacks, with both clamps."""
    stack = 1024 * 4 * 512 * 80
    rng = np.random.default_rng(5)
    cases = []
    for ps in (0, 16, 64, 1024):
        for n in (1, 5, 63, 4096, 57600, 2073600, 1 << 23):
            for budget in (0, stack - 1, stack, stack + 1, 48 << 20, 8 << 30, 64 << 30):
                cases.append(([0.0] * 5, 0, n, ps, 50, 3, budget, stack))
                cases.append(([0.0, 7.0, 0.0, 3.0, 0.0], 0, n, ps, 50, 3, budget, stack))         # (not known: children and path rays alone)
                for seeded in (0, 1):
                    rate = list(rng.uniform(1e-3, 30.0, 5) * (ps + 1))
                    rate[R] = float(rng.choice([1e-3, 0.25, 0.999, 1.0, 7.5]))
                    cases.append((rate, seeded, n, ps, 50, 3, budget, stack))
    # a demand above 4e9 records; a budget that scales such a demand down
    cases.append(([1.0, 3.0e5, 1.0, 1.0, 1.0], 0, 1 << 22, 1024, 30, 17, (1 << 64) - 1, 0))
    cases.append(([1.0, 3.0e5, 5.0e4, 1.0, 1.0], 0, 1 << 22, 1024, 30, 17, 64 << 30, stack))
    for c in cases:
        assert wanted(qp, *c) == m_wanted_caps(*c), c
    assert wanted(qp, *cases[-2])[CH] == MAXCAP
    assert wanted(qp, [0.0] * 5, 0, 57600, 64, 50, 3, stack - 1, stack) == [65536] * 5          # a budget smaller than the stacks: the floor
    assert wanted(qp, [2.0] * 5, 0, 57600, 64, 50, 3, stack - 1, stack) == [65536] * 5
    few = wanted(qp, [0.0] * 5, 0, 5, 16, 50, 3, 8 << 30, stack)                                # n below 64
    assert few[T] == 5 * (18 + 150) + 65536 and few[HS] == 2 * few[T]
    # a ray call whose learned ray rate is below 1 plans one slot per ray
    low = [2.0, 2.0, 2.0, 2.0, 0.25]
    assert qp.qp_queue_demand(dbl(low), R, 1) == 1.0 and qp.qp_queue_demand(dbl(low), R, 0) == 0.25 and qp.qp_queue_demand(dbl(low), T, 1) == 2.0
    assert wanted(qp, low, 1, 57600, 64, 50, 3, 8 << 30, stack)[R] == int(1.4 * 1.0 * 57600.0 / 0.7 + 65536.0)
    assert wanted(qp, low, 0, 57600, 64, 50, 3, 8 << 30, stack)[R] == int(1.4 * 0.25 * 57600.0 / 0.7 + 65536.0)


def test_keep_trim_and_halve(qp):
    """Queues stay while they hold want / 1.4; they are trimmed once, when they hold 25 % and half a GiB more than wanted, and only in
    the first three sizing steps after rates from a large chunk: sized_calls 3 trims, 4 does not."""
    rng = np.random.default_rng(6)

    def both(cap, have_waves, waves, want, known, rate_cnt, trimmed, sized_calls):
        sc, tr = C.c_uint32(sized_calls), C.c_int(7)
        fits = qp.qp_keep_caps(u32(cap), have_waves, waves, u64(want), u64(REC), known, rate_cnt, trimmed, C.byref(sc), C.byref(tr))
        assert (bool(fits), bool(tr.value), sc.value) == m_keep_caps(cap, have_waves, waves, want, known, rate_cnt, trimmed, sized_calls)
        return bool(fits), bool(tr.value), sc.value

    big, small = [1 << 24] * 5, [1 << 20] * 5
    assert both(big, 4096, 4096, small, 1, 40000, 0, 2) == (False, True, 3)           # the third sizing step still trims
    assert both(big, 4096, 4096, small, 1, 40000, 0, 3) == (True, False, 4)           # the fourth does not
    assert both(big, 4096, 4096, small, 1, 40000, 1, 0) == (True, False, 1)           # trimmed once already
    assert both(big, 4096, 4096, small, 1, 32767, 0, 0) == (True, False, 0)           # rates from a small chunk: no window yet
    assert both(big, 4095, 4096, small, 1, 40000, 0, 0) == (False, False, 1)          # the stacks are short: allocated anew, not a trim
    assert both(small, 4096, 4096, [int(1.4 * (1 << 20))] * 5, 0, 0, 0, 0)[0] is True
    assert both(small, 4096, 4096, [int(1.4 * (1 << 20)) + 2] * 5, 0, 0, 0, 0)[0] is False
    for _ in range(300):
        cap = [int(x) for x in rng.integers(65536, 1 << 26, 5)]
        want = [int(x) for x in rng.integers(65536, 1 << 26, 5)] if rng.random() < 0.5 else [max(65536, c // int(rng.integers(1, 4))) for c in cap]
        both(cap, int(rng.integers(4094, 4098)), 4096, want, int(rng.random() < 0.8), int(rng.choice([0, 8192, 32767, 32768, 1 << 20])),
             int(rng.random() < 0.2), int(rng.integers(0, 5)))
    for want in ([65536] * 5, [65537, 65536, 65536, 65536, 65536], [131071, 131072, 131073, 1 << 20, MAXCAP]):
        w = u64(want)
        floor = qp.qp_halve_caps(w)
        assert floor == int(all(x <= 65536 for x in want)) and list(w) == [max(65536, x // 2) for x in want]


def test_queue_demand_and_chunk_for_caps(qp):
    rng = np.random.default_rng(7)
    for _ in range(400):
        rate = [float(x) for x in rng.choice([0.0, 1e-4, 1e-3, 0.5, 1.0, 15.0, 3.0e5], 5)]
        cap = [int(x) for x in rng.choice([0, 1, 65536, 1 << 20, MAXCAP], 5)]
        seeded, target = int(rng.random() < 0.5), float(rng.choice([0.3, 0.7, 0.595]))
        assert qp.qp_rates_known(dbl(rate)) == int(m_known(rate))
        assert qp.qp_chunk_for_caps(dbl(rate), seeded, target, u32(cap)) == m_chunk_for_caps(rate, seeded, target, cap)
    assert qp.qp_chunk_for_caps(dbl([0.0] * 5), 0, 0.7, u32([MAXCAP] * 5)) == 2000000000
    assert qp.qp_chunk_for_caps(dbl([1e9] * 5), 0, 0.7, u32([65536] * 5)) == 64


def test_rate_updates(qp):
    """set_rates with the dead-share correction, the follow-upwards and forget-slowly rule and the lower bounds of an overflowed chunk"""
    rng = np.random.default_rng(8)
    for _ in range(400):
        cnt = int(rng.choice([1, 64, 4095, 4096, 4097, 32768, 230400]))
        fill = [int(x) for x in rng.integers(0, 1 << 22, 5)]
        dead = float(rng.choice([0.0, -0.1, 0.3, 0.949, 0.95, 0.99]))
        rate0 = [float(x) for x in rng.choice([0.0, 1e-3, 0.8, 12.0, 400.0], 5)]
        cnt0 = int(rng.choice([0, 1024, 8192, 57600, (1 << 30) + 5]))
        r, rc = dbl([0.0] * 5), C.c_uint32(0)
        qp.qp_set_rates(r, C.byref(rc), cnt, u32(fill), dead)
        want, want_cnt = m_set_rates(cnt, fill, dead)
        assert same_bits(list(r), want) and rc.value == want_cnt
        r, rc = dbl(rate0), C.c_uint32(cnt0)
        qp.qp_learn_rates(r, C.byref(rc), cnt, u32(fill), dead)
        want, want_cnt = m_learn_rates(rate0, cnt0, cnt, fill, dead)
        assert same_bits(list(r), want) and rc.value == want_cnt, (rate0, cnt0, cnt, fill, dead)
        r = dbl(rate0)
        qp.qp_overflow_rates(r, cnt, u32(fill))
        assert same_bits(list(r), [max(rate0[q], float(fill[q]) / float(cnt)) for q in range(5)])


def test_rates_of_the_learning_sample(qp):
    """Live records per level from the counter words (marks less dead slots, the fullest level), the ray bound, a fifth on top and the
    dead slots of a chunk of the planned size on the planned grid"""
    rng = np.random.default_rng(9)
    for trial in range(200):
        levels = int(rng.integers(1, 7))
        counts = [int(x) for x in rng.integers(0, 1 << int(rng.integers(1, 31)), QC_N * levels)]
        if trial % 3 == 0:                                              # dead slots above the marks: negative live counts lose
            for level in range(levels):
                counts[level * QC_N + LAYOUT["QS_DEAD_T"]] = MAXCAP
                counts[level * QC_N + LAYOUT["QS_DEAD_R"]] = MAXCAP
        cnt, pp, grid = int(rng.choice([64, 256, 4096])), int(rng.choice([1, 9600, 57600, 1 << 22, 1 << 25])), int(rng.choice([7, 256, 1024]))
        r = dbl([0.0] * 5)
        qp.qp_sample_rates(u32(counts), levels, cnt, pp, grid, r)
        assert same_bits(list(r), m_sample_rates(counts, levels, cnt, pp, grid)), (trial, levels, cnt, pp, grid)


def test_the_counter_block_is_where_it_was(qp):
    """The words of a level's counter block, stated: the kernels write them, acn_counts.h names them once, and the planner, Handle.QC
    and these tests read the same table"""
    import actinon_amd as A
    for name, value in LAYOUT.items():
        assert qp.qp_constant(name.encode()) == value, name
    assert qp.qp_constant(b"QS_NO_SUCH_WORD") == -1
    for name, value in (("ACN_MAX_WALK_PASSES", GENS - 1), ("ACN_LEVEL_BLOCKS", LEVEL_BLOCKS), ("ACN_MAX_PATH_LEVELS", LEVEL_BLOCKS - 1), ("ACN_NCLASS", 4),
                        ("QC_CUR_GEN", GEN + GENS), ("WQ_N", 5), ("ACN_FLAG_TASK_OVERFLOW", TASK_OVERFLOW), ("ACN_FLAG_CHILD_OVERFLOW", CHILD_OVERFLOW),
                        ("ACN_FLAG_STACK_OVERFLOW", STACK_OVERFLOW), ("ACN_FLAG_CLAMPED", CLAMPED), ("ACN_FLAGS_CHUNK_LOST", TASK_OVERFLOW | CHILD_OVERFLOW),
                        ("ACN_CHUNK_FITS", FITS), ("ACN_CHUNK_OVERFLOW", OVERFLOW), ("ACN_CHUNK_STACK_OVERFLOW", FAILS)):
        assert qp.qp_constant(name.encode()) == value, name
    names = {"tasks": "QC_TASKS", "class0": "QC_CLASS0", "children": "QC_CHILDREN", "flags": "QC_FLAGS", "hard_shadow": "QC_HARD_SHADOW",
             "hard_path": "QC_HARD_PATH", "walk_rays": "QS_WALK_RAYS", "s_hard_shadow": "QS_HARD_SHADOW", "s_hard_path": "QS_HARD_PATH",
             "s_children": "QS_CHILDREN", "s_tasks": "QS_TASKS", "s_probes": "QS_PROBES", "dead_t": "QS_DEAD_T", "dead_c": "QS_DEAD_C",
             "dead_hp": "QS_DEAD_HP", "dead_r": "QS_DEAD_R", "gen0": "QC_GEN"}
    assert A.Handle.QC == {k: LAYOUT[v] for k, v in names.items()}


def test_last_stage_names_are_the_headers_enum():
    """Handle.last_stages names the 25 slots of acn_last_stage_ms as the ACN_LAST_* enum of include/actinon_hip.h does, in its order"""
    import actinon_amd as A
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    body = re.search(r"enum\s*\{([^}]*?ACN_LAST_N[^}]*)\};\s*int acn_last_stage_ms\s*\(", text, re.S).group(1)
    members = re.findall(r"\bACN_LAST_(\w+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert members[-1] == "N" and "= 0" in body.split(",")[0] and body.count("=") == 1          # counted from 0, no slot moved by hand
    assert [m.lower() for m in members[:-1]] == A.Handle.STAGES and len(A.Handle.STAGES) == 25


def read_chunk(qp, counts, levels, passes, seeded):
    """acn_read_chunk on a copy of the words -> the report as m_read_chunk makes it, and the words as it left them"""
    c, words, dead = u32(counts), u64([0] * (7 + LEVEL_BLOCKS + len(STATS))), C.c_double(-1.0)
    qp.qp_read_chunk(c, levels, u32(passes), seeded, words, C.byref(dead))
    words = list(words)
    rep = dict(flags=words[0], verdict=words[1], fill=words[2:7], passes_seen=words[7:7 + LEVEL_BLOCKS], dead_share=dead.value)
    rep.update(zip(STATS, words[7 + LEVEL_BLOCKS:]))
    return rep, list(c)


def same_report(a, b):
    return {k: v for k, v in a.items() if k != "dead_share"} == {k: v for k, v in b.items() if k != "dead_share"} and same_bits([a["dead_share"]], [b["dead_share"]])


def test_reading_a_chunks_counter_blocks(qp):
    """acn_read_chunk against the expressions render_chunk had after its synchronisation: random blocks, then every edge by hand"""
    w = LAYOUT
    rng = np.random.default_rng(12)
    verdicts = set()
    for trial in range(400):
        levels = int(rng.integers(1, LEVEL_BLOCKS + 1))
        counts = [int(x) for x in rng.integers(0, 1 << int(rng.integers(1, 31)), QC_N * levels)]
        passes = [int(x) for x in rng.integers(1, GENS, LEVEL_BLOCKS)]
        if trial % 4:                                                   # random flag words nearly always say overflow: mostly choose them
            for level in range(levels):
                counts[level * QC_N + w["QC_FLAGS"]] = int(rng.choice([0, 0, 0, CLAMPED, STACK_OVERFLOW, TASK_OVERFLOW, CHILD_OVERFLOW | CLAMPED], p=[.3, .2, .2, .15, .05, .05, .05]))
                if trial % 4 > 1:
                    counts[level * QC_N + GEN + passes[level]] = 0     # ... and leave no rays behind the last pass
        if trial % 5 == 0:                                              # levels that end early
            for i in range(int(rng.integers(0, levels)) * QC_N, levels * QC_N):
                counts[i] = 0 if rng.random() < 0.9 else counts[i]
        seeded = int(rng.random() < 0.5)
        got, want = read_chunk(qp, counts, levels, passes, seeded), m_read_chunk(counts, levels, passes, seeded)
        assert same_report(got[0], want[0]) and got[1] == want[1], (trial, levels, passes, seeded)
        verdicts.add(want[0]["verdict"])
    assert verdicts == {FITS, OVERFLOW, FAILS}

    def chunk(levels, words, passes=4, seeded=0):
        """levels zero blocks with words[(level, name or index)] = value -> the report both ways agree on, and the words left"""
        counts = [0] * (QC_N * levels)
        for (level, word), v in words.items():
            counts[level * QC_N + (w[word] if isinstance(word, str) else word)] = v
        got, want = read_chunk(qp, counts, levels, [passes] * LEVEL_BLOCKS, seeded), m_read_chunk(counts, levels, [passes] * LEVEL_BLOCKS, seeded)
        assert same_report(got[0], want[0]) and got[1] == want[1], words
        return got

    busy, busy2 = ({(level, k): 10 + level for level in range(n) for k in ("QC_TASKS", "QS_WALK_RAYS")} for n in (3, 2))
    # a task overflow in a middle level only
    r, _ = chunk(3, {**busy, (1, "QC_FLAGS"): TASK_OVERFLOW})
    assert r["verdict"] == OVERFLOW and r["flags"] == TASK_OVERFLOW and r["levels"] == 0 and r["fill"][T] == 12
    # rays left in QC_GEN + passes of one level and no flag anywhere
    r, _ = chunk(3, {**busy, (2, GEN + 4): 1})
    assert r["verdict"] == OVERFLOW and r["flags"] == CHILD_OVERFLOW and r["fill"][R] == 1
    r, _ = chunk(3, {**busy, (2, GEN + 3): 1, (2, GEN + 5): 1})         # ... the words beside it do not say so
    assert r["verdict"] == FITS and r["flags"] == 0
    # a stack overflow with a task overflow is a lost chunk, alone it fails the call
    r, _ = chunk(3, {**busy, (0, "QC_FLAGS"): STACK_OVERFLOW, (2, "QC_FLAGS"): TASK_OVERFLOW})
    assert r["verdict"] == OVERFLOW and r["flags"] == STACK_OVERFLOW | TASK_OVERFLOW
    r, _ = chunk(3, {**busy, (1, "QC_FLAGS"): STACK_OVERFLOW})
    assert r["verdict"] == FAILS and r["flags"] == STACK_OVERFLOW and r["levels"] == 0
    # a clamped contribution alone: the chunk fits and the flag is carried -- whatever the verdict
    r, _ = chunk(3, {**busy, (2, "QC_FLAGS"): CLAMPED})
    assert r["verdict"] == FITS and r["flags"] == CLAMPED and r["levels"] == 3 and r["walk_rays"] == 33
    assert chunk(3, {**busy, (2, "QC_FLAGS"): CLAMPED, (0, "QC_FLAGS"): CHILD_OVERFLOW})[0]["flags"] == CLAMPED | CHILD_OVERFLOW
    assert chunk(3, {**busy, (2, "QC_FLAGS"): CLAMPED | STACK_OVERFLOW})[0]["flags"] == CLAMPED | STACK_OVERFLOW
    # the seeded generation: cleared before anything reads it, in level 0 alone
    r, left = chunk(2, {**busy2, (0, GEN): 5000, (1, GEN): 7, (0, GEN + 1): 40}, seeded=1)
    assert left[GEN] == 0 and left[QC_N + GEN] == 7 and r["fill"][R] == 40 and r["passes_seen"][:2] == [2, 1]
    r, left = chunk(2, {**busy2, (0, GEN): 5000, (1, GEN): 7, (0, GEN + 1): 40}, seeded=0)
    assert left[GEN] == 5000 and r["fill"][R] == 5000 and r["passes_seen"][:2] == [2, 1]
    r, _ = chunk(1, {(0, GEN): 5000}, passes=1, seeded=1)               # ... also where it is the only pass: no rays are left over
    assert r["verdict"] == FITS and r["fill"][R] == 0 and r["passes_seen"][0] == 1
    assert chunk(1, {(0, GEN + 1): 5000}, passes=1, seeded=1)[0]["verdict"] == OVERFLOW
    # an all-zero level followed by a non-zero one: the statistics stop before it, the marks do not
    r, _ = chunk(4, {(0, "QC_TASKS"): 9, (0, "QS_WALK_STEPS"): 3, (1, "QS_WALK_STEPS"): 100, (1, "QC_CHILDREN"): 50, (2, "QS_WALK_RAYS"): 77, (2, "QC_TASKS"): 400})
    assert (r["levels"], r["walk_rays"], r["walk_steps"], r["peak_tasks"], r["peak_children"]) == (1, 0, 3, 9, 0) and r["fill"][:2] == [400, 50]
    r, _ = chunk(3, {(0, "QC_TASKS"): 9, (0, "QS_WALK_RAYS"): 4, (2, "QC_TASKS"): 400, (2, "QS_WALK_RAYS"): 77})
    assert (r["levels"], r["walk_rays"], r["peak_tasks"]) == (1, 4, 9) and r["fill"][T] == 400
    r, _ = chunk(3, {(0, "QS_WALK_RAYS"): 1, (1, "QC_TASKS"): 1, (2, "QS_WALK_STEPS"): 5, (1, "QS_HARD_SHADOW"): 0xFFFFFFFF, (1, "QS_HARD_PATH"): 0xFFFFFFFF,
                     (0, "QS_CHILDREN"): 6, (1, "QS_PRIVATE_RAYS"): 8, (1, "QS_PROBES"): 2})
    assert (r["levels"], r["hard_rays"], r["shade_hit_recs"], r["private_rays"], r["probe_rays"]) == (2, 2 * 0xFFFFFFFF, 6, 8, 2)
    # the marks of the size classes count into the task queue
    for k in range(4):
        r, _ = chunk(2, {**busy2, (1, w["QC_CLASS0"] + k): 300 + k})
        assert r["fill"][T] == 300 + k and r["peak_tasks"] == 11
    # the dead share comes from the level with the largest deferred-shadow mark: the last one here
    marks = {**busy, (0, "QC_HARD_SHADOW"): 999, (0, "QS_HARD_SHADOW"): 1, (2, "QC_HARD_SHADOW"): 1000}
    r, _ = chunk(3, {**marks, (2, "QS_HARD_SHADOW"): 900, (2, "QS_PROBES"): 100})
    assert r["dead_share"] == 0.0 and r["fill"][HS] == 1000
    r, _ = chunk(3, {**marks, (2, "QS_HARD_SHADOW"): 900, (2, "QS_PROBES"): 99})
    assert r["dead_share"] == 1.0 / 1000.0
    r, _ = chunk(3, {**marks, (2, "QS_HARD_SHADOW"): 900, (2, "QS_PROBES"): 101})               # (more records than the mark: no share)
    assert r["dead_share"] == 0.0
    r, _ = chunk(3, {**marks, (2, "QC_HARD_SHADOW"): 999, (2, "QS_HARD_SHADOW"): 999})          # an equal mark: the first level keeps it
    assert r["dead_share"] == 998.0 / 999.0
    # every level and every pass the device has
    r, _ = chunk(LEVEL_BLOCKS, {(LEVEL_BLOCKS - 1, GEN + GENS - 1): 3}, passes=GENS - 1)
    assert r["verdict"] == OVERFLOW and r["fill"][R] == 3


def test_walk_passes(qp):
    for depth in (0, 1, 2, 9, 10, 11, 20, 50, 60):
        for level in range(6):
            for tun in (1, 3, 4, 12, 32):
                for seen in (0, 1, 2, 3, 5, 31, 34):
                    assert qp.qp_walk_passes(depth, level, tun, seen) == m_walk_passes(depth, level, tun, seen)
    rng = np.random.default_rng(10)
    for _ in range(300):
        gen = [int(x) for x in rng.choice([0, 0, 0, 1, 77], 33)]
        for launched in (0, 1, 2, 4, 32):
            assert qp.qp_walk_passes_seen(u32(gen), launched) == m_walk_passes_seen(gen, launched)
    assert qp.qp_walk_passes_seen(u32([9, 0, 0, 0]), 4) == 1 and qp.qp_walk_passes_seen(u32([9, 0, 0, 1]), 4) == 6


def test_lanes_and_shards(qp):
    """Every position belongs to exactly one lane, also when the last tile is short, whichever lane it falls to"""
    for lanes in range(1, 17):
        for n in (0, 1, 255, 256, 257, 57600, MAXCAP):
            for tiles in range(lanes + 1):
                m = n + 256 * tiles
                counts = [qp.qp_lane_count(m, lanes, k) for k in range(lanes)]
                assert counts == [m_lane_count(m, lanes, k) for k in range(lanes)]
                assert sum(counts) == m
    for tun in range(1, 17):
        for n in (0, 1, 8191, 8192, 20000, 41472, 57600, 65536, 230400, 2073600):
            for ps in (0, 16, 64, 256, 1024):
                assert qp.qp_lanes_for_counts(tun, n, ps) == m_lanes_for_counts(tun, n, ps)
    assert qp.qp_lanes_for_counts(4, 57600, 16) == 1          # 57 600 x 17 is below 2 << 20
    assert qp.qp_lanes_for_counts(4, 57600, 64) == 3
    rng = np.random.default_rng(11)
    for _ in range(300):
        rate = [float(x) for x in rng.uniform(1e-3, 3000.0, 5)]
        rate[R] = float(rng.choice([0.25, 1.0, 9.0]))
        n, budget = int(rng.choice([57600, 2073600, 8294400])), int(rng.choice([48 << 20, 8 << 30, 64 << 30]))
        for seeded in (0, 1):
            for sticky in (0, 1):
                assert bool(qp.qp_one_lane(dbl(rate), seeded, n, u64(REC), budget, sticky)) == m_one_lane(rate, seeded, n, budget, sticky)
    # the sticky 30 %: a call at 0.8 of the bound stays on one lane once it was there
    rate = [1.0, 0.0, 0.0, 0.0, 0.0]
    budget = int(1000 / 0.7 * REC[T] / 0.8)
    assert not qp.qp_one_lane(dbl(rate), 0, 1000, u64(REC), budget, 0) and qp.qp_one_lane(dbl(rate), 0, 1000, u64(REC), budget, 1)


def test_tile_order_multiplier_is_coprime(qp):
    for tiles in list(range(0, 5001)) + [8100, 65536, MAXCAP >> 8]:
        for n in {tiles * 256, max(0, tiles * 256 - 255)}:
            mul = C.c_uint32(0)
            got = qp.qp_tile_order(n, 8, C.byref(mul))
            assert (got, mul.value) == m_tile_order(n), n
            if got >= 3:
                assert gcd(mul.value, got) == 1 and 0 < mul.value < got


def test_planning_arithmetic_in_a_sanitized_program(tmp_path):
    """tests/csrc/queueplan_cpu.cpp with its own main under -fsanitize=address,undefined -fno-sanitize-recover=all: the edges of every
    rule with each array in a heap block of exactly its size.  Nothing sanitized is loaded here."""
    exe = tmp_path / "queueplan_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DQUEUEPLAN_CPU_MAIN"] + INCLUDES + [SOURCE, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_gpu_tests_that_say_lanes_get_lanes(qp):
    """The shapes of the GPU tests that say they run on concurrent lanes, through acn_lanes_for_counts with the ACN_LANES they set (6
    where they set none).  test_lanes_grid_and_walk_arrangement_do_not_change_a_pixel rendered 320 x 180 at path_samples 16 on ONE
    lane under ACN_LANES=4 and 3 until it was raised to 64: the work condition had been added after the test was written."""
    lanes = qp.qp_lanes_for_counts
    n = 320 * 180
    # tests/test_gpu_parity.py::test_lanes_grid_and_walk_arrangement_do_not_change_a_pixel ("lanes", "all")
    assert n >= 4 * 32 * 256 and lanes(4, n, 64) == 3 and lanes(3, n, 64) == 3 and lanes(1, n, 64) == 1
    # tests/test_gpu_configs.py: test_one_handle_moves_between_its_lanes_and_its_own_run: three lanes, and its 4096 positions one
    assert lanes(3, n, 64) == 3 and lanes(3, 4096, 64) == 1
    # ... test_queue_overflow_retry_is_bit_identical, test_cold_handle_learns_from_a_sample_and_renders_the_same_bits, test_cancel_flag_inside_the_library
    assert lanes(2, n, 64) == 2 and lanes(6, n, 64) == 3 and lanes(6, 20000, 64) == 1 and lanes(4, 256 * 256, 256) == 4
    # tests/test_gpu_lens.py::test_render_lens_is_the_ordered_mean_of_its_rays: the whole 96 x 54 raster at K = 8, "enough for two lanes"
    assert lanes(6, 96 * 54 * 8, 64) == 2 and lanes(1, 96 * 54 * 8, 64) == 1
    # tests/test_gpu_lens_stats.py renders at most 700 positions x 4 and 130 x 33 rays per call: one lane, with or without ACN_LANES=1
    assert lanes(6, 700 * 4, 64) == 1 and lanes(6, 130 * 33, 64) == 1
