#!/usr/bin/env python3
"""Times acn_fill_stats_dev and the preview it makes possible, on the wine glass scene at 1920 x 1080, p64 / d200 (DESIGN section 7,
"Filling").

    python scripts/measure_fill.py [--repeats 20] [--width 1920 --height 1080] [--out profiles/r26/fill.json]

One process, one handle.  Every timed call is a device-buffer call on the handle's own stream, which waits for the device: the host
clock around it is the call's time.  Each figure is the median of --repeats calls after two warm-up calls, with its minimum and
maximum; calls that are compared (the fill at lattice 2 and 4, a full frame, acn_denoise_stats_dev with iterations = 1) alternate
inside one loop.
The preview, stage by stage at K = 4 through the lens path (jitter, closed aperture), against the full
acn_render_lens_stats_main_pass_dev frame at the same K; MSE of clip( x, 0, 1 ) against a converged frame: 64 full passes of K = 4 with
seeds of their own, merged."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reference-passes", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import actinon_amd as A
    from render_preview import class_counts
    w, hh, K = args.width, args.height, args.samples
    n = w * hh
    sc = A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=64, direct_samples=200)
    h = A.Handle(sc.flatten())
    dev = torch.device("cuda", h.device)
    f64 = dict(dtype=torch.float64, device=dev)
    d_all = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
    d_surf = torch.empty((n, 16), **f64)
    d_full = torch.empty((n, 8), **f64)
    d_filled = torch.empty((n, 8), **f64)
    d_need = torch.empty((n,), **f64)
    d_lin = torch.empty((n, 3), **f64)
    d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    result = dict(scene="wine_glass", width=w, height=hh, path_samples=64, direct_samples=200, samples=K, repeats=args.repeats,
                  device=torch.cuda.get_device_name(dev))

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def summary(ms):
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls=len(ms))

    def alternate(calls, repeats=args.repeats):
        """calls: name -> function; two warm-up rounds, then `repeats` rounds that run every call once, in order"""
        times = {k: [] for k in calls}
        for r in range(repeats + 2):
            for k, fn in calls.items():
                t = timed(fn)
                if r >= 2:
                    times[k].append(t)
        return {k: summary(v) for k, v in times.items()}

    def lattice(S):
        ys, xs = np.mgrid[0:hh:S, 0:w:S]
        d_idx = torch.from_numpy((ys * w + xs).reshape(-1).astype(np.int64)).to(dev)
        return d_idx, d_all[d_idx].contiguous()

    def sparse_pass(d_acc, d_pos, d_idx, seed, d_part):
        m = int(d_idx.numel())
        h.render_lens_stats_dev(d_pos.data_ptr(), m, None, d_part.data_ptr(), linear=True, samples=K, jitter=True, seed=seed)
        h.lens_stats_merge_dev(d_acc.data_ptr(), n, d_part.data_ptr(), m, d_idx.data_ptr())

    def fill(d_acc):
        h.fill_stats_dev(d_acc.data_ptr(), d_surf.data_ptr(), w, hh, d_filled.data_ptr(), d_need.data_ptr())

    def mse(d_rgb, d_ref):
        return float(((d_rgb.clamp(0, 1) - d_ref.clamp(0, 1)) ** 2).mean())

    # surface records of the raster, and a full frame at K
    result["surface"] = alternate({"surface_positions_dev": lambda: h.surface_positions_dev(d_all.data_ptr(), n, d_surf.data_ptr(), follow=True)}, 5)
    result["full_frame"] = alternate({"render_lens_stats_main_pass_dev": lambda: h.render_lens_stats_main_pass_dev(
        0, n, None, d_full.data_ptr(), linear=True, samples=K, jitter=True, seed=0)}, 3)

    # the sparse accumulators
    acc, sparse = {}, {}
    for S in (2, 4):
        d_idx, d_pos = lattice(S)
        d_part = torch.empty((int(d_idx.numel()), 8), **f64)
        acc[S] = torch.zeros((n, 8), **f64)
        t = []
        for r in range(4):
            acc[S].zero_()
            t.append(timed(lambda: sparse_pass(acc[S], d_pos, d_idx, 0, d_part)))
        sparse[S] = summary(t[1:])
    result["sparse_pass"] = {f"lattice{S}": v for S, v in sparse.items()}

    # the fill at both lattices, the early-out and the yardstick, alternating
    calls = {f"fill_lattice{S}": (lambda S=S: fill(acc[S])) for S in (2, 4)}
    calls["fill_no_empty_record"] = lambda: fill(d_full)
    calls["denoise_stats_iterations1"] = lambda: h.denoise_stats_dev(d_full.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr(), iterations=1)
    calls["denoise_stats_default"] = lambda: h.denoise_stats_dev(d_full.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr())
    result["fill"] = alternate(calls)
    for S in (2, 4):
        fill(acc[S])
        result[f"classes_lattice{S}"] = class_counts(acc[S], d_surf, d_need)

    # the converged frame
    d_ref_acc = d_full.clone()
    d_pass = torch.empty((n, 8), **f64)
    t0 = time.perf_counter()
    for s in range(1, args.reference_passes):
        h.render_lens_stats_main_pass_dev(0, n, None, d_pass.data_ptr(), linear=True, samples=K, jitter=True, seed=100 + s)
        h.lens_stats_merge_dev(d_ref_acc.data_ptr(), n, d_pass.data_ptr(), n, None)
    torch.cuda.synchronize(dev)
    result["reference"] = dict(passes=args.reference_passes, samples_per_pixel=args.reference_passes * K, seconds=time.perf_counter() - t0)
    d_ref = d_ref_acc[:, 1:4].contiguous()
    # (the full frame of seed 0 is one of the reference's 64 passes: its error against the reference is 63/64 of its own)

    # the preview end to end, stage by stage, lattice 2 and 4, with and without refinement
    previews = {}
    for S in (2, 4):
        d_idx, d_pos = lattice(S)
        d_part = torch.empty((int(d_idx.numel()), 8), **f64)
        d_sel = torch.empty((n,), dtype=torch.int64, device=dev)
        d_sel_pos = torch.empty((n, 2), **f64)
        stages = {k: [] for k in ("sparse_pass", "surface", "fill", "select", "refinement_pass", "fill_again", "denoise", "resolve")}
        for r in range(5):
            d_acc = torch.zeros((n, 8), **f64)
            st = {}
            st["sparse_pass"] = timed(lambda: sparse_pass(d_acc, d_pos, d_idx, 0, d_part))
            st["surface"] = timed(lambda: h.surface_positions_dev(d_all.data_ptr(), n, d_surf.data_ptr(), follow=True))
            st["fill"] = timed(lambda: fill(d_acc))
            h.lens_stats_resolve_dev(d_filled.data_ptr(), n, d_lin.data_ptr(), None, linear=True)
            mse_plain = mse(d_lin, d_ref)
            h.denoise_stats_dev(d_filled.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr())
            mse_plain_dn = mse(d_lin, d_ref)
            counts0 = class_counts(d_acc, d_surf, d_need)
            box = {}
            st["select"] = timed(lambda: box.update(m=h.select_above_dev(d_need.data_ptr(), n, 0.5, n, d_index_ptr=d_sel.data_ptr(),
                                                                         d_pos_ptr=d_sel_pos.data_ptr(), raster_width=w, raster_first=0)))
            m = box["m"]
            d_part2 = torch.empty((max(m, 1), 8), **f64)
            st["refinement_pass"] = timed(lambda: (h.render_lens_stats_dev(d_sel_pos.data_ptr(), m, None, d_part2.data_ptr(), linear=True, samples=K,
                                                                           jitter=True, seed=1),
                                                   h.lens_stats_merge_dev(d_acc.data_ptr(), n, d_part2.data_ptr(), m, d_sel.data_ptr())))
            st["fill_again"] = timed(lambda: fill(d_acc))
            counts1 = class_counts(d_acc, d_surf, d_need)
            h.lens_stats_resolve_dev(d_filled.data_ptr(), n, d_lin.data_ptr(), None, linear=True)
            mse_refined = mse(d_lin, d_ref)
            st["denoise"] = timed(lambda: h.denoise_stats_dev(d_filled.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr()))
            mse_refined_dn = mse(d_lin, d_ref)
            st["resolve"] = timed(lambda: h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr()))
            if r >= 1:
                for k, v in st.items():
                    stages[k].append(v)
        rays0, rays1 = int(d_idx.numel()) * K, (int(d_idx.numel()) + m) * K
        previews[f"lattice{S}"] = dict(stages_ms={k: summary(v) for k, v in stages.items()}, refined_positions=m,
                                       rays=dict(preview=rays0, preview_refined=rays1, full=n * K, share=rays0 / (n * K), share_refined=rays1 / (n * K)),
                                       classes=dict(first_fill=counts0, second_fill=counts1),
                                       mse=dict(preview=mse_plain, preview_denoised=mse_plain_dn, preview_refined=mse_refined,
                                                preview_refined_denoised=mse_refined_dn))
    result["preview"] = previews
    h.lens_stats_resolve_dev(d_full.data_ptr(), n, d_lin.data_ptr(), None, linear=True)
    full_mse = mse(d_lin, d_ref)
    h.denoise_stats_dev(d_full.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr())
    result["full_frame_mse"] = dict(raw=full_mse, denoised=mse(d_lin, d_ref))
    h.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
