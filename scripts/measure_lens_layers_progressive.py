#!/usr/bin/env python3
"""What merged layered passes are worth beside one layered call of as many samples.

    python scripts/measure_lens_layers_progressive.py [--passes 4] [--samples 4] [--ref-samples 1024] [--out profiles/r13/lens_layers_progressive.json]

Frame: wine_glass as its script sets it (400 x 400, p500 / d200) through the lens of tools/render_dof.py -- aperture 0.15, focus 12,
jitter --, FOLLOW records: the frame of scripts/measure_lens_layers.py.
  merged   --passes passes of --samples rays per pixel over the whole raster, seeds 0 .. passes - 1, each acn_render_lens_layers_main_pass_dev,
           merged by acn_lens_layers_merge_dev into a zero-filled accumulator -> acn_denoise_layers_dev
  single   one acn_render_lens_layers_main_pass_dev of passes * samples rays per pixel -> acn_denoise_layers_dev, with seeds 0, 1 and 2: the
           spread from seed to seed is what a difference between merged and single has to be read against
both against acn_render_lens_main_pass_dev of --ref-samples rays per pixel and seed 9, unfiltered.  RMSE, linear and after cl_s_sat, over
the pixels whose plane-0 coverage in the single call of seed 0 is below 0.9 and over all pixels; the same for the unfiltered pooled
means.  demoted: the pixels in which the merge sent a class to the rest that one split of all the samples would have kept, as far as
the passes' keys tell: per pixel the eight ( key, n ) of the passes' layers are added up by key, and the pixel counts when the two
largest of those sums hold more samples than the merged layers do.  Prints one JSON line."""
import argparse
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LENS = dict(aperture=0.15, focus=12.0, jitter=True)


def kept_by_one_split(surfs, stats):
    """surfs: per pass [2,n,16], stats: per pass [3,n,8] -> per pixel the samples the two largest classes over all passes hold"""
    import numpy as np
    key, cnt = [], []
    for surf, st in zip(surfs, stats):
        for l in range(2):
            present = (st[l][:, 0] >= 1) & (st[l][:, 0] < np.inf)
            hit = surf[l][:, 0] < np.inf
            code = ((surf[l][:, 7].astype(np.int64) + 2) * 4096 + (surf[l][:, 8].astype(np.int64) + 2)) * 4096 + surf[l][:, 13].astype(np.int64) * 2 + hit
            key.append(np.where(present, code, -1 - len(key)))                # an absent slot: a key of its own, no samples
            cnt.append(np.where(present, st[l][:, 0], 0.0))
    key, cnt = np.stack(key, axis=1), np.stack(cnt, axis=1)
    total = (cnt[:, None, :] * (key[:, None, :] == key[:, :, None])).sum(axis=2)
    first = np.ones(key.shape, bool)
    for s in range(key.shape[1]):
        for t in range(s):
            first[:, s] &= key[:, t] != key[:, s]
    total = np.sort(np.where(first, total, 0.0), axis=1)
    return total[:, -1] + total[:, -2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--ref-samples", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A

    flat = A.Scene.build("wine_glass").flatten()
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n, K, P = w * hh, args.samples, args.passes
    h = A.Handle(flat)
    f64 = dict(dtype=torch.float64, device=torch.device("cuda", h.device))
    d_surf, d_st = torch.zeros((2, n, 16), **f64), torch.zeros((3, n, 8), **f64)
    d_ps, d_pt = torch.empty((2, n, 16), **f64), torch.empty((3, n, 8), **f64)
    d_out, d_raw = torch.empty((n, 3), **f64), torch.empty((n, 3), **f64)
    torch.cuda.synchronize()

    def finish(d_stats, d_surface):
        h.denoise_layers_dev(d_stats.data_ptr(), d_surface.data_ptr(), w, hh, d_out.data_ptr())
        h.lens_layers_resolve_dev(d_stats.data_ptr(), n, d_raw.data_ptr(), None, None, linear=True)
        return d_out.cpu().numpy(), d_raw.cpu().numpy()

    frames, surfs, stats = {}, [], []
    for p in range(P):
        h.render_lens_layers_main_pass_dev(0, n, None, d_ps.data_ptr(), d_pt.data_ptr(), follow=True, linear=True, samples=K, seed=p, **LENS)
        h.lens_layers_merge_dev(d_surf.data_ptr(), d_st.data_ptr(), n, d_ps.data_ptr(), d_pt.data_ptr(), n)
        surfs.append(d_ps.cpu().numpy()); stats.append(d_pt.cpu().numpy())
        print(f"pass {p} merged", file=sys.stderr, flush=True)
    frames["merged"], frames["merged_unfiltered"] = finish(d_st, d_surf)
    merged_st = d_st.cpu().numpy()
    in_layers = merged_st[0][:, 0] + merged_st[1][:, 0]
    demoted = in_layers < kept_by_one_split(surfs, stats)
    cover = None
    single_st = None
    for seed in (0, 1, 2):
        h.render_lens_layers_main_pass_dev(0, n, None, d_ps.data_ptr(), d_pt.data_ptr(), follow=True, linear=True, samples=K * P, seed=seed, **LENS)
        frames[f"single_seed{seed}"], frames[f"single_seed{seed}_unfiltered"] = finish(d_pt, d_ps)
        if seed == 0:
            cover, single_st = d_ps[0, :, 15].cpu().numpy(), d_pt.cpu().numpy()
        print(f"single call, seed {seed}", file=sys.stderr, flush=True)
    res = {"scene": f"wine_glass {w}x{hh} p{flat.params.path_samples} d{flat.params.direct_samples}", "passes": P, "samples_per_pass": K,
           "ref_samples": args.ref_samples, "lens": LENS, "pixels": n, "coverage_below_0.9": int((cover < 0.9).sum()),
           "pixels_with_layer_1": {"merged": int((merged_st[1][:, 0] >= 1).sum()), "single_seed0": int((single_st[1][:, 0] >= 1).sum())},
           "pixels_with_rest": {"merged": int((merged_st[2][:, 0] >= 1).sum()), "single_seed0": int((single_st[2][:, 0] >= 1).sum())},
           "samples_in_rest": {"merged": float(merged_st[2][:, 0].sum()), "single_seed0": float(single_st[2][:, 0].sum())},
           "pixels_demoted_by_the_merge": int(demoted.sum()), "samples_conserved": bool((merged_st[:, :, 0].sum(axis=0) == K * P).all())}
    if args.ref_samples:
        ref = np.empty((n, 3))
        block = 16384
        d_ref = torch.empty((block, 3), **f64)
        for first in range(0, n, block):
            cnt = min(block, n - first)
            h.render_lens_main_pass_dev(first, cnt, d_ref.data_ptr(), linear=True, samples=args.ref_samples, seed=9, **LENS)
            ref[first:first + cnt] = d_ref[:cnt].cpu().numpy()
            print(f"reference: {first + cnt} of {n} pixels", file=sys.stderr, flush=True)
        gamma = float(flat.params.gamma)

        def sat(x):                                                           # cl_s_sat
            with np.errstate(invalid="ignore"):
                return np.clip(np.power(np.maximum(x, 0.0), gamma), 0.0, 1.0)

        for label, mask in (("coverage_below_0.9", cover < 0.9), ("all", np.ones(n, bool))):
            for name, img in frames.items():
                for kind, f in (("linear", lambda x: x), ("saturated", sat)):
                    d = f(img[mask]) - f(ref[mask])
                    res.setdefault("rmse_" + kind, {}).setdefault(label, {})[name] = float(np.sqrt(np.mean(d * d)))
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
