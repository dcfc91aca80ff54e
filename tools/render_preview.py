#!/usr/bin/env python3
"""A preview of an Actinon scene from a fraction of its rays: a sparse pass, filled from the rendered neighbours (acn_fill_stats).

    python tools/render_preview.py SCENE OUT.pnm --lattice S [--samples K] [--refine-above T] [--denoise]
                                   [--width W --height H --path-samples P --direct-samples D]

SCENE is an .acn script (the scene of its first create_image) or a flattened scene .npz, as for tools/render_panorama.py.
Everything stays on the device, in this order:
  1  a lens-statistics pass (K jittered samples, closed aperture, seed 0) over every S-th pixel of every S-th row
     (acn_render_lens_stats_dev), merged by index into a zero accumulator (acn_lens_stats_merge_dev);
  2  the FOLLOW surface records of the whole raster (acn_surface_positions_dev);
  3  the fill (acn_fill_stats_dev): the accumulator stays sparse, the filled frame is a buffer of its own;
  4  with --refine-above T: one pass (seed 1) over acn_select_above_dev( need, T ) -- the positions most of whose neighbourhood is of
     other surfaces, and every one the fill could not explain -- merged into the accumulator, which is filled again;
  5  with --denoise: acn_denoise_stats_dev of the filled frame, else its means (acn_lens_stats_resolve_dev, linear);
  6  gamma, saturation and the 8-bit pack (acn_resolve_dev), written as a P6 PNM.
The count of every class after each fill and the rays spent against those of a full frame at the same K are printed."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLASSES = ("rendered", "background", "filled", "unfilled")


def class_counts(d_acc, d_surf, d_need):
    """the positions of every class, from the sparse accumulator, the surface records and the need of its fill (tensors)"""
    import torch
    cnt = d_acc[:, 0]
    empty = ~((cnt >= 1.0) & (cnt < float("inf")))
    background = empty & ~(d_surf[:, 0] < float("inf"))
    unfilled = empty & ~background & torch.isinf(d_need)
    filled = empty & ~background & ~unfilled
    return dict(zip(CLASSES, (int((~empty).sum()), int(background.sum()), int(filled.sum()), int(unfilled.sum()))))


def preview(h, width, height, lattice, samples, refine_above=None, denoise=False, log=print, fill_params=None):
    """-> ( the frame [H,W,3] uint8, the class counts of every fill, rays spent ).  h: an actinon_amd.Handle"""
    import torch
    import actinon_amd as A
    fill_params = dict(fill_params or {})
    n = width * height
    dev = torch.device("cuda", h.device)
    d_acc = torch.zeros((n, A.abi.ACN_STATS_STRIDE), dtype=torch.float64, device=dev)
    d_filled = torch.empty_like(d_acc)
    d_need = torch.empty((n,), dtype=torch.float64, device=dev)
    d_surf = torch.empty((n, A.abi.ACN_SURF_STRIDE), dtype=torch.float64, device=dev)
    d_lin = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    d_all = torch.from_numpy(A.main_pass_positions(width, height)).to(dev)
    ys, xs = np.mgrid[0:height:lattice, 0:width:lattice]
    d_idx = torch.from_numpy((ys * width + xs).reshape(-1).astype(np.int64)).to(dev)
    d_pos = d_all[d_idx].contiguous()
    rays = 0
    counts = []

    def render_pass(d_pos, d_idx, m, seed):
        d_part = torch.empty((m, A.abi.ACN_STATS_STRIDE), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        h.render_lens_stats_dev(d_pos.data_ptr(), m, None, d_part.data_ptr(), linear=True, samples=samples, jitter=True, seed=seed)
        h.lens_stats_merge_dev(d_acc.data_ptr(), n, d_part.data_ptr(), m, d_idx.data_ptr())
        return m * samples

    def fill():
        h.fill_stats_dev(d_acc.data_ptr(), d_surf.data_ptr(), width, height, d_filled.data_ptr(), d_need.data_ptr(), **fill_params)
        counts.append(class_counts(d_acc, d_surf, d_need))
        log("fill %d: " % len(counts) + "  ".join(f"{k} {v}" for k, v in counts[-1].items()))

    rays += render_pass(d_pos, d_idx, int(d_idx.numel()), 0)
    h.surface_positions_dev(d_all.data_ptr(), n, d_surf.data_ptr(), follow=True)
    fill()
    if refine_above is not None:
        d_sel = torch.empty((n,), dtype=torch.int64, device=dev)
        d_sel_pos = torch.empty((n, 2), dtype=torch.float64, device=dev)
        m = h.select_above_dev(d_need.data_ptr(), n, refine_above, n, d_index_ptr=d_sel.data_ptr(), d_pos_ptr=d_sel_pos.data_ptr(),
                               raster_width=width, raster_first=0)
        log(f"refinement: {m} positions above {refine_above}")
        if m:
            rays += render_pass(d_sel_pos[:m], d_sel[:m], m, 1)
            fill()
    if denoise:
        h.denoise_stats_dev(d_filled.data_ptr(), d_surf.data_ptr(), width, height, d_lin.data_ptr())
    else:
        h.lens_stats_resolve_dev(d_filled.data_ptr(), n, d_lin.data_ptr(), None, linear=True)
    h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr())
    log(f"rays: {rays} of the {n * samples} of a full frame at K = {samples} ({rays / (n * samples):.3f})")
    return d_rgb8.cpu().numpy().reshape(height, width, 3), counts, rays


def main(argv=None):
    ap = argparse.ArgumentParser(description="A preview from a sparse pass, filled from the rendered neighbours (acn_fill_stats)")
    ap.add_argument("scene", help=".acn script or flattened scene .npz")
    ap.add_argument("out", help="output image, P6 PNM")
    ap.add_argument("--lattice", type=int, required=True, help="S: every S-th pixel of every S-th row is rendered")
    ap.add_argument("--samples", type=int, default=4, help="K: lens samples per rendered position")
    ap.add_argument("--refine-above", type=float, default=None, help="T >= 0: one more pass over the positions whose need exceeds T")
    ap.add_argument("--denoise", action="store_true", help="filter the filled frame with acn_denoise_stats")
    ap.add_argument("--path-samples", type=int, default=None)
    ap.add_argument("--direct-samples", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    args = ap.parse_args(argv)
    if args.lattice < 1 or args.samples < 1:
        ap.error("--lattice and --samples are at least 1")
    if args.refine_above is not None and not args.refine_above >= 0:
        ap.error("--refine-above takes a threshold >= 0: the need of a rendered position is -1")
    from render_aovs import write_pnm
    from render_panorama import load_scene
    import actinon_amd as A
    flat = load_scene(args.scene)
    prm = flat.params
    for name, value in (("path_samples", args.path_samples), ("direct_samples", args.direct_samples),
                        ("image_width", args.width), ("image_height", args.height)):
        if value is not None:
            if value < 0:
                ap.error("sample counts and sizes are not negative")
            setattr(prm, name, value)
    if prm.image_width < 1 or prm.image_height < 2:
        ap.error("the image needs a width of at least 1 and a height of at least 2")
    h = A.Handle(flat)
    out8, _, _ = preview(h, int(prm.image_width), int(prm.image_height), args.lattice, args.samples, args.refine_above, args.denoise)
    h.close()
    write_pnm(args.out, np.ascontiguousarray(out8))


if __name__ == "__main__":
    main()
