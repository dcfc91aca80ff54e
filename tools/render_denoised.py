#!/usr/bin/env python3
"""A low-sample frame of an Actinon scene, filtered with the guides the library computes exactly (acn_denoise).

    python tools/render_denoised.py SCENE OUT.pnm [--path-samples P --direct-samples D --width W --height H --no-follow --raw RAW.pnm]

SCENE is an .acn script (the scene of its first create_image) or a flattened scene .npz, as for tools/render_panorama.py.
Everything stays on the device: the main pass, linear (acn_render_main_pass_dev); the surface records of the same positions
(acn_surface_positions_dev, ACN_SURF_FOLLOW unless --no-follow); the filter, in place (acn_denoise_dev); gamma, saturation and
the 8-bit pack (acn_resolve_dev).  OUT is a P6 PNM; --raw also writes the unfiltered frame, for comparison.
--path-samples / --direct-samples replace the scene's own: an eighth of them is what the filter is meant for."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def render(flat, follow=True, raw=False, **params):
    """-> the filtered frame [H,W,3] uint8, and the unfiltered one if `raw` (else None)"""
    import torch
    import actinon_amd as A
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n = w * hh
    h = A.Handle(flat)
    dev = torch.device("cuda", h.device)
    d_lin = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_surf = torch.empty((n, A.abi.ACN_SURF_STRIDE), dtype=torch.float64, device=dev)
    d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
    h.render_main_pass_dev(0, n, d_lin.data_ptr(), linear=True)
    h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr(), follow=follow)
    raw8 = None
    if raw:
        h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr())
        raw8 = d_rgb8.cpu().numpy().reshape(hh, w, 3)
    h.denoise_dev(d_lin.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr(), **params)
    h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr())
    out8 = d_rgb8.cpu().numpy().reshape(hh, w, 3)
    h.close()
    return out8, raw8


def main(argv=None):
    ap = argparse.ArgumentParser(description="A low-sample frame of an Actinon scene, filtered (acn_denoise)")
    ap.add_argument("scene", help=".acn script or flattened scene .npz")
    ap.add_argument("out", help="output image, P6 PNM")
    ap.add_argument("--path-samples", type=int, default=None)
    ap.add_argument("--direct-samples", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--no-follow", action="store_true", help="guide with the first surface instead of the one seen through glass and mirrors")
    ap.add_argument("--raw", default=None, help="also write the unfiltered frame here")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from render_aovs import write_pnm
    from render_panorama import load_scene
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
    out8, raw8 = render(flat, follow=not args.no_follow, raw=args.raw is not None)
    write_pnm(args.out, np.ascontiguousarray(out8))
    if args.raw is not None:
        write_pnm(args.raw, np.ascontiguousarray(raw8))


if __name__ == "__main__":
    main()
