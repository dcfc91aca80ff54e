#!/usr/bin/env python3
"""A frame of an Actinon scene through a thin lens: depth of field, and sub-pixel jitter against aliasing (acn_render_lens).

    python tools/render_dof.py SCENE OUT.pnm --aperture A (--focus D | --focus-at X,Y)
                               [--samples K --jitter --layers [--iterations I] --width W --height H --path-samples P --direct-samples D]

SCENE is an .acn script (the scene of its first create_image) or a flattened scene .npz, as for tools/render_panorama.py.
--aperture is the lens radius in scene units (0: a pinhole, and then --jitter alone makes an anti-aliased frame); --focus the
distance of the plane in focus from the camera, measured along the view direction; --focus-at X,Y focuses on what lies under
sample position ( X, Y ) of the frame (Handle.pick), i.e. D = dot( position - camera_position, view direction ).
The frame stays on the device: K lens rays per pixel centre, rendered and averaged in one call (acn_render_lens_main_pass_dev,
linear), then gamma, saturation and the 8-bit pack (acn_resolve_dev).  OUT is a P6 PNM.
--layers renders the layered records of the same rays instead (acn_render_lens_layers_main_pass_dev, FOLLOW records: per pixel the
two largest surfaces its K samples met, each with its own statistics, and the rest) and filters them with acn_denoise_layers before
the resolve: a pixel on a defocused edge is denoised per surface, not as one mixture.  --iterations: the a-trous levels (default 5)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from render_panorama import load_scene  # noqa: E402,F401  (the scene of a script or an .npz)


def focus_depth(prm, position):
    """distance of `position` from the camera along the view direction"""
    view = np.array(prm.camera_view_direction[:], dtype=np.float64)
    view = view / np.sqrt(view @ view)
    return float((np.asarray(position, dtype=np.float64) - np.array(prm.camera_position[:])) @ view)


def render(flat, aperture, focus=None, focus_at=None, samples=None, jitter=False, layers=False, iterations=None):
    """-> the frame [H,W,3] uint8 and the focus distance used"""
    import torch
    import actinon_amd as A
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n = w * hh
    h = A.Handle(flat)
    if focus is None:
        hit = h.pick(*focus_at)
        if hit is None:
            h.close()
            raise ValueError(f"nothing to focus on at sample position {focus_at}")
        focus = focus_depth(flat.params, hit["position"])
    dev = torch.device("cuda", h.device)
    d_lin = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    lens = dict(samples=samples, aperture=aperture, focus=focus, jitter=jitter)
    if layers:
        d_surf = torch.empty((2, n, 16), dtype=torch.float64, device=dev)
        d_stats = torch.empty((3, n, 8), dtype=torch.float64, device=dev)
        h.render_lens_layers_main_pass_dev(0, n, None, d_surf.data_ptr(), d_stats.data_ptr(), follow=True, **lens)
        h.denoise_layers_dev(d_stats.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr(), iterations=iterations)
    else:
        h.render_lens_main_pass_dev(0, n, d_lin.data_ptr(), linear=True, **lens)
    h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr())
    out8 = d_rgb8.cpu().numpy().reshape(hh, w, 3)
    h.close()
    return out8, focus


def parse_args(argv=None):
    def xy(text):
        x, y = (float(v) for v in text.split(","))
        return x, y
    ap = argparse.ArgumentParser(description="A frame of an Actinon scene through a thin lens (acn_render_lens)")
    ap.add_argument("scene", help=".acn script or flattened scene .npz")
    ap.add_argument("out", help="output image, P6 PNM")
    ap.add_argument("--aperture", type=float, required=True, help="lens radius in scene units; 0: pinhole")
    where = ap.add_mutually_exclusive_group(required=True)
    where.add_argument("--focus", type=float, default=None, help="distance of the plane in focus along the view direction")
    where.add_argument("--focus-at", type=xy, default=None, metavar="X,Y", help="focus on what lies under this sample position")
    ap.add_argument("--samples", type=int, default=None, help="lens rays per pixel (default 16)")
    ap.add_argument("--jitter", action="store_true", help="move every sample inside its pixel: anti-aliasing")
    ap.add_argument("--layers", action="store_true", help="render layered records and filter them per surface (acn_denoise_layers)")
    ap.add_argument("--iterations", type=int, default=None, help="a-trous levels of --layers, 1 .. 8 (default 5)")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--path-samples", type=int, default=None)
    ap.add_argument("--direct-samples", type=int, default=None)
    args = ap.parse_args(argv)
    if args.aperture < 0 or (args.focus is not None and args.focus <= 0 and args.aperture > 0):
        ap.error("the aperture is not negative and the focus distance of an open aperture is positive")
    if args.samples is not None and not 1 <= args.samples <= 4096:
        ap.error("--samples is 1 .. 4096")
    if args.iterations is not None and (not args.layers or not 1 <= args.iterations <= 8):
        ap.error("--iterations is 1 .. 8 and belongs to --layers")
    for value in (args.width, args.height, args.path_samples, args.direct_samples):
        if value is not None and value < 0:
            ap.error("sample counts and sizes are not negative")
    return args


def main(argv=None):
    args = parse_args(argv)
    from render_aovs import write_pnm
    flat = load_scene(args.scene)
    prm = flat.params
    for name, value in (("path_samples", args.path_samples), ("direct_samples", args.direct_samples),
                        ("image_width", args.width), ("image_height", args.height)):
        if value is not None:
            setattr(prm, name, value)
    if prm.image_width < 1 or prm.image_height < 2:
        sys.exit("the image needs a width of at least 1 and a height of at least 2")
    out8, focus = render(flat, args.aperture, focus=args.focus, focus_at=args.focus_at, samples=args.samples, jitter=args.jitter,
                         layers=args.layers, iterations=args.iterations)
    write_pnm(args.out, np.ascontiguousarray(out8))
    print(f"{args.out}: {prm.image_width}x{prm.image_height}, {args.samples or 16} lens rays per pixel, aperture {args.aperture}, "
          f"plane in focus at {focus:.6g}" + (", filtered per layer" if args.layers else ""))


if __name__ == "__main__":
    main()
