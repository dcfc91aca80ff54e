#!/usr/bin/env python3
"""A turntable of an Actinon scene on one handle: one upload, then one acn_scene_set_params per frame.

    python tools/render_turntable.py SCENE OUT_%03d.pnm --frames N --orbit-deg D [--path-samples P --direct-samples D --target-distance T]

SCENE is an .acn script (the scene of its first create_image) or a flattened scene .npz, as for tools/render_panorama.py.  The camera
orbits the scene's view target -- the point camera_view_direction away from the camera, or --target-distance along it -- about the
top direction, --orbit-deg degrees in all, frame 0 at the scene's own camera (actinon_amd.cameras.orbit_camera).  Only the first frame pays
for a handle: the streams, the lanes and what the pipeline learned about the scene's queue demand stay from frame to frame, since a moved
camera does not change the kind of the scene (include/actinon_hip.h: acn_scene_replace).  Each frame is a main pass on the device
(acn_render_main_pass_dev, linear), resolved to 8 bits there (acn_resolve_dev) and written as a P6 PNM to OUT % frame."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def render(flat, frames, orbit_deg, write, target_distance=None):
    """write( frame, rgb8 [H,W,3] uint8 ) for every frame -> the handle's counters after the last (Handle.info)"""
    import torch
    import actinon_amd as A
    from actinon_amd.cameras import orbit_camera
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n = w * hh
    h = A.Handle(flat)
    try:
        dev = torch.device("cuda", h.device)
        d_lin = torch.empty((n, 3), dtype=torch.float64, device=dev)
        d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        for f in range(frames):
            if f:
                h.set_params(**orbit_camera(flat.params, orbit_deg * f / frames, target_distance))
            h.render_main_pass_dev(0, n, d_lin.data_ptr(), linear=True)
            h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr())
            write(f, d_rgb8.cpu().numpy().reshape(hh, w, 3))
        return h.info()
    finally:
        h.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description="A turntable of an Actinon scene on one handle (acn_scene_set_params)")
    ap.add_argument("scene", help=".acn script or flattened scene .npz")
    ap.add_argument("out", help="output images, P6 PNM: a pattern with one integer conversion, e.g. out_%%03d.pnm")
    ap.add_argument("--frames", type=int, required=True)
    ap.add_argument("--orbit-deg", type=float, required=True, help="degrees the camera turns over all frames (360: a full turn)")
    ap.add_argument("--path-samples", type=int, default=None)
    ap.add_argument("--direct-samples", type=int, default=None)
    ap.add_argument("--target-distance", type=float, default=None, help="distance of the view target from the camera (default: the length of camera_view_direction)")
    args = ap.parse_args(argv)
    if args.frames < 1:
        ap.error("--frames is at least 1")
    try:
        if args.out % 0 == args.out % 1:
            raise TypeError
    except TypeError:
        ap.error("OUT needs one integer conversion such as %03d: every frame is a file of its own")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from render_aovs import write_pnm
    from render_panorama import load_scene
    flat = load_scene(args.scene)
    for name, value in (("path_samples", args.path_samples), ("direct_samples", args.direct_samples)):
        if value is not None:
            if value < 0:
                ap.error("sample counts are not negative")
            setattr(flat.params, name, value)
    info = render(flat, args.frames, args.orbit_deg, lambda f, rgb8: write_pnm(args.out % f, np.ascontiguousarray(rgb8)), args.target_distance)
    print(f"{args.frames} frames on one handle: {info['param_sets']} parameter changes, {info['streams']} streams, {info['lanes']} lanes, "
          f"{info['learning_passes']} learning pass(es)")


if __name__ == "__main__":
    main()
