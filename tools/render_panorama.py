#!/usr/bin/env python3
"""Equirectangular 360-degree panorama of an Actinon scene, rendered on the GPU through acn_render_rays.

    python tools/render_panorama.py SCENE OUT.pnm --width W --height H [--origin x,y,z]

SCENE is an .acn script -- the scene of its first create_image, captured through run_script's hook, so the script itself
renders nothing -- or a flattened scene .npz (Flat.save).  The panorama is seen from the scene camera's position or from
--origin; longitude 0 looks along the camera's view direction and latitude rises toward its top direction
(actinon_amd.cameras.panorama_rays).  The image is written as P6 PNM with the reference's 8-bit quantisation (cps_from_cl)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import actinon_amd as A  # noqa: E402
from actinon_amd.cameras import panorama_rays  # noqa: E402


def load_scene(path):
    """The flat scene of a .npz, or of the first create_image of an .acn script."""
    if path.endswith(".npz"):
        return A.Flat.load(path)
    flats = []

    def capture(scene, file):
        if not flats:
            flats.append(scene.flatten())

    A.run_script(path, on_create_image=capture)
    if not flats:
        raise SystemExit(f"{path}: the script creates no image")
    return flats[0]


def main(argv=None):
    ap = argparse.ArgumentParser(description="Equirectangular panorama of an Actinon scene (acn_render_rays)")
    ap.add_argument("scene", help=".acn script or flattened scene .npz")
    ap.add_argument("out", help="output image, P6 PNM")
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--origin", default=None, help="x,y,z (default: the scene camera's position)")
    args = ap.parse_args(argv)
    if args.width < 1 or args.height < 1:
        ap.error("--width and --height must be positive")
    flat = load_scene(args.scene)
    prm = flat.params
    origin = [float(v) for v in args.origin.split(",")] if args.origin else list(prm.camera_position)
    if len(origin) != 3:
        ap.error("--origin takes three numbers: x,y,z")
    rays = panorama_rays(origin, list(prm.camera_view_direction), list(prm.camera_top_direction), args.width, args.height)
    h = A.Handle(flat)
    rgb8 = A.cps_from_cl(h.render_rays(rays))
    h.close()
    with open(args.out, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (args.width, args.height))
        f.write(rgb8.tobytes())


if __name__ == "__main__":
    main()
