#!/usr/bin/env python3
"""Depth, normal, albedo and object-id images of an Actinon scene: one surface call (acn_surface_positions) over the
main-pass positions.

    python tools/render_aovs.py SCENE OUTDIR [--follow] [--shadow S] [--width W --height H]

SCENE is an .acn script (the scene of its first create_image) or a flattened scene .npz, as for tools/render_panorama.py.
OUTDIR receives
    depth.pfm       distance, one channel of float32, misses as inf (PFM rows run bottom to top)
    normal.pnm      0.5 + 0.5 * normal (the normal that faces the viewer), 8 bit
    albedo.pnm      the surface colour, 8 bit, the reference's quantisation (cps_from_cl)
    object_id.pgm   16 bit, big endian: 1 + the enter object if there is one, else 1 + the exit object; misses 0
    surface.npy     the raw records [ H * W, 16 ] float64 (include/actinon_hip.h)
--follow looks through glass and mirrors: the dominant specular branch to the first diffuse or emitting surface.
--shadow S adds shadow.pfm, the share of the lights each surface point sees (acn_shadow_records with S samples per light: clear /
asked, one channel of float32; misses, emitters and points no sample could ask a light from are 0) and shadow.npy, the raw shadow
records [ H * W, 16 ]."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_pfm(path, img):
    """img [H, W] (Pf) or [H, W, 3] (PF) -> little-endian float32 PFM, rows bottom to top"""
    img = np.asarray(img, dtype=np.float32)
    if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError(f"a PFM image is [H,W] or [H,W,3], got {img.shape}")
    h, w = img.shape[:2]
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n-1.0\n" % (b"PF" if img.ndim == 3 else b"Pf", w, h))
        f.write(np.ascontiguousarray(img[::-1]).astype("<f4").tobytes())


def write_pnm(path, rgb8):
    """rgb8 [H, W, 3] uint8 -> P6"""
    rgb8 = np.asarray(rgb8)
    if rgb8.dtype != np.uint8 or rgb8.ndim != 3 or rgb8.shape[2] != 3:
        raise ValueError("a P6 image is [H,W,3] uint8")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb8.shape[1], rgb8.shape[0]))
        f.write(np.ascontiguousarray(rgb8).tobytes())


def write_pgm16(path, img):
    """img [H, W] of integers in 0 .. 65535 -> P5 with maxval 65535 (big endian)"""
    img = np.asarray(img)
    if img.ndim != 2 or img.min(initial=0) < 0 or img.max(initial=0) > 65535:
        raise ValueError("a 16-bit P5 image is [H,W] with values in 0 .. 65535")
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).astype(">u2").tobytes())


def _header(data, n):
    """n whitespace-separated tokens of a PNM / PFM header and the offset of the raster behind them"""
    tok, i = [], 0
    while len(tok) < n:
        while data[i:i + 1].isspace():
            i += 1
        j = i
        while not data[j:j + 1].isspace():
            j += 1
        tok.append(data[i:j])
        i = j
    return tok, i + 1


def read_pfm(path):
    data = open(path, "rb").read()
    (magic, w, h, scale), off = _header(data, 4)
    ch = {b"PF": 3, b"Pf": 1}[magic]
    w, h = int(w), int(h)
    img = np.frombuffer(data, dtype="<f4" if float(scale) < 0 else ">f4", count=w * h * ch, offset=off)
    img = img.reshape((h, w, 3) if ch == 3 else (h, w))[::-1]
    return img.astype(np.float32)


def read_pnm(path):
    """P6 with maxval 255 -> [H, W, 3] uint8; P5 with maxval 65535 -> [H, W] uint16"""
    data = open(path, "rb").read()
    (magic, w, h, maxval), off = _header(data, 4)
    w, h = int(w), int(h)
    if magic == b"P6" and int(maxval) == 255:
        return np.frombuffer(data, dtype=np.uint8, count=w * h * 3, offset=off).reshape(h, w, 3).copy()
    if magic == b"P5" and int(maxval) == 65535:
        return np.frombuffer(data, dtype=">u2", count=w * h, offset=off).reshape(h, w).astype(np.uint16)
    raise ValueError(f"{path}: {magic!r} with maxval {maxval!r} is not written by this tool")


def aov_images(surface, width, height):
    """depth [H,W] float32, normal [H,W,3] uint8, albedo [H,W,3] uint8, object id [H,W] uint16 of a Surface over H * W records"""
    import actinon_amd as A
    hit = surface.hit
    depth = surface.distance.astype(np.float32).reshape(height, width)
    normal = A.cps_from_cl(np.where(hit[:, None], 0.5 + 0.5 * surface.normal, 0.0)).reshape(height, width, 3)
    albedo = A.cps_from_cl(surface.albedo).reshape(height, width, 3)
    obj = np.where(surface.enter >= 0, surface.enter, surface.exit)
    ids = np.where(hit, obj + 1, 0)
    if ids.max(initial=0) > 65535:
        raise SystemExit("the scene has more than 65535 nodes: object ids do not fit 16 bits")
    return depth, normal, albedo, ids.astype(np.uint16).reshape(height, width)


def write_aovs(outdir, surface, width, height):
    os.makedirs(outdir, exist_ok=True)
    depth, normal, albedo, ids = aov_images(surface, width, height)
    write_pfm(os.path.join(outdir, "depth.pfm"), depth)
    write_pnm(os.path.join(outdir, "normal.pnm"), normal)
    write_pnm(os.path.join(outdir, "albedo.pnm"), albedo)
    write_pgm16(os.path.join(outdir, "object_id.pgm"), ids)
    np.save(os.path.join(outdir, "surface.npy"), surface.raw)


def shadow_image(records, width, height):
    """the share plane [ 5 ] of shadow records over H * W positions -> [H,W] float32"""
    return np.asarray(records, dtype=np.float64).reshape(height * width, 16)[:, 5].astype(np.float32).reshape(height, width)


def write_shadow(outdir, records, width, height):
    os.makedirs(outdir, exist_ok=True)
    write_pfm(os.path.join(outdir, "shadow.pfm"), shadow_image(records, width, height))
    np.save(os.path.join(outdir, "shadow.npy"), np.asarray(records))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Depth, normal, albedo and object-id images of an Actinon scene (acn_surface_positions)")
    ap.add_argument("scene", help=".acn script or flattened scene .npz")
    ap.add_argument("outdir", help="directory for depth.pfm, normal.pnm, albedo.pnm, object_id.pgm, surface.npy")
    ap.add_argument("--follow", action="store_true", help="follow the dominant specular branch to the first diffuse / emitting surface")
    ap.add_argument("--shadow", type=int, default=None, metavar="S", help="also write shadow.pfm: the share of the lights each point sees, S samples per light (1, 2, 4, ... 64)")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    args = ap.parse_args(argv)
    if args.shadow is not None and args.shadow not in (1, 2, 4, 8, 16, 32, 64):
        ap.error("--shadow S: S is 1, 2, 4, 8, 16, 32 or 64")
    import actinon_amd as A
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from render_panorama import load_scene
    flat = load_scene(args.scene)
    prm = flat.params
    if args.width is not None:
        prm.image_width = args.width
    if args.height is not None:
        prm.image_height = args.height
    w, hh = int(prm.image_width), int(prm.image_height)
    if w < 1 or hh < 2:
        ap.error("the image needs a width of at least 1 and a height of at least 2")
    h = A.Handle(flat)
    surface = h.surface_positions(A.main_pass_positions(w, hh), follow=args.follow)
    shadow = h.shadow_records(surface, args.shadow) if args.shadow is not None else None
    h.close()
    write_aovs(args.outdir, surface, w, hh)
    if shadow is not None:
        write_shadow(args.outdir, shadow, w, hh)


if __name__ == "__main__":
    main()
