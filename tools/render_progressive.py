#!/usr/bin/env python3
"""A frame of an Actinon scene rendered in passes that go where the frame is still noisy (acn_render_lens_stats, acn_lens_stats_*).

    python tools/render_progressive.py SCENE OUT.pnm --samples K --passes P --target-noise T [--denoise] [--noise-map FILE]
                                       [--select torch|library] [--rays-per-pass B] [--guides pinhole|lens] [--min-coverage C] [--layers]
                                       [--aperture A --focus D --width W --height H --path-samples P --direct-samples D]

SCENE is an .acn script (the scene of its first create_image) or a flattened scene .npz, as for tools/render_panorama.py.
Pass 0 renders every pixel with K jittered lens samples, seed 0, into an accumulator of per-pixel sample statistics on the device.
Pass p > 0 takes the pixels whose resolved noise -- the standard error of the mean's luminance, relative to that luminance
(include/actinon_hip.h) -- exceeds T, renders only those with seed p and merges their records into the accumulator by index.  The
tool stops after P passes or when no pixel is left, resolves the accumulator (--denoise: acn_denoise_stats first, guided by the
frame's surface records and the measured variance), and writes a P6 PNM.  --noise-map writes the final noise per pixel as a [H,W]
float64 .npy.  Ray counts are printed pass by pass.

--select library takes the pixels of a pass with acn_select_above_dev -- the indices and the pixel centres in one call, as a C host
would -- instead of torch.nonzero and a torch.stack; the passes are the same, bit for bit.  --rays-per-pass B bounds every pass after
the first: the pass takes the histogram of the noise (acn_key_histogram_dev), T_B = acn_key_hist_threshold( hist, B // K ) and selects
above max( T, T_B ), so it casts at most B rays, on the noisiest pixels.  Pixels with one sample have noise +inf and are taken only
by a budget at least as large as their number.

Stopping on the samples' own variance is slightly biased toward dark estimates: a pixel whose first samples happen to come out
dark and alike looks converged and keeps its dark mean, while one whose samples come out bright is refined.  That is why the
policy lives here, in a tool a caller can read and change, and not in the library, which supplies the statistics alone.

--guides says which surface records guide --denoise.  pinhole (the default): the FOLLOW record of the ray through each pixel centre
(acn_surface_positions).  lens: the aggregate FOLLOW record of the K lens rays of pass 0 (acn_surface_lens_main_pass_dev with the
tool's --samples, --aperture, --focus, jitter and seed 0), which at a defocused edge or an anti-aliased silhouette names the surface
most of the pixel's samples met.  --min-coverage C (with lens guides): a pixel whose dominant class holds less than C of its K
samples gets distance inf in its record before the filter, so it is copied through and is never a tap; a pixel of coverage 0.55
still carries 45 % of another surface's radiance, and how much of that a frame tolerates is the caller's decision, like the rest.

--layers keeps the two largest surfaces of every pixel apart through all passes: a pass is acn_render_lens_layers_dev (FOLLOW records)
on the selected pixels, merged into the accumulator's five planes by surface class (acn_lens_layers_merge_dev) by the selection's
index list; the noise that selects is that of the pixel's pooled record (acn_lens_layers_resolve_dev): all its samples as one
population, which is the noise of the tool without --layers to rounding.  With --denoise the end is acn_denoise_layers_dev, which
filters each surface of a mixed pixel with its own neighbours; without it the end is the pooled mean.  The guides are the passes' own
records: --guides and --min-coverage do not apply."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from render_panorama import load_scene  # noqa: E402,F401  (the scene of a script or an .npz)


def select(d_noise, target):
    """the pixels of the next pass: int64 indices, ascending, of the entries of d_noise above target (on d_noise's device)"""
    import torch
    return torch.nonzero(d_noise > target).reshape(-1)


def centres(idx, width):
    """pixel centres [m,2] float64 of pixel indices idx of a raster `width` wide (on idx's device)"""
    import torch
    return torch.stack([(idx % width).to(torch.float64) + 0.5, torch.div(idx, width, rounding_mode="floor").to(torch.float64) + 0.5], dim=1).contiguous()


def sync(dev):
    import torch
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def run_passes(h, width, height, samples, passes, target, dev, lens=None, log=print, *, select_mode="torch", rays_per_pass=None, on_pass=None,
               layers=False):
    """-> the accumulator [n,8] and the noise [n] as tensors on dev, and the rays of every pass.  h: an actinon_amd.Handle.
    layers: every pass is a layered call (FOLLOW records), the accumulator is the pair ( surface planes [2,n,16], statistics planes
    [3,n,8] ), a pass is merged into it by surface class (lens_layers_merge_dev) and the noise is that of the pooled record
    (lens_layers_resolve_dev); the selection is the same.
    select_mode "library": the pixels of a pass come from h.select_above_dev, not from select and centres.  rays_per_pass B: a pass
    after the first selects above max( target, key_hist_threshold( histogram of the noise, B // samples ) ).
    on_pass( p, threshold, idx, d_noise ): called for every pass after the first with its threshold, the selected indices and the noise
    they were selected from (tensors on dev)"""
    import torch
    lens = dict(lens or {})
    n = width * height
    d_acc = torch.zeros((3, n, 8) if layers else (n, 8), dtype=torch.float64, device=dev)
    d_acc_surf = torch.zeros((2, n, 16), dtype=torch.float64, device=dev) if layers else None
    d_noise = torch.empty((n,), dtype=torch.float64, device=dev)

    def resolve_noise():
        if layers:
            h.lens_layers_resolve_dev(d_acc.data_ptr(), n, None, d_noise.data_ptr(), None, linear=True)
        else:
            h.lens_stats_resolve_dev(d_acc.data_ptr(), n, None, d_noise.data_ptr(), linear=True)
    budget = None if rays_per_pass is None else int(rays_per_pass) // samples
    if budget is not None:
        import actinon_amd as A
        d_hist = torch.zeros((A.abi.ACN_KEY_HIST_WORDS,), dtype=torch.int64, device=dev)
    if select_mode == "library":
        room = n if budget is None else min(n, budget)
        d_idx_all = torch.empty((max(room, 1),), dtype=torch.int64, device=dev)
        d_pos_all = torch.empty((max(room, 1), 2), dtype=torch.float64, device=dev)
    sync(dev)
    if layers:
        h.render_lens_layers_main_pass_dev(0, n, None, d_acc_surf.data_ptr(), d_acc.data_ptr(), follow=True, linear=True, samples=samples, seed=0, **lens)
    else:
        h.render_lens_stats_main_pass_dev(0, n, None, d_acc.data_ptr(), linear=True, samples=samples, seed=0, **lens)
    rays = [n * samples]
    log(f"pass 0: {n} pixels, {rays[0]} rays")
    for p in range(1, passes):
        resolve_noise()
        above = target
        if budget is not None:
            h.key_histogram_dev(d_noise.data_ptr(), n, d_hist.data_ptr())
            above = max(target, A.key_hist_threshold(d_hist.cpu().numpy().view(np.uint64), budget))
        if select_mode == "library":
            m = min(h.select_above_dev(d_noise.data_ptr(), n, above, room, d_index_ptr=d_idx_all.data_ptr(), d_pos_ptr=d_pos_all.data_ptr(),
                                       raster_width=width, raster_first=0), room)
            idx, d_pos = d_idx_all[:m], d_pos_all[:m]
        else:
            idx = select(d_noise, above)
            m = int(idx.numel())
        if on_pass is not None:
            on_pass(p, above, idx, d_noise)
        if m == 0:
            log(f"pass {p}: no pixel above {above}")
            break
        if select_mode != "library":
            d_pos = centres(idx, width)
        d_part = torch.empty((3, m, 8) if layers else (m, 8), dtype=torch.float64, device=dev)
        d_part_surf = torch.empty((2, m, 16), dtype=torch.float64, device=dev) if layers else None
        sync(dev)
        if layers:
            h.render_lens_layers_dev(d_pos.data_ptr(), m, None, d_part_surf.data_ptr(), d_part.data_ptr(), follow=True, linear=True, samples=samples,
                                     seed=p, **lens)
            h.lens_layers_merge_dev(d_acc_surf.data_ptr(), d_acc.data_ptr(), n, d_part_surf.data_ptr(), d_part.data_ptr(), m, idx.data_ptr())
        else:
            h.render_lens_stats_dev(d_pos.data_ptr(), m, None, d_part.data_ptr(), linear=True, samples=samples, seed=p, **lens)
            h.lens_stats_merge_dev(d_acc.data_ptr(), n, d_part.data_ptr(), m, idx.data_ptr())
        rays.append(m * samples)
        log(f"pass {p}: {m} pixels, {rays[-1]} rays")
    resolve_noise()
    return ((d_acc_surf, d_acc) if layers else d_acc), d_noise, rays


def render(flat, samples, passes, target, denoise=False, aperture=0.0, focus=0.0, log=print, *, select_mode="torch", rays_per_pass=None,
           on_pass=None, guides="pinhole", min_coverage=0.0, layers=False):
    """-> the frame [H,W,3] uint8, the records [n,8] (layers: the statistics planes [3,n,8]), the noise [H,W] and the rays of every pass"""
    import torch
    import actinon_amd as A
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n = w * hh
    h = A.Handle(flat)
    dev = torch.device("cuda", h.device)
    d_acc, d_noise, rays = run_passes(h, w, hh, samples, passes, target, dev, lens=dict(jitter=True, aperture=aperture, focus=focus), log=log,
                                     select_mode=select_mode, rays_per_pass=rays_per_pass, on_pass=on_pass, layers=layers)
    if layers:
        d_surf, d_acc = d_acc
    d_lin = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    sync(dev)
    if layers and denoise:
        h.denoise_layers_dev(d_acc.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr())
    elif layers:
        h.lens_layers_resolve_dev(d_acc.data_ptr(), n, d_lin.data_ptr(), None, None, linear=True)
    elif denoise:
        d_surf = torch.empty((n, A.abi.ACN_SURF_STRIDE), dtype=torch.float64, device=dev)
        if guides == "lens":
            sync(dev)
            h.surface_lens_main_pass_dev(0, n, d_surf.data_ptr(), follow=True, samples=samples, seed=0, jitter=True, aperture=aperture, focus=focus)
            if min_coverage > 0:
                d_surf[:, 0] = torch.where(d_surf[:, 15] < min_coverage, torch.full_like(d_surf[:, 0], float("inf")), d_surf[:, 0])
                sync(dev)
        else:
            d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
            sync(dev)
            h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr(), follow=True)
        h.denoise_stats_dev(d_acc.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr())
    else:
        h.lens_stats_resolve_dev(d_acc.data_ptr(), n, d_lin.data_ptr(), None, linear=True)
    h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr())
    out = d_rgb8.cpu().numpy().reshape(hh, w, 3), d_acc.cpu().numpy(), d_noise.cpu().numpy().reshape(hh, w), rays
    h.close()
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="A frame rendered in passes that go where it is still noisy (acn_render_lens_stats)")
    ap.add_argument("scene", help=".acn script or flattened scene .npz")
    ap.add_argument("out", help="output image, P6 PNM")
    ap.add_argument("--samples", type=int, required=True, help="K: jittered lens samples per pixel and pass, 1 .. 4096")
    ap.add_argument("--passes", type=int, required=True, help="P: passes at most, the first over the whole raster")
    ap.add_argument("--target-noise", type=float, required=True, help="T: a pixel whose noise exceeds it is sampled again")
    ap.add_argument("--denoise", action="store_true", help="filter the result with acn_denoise_stats before it is resolved")
    ap.add_argument("--noise-map", default=None, metavar="FILE", help="write the final noise per pixel, [H,W] float64 .npy")
    ap.add_argument("--select", choices=("torch", "library"), default="torch",
                    help="how the pixels of a pass are taken: torch.nonzero, or the library's acn_select_above_dev")
    ap.add_argument("--rays-per-pass", type=int, default=None, metavar="B",
                    help="a pass after the first casts at most B rays, on the noisiest pixels (acn_key_histogram_dev)")
    ap.add_argument("--guides", choices=("pinhole", "lens"), default="pinhole",
                    help="the surface records that guide --denoise: of the pixel centres, or the aggregate of the K lens rays (acn_surface_lens)")
    ap.add_argument("--min-coverage", type=float, default=0.0, metavar="C",
                    help="with lens guides: a pixel whose coverage is below C is copied through the filter and is never a tap")
    ap.add_argument("--layers", action="store_true",
                    help="layered passes: the two largest surfaces of a pixel kept apart, merged by class, filtered by acn_denoise_layers")
    ap.add_argument("--aperture", type=float, default=0.0, help="lens radius in scene units (default 0: a pinhole with jitter)")
    ap.add_argument("--focus", type=float, default=0.0, help="distance of the plane in focus, for an open aperture")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--path-samples", type=int, default=None)
    ap.add_argument("--direct-samples", type=int, default=None)
    args = ap.parse_args(argv)
    if not 1 <= args.samples <= 4096:
        ap.error("--samples is 1 .. 4096")
    if args.passes < 1:
        ap.error("--passes is at least 1")
    if not args.target_noise >= 0:
        ap.error("--target-noise is not negative")
    if args.rays_per_pass is not None and args.rays_per_pass < 0:
        ap.error("--rays-per-pass is not negative")
    if not 0 <= args.min_coverage <= 1:
        ap.error("--min-coverage is 0 .. 1")
    if args.layers and (args.guides != "pinhole" or args.min_coverage > 0):
        ap.error("--layers takes its guides from the passes themselves: --guides and --min-coverage do not apply")
    if args.aperture < 0 or (args.aperture > 0 and not args.focus > 0):
        ap.error("the aperture is not negative and the focus distance of an open aperture is positive")
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
    out8, records, noise, rays = render(flat, args.samples, args.passes, args.target_noise, denoise=args.denoise,
                                        aperture=args.aperture, focus=args.focus, select_mode=args.select, rays_per_pass=args.rays_per_pass,
                                        guides=args.guides, min_coverage=args.min_coverage, layers=args.layers)
    write_pnm(args.out, np.ascontiguousarray(out8))
    if args.noise_map:
        with open(args.noise_map, "wb") as f:
            np.save(f, noise)
    pixels = int(prm.image_width) * int(prm.image_height)
    print(f"{args.out}: {prm.image_width}x{prm.image_height}, {len(rays)} passes of {args.samples} samples, {sum(rays)} rays "
          f"({sum(rays) / (args.passes * args.samples * pixels):.3f} of {args.passes} full passes), "
          f"{int((noise > args.target_noise).sum())} pixels still above {args.target_noise}")


if __name__ == "__main__":
    main()
