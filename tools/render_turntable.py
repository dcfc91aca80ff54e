#!/usr/bin/env python3
"""A turntable of an Actinon scene on one handle: one upload, then one acn_scene_set_params per frame.

    python tools/render_turntable.py SCENE OUT_%03d.pnm --frames N --orbit-deg D [--path-samples P --direct-samples D --target-distance T]

SCENE is an .acn script (the scene of its first create_image) or a flattened scene .npz, as for tools/render_panorama.py.  The camera
orbits the scene's view target -- the point camera_view_direction away from the camera, or --target-distance along it -- about the
top direction, --orbit-deg degrees in all, frame 0 at the scene's own camera (actinon_amd.cameras.orbit_camera).  Only the first frame pays
for a handle: the streams, the lanes and what the pipeline learned about the scene's queue demand stay from frame to frame, since a moved
camera does not change the kind of the scene (include/actinon_hip.h: acn_scene_replace).  Each frame is a main pass on the device
(acn_render_main_pass_dev, linear), resolved to 8 bits there (acn_resolve_dev) and written as a P6 PNM to OUT % frame.

    ... --temporal --samples K [--denoise] [--max-history M] [--allow-fresnel]

keeps the samples of the frames before: every frame renders K jittered samples per pixel with their statistics
(acn_render_lens_stats_main_pass_dev, pinhole, seed = frame), fetches for every pixel the statistics accumulated where its surface point
lay in the previous frame (acn_reproject_dev, against the previous frame's first-hit surface records) and pools the two
(acn_lens_stats_merge_dev); --denoise filters the pooled frame with its measured variance (acn_denoise_stats_dev).  History is taken
only where the radiance does not depend on the view direction -- --allow-fresnel also takes it on Fresnel surfaces -- and carries at
most --max-history samples (default 32), so a pixel converges over the frames without lagging behind the camera for long.  The world is
taken to be at rest: only the camera moves (include/actinon_hip.h: acn_reproject).

    ... --spin NODE [--spin-axis x,y,z] [--moved-max-history M]

turns an object instead of the camera: the camera stays, and root element NODE of the scene's matter turns about the axis (default
0,0,1) through its own position, --orbit-deg degrees in all.  Every frame is a copy of the scene with that object turned
(actinon_amd.motion.rigid_copy) made resident by acn_scene_replace.  With --temporal the history comes from acn_reproject_moving_dev
with the motion table of the previous and the current scene (acn_motion_from_scenes): a point of the turned object takes the samples
of where it was one frame ago.  Its shading changes as it turns to the light, and so does that of surfaces its shadow crosses; the
first is not detected, so --moved-max-history (a cap for the object that moved) and --max-history bound how long old samples weigh.

    ... --temporal --shadow-guard [--shadow-samples S] [--shadow-tolerance T] [--shadow-drop]

detects the second: every frame computes shadow records (acn_shadow_records_dev: how much of each light a pixel's surface point sees,
S samples per light, default 16), keeps the previous frame's, and between reproject and merge acn_shadow_limit_history_dev caps the
history at one sample -- or with --shadow-drop takes it away -- wherever that share changed by more than T (default 0.25).  A change
that arrives through a mirror or through glass stays undetected."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spun(flat, spin, degrees):
    """a copy of the scene with the node spin[ 0 ] turned by `degrees` about the axis spin[ 1 ] through its own position"""
    from actinon_amd.motion import rigid_copy, rotation_about
    return rigid_copy(flat, spin[0], rotation_about(spin[1], degrees), pivot=list(flat.node(spin[0]).pos))


def render(flat, frames, orbit_deg, write, target_distance=None, spin=None):
    """write( frame, rgb8 [H,W,3] uint8 ) for every frame -> the handle's counters after the last (Handle.info).  spin: None, or
    ( node index, axis ): that object turns and the camera stays"""
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
            if f and spin:
                h.replace(spun(flat, spin, orbit_deg * f / frames))
            elif f:
                h.set_params(**orbit_camera(flat.params, orbit_deg * f / frames, target_distance))
            h.render_main_pass_dev(0, n, d_lin.data_ptr(), linear=True)
            h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr())
            write(f, d_rgb8.cpu().numpy().reshape(hh, w, 3))
        return h.info()
    finally:
        h.close()


def render_temporal(flat, frames, orbit_deg, write, samples, target_distance=None, denoise=False, max_history=None, allow_fresnel=False,
                    spin=None, moved_max_history=None, shadow_guard=None):
    """The same frames with the history of the frames before them; write( frame, rgb8 ) -> ( Handle.info, per frame the share of pixels
    that took a history and their mean n after the merge, and with shadow_guard the share of the history-carrying pixels it limited ).
    spin: None, or ( node index, axis ): that object turns, the camera stays, and the history goes through the motion table of the two
    scenes.  shadow_guard: None, or dict( samples, tolerance, drop ): shadow records of every frame (acn_shadow_records_dev), the previous
    frame's kept, and acn_shadow_limit_history_dev between reproject and merge"""
    import ctypes as C
    import torch
    import actinon_amd as A
    from actinon_amd import abi
    from actinon_amd.cameras import orbit_camera
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n = w * hh
    params = {}
    if max_history is not None:
        params["max_history"] = max_history
    if allow_fresnel:
        params["reject_kinds"] = abi.ACN_REPROJECT_DEFAULT_REJECT_KINDS & ~abi.ACN_SURF_FRESNEL
    h = A.Handle(flat)
    try:
        dev = torch.device("cuda", h.device)
        new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
        d_surf, d_prev_surf = new(n, abi.ACN_SURF_STRIDE), new(n, abi.ACN_SURF_STRIDE)
        d_cur, d_acc, d_prev = new(n, abi.ACN_STATS_STRIDE), new(n, abi.ACN_STATS_STRIDE), new(n, abi.ACN_STATS_STRIDE)
        d_lin = new(n, 3)
        d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        if shadow_guard:
            d_shadow, d_prev_shadow, d_motion, d_change = new(n, abi.ACN_SHADOW_STRIDE), new(n, abi.ACN_SHADOW_STRIDE), new(n, 2), new(n)
        torch.cuda.synchronize(dev)
        prev_params, prev_flat, report = None, flat, []
        for f in range(frames):
            if f and spin:
                cur_flat = spun(flat, spin, orbit_deg * f / frames)
                h.replace(cur_flat)
            elif f:
                h.set_params(**orbit_camera(flat.params, orbit_deg * f / frames, target_distance))
            h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr())
            h.render_lens_stats_main_pass_dev(0, n, None, d_cur.data_ptr(), linear=True, samples=samples, jitter=True, seed=f)
            if shadow_guard:
                h.shadow_records_dev(d_surf.data_ptr(), n, d_shadow.data_ptr(), samples=shadow_guard["samples"])
            d_out_motion = d_motion.data_ptr() if shadow_guard else None
            if f and spin:
                table, _ = A.motion_from_scenes(prev_flat, cur_flat, moved_max_history)
                d_table = torch.from_numpy(table).to(dev)
                h.reproject_moving_dev(d_surf.data_ptr(), n, prev_params, d_prev_surf.data_ptr(), d_prev.data_ptr(), d_table.data_ptr(), len(table),
                                       d_acc.data_ptr(), d_out_motion, **params)
                prev_flat = cur_flat
            elif f:
                h.reproject_dev(d_surf.data_ptr(), n, prev_params, d_prev_surf.data_ptr(), d_prev.data_ptr(), d_acc.data_ptr(), d_out_motion, **params)
            limited = 0.0
            if f:
                took = float((d_acc[:, 0] >= 1).double().mean())
                if shadow_guard:
                    h.shadow_limit_history_dev(d_acc.data_ptr(), d_motion.data_ptr(), d_shadow.data_ptr(), d_prev_shadow.data_ptr(), n,
                                               int(prev_params.image_width), int(prev_params.image_height), d_change.data_ptr(),
                                               tolerance=shadow_guard["tolerance"], drop=shadow_guard["drop"])
                    tol = abi.ACN_SHADOW_HISTORY_DEFAULT_TOLERANCE if not shadow_guard["tolerance"] else shadow_guard["tolerance"]
                    limited = float((d_change > tol).double().sum()) / max(1.0, took * n)      # (a NaN change compares false)
                h.lens_stats_merge_dev(d_acc.data_ptr(), n, d_cur.data_ptr(), n)
            else:
                took = 0.0
                d_acc.copy_(d_cur)
                torch.cuda.synchronize(dev)
            report.append((took, float(d_acc[:, 0].mean())) + ((limited,) if shadow_guard else ()))
            if denoise:
                h.denoise_stats_dev(d_acc.data_ptr(), d_surf.data_ptr(), w, hh, d_lin.data_ptr())
            else:
                h.lens_stats_resolve_dev(d_acc.data_ptr(), n, d_lin.data_ptr(), None, linear=True)
            h.resolve_dev(d_lin.data_ptr(), n, None, d_rgb8.data_ptr())
            write(f, d_rgb8.cpu().numpy().reshape(hh, w, 3))
            d_surf, d_prev_surf = d_prev_surf, d_surf                          # this frame's records and pooled statistics become "previous"
            d_acc, d_prev = d_prev, d_acc
            if shadow_guard:
                d_shadow, d_prev_shadow = d_prev_shadow, d_shadow
            prev_params = abi.Params()
            C.memmove(C.addressof(prev_params), C.addressof(h.params), C.sizeof(abi.Params))
        return h.info(), report
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
    ap.add_argument("--temporal", action="store_true", help="keep the samples of the frames before: K jittered samples per frame, pooled with the reprojected history")
    ap.add_argument("--samples", type=int, default=None, help="--temporal: samples per pixel and frame")
    ap.add_argument("--denoise", action="store_true", help="--temporal: filter every pooled frame with its measured variance")
    ap.add_argument("--max-history", type=float, default=None, help="--temporal: samples a history carries at most (default 32)")
    ap.add_argument("--allow-fresnel", action="store_true", help="--temporal: take history on Fresnel surfaces too")
    ap.add_argument("--spin", type=int, default=None, metavar="NODE", help="turn root element NODE of the scene's matter instead of the camera, --orbit-deg in all")
    ap.add_argument("--spin-axis", default=None, metavar="x,y,z", help="--spin: the axis through the object's position (default 0,0,1)")
    ap.add_argument("--moved-max-history", type=float, default=None, help="--spin --temporal: samples the history of the turned object carries at most")
    ap.add_argument("--shadow-guard", action="store_true", help="--temporal: limit the history where the light a point sees has changed (acn_shadow_limit_history)")
    ap.add_argument("--shadow-samples", type=int, default=None, metavar="S", help="--shadow-guard: samples per light of the shadow records (default 16)")
    ap.add_argument("--shadow-tolerance", type=float, default=None, metavar="T", help="--shadow-guard: the change of the visible share that limits a history (default 0.25)")
    ap.add_argument("--shadow-drop", action="store_true", help="--shadow-guard: a changed pixel loses its history instead of having it capped at 1")
    args = ap.parse_args(argv)
    if args.frames < 1:
        ap.error("--frames is at least 1")
    if args.shadow_guard and not args.temporal:
        ap.error("--shadow-guard belongs to --temporal")
    if not args.shadow_guard and (args.shadow_samples is not None or args.shadow_tolerance is not None or args.shadow_drop):
        ap.error("--shadow-samples, --shadow-tolerance and --shadow-drop belong to --shadow-guard")
    if args.shadow_samples is not None and args.shadow_samples not in (1, 2, 4, 8, 16, 32, 64):
        ap.error("--shadow-samples is 1, 2, 4, 8, 16, 32 or 64")
    if args.shadow_tolerance is not None and not (0 < args.shadow_tolerance < float("inf")):
        ap.error("--shadow-tolerance is a positive number")
    if args.temporal and (args.samples is None or args.samples < 1):
        ap.error("--temporal needs --samples K, at least 1")
    if not args.temporal and (args.samples is not None or args.denoise or args.max_history is not None or args.allow_fresnel):
        ap.error("--samples, --denoise, --max-history and --allow-fresnel belong to --temporal")
    if args.max_history is not None and not args.max_history >= 1:
        ap.error("--max-history is at least 1")
    if args.spin is None and (args.spin_axis is not None or args.moved_max_history is not None):
        ap.error("--spin-axis and --moved-max-history belong to --spin")
    if args.moved_max_history is not None and not (args.temporal and args.moved_max_history >= 1):
        ap.error("--moved-max-history belongs to --temporal and is at least 1")
    axis = (0.0, 0.0, 1.0)
    if args.spin_axis is not None:
        try:
            axis = tuple(float(v) for v in args.spin_axis.split(","))
        except ValueError:
            axis = ()
        if len(axis) != 3 or not sum(v * v for v in axis) > 0:
            ap.error("--spin-axis is x,y,z with a length")
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
    write = lambda f, rgb8: write_pnm(args.out % f, np.ascontiguousarray(rgb8))
    spin = None
    if args.spin is not None:
        elems = flat.elems_of(flat.c.matter_root)
        if not 0 <= args.spin < len(elems):
            ap.error(f"--spin: the scene's matter has {len(elems)} root elements")
        spin = (elems[args.spin], axis)
    if args.temporal:
        guard = dict(samples=args.shadow_samples or 16, tolerance=args.shadow_tolerance, drop=args.shadow_drop) if args.shadow_guard else None
        info, report = render_temporal(flat, args.frames, args.orbit_deg, write, args.samples, args.target_distance, args.denoise, args.max_history,
                                       args.allow_fresnel, spin, args.moved_max_history, guard)
        for f, row in enumerate(report):
            said = f"frame {f}: {row[0]:.3f} of the pixels took a history, mean n {row[1]:.1f}"
            print(said + (f", the shadow guard limited {row[2]:.4f} of the histories" if guard else ""))
    else:
        info = render(flat, args.frames, args.orbit_deg, write, args.target_distance, spin)
    changes = f"{info['replaces']} scene changes" if spin else f"{info['param_sets']} parameter changes"
    print(f"{args.frames} frames on one handle: {changes}, {info['streams']} streams, {info['lanes']} lanes, "
          f"{info['learning_passes']} learning pass(es)")


if __name__ == "__main__":
    main()
