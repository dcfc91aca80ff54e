"""Python face of the host-side scene model (libactinon_host.so) and of the render seam (libactinon_hip.so).

Everything here is plumbing over the C ABI: scene assembly happens in C (actinon_amd/host/*.c), rendering in the
HIP library.  Mirrors, for this path, what the reference's script interpreter does with scene_s
(/root/reference/src/scene.c:293-331): set fields, push objects, create_image."""
import ctypes as C

import numpy as np

from . import abi
from ._lib import hip, host, check, AcnError


def v3(x, y=None, z=None):
    if y is None:
        x, y, z = x
    return abi.V3(float(x), float(y), float(z))


class Flat:
    """An acn_flat_scene owned by Python (arrays allocated by libactinon_host, freed on __del__)."""

    def __init__(self):
        self.c = abi.FlatScene()
        self._owned = False

    def __del__(self):
        if getattr(self, "_owned", False):
            host.acn_flat_scene_free(C.byref(self.c))
            self._owned = False

    @property
    def n_nodes(self):
        return self.c.n_nodes

    @property
    def params(self):
        return self.c.params

    def node(self, i):
        return self.c.nodes[i]

    def elems_of(self, compound_index):
        n = self.c.nodes[compound_index]
        return [self.c.elems[n.child0 + k] for k in range(n.child1)]

    def nodes_bytes(self):
        return C.string_at(self.c.nodes, C.sizeof(abi.Node) * self.c.n_nodes)

    def save(self, path, driver=(0.1, 10, 1)):
        """Writes the flat scene as a compressed .npz (nodes / elems / params / textures as raw ABI bytes)."""
        tex = C.string_at(self.c.textures, C.sizeof(abi.Texture) * self.c.n_textures) if self.c.n_textures else b""
        np.savez_compressed(
            path, abi_version=self.c.abi_version, nodes=np.frombuffer(self.nodes_bytes(), dtype=np.uint8),
            elems=np.array(self.c.elems[:self.c.n_elems], dtype=np.int32),
            params=np.frombuffer(C.string_at(C.addressof(self.c.params), C.sizeof(abi.Params)), dtype=np.uint8),
            textures=np.frombuffer(tex, dtype=np.uint8),
            roots=np.array([self.c.light_root, self.c.matter_root], dtype=np.int32), driver=np.array(driver, dtype=np.float64))

    @classmethod
    def load(cls, path, **overrides):
        """Inverse of save(); arrays are owned by Python.  overrides set acn_params fields."""
        z = np.load(path)
        if int(z["abi_version"]) != abi.ACN_ABI_VERSION:
            raise AcnError(abi.ACN_ERR_ARG, f"{path}: flat scene of ABI {int(z['abi_version'])}, library is {abi.ACN_ABI_VERSION}")
        f = cls()
        nb = z["nodes"].tobytes()
        n = len(nb) // C.sizeof(abi.Node)
        f._nodes = (abi.Node * max(1, n)).from_buffer_copy(nb.ljust(C.sizeof(abi.Node), b"\0"))
        el = z["elems"].astype(np.int32)
        f._elems = (C.c_int32 * max(1, len(el)))(*[int(v) for v in el])
        tb = z["textures"].tobytes() if "textures" in z.files else b""
        nt = len(tb) // C.sizeof(abi.Texture)
        f._tex = (abi.Texture * max(1, nt)).from_buffer_copy(tb.ljust(C.sizeof(abi.Texture), b"\0"))
        f.c.abi_version = abi.ACN_ABI_VERSION
        f.c.n_nodes, f.c.n_elems, f.c.n_textures = n, len(el), nt
        f.c.light_root, f.c.matter_root = int(z["roots"][0]), int(z["roots"][1])
        f.c.nodes = C.cast(f._nodes, C.POINTER(abi.Node))
        f.c.elems = C.cast(f._elems, C.POINTER(C.c_int32))
        f.c.textures = C.cast(f._tex, C.POINTER(abi.Texture))
        C.memmove(C.addressof(f.c.params), z["params"].tobytes(), C.sizeof(abi.Params))
        f.driver = tuple(float(v) for v in z["driver"]) if "driver" in z.files else (0.1, 10, 1)
        for k, v in overrides.items():
            cur = getattr(f.c.params, k)
            if hasattr(cur, "__len__"):
                for i in range(len(cur)):
                    cur[i] = float(v[i])
            else:
                setattr(f.c.params, k, v)
        return f


class Scene:
    """Wraps an acn_scene* (scene_s counterpart)."""

    BUILDERS = {"primitives": "acn_scene_primitives", "wine_glass": "acn_scene_wine_glass",
                "diamond": "acn_scene_diamond"}

    def __init__(self, ptr=None):
        if ptr is None:
            ptr = C.cast(host.acn_scene_s_create(), C.c_void_p).value
        if not ptr:
            raise AcnError(abi.ACN_ERR_ARG, "scene construction failed")
        self.ptr = ptr
        self.s = C.cast(ptr, C.POINTER(abi.SceneStruct)).contents

    def __del__(self):
        if getattr(self, "ptr", None):
            host.acn_scene_s_discard(self.ptr)
            self.ptr = None

    @classmethod
    def build(cls, name, **overrides):
        """name: primitives | wine_glass | diamond | many_spheres[:levels[:exact]]; overrides set acn_params fields."""
        if name.startswith("many_spheres"):
            parts = name.split(":")
            levels = int(parts[1]) if len(parts) > 1 else 5
            exact = int(parts[2]) if len(parts) > 2 else 0
            ptr = host.acn_scene_many_spheres(levels, exact)
        else:
            ptr = getattr(host, cls.BUILDERS[name])()
        sc = cls(ptr)
        sc.set(**overrides)
        return sc

    AUTOENV_GPU, AUTOENV_SKIP = 0, 1

    @classmethod
    def from_script(cls, path, auto_envelope=0, **overrides):
        """Interprets an .acn script (include/acn_interp.h) without rendering; returns the scene as it was at the
        script's first create_image call."""
        ptr = host.acn_scene_from_script(str(path).encode(), auto_envelope)
        if not ptr:
            raise AcnError(abi.ACN_ERR_ARG, host.acn_interp_last_error().decode())
        sc = cls(ptr)
        sc.set(**overrides)
        return sc

    def set(self, **kw):
        for k, v in kw.items():
            if hasattr(self.s.prm, k):
                cur = getattr(self.s.prm, k)
                if hasattr(cur, "__len__"):
                    for i in range(len(cur)):
                        cur[i] = float(v[i])
                else:
                    setattr(self.s.prm, k, v)
            elif hasattr(self.s, k):
                setattr(self.s, k, v)
            else:
                raise AttributeError(f"scene_s has no member '{k}'")
        return self

    @property
    def prm(self):
        return self.s.prm

    def objects(self):
        return host.acn_scene_s_objects(self.ptr)

    def clear(self):
        host.acn_scene_s_clear(self.ptr)

    def push(self, obj_ptr):
        return host.acn_scene_s_push(self.ptr, obj_ptr)

    def flatten(self):
        f = Flat()
        check(host.acn_scene_s_flatten(self.ptr or self._borrowed, C.byref(f.c)), "acn_scene_s_flatten")
        f._owned = True
        return f

    def create_image_file(self, path, overwrite=True, keep=None):
        """Renders the scene and writes the PNM (acn_scene_s_create_image_file).  keep: a KeptHandle that holds one handle over many
        images -- of this scene as it changes, or of other scenes; the caller closes it after the last image."""
        C.c_int.in_dll(host, "acn_scene_s_overwrite_output_files_g").value = 1 if overwrite else 0
        ptr = self.ptr or self._borrowed
        if keep is None:
            check(host.acn_scene_s_create_image_file(ptr, path.encode()), "acn_scene_s_create_image_file")
        else:
            check(host.acn_scene_s_create_image_file_keep(ptr, path.encode(), C.byref(keep.h)), "acn_scene_s_create_image_file_keep")


class KeptHandle:
    """The handle Scene.create_image_file( keep=... ) renders on: uploaded by the first image, its scene replaced by every later one."""

    def __init__(self):
        self.h = C.c_void_p()

    def info(self):
        return Handle.info(self)

    def close(self):
        if self.h.value:
            hip.acn_scene_free(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def set_host_cycles(on):
    """The render driver's gradient cycles on host arrays (True) or on a device-resident frame (False): acn_scene_s_host_cycles_g.
    Returns what it was."""
    g = C.c_int.in_dll(host, "acn_scene_s_host_cycles_g")
    was = bool(g.value)
    g.value = 1 if on else 0
    return was


def run_script(path, on_create_image=None, auto_envelope=0, readonly_fs=False, args=(), overwrite=True, host_cycles=None):
    """Interprets an .acn script (acn_interpret_file).  on_create_image( scene: Scene, file: str ) -> None replaces
    the render driver for `scene.create_image( file )`; None renders on the GPU and writes the PNM like the
    reference's actinon binary does.  host_cycles: None leaves the driver as it is set, True / False selects its loop on host
    arrays / on a device-resident frame for this script."""
    from ._lib import InterpOpts, CREATE_IMAGE_FN
    C.c_int.in_dll(host, "acn_scene_s_overwrite_output_files_g").value = 1 if overwrite else 0
    if host_cycles is not None:
        was = set_host_cycles(host_cycles)
        try:
            return run_script(path, on_create_image, auto_envelope, readonly_fs, args, overwrite)
        finally:
            set_host_cycles(was)
    raised = []

    def hook(ctx, scene_ptr, file):
        try:
            view = Scene.__new__(Scene)
            view.ptr = None                      # borrowed: the interpreter owns the scene
            view.s = C.cast(scene_ptr, C.POINTER(abi.SceneStruct)).contents
            view._borrowed = scene_ptr
            on_create_image(view, file.decode())
            return abi.ACN_OK
        except Exception as ex:                  # noqa: BLE001 - surfaced after the C call returns
            raised.append(ex)
            return abi.ACN_ERR_ARG

    opts = InterpOpts()
    cb = CREATE_IMAGE_FN(hook) if on_create_image else CREATE_IMAGE_FN()
    opts.on_create_image = cb
    opts.auto_envelope = auto_envelope
    opts.readonly_fs = 1 if readonly_fs else 0
    argv = (C.c_char_p * max(1, len(args)))(*[a.encode() for a in args])
    opts.argc = len(args)
    opts.argv = argv
    st = host.acn_interpret_file(str(path).encode(), C.byref(opts))
    if raised:
        raise raised[0]
    if st != abi.ACN_OK:
        raise AcnError(st, host.acn_interp_last_error().decode())


class Handle:
    """A flattened scene resident on one GPU (acn_scene_handle)."""

    def __init__(self, flat, device=0, count_work=False):
        self.flat = flat
        self.device = device
        self.count_work = count_work   # instrumented kernels: last_counters() is only meaningful when set
        self.stage_timing = False      # per-launch HIP events: last_stages() then carries walk / shade / hard ms
        self.cancel = None             # optional ctypes.c_int polled by the library (acn_render_opts.cancel)
        self.sample_shard = None       # (rank, world): ACN_SHARD_SAMPLES for the following render calls (linear output)
        self.h = C.c_void_p()
        check(hip.acn_scene_upload(C.byref(flat.c), device, C.byref(self.h)), "acn_scene_upload")

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            hip.acn_scene_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        self.close()

    # the scene of a live handle changes (acn_scene_replace, acn_scene_set_params): streams, lanes and queues stay
    @property
    def params(self):
        """The render parameters the handle renders with now: a copy (abi.Params) of the flat scene's, as set_params left them."""
        if getattr(self, "_params", None) is None:
            p = abi.Params()
            C.memmove(C.addressof(p), C.addressof(self.flat.c.params), C.sizeof(abi.Params))
            self._params = p
        return self._params

    def replace(self, flat, forget=False):
        """Makes `flat` the resident scene (acn_scene_replace); self.flat follows.  What the handle learned about its queue demand
        stays if the scene is of the kind it was (include/actinon_hip.h), unless forget.  A refused scene raises and changes nothing."""
        check(hip.acn_scene_replace(self.h, C.byref(flat.c), abi.ACN_REPLACE_FORGET if forget else 0), "acn_scene_replace")
        self.flat = flat
        self._params = None

    def set_params(self, **fields):
        """Changes members of the acn_params the handle renders with (acn_scene_set_params): camera, raster, samples, depth.
        self.params follows; self.flat is the caller's and stays as it is."""
        p = abi.Params()
        C.memmove(C.addressof(p), C.addressof(self.params), C.sizeof(abi.Params))
        for k, v in fields.items():
            cur = getattr(p, k)
            if hasattr(cur, "__len__"):
                for i in range(len(cur)):
                    cur[i] = float(v[i])
            else:
                setattr(p, k, v)
        check(hip.acn_scene_set_params(self.h, C.byref(p)), "acn_scene_set_params")
        self._params = p

    INFO = ["replaces", "param_sets", "streams", "lanes", "learning_passes", "nodes", "rates_known", "device"]

    def info(self):
        """Counters of the handle since its upload (acn_scene_info): how a caller sees that it stayed warm."""
        buf = (C.c_uint64 * abi.ACN_INFO_N)()
        check(hip.acn_scene_info(self.h, buf, abi.ACN_INFO_N), "acn_scene_info")
        return dict(zip(Handle.INFO, [int(v) for v in buf]))

    def _opts(self, linear, stream):
        o = abi.RenderOpts()
        o.struct_size = C.sizeof(abi.RenderOpts)
        o.flags = ((abi.ACN_OPT_LINEAR_OUT if linear else 0) | (abi.ACN_OPT_COUNT_WORK if self.count_work else 0)
                   | (abi.ACN_OPT_STAGE_TIMING if self.stage_timing else 0))
        o.stream = stream
        if self.cancel is not None:
            o.cancel = C.pointer(self.cancel)
        if self.sample_shard is not None:
            o.shard_mode = abi.ACN_SHARD_SAMPLES
            o.shard_rank, o.shard_world = self.sample_shard
        return o

    def render_positions(self, pos_xy, linear=False):
        """lum_machine_s_run on host arrays: pos_xy [n,2] float64 -> rgb [n,3] float64."""
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((pos.shape[0], 3), dtype=np.float64)
        o = self._opts(linear, None)
        check(hip.acn_render_positions(self.h, pos.ctypes.data, pos.shape[0], out.ctypes.data, C.byref(o)),
              "acn_render_positions")
        return out

    def render_positions_dev(self, d_pos_ptr, n, d_out_ptr, linear=False, stream=None):
        o = self._opts(linear, stream)
        check(hip.acn_render_positions_dev(self.h, d_pos_ptr, n, d_out_ptr, C.byref(o)), "acn_render_positions_dev")

    def render_main_pass_dev(self, first, count, d_out_ptr, linear=False, stream=None):
        o = self._opts(linear, stream)
        check(hip.acn_render_main_pass_dev(self.h, first, count, d_out_ptr, C.byref(o)), "acn_render_main_pass_dev")

    def render_rays(self, rays, linear=False):
        """Radiance of caller-supplied rays (acn_render_rays): rays [n,6] float64 origin, direction -> rgb [n,3] float64."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.empty((r.shape[0], 3), dtype=np.float64)
        o = self._opts(linear, None)
        check(hip.acn_render_rays(self.h, r.ctypes.data, r.shape[0], out.ctypes.data, C.byref(o)), "acn_render_rays")
        return out

    def render_rays_dev(self, d_rays_ptr, n, d_out_ptr, linear=False, stream=None):
        o = self._opts(linear, stream)
        check(hip.acn_render_rays_dev(self.h, d_rays_ptr, n, d_out_ptr, C.byref(o)), "acn_render_rays_dev")

    def camera_rays(self, pos_xy):
        """The rays the pipeline casts for sample positions (acn_camera_rays): pos_xy [n,2] -> [n,6] origin, direction."""
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((pos.shape[0], 6), dtype=np.float64)
        check(hip.acn_camera_rays(self.h, pos.ctypes.data, pos.shape[0], out.ctypes.data), "acn_camera_rays")
        return out

    def camera_rays_dev(self, d_pos_ptr, n, d_out_ptr, stream=None):
        o = self._opts(False, stream)
        check(hip.acn_camera_rays_dev(self.h, d_pos_ptr, n, d_out_ptr, C.byref(o)), "acn_camera_rays_dev")

    def render_main_pass_shard_dev(self, first, count, rank, world, d_part_ptr, linear=True, stream=None):
        """This rank's tiles of the main pass (acn_shard_tile_*), into a part of acn_shard_tile_padded(count, world) rows."""
        o = self._opts(linear, stream)
        check(hip.acn_render_main_pass_shard_dev(self.h, first, count, rank, world, d_part_ptr, C.byref(o)),
              "acn_render_main_pass_shard_dev")

    def shard_unpack_dev(self, d_gathered_ptr, count, world, d_frame_ptr, stream=None):
        o = self._opts(True, stream)
        check(hip.acn_shard_unpack_dev(self.h, d_gathered_ptr, count, world, d_frame_ptr, C.byref(o)), "acn_shard_unpack_dev")

    def resolve_dev(self, d_linear_ptr, n, d_out_rgb_ptr=None, d_out_rgb8_ptr=None, stream=None):
        """cl_s_sat + 8-bit pack on a device-resident linear radiance buffer (after accumulation / all-reduce)."""
        o = self._opts(False, stream)
        check(hip.acn_resolve_dev(self.h, d_linear_ptr, n, d_out_rgb_ptr, d_out_rgb8_ptr, C.byref(o)), "acn_resolve_dev")

    def last_kernel_ms(self):
        ms = C.c_double()
        check(hip.acn_last_kernel_ms(self.h, C.byref(ms)), "acn_last_kernel_ms")
        return ms.value

    # the slots of acn_last_stage_ms, in order: the ACN_LAST_* enum of include/actinon_hip.h
    STAGES = ["walk_ms", "shade_ms", "finalize_ms", "total_ms", "walk_launches", "shade_launches", "finalize_launches",
              "chunks", "retries", "levels", "peak_tasks", "peak_children", "queue_cap", "hard_ms", "hard_launches",
              "hard_rays", "walk_rays", "path_hits", "host_syncs", "walk_steps", "flags", "private_rays", "probe_rays",
              "workspace_bytes", "workspace_allocs"]

    def last_stages(self):
        """Per-stage device time (ms) and pipeline statistics of the last render call."""
        buf = (C.c_double * len(self.STAGES))()
        check(hip.acn_last_stage_ms(self.h, buf, len(self.STAGES)), "acn_last_stage_ms")
        return dict(zip(self.STAGES, [float(v) for v in buf]))

    COUNTERS = ["trans_rays", "shadow_rays", "obj_hits", "lum_calls", "cap_samples", "side_calls", "sdf_evals",
                "overflows", "flop", "transcendentals"]

    def last_counters(self):
        buf = (C.c_uint64 * 10)()
        check(hip.acn_last_counters(self.h, buf, 10), "acn_last_counters")
        return dict(zip(self.COUNTERS, [int(v) for v in buf]))

    def stage_last_counters(self):
        """The work counters of the last stage call (run_stage / run_stage_walk with count_work), named as last_counters names them."""
        buf = (C.c_uint64 * 10)()
        check(hip.acn_stage_last_counters(self.h, buf, 10), "acn_stage_last_counters")
        return dict(zip(self.COUNTERS, [int(v) for v in buf]))

    PHASES = ["other", "light", "root_leaf", "prune", "m_leaf", "m_pair", "m_frame", "m_side", "shade", "compound", "fetch",
              "tail", "light_setup", "path_setup"]   # the last two: k_shade alone (machine tallies in the other kernels' slots)

    def last_counters_raw(self, n):
        buf = (C.c_uint64 * n)()
        check(hip.acn_last_counters(self.h, buf, n), "acn_last_counters")
        return [int(v) for v in buf]

    def last_phase_ticks(self):
        """{kernel: {phase: shader-clock ticks}} of a library built with -DACN_PHASE_TIMERS (all zero otherwise)"""
        buf = (C.c_uint64 * 74)()
        check(hip.acn_last_counters(self.h, buf, 74), "acn_last_counters")
        out = {}
        for k, kernel in enumerate(["walk", "hard_shadow", "hard_path", "shade"]):
            out[kernel] = {p: int(buf[10 + 16 * k + i]) for i, p in enumerate(self.PHASES)}
        return out

    def estimate_envelope(self, node, samples=1000, rseed=123, radius_factor=1.1):
        out = (C.c_double * 4)()
        check(hip.acn_estimate_envelope(self.h, node, samples, rseed, radius_factor, out), "acn_estimate_envelope")
        return list(out)


    # surface records (acn_surface_*): what a ray meets instead of the radiance it carries
    def _surface_mode(self, follow):
        return abi.ACN_SURF_FOLLOW if follow else abi.ACN_SURF_FIRST_HIT

    def surface_rays(self, rays, follow=False):
        """The surface each ray meets (acn_surface_rays): rays [n,6] float64 origin, direction -> Surface over [n,16].
        follow=True follows the dominant specular branch to the first diffuse or emitting surface."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.empty((r.shape[0], abi.ACN_SURF_STRIDE), dtype=np.float64)
        o = self._opts(False, None)
        o.shard_mode, o.shard_rank, o.shard_world = abi.ACN_SHARD_NONE, 0, 0
        check(hip.acn_surface_rays(self.h, r.ctypes.data, r.shape[0], self._surface_mode(follow), out.ctypes.data, C.byref(o)),
              "acn_surface_rays")
        return Surface(out)

    def surface_positions(self, pos_xy, follow=False):
        """The same for sample positions, through the camera (acn_surface_positions): pos_xy [n,2] -> Surface."""
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((pos.shape[0], abi.ACN_SURF_STRIDE), dtype=np.float64)
        o = self._opts(False, None)
        o.shard_mode, o.shard_rank, o.shard_world = abi.ACN_SHARD_NONE, 0, 0
        check(hip.acn_surface_positions(self.h, pos.ctypes.data, pos.shape[0], self._surface_mode(follow), out.ctypes.data,
                                        C.byref(o)), "acn_surface_positions")
        return Surface(out)

    def surface_rays_dev(self, d_rays_ptr, n, d_out_ptr, follow=False, stream=None):
        """Device buffers: d_out [n,16] float64, 128-byte aligned; enqueued on `stream` (None: synchronous)."""
        o = self._opts(False, stream)
        o.shard_mode, o.shard_rank, o.shard_world = abi.ACN_SHARD_NONE, 0, 0
        check(hip.acn_surface_rays_dev(self.h, d_rays_ptr, n, self._surface_mode(follow), d_out_ptr, C.byref(o)),
              "acn_surface_rays_dev")

    def surface_positions_dev(self, d_pos_ptr, n, d_out_ptr, follow=False, stream=None):
        o = self._opts(False, stream)
        o.shard_mode, o.shard_rank, o.shard_world = abi.ACN_SHARD_NONE, 0, 0
        check(hip.acn_surface_positions_dev(self.h, d_pos_ptr, n, self._surface_mode(follow), d_out_ptr, C.byref(o)),
              "acn_surface_positions_dev")

    # the edge-avoiding filter (acn_denoise): a low-sample linear frame and its surface records -> a filtered linear frame
    @staticmethod
    def denoise_params(iterations=None, normal_power_log2=None, demodulate=True, sigma_plane=None, sigma_lum=None):
        """acn_denoise_params of keyword arguments; None is the library's default"""
        p = abi.DenoiseParams()
        p.struct_size = C.sizeof(abi.DenoiseParams)
        p.iterations = 0 if iterations is None else int(iterations)
        if normal_power_log2 is not None:
            p.normal_power_log2 = int(normal_power_log2)
            p.flags |= abi.ACN_DENOISE_NORMAL_POWER_SET
        if not demodulate:
            p.flags |= abi.ACN_DENOISE_NO_DEMODULATE
        p.sigma_plane = 0.0 if sigma_plane is None else float(sigma_plane)
        p.sigma_lum = 0.0 if sigma_lum is None else float(sigma_lum)
        return p

    def denoise(self, linear, surface, **params):
        """Filters a linear frame (acn_denoise): linear [h,w,3] float64 as render_*(linear=True) gives it, surface the Surface
        (or its [h*w,16] records) of the same positions, FOLLOW recommended -> [h,w,3] float64, linear.  params: iterations,
        normal_power_log2, demodulate, sigma_plane, sigma_lum (Handle.denoise_params)."""
        lin = np.ascontiguousarray(linear, dtype=np.float64)
        if lin.ndim != 3 or lin.shape[2] != 3:
            raise ValueError(f"a frame to denoise is [h,w,3], got {lin.shape}")
        hh, w = lin.shape[:2]
        raw = np.ascontiguousarray(surface.raw if isinstance(surface, Surface) else surface, dtype=np.float64)
        if raw.size != hh * w * abi.ACN_SURF_STRIDE:
            raise ValueError(f"{hh}x{w} pixels need {hh * w} surface records of {abi.ACN_SURF_STRIDE}, got {raw.shape}")
        out = np.empty_like(lin)
        p = self.denoise_params(**params)
        o = self._opts(False, None)
        o.shard_mode, o.shard_rank, o.shard_world = abi.ACN_SHARD_NONE, 0, 0
        check(hip.acn_denoise(self.h, lin.ctypes.data, raw.ctypes.data, w, hh, C.byref(p), out.ctypes.data, C.byref(o)), "acn_denoise")
        return out

    def denoise_dev(self, d_linear_ptr, d_surface_ptr, width, height, d_out_ptr, stream=None, **params):
        """Device buffers: d_linear, d_out [h*w,3] float64 (they may be the same), d_surface [h*w,16] float64; enqueued on
        `stream` without a synchronisation (None: the handle's stream, synchronous)."""
        p = self.denoise_params(**params)
        o = self._opts(False, stream)
        o.shard_mode, o.shard_rank, o.shard_world = abi.ACN_SHARD_NONE, 0, 0
        check(hip.acn_denoise_dev(self.h, d_linear_ptr, d_surface_ptr, width, height, C.byref(p), d_out_ptr, C.byref(o)), "acn_denoise_dev")

    # the thin-lens camera (acn_lens_rays, acn_render_lens): K rays per sample position, averaged on the device
    @staticmethod
    def lens_params(samples=None, aperture=0.0, focus=0.0, jitter=False, seed=0):
        """acn_lens_params of keyword arguments; samples=None is the library's default (16)"""
        p = abi.LensParams()
        p.struct_size = C.sizeof(abi.LensParams)
        p.samples = 0 if samples is None else int(samples)
        p.flags = abi.ACN_LENS_JITTER if jitter else 0
        p.seed = int(seed)
        p.aperture_radius = float(aperture)
        p.focus_distance = float(focus)
        return p

    @staticmethod
    def _lens(lens, params):
        if lens is not None and params:
            raise ValueError("give either an acn_lens_params or its keyword arguments")
        return lens if lens is not None else Handle.lens_params(**params)

    def lens_rays(self, pos_xy, first_sample=0, n_samples=None, lens=None, **params):
        """The lens rays of sample positions (acn_lens_rays): pos_xy [n,2] -> [n, n_samples, 6] origin, direction of the samples
        first_sample .. first_sample + n_samples - 1 (default: all from first_sample on).  lens: an abi.LensParams, or its
        keyword arguments (Handle.lens_params)."""
        p = self._lens(lens, params)
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        if n_samples is None:
            n_samples = (p.samples or abi.ACN_LENS_DEFAULT_SAMPLES) - first_sample
        out = np.empty((pos.shape[0], max(int(n_samples), 0), 6), dtype=np.float64)
        check(hip.acn_lens_rays(self.h, pos.ctypes.data, pos.shape[0], C.byref(p), first_sample, n_samples, out.ctypes.data),
              "acn_lens_rays")
        return out

    def lens_rays_dev(self, d_pos_ptr, n, d_out_ptr, first_sample=0, n_samples=None, stream=None, lens=None, **params):
        p = self._lens(lens, params)
        if n_samples is None:
            n_samples = (p.samples or abi.ACN_LENS_DEFAULT_SAMPLES) - first_sample
        o = self._opts(False, stream)
        check(hip.acn_lens_rays_dev(self.h, d_pos_ptr, n, C.byref(p), first_sample, n_samples, d_out_ptr, C.byref(o)),
              "acn_lens_rays_dev")

    def render_lens(self, pos_xy, linear=False, lens=None, **params):
        """The mean radiance of the lens rays of every position (acn_render_lens): pos_xy [n,2] -> rgb [n,3] float64."""
        p = self._lens(lens, params)
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((pos.shape[0], 3), dtype=np.float64)
        o = self._opts(linear, None)
        check(hip.acn_render_lens(self.h, pos.ctypes.data, pos.shape[0], C.byref(p), out.ctypes.data, C.byref(o)), "acn_render_lens")
        return out

    def render_lens_dev(self, d_pos_ptr, n, d_out_ptr, linear=False, stream=None, lens=None, **params):
        p = self._lens(lens, params)
        o = self._opts(linear, stream)
        check(hip.acn_render_lens_dev(self.h, d_pos_ptr, n, C.byref(p), d_out_ptr, C.byref(o)), "acn_render_lens_dev")

    def render_lens_main_pass_dev(self, first, count, d_out_ptr, linear=False, stream=None, lens=None, **params):
        p = self._lens(lens, params)
        o = self._opts(linear, stream)
        check(hip.acn_render_lens_main_pass_dev(self.h, first, count, C.byref(p), d_out_ptr, C.byref(o)),
              "acn_render_lens_main_pass_dev")

    # lens sample statistics (acn_render_lens_stats, acn_lens_stats_*, acn_denoise_stats): one [8] float64 record per position
    def _plain_opts(self, linear, stream):
        o = self._opts(linear, stream)
        o.shard_mode, o.shard_rank, o.shard_world = abi.ACN_SHARD_NONE, 0, 0
        return o

    def render_lens_stats(self, pos_xy, linear=False, lens=None, **params):
        """render_lens and the sample statistics of every position (acn_render_lens_stats): pos_xy [n,2] -> ( rgb [n,3] float64,
        saturated or linear as render_lens gives it, LensStats over [n,8] )."""
        p = self._lens(lens, params)
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((pos.shape[0], 3), dtype=np.float64)
        raw = np.empty((pos.shape[0], abi.ACN_STATS_STRIDE), dtype=np.float64)
        o = self._opts(linear, None)
        check(hip.acn_render_lens_stats(self.h, pos.ctypes.data, pos.shape[0], C.byref(p), out.ctypes.data, raw.ctypes.data, C.byref(o)),
              "acn_render_lens_stats")
        return out, LensStats(raw, self)

    def render_lens_stats_dev(self, d_pos_ptr, n, d_out_ptr, d_stats_ptr, linear=False, stream=None, lens=None, **params):
        """Device buffers: d_out [n,3] float64 or None, d_stats [n,8] float64, 16-byte aligned."""
        p = self._lens(lens, params)
        o = self._opts(linear, stream)
        check(hip.acn_render_lens_stats_dev(self.h, d_pos_ptr, n, C.byref(p), d_out_ptr, d_stats_ptr, C.byref(o)),
              "acn_render_lens_stats_dev")

    def render_lens_stats_main_pass_dev(self, first, count, d_out_ptr, d_stats_ptr, linear=False, stream=None, lens=None, **params):
        p = self._lens(lens, params)
        o = self._opts(linear, stream)
        check(hip.acn_render_lens_stats_main_pass_dev(self.h, first, count, C.byref(p), d_out_ptr, d_stats_ptr, C.byref(o)),
              "acn_render_lens_stats_main_pass_dev")

    def lens_stats_merge(self, acc, part, index=None):
        """Merges the records `part` into a copy of `acc` (acn_lens_stats_merge), part[j] into acc[index[j]] (index None: acc[j]);
        LensStats or [n,8] arrays -> LensStats.  Indices out of range or given twice are refused."""
        a = np.array(acc.raw if isinstance(acc, LensStats) else acc, dtype=np.float64).reshape(-1, abi.ACN_STATS_STRIDE)
        b = np.ascontiguousarray(part.raw if isinstance(part, LensStats) else part, dtype=np.float64).reshape(-1, abi.ACN_STATS_STRIDE)
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
        if idx is not None and len(idx) != len(b):
            raise ValueError(f"{len(b)} records need {len(b)} indices, got {len(idx)}")
        o = self._plain_opts(False, None)
        check(hip.acn_lens_stats_merge(self.h, a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0],
                                       None if idx is None else idx.ctypes.data, C.byref(o)), "acn_lens_stats_merge")
        return LensStats(a, self)

    def lens_stats_merge_dev(self, d_acc_ptr, n_acc, d_part_ptr, n_part, d_index_ptr=None, stream=None):
        """Device buffers; d_index int64 [n_part] or None.  An index outside [0, n_acc) is skipped."""
        o = self._plain_opts(False, stream)
        check(hip.acn_lens_stats_merge_dev(self.h, d_acc_ptr, n_acc, d_part_ptr, n_part, d_index_ptr, C.byref(o)),
              "acn_lens_stats_merge_dev")

    def lens_stats_resolve_dev(self, d_stats_ptr, n, d_out_rgb_ptr=None, d_out_noise_ptr=None, linear=False, stream=None):
        """The colour [n,3] (saturated unless linear; the background for an EMPTY record) and the noise [n] of device records."""
        o = self._plain_opts(linear, stream)
        check(hip.acn_lens_stats_resolve_dev(self.h, d_stats_ptr, n, d_out_rgb_ptr, d_out_noise_ptr, C.byref(o)),
              "acn_lens_stats_resolve_dev")

    def lens_stats_resolve(self, stats, linear=False):
        """acn_lens_stats_resolve_dev on host records (LensStats or [n,8]) -> ( rgb [n,3], noise [n] ); the copies go through torch."""
        import torch
        raw = np.ascontiguousarray(stats.raw if isinstance(stats, LensStats) else stats, dtype=np.float64).reshape(-1, abi.ACN_STATS_STRIDE)
        n = raw.shape[0]
        dev = torch.device("cuda", self.device)
        d = torch.from_numpy(raw).to(dev)
        rgb = torch.empty((n, 3), dtype=torch.float64, device=dev)
        noise = torch.empty((n,), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.lens_stats_resolve_dev(d.data_ptr(), n, rgb.data_ptr(), noise.data_ptr(), linear=linear)
        return rgb.cpu().numpy(), noise.cpu().numpy()

    def denoise_stats(self, stats, surface, width, height, **params):
        """acn_denoise with the measured variance (acn_denoise_stats): stats the LensStats (or [h*w,8] records) of a frame's pixels,
        surface the Surface of the same positions -> [h,w,3] float64, linear.  params: as for denoise."""
        raw = np.ascontiguousarray(stats.raw if isinstance(stats, LensStats) else stats, dtype=np.float64)
        srf = np.ascontiguousarray(surface.raw if isinstance(surface, Surface) else surface, dtype=np.float64)
        n = int(width) * int(height)
        if raw.size != n * abi.ACN_STATS_STRIDE or srf.size != n * abi.ACN_SURF_STRIDE:
            raise ValueError(f"{height}x{width} pixels need {n} statistics and surface records, got {raw.shape} and {srf.shape}")
        out = np.empty((int(height), int(width), 3), dtype=np.float64)
        p = self.denoise_params(**params)
        o = self._plain_opts(False, None)
        check(hip.acn_denoise_stats(self.h, raw.ctypes.data, srf.ctypes.data, width, height, C.byref(p), out.ctypes.data, C.byref(o)),
              "acn_denoise_stats")
        return out

    def denoise_stats_dev(self, d_stats_ptr, d_surface_ptr, width, height, d_out_ptr, stream=None, **params):
        """Device buffers: d_stats [h*w,8], d_surface [h*w,16], d_out [h*w,3] float64; enqueued on `stream` without a
        synchronisation (None: the handle's stream, synchronous)."""
        p = self.denoise_params(**params)
        o = self._plain_opts(False, stream)
        check(hip.acn_denoise_stats_dev(self.h, d_stats_ptr, d_surface_ptr, width, height, C.byref(p), d_out_ptr, C.byref(o)),
              "acn_denoise_stats_dev")

    # filling a sparse frame (acn_fill_stats): the EMPTY records of a frame from the rendered neighbours of the same surface
    @staticmethod
    def fill_params(radius=None, normal_power_log2=None, demodulate=True, sigma_px=None, sigma_plane=None):
        """acn_fill_params of keyword arguments; None is the library's default"""
        p = abi.FillParams()
        p.struct_size = C.sizeof(abi.FillParams)
        p.radius = 0 if radius is None else int(radius)
        if normal_power_log2 is not None:
            p.normal_power_log2 = int(normal_power_log2)
            p.flags |= abi.ACN_DENOISE_NORMAL_POWER_SET
        if not demodulate:
            p.flags |= abi.ACN_DENOISE_NO_DEMODULATE
        p.sigma_px = 0.0 if sigma_px is None else float(sigma_px)
        p.sigma_plane = 0.0 if sigma_plane is None else float(sigma_plane)
        return p

    def fill_stats(self, stats, surface, width, height, **params):
        """Fills the unrendered positions of a sparse frame (acn_fill_stats): stats the LensStats (or [h*w,8] records) of the raster,
        EMPTY where nothing was rendered, surface the Surface of EVERY position -> ( LensStats over [h*w,8], need [h,w] float64:
        -1 rendered, 0 background, 1 - sw / sa filled, +inf unfilled ).  params: radius, normal_power_log2, demodulate, sigma_px,
        sigma_plane (Handle.fill_params)."""
        raw = np.ascontiguousarray(stats.raw if isinstance(stats, LensStats) else stats, dtype=np.float64)
        srf = np.ascontiguousarray(surface.raw if isinstance(surface, Surface) else surface, dtype=np.float64)
        n = int(width) * int(height)
        if raw.size != n * abi.ACN_STATS_STRIDE or srf.size != n * abi.ACN_SURF_STRIDE:
            raise ValueError(f"{height}x{width} pixels need {n} statistics and surface records, got {raw.shape} and {srf.shape}")
        out = np.empty((n, abi.ACN_STATS_STRIDE), dtype=np.float64)
        need = np.empty((int(height), int(width)), dtype=np.float64)
        p = self.fill_params(**params)
        o = self._plain_opts(False, None)
        check(hip.acn_fill_stats(self.h, raw.ctypes.data, srf.ctypes.data, width, height, C.byref(p), out.ctypes.data, need.ctypes.data,
                                 C.byref(o)), "acn_fill_stats")
        return LensStats(out, self), need

    def fill_stats_dev(self, d_stats_ptr, d_surface_ptr, width, height, d_out_stats_ptr, d_out_need_ptr=None, stream=None, **params):
        """Device buffers: d_stats, d_out_stats [h*w,8] (they may not overlap), d_surface [h*w,16], d_out_need [h*w] float64 or None;
        enqueued on `stream` without a synchronisation (None: the handle's stream, synchronous)."""
        p = self.fill_params(**params)
        o = self._plain_opts(False, stream)
        check(hip.acn_fill_stats_dev(self.h, d_stats_ptr, d_surface_ptr, width, height, C.byref(p), d_out_stats_ptr, d_out_need_ptr,
                                     C.byref(o)), "acn_fill_stats_dev")

    # lens surface records (acn_surface_reduce, acn_surface_lens): the K records of a position reduced to one aggregate record
    def surface_reduce(self, records):
        """The aggregate record of every position (acn_surface_reduce): records [n,K,16] float64, the surface records of the K rays
        of each position -> Surface over [n,16]; .coverage is the share of the K samples in the dominant class."""
        r = np.ascontiguousarray(records, dtype=np.float64)
        if r.ndim != 3 or r.shape[2] != abi.ACN_SURF_STRIDE:
            raise ValueError(f"records to reduce are [n,K,{abi.ACN_SURF_STRIDE}] float64, got {r.shape}")
        out = np.empty((r.shape[0], abi.ACN_SURF_STRIDE), dtype=np.float64)
        o = self._plain_opts(False, None)
        check(hip.acn_surface_reduce(self.h, r.ctypes.data, r.shape[0], r.shape[1], out.ctypes.data, C.byref(o)), "acn_surface_reduce")
        return Surface(out)

    def surface_reduce_dev(self, d_records_ptr, n, samples, d_out_ptr, stream=None):
        """Device buffers: d_records [n,samples,16], d_out [n,16] float64, 16-byte aligned; enqueued on `stream` without a
        synchronisation (None: the handle's stream, synchronous)."""
        o = self._plain_opts(False, stream)
        check(hip.acn_surface_reduce_dev(self.h, d_records_ptr, n, samples, d_out_ptr, C.byref(o)), "acn_surface_reduce_dev")

    def surface_lens(self, pos_xy, follow=False, lens=None, **params):
        """The aggregate surface record of the lens rays of every position (acn_surface_lens): pos_xy [n,2] -> Surface.  lens: an
        abi.LensParams, or its keyword arguments samples, aperture, focus, jitter, seed (Handle.lens_params): with those of a
        render_lens_stats call the records describe the samples behind its statistics."""
        p = self._lens(lens, params)
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((pos.shape[0], abi.ACN_SURF_STRIDE), dtype=np.float64)
        o = self._plain_opts(False, None)
        check(hip.acn_surface_lens(self.h, pos.ctypes.data, pos.shape[0], C.byref(p), self._surface_mode(follow), out.ctypes.data,
                                   C.byref(o)), "acn_surface_lens")
        return Surface(out)

    def surface_lens_dev(self, d_pos_ptr, n, d_out_ptr, follow=False, stream=None, lens=None, **params):
        """Device buffers: d_pos [n,2], d_out [n,16] float64, 16-byte aligned."""
        p = self._lens(lens, params)
        o = self._plain_opts(False, stream)
        check(hip.acn_surface_lens_dev(self.h, d_pos_ptr, n, C.byref(p), self._surface_mode(follow), d_out_ptr, C.byref(o)),
              "acn_surface_lens_dev")

    def surface_lens_main_pass_dev(self, first, count, d_out_ptr, follow=False, stream=None, lens=None, **params):
        p = self._lens(lens, params)
        o = self._plain_opts(False, stream)
        check(hip.acn_surface_lens_main_pass_dev(self.h, first, count, C.byref(p), self._surface_mode(follow), d_out_ptr, C.byref(o)),
              "acn_surface_lens_main_pass_dev")

    # layered lens records (acn_lens_layers_reduce, acn_render_lens_layers, acn_denoise_layers): the two largest classes of a
    # position's samples as records of their own, planar: surface [2,n,16] (layer 0, layer 1), statistics [3,n,8] (layer 0, layer 1, rest)
    def lens_layers_reduce(self, records, radiance):
        """The split alone (acn_lens_layers_reduce): records [n,K,16] and linear radiance [n,K,3] of the K rays of each position ->
        ( [Surface, Surface], [LensStats, LensStats, LensStats] ): layer 0, layer 1 and, of the statistics, the rest."""
        r = np.ascontiguousarray(records, dtype=np.float64)
        L = np.ascontiguousarray(radiance, dtype=np.float64)
        if r.ndim != 3 or r.shape[2] != abi.ACN_SURF_STRIDE or L.shape != r.shape[:2] + (3,):
            raise ValueError(f"layers are split from records [n,K,{abi.ACN_SURF_STRIDE}] and radiance [n,K,3], got {r.shape} and {L.shape}")
        n = r.shape[0]
        surf = np.empty((abi.ACN_LAYERS_SURFACE_PLANES, n, abi.ACN_SURF_STRIDE), dtype=np.float64)
        st = np.empty((abi.ACN_LAYERS_STATS_PLANES, n, abi.ACN_STATS_STRIDE), dtype=np.float64)
        o = self._plain_opts(False, None)
        check(hip.acn_lens_layers_reduce(self.h, r.ctypes.data, L.ctypes.data, n, r.shape[1], surf.ctypes.data, st.ctypes.data, C.byref(o)),
              "acn_lens_layers_reduce")
        return [Surface(p) for p in surf], [LensStats(p, self) for p in st]

    def lens_layers_reduce_dev(self, d_records_ptr, d_radiance_ptr, n, samples, d_out_surface_ptr, d_out_stats_ptr, stream=None):
        """Device buffers: d_records [n,samples,16], d_radiance [n,samples,3], d_out_surface [2,n,16], d_out_stats [3,n,8] float64,
        the records 16-byte aligned; enqueued on `stream` without a synchronisation (None: the handle's stream, synchronous)."""
        o = self._plain_opts(False, stream)
        check(hip.acn_lens_layers_reduce_dev(self.h, d_records_ptr, d_radiance_ptr, n, samples, d_out_surface_ptr, d_out_stats_ptr, C.byref(o)),
              "acn_lens_layers_reduce_dev")

    def render_lens_layers(self, pos_xy, follow=False, linear=False, lens=None, **params):
        """render_lens and the layered records of every position (acn_render_lens_layers): pos_xy [n,2] -> ( rgb [n,3] float64 as
        render_lens gives it, [Surface, Surface], [LensStats, LensStats, LensStats] ).  lens: an abi.LensParams, or its keyword
        arguments samples, aperture, focus, jitter, seed (Handle.lens_params)."""
        p = self._lens(lens, params)
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        n = pos.shape[0]
        out = np.empty((n, 3), dtype=np.float64)
        surf = np.empty((abi.ACN_LAYERS_SURFACE_PLANES, n, abi.ACN_SURF_STRIDE), dtype=np.float64)
        st = np.empty((abi.ACN_LAYERS_STATS_PLANES, n, abi.ACN_STATS_STRIDE), dtype=np.float64)
        o = self._opts(linear, None)
        check(hip.acn_render_lens_layers(self.h, pos.ctypes.data, n, C.byref(p), self._surface_mode(follow), out.ctypes.data, surf.ctypes.data,
                                         st.ctypes.data, C.byref(o)), "acn_render_lens_layers")
        return out, [Surface(q) for q in surf], [LensStats(q, self) for q in st]

    def render_lens_layers_dev(self, d_pos_ptr, n, d_out_ptr, d_out_surface_ptr, d_out_stats_ptr, follow=False, linear=False, stream=None,
                               lens=None, **params):
        """Device buffers: d_pos [n,2], d_out [n,3] or None, d_out_surface [2,n,16], d_out_stats [3,n,8] float64, 16-byte aligned."""
        p = self._lens(lens, params)
        o = self._opts(linear, stream)
        check(hip.acn_render_lens_layers_dev(self.h, d_pos_ptr, n, C.byref(p), self._surface_mode(follow), d_out_ptr, d_out_surface_ptr,
                                             d_out_stats_ptr, C.byref(o)), "acn_render_lens_layers_dev")

    def render_lens_layers_main_pass_dev(self, first, count, d_out_ptr, d_out_surface_ptr, d_out_stats_ptr, follow=False, linear=False,
                                         stream=None, lens=None, **params):
        p = self._lens(lens, params)
        o = self._opts(linear, stream)
        check(hip.acn_render_lens_layers_main_pass_dev(self.h, first, count, C.byref(p), self._surface_mode(follow), d_out_ptr,
                                                       d_out_surface_ptr, d_out_stats_ptr, C.byref(o)), "acn_render_lens_layers_main_pass_dev")

    @staticmethod
    def _planes(records, cls, planes, stride):
        """[planes,n,stride] float64 of a list of Surface / LensStats or of an array"""
        if isinstance(records, (list, tuple)):
            records = [r.raw if isinstance(r, cls) else r for r in records]
        raw = np.ascontiguousarray(records, dtype=np.float64)
        if raw.ndim != 3 or raw.shape[0] != planes or raw.shape[2] != stride:
            raise ValueError(f"layered records are [{planes},n,{stride}] float64, got {raw.shape}")
        return raw

    def denoise_layers(self, stats, surface, width, height, **params):
        """The layered filter (acn_denoise_layers): stats the three LensStats (or [3,h*w,8]) and surface the two Surface (or
        [2,h*w,16]) of a frame's pixels, as render_lens_layers gives them -> [h,w,3] float64, linear.  params: as for denoise."""
        raw = self._planes(stats, LensStats, abi.ACN_LAYERS_STATS_PLANES, abi.ACN_STATS_STRIDE)
        srf = self._planes(surface, Surface, abi.ACN_LAYERS_SURFACE_PLANES, abi.ACN_SURF_STRIDE)
        n = int(width) * int(height)
        if raw.shape[1] != n or srf.shape[1] != n:
            raise ValueError(f"{height}x{width} pixels need {n} records per plane, got {raw.shape} and {srf.shape}")
        out = np.empty((int(height), int(width), 3), dtype=np.float64)
        p = self.denoise_params(**params)
        o = self._plain_opts(False, None)
        check(hip.acn_denoise_layers(self.h, raw.ctypes.data, srf.ctypes.data, width, height, C.byref(p), out.ctypes.data, C.byref(o)),
              "acn_denoise_layers")
        return out

    def denoise_layers_dev(self, d_stats_ptr, d_surface_ptr, width, height, d_out_ptr, stream=None, **params):
        """Device buffers: d_stats [3,h*w,8], d_surface [2,h*w,16], d_out [h*w,3] float64; enqueued on `stream` without a
        synchronisation (None: the handle's stream, synchronous)."""
        p = self.denoise_params(**params)
        o = self._plain_opts(False, stream)
        check(hip.acn_denoise_layers_dev(self.h, d_stats_ptr, d_surface_ptr, width, height, C.byref(p), d_out_ptr, C.byref(o)),
              "acn_denoise_layers_dev")

    # layered records across passes (acn_lens_layers_merge, acn_lens_layers_resolve_dev): layers matched by surface class
    def lens_layers_merge(self, acc_surface, acc_stats, part_surface, part_stats, index=None):
        """Merges the layered records of a part into copies of an accumulator's (acn_lens_layers_merge), position j of the part into
        position index[j] (index None: j).  Surface planes: two Surface or [2,n,16]; statistics planes: three LensStats or [3,n,8]
        -> ( [Surface, Surface], [LensStats, LensStats, LensStats] ).  Indices out of range or given twice are refused."""
        a_s = np.array(self._planes(acc_surface, Surface, abi.ACN_LAYERS_SURFACE_PLANES, abi.ACN_SURF_STRIDE))
        a_t = np.array(self._planes(acc_stats, LensStats, abi.ACN_LAYERS_STATS_PLANES, abi.ACN_STATS_STRIDE))
        b_s = self._planes(part_surface, Surface, abi.ACN_LAYERS_SURFACE_PLANES, abi.ACN_SURF_STRIDE)
        b_t = self._planes(part_stats, LensStats, abi.ACN_LAYERS_STATS_PLANES, abi.ACN_STATS_STRIDE)
        if a_s.shape[1] != a_t.shape[1] or b_s.shape[1] != b_t.shape[1]:
            raise ValueError(f"surface and statistics planes of one side hold the same positions, got {a_s.shape}, {a_t.shape}, {b_s.shape}, {b_t.shape}")
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
        if idx is not None and len(idx) != b_t.shape[1]:
            raise ValueError(f"{b_t.shape[1]} positions need {b_t.shape[1]} indices, got {len(idx)}")
        o = self._plain_opts(False, None)
        check(hip.acn_lens_layers_merge(self.h, a_s.ctypes.data, a_t.ctypes.data, a_t.shape[1], b_s.ctypes.data, b_t.ctypes.data, b_t.shape[1],
                                        None if idx is None else idx.ctypes.data, C.byref(o)), "acn_lens_layers_merge")
        return [Surface(p) for p in a_s], [LensStats(p, self) for p in a_t]

    def lens_layers_merge_dev(self, d_acc_surface_ptr, d_acc_stats_ptr, n_acc, d_part_surface_ptr, d_part_stats_ptr, n_part, d_index_ptr=None,
                              stream=None):
        """Device buffers: accumulator [2,n_acc,16] and [3,n_acc,8], part [2,n_part,16] and [3,n_part,8] float64, 16-byte aligned;
        d_index int64 [n_part] or None.  An index outside [0, n_acc) is skipped; a caller's stream is never synchronised."""
        o = self._plain_opts(False, stream)
        check(hip.acn_lens_layers_merge_dev(self.h, d_acc_surface_ptr, d_acc_stats_ptr, n_acc, d_part_surface_ptr, d_part_stats_ptr, n_part,
                                            d_index_ptr, C.byref(o)), "acn_lens_layers_merge_dev")

    def lens_layers_resolve_dev(self, d_stats_ptr, n, d_out_rgb_ptr=None, d_out_noise_ptr=None, d_out_pooled_ptr=None, linear=False, stream=None):
        """Device statistics planes [3,n,8] as one population per position: the colour [n,3] (saturated unless linear; the
        background where all three records are EMPTY), the noise [n] and the pooled record [n,8]; each output may be None."""
        o = self._plain_opts(linear, stream)
        check(hip.acn_lens_layers_resolve_dev(self.h, d_stats_ptr, n, d_out_rgb_ptr, d_out_noise_ptr, d_out_pooled_ptr, C.byref(o)),
              "acn_lens_layers_resolve_dev")

    def lens_layers_resolve(self, stats, linear=False):
        """acn_lens_layers_resolve_dev on host planes (three LensStats or [3,n,8]) -> ( rgb [n,3], noise [n], pooled LensStats ); the
        copies go through torch."""
        import torch
        raw = self._planes(stats, LensStats, abi.ACN_LAYERS_STATS_PLANES, abi.ACN_STATS_STRIDE)
        n = raw.shape[1]
        dev = torch.device("cuda", self.device)
        d = torch.from_numpy(raw).to(dev)
        rgb = torch.empty((n, 3), dtype=torch.float64, device=dev)
        noise = torch.empty((n,), dtype=torch.float64, device=dev)
        pooled = torch.empty((n, abi.ACN_STATS_STRIDE), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.lens_layers_resolve_dev(d.data_ptr(), n, rgb.data_ptr(), noise.data_ptr(), pooled.data_ptr(), linear=linear)
        return rgb.cpu().numpy(), noise.cpu().numpy(), LensStats(pooled.cpu().numpy(), self)

    # projected points and reprojected statistics (acn_project_points, acn_reproject): the history of the next frame of an animation
    def project_points(self, points):
        """The sample positions of world points with the handle's current camera (acn_project_points), the inverse of camera_rays:
        points [n,3] -> ( pos_xy [n,2], NaN where the point is not in front of the camera; depth [n] along the view direction )."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        pos = np.empty((pts.shape[0], 2), dtype=np.float64)
        depth = np.empty((pts.shape[0],), dtype=np.float64)
        check(hip.acn_project_points(self.h, pts.ctypes.data, pts.shape[0], pos.ctypes.data, depth.ctypes.data), "acn_project_points")
        return pos, depth

    def project_points_dev(self, d_points_ptr, n, d_out_pos_ptr, d_out_depth_ptr=None, stream=None):
        o = self._plain_opts(False, stream)
        check(hip.acn_project_points_dev(self.h, d_points_ptr, n, d_out_pos_ptr, d_out_depth_ptr, C.byref(o)), "acn_project_points_dev")

    @staticmethod
    def reproject_params(reject_kinds=None, max_hops=None, normal_min=None, plane_tolerance=None, max_history=None):
        """acn_reproject_params of keyword arguments; None is the library's default"""
        p = abi.ReprojectParams()
        p.struct_size = C.sizeof(abi.ReprojectParams)
        if reject_kinds is not None:
            p.reject_kinds = int(reject_kinds)
            p.flags |= abi.ACN_REPROJECT_KINDS_SET
        if max_hops is not None:
            p.max_hops = int(max_hops)
            p.flags |= abi.ACN_REPROJECT_HOPS_SET
        p.normal_min = 0.0 if normal_min is None else float(normal_min)
        p.plane_tolerance = 0.0 if plane_tolerance is None else float(plane_tolerance)
        p.max_history = 0.0 if max_history is None else float(max_history)
        return p

    def reproject(self, cur_surface, prev_params, prev_surface, prev_stats, **params):
        """The statistics the previous frame accumulated where the current frame's surface points lay in it (acn_reproject):
        cur_surface the Surface (or [n,16] records) of the current positions, prev_params the abi.Params the previous frame was rendered
        with, prev_surface and prev_stats the Surface and LensStats (or records) of its whole raster -> ( LensStats over [n,8], motion
        [n,2]: the position on the previous raster, NaN where there is none ).  params: reject_kinds, max_hops, normal_min,
        plane_tolerance, max_history (Handle.reproject_params).  Merge the result with the current frame's statistics by lens_stats_merge."""
        return self._reproject_host(cur_surface, prev_params, prev_surface, prev_stats, None, params)

    def _reproject_host(self, cur_surface, prev_params, prev_surface, prev_stats, motion, params):
        """the host form of acn_reproject, or with a motion table of acn_reproject_moving"""
        cur = np.ascontiguousarray(cur_surface.raw if isinstance(cur_surface, Surface) else cur_surface, dtype=np.float64).reshape(-1, abi.ACN_SURF_STRIDE)
        ps = np.ascontiguousarray(prev_surface.raw if isinstance(prev_surface, Surface) else prev_surface, dtype=np.float64).reshape(-1, abi.ACN_SURF_STRIDE)
        pt = np.ascontiguousarray(prev_stats.raw if isinstance(prev_stats, LensStats) else prev_stats, dtype=np.float64).reshape(-1, abi.ACN_STATS_STRIDE)
        pixels = int(prev_params.image_width) * int(prev_params.image_height)
        if len(ps) != pixels or len(pt) != pixels:
            raise ValueError(f"the previous raster has {pixels} pixels: got {len(ps)} surface and {len(pt)} statistics records")
        out = np.empty((cur.shape[0], abi.ACN_STATS_STRIDE), dtype=np.float64)
        out_motion = np.empty((cur.shape[0], 2), dtype=np.float64)
        p = self.reproject_params(**params)
        o = self._plain_opts(False, None)
        if motion is None:
            check(hip.acn_reproject(self.h, cur.ctypes.data, cur.shape[0], C.byref(prev_params), ps.ctypes.data, pt.ctypes.data, C.byref(p),
                                    out.ctypes.data, out_motion.ctypes.data, C.byref(o)), "acn_reproject")
        else:
            table = np.ascontiguousarray(motion, dtype=np.float64).reshape(-1, abi.ACN_MOTION_STRIDE)
            check(hip.acn_reproject_moving(self.h, cur.ctypes.data, cur.shape[0], C.byref(prev_params), ps.ctypes.data, pt.ctypes.data, table.ctypes.data,
                                           table.shape[0], C.byref(p), out.ctypes.data, out_motion.ctypes.data, C.byref(o)), "acn_reproject_moving")
        return LensStats(out, self), out_motion

    def reproject_dev(self, d_cur_surface_ptr, n, prev_params, d_prev_surface_ptr, d_prev_stats_ptr, d_out_stats_ptr, d_out_motion_ptr=None,
                      stream=None, **params):
        """Device buffers: records 16-byte aligned, d_out_motion [n,2] float64 or None; enqueued on `stream` without a synchronisation
        (None: the handle's stream, synchronous)."""
        p = self.reproject_params(**params)
        o = self._plain_opts(False, stream)
        check(hip.acn_reproject_dev(self.h, d_cur_surface_ptr, n, C.byref(prev_params), d_prev_surface_ptr, d_prev_stats_ptr, C.byref(p),
                                    d_out_stats_ptr, d_out_motion_ptr, C.byref(o)), "acn_reproject_dev")

    # reprojection through moving objects (acn_reproject_moving): a motion table, one row per node index (motion_from_scenes)
    def reproject_moving(self, cur_surface, prev_params, prev_surface, prev_stats, motion, **params):
        """reproject() with a motion table [n_nodes,16] (motion_from_scenes, or hand-made rows: include/actinon_hip.h): the history of
        a point on a moved object is taken where that point was one frame ago -> ( LensStats over [n,8], motion [n,2] )."""
        return self._reproject_host(cur_surface, prev_params, prev_surface, prev_stats, motion, params)

    def reproject_moving_dev(self, d_cur_surface_ptr, n, prev_params, d_prev_surface_ptr, d_prev_stats_ptr, d_motion_ptr, n_motion, d_out_stats_ptr,
                             d_out_motion_ptr=None, stream=None, **params):
        """Device buffers, the table [n_motion,16] float64 among them, all 16-byte aligned; enqueued on `stream` without a synchronisation
        (None: the handle's stream, synchronous)."""
        p = self.reproject_params(**params)
        o = self._plain_opts(False, stream)
        check(hip.acn_reproject_moving_dev(self.h, d_cur_surface_ptr, n, C.byref(prev_params), d_prev_surface_ptr, d_prev_stats_ptr, d_motion_ptr,
                                           n_motion, C.byref(p), d_out_stats_ptr, d_out_motion_ptr, C.byref(o)), "acn_reproject_moving_dev")

    # shadow records and the history guard (acn_shadow_records, acn_shadow_limit_history)
    @staticmethod
    def shadow_params(samples=None):
        """acn_shadow_params of keyword arguments; None is the library's default"""
        p = abi.ShadowParams()
        p.struct_size = C.sizeof(abi.ShadowParams)
        p.samples = 0 if samples is None else int(samples)
        return p

    @staticmethod
    def shadow_history_params(tolerance=None, changed_max_history=None, drop=False):
        """acn_shadow_history_params of keyword arguments; None is the library's default"""
        p = abi.ShadowHistoryParams()
        p.struct_size = C.sizeof(abi.ShadowHistoryParams)
        p.flags = abi.ACN_SHADOW_HISTORY_DROP if drop else 0
        p.tolerance = 0.0 if tolerance is None else float(tolerance)
        p.changed_max_history = 0.0 if changed_max_history is None else float(changed_max_history)
        return p

    def shadow_records(self, surface, samples=16):
        """How much of each light the surface points see (acn_shadow_records): surface a Surface or [n,16] records, samples one of
        1, 2, 4, 8, 16, 32, 64 -> [n,16] float64: state, S, L, asked, clear, clear / asked, clear of lights 0..4, asked of lights 0..4."""
        s = np.ascontiguousarray(surface.raw if isinstance(surface, Surface) else surface, dtype=np.float64).reshape(-1, abi.ACN_SURF_STRIDE)
        out = np.empty((s.shape[0], abi.ACN_SHADOW_STRIDE), dtype=np.float64)
        p = self.shadow_params(samples)
        o = self._plain_opts(False, None)
        check(hip.acn_shadow_records(self.h, s.ctypes.data, s.shape[0], C.byref(p), out.ctypes.data, C.byref(o)), "acn_shadow_records")
        return out

    def shadow_records_dev(self, d_surface_ptr, n, d_out_ptr, samples=16, stream=None):
        """Device buffers, both 16-byte aligned: d_out [n,16] float64; enqueued on `stream` (None: the handle's stream, synchronous)."""
        p = self.shadow_params(samples)
        o = self._plain_opts(False, stream)
        check(hip.acn_shadow_records_dev(self.h, d_surface_ptr, n, C.byref(p), d_out_ptr, C.byref(o)), "acn_shadow_records_dev")

    def shadow_limit_history(self, stats, motion, cur_shadow, prev_shadow, prev_w, prev_h, tolerance=None, changed_max_history=None, drop=False):
        """Limits a reprojected history where the light a point sees has changed (acn_shadow_limit_history): stats the LensStats (or
        [n,8] records) and motion [n,2] that reproject / reproject_moving returned, cur_shadow [n,16] the shadow records of the same
        positions, prev_shadow those of the whole previous raster prev_w x prev_h -> ( LensStats over a limited COPY, change [n]: NaN
        where nothing was compared )."""
        t = np.array(stats.raw if isinstance(stats, LensStats) else stats, dtype=np.float64).reshape(-1, abi.ACN_STATS_STRIDE)
        m = np.ascontiguousarray(motion, dtype=np.float64).reshape(-1, 2)
        c = np.ascontiguousarray(cur_shadow, dtype=np.float64).reshape(-1, abi.ACN_SHADOW_STRIDE)
        q = np.ascontiguousarray(prev_shadow, dtype=np.float64).reshape(-1, abi.ACN_SHADOW_STRIDE)
        if len(m) != len(t) or len(c) != len(t):
            raise ValueError(f"{len(t)} statistics records: got {len(m)} motion rows and {len(c)} shadow records")
        if len(q) != int(prev_w) * int(prev_h):
            raise ValueError(f"the previous raster has {int(prev_w) * int(prev_h)} pixels: got {len(q)} shadow records")
        change = np.empty((t.shape[0],), dtype=np.float64)
        p = self.shadow_history_params(tolerance, changed_max_history, drop)
        o = self._plain_opts(False, None)
        check(hip.acn_shadow_limit_history(self.h, t.ctypes.data, m.ctypes.data, c.ctypes.data, q.ctypes.data, t.shape[0], int(prev_w), int(prev_h),
                                           C.byref(p), change.ctypes.data, C.byref(o)), "acn_shadow_limit_history")
        return LensStats(t, self), change

    def shadow_limit_history_dev(self, d_stats_ptr, d_motion_ptr, d_cur_shadow_ptr, d_prev_shadow_ptr, n, prev_w, prev_h, d_out_change_ptr=None,
                                 tolerance=None, changed_max_history=None, drop=False, stream=None):
        """Device buffers, the records 16-byte aligned; d_stats [n,8] is limited IN PLACE, d_out_change [n] float64 or None; enqueued on
        `stream` without a synchronisation (None: the handle's stream, synchronous)."""
        p = self.shadow_history_params(tolerance, changed_max_history, drop)
        o = self._plain_opts(False, stream)
        check(hip.acn_shadow_limit_history_dev(self.h, d_stats_ptr, d_motion_ptr, d_cur_shadow_ptr, d_prev_shadow_ptr, n, int(prev_w), int(prev_h),
                                               C.byref(p), d_out_change_ptr, C.byref(o)), "acn_shadow_limit_history_dev")

    def frame(self, w=None, h=None):
        """A device-resident frame of this handle (acn_frame_create), zeroed; by default of the raster the handle renders now."""
        return Frame(self, self.params.image_width if w is None else w, self.params.image_height if h is None else h)

    # selecting positions by a key (acn_select_above, acn_key_histogram): the step between a noise map and the next pass
    @staticmethod
    def select_params(threshold, capacity=0, raster_width=0, raster_first=0):
        p = abi.SelectParams()
        p.struct_size = C.sizeof(abi.SelectParams)
        p.threshold, p.capacity, p.raster_width, p.raster_first = threshold, capacity, raster_width, raster_first
        return p

    def select_above_dev(self, d_key_ptr, n, threshold, capacity, d_index_ptr=None, d_pos_ptr=None, d_src_pos_ptr=None, raster_width=0,
                         raster_first=0, d_count_ptr=None, want_count=True, stream=None):
        """The entries of the device keys [n] float64 above threshold, in ascending order (acn_select_above_dev): their indices into
        d_index int64 [capacity] and their positions into d_pos [capacity,2] float64 (either may be None) -- gathered from d_src_pos
        [n,2], or the pixel centres raster_first + i of a raster raster_width wide (0: the scene's).  The total goes to d_count
        (uint64 on the device, or None) and, with want_count, is returned, which synchronises `stream` once; else None is returned."""
        p = self.select_params(threshold, capacity, raster_width, raster_first)
        o = self._plain_opts(False, stream)
        count = C.c_uint64(0)
        check(hip.acn_select_above_dev(self.h, d_key_ptr, n, C.byref(p), d_src_pos_ptr, d_index_ptr, d_pos_ptr, d_count_ptr,
                                       C.byref(count) if want_count else None, C.byref(o)), "acn_select_above_dev")
        return int(count.value) if want_count else None

    def select_above(self, key, threshold, src_pos=None, raster_width=0, raster_first=0, capacity=None):
        """acn_select_above on host arrays: key [n] float64 -> ( index int64 [m], pos [m,2] float64, count ), m = min( count, capacity );
        capacity None: n.  count is the total selected, also beyond the capacity."""
        k = np.ascontiguousarray(key, dtype=np.float64).reshape(-1)
        n = k.shape[0]
        cap = n if capacity is None else int(capacity)
        src = None if src_pos is None else np.ascontiguousarray(src_pos, dtype=np.float64).reshape(-1, 2)
        if src is not None and src.shape[0] != n:
            raise ValueError(f"{n} keys need {n} positions, got {src.shape[0]}")
        room = min(cap, n)
        index = np.empty((room,), dtype=np.int64)
        pos = np.empty((room, 2), dtype=np.float64)
        p = self.select_params(threshold, cap, raster_width, raster_first)
        count = C.c_uint64(0)
        check(hip.acn_select_above(self.h, k.ctypes.data, n, C.byref(p), None if src is None else src.ctypes.data,
                                   index.ctypes.data if room else None, pos.ctypes.data if room else None, C.byref(count)), "acn_select_above")
        m = min(int(count.value), room)
        return index[:m], pos[:m], int(count.value)

    def key_histogram_dev(self, d_key_ptr, n, d_hist_ptr, stream=None):
        """The exact histogram of device keys [n] float64 into d_hist uint64 [257], overwritten (acn_key_histogram_dev)."""
        o = self._plain_opts(False, stream)
        check(hip.acn_key_histogram_dev(self.h, d_key_ptr, n, d_hist_ptr, C.byref(o)), "acn_key_histogram_dev")

    def key_histogram(self, key):
        """acn_key_histogram on a host array: key [n] float64 -> uint64 [257]; word 256 counts the NaN keys."""
        k = np.ascontiguousarray(key, dtype=np.float64).reshape(-1)
        hist = np.empty((abi.ACN_KEY_HIST_WORDS,), dtype=np.uint64)
        check(hip.acn_key_histogram(self.h, k.ctypes.data, k.shape[0], hist.ctypes.data), "acn_key_histogram")
        return hist

    def pick(self, x, y):
        """The object under sample position (x, y): None on a miss, else node (enter object if any, else exit object), its
        type name, distance and position."""
        s = self.surface_positions(np.array([[x, y]], dtype=np.float64))
        if not s.hit[0]:
            return None
        node = int(s.enter[0]) if s.enter[0] >= 0 else int(s.exit[0])
        return {"node": node, "type": abi.NODE_TYPES.get(int(self.flat.node(node).type)), "distance": float(s.distance[0]),
                "position": s.position[0].copy()}

    # test seam acn_query_rays (include/actinon_hip.h): the device's traversal shortcuts one ray per lane
    QUERY_OPS = {"hit_lane": 0, "hit_uni": 1, "element_hit": 2, "side_lane": 3, "side_uni": 4, "prune": 5, "leaf_iv": 6,
                 "trans": 7, "occluded": 8, "cone_cull": 9, "sc_hit": 10, "elements": 11}
    QUERY_STRIDE = 16

    def query_rays(self, op, node, rays=None, limits=None, skip=None, lds=True, prune=True, n=None):
        """[n, 16] float64 results of query `op` on node `node` for rays [n, 6] (origin, direction), ray i on lane i % 64
        of wave i / 64.  limits [n] and skip masks [n] (uint64) where the query takes them.  lds=False reads the node
        array from global memory where the handle stages it in LDS; prune=False runs the plain scene view (no interval-prune
        programs, no in-line simple compounds).  "elements" takes no rays: n is the number of elements to list."""
        code = self.QUERY_OPS[op] | (0 if lds else 0x100) | (0 if prune else 0x200)
        if rays is None:
            r, cnt = None, int(n)
        else:
            r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
            cnt = r.shape[0]
        lim = None
        if limits is not None or skip is not None:
            lim = np.zeros((cnt, 2), dtype=np.float64)
            lim[:, 0] = np.inf if limits is None else np.asarray(limits, dtype=np.float64)
            if skip is not None:
                lim.view(np.uint64)[:, 1] = np.asarray(skip, dtype=np.uint64)
        out = np.zeros((max(cnt, 1), self.QUERY_STRIDE), dtype=np.float64)
        check(hip.acn_query_rays(self.h, code, int(node), None if r is None else r.ctypes.data, cnt,
                                 None if lim is None else lim.ctypes.data, out.ctypes.data), "acn_query_rays")
        return out[:cnt]

    # test seam acn_run_stage (include/actinon_hip.h): one shading kernel alone.  The records of csrc/acn_records.h as numpy dtypes;
    # run_stage asserts their sizes against the library's
    _V = (np.float64, 3)
    STAGE_RECORDS = {
        "ray": np.dtype([("p", *_V), ("d", *_V), ("T", *_V), ("intensity", "f8"), ("depth", "i4"), ("pixel", "u4")]),
        "task": np.dtype([("pos", *_V), ("surface_d", *_V), ("ray_projection", *_V), ("theta_i", "f8"), ("on_a", "f8"), ("on_b", "f8"),
                          ("diffuse_intensity", "f8"), ("Tc", *_V), ("rv", "u8"), ("depth", "i4"), ("pixel", "u4")]),
        "hit": np.dtype([("p", *_V), ("d", *_V), ("offs", "f8"), ("exit_nor", *_V), ("T", *_V), ("intensity", "f8"), ("exit_obj", "i4"),
                         ("enter_obj", "i4"), ("depth", "i4"), ("pixel", "u4")]),
        "hard_shadow": np.dtype([("pos", *_V), ("d", *_V), ("limit", "f8"), ("contrib", *_V), ("pixel", "u4"), ("pad", "u4")]),
        "hard_path": np.dtype([("pos", *_V), ("d", *_V), ("T", *_V), ("intensity", "f8"), ("depth", "i4"), ("pixel", "u4"), ("resume", "u4"),
                               ("pad", "u4")]),
    }
    del _V
    STAGE_INVALID = 0xFFFFFFFF
    # words of the level's counter block (acn_counts.h)
    QC = {"tasks": 0, "class0": 1, "children": 5, "flags": 6, "hard_shadow": 7, "hard_path": 8, "walk_rays": 12, "s_hard_shadow": 13,
          "s_hard_path": 14, "s_children": 15, "s_tasks": 16, "s_probes": 19, "dead_t": 28, "dead_c": 29, "dead_hp": 30, "dead_r": 31, "gen0": 32}
    # the words only the walk writes: QS_WALK_STEPS, QS_PRIVATE_RAYS, QC_CUR_GEN + 0 (the work-fetch cursor of pass 0)
    QC_WALK = {"walk_steps": 17, "private_rays": 18, "cur_gen0": 65}

    def stage_info(self):
        """Sizes of the five records, words of a counter block, DevScene.class0_min, nodes, lights and the handle's kernel variant
        (prune programs, leaf lights, the node array staged in LDS)."""
        w = np.zeros(abi.ACN_STAGE_INFO_WORDS, dtype=np.uint32)
        check(hip.acn_stage_info(self.h, w.ctypes.data, w.size), "acn_stage_info")
        names = ("ray", "task", "hit", "hard_shadow", "hard_path")
        info = {"sizeof": {k: int(w[i]) for i, k in enumerate(names)}, "counter_words": int(w[5]), "class0_min": int(w[6]),
                "nodes": int(w[7]), "lights": int(w[8]), "prune": bool(w[9] & 1), "leaf_lights": bool(w[9] & 2), "lds_nodes": bool(w[9] & 4)}
        return info

    def run_stage(self, stage, records, index=None, cls=0, shard_rank=0, shard_world=1, prune=True, leaf_lights=True, emit_terms=True, grid=0,
                  count_work=False):
        """Runs one production shading kernel on `records` and returns everything it wrote as a dict of numpy arrays.
        stage "shade_hits": records are "hit" records (pixel = own index, or STAGE_INVALID); returns tasks, idx (four lists), rays,
        hard_shadow (the probes), counts, flags, accum.  stage "shade": records are "task" records, index the uint32 list the kernel of
        size class `cls` works off; returns children, hard_shadow, hard_path, counts, flags, accum.  stage "hard_shadow" / "hard_path":
        records are the queue of k_hard_shadow / k_hard_path as the kernel meets it, dead slots (pixel STAGE_INVALID) included, on
        `grid` workgroups (0: one per 256 records); returns counts, flags, accum, the queue slot for slot as "hard_shadow" left it, and
        children for "hard_path".  Queues come back up to their
        high-water mark with the dead slots (pixel STAGE_INVALID) taken out; accum is [n, 3] int64 in units of 2^-40.
        count_work: the counting variant of the kernel runs, and "counters" holds its work counters under the names of last_counters."""
        info = self.stage_info()
        for k, dt in self.STAGE_RECORDS.items():
            assert dt.itemsize == info["sizeof"][k], (k, dt.itemsize, info["sizeof"][k])
        code, kind = {"shade_hits": (abi.ACN_STAGE_SHADE_HITS, "hit"), "shade": (abi.ACN_STAGE_SHADE, "task"),
                      "hard_shadow": (abi.ACN_STAGE_HARD_SHADOW, "hard_shadow"), "hard_path": (abi.ACN_STAGE_HARD_PATH, "hard_path")}[stage]
        shade, hard = stage == "shade", stage in ("hard_shadow", "hard_path")
        rec = np.ascontiguousarray(records, dtype=self.STAGE_RECORDS[kind])
        a = abi.StageArgs()
        a.stage = code
        a.flags = ((0 if prune else abi.ACN_STAGE_NO_PRUNE) | (0 if leaf_lights else abi.ACN_STAGE_NO_LEAF_LIGHTS)
                   | (0 if emit_terms else abi.ACN_STAGE_NO_EMIT_TERMS) | (abi.ACN_STAGE_COUNT_WORK if count_work else 0))
        a.cls, a.shard_rank, a.shard_world, a.n = int(grid if hard else cls), int(shard_rank), int(shard_world), rec.shape[0]
        a.input = rec.ctypes.data
        ix = None
        if shade:
            ix = np.ascontiguousarray(np.arange(rec.shape[0]) if index is None else index, dtype=np.uint32)
            a.index, a.n_index = ix.ctypes.data, ix.shape[0]
        caps = abi.StageCaps()
        check(hip.acn_stage_plan(self.h, C.byref(a), C.byref(caps)), "acn_stage_plan")
        R = self.STAGE_RECORDS
        bufs = {"counts": np.zeros(info["counter_words"], dtype=np.uint32), "accum": np.zeros((rec.shape[0], 3), dtype=np.int64)}
        if stage != "hard_path":
            bufs["hard_shadow"] = np.zeros(max(caps.cap_hard_shadow, 1), dtype=R["hard_shadow"])
        if shade or stage == "hard_path":
            bufs["children"] = np.zeros(max(caps.cap_children, 1), dtype=R["hit"])
        if shade:
            bufs["hard_path"] = np.zeros(max(caps.cap_hard_path, 1), dtype=R["hard_path"])
        elif not hard:
            bufs["tasks"] = np.zeros(max(caps.cap_tasks, 1), dtype=R["task"])
            bufs["rays"] = np.zeros(max(caps.cap_rays, 1), dtype=R["ray"])
            idx = [np.zeros(max(caps.cap_tasks, 1), dtype=np.uint32) for _ in range(4)]
        o = abi.StageOut()
        for k, b in bufs.items():
            setattr(o, k, b.ctypes.data)
        if not shade and not hard:
            for k in range(4):
                o.idx[k] = idx[k].ctypes.data
        check(hip.acn_run_stage(self.h, C.byref(a), C.byref(o)), "acn_run_stage")
        c = bufs["counts"]
        live = lambda q, mark: q[:mark][q["pixel"][:mark] != self.STAGE_INVALID]   # noqa: E731
        res = {"counts": c, "flags": int(c[self.QC["flags"]]), "accum": bufs["accum"], "caps": caps}
        if count_work:
            res["counters"] = self.stage_last_counters()
        if not hard:
            res["hard_shadow"] = live(bufs["hard_shadow"], c[self.QC["hard_shadow"]])
        elif stage == "hard_shadow":
            res["hard_shadow"] = bufs["hard_shadow"][:rec.shape[0]]   # slot for slot, as the kernel left it
        if shade or stage == "hard_path":
            res["children"] = live(bufs["children"], c[self.QC["children"]])
        if shade:
            res["hard_path"] = live(bufs["hard_path"], c[self.QC["hard_path"]])
        elif not hard:
            res["tasks"] = bufs["tasks"][:c[self.QC["tasks"]]]       # with the unused ends of reservations: reached through idx only
            res["rays"] = live(bufs["rays"], c[self.QC["gen0"]])
            res["idx"] = [l[:c[self.QC["class0"] + k]][l[:c[self.QC["class0"] + k]] != self.STAGE_INVALID] for k, l in enumerate(idx)]
        return res

    def run_stage_walk(self, rays=None, pos_xy=None, n=None, first_pixel=0, room_rays=None, passes=1, private_limit=0xFFFFFFFF, stack_cap=512,
                       stack_use=0, fetch=64, grid=0, prune=True, lds=True, emit_terms=True, flags=None, count_work=False):
        """The specular walk of one path level alone (acn_run_stage_walk): `passes` launches of k_walk as the pipeline runner enqueues
        them.  rays: "ray" records (pixel = own index, or STAGE_INVALID), generation 0 of the level; or the camera form: pos_xy [n, 2],
        or n pixel centres of the raster from first_pixel.  room_rays: the rays the walk traces in all, by the caller's model.  Returns
        tasks, idx (four lists), hard_shadow (the probes), counts, flags, accum [n, 3] int64, and rays: what the last pass left for a
        generation no launch reads (dead slots taken out), and gen: the generation marks QC_GEN + 0 .. passes.  count_work: the
        counting variant of k_walk runs, and "counters" holds the work counters of all passes under the names of last_counters."""
        info = self.stage_info()
        R = self.STAGE_RECORDS
        for k, dt in R.items():
            assert dt.itemsize == info["sizeof"][k], (k, dt.itemsize, info["sizeof"][k])
        a = abi.StageWalkArgs()
        a.stage = abi.ACN_STAGE_WALK
        a.flags = ((0 if prune else abi.ACN_STAGE_NO_PRUNE) | (0 if lds else abi.ACN_STAGE_GLOBAL_NODES)
                   | (0 if emit_terms else abi.ACN_STAGE_NO_EMIT_TERMS)) if flags is None else int(flags)
        a.flags |= abi.ACN_STAGE_COUNT_WORK if count_work else 0
        rec = pos = None
        if rays is not None:
            rec = np.ascontiguousarray(rays, dtype=R["ray"])
            a.n, a.input = rec.shape[0], rec.ctypes.data
        if pos_xy is not None:
            pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
            a.pos_xy = pos.ctypes.data
        if rays is None:
            a.n = pos.shape[0] if pos is not None else int(n or 0)
        a.camera = 1 if (pos_xy is not None or n is not None) else 0
        a.first_pixel = int(first_pixel)
        a.passes, a.private_limit, a.stack_cap, a.stack_use, a.fetch, a.grid = int(passes), int(private_limit), int(stack_cap), int(stack_use), int(fetch), int(grid)
        a.room_rays = int(a.n if room_rays is None else room_rays)
        caps = abi.StageCaps()
        check(hip.acn_stage_walk_plan(self.h, C.byref(a), C.byref(caps)), "acn_stage_walk_plan")
        bufs = {"counts": np.zeros(info["counter_words"], dtype=np.uint32), "accum": np.zeros((a.n, 3), dtype=np.int64),
                "hard_shadow": np.zeros(caps.cap_hard_shadow, dtype=R["hard_shadow"]), "tasks": np.zeros(caps.cap_tasks, dtype=R["task"]),
                "rays": np.zeros(caps.cap_rays, dtype=R["ray"])}
        idx = [np.zeros(caps.cap_tasks, dtype=np.uint32) for _ in range(4)]
        o = abi.StageOut()
        for k, b in bufs.items():
            setattr(o, k, b.ctypes.data)
        for k in range(4):
            o.idx[k] = idx[k].ctypes.data
        check(hip.acn_run_stage_walk(self.h, C.byref(a), C.byref(o)), "acn_run_stage_walk")
        c = bufs["counts"]
        live = lambda q, mark: q[:mark][q["pixel"][:mark] != self.STAGE_INVALID]   # noqa: E731
        gen = c[self.QC["gen0"]:self.QC["gen0"] + a.passes + 1].copy()
        res = {"counts": c, "flags": int(c[self.QC["flags"]]), "accum": bufs["accum"], "caps": caps, "gen": gen,
               "hard_shadow": live(bufs["hard_shadow"], c[self.QC["hard_shadow"]]), "tasks": bufs["tasks"][:c[self.QC["tasks"]]],
               "rays": live(bufs["rays"], gen[a.passes]),
               "idx": [l[:c[self.QC["class0"] + k]][l[:c[self.QC["class0"] + k]] != self.STAGE_INVALID] for k, l in enumerate(idx)]}
        if count_work:
            res["counters"] = self.stage_last_counters()
        return res


class Surface:
    """Named views over the [n,16] float64 records of a surface call (include/actinon_hip.h, acn_surface_rays)."""

    def __init__(self, raw):
        raw = np.asarray(raw, dtype=np.float64)
        if raw.ndim != 2 or raw.shape[1] != abi.ACN_SURF_STRIDE:
            raise ValueError(f"surface records are [n,{abi.ACN_SURF_STRIDE}] float64, got {raw.shape}")
        self.raw = raw

    def __len__(self):
        return self.raw.shape[0]

    distance = property(lambda self: self.raw[:, 0])
    position = property(lambda self: self.raw[:, 1:4])
    exit_normal = property(lambda self: self.raw[:, 4:7])
    normal = property(lambda self: -self.raw[:, 4:7])          # the normal that faces the viewer
    enter = property(lambda self: self.raw[:, 7].astype(np.int64))
    exit = property(lambda self: self.raw[:, 8].astype(np.int64))
    albedo = property(lambda self: self.raw[:, 9:12])
    kind = property(lambda self: self.raw[:, 12].astype(np.int64))
    hops = property(lambda self: self.raw[:, 13].astype(np.int64))
    weight = property(lambda self: self.raw[:, 14])
    coverage = property(lambda self: self.raw[:, 15])          # 0 in a pinhole record; the dominant class's share in an aggregate
    hit = property(lambda self: self.raw[:, 0] < np.inf)


class LensStats:
    """Named views over the [n,8] float64 records of a lens statistics call (include/actinon_hip.h, ACN_STATS_STRIDE).  `handle`
    (optional) is the Handle that resolves them: .noise is computed by acn_lens_stats_resolve_dev on the device."""

    def __init__(self, raw, handle=None):
        raw = np.asarray(raw, dtype=np.float64)
        if raw.ndim != 2 or raw.shape[1] != abi.ACN_STATS_STRIDE:
            raise ValueError(f"lens statistics are [n,{abi.ACN_STATS_STRIDE}] float64, got {raw.shape}")
        self.raw = raw
        self.handle = handle

    def __len__(self):
        return self.raw.shape[0]

    n = property(lambda self: self.raw[:, 0])
    mean = property(lambda self: self.raw[:, 1:4])
    m2 = property(lambda self: self.raw[:, 4:7])
    empty = property(lambda self: ~(np.isfinite(self.raw[:, 0]) & (self.raw[:, 0] >= 1)))

    @property
    def variance_of_mean(self):
        """( m2 / ( n - 1 ) ) / n per channel; NaN where n <= 1 or the record is EMPTY"""
        n = self.raw[:, 0:1]
        with np.errstate(all="ignore"):
            vm = (self.raw[:, 4:7] / (n - 1.0)) / n
        return np.where((n > 1) & ~self.empty[:, None], vm, np.nan)

    @property
    def noise(self):
        if self.handle is None:
            raise AcnError(abi.ACN_ERR_ARG, "LensStats.noise is resolved on the device: construct it with a Handle")
        return self.handle.lens_stats_resolve(self.raw, linear=True)[1]


class Frame:
    """A device-resident frame of a handle (acn_frame_*): the accumulator of the gradient cycles in the layout of acn_lum.  Made by
    Handle.frame(); the handle must outlive it (closing the handle releases its frames)."""

    def __init__(self, handle, width, height):
        self.handle, self.width, self.height = handle, int(width), int(height)
        self.f = C.c_void_p()
        check(hip.acn_frame_create(handle.h, self.width, self.height, C.byref(self.f)), "acn_frame_create")

    def close(self):
        """Releases the frame (acn_frame_free), unless its handle is closed already and took it along."""
        if getattr(self, "f", None) and self.f.value:
            if self.handle.h.value:
                hip.acn_frame_free(self.f)
            self.f = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def upload(self, lum):
        """lum [h*w,6] float64: pos_x pos_y clr[3] weight per pixel, what a recovery file holds; drops a plan"""
        a = np.ascontiguousarray(lum, dtype=np.float64)
        if a.size != self.width * self.height * 6:
            raise ValueError(f"a frame of {self.width} x {self.height} has {self.width * self.height} records of 6, got {a.size} words")
        check(hip.acn_frame_upload(self.f, a.ctypes.data), "acn_frame_upload")

    def download(self):
        out = np.empty((self.width * self.height, 6), dtype=np.float64)
        check(hip.acn_frame_download(self.f, out.ctypes.data), "acn_frame_download")
        return out

    def main_pass(self):
        """The pixel centres of every pixel planned, rendered and pushed (cycle 0 of the render driver)."""
        o = self.handle._opts(False, None)
        check(hip.acn_frame_main_pass(self.f, C.byref(o)), "acn_frame_main_pass")

    def plan(self, sqr_threshold, samples, rval):
        """Key, selection and positions of one gradient pass -> ( flagged pixels, rval after the pass's draws )"""
        flagged, out = C.c_uint64(0), C.c_uint64(0)
        check(hip.acn_frame_plan(self.f, float(sqr_threshold), int(samples), int(rval), C.byref(flagged), C.byref(out)), "acn_frame_plan")
        return int(flagged.value), int(out.value)

    def render(self):
        o = self.handle._opts(False, None)
        check(hip.acn_frame_render(self.f, C.byref(o)), "acn_frame_render")

    def push(self):
        check(hip.acn_frame_push(self.f), "acn_frame_push")

    def gradient_pass(self, sqr_threshold, samples, rval):
        """plan + render + push (acn_frame_pass) -> ( flagged pixels, rval after the pass )"""
        flagged, rv = C.c_uint64(0), C.c_uint64(int(rval))
        o = self.handle._opts(False, None)
        check(hip.acn_frame_pass(self.f, float(sqr_threshold), int(samples), C.byref(rv), C.byref(flagged), C.byref(o)), "acn_frame_pass")
        return int(flagged.value), int(rv.value)

    def image(self, rgb=True, rgb8=True):
        """-> ( averages [h*w,3] float64 or None, their 8-bit values [h*w,3] uint8 or None )"""
        n = self.width * self.height
        a = np.empty((n, 3), dtype=np.float64) if rgb else None
        b = np.empty((n, 3), dtype=np.uint8) if rgb8 else None
        check(hip.acn_frame_image(self.f, a.ctypes.data if rgb else None, b.ctypes.data if rgb8 else None), "acn_frame_image")
        return a, b

    def view(self):
        """abi.FrameBuffers: the device pointers of the frame's buffers and the counts of its plan, as they are now"""
        b = abi.FrameBuffers()
        b.struct_size = C.sizeof(abi.FrameBuffers)
        check(hip.acn_frame_view(self.f, C.byref(b)), "acn_frame_view")
        return b


def lcg00_jump(rval, draws):
    """rval after `draws` steps of the position generator (acn_lcg00_jump).  No GPU."""
    return int(hip.acn_lcg00_jump(int(rval) & (2 ** 64 - 1), int(draws) & (2 ** 64 - 1)))


def main_pass_positions(width, height, first=0, count=None):
    """Pixel centres of the main pass, row-major (scene.c:1110-1119)."""
    n = width * height if count is None else count
    idx = np.arange(first, first + n)
    pos = np.empty((n, 2), dtype=np.float64)
    pos[:, 0] = (idx % width) + 0.5
    pos[:, 1] = (idx // width) + 0.5
    return pos


def key_hist_edge(bin):
    """The lower edge of bin `bin` of acn_key_histogram (acn_key_hist_edge): -inf for bin 0, NaN above 255.  No GPU."""
    return float(hip.acn_key_hist_edge(int(bin)))


def key_hist_threshold(hist, budget):
    """The threshold above which at most `budget` of the keys behind `hist` (uint64 [257]) lie (acn_key_hist_threshold): the edge
    of the lowest bin from which upward the counts fit the budget, +inf if none does.  No GPU."""
    hh = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    if hh.shape[0] != abi.ACN_KEY_HIST_WORDS:
        raise ValueError(f"a key histogram has {abi.ACN_KEY_HIST_WORDS} words, got {hh.shape[0]}")
    return float(hip.acn_key_hist_threshold(hh.ctypes.data, int(budget)))


def motion_from_scenes(prev_flat, cur_flat, moved_max_history=None):
    """The motion table of two flat scenes, prev_flat one frame before cur_flat (acn_motion_from_scenes): per node of cur_flat where a
    point of that object was one frame ago -> ( table [n_nodes,16], report: rows `rest`, `moved`, `none` and `same_shape` ).
    moved_max_history: the history cap of the rows that moved, None for the call's own.  No GPU."""
    table = np.empty((cur_flat.c.n_nodes, abi.ACN_MOTION_STRIDE), dtype=np.float64)
    rep = abi.MotionReport()
    check(hip.acn_motion_from_scenes(C.byref(prev_flat.c), C.byref(cur_flat.c), 0.0 if moved_max_history is None else float(moved_max_history),
                                     table.ctypes.data, C.byref(rep)), "acn_motion_from_scenes")
    return table, dict(rest=int(rep.n_rest), moved=int(rep.n_moved), none=int(rep.n_none), same_shape=bool(rep.same_shape))


def cps_from_cl(rgb):
    """8-bit quantisation of scene.c:76-82 on an [...,3] array."""
    rgb = np.asarray(rgb)
    q = np.where(rgb > 0.0, np.where(rgb < 1.0, (rgb * 256).astype(np.int64), 255), 0)
    return q.astype(np.uint8)


def device_count():
    return hip.acn_device_count()


def detmath_eval(op, x, y=None, device=0):
    ops = {"sin": 0, "cos": 1, "tan": 2, "acos": 3, "log": 4, "exp": 5, "pow": 6, "sqrt": 7, "div": 8, "u64_to_f64": 9,
           "frexp_mant": 10, "asin": 11, "atan": 12, "atan2": 13, "llrint": 14}
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    yp = None
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float64)
        yp = y.ctypes.data
    check(hip.acn_detmath_eval(device, ops[op], x.ctypes.data, yp, out.ctypes.data, x.size), "acn_detmath_eval")
    return out
