"""ctypes mirror of include/actinon_hip.h and include/acn_scene.h (layout only, no logic)."""
import ctypes as C

ACN_ABI_VERSION = 2
ACN_OPT_LINEAR_OUT = 1
ACN_OPT_COUNT_WORK = 2
ACN_OPT_STAGE_TIMING = 4
ACN_SHARD_NONE, ACN_SHARD_SAMPLES = 0, 1
ACN_SHARD_TILE = 256
# surface records (acn_surface_*): doubles per record, modes, kind bits
ACN_SURF_STRIDE = 16
ACN_SURF_FIRST_HIT, ACN_SURF_FOLLOW = 0, 1
(ACN_SURF_EMITTER, ACN_SURF_DIFFUSE, ACN_SURF_CHROMATIC, ACN_SURF_FRESNEL, ACN_SURF_TRANSPARENT, ACN_SURF_LIGHT_ROOT,
 ACN_SURF_CUT) = 1, 2, 4, 8, 16, 32, 64

# the edge-avoiding filter (acn_denoise): flags, defaults and limits of acn_denoise_params
ACN_DENOISE_NO_DEMODULATE, ACN_DENOISE_NORMAL_POWER_SET = 1, 2
ACN_DENOISE_DEFAULT_ITERATIONS, ACN_DENOISE_DEFAULT_NORMAL_POWER_LOG2 = 5, 7
ACN_DENOISE_DEFAULT_SIGMA_PLANE, ACN_DENOISE_DEFAULT_SIGMA_LUM = 0.1, 4.0
ACN_DENOISE_MAX_ITERATIONS, ACN_DENOISE_MAX_NORMAL_POWER_LOG2 = 8, 10

# the thin-lens camera (acn_lens_rays, acn_render_lens): flags, defaults and limits of acn_lens_params
ACN_LENS_JITTER = 1
ACN_LENS_DEFAULT_SAMPLES, ACN_LENS_MAX_SAMPLES = 16, 4096
ACN_LENS_SEED = 2718281828

# lens sample statistics (acn_render_lens_stats, acn_lens_stats_*, acn_denoise_stats): doubles per record, the floor of `noise`
ACN_STATS_STRIDE = 8
ACN_STATS_NOISE_FLOOR = 0.01

# filling a sparse frame (acn_fill_stats): defaults and the limit of acn_fill_params; its flags are the two ACN_DENOISE_* above
ACN_FILL_DEFAULT_RADIUS, ACN_FILL_MAX_RADIUS = 3, 8
ACN_FILL_DEFAULT_SIGMA_PX, ACN_FILL_DEFAULT_SIGMA_PLANE = 1.5, 0.1

# layered lens records (acn_lens_layers_reduce, acn_render_lens_layers, acn_denoise_layers, acn_lens_layers_merge,
# acn_lens_layers_resolve_dev): planes of surface and statistics records
ACN_LAYERS_SURFACE_PLANES, ACN_LAYERS_STATS_PLANES = 2, 3

# selecting positions by a key (acn_select_above, acn_key_histogram): bins of the histogram, its words (the last counts NaN keys)
ACN_KEY_HIST_BINS, ACN_KEY_HIST_WORDS = 256, 257

# projecting points and reprojecting sample statistics (acn_project_points, acn_reproject): flags and defaults of acn_reproject_params
ACN_REPROJECT_KINDS_SET, ACN_REPROJECT_HOPS_SET = 1, 2
ACN_REPROJECT_DEFAULT_REJECT_KINDS = ACN_SURF_CHROMATIC | ACN_SURF_FRESNEL | ACN_SURF_TRANSPARENT | ACN_SURF_CUT
ACN_REPROJECT_DEFAULT_MAX_HOPS = 0
ACN_REPROJECT_DEFAULT_NORMAL_MIN, ACN_REPROJECT_DEFAULT_PLANE_TOLERANCE, ACN_REPROJECT_DEFAULT_MAX_HISTORY = 0.9, 0.01, 32.0

# reprojection through moving objects (acn_reproject_moving, acn_motion_from_scenes): doubles per row of the motion table, the states
ACN_MOTION_STRIDE = 16
ACN_MOTION_REST, ACN_MOTION_MOVED, ACN_MOTION_NONE = 0.0, 1.0, 2.0

# replacing the scene of a live handle (acn_scene_replace, acn_scene_info): the flag, the slots of the counters
ACN_REPLACE_FORGET = 1
ACN_INFO_N = 8

ACN_OK, ACN_ERR_ARG, ACN_ERR_UNSUPPORTED, ACN_ERR_NO_FOV, ACN_ERR_DEVICE, ACN_ERR_CANCELLED = 0, -1, -2, -3, -4, -5

NODE_TYPES = {1: "plane", 2: "sphere", 3: "squaroid", 4: "distance", 5: "pair_inside", 6: "pair_outside",
              7: "neg", 8: "scale", 9: "compound"}
ACN_PLANE, ACN_SPHERE, ACN_SQUAROID, ACN_DISTANCE, ACN_PAIR_INSIDE, ACN_PAIR_OUTSIDE, ACN_NEG, ACN_SCALE, ACN_COMPOUND = range(1, 10)
ACN_SDF_SPHERE, ACN_SDF_TORUS = 0, 1   # enum acn_sdf_kind
ACN_NODE_HAS_ENVELOPE = 1


class Node(C.Structure):
    _fields_ = [("type", C.c_int32), ("flags", C.c_uint32), ("child0", C.c_int32), ("child1", C.c_int32),
                ("sdf_kind", C.c_int32), ("cycles", C.c_int32), ("texture", C.c_int32), ("reserved", C.c_int32),
                ("pos", C.c_double * 3), ("rax", C.c_double * 9), ("env_pos", C.c_double * 3), ("env_radius", C.c_double),
                ("prm", C.c_double * 4), ("color", C.c_double * 3), ("radiance", C.c_double),
                ("refractive_index", C.c_double), ("fresnel_reflectivity", C.c_double),
                ("chromatic_reflectivity", C.c_double), ("diffuse_reflectivity", C.c_double), ("sigma", C.c_double),
                ("surface_roughness", C.c_double), ("transparency", C.c_double * 3), ("pad_", C.c_double)]


class Params(C.Structure):
    _fields_ = [("image_width", C.c_uint64), ("image_height", C.c_uint64), ("gamma", C.c_double),
                ("background_color", C.c_double * 3), ("camera_position", C.c_double * 3),
                ("camera_view_direction", C.c_double * 3), ("camera_top_direction", C.c_double * 3),
                ("camera_focal_length", C.c_double), ("trace_depth", C.c_uint64), ("trace_min_intensity", C.c_double),
                ("direct_samples", C.c_uint64), ("path_samples", C.c_uint64), ("max_path_length", C.c_double),
                ("experimental_level", C.c_int64)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("color1", C.c_double * 3), ("color2", C.c_double * 3),
                ("scale", C.c_double)]


class FlatScene(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_nodes", C.c_uint32), ("n_elems", C.c_uint32),
                ("light_root", C.c_int32), ("matter_root", C.c_int32), ("reserved", C.c_uint32),
                ("nodes", C.POINTER(Node)), ("elems", C.POINTER(C.c_int32)), ("params", Params),
                ("n_textures", C.c_uint32), ("reserved2", C.c_uint32), ("textures", C.POINTER(Texture))]


class RenderOpts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("struct_size", C.c_uint32), ("cancel", C.POINTER(C.c_int)), ("stream", C.c_void_p),
                ("shard_mode", C.c_uint32), ("shard_rank", C.c_uint32), ("shard_world", C.c_uint32), ("reserved2", C.c_uint32)]


class DenoiseParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32), ("flags", C.c_uint32),
                ("sigma_plane", C.c_double), ("sigma_lum", C.c_double)]


class FillParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_uint32), ("normal_power_log2", C.c_uint32), ("flags", C.c_uint32),
                ("sigma_px", C.c_double), ("sigma_plane", C.c_double)]


class LensParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("samples", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint32),
                ("aperture_radius", C.c_double), ("focus_distance", C.c_double)]


class SelectParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("threshold", C.c_double), ("capacity", C.c_uint64),
                ("raster_width", C.c_uint64), ("raster_first", C.c_uint64)]


class FrameBuffers(C.Structure):
    """acn_frame_buffers: what acn_frame_view reports of a device-resident frame"""
    _fields_ = [("struct_size", C.c_uint32), ("planned", C.c_uint32), ("width", C.c_uint64), ("height", C.c_uint64),
                ("flagged", C.c_uint64), ("samples", C.c_uint64), ("d_accumulator", C.c_void_p), ("d_key", C.c_void_p),
                ("d_index", C.c_void_p), ("d_positions", C.c_void_p), ("d_colours", C.c_void_p)]


class ReprojectParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("reject_kinds", C.c_uint32), ("max_hops", C.c_int32),
                ("normal_min", C.c_double), ("plane_tolerance", C.c_double), ("max_history", C.c_double)]


class MotionReport(C.Structure):
    _fields_ = [("n_rest", C.c_uint32), ("n_moved", C.c_uint32), ("n_none", C.c_uint32), ("same_shape", C.c_uint32)]


# shadow records and the history guard (acn_shadow_records, acn_shadow_limit_history): doubles per record, states, defaults, the flag
ACN_SHADOW_STRIDE = 16
ACN_SHADOW_NONE, ACN_SHADOW_SAMPLED = 0.0, 1.0
ACN_SHADOW_DEFAULT_SAMPLES, ACN_SHADOW_MAX_SAMPLES = 16, 64
ACN_SHADOW_HISTORY_DROP = 1
ACN_SHADOW_HISTORY_DEFAULT_TOLERANCE, ACN_SHADOW_HISTORY_DEFAULT_MAX_HISTORY = 0.25, 1.0


class ShadowParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("samples", C.c_uint32)]


class ShadowHistoryParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("tolerance", C.c_double), ("changed_max_history", C.c_double)]


# the stage-runner test seam (acn_run_stage): stages, option bits, limits
ACN_STAGE_SHADE_HITS, ACN_STAGE_SHADE, ACN_STAGE_HARD_SHADOW, ACN_STAGE_HARD_PATH = 0, 1, 2, 3
ACN_STAGE_NO_PRUNE, ACN_STAGE_NO_LEAF_LIGHTS, ACN_STAGE_NO_EMIT_TERMS = 1, 2, 4
ACN_STAGE_COUNT_WORK = 16       # both seams: the counting kernel variants; acn_stage_last_counters returns their work counters
ACN_STAGE_MAX_RECORDS, ACN_STAGE_MAX_SAMPLES, ACN_STAGE_MAX_DEPTH = 1 << 20, 1 << 16, 1 << 20
ACN_STAGE_INFO_WORDS = 10
# the walk of a level alone (acn_run_stage_walk)
ACN_STAGE_WALK, ACN_STAGE_GLOBAL_NODES, ACN_STAGE_WALK_MAX_STACK, ACN_MAX_WALK_PASSES = 4, 8, 4096, 32
QS_DEAD_HS = 24          # word of a level's counter block (csrc/acn_counts.h): dead slots k_hard_shadow stepped over


class StageArgs(C.Structure):
    _fields_ = [("stage", C.c_uint32), ("flags", C.c_uint32), ("cls", C.c_uint32), ("shard_rank", C.c_uint32), ("shard_world", C.c_uint32),
                ("n", C.c_uint32), ("n_index", C.c_uint32), ("pad", C.c_uint32), ("input", C.c_void_p), ("index", C.c_void_p)]


class StageWalkArgs(C.Structure):
    _fields_ = [("stage", C.c_uint32), ("flags", C.c_uint32), ("n", C.c_uint32), ("camera", C.c_uint32), ("passes", C.c_uint32),
                ("private_limit", C.c_uint32), ("stack_cap", C.c_uint32), ("stack_use", C.c_uint32), ("fetch", C.c_uint32), ("grid", C.c_uint32),
                ("room_rays", C.c_uint32), ("pad", C.c_uint32), ("input", C.c_void_p), ("pos_xy", C.c_void_p), ("first_pixel", C.c_uint64)]


class StageCaps(C.Structure):
    _fields_ = [("cap_tasks", C.c_uint32), ("cap_rays", C.c_uint32), ("cap_children", C.c_uint32), ("cap_hard_shadow", C.c_uint32),
                ("cap_hard_path", C.c_uint32), ("grid", C.c_uint32), ("chunk", C.c_uint32), ("pad", C.c_uint32)]


class StageOut(C.Structure):
    _fields_ = [("tasks", C.c_void_p), ("idx", C.c_void_p * 4), ("rays", C.c_void_p), ("children", C.c_void_p), ("hard_shadow", C.c_void_p),
                ("hard_path", C.c_void_p), ("counts", C.c_void_p), ("accum", C.c_void_p)]


class V3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class M3(C.Structure):
    _fields_ = [("x", V3), ("y", V3), ("z", V3)]


class SceneStruct(C.Structure):
    """struct acn_scene (include/acn_scene.h)"""
    _fields_ = [("threads", C.c_uint64), ("gradient_threshold", C.c_double), ("gradient_samples", C.c_uint64),
                ("gradient_cycles", C.c_uint64), ("prm", Params), ("light", C.c_void_p), ("matter", C.c_void_p),
                ("device", C.c_int)]


assert C.sizeof(Node) == 304, C.sizeof(Node)
assert C.sizeof(DenoiseParams) == 32, C.sizeof(DenoiseParams)
assert C.sizeof(FillParams) == 32, C.sizeof(FillParams)
assert C.sizeof(LensParams) == 32, C.sizeof(LensParams)
assert C.sizeof(SelectParams) == 40, C.sizeof(SelectParams)
assert C.sizeof(ReprojectParams) == 40, C.sizeof(ReprojectParams)
assert C.sizeof(ShadowParams) == 12, C.sizeof(ShadowParams)
assert C.sizeof(ShadowHistoryParams) == 24, C.sizeof(ShadowHistoryParams)
assert C.sizeof(FrameBuffers) == 80, C.sizeof(FrameBuffers)
assert C.sizeof(StageWalkArgs) == 72, C.sizeof(StageWalkArgs)
