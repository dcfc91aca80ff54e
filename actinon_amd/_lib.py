"""Loads the two product libraries. There is NO fallback: a missing libactinon_hip.so is an ImportError, and a
render call without a GPU fails with ACN_ERR_DEVICE from the library itself."""
import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# ACN_LIBDIR: an alternative build of the two libraries (kernel variants under test); default: actinon_amd/lib
LIBDIR = os.environ.get("ACN_LIBDIR") or os.path.join(_HERE, "lib")


def _load(name):
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `make` (or __graft_entry__.build()); "
                          "actinon_amd has no pure-Python or CPU rendering path")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


hip = _load("libactinon_hip.so")
host = _load("libactinon_host.so")

# symbols declared by include/actinon_hip.h
HIP_SYMBOLS = ["acn_device_count", "acn_scene_upload", "acn_scene_free", "acn_scene_replace", "acn_scene_set_params", "acn_scene_info",
               "acn_render_positions",
               "acn_render_positions_dev", "acn_render_main_pass_dev", "acn_resolve_dev", "acn_last_kernel_ms", "acn_last_stage_ms", "acn_last_counters",
               "acn_estimate_envelope", "acn_detmath_eval", "acn_last_error", "acn_shard_tile_count", "acn_shard_tile_padded",
               "acn_shard_tile_index", "acn_render_main_pass_shard_dev", "acn_shard_unpack_dev", "acn_query_rays",
               "acn_stage_info", "acn_stage_plan", "acn_run_stage", "acn_stage_walk_plan", "acn_run_stage_walk", "acn_stage_last_counters",
               "acn_render_rays", "acn_render_rays_dev", "acn_camera_rays", "acn_camera_rays_dev",
               "acn_surface_rays", "acn_surface_rays_dev", "acn_surface_positions", "acn_surface_positions_dev",
               "acn_denoise", "acn_denoise_dev",
               "acn_lens_rays", "acn_lens_rays_dev", "acn_render_lens", "acn_render_lens_dev", "acn_render_lens_main_pass_dev",
               "acn_render_lens_stats", "acn_render_lens_stats_dev", "acn_render_lens_stats_main_pass_dev", "acn_lens_stats_merge",
               "acn_lens_stats_merge_dev", "acn_lens_stats_resolve_dev", "acn_denoise_stats", "acn_denoise_stats_dev",
               "acn_fill_stats", "acn_fill_stats_dev",
               "acn_select_above", "acn_select_above_dev", "acn_key_histogram", "acn_key_histogram_dev", "acn_key_hist_edge",
               "acn_key_hist_threshold",
               "acn_surface_reduce", "acn_surface_reduce_dev", "acn_surface_lens", "acn_surface_lens_dev", "acn_surface_lens_main_pass_dev",
               "acn_lens_layers_reduce", "acn_lens_layers_reduce_dev", "acn_render_lens_layers", "acn_render_lens_layers_dev",
               "acn_render_lens_layers_main_pass_dev", "acn_denoise_layers", "acn_denoise_layers_dev",
               "acn_lens_layers_merge", "acn_lens_layers_merge_dev", "acn_lens_layers_resolve_dev",
               "acn_project_points", "acn_project_points_dev", "acn_reproject", "acn_reproject_dev",
               "acn_reproject_moving", "acn_reproject_moving_dev", "acn_motion_from_scenes",
               "acn_shadow_records", "acn_shadow_records_dev", "acn_shadow_limit_history", "acn_shadow_limit_history_dev",
               "acn_frame_create", "acn_frame_free", "acn_frame_upload", "acn_frame_download", "acn_frame_main_pass", "acn_frame_plan",
               "acn_frame_render", "acn_frame_push", "acn_frame_pass", "acn_frame_image", "acn_frame_view", "acn_lcg00_jump"]
# symbols declared by include/acn_scene.h
HOST_SYMBOLS = ["acn_rotx", "acn_roty", "acn_rotz", "acn_obj_plane_s_create", "acn_obj_sphere_s_create",
                "acn_obj_squaroid_s_create_squaroid", "acn_obj_squaroid_s_create_ellipsoid",
                "acn_obj_squaroid_s_create_hyperboloid1", "acn_obj_squaroid_s_create_hyperboloid2",
                "acn_obj_squaroid_s_create_cone", "acn_obj_squaroid_s_create_cylinder", "acn_obj_torus_create", "acn_obj_distance_s_create", "acn_obj_set_distance_function",
                "acn_obj_pair_inside_s_create_pair", "acn_obj_pair_outside_s_create_pair", "acn_obj_neg_s_create_neg",
                "acn_obj_scale_s_create_scale", "acn_create_inside_composite", "acn_create_outside_composite",
                "acn_obj_clone", "acn_obj_discard", "acn_obj_type", "acn_obj_move", "acn_obj_rotate", "acn_obj_scale",
                "acn_obj_set_color", "acn_obj_set_transparency", "acn_obj_set_refractive_index", "acn_obj_set_radiance",
                "acn_obj_set_fresnel_reflectivity", "acn_obj_set_chromatic_reflectivity",
                "acn_obj_set_diffuse_reflectivity", "acn_obj_set_sigma", "acn_obj_set_surface_roughness",
                "acn_obj_set_material", "acn_obj_set_texture_field_plain", "acn_obj_set_texture_field_chess",
                "acn_obj_clear_texture_field", "acn_obj_set_envelope", "acn_obj_set_auto_envelope", "acn_obj_radiance",
                "acn_obj_get_envelope", "acn_compound_s_create", "acn_compound_s_push", "acn_compound_s_get_size",
                "acn_compound_s_clear", "acn_compound_s_set_sphere_envelopes", "acn_scene_s_create",
                "acn_scene_s_discard", "acn_scene_s_clear", "acn_scene_s_push", "acn_scene_s_objects",
                "acn_scene_s_flatten", "acn_flat_scene_free", "acn_obj_flatten", "acn_lum_machine_s_run",
                "acn_scene_s_create_image_file", "acn_scene_s_create_image_file_keep", "acn_write_pnm", "acn_write_pnm8", "acn_cps_from_cl", "acn_scene_primitives",
                "acn_scene_wine_glass", "acn_scene_diamond", "acn_scene_many_spheres", "acn_obj_get_pos",
                "acn_obj_sphere_s_get_radius", "acn_obj_get_field", "acn_obj_set_field", "acn_set_envelope_estimator"]
# symbols declared by include/acn_interp.h
INTERP_SYMBOLS = ["acn_interpret_file", "acn_interpret_string", "acn_interp_last_error", "acn_scene_from_script",
                  "acn_scene_s_clone"]

P = C.POINTER
vp = C.c_void_p

hip.acn_device_count.restype = C.c_int
hip.acn_scene_upload.argtypes = [P(abi.FlatScene), C.c_int, P(vp)]
hip.acn_scene_free.argtypes = [vp]
hip.acn_scene_free.restype = None
hip.acn_scene_replace.argtypes = [vp, P(abi.FlatScene), C.c_uint32]
hip.acn_scene_set_params.argtypes = [vp, P(abi.Params)]
hip.acn_scene_info.argtypes = [vp, P(C.c_uint64), C.c_int]
hip.acn_render_positions.argtypes = [vp, vp, C.c_size_t, vp, P(abi.RenderOpts)]
hip.acn_render_positions_dev.argtypes = [vp, vp, C.c_size_t, vp, P(abi.RenderOpts)]
hip.acn_render_main_pass_dev.argtypes = [vp, C.c_size_t, C.c_size_t, vp, P(abi.RenderOpts)]
hip.acn_render_rays.argtypes = [vp, vp, C.c_size_t, vp, P(abi.RenderOpts)]
hip.acn_render_rays_dev.argtypes = [vp, vp, C.c_size_t, vp, P(abi.RenderOpts)]
hip.acn_camera_rays.argtypes = [vp, vp, C.c_size_t, vp]
hip.acn_camera_rays_dev.argtypes = [vp, vp, C.c_size_t, vp, P(abi.RenderOpts)]
for _n in ["acn_surface_rays", "acn_surface_rays_dev", "acn_surface_positions", "acn_surface_positions_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, P(abi.RenderOpts)]
for _n in ["acn_denoise", "acn_denoise_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, P(abi.DenoiseParams), vp, P(abi.RenderOpts)]
hip.acn_lens_rays.argtypes = [vp, vp, C.c_size_t, P(abi.LensParams), C.c_uint32, C.c_uint32, vp]
hip.acn_lens_rays_dev.argtypes = [vp, vp, C.c_size_t, P(abi.LensParams), C.c_uint32, C.c_uint32, vp, P(abi.RenderOpts)]
hip.acn_render_lens.argtypes = [vp, vp, C.c_size_t, P(abi.LensParams), vp, P(abi.RenderOpts)]
hip.acn_render_lens_dev.argtypes = [vp, vp, C.c_size_t, P(abi.LensParams), vp, P(abi.RenderOpts)]
hip.acn_render_lens_main_pass_dev.argtypes = [vp, C.c_size_t, C.c_size_t, P(abi.LensParams), vp, P(abi.RenderOpts)]
hip.acn_render_lens_stats.argtypes = [vp, vp, C.c_size_t, P(abi.LensParams), vp, vp, P(abi.RenderOpts)]
hip.acn_render_lens_stats_dev.argtypes = [vp, vp, C.c_size_t, P(abi.LensParams), vp, vp, P(abi.RenderOpts)]
hip.acn_render_lens_stats_main_pass_dev.argtypes = [vp, C.c_size_t, C.c_size_t, P(abi.LensParams), vp, vp, P(abi.RenderOpts)]
for _n in ["acn_lens_stats_merge", "acn_lens_stats_merge_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, P(abi.RenderOpts)]
hip.acn_lens_stats_resolve_dev.argtypes = [vp, vp, C.c_size_t, vp, vp, P(abi.RenderOpts)]
for _n in ["acn_denoise_stats", "acn_denoise_stats_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, P(abi.DenoiseParams), vp, P(abi.RenderOpts)]
for _n in ["acn_fill_stats", "acn_fill_stats_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, P(abi.FillParams), vp, vp, P(abi.RenderOpts)]
for _n in ["acn_surface_reduce", "acn_surface_reduce_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, P(abi.RenderOpts)]
for _n in ["acn_surface_lens", "acn_surface_lens_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, C.c_size_t, P(abi.LensParams), C.c_uint32, vp, P(abi.RenderOpts)]
hip.acn_surface_lens_main_pass_dev.argtypes = [vp, C.c_size_t, C.c_size_t, P(abi.LensParams), C.c_uint32, vp, P(abi.RenderOpts)]
for _n in ["acn_lens_layers_reduce", "acn_lens_layers_reduce_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, P(abi.RenderOpts)]
for _n in ["acn_render_lens_layers", "acn_render_lens_layers_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, C.c_size_t, P(abi.LensParams), C.c_uint32, vp, vp, vp, P(abi.RenderOpts)]
hip.acn_render_lens_layers_main_pass_dev.argtypes = [vp, C.c_size_t, C.c_size_t, P(abi.LensParams), C.c_uint32, vp, vp, vp, P(abi.RenderOpts)]
for _n in ["acn_denoise_layers", "acn_denoise_layers_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, P(abi.DenoiseParams), vp, P(abi.RenderOpts)]
for _n in ["acn_lens_layers_merge", "acn_lens_layers_merge_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, P(abi.RenderOpts)]
hip.acn_lens_layers_resolve_dev.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, P(abi.RenderOpts)]
hip.acn_project_points.argtypes = [vp, vp, C.c_size_t, vp, vp]
hip.acn_project_points_dev.argtypes = [vp, vp, C.c_size_t, vp, vp, P(abi.RenderOpts)]
for _n in ["acn_reproject", "acn_reproject_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, C.c_size_t, P(abi.Params), vp, vp, P(abi.ReprojectParams), vp, vp, P(abi.RenderOpts)]
for _n in ["acn_reproject_moving", "acn_reproject_moving_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, C.c_size_t, P(abi.Params), vp, vp, vp, C.c_size_t, P(abi.ReprojectParams), vp, vp, P(abi.RenderOpts)]
for _n in ["acn_shadow_records", "acn_shadow_records_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, C.c_size_t, P(abi.ShadowParams), vp, P(abi.RenderOpts)]
for _n in ["acn_shadow_limit_history", "acn_shadow_limit_history_dev"]:
    getattr(hip, _n).argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, P(abi.ShadowHistoryParams), vp, P(abi.RenderOpts)]
hip.acn_motion_from_scenes.argtypes =[P(abi.FlatScene), P(abi.FlatScene), C.c_double, vp, P(abi.MotionReport)]
hip.acn_select_above_dev.argtypes =[vp, vp, C.c_size_t, P(abi.SelectParams), vp, vp, vp, vp, P(C.c_uint64), P(abi.RenderOpts)]
hip.acn_select_above.argtypes = [vp, vp, C.c_size_t, P(abi.SelectParams), vp, vp, vp, P(C.c_uint64)]
hip.acn_key_histogram_dev.argtypes = [vp, vp, C.c_size_t, vp, P(abi.RenderOpts)]
hip.acn_key_histogram.argtypes = [vp, vp, C.c_size_t, vp]
hip.acn_key_hist_edge.argtypes = [C.c_uint32]
hip.acn_key_hist_edge.restype = C.c_double
hip.acn_key_hist_threshold.argtypes = [vp, C.c_uint64]
hip.acn_key_hist_threshold.restype = C.c_double
hip.acn_frame_create.argtypes = [vp, C.c_uint64, C.c_uint64, P(vp)]
hip.acn_frame_free.argtypes = [vp]
hip.acn_frame_free.restype = None
hip.acn_frame_upload.argtypes = [vp, vp]
hip.acn_frame_download.argtypes = [vp, vp]
hip.acn_frame_main_pass.argtypes = [vp, P(abi.RenderOpts)]
hip.acn_frame_plan.argtypes = [vp, C.c_double, C.c_uint64, C.c_uint64, P(C.c_uint64), P(C.c_uint64)]
hip.acn_frame_render.argtypes = [vp, P(abi.RenderOpts)]
hip.acn_frame_push.argtypes = [vp]
hip.acn_frame_pass.argtypes = [vp, C.c_double, C.c_uint64, P(C.c_uint64), P(C.c_uint64), P(abi.RenderOpts)]
hip.acn_frame_image.argtypes = [vp, vp, vp]
hip.acn_frame_view.argtypes = [vp, P(abi.FrameBuffers)]
hip.acn_lcg00_jump.argtypes = [C.c_uint64, C.c_uint64]
hip.acn_lcg00_jump.restype = C.c_uint64
hip.acn_resolve_dev.argtypes = [vp, vp, C.c_size_t, vp, vp, P(abi.RenderOpts)]
hip.acn_last_kernel_ms.argtypes = [vp, P(C.c_double)]
hip.acn_last_stage_ms.argtypes = [vp, P(C.c_double), C.c_int]
hip.acn_last_counters.argtypes = [vp, P(C.c_uint64), C.c_int]
hip.acn_estimate_envelope.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint32, C.c_double, P(C.c_double)]
hip.acn_detmath_eval.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_size_t]
hip.acn_query_rays.argtypes = [vp, C.c_int, C.c_int32, vp, C.c_size_t, vp, vp]
hip.acn_stage_info.argtypes = [vp, vp, C.c_int]
hip.acn_stage_plan.argtypes = [vp, P(abi.StageArgs), P(abi.StageCaps)]
hip.acn_run_stage.argtypes = [vp, P(abi.StageArgs), P(abi.StageOut)]
hip.acn_stage_walk_plan.argtypes = [vp, P(abi.StageWalkArgs), P(abi.StageCaps)]
hip.acn_run_stage_walk.argtypes = [vp, P(abi.StageWalkArgs), P(abi.StageOut)]
hip.acn_stage_last_counters.argtypes = [vp, P(C.c_uint64), C.c_int]
hip.acn_last_error.restype = C.c_char_p
hip.acn_shard_tile_count.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32]
hip.acn_shard_tile_count.restype = C.c_size_t
hip.acn_shard_tile_padded.argtypes = [C.c_size_t, C.c_uint32]
hip.acn_shard_tile_padded.restype = C.c_size_t
hip.acn_shard_tile_index.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32, C.c_size_t]
hip.acn_shard_tile_index.restype = C.c_size_t
hip.acn_render_main_pass_shard_dev.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, vp, P(abi.RenderOpts)]
hip.acn_shard_unpack_dev.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, P(abi.RenderOpts)]

for _n in ["acn_rotx", "acn_roty", "acn_rotz"]:
    getattr(host, _n).argtypes = [C.c_double]
    getattr(host, _n).restype = abi.M3
for _n in ["acn_obj_plane_s_create", "acn_compound_s_create", "acn_scene_primitives", "acn_scene_wine_glass",
           "acn_scene_diamond"]:
    getattr(host, _n).restype = vp
host.acn_scene_s_create.restype = P(abi.SceneStruct)
host.acn_scene_many_spheres.argtypes = [C.c_int, C.c_int]
host.acn_scene_many_spheres.restype = vp
host.acn_obj_sphere_s_create.argtypes = [C.c_double]
host.acn_obj_sphere_s_create.restype = vp
host.acn_obj_squaroid_s_create_squaroid.argtypes = [C.c_double] * 4
host.acn_obj_squaroid_s_create_squaroid.restype = vp
for _n in ["ellipsoid", "hyperboloid1", "hyperboloid2", "cone"]:
    f = getattr(host, "acn_obj_squaroid_s_create_" + _n)
    f.argtypes = [C.c_double] * 3
    f.restype = vp
host.acn_obj_squaroid_s_create_cylinder.argtypes = [C.c_double] * 2
host.acn_obj_squaroid_s_create_cylinder.restype = vp
host.acn_obj_torus_create.argtypes = [C.c_double] * 2
host.acn_obj_torus_create.restype = vp
host.acn_obj_distance_s_create.argtypes = []
host.acn_obj_distance_s_create.restype = vp
host.acn_obj_set_distance_function.argtypes = [vp, C.c_int, C.c_double]
host.acn_obj_set_distance_function.restype = C.c_int
for _n in ["acn_obj_pair_inside_s_create_pair", "acn_obj_pair_outside_s_create_pair"]:
    getattr(host, _n).argtypes = [vp, vp]
    getattr(host, _n).restype = vp
host.acn_obj_neg_s_create_neg.argtypes = [vp]
host.acn_obj_neg_s_create_neg.restype = vp
host.acn_obj_scale_s_create_scale.argtypes = [vp, abi.V3]
host.acn_obj_scale_s_create_scale.restype = vp
for _n in ["acn_create_inside_composite", "acn_create_outside_composite"]:
    getattr(host, _n).argtypes = [P(vp), C.c_size_t]
    getattr(host, _n).restype = vp
host.acn_obj_clone.argtypes = [vp]
host.acn_obj_clone.restype = vp
host.acn_obj_discard.argtypes = [vp]
host.acn_obj_discard.restype = None
host.acn_obj_type.argtypes = [vp]
host.acn_obj_move.argtypes = [vp, abi.V3]
host.acn_obj_move.restype = None
host.acn_obj_rotate.argtypes = [vp, P(abi.M3)]
host.acn_obj_rotate.restype = None
host.acn_obj_scale.argtypes = [vp, C.c_double]
host.acn_obj_scale.restype = None
for _n in ["acn_obj_set_color", "acn_obj_set_transparency"]:
    getattr(host, _n).argtypes = [vp, abi.V3]
    getattr(host, _n).restype = None
for _n in ["refractive_index", "radiance", "fresnel_reflectivity", "chromatic_reflectivity", "diffuse_reflectivity",
           "sigma", "surface_roughness"]:
    f = getattr(host, "acn_obj_set_" + _n)
    f.argtypes = [vp, C.c_double]
    f.restype = None
host.acn_obj_set_texture_field_plain.argtypes = [vp, abi.V3]
host.acn_obj_set_texture_field_plain.restype = None
host.acn_obj_set_texture_field_chess.argtypes = [vp, abi.V3, abi.V3, C.c_double]
host.acn_obj_set_texture_field_chess.restype = None
host.acn_obj_clear_texture_field.argtypes = [vp]
host.acn_obj_clear_texture_field.restype = None
host.acn_obj_set_material.argtypes = [vp, C.c_char_p]
host.acn_obj_set_envelope.argtypes = [vp, abi.V3, C.c_double]
host.acn_obj_set_envelope.restype = None
host.acn_obj_set_auto_envelope.argtypes = [vp]
host.acn_obj_radiance.argtypes = [vp]
host.acn_obj_radiance.restype = C.c_double
host.acn_obj_get_envelope.argtypes = [vp, P(C.c_double)]
host.acn_compound_s_push.argtypes = [vp, vp]
host.acn_compound_s_push.restype = None
host.acn_compound_s_get_size.argtypes = [vp]
host.acn_compound_s_get_size.restype = C.c_size_t
host.acn_compound_s_clear.argtypes = [vp]
host.acn_compound_s_clear.restype = None
host.acn_compound_s_set_sphere_envelopes.argtypes = [vp, C.c_double]
host.acn_compound_s_set_sphere_envelopes.restype = None
host.acn_scene_s_discard.argtypes = [vp]
host.acn_scene_s_discard.restype = None
host.acn_scene_s_clear.argtypes = [vp]
host.acn_scene_s_clear.restype = None
host.acn_scene_s_push.argtypes = [vp, vp]
host.acn_scene_s_push.restype = C.c_size_t
host.acn_scene_s_objects.argtypes = [vp]
host.acn_scene_s_objects.restype = C.c_size_t
host.acn_scene_s_flatten.argtypes = [vp, P(abi.FlatScene)]
host.acn_obj_get_pos.argtypes = [vp, P(C.c_double)]
host.acn_obj_get_pos.restype = None
host.acn_obj_sphere_s_get_radius.argtypes = [vp]
host.acn_obj_sphere_s_get_radius.restype = C.c_double
host.acn_obj_get_field.argtypes = [vp, C.c_char_p, P(C.c_double)]
host.acn_obj_set_field.argtypes = [vp, C.c_char_p, C.c_double]
host.acn_set_envelope_estimator.argtypes = [vp]
host.acn_set_envelope_estimator.restype = None
CREATE_IMAGE_FN = C.CFUNCTYPE(C.c_int, vp, vp, C.c_char_p)


class InterpOpts(C.Structure):
    _fields_ = [("on_create_image", CREATE_IMAGE_FN), ("ctx", vp), ("auto_envelope", C.c_int), ("readonly_fs", C.c_int),
                ("argc", C.c_int),
                ("argv", P(C.c_char_p))]


host.acn_interpret_file.argtypes = [C.c_char_p, P(InterpOpts)]
host.acn_interpret_string.argtypes = [C.c_char_p, C.c_char_p, P(InterpOpts)]
host.acn_interp_last_error.restype = C.c_char_p
host.acn_scene_from_script.argtypes = [C.c_char_p, C.c_int]
host.acn_scene_from_script.restype = vp
host.acn_scene_s_clone.argtypes = [vp]
host.acn_scene_s_clone.restype = vp
host.acn_flat_scene_free.argtypes = [P(abi.FlatScene)]
host.acn_flat_scene_free.restype = None
host.acn_obj_flatten.argtypes = [vp, P(abi.FlatScene), P(C.c_int32)]
host.acn_lum_machine_s_run.argtypes = [vp, vp, C.c_size_t]
host.acn_scene_s_create_image_file.argtypes = [vp, C.c_char_p]
host.acn_scene_s_create_image_file_keep.argtypes = [vp, C.c_char_p, P(vp)]
host.acn_write_pnm.argtypes = [C.c_char_p, vp, C.c_size_t, C.c_size_t]
host.acn_write_pnm8.argtypes = [C.c_char_p, vp, C.c_size_t, C.c_size_t]
host.acn_cps_from_cl.argtypes = [P(C.c_double)]
host.acn_cps_from_cl.restype = C.c_uint32


class AcnError(RuntimeError):
    def __init__(self, status, where):
        msg = hip.acn_last_error()
        super().__init__(f"{where}: status {status} ({msg.decode() if msg else ''})")
        self.status = status


def check(status, where):
    if status != abi.ACN_OK:
        raise AcnError(status, where)
