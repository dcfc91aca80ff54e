/* acn_launch.h -- what the host passes to the kernels (SceneArgs, KernelFlags, LevelQ, WalkLaunch, the setups of the side kernels)
 * and the prototype of every launch wrapper, once.  No kernel template: the orchestrating units (actinon_hip.hip: the pipeline;
 * acn_calls.hip: the entry points beside it; k_stage.hip, k_query.hip) and the side kernels see the records (acn_records.h) alone.  The
 * pipeline kernels live in one header per family (acn_k_walk.h, acn_k_shade.h, acn_k_hard.h, over acn_queues.h), included by the
 * family's own units: one unit per family and size, so that `make -j` compiles the 58 instantiations (32 of k_shade, 8 each of k_walk,
 * k_hard_shadow and k_hard_path, 2 of k_shade_hits) side by side: about 3 minutes, 8.5 in one file.  Variants: acn_variant.h. */
#ifndef ACN_LAUNCH_H
#define ACN_LAUNCH_H

#include "acn_records.h"

/* what every pipeline kernel receives first (ACN_SCENE_PARAMS) */
struct SceneArgs
{
    DevScene dev;
    const GNode* nodes;
    const GMat* mats;
    const int32_t* elems;
    const acn_texture* textures;
    uint32_t elem_pos_base;   /* elems[ elem_pos_base + k ]: see root_occluded_rec (k_hard_shadow alone reads it: no DevScene field) */
};

/* variant selection.  The instrumented kernels (count) exist with and without the prune programs / in-line simple
 * compounds as well, so that a counted pass walks the traversal the timed pass walks */
struct KernelFlags { bool count, leaf_lights, lds_nodes, prune; };

/* the queues of one pipeline run (a handle's or a lane's workspace) as the kernels of path level L see them:
 * `counts` is the level's counter block, `prev_children` the QC_CHILDREN word of the level before */
struct LevelQ
{
    DTask* tasks; uint32_t* idx[ ACN_NCLASS ]; uint32_t task_cap;
    HitRec* children; uint32_t child_cap;
    HardShadow* hard_shadow; uint32_t hs_cap;               /* twice the other queues: it also takes the probes of the walk (probe_push) */
    HardPath* hard_path; uint32_t hard_cap;
    RayTask* rays[ 2 ]; uint32_t ray_cap;                   /* generation g of the walk waits in rays[ g & 1 ] */
    RayTask* stacks; uint32_t stack_cap;                    /* private ray stacks of the k_walk waves: grid * 4 of them */
    uint32_t stack_use;                                     /* slots of a stack every pass but the last uses (< stack_cap: tests) */
    uint32_t* counts;
    const uint32_t* prev_children;
    unsigned grid;                                          /* workgroups of k_shade_hits and the hard-ray kernels */
    unsigned shade_grid;                                    /* workgroups of k_shade */
    unsigned walk_grid;                                     /* workgroups of k_walk */
    uint32_t fetch_walk, fetch_hard;                        /* input items a wave reserves per cursor atomic */
    uint32_t fetch_shade;                                   /* k_shade: steps of 64 / LPT tasks a wave reserves per atomic */
    uint32_t private_limit;                                 /* generations of at most this many rays are finished on private stacks */
    uint32_t shard_rank, shard_world;                       /* ACN_SHARD_SAMPLES at level 0: the rank's share of the sample loops; else 0, 1 */
    uint32_t emit_terms;                                    /* 0: k_walk drops its pixel terms (level 0 of a rank > 0 of such a call) */
};

/* one launch of k_walk: pass `pass` of the specular walk of the level.  n_cam > 0 (pass 0 of level 0): the input are the camera rays
 * of positions [ base, base + n_cam ); else generation `pass` of the level's ray queues.  last: the input is finished on the private
 * stacks whatever its size. */
struct WalkLaunch
{
    uint32_t pass; bool last; const double* pos_xy; size_t first_pixel; uint32_t base, n_cam; TileOrder order; size_t lds_bytes;
    unsigned long long* accum; unsigned long long* counters;
};
/* acn_launch_walk launches its own instantiations or forwards down the chain of the k_walk units: _lds -> _count -> _count_prune, _lds -> _glb */
void acn_launch_walk( KernelFlags f, const LevelQ& q, const WalkLaunch& w, hipStream_t stream, const SceneArgs& s );
void acn_launch_walk_glb( KernelFlags f, const LevelQ& q, const WalkLaunch& w, hipStream_t stream, const SceneArgs& s );
void acn_launch_walk_count( KernelFlags f, const LevelQ& q, const WalkLaunch& w, hipStream_t stream, const SceneArgs& s );
void acn_launch_walk_count_prune( KernelFlags f, const LevelQ& q, const WalkLaunch& w, hipStream_t stream, const SceneArgs& s );
void acn_launch_shade_hits( bool count, const LevelQ& q, hipStream_t stream, const SceneArgs& s,
                            unsigned long long* accum, unsigned long long* counters );
/* k_shade, one wrapper per size class: it carries the class's lanes per task, the list it reads and its cursor */
void acn_launch_shade64( KernelFlags, const LevelQ&, hipStream_t, const SceneArgs&, unsigned long long*, unsigned long long* );
void acn_launch_shade16( KernelFlags, const LevelQ&, hipStream_t, const SceneArgs&, unsigned long long*, unsigned long long* );
void acn_launch_shade4( KernelFlags, const LevelQ&, hipStream_t, const SceneArgs&, unsigned long long*, unsigned long long* );
void acn_launch_shade1( KernelFlags, const LevelQ&, hipStream_t, const SceneArgs&, unsigned long long*, unsigned long long* );
void acn_launch_hard_shadow( KernelFlags f, const LevelQ& q, size_t lds_bytes, hipStream_t stream, const SceneArgs& s,
                             unsigned long long* accum, unsigned long long* counters );
void acn_launch_hard_path( KernelFlags f, const LevelQ& q, size_t lds_bytes, hipStream_t stream, const SceneArgs& s,
                           unsigned long long* accum, unsigned long long* counters );

/* caller-supplied primary rays (k_rays.hip).  rays: [ n ][ 6 ] origin, direction.
 * seed: slots [ base, base + cnt ) of the call's TileOrder -> generation 0 of the level's ray queue ( q.rays[ 0 ], the count
 * QC_GEN + 0 ), as k_walk would make them of camera rays; cnt <= q.ray_cap (no slot past it is written).
 * check: *first_bad = min( *first_bad, index of a ray with a non-finite component or a direction of no length ).
 * camera: out[ i ] = camera_ray( pos_xy[ i ] ), the rays k_walk casts for sample positions. */
void acn_launch_seed_rays( const double* rays, uint32_t base, uint32_t cnt, TileOrder order, int depth, const LevelQ& q, hipStream_t stream );
void acn_launch_check_rays( const double* rays, size_t n, unsigned long long* first_bad, hipStream_t stream );
void acn_launch_camera_rays( const DevScene& sc, const double* pos_xy, size_t n, double* out, hipStream_t stream );

/* surface records (k_surface.hip): one ray per lane, no queues.  mode: ACN_SURF_*.  Exactly one of rays ( [ n ][ 6 ] ) and pos_xy
 * ( [ n ][ 2 ], through camera_ray ) is given; out: [ n ][ ACN_SURF_STRIDE ].  lds_bytes: the staged nodes (lds_nodes) and the
 * CSG stacks, as the machine kernels get them.  s.dev.flags: the word that takes ACN_FLAG_STACK_OVERFLOW. */
void acn_launch_surface( uint32_t mode, bool lds_nodes, size_t lds_bytes, hipStream_t stream, const SceneArgs& s,
                         const double* rays, const double* pos_xy, size_t n, double* out );

/* shadow records and the history guard (k_shadow.hip; include/actinon_hip.h states both).  shadow: surface [ n ][ ACN_SURF_STRIDE ] -> out
 * [ n ][ ACN_SHADOW_STRIDE ], both 16-byte aligned, 1 << log2_samples <= 64 lanes per position; lds_bytes and s.dev.flags as for
 * acn_launch_surface; leaf_lights: KernelFlags.leaf_lights of the handle's scene.  limit_history: stats [ n ][ ACN_STATS_STRIDE ] in place,
 * motion [ n ][ 2 ], cur_shadow [ n ][ . ], prev_shadow [ height * width ][ . ], out_change (nullable) [ n ]; n >= 1.  ShadowHistorySetup:
 * acn_shadow_history_params after the host's checks, final values, no defaults. */
struct ShadowHistorySetup { uint32_t drop; double tolerance, cap; };
void acn_launch_shadow( bool lds_nodes, bool leaf_lights, size_t lds_bytes, hipStream_t stream, const SceneArgs& s, const double* surface,
                        size_t n, uint32_t log2_samples, double* out );
void acn_launch_shadow_limit_history( double* stats, const double* motion, const double* cur_shadow, const double* prev_shadow, size_t n,
                                      uint64_t width, uint64_t height, const ShadowHistorySetup& su, double* out_change, hipStream_t stream );

/* the filter of acn_denoise (k_denoise.hip): prepare, variance and one launch per level, the last of which writes out_rgb (which may
 * be lin).  scratch: ACN_DENOISE_SCRATCH_PER_PIXEL bytes per pixel, 128-byte aligned.  The parameters are final values, no defaults. */
#define ACN_DENOISE_SCRATCH_PER_PIXEL 128
void acn_launch_denoise( const double* lin, const double* surf, size_t width, size_t height, uint32_t iterations, uint32_t normal_power_log2,
                         uint32_t no_demodulate, double sigma_plane, double sigma_lum, void* scratch, double* out_rgb, hipStream_t stream );

/* the filter of acn_denoise_stats: steps 1 and 2 from the statistics records [ n ][ ACN_STATS_STRIDE ] (16-byte aligned), the levels of
 * acn_launch_denoise.  background: the linear value of an EMPTY record's pixel.  out_rgb is written by the first launch already */
void acn_launch_denoise_stats( const double* stats, const double* surf, size_t width, size_t height, uint32_t iterations, uint32_t normal_power_log2,
                               uint32_t no_demodulate, double sigma_plane, double sigma_lum, const double* background, void* scratch,
                               double* out_rgb, hipStream_t stream );

/* acn_fill_stats (k_fill.hip): prepare, which also writes every position's output but a FILLED one's, and one gather over the
 * ( 2 * radius + 1 )^2 window.  stats, surf, out_stats 16-byte aligned, out_need nullable; the parameters are final values; scratch:
 * ACN_FILL_SCRATCH_PER_PIXEL bytes per pixel (no more than the denoiser's, whose scratch serves), 128-byte aligned */
#define ACN_FILL_SCRATCH_PER_PIXEL 112
void acn_launch_fill_stats( const double* stats, const double* surf, size_t width, size_t height, uint32_t radius, uint32_t normal_power_log2,
                            uint32_t no_demodulate, double sigma_px, double sigma_plane, const double* background, void* scratch,
                            double* out_stats, double* out_need, hipStream_t stream );

/* the thin-lens camera (k_lens.hip).  LensSetup: acn_lens_params after the host's checks, final values, no defaults.
 * rays: out_rays[ i ][ s ][ 6 ] = the ray of position i, sample first_sample + s (s < n_samples); pos_xy [ n ][ 2 ], or null: the pixel
 * centres first_pixel + i of the scene's raster.  n * n_samples fits a grid of 256-lane workgroups (the host checks).
 * reduce: out_rgb[ i ] = ( ( ( 0.0 + rad[ i ][ 0 ] ) + rad[ i ][ 1 ] ) + ... ) / samples, through cl_s_sat unless linear; rad [ n ][ samples ][ 3 ]. */
struct LensSetup { uint64_t seed; uint32_t samples, jitter; double aperture_radius, focus_distance; };
void acn_launch_lens_rays( const DevScene& sc, const double* pos_xy, size_t first_pixel, size_t n, const LensSetup& ls,
                           uint32_t first_sample, uint32_t n_samples, double* out_rays, hipStream_t stream );
void acn_launch_lens_reduce( const double* rad, size_t n, uint32_t samples, double gamma, int linear, double* out_rgb, hipStream_t stream );
/* reduce_stats: the same out_rgb (nullable) and stats[ i ] = { samples, mean, m2, 0 }, always linear; stats 16-byte aligned.
 * merge: acc[ index ? index[ j ] : j ] <- part[ j ], j < n_part; indices outside [ 0, n_acc ) are skipped.
 * resolve: out_rgb (nullable) the mean or, of an EMPTY record, background; out_noise (nullable) [ n ]. */
void acn_launch_lens_reduce_stats( const double* rad, size_t n, uint32_t samples, double gamma, int linear, double* out_rgb, double* stats,
                                   hipStream_t stream );
void acn_launch_stats_merge( double* acc, size_t n_acc, const double* part, size_t n_part, const int64_t* index, hipStream_t stream );
void acn_launch_stats_resolve( const double* stats, size_t n, const double* background, double gamma, int linear, double* out_rgb,
                               double* out_noise, hipStream_t stream );

/* the aggregate surface record (k_lens_surface.hip; include/actinon_hip.h states it): records [ n ][ samples ][ ACN_SURF_STRIDE ] ->
 * out [ n ][ ACN_SURF_STRIDE ], both 16-byte aligned, samples 1 .. ACN_LENS_MAX_SAMPLES */
void acn_launch_surface_reduce( const double* records, size_t n, uint32_t samples, double* out, hipStream_t stream );

/* the layered records (k_lens_layers.hip; include/actinon_hip.h states them): records [ n ][ samples ][ ACN_SURF_STRIDE ] and rad
 * [ n ][ samples ][ 3 ] -> plane l of out_surface at out_surface + l * surface_plane * ACN_SURF_STRIDE (l = 0, 1) and plane l of
 * out_stats at out_stats + l * stats_plane * ACN_STATS_STRIDE (l = 0, 1, 2: layer 0, layer 1, rest); the planes are counted in
 * positions, so a slice of a larger call writes into the caller's planes.  records and both outputs 16-byte aligned */
void acn_launch_lens_layers( const double* records, const double* rad, size_t n, uint32_t samples, double* out_surface, size_t surface_plane,
                             double* out_stats, size_t stats_plane, hipStream_t stream );

/* layered records of two passes merged by surface class, and their resolve (k_lens_layers_merge.hip; include/actinon_hip.h states
 * both).  merge: the accumulator's planes acc_surface [ 2 ][ n_acc ][ ACN_SURF_STRIDE ] and acc_stats [ 3 ][ n_acc ][ ACN_STATS_STRIDE ] take the
 * part's planes [ . ][ n_part ][ . ], position j into index ? index[ j ] : j; indices outside [ 0, n_acc ) are skipped; n_part >= 1.
 * resolve: stats [ 3 ][ n ][ ACN_STATS_STRIDE ] -> out_rgb, out_noise as acn_launch_stats_resolve of the pooled record, out_pooled
 * [ n ][ ACN_STATS_STRIDE ]; each nullable.  Every record buffer 16-byte aligned */
void acn_launch_lens_layers_merge( double* acc_surface, double* acc_stats, size_t n_acc, const double* part_surface, const double* part_stats,
                                   size_t n_part, const int64_t* index, hipStream_t stream );
void acn_launch_lens_layers_resolve( const double* stats, size_t n, const double* background, double gamma, int linear, double* out_rgb,
                                     double* out_noise, double* out_pooled, hipStream_t stream );

/* acn_project_points* and acn_reproject* (k_reproject.hip; include/actinon_hip.h states both).  project: points [ n ][ 3 ] -> out_pos_xy
 * [ n ][ 2 ] and out_depth [ n ] (nullable) with the camera of sc.  reproject: cur_surface [ n ][ ACN_SURF_STRIDE ], the previous raster's
 * prev_surface and prev_stats [ prev.image_height * prev.image_width ][ . ] -> out_stats [ n ][ ACN_STATS_STRIDE ] and out_motion [ n ][ 2 ]
 * (nullable); of prev the raster size and the camera are read.  ReprojectSetup: acn_reproject_params after the host's checks, final
 * values, no defaults.  Every record buffer 16-byte aligned; n >= 1 */
struct ReprojectSetup { uint32_t reject_kinds; int32_t max_hops; double normal_min, plane_tolerance, max_history; };
void acn_launch_project_points( const DevScene& sc, const double* points, size_t n, double* out_pos_xy, double* out_depth, hipStream_t stream );
void acn_launch_reproject( const double* cur_surface, size_t n, const acn_params& prev, const double* prev_surface, const double* prev_stats,
                           const ReprojectSetup& su, double* out_stats, double* out_motion, hipStream_t stream );
/* acn_reproject_moving*: the same with motion [ n_motion ][ ACN_MOTION_STRIDE ], 16-byte aligned, n_motion >= 1: one row per node index */
void acn_launch_reproject_moving( const double* cur_surface, size_t n, const acn_params& prev, const double* prev_surface, const double* prev_stats,
                                  const double* motion, uint64_t n_motion, const ReprojectSetup& su, double* out_stats, double* out_motion,
                                  hipStream_t stream );

/* the filter of acn_denoise_layers (k_denoise_layers.hip): stats [ 3 ][ n ][ ACN_STATS_STRIDE ], surf [ 2 ][ n ][ ACN_SURF_STRIDE ], both 16-byte
 * aligned; the parameters are final values; scratch: ACN_DENOISE_LAYERS_SCRATCH_PER_PIXEL bytes per pixel, 128-byte aligned */
#define ACN_DENOISE_LAYERS_SCRATCH_PER_PIXEL 256
void acn_launch_denoise_layers( const double* stats, const double* surf, size_t width, size_t height, uint32_t iterations, uint32_t normal_power_log2,
                                uint32_t no_demodulate, double sigma_plane, double sigma_lum, const double* background, void* scratch,
                                double* out_rgb, hipStream_t stream );

/* acn_select_above* and acn_key_histogram* (k_select.hip), after the host's checks (acn_select_host.h); n >= 1.
 * select: three launches -- the count per tile of ACN_SELECT_TILE entries, the exclusive scan of the counts, the scatter (left out
 * when capacity is 0 or both out buffers are null).  tiles: acn_select_tiles( n ) + 1 words of the handle; the last one and
 * *out_count (nullable, device) receive the total.  raster_width > 0 whenever src_pos_xy is null and out_pos_xy is not.
 * key_hist: adds the bins of the keys to out_hist [ ACN_KEY_HIST_WORDS ], which the caller has zeroed on the same stream. */
void acn_launch_select( const double* key, size_t n, double threshold, unsigned long long* tiles, unsigned long long capacity,
                        const double* src_pos_xy, unsigned long long raster_width, unsigned long long raster_first, int64_t* out_index,
                        double* out_pos_xy, unsigned long long* out_count, hipStream_t stream );
void acn_launch_key_hist( const double* key, size_t n, unsigned long long* out_hist, hipStream_t stream );

/* the device-resident frame (k_frame.hip; include/actinon_hip.h states every step, acn_frame_host.h holds the expressions), after the
 * host's checks.  acc [ height * width ][ 6 ], 16-byte aligned; index: the flagged pixels, or null for the plan of the main pass (group
 * r is pixel r); pos_xy [ entries ][ 2 ] and clr [ entries ][ 3 ] with entries = groups * samples.
 * key: every pixel.  jitter: entries [ e0, e0 + cnt ), cnt >= 1 and at most 2^24.  foreign: zeroes the count, lists the foreign entries
 * of the whole plan in foreign [ 1 + slots ] and adds them with one lane.  push: groups [ g0, g0 + cnt ), their own entries.
 * image: out_rgb [ pixels ][ 3 ] f64 and out_rgb8 [ pixels ][ 3 ], each nullable. */
void acn_launch_frame_key( const double* acc, uint64_t width, uint64_t height, double* key, hipStream_t stream );
void acn_launch_frame_jitter( const long long* index, uint64_t e0, uint64_t cnt, uint64_t samples, uint64_t rval, uint64_t width, double* pos_xy,
                              hipStream_t stream );
void acn_launch_frame_foreign( const long long* index, const double* pos_xy, const double* clr, uint64_t entries, uint64_t samples, uint64_t width,
                               uint64_t height, uint32_t slots, unsigned long long* foreign, double* acc, hipStream_t stream );
void acn_launch_frame_push( const long long* index, const double* pos_xy, const double* clr, uint64_t g0, uint64_t cnt, uint64_t samples,
                            uint64_t width, uint64_t height, double* acc, hipStream_t stream );
void acn_launch_frame_image( const double* acc, uint64_t pixels, double* out_rgb, unsigned char* out_rgb8, hipStream_t stream );

#define ACN_SCENE_ARGS_OF( s ) ( s ).dev, ( s ).nodes, ( s ).mats, ( s ).elems, ( s ).textures
#define ACN_TASKQ_ARGS_OF( q ) ( q ).tasks, ( q ).idx[ 0 ], ( q ).idx[ 1 ], ( q ).idx[ 2 ], ( q ).idx[ 3 ], ( q ).counts, ( q ).task_cap, ( q ).hard_shadow, ( q ).hs_cap, ( q ).emit_terms

#endif
