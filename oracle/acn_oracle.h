/* acn_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain recursive C, fp64) of Actinon's trace/radiance hot path, operating on the same
 * flattened scene the GPU library consumes (include/actinon_hip.h).  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load this; the product (actinon_amd/, libactinon_hip.so,
 * libactinon_host.so) never links, imports or calls it.
 *
 * PARITY STATUS: the reference (johsteffens/actinon) cannot be built here (it needs the absent library
 * `beth`; building it behind hand-written stand-ins is not allowed), it ships no tests, golden vectors or
 * fixtures, and its Monte-Carlo LCG constants live in beth.  This oracle is therefore pinned only
 *   (a) statistically, against block means of the reference's own shipped renders (image/NAME.png ->
 *       tests/golden/ref_image_blocks.json, tests/test_oracle_vs_reference_images.py), and
 *   (b) by the three known-answer values SURVEY.md 8(c) recorded from the verbatim-compiled gmath.c.
 * Bit-level / sample-stream parity with an upstream build is UNPINNED.
 *
 * Arithmetic: IEEE binary64, expressions in the reference's order, no FP contraction.  Transcendentals come
 * from actinon_amd/csrc/acn_detmath.h (default; bit-identical to the GPU) or, with -DACN_ORACLE_LIBM, from
 * libm as in the reference.
 */
#ifndef ACN_ORACLE_H
#define ACN_ORACLE_H

#include "actinon_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* event counters */
enum
{
    ORC_N_LUM = 0,        /* scene_s_lum calls */
    ORC_N_TRANS_RAY,      /* compound_s_ray_trans_hit calls on a root compound */
    ORC_N_SHADOW_RAY,     /* compound_s_ray_hit(matter) occlusion tests */
    ORC_N_OBJ_HIT,        /* obj_ray_hit calls (all levels) */
    ORC_N_ENV_TEST,       /* envelope_s_ray_hits / envelope side tests */
    ORC_N_PLANE_HIT,
    ORC_N_SPHERE_HIT,     /* sphere objects only */
    ORC_N_SQUAROID_HIT,
    ORC_N_SDF_RAY,
    ORC_N_SDF_EVAL,
    ORC_N_PAIR_HIT,
    ORC_N_SIDE,           /* obj_side calls (all levels) */
    ORC_N_CAP_SAMPLE,
    ORC_N_OREN_NAYAR,
    ORC_N_FRESNEL,
    ORC_N_NODE_VISIT,     /* nodes touched by ray traversal */
    ORC_N_FLOP,           /* F_alg: sum of event costs (actinon_amd/csrc/acn_costs.h) */
    ORC_N_TRANSC,         /* T_alg: transcendental calls */
    /* (appended: 0 .. 17 keep their meaning) */
    ORC_N_OREN_NAYAR_DIRECT, /* oren_nayar_weight calls of the direct-light loop of scene_s_lum ... */
    ORC_N_OREN_NAYAR_PATH,   /* ... and of its path loop: the two add up to ORC_N_OREN_NAYAR */
    /* The part of F_alg / T_alg booked by scene_s_lum itself and by the camera ray: the events a device kernel cannot skip
     * (ACN_F_LUM_FIXED, EMISSION, ABSORB, FRESNEL_REFL / REFR, REFLECTION, SHADE_DIFFUSE, SEED, FOV, FRAME, CAP_SAMPLE, OREN_NAYAR,
     * DIRECT_TAIL, PATH_TAIL, CAMERA_RAY).  The rest, FLOP - FLOP_SHADE, is geometry: obj_ray_hit, obj_side, the envelope tests,
     * the roughness perturbation and the trans-hit resolve, which the device's traversal shortcuts may leave out. */
    ORC_N_FLOP_SHADE,
    ORC_N_TRANSC_SHADE,
    ORC_N_COUNTERS
};

/* out_rgb[i] = cl_s_sat( lum( pos_xy[i] ) ); flags: ACN_OPT_LINEAR_OUT. threads >= 1 (pthread pixel farm,
 * src/scene.c:1017-1028). counters (nullable): the sums over all positions of the first 18 counters, [ 0 .. ORC_N_TRANSC ]. Returns acn_status. */
int acn_oracle_render_positions( const acn_flat_scene* scene, const double* pos_xy, size_t n, double* out_rgb,
                                 uint32_t flags, int threads, uint64_t* counters );

/* the same for rank `rank` of `world` of a sample-sharded call (ACN_SHARD_SAMPLES, include/actinon_hip.h): linear
 * partial radiance; the sum over the ranks is the unsharded result up to floating-point reassociation */
int acn_oracle_render_positions_shard( const acn_flat_scene* scene, const double* pos_xy, size_t n, double* out_rgb,
                                       uint32_t flags, int threads, uint64_t* counters, uint32_t rank, uint32_t world );

/* The two calls above fill counters[ 0 .. ORC_N_TRANSC ], the 18 words they always have.  This one fills the first n_counters words
 * (ORC_N_COUNTERS at most) of a buffer of that length: the split counters behind ORC_N_TRANSC come through it alone. */
int acn_oracle_render_positions_work( const acn_flat_scene* scene, const double* pos_xy, size_t n, double* out_rgb, uint32_t flags,
                                      int threads, uint64_t* counters, size_t n_counters, uint32_t rank, uint32_t world );

/* obj_estimate_envelope (src/objects.c:312-363): out = pos[3], radius */
int acn_oracle_estimate_envelope( const acn_flat_scene* scene, int32_t node, uint64_t samples, uint32_t rseed,
                                  double radius_factor, double* out_pos3_radius );

/* leaf functions exposed for known-answer tests */
double acn_oracle_sphere_ray_hit( const double* pos3, double r, const double* ray_p3, const double* ray_d3, double* nor3 );
double acn_oracle_plane_ray_hit( const double* pos3, const double* nor3, const double* ray_p3, const double* ray_d3 );
double acn_oracle_fresnel_reflection( const double* dir3, const double* exit_nor3, double trix, double* out_dir3 );
void   acn_oracle_fresnel_refraction( const double* dir3, const double* exit_nor3, double trix, double* out_dir3 );
double acn_oracle_obj_ray_hit( const acn_flat_scene* scene, int32_t node, const double* ray_p3, const double* ray_d3, double* nor3 );
int    acn_oracle_obj_side( const acn_flat_scene* scene, int32_t node, const double* pos3 );
double acn_oracle_trans_hit( const acn_flat_scene* scene, const double* ray_p3, const double* ray_d3,
                             double* exit_nor3, int32_t* exit_obj, int32_t* enter_obj );
/* The one-ray functions above (and compound_s_ray_hit, which is not exported on its own) over arrays, on `threads` pthreads.
 * rays: [ n ][ 6 ] origin, direction; limits (nullable = inf): [ n ]; out: [ n ][ ACN_ORACLE_QUERY_STRIDE ].
 *   OBJ_RAY_HIT        obj_ray_hit( node ): a, normal[3]
 *   OBJ_SIDE           obj_side( node ) at the origin: side
 *   COMPOUND_RAY_HIT   compound_s_ray_hit( node ): a, normal[3], hit object
 *   TRANS_HIT          compound_s_ray_trans_hit( node ): a, exit normal[3], exit object, enter object (-1: none)
 *   OCCLUDED           COMPOUND_RAY_HIT and [ 5 ] = a <= limit, the occlusion test of scene_s_lum
 * node must be a compound for the last three and must not be one for the first two. */
enum { ACN_ORACLE_Q_OBJ_RAY_HIT = 0, ACN_ORACLE_Q_OBJ_SIDE, ACN_ORACLE_Q_COMPOUND_RAY_HIT, ACN_ORACLE_Q_TRANS_HIT, ACN_ORACLE_Q_OCCLUDED,
       ACN_ORACLE_Q_N };
#define ACN_ORACLE_QUERY_STRIDE 8

/* The tap: scene_s_lum (src/scene.c:420-667) for ONE hit, without recursing, recorded.  scene_lum itself writes the rows while it
 * runs (the arithmetic is not restated); where the reference would call itself for a child, the row holds the arguments of that call.
 * hit: [ 14 ] ray origin[3], direction[3], offs, exit normal[3], exit object, enter object (-1: none), depth, intensity.
 * rows: [ room ][ ACN_ORACLE_TAP_STRIDE ] doubles, row[ 0 ] the kind, in the order scene_s_lum computes them; *n_rows: the rows the hit
 * has (above room: the rest was not written).  out_lum3 (nullable): what the call returns with every child's radiance zero.
 *   EMISSION    [1..3] the returned colour, [4] diff_sqr, [5] light_intensity                     (the only row of such a hit)
 *   SURFACE     [1..3] pos, [4..6] enter_color, [7] trix, [8] on_a, [9] on_b, [10] fresnel, [11] chromatic, [12] diffuse
 *               reflectivity, [13] transparent
 *   FRESNEL, CHROMATIC, REFRACTION   a specular child: [1..3] origin, [4..6] direction, [7] intensity, [8] depth, [9..11] the colour
 *               multiplied onto what it returns
 *   DIFFUSE     [1..3] surface_d, [4] theta_i, [5..7] ray_projection, [8] diffuse_intensity, [9] rv (raw 64 bits), [10] depth
 *   LIGHT       [1] light node, [2] cyl_hgt, [3..5] colour, [6] direct samples, [7..9] axis of the sampling cone
 *   DIRECT      sample j of the light before: [1] j, [2] light node, [3..5] out_d, [6] raw weight, [7] light-hit distance (inf: none,
 *               or not asked because weight <= 0), [8] exact Oren-Nayar weight, [9] 1: occluded, [10] local_intensity, [11] the
 *               term local_intensity * weight * diffuse_intensity ([8] .. [11] zero where the sample did not get that far)
 *   PATHS       [1] path samples
 *   PATH        sample j: [1] j, [2..4] out_d, [5] raw weight, [6] exact weight, [7] a, [8..10] exit normal, [11] exit, [12] enter
 *               object, [13] weight * diffuse_intensity, [14] 1: a < max_path_length, the reference recurses
 *   ABSORB      [1..3] the factors on everything the call returns */
enum { ACN_ORACLE_TAP_EMISSION = 0, ACN_ORACLE_TAP_SURFACE, ACN_ORACLE_TAP_FRESNEL, ACN_ORACLE_TAP_CHROMATIC, ACN_ORACLE_TAP_REFRACTION,
       ACN_ORACLE_TAP_DIFFUSE, ACN_ORACLE_TAP_LIGHT, ACN_ORACLE_TAP_DIRECT, ACN_ORACLE_TAP_PATHS, ACN_ORACLE_TAP_PATH, ACN_ORACLE_TAP_ABSORB };
#define ACN_ORACLE_TAP_STRIDE 16
int acn_oracle_shade_point( const acn_flat_scene* scene, const double* hit, double* rows, size_t room, size_t* n_rows, double* out_lum3 );
int acn_oracle_query_rays( const acn_flat_scene* scene, int op, int32_t node, const double* rays, size_t n, const double* limits,
                           double* out, int threads );
/* The same two with the event counters of the calls ADDED to counters[ ORC_N_COUNTERS ] (the caller zeroes them): what the oracle spends
 * on exactly these rays / on this one scene_s_lum call -- its two sample loops with their light hits, shadow rays and path transition
 * hits, and no specular child, which the tap does not trace. */
int acn_oracle_query_rays_counted( const acn_flat_scene* scene, int op, int32_t node, const double* rays, size_t n, const double* limits,
                                   double* out, int threads, uint64_t* counters );
int acn_oracle_shade_point_counters( const acn_flat_scene* scene, const double* hit, uint64_t* counters );
uint64_t acn_oracle_random_seed( const double* v3, uint64_t rv );
void   acn_oracle_sphere_cap( uint64_t* rv, double h, double* out3 );
/* 0: detmath, 1: libm */
int    acn_oracle_math_mode( void );

#ifdef __cplusplus
}
#endif
#endif
