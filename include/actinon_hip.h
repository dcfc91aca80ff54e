/* actinon_hip.h -- C ABI of libactinon_hip.so: the MI355X (gfx950) replacement for Actinon's
 * per-sample trace/radiance path.
 *
 * Drop-in seam (reference, all paths relative to /root/reference):
 *   void lum_machine_s_run( const scene_s* scene, lum_arr_s* lum_arr )      src/scene.c:1017-1028
 * called from exactly one place, scene_s_create_image_file (src/scene.c:1141).  The reference has no
 * FFI layer; this header promotes that internal function boundary to a C ABI:
 *
 *   reference input                                  ->  this ABI
 *   scene_s render fields (src/scene.c:153-183)      ->  acn_params
 *   scene->light / scene->matter compound_s graphs   ->  acn_flat_scene.nodes / .elems (POD, index-linked)
 *   lum_arr->data[i].pos  (v2d_s, src/scene.c:682)   ->  pos_xy[i*2 .. i*2+1]
 *   lum_arr->data[i].clr  (cl_s after cl_s_sat)      ->  out_rgb[i*3 .. i*3+2]
 *
 * Everything is plain pointers + sizes; no torch / HIP types appear in a signature (streams and device
 * pointers are passed as void*).  All floating point is IEEE binary64, as in the reference (f3_t).
 */
#ifndef ACTINON_HIP_H
#define ACTINON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACN_ABI_VERSION 2

/* ------------------------------------------------------------------------------------------------------------------ */
/* Flattened scene.  One acn_node per reference object (obj_*_s, src/objects.c) or compound_s (src/compound.c:36-50).
 * Pointers of the reference become int32 indices into nodes[]; a compound's element array becomes a slice of elems[]. */

enum acn_node_type
{
    ACN_PLANE        = 1, /* obj_plane_s         src/objects.c:480-547   */
    ACN_SPHERE       = 2, /* obj_sphere_s        src/objects.c:552-661   */
    ACN_SQUAROID     = 3, /* obj_squaroid_s      src/objects.c:669-831   */
    ACN_DISTANCE     = 4, /* obj_distance_s      src/objects.c:836-970   */
    ACN_PAIR_INSIDE  = 5, /* obj_pair_inside_s   src/objects.c:975-1120  */
    ACN_PAIR_OUTSIDE = 6, /* obj_pair_outside_s  src/objects.c:1125-1277 */
    ACN_NEG          = 7, /* obj_neg_s           src/objects.c:1282-1348 */
    ACN_SCALE        = 8, /* obj_scale_s         src/objects.c:1353-1459 */
    ACN_COMPOUND     = 9  /* compound_s          src/compound.c:36-50    */
};

enum acn_sdf_kind
{
    ACN_SDF_SPHERE = 0,   /* distance_sphere_s_call  src/distance.c:39-42 */
    ACN_SDF_TORUS  = 1    /* distance_torus_s_call   src/distance.c:83-92 */
};

#define ACN_NODE_HAS_ENVELOPE 1u

/* 304 bytes, 16-byte aligned.  prp fields follow properties_s (src/objects.h:51-78). */
typedef struct acn_node
{
    int32_t  type;        /* enum acn_node_type */
    uint32_t flags;       /* ACN_NODE_HAS_ENVELOPE */
    int32_t  child0;      /* pair: o1 | neg, scale: o1 | compound: first index into elems[] | else -1 */
    int32_t  child1;      /* pair: o2 | compound: number of elements | else -1 */
    int32_t  sdf_kind;    /* ACN_DISTANCE: enum acn_sdf_kind */
    int32_t  cycles;      /* ACN_DISTANCE: obj_distance_s.cycles */
    int32_t  texture;     /* prp.texture_field: index into acn_flat_scene.textures, -1 = none */
    int32_t  reserved;

    double pos[3];        /* prp.pos */
    double rax[9];        /* prp.rax, rows x,y,z */
    double env_pos[3];    /* prp.envelope->pos   (compound: compound_s.envelope) */
    double env_radius;    /* prp.envelope->radius */
    double prm[4];        /* sphere: radius,-,-,- | squaroid: a,b,c,r | distance: inv_scale,ex_radius,-,- | scale: inv_scale.xyz,- */

    double color[3];      /* prp.color */
    double radiance;
    double refractive_index;
    double fresnel_reflectivity;
    double chromatic_reflectivity;
    double diffuse_reflectivity;
    double sigma;
    double surface_roughness;
    double transparency[3];
    double pad_;
} acn_node;

/* Texture fields (src/textures.c): the colour of an object's surface as a function of position, obj_color
 * src/objects.c:411-422.  ACN_TXM_CHESS uses obj_projection, which only planes (objects.c:514-518), spheres (:602-617)
 * and distance objects (:893-896) implement; on any other object type it is rejected at upload. */
enum acn_texture_kind
{
    ACN_TXM_PLAIN = 0,    /* txm_plain_s src/textures.c:62-102 : color1 */
    ACN_TXM_CHESS = 1     /* txm_chess_s src/textures.c:118-148: ( llrint( p.x*scale ) ^ llrint( p.y*scale ) ) & 1 ? color1 : color2 */
};

typedef struct acn_texture
{
    int32_t kind;
    int32_t reserved;
    double  color1[3];
    double  color2[3];
    double  scale;
} acn_texture;

/* Render parameters: the scene_s fields the hot path reads (src/scene.c:153-183; defaults :185-213). */
typedef struct acn_params
{
    uint64_t image_width;
    uint64_t image_height;
    double   gamma;
    double   background_color[3];
    double   camera_position[3];
    double   camera_view_direction[3];
    double   camera_top_direction[3];
    double   camera_focal_length;
    uint64_t trace_depth;
    double   trace_min_intensity;
    uint64_t direct_samples;
    uint64_t path_samples;
    double   max_path_length;
    int64_t  experimental_level;   /* must be 0 (src/scene.c:1000-1007) */
} acn_params;

typedef struct acn_flat_scene
{
    uint32_t        abi_version;   /* ACN_ABI_VERSION */
    uint32_t        n_nodes;
    uint32_t        n_elems;
    int32_t         light_root;    /* node index of scene->light  (an ACN_COMPOUND) */
    int32_t         matter_root;   /* node index of scene->matter (an ACN_COMPOUND) */
    uint32_t        reserved;
    const acn_node* nodes;
    const int32_t*  elems;
    acn_params      params;
    uint32_t        n_textures;
    uint32_t        reserved2;
    const acn_texture* textures;
} acn_flat_scene;

/* The 64-bit LCG triple the reference takes from beth (bcore_lcg00/01/02_u3; src/vectors.h:45-48,185-189).
 * beth is not available offline, so the constants are DECLARED here; stream-exact parity with an upstream
 * build is therefore unpinned. x' = a*x + c (mod 2^64). */
#ifndef ACN_LCG00_A   /* (the statistical pin of the test oracle builds it with other triples too: tests/test_reference_images.py) */
#define ACN_LCG00_A 6364136223846793005ull
#define ACN_LCG00_C 1442695040888963407ull
#define ACN_LCG01_A 2862933555777941757ull
#define ACN_LCG01_C 3037000493ull
#define ACN_LCG02_A 3202034522624059733ull
#define ACN_LCG02_C 4354685564936845319ull
#endif

/* ------------------------------------------------------------------------------------------------------------------ */
/* Render call */

#define ACN_OPT_LINEAR_OUT 1u   /* skip cl_s_sat (src/vectors.h:372-384): caller accumulates / reduces first */
#define ACN_OPT_COUNT_WORK 2u   /* run the instrumented kernels: acn_last_counters() reports rays / samples / hit tests */
#define ACN_OPT_STAGE_TIMING 4u /* record HIP events around every launch: acn_last_stage_ms() reports per-stage times */

/* Sharding of one call over the ranks of a multi-GPU job (one process per GPU).  The reference has one process and
 * no counterpart; what shards is what its pixel farm makes independent (src/scene.c:976-1011): sample positions, and
 * inside a position the iterations of the outermost sample loops (src/scene.c:556,596).
 *   ACN_SHARD_SAMPLES  every rank renders every position of the call, but of each OUTERMOST direct-light loop and path
 *                      loop only the iterations [ n * rank / world, n * ( rank + 1 ) / world ) -- n, the normalisation
 *                      2 * cyl_hgt / n resp. 2 / n and the LCG stream position of an iteration stay those of the whole
 *                      loop.  Terms that are under no such loop (emission and background reached through specular
 *                      chains, src/scene.c:432-437,488-491,511-514,648-651; a camera ray that hits nothing) come from
 *                      rank 0 alone.  Out: LINEAR partial radiance (use ACN_OPT_LINEAR_OUT); the caller sum-reduces the
 *                      ranks' buffers and then applies acn_resolve_dev.  For few positions with many samples.
 * Whole positions are sharded with the acn_shard_tile_* functions below (disjoint supports, no floating-point reduce). */
#define ACN_SHARD_NONE    0u
#define ACN_SHARD_SAMPLES 1u

typedef struct acn_render_opts
{
    uint32_t flags;
    uint32_t struct_size;          /* sizeof( acn_render_opts ) as the CALLER was compiled; 0 = the base layout of this struct
                                      (ACN_RENDER_OPTS_BASE_SIZE = 40 bytes: flags .. reserved2 -- a zero-initialised struct with
                                      the shard members set keeps its meaning).  The library reads no member beyond it, so a host
                                      built against an older header keeps working when members are appended (ACN_RENDER_OPTS_INIT) */
    const volatile int* cancel;    /* optional; polled between launches; the SIGINT flag of src/scene.c:893,978 */
    void*    stream;               /* optional hipStream_t; NULL = the handle's own stream */
    uint32_t shard_mode;           /* ACN_SHARD_* */
    uint32_t shard_rank;           /* 0 .. shard_world - 1 */
    uint32_t shard_world;          /* 0 or 1: the call is not sharded */
    uint32_t reserved2;
} acn_render_opts;
#define ACN_RENDER_OPTS_BASE_SIZE 40
#define ACN_RENDER_OPTS_INIT { 0u, ( uint32_t )sizeof( acn_render_opts ), 0, 0, ACN_SHARD_NONE, 0u, 0u, 0u }

typedef struct acn_scene_handle acn_scene_handle;

enum acn_status
{
    ACN_OK              =  0,
    ACN_ERR_ARG         = -1,  /* malformed scene / argument */
    ACN_ERR_UNSUPPORTED = -2,  /* experimental_level != 0 (src/scene.c:1004-1007), projection-less chess texture, too-deep CSG */
    ACN_ERR_NO_FOV      = -3,  /* light object without fov function (src/objects.c:254-258) */
    ACN_ERR_DEVICE      = -4,  /* HIP failure, no GPU */
    ACN_ERR_CANCELLED   = -5
};

/* Number of visible HIP devices (0 if none). */
int acn_device_count( void );

/* Validates the flat scene, converts it to the device layout and makes it resident on `device`.
 * Replaces nothing in the reference (which traverses host pointers); it is the price of the seam. */
int acn_scene_upload( const acn_flat_scene* scene, int device, acn_scene_handle** out );
void acn_scene_free( acn_scene_handle* h );

/* Replacing the scene of a live handle: the next frame of an animation, another camera, preview samples turned into final ones --
 * without the cold start of a fresh handle.  acn_scene_replace makes `scene` the resident scene of h, on the handle's device;
 * acn_scene_set_params is the same change for the render parameters alone (camera, raster, samples, depth: no table is built and
 * nothing is allocated).  Every later call on the handle renders the new scene with exactly the bits a fresh handle of it gives.
 *   Kept       the handle's stream and events; every concurrent lane (stream, events, counter blocks, worker thread); the work queues as
 *              allocated (neither call allocates or frees a queue); the scratch buffers of the other entry points; the workspace bound
 *              and every tunable of the environment, which are read at acn_scene_upload and not again.
 *   Learned    What the pipeline learned about the scene (queue demand per position, walk passes) is kept iff the new scene is of the
 *              KIND of the old one: equal numbers of nodes, elements, light elements and path levels, both or neither with prune
 *              programs, equal path_samples, direct_samples and trace_depth, and a trace_min_intensity of the same bits
 *              (csrc/acn_queueplan.h: acn_replace_keeps_learned).  The raster and the camera are no part of the kind: a moved camera or a
 *              moved object keeps it.  Otherwise, or with ACN_REPLACE_FORGET, the next call learns again as a cold handle does -- on
 *              the lanes and queues that exist.  Pixels never depend on this: demand that was misjudged costs a chunk rendered twice.
 *   Statistics acn_last_stage_ms, acn_last_kernel_ms and acn_last_counters describe a render call: after a change there is none until
 *              the next one.  acn_last_stage_ms [ 24 ] keeps counting since the upload.
 *   Failure    ACN_ERR_ARG (a null handle, scene or params; unknown flag bits; a malformed scene), ACN_ERR_UNSUPPORTED, ACN_ERR_NO_FOV --
 *              what acn_scene_upload refuses -- and ACN_ERR_DEVICE while the new scene's device blocks are made leave the handle
 *              rendering the scene and parameters it had; acn_last_error says why.
 *   Caller     Both calls wait for the handle's own stream and for its lanes.  Work that earlier _dev calls queued on streams of the
 *              CALLER's must be complete before either is called: the library cannot see those streams.  A handle serves one
 *              caller at a time, here as everywhere. */
#define ACN_REPLACE_FORGET 1u   /* drop what the runners learned even if the rule above would keep it */
int acn_scene_replace( acn_scene_handle* h, const acn_flat_scene* scene, uint32_t flags );
int acn_scene_set_params( acn_scene_handle* h, const acn_params* prm );
/* Counters of a handle, since its upload unless said otherwise: how a host (or a test) sees that a handle stayed warm.  n <= ACN_INFO_N. */
enum
{
    ACN_INFO_REPLACES = 0,      /* acn_scene_replace calls accepted */
    ACN_INFO_PARAM_SETS,        /* acn_scene_set_params calls accepted */
    ACN_INFO_STREAMS,           /* streams made by this handle: its own and its lanes' */
    ACN_INFO_LANES,             /* lanes alive now */
    ACN_INFO_LEARNING_PASSES,   /* learning passes run (the sampled pass of a handle that does not know its scene's queue demand) */
    ACN_INFO_NODES,             /* nodes resident now */
    ACN_INFO_RATES_KNOWN,       /* 1 if some runner's rates are known now */
    ACN_INFO_DEVICE,            /* the device of the handle */
    ACN_INFO_N   /* 8 */
};
int acn_scene_info( acn_scene_handle* h, uint64_t* out, int n );

/* lum_machine_s_run counterpart on host buffers (src/scene.c:1017): out_rgb[i] = cl_s_sat( lum( pos_xy[i] ) ).
 * Synchronous. Returns acn_status. */
int acn_render_positions( acn_scene_handle* h, const double* pos_xy, size_t n, double* out_rgb,
                          const acn_render_opts* opts );

/* Same on device-resident buffers (d_pos_xy, d_out_rgb are device pointers on the handle's device).
 * Work is enqueued on opts->stream (NULL = the handle's own stream, then the call also waits for completion).
 * The call synchronises that stream once per chunk of positions (queue-overflow check); on return the last kernels may
 * still be in flight on a caller-provided stream. */
int acn_render_positions_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, void* d_out_rgb,
                              const acn_render_opts* opts );

/* Main-pass helper: pos = (i+0.5, j+0.5) row-major (src/scene.c:1110-1119) generated on the device,
 * for the pixel sub-range [first, first+count) of the image_width x image_height raster. */
int acn_render_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, void* d_out_rgb,
                              const acn_render_opts* opts );

/* Radiance of caller-supplied rays (custom cameras, panoramas, lens samples, light probes): the body of lum_machine_s_func
 * (src/scene.c:956-1013) after its camera ray.  rays: [ n ][ 6 ] f64 origin, direction (the layout of acn_query_rays).
 * out_rgb[ i ] = cl_s_sat( background_color ) if ray i hits nothing, else cl_s_sat( scene_s_lum( ray, offs, trans,
 * trace_depth, 1.0 ) ); linear with ACN_OPT_LINEAR_OUT.  Each direction goes through v3d_s_of_length( d, 1 )
 * (src/vectors.h:148-154), which leaves it unchanged, bit for bit, when |d|^2 is within 1e-8 of 1.  A non-finite component or
 * a zero direction (|d|^2 not a positive finite number) anywhere fails the call with ACN_ERR_ARG before anything is written;
 * acn_last_error names the first such ray.  opts: as for the position calls (flags, cancel, stream, ACN_SHARD_SAMPLES).
 * The scene's image_width, image_height and camera fields are not used; gamma, background_color and every sampling
 * parameter are.  Streams as for acn_render_positions_dev; the _dev call synchronises the stream once more, before it
 * renders, to read the check's one word.  Tile sharding is for positions: a caller shards rays by slicing the array. */
int acn_render_rays( acn_scene_handle* h, const double* rays, size_t n, double* out_rgb, const acn_render_opts* opts );
int acn_render_rays_dev( acn_scene_handle* h, const void* d_rays, size_t n, void* d_out_rgb, const acn_render_opts* opts );
/* The rays the pipeline casts for sample positions (camera_ray, src/scene.c:980-990), bit for bit: out_rays[ i ] = origin,
 * direction [ 6 ] f64 of pos_xy[ i ].  The _dev variant follows the stream rules of acn_render_positions_dev. */
int acn_camera_rays( acn_scene_handle* h, const double* pos_xy, size_t n, double* out_rays );
int acn_camera_rays_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, void* d_out_rays, const acn_render_opts* opts );

/* The surface a ray meets, one record per ray: what a denoiser takes as guides (depth, normal, albedo), what compositing and
 * picking need (object ids), none of it sampled.  out[ i ][ 0 .. ACN_SURF_STRIDE ), all f64, integers stored as doubles:
 *   [ 0 ]       distance: the `a` of scene_s_trans_hit (src/scene.c:362-382: lights first, matter only if strictly nearer);
 *               ACN_SURF_FOLLOW: the sum of the `a` of every segment, added in hop order.  inf: the (last) ray hit nothing
 *   [ 1 .. 3 ]  position ray.p + ray.d * a of the reported hit (as scene_s_lum forms pos)
 *   [ 4 .. 6 ]  trans.exit_nor, bit for bit; the normal that faces the viewer is its negative (src/scene.c:530)
 *   [ 7 ], [ 8 ] enter_obj, exit_obj: node indices of the media transition, -1 = none
 *   [ 9 .. 11 ] obj_color( s, position ), s = enter_obj if there is one, else exit_obj (src/objects.c:411-422, textures included)
 *   [ 12 ]      ACN_SURF_* kind bits: the material rules of scene_s_lum (src/scene.c:432-470) for this hit
 *   [ 13 ]      hops followed (0 with ACN_SURF_FIRST_HIT)
 *   [ 14 ]      weight: the product of the shares of the branches followed (1.0 with no hop)
 *   [ 15 ]      0; an aggregate record (acn_surface_reduce*, acn_surface_lens*) carries its coverage here, which is > 0
 * A miss has inf, -1, -1 in [ 0 ], [ 7 ], [ 8 ], keeps [ 13 ] and [ 14 ], and is zero elsewhere.
 * mode ACN_SURF_FIRST_HIT reports the first surface.  ACN_SURF_FOLLOW follows the dominant specular branch to the first
 * diffuse or emitting surface -- through a glass to the table behind it.  This is a definition of this library, not a function
 * of the reference; its terms are the intensities scene_s_lum hands its children (src/scene.c:473-653) with trace_min_intensity
 * left out.  At each hit, in this order:
 *   EMITTER: stop.
 *   refl = fresnel_reflectivity > 0 ? fresnel_reflection( d, exit_nor, trix, &refl_d ) * fresnel_reflectivity : 0;  rest = 1 - refl
 *   w[ 0 ] = refl                                                                   -> ray ( pos, refl_d )
 *   w[ 1 ] = chromatic_reflectivity * rest;  rest = rest * ( 1 - chromatic_reflectivity )  -> ( pos, v_reflection( d, exit_nor ) )
 *   w[ 2 ] = diffuse_reflectivity * rest;    rest = rest * ( 1 - diffuse_reflectivity )    -> stop
 *   w[ 3 ] = transparent ? rest : 0          -> ( ray.p + ray.d * ( a + 2 * f3_eps ), fresnel_refraction( d, exit_nor, trix ) )
 *   The largest w wins, the lowest index on a tie; if it is not positive or it is w[ 2 ]: stop.  Else weight *= w, hops += 1.
 * A chain reports at most max( trace_depth, 1 ) hits: a hit of that number that would continue is reported with ACN_SURF_CUT.
 * A continued ray that hits nothing reports a miss with the hops and the weight so far.
 * rays: the contract of acn_render_rays (each direction through v3d_s_of_length( d, 1 ); a non-finite component or a zero
 * direction fails the whole call with ACN_ERR_ARG before anything is written, acn_last_error names the first such ray).
 * Positions go through camera_ray: acn_surface_positions( pos ) equals acn_surface_rays( acn_camera_rays( pos ) ) bit for bit.
 * opts: only `stream` is used, by the _dev calls, with the rules of acn_render_positions_dev (the ray call synchronises the
 * stream once, to read the check's word; the position call never); shard_world > 1 or an unknown mode is ACN_ERR_ARG.
 * The _dev buffers should be 128-byte aligned: a record is 128 bytes and every lane writes its own line whole.  A surface call
 * uses no work queue and changes nothing a render call on the same handle sees.  A CSG nesting too deep for the device stacks
 * fails a call on the handle's own stream with ACN_ERR_UNSUPPORTED; a call on a caller's stream cannot wait for the word, which is then
 * reported by the handle's next surface call on its own stream. */
#define ACN_SURF_STRIDE 16          /* doubles per record: 128 bytes */
#define ACN_SURF_FIRST_HIT 0u
#define ACN_SURF_FOLLOW    1u       /* follow the dominant specular branch to the first diffuse / emitting surface */
#define ACN_SURF_EMITTER     1u     /* enter_obj has radiance > 0 */
#define ACN_SURF_DIFFUSE     2u     /* diffuse_reflectivity > 0 after the exit rule */
#define ACN_SURF_CHROMATIC   4u     /* chromatic_reflectivity > 0 after the exit rule */
#define ACN_SURF_FRESNEL     8u     /* fresnel_reflectivity > 0 after the rules (src/scene.c:451, :467) */
#define ACN_SURF_TRANSPARENT 16u
#define ACN_SURF_LIGHT_ROOT  32u    /* the hit came from the light compound */
#define ACN_SURF_CUT         64u    /* ACN_SURF_FOLLOW stopped because of trace_depth */
int acn_surface_rays( acn_scene_handle* h, const double* rays, size_t n, uint32_t mode, double* out, const acn_render_opts* opts );
int acn_surface_rays_dev( acn_scene_handle* h, const void* d_rays, size_t n, uint32_t mode, void* d_out, const acn_render_opts* opts );
int acn_surface_positions( acn_scene_handle* h, const double* pos_xy, size_t n, uint32_t mode, double* out, const acn_render_opts* opts );
int acn_surface_positions_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, uint32_t mode, void* d_out, const acn_render_opts* opts );

/* Sharding of whole positions: the n positions of a call (or pixels of a frame) are cut into tiles of ACN_SHARD_TILE
 * consecutive positions dealt round-robin to the ranks -- interleaving balances sky, floor and glass between them.
 * These three are plain arithmetic (no GPU): */
#define ACN_SHARD_TILE 256
/* number of positions rank `rank` of `world` owns */
size_t acn_shard_tile_count( size_t n, uint32_t rank, uint32_t world );
/* common length of the ranks' parts for an all-gather: the largest count, i.e. ceil( ceil( n / TILE ) / world ) * TILE */
size_t acn_shard_tile_padded( size_t n, uint32_t world );
/* index in [ 0, n ) of the i-th position of the rank's part (i < acn_shard_tile_count) */
size_t acn_shard_tile_index( size_t n, uint32_t rank, uint32_t world, size_t i );

/* Main pass of rank `rank`: renders the rank's tiles of the pixel range [ first, first + count ) (acn_render_main_pass_dev's
 * positions) into d_part, [ acn_shard_tile_padded( count, world ) ][ 3 ] f64, part order, zero behind the rank's count. */
int acn_render_main_pass_shard_dev( acn_scene_handle* h, size_t first, size_t count, uint32_t rank, uint32_t world,
                                    void* d_part, const acn_render_opts* opts );
/* After the all-gather of the ranks' parts (d_gathered: [ world ][ padded ][ 3 ] f64, rank-major): the frame
 * d_frame[ count ][ 3 ] in position order.  Every value is copied, none is added: bit-identical to one GPU. */
int acn_shard_unpack_dev( acn_scene_handle* h, const void* d_gathered, size_t count, uint32_t world, void* d_frame,
                          const acn_render_opts* opts );

/* cl_s_sat (src/vectors.h:372-384) + cps_from_cl (src/scene.c:76-82) on a device-resident LINEAR radiance buffer,
 * e.g. after the cross-GPU sum-reduce: d_out_rgb (nullable) receives the gamma-saturated colours [n][3] f64,
 * d_out_rgb8 (nullable) the packed 8-bit pixels [n][3] u8 in PNM order. In-place (d_out_rgb == d_linear_rgb) allowed. */
int acn_resolve_dev( acn_scene_handle* h, const void* d_linear_rgb, size_t n, void* d_out_rgb, void* d_out_rgb8,
                     const acn_render_opts* opts );

/* Edge-avoiding filter for a low-sample LINEAR frame, guided by the frame's surface records (k_denoise.hip).  This filter is a
 * definition of this library, not a function of the reference, which has no denoiser: an a-trous wavelet filter on the
 * albedo-demodulated radiance whose stops are the records' object ids, normals and positions and a luminance stop scaled by
 * a variance estimated from the frame itself.
 *   linear_rgb [ height * width ][ 3 ]  f64 radiance as ACN_OPT_LINEAR_OUT gives it, one sample position per pixel, row-major
 *   surface    [ height * width ][ ACN_SURF_STRIDE ]  the records of the same positions or rays, either mode (ACN_SURF_FOLLOW
 *              is the recommended one: behind glass it guides with the surface that is seen through it)
 *   out_rgb    [ height * width ][ 3 ]  linear; the caller applies acn_resolve_dev afterwards.  out_rgb == linear_rgb is allowed.
 * The scene is not consulted: the handle supplies the device, the stream and the scratch memory (two colour buffers of 32 bytes
 * and one guide of 64 bytes per pixel: 128 bytes per pixel, owned by the handle, grown on demand, freed by acn_scene_free, apart
 * from the render workspace: render calls before and after compute the same bits and acn_last_stage_ms [ 23 ], [ 24 ] stay).
 * Work goes to opts->stream; NULL is the handle's own stream, and then the call waits.  On a caller's stream the call never
 * synchronises: every check is made on the host.  Of opts only `stream` is used; shard_world > 1 is ACN_ERR_ARG.
 * ACN_ERR_ARG, with acn_last_error set and nothing written: a null handle or buffer; a zero width or height or width * height
 * above 2^31; iterations > 8; normal_power_log2 > 10; a negative or non-finite sigma; struct_size < 4; unknown flag bits; a
 * d_surface that is not 16-byte aligned (the records are read 16 bytes at a time; 128-byte alignment, as the surface calls ask, is best).
 *
 * Everything is IEEE binary64 without contraction, a / b is IEEE division, exp and sqrt are acn_exp and acn_sqrt of
 * csrc/acn_detmath.h, a sum a + b + c is ( a + b ) + c, dot( u, v ) is ( u.x * v.x + u.y * v.y ) + u.z * v.z, max( 0, x ) is
 * x > 0 ? x : 0, and a tap that is skipped adds nothing.  r = record of the pixel, L = its radiance:
 * 1 demodulate   a.c = r[ 9 + c ] > 0.01 ? r[ 9 + c ] : 1 per channel (1 with ACN_DENOISE_NO_DEMODULATE);  c = L / a.
 *                A pixel is FILTERABLE iff r[ 0 ] < inf, ( uint32 )r[ 12 ] has no ACN_SURF_EMITTER and c.x, c.y, c.z are finite.
 *                Any other pixel (a miss, an emitter, non-finite radiance) is copied to the output bit for bit and is never a tap.
 *                Two filterable pixels MATCH iff r[ 7 ], r[ 8 ] and r[ 13 ] (enter object, exit object, hops), converted to int32,
 *                are equal.  N = r[ 4 .. 6 ], P = r[ 1 .. 3 ].
 * 2 variance     lum( c ) = 0.2126 * c.x + 0.7152 * c.y + 0.0722 * c.z.  Over the 7 x 7 window around the pixel, rows outer, left
 *                to right, the in-image filterable pixels that match it (itself included): n += 1, s1 += l', s2 += l' * l'.
 *                m = s1 / n;  var = max( 0, s2 / n - m * m ).
 * 3 levels       i = 0 .. iterations - 1, stride s = 2^i, k = { 1/16, 1/4, 3/8, 1/4, 1/16 }.  The 5 x 5 taps at ( x + ( ti - 2 ) * s,
 *                y + ( tj - 2 ) * s ), tj outer, ti inner; a tap off the image or not filterable or not matching is skipped.
 *                  centre tap       w = k[ 2 ] * k[ 2 ]
 *                  any other tap    w = ( ( k[ tj ] * k[ ti ] ) * w_n ) * exp( -( t_p + t_l ) )
 *                    w_n = max( 0, dot( N, N' ) ), then normal_power_log2 times w_n = w_n * w_n
 *                    D = P' - P;  len = sqrt( dot( D, D ) );  t_p = len > 0 ? ( |dot( N, D )| / len ) / sigma_plane : 0
 *                    t_l = |l' - l| / ( sigma_lum * sqrt( var ) + 1e-8 ),  l = lum( c ), l' = lum( c' ) of the level's input,
 *                    var the centre's
 *                  sw += w;  sd += w * ( c' - c );  sv += ( w * w ) * var'
 *                c_out = c + sd / sw: the weighted mean sum( w c' ) / sum( w ), taken about the centre so that a mean of equal
 *                numbers is that number;  var_out = sv / ( sw * sw ).  The levels ping-pong between the two colour buffers.
 * 4 remodulate   out = c * a.
 * A result does not depend on which pixels share a wavefront.  What the filter is for: main-pass frames of few samples.  A pixel
 * that stands for several rays (lens samples, the positions of a gradient-cycle refinement) has no single pinhole record: reduce the
 * records of its rays with acn_surface_reduce* (acn_surface_lens* for the lens) and guide with the aggregate.  The filter is biased
 * where a texture edge is not in the albedo. */
#define ACN_DENOISE_NO_DEMODULATE     1u
#define ACN_DENOISE_NORMAL_POWER_SET  2u   /* normal_power_log2 is taken as it stands: without this flag a 0 there means the default */
#define ACN_DENOISE_DEFAULT_ITERATIONS        5
#define ACN_DENOISE_DEFAULT_NORMAL_POWER_LOG2 7
#define ACN_DENOISE_DEFAULT_SIGMA_PLANE       0.1
#define ACN_DENOISE_DEFAULT_SIGMA_LUM         4.0
#define ACN_DENOISE_MAX_ITERATIONS            8
#define ACN_DENOISE_MAX_NORMAL_POWER_LOG2     10
typedef struct acn_denoise_params
{
    uint32_t struct_size;        /* sizeof( acn_denoise_params ) as the CALLER was compiled; the library reads nothing beyond it,
                                    and members it does not reach take their defaults */
    uint32_t iterations;         /* a-trous levels 1 .. 8; 0 = default 5 */
    uint32_t normal_power_log2;  /* w_n = max( 0, N.N' )^( 2^k ) by k squarings, k 0 .. 10; 0 = default 7, unless flags has
                                    ACN_DENOISE_NORMAL_POWER_SET: then 0 is k = 0, w_n = max( 0, N.N' ) */
    uint32_t flags;              /* ACN_DENOISE_* */
    double   sigma_plane;        /* default 0.1; a member that is 0 takes its default */
    double   sigma_lum;          /* default 4.0 */
} acn_denoise_params;
#define ACN_DENOISE_PARAMS_INIT { ( uint32_t )sizeof( acn_denoise_params ), 0u, 0u, 0u, 0.0, 0.0 }
int acn_denoise_dev( acn_scene_handle* h, const void* d_linear_rgb, const void* d_surface, size_t width, size_t height,
                     const acn_denoise_params* prm /* nullable: defaults */, void* d_out_rgb, const acn_render_opts* opts );
int acn_denoise    ( acn_scene_handle* h, const double* linear_rgb, const double* surface, size_t width, size_t height,
                     const acn_denoise_params* prm, double* out_rgb, const acn_render_opts* opts );

/* Thin-lens camera: depth of field and sub-pixel jitter (k_lens.hip).  The reference has a pinhole only; the lens is a definition
 * of this library.  Every sample position gets K primary rays from the generator below; the production pipeline renders them as
 * acn_render_rays does, and the K radiances of a position are averaged on the device in the order of k.
 *
 * The ray of position ( px, py ), sample k (0 <= k < K).  Everything is IEEE binary64 without contraction, a / b is IEEE division,
 * sqrt is acn_sqrt of csrc/acn_detmath.h; f3_rnd0, f3_rnd1 (one step of the LCG each, uniform in [ -1, 1 ] and [ 0, 1 ]),
 * v_random_seed, v_of_length and m_mlv are those of csrc/acn_dev_base.h, camera_ray that of csrc/acn_dev_image.h; camera_rotation is the matrix camera_ray uses;
 * dot( a, b ) = ( a.x * b.x + a.y * b.y ) + a.z * b.z; vector sums, differences and products by a number are per component.
 *   rv = v_random_seed( ( px, py, ( double )( 2 * k + 1 ) ), ACN_LENS_SEED + seed )        (64-bit sum.  v_random_seed reads of a
 *                     component only its frexp mantissa, which 1, 2, 4, 8 ... share: the odd numbers 2 k + 1 all differ in it,
 *                     as the pixel centres i + 0.5 do, so the K samples of a position are K different samples)
 *   ACN_LENS_JITTER:  jx = f3_rnd1( &rv ) - 0.5;  jy = f3_rnd1( &rv ) - 0.5;  qx = px + jx;  qy = py + jy
 *   else              qx = px;  qy = py;  nothing is drawn
 *   ( o, d ) = camera_ray( qx, qy )
 *   aperture_radius == 0:  the ray is ( o, d ), bit for bit, and nothing more is drawn.  Else
 *     at most 32 rounds:  u = f3_rnd0( &rv );  v = f3_rnd0( &rv );  the first pair with u * u + v * v <= 1.0 is taken and ends the
 *                         rounds; if none is, u = v = 0
 *     R = m_mlv( camera_rotation, ( 1, 0, 0 ) );  V = m_mlv( camera_rotation, ( 0, 1, 0 ) );  T = m_mlv( camera_rotation, ( 0, 0, 1 ) )
 *                         (right, view and top direction of the camera)
 *     t  = focus_distance / dot( d, V )
 *     F  = o + d * t                                  the point of the plane in focus that the pinhole ray meets
 *     o' = o + ( R * ( aperture_radius * u ) + T * ( aperture_radius * v ) )
 *     the ray is ( o', v_of_length( F - o', 1 ) )
 * The mean.  L( ray ) is what acn_render_rays returns for that ray with ACN_OPT_LINEAR_OUT (a miss gives background_color);
 * sum = ( ( 0.0 + L0 ) + L1 ) + ... in the order of k;  mean = sum / ( double )K;  the output is cl_s_sat( mean ), or mean itself
 * with ACN_OPT_LINEAR_OUT.  So K = 1 without jitter and with aperture 0 is acn_render_positions, bit for bit.  A result does not
 * depend on which positions or samples share a wavefront, nor on how the call is cut into slices.
 *
 * acn_lens_rays writes the rays of samples [ first_sample, first_sample + n_samples ) of every position: out [ n ][ n_samples ][ 6 ].
 * The _dev form uses of opts only `stream` and never synchronises a caller's stream (NULL: the handle's own, and then it waits).
 * acn_render_lens*: opts as for acn_render_rays_dev: flags, cancel (polled at least between slices), stream, ACN_SHARD_SAMPLES --
 * which needs ACN_OPT_LINEAR_OUT; the mean of partial sums is then a partial mean, and the caller sum-reduces the ranks' buffers.
 * A call is cut into slices of floor( S / K ) positions, at least 1 (S: ACN_LENS_SLICE_RAYS, default 2^21, read at
 * acn_scene_upload; it changes no pixel).  Per slice the rays are made, rendered by the ray path of acn_render_rays_dev as it
 * stands (its validity check left out: the rays are valid by construction) and reduced into the caller's buffer.  The handle owns
 * one rays buffer and one radiance buffer of a slice (72 bytes per ray), apart from the render workspace and the denoiser's
 * scratch, grown on demand, freed by acn_scene_free.  acn_last_stage_ms, acn_last_counters and acn_last_kernel_ms describe the
 * render of the LAST slice.
 * ACN_ERR_ARG, checked on the host before anything is written, acn_last_error set: a null handle or (with n > 0) a null buffer;
 * samples > 4096; unknown flag bits; struct_size < 4; an aperture_radius that is negative or not finite; aperture_radius > 0 with a
 * focus_distance that is not positive and finite, or with camera_focal_length <= 0; n_samples == 0 or first_sample + n_samples > K;
 * more than 2^32 - 256 rays in one acn_lens_rays call; a pixel range outside the image; ACN_SHARD_SAMPLES without
 * ACN_OPT_LINEAR_OUT.  A null acn_lens_params is ACN_LENS_PARAMS_INIT. */
#define ACN_LENS_JITTER 1u              /* each sample's position is moved uniformly inside its pixel-sized square */
#define ACN_LENS_DEFAULT_SAMPLES 16
#define ACN_LENS_MAX_SAMPLES     4096
#define ACN_LENS_SEED            2718281828ull
typedef struct acn_lens_params
{
    uint32_t struct_size;      /* sizeof as the CALLER was compiled; nothing beyond it is read; < 4 is ACN_ERR_ARG */
    uint32_t samples;          /* K: rays per position, 1 .. 4096; 0 = default 16 */
    uint32_t flags;            /* ACN_LENS_*; unknown bits are ACN_ERR_ARG */
    uint32_t seed;             /* added to ACN_LENS_SEED: another seed, another sample set */
    double   aperture_radius;  /* lens radius in scene units, >= 0, finite; 0 = pinhole */
    double   focus_distance;   /* distance of the plane in focus from the camera position, measured ALONG the view
                                  direction; > 0 and finite whenever aperture_radius > 0, otherwise not read */
} acn_lens_params;
#define ACN_LENS_PARAMS_INIT { ( uint32_t )sizeof( acn_lens_params ), 0u, 0u, 0u, 0.0, 0.0 }

/* the rays of samples [ first_sample, first_sample + n_samples ) of every position: out [ n ][ n_samples ][ 6 ] f64 */
int acn_lens_rays    ( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, uint32_t first_sample,
                       uint32_t n_samples, double* out_rays );
int acn_lens_rays_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, uint32_t first_sample,
                       uint32_t n_samples, void* d_out_rays, const acn_render_opts* opts );
/* out_rgb[ i ] = cl_s_sat( mean over k of L( ray( i, k ) ) ); linear with ACN_OPT_LINEAR_OUT */
int acn_render_lens    ( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, double* out_rgb,
                         const acn_render_opts* opts );
int acn_render_lens_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, void* d_out_rgb,
                         const acn_render_opts* opts );
/* the same for the pixel centres [ first, first + count ) of the scene's raster (positions of acn_render_main_pass_dev) */
int acn_render_lens_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, void* d_out_rgb,
                                   const acn_render_opts* opts );

/* Lens sample statistics: how noisy each position of a lens call still is (k_lens.hip, k_denoise.hip).  A lens call sees all K
 * radiances of a position; these calls keep, beside their mean, the sum of their squared deviations, as one record per position
 * that stays on the device, can be merged with the records of another call (another seed: 2 K independent samples) and resolved
 * to a colour and a noise figure.  A sampling policy -- refine where the noise is high, stop when converged -- is the caller's
 * (tools/render_progressive.py is one): the library supplies the statistics, not the policy.
 *
 * The record, ACN_STATS_STRIDE doubles, 64 bytes; buffers of records must be 16-byte aligned (they are moved 16 bytes at a time):
 *   [ 0 ]       n     samples behind the record, stored as a double.  A record whose [ 0 ] is not a finite number >= 1 is EMPTY
 *                     (a zero-filled buffer is all EMPTY records)
 *   [ 1 .. 3 ]  mean  linear radiance per channel
 *   [ 4 .. 6 ]  m2    sum over the samples of ( L_k.c - mean.c )^2 per channel
 *   [ 7 ]       0     reserved
 * Everything is IEEE binary64 without contraction, a / b is IEEE division, sqrt is acn_sqrt of csrc/acn_detmath.h, a sum a + b + c is
 * ( a + b ) + c, lum( c ) = ( 0.2126 * c.x + 0.7152 * c.y ) + 0.0722 * c.z.  Derived from a record:
 *   vm.c  = n > 1 ? ( m2.c / ( n - 1 ) ) / n : none                      the variance of the mean
 *   noise = n > 1 ? acn_sqrt( ( ( 0.2126 * 0.2126 ) * vm.x + ( 0.7152 * 0.7152 ) * vm.y ) + ( 0.0722 * 0.0722 ) * vm.z )
 *                   / ( |lum( mean )| + ACN_STATS_NOISE_FLOOR ) : +inf       the standard error of the luminance, relative
 *
 * acn_render_lens_stats* behave exactly as acn_render_lens* do -- slices, buffers, streams, cancel, stage counters, out_rgb saturated
 * or linear by ACN_OPT_LINEAR_OUT and bit for bit what acn_render_lens* writes -- except that out_rgb may be null and that every
 * position also gets its record, which is always linear:
 *   n      = K
 *   mean.c = ( ( ( 0.0 + L0.c ) + L1.c ) + ... ) / ( double )K               the bits of acn_render_lens with ACN_OPT_LINEAR_OUT
 *   m2.c   = ( ( 0.0 + d0 * d0 ) + d1 * d1 ) + ...,  dk = Lk.c - mean.c      in the order of k: a second pass over the K samples,
 *                                                                            not the s2 / n - m * m form
 * A slice holds all K samples of each of its positions; a record does not depend on which positions share a wavefront, a workgroup
 * or a slice.  ACN_ERR_ARG, on the host before anything is written, acn_last_error set: everything acn_render_lens* refuses; a null
 * stats buffer with n > 0; a stats buffer that is not 16-byte aligned; ACN_SHARD_SAMPLES with shard_world > 1 (deviations of partial
 * radiances mean nothing).
 *
 * acn_lens_stats_merge*: for j in [ 0, n_part ), i = index ? index[ j ] : j, a = acc[ i ], b = part[ j ]:
 *   b EMPTY:  acc[ i ] is untouched.     a EMPTY:  acc[ i ] = b, bit for bit (a zero-filled accumulator is a valid start).     Else
 *   n      = na + nb
 *   dl.c   = mean_b.c - mean_a.c
 *   mean.c = mean_a.c + dl.c * ( nb / n )
 *   m2.c   = ( m2_a.c + m2_b.c ) + ( dl.c * dl.c ) * ( ( na * nb ) / n )
 *   [ 7 ]  = 0
 * A merged mean is NOT the bits of one call with na + nb samples: it equals that call to rounding (and the samples of two seeds are
 * other samples than those of one seed anyway).  A null index requires n_part <= n_acc.  In the _dev form an index outside
 * [ 0, n_acc ) is skipped -- nothing is read or written for it -- so the call never faults and never synchronises a caller's stream;
 * duplicate indices leave the records at those indices, and only those, unspecified.  The host form checks the indices first and
 * refuses any that is out of range or comes twice with ACN_ERR_ARG, nothing written.  d_index: int64_t [ n_part ] on the device.
 * acn_lens_stats_resolve_dev: out_rgb (nullable) [ n ][ 3 ] = mean, through cl_s_sat unless ACN_OPT_LINEAR_OUT; an EMPTY record gives
 * the scene's background_color the same way.  out_noise (nullable) [ n ] = noise as above; EMPTY or n == 1 gives +inf.
 * Of opts, merge and resolve use `stream` (NULL: the handle's own, and then the call waits; a caller's stream is never synchronised)
 * and resolve `flags`; shard_world > 1 is ACN_ERR_ARG, as are a null handle or buffer and a buffer that is not 16-byte aligned.
 *
 * acn_denoise_stats*: the filter of acn_denoise with the measured variance in place of the spatial guess -- steps 1 and 2 change,
 * steps 3 and 4, the parameters, the scratch memory (128 bytes per pixel) and the stream rules are those of acn_denoise.
 * 1 demodulate   L of a pixel is its record's mean.  An EMPTY record makes the pixel not FILTERABLE, and its output is the linear
 *                resolve above: background_color.  Else as in acn_denoise: a, c = L / a, FILTERABLE, MATCH, N, P.
 * 2 variance     var_raw = n > 1 ? ( ( 0.2126 * 0.2126 ) * ( vm.x / ( a.x * a.x ) ) + ( 0.7152 * 0.7152 ) * ( vm.y / ( a.y * a.y ) ) )
 *                                  + ( 0.0722 * 0.0722 ) * ( vm.z / ( a.z * a.z ) ) : none          (a negative var_raw counts as none)
 *                Over the 3 x 3 window around the pixel, rows outer, left to right, g = { 1/4, 1/2, 1/4 }: the in-image filterable
 *                pixels that match it and have a var_raw, itself included if it has one:
 *                sw += g[ j ] * g[ i ];  sv += ( g[ j ] * g[ i ] ) * var_raw'.     var = sw > 0 ? sv / sw : 0.
 *                So a pixel with one sample borrows the variance of its neighbours, and a pixel with no measured neighbour has
 *                var = 0: it is not smoothed across luminance.
 * ACN_ERR_ARG: what acn_denoise_dev refuses, and a d_stats that is not 16-byte aligned.  out_rgb is [ height * width ][ 3 ], linear.
 * What the call is for: frames of acn_render_lens_stats*.  With a closed or small aperture the pinhole records of the pixel centres
 * guide it; with a wide aperture or at anti-aliased silhouettes they do not describe the blurred frame: guide with the aggregate
 * records of acn_surface_lens* for the same acn_lens_params.  A pixel of coverage 0.55 still carries 45 % of another surface's radiance
 * and is matched to its dominant class only (acn_render_lens_layers* and acn_denoise_layers*, below, keep the two surfaces apart); like
 * acn_denoise the filter is biased where a texture edge is not in the albedo. */
#define ACN_STATS_STRIDE 8      /* doubles per record: 64 bytes */
#define ACN_STATS_NOISE_FLOOR 0.01
int acn_render_lens_stats_dev          ( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm,
                                         void* d_out_rgb /* nullable */, void* d_stats, const acn_render_opts* opts );
int acn_render_lens_stats_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm,
                                         void* d_out_rgb /* nullable */, void* d_stats, const acn_render_opts* opts );
int acn_render_lens_stats              ( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm,
                                         double* out_rgb /* nullable */, double* stats, const acn_render_opts* opts );
int acn_lens_stats_merge_dev  ( acn_scene_handle* h, void* d_acc, size_t n_acc, const void* d_part, size_t n_part,
                                const int64_t* d_index /* nullable */, const acn_render_opts* opts );
int acn_lens_stats_merge      ( acn_scene_handle* h, double* acc, size_t n_acc, const double* part, size_t n_part,
                                const int64_t* index /* nullable */, const acn_render_opts* opts );
int acn_lens_stats_resolve_dev( acn_scene_handle* h, const void* d_stats, size_t n, void* d_out_rgb /* nullable */,
                                void* d_out_noise /* nullable, [ n ] f64 */, const acn_render_opts* opts );
int acn_denoise_stats_dev( acn_scene_handle* h, const void* d_stats, const void* d_surface, size_t width, size_t height,
                           const acn_denoise_params* prm /* nullable: defaults */, void* d_out_rgb, const acn_render_opts* opts );
int acn_denoise_stats    ( acn_scene_handle* h, const double* stats, const double* surface, size_t width, size_t height,
                           const acn_denoise_params* prm, double* out_rgb, const acn_render_opts* opts );

/* Filling: the unrendered positions of a sparse frame from their rendered neighbours (k_fill.hip).  A frame of which only a subset
 * was rendered (a lattice, the positions of acn_select_above*, the history acn_reproject* kept) holds EMPTY records elsewhere, which
 * resolve and the filters show as background.  The surface records of the whole raster cost a small part of shading it and say, for
 * every position, which object it shows, through which hops, with which normal, position and albedo: which rendered neighbours a
 * position may borrow from, and which positions no neighbour explains and must be rendered.  All of it is a definition of this library.
 *   stats      [ height * width ][ ACN_STATS_STRIDE ]  records, EMPTY where nothing was rendered
 *   surface    [ height * width ][ ACN_SURF_STRIDE ]   the records of EVERY position of the raster, either mode (ACN_SURF_FOLLOW
 *              recommended, as for acn_denoise)
 *   out_stats  [ height * width ][ ACN_STATS_STRIDE ]  the records and the filled estimates
 *   out_need   [ height * width ] f64, nullable        how much each position still wants rendering
 * Everything is IEEE binary64 without contraction, a / b is IEEE division, exp and sqrt are acn_exp and acn_sqrt of
 * csrc/acn_detmath.h, a sum a + b + c is ( a + b ) + c, dot( u, v ) is ( u.x * v.x + u.y * v.y ) + u.z * v.z, max( 0, x ) is
 * x > 0 ? x : 0, and a tap that is skipped adds nothing (the preamble of acn_denoise).  Every sum starts at +0.
 * Per position, from its surface record r: a.c = r[ 9 + c ] > 0.01 ? r[ 9 + c ] : 1 (1 with ACN_DENOISE_NO_DEMODULATE), N = r[ 4 .. 6 ],
 * P = r[ 1 .. 3 ], and the KEY ( r[ 7 ], r[ 8 ], r[ 13 ] ) converted to int32: enter object, exit object, hops.  From its statistics
 * record: n, mean, m2, and vm.c = ( m2.c / ( n - 1 ) ) / n where n > 1.
 * A position is a DONOR iff its record is not EMPTY, r[ 0 ] < inf, ( uint32 )r[ 12 ] has no ACN_SURF_EMITTER and c = mean / a is finite
 * in all three channels (a FILTERABLE pixel of acn_denoise_stats).
 * Each position gets exactly one class, tested in this order:
 * 1 RENDERED    its record is not EMPTY:  out_stats = the record, bit for bit;  need = -1.0.
 * 2 BACKGROUND  r[ 0 ] is not < inf (a miss):  out_stats = { 1, background_color, 0, 0, 0, 0 } -- the colour acn_lens_stats_resolve_dev
 *               gives an EMPTY record with ACN_OPT_LINEAR_OUT;  need = 0.0.
 * 3 RECEIVER    no ACN_SURF_EMITTER in ( uint32 )r[ 12 ], and the six numbers of N and P are finite.  It gathers over the window
 *               dy = -R .. R outer, dx = -R .. R inner, R = radius; a tap ( x + dx, y + dy ) off the image is skipped (the centre is
 *               EMPTY and adds nothing).  Per tap, primes marking what is the tap's:
 *                 t_s = ( double )( dx * dx + dy * dy ) / ( sigma_px * sigma_px );   k = exp( -t_s )
 *                 the tap's record is not EMPTY:   sa += k
 *                 the tap is a DONOR and its KEY equals the receiver's, all three numbers:
 *                   w_n = max( 0, dot( N, N' ) ), then normal_power_log2 times w_n = w_n * w_n          (step 3 of acn_denoise)
 *                   D = P' - P;  len = sqrt( dot( D, D ) );  t_p = len > 0 ? ( |dot( N, D )| / len ) / sigma_plane : 0
 *                   w = w_n * exp( -( t_s + t_p ) )
 *                   sw += w;   sc.c += w * c'.c
 *                   n' > 1:   swv += w;   su.c += w * ( vm'.c / ( a'.c * a'.c ) )
 *               sw > 0: the position is FILLED:
 *                 mean.c = ( sc.c / sw ) * a.c
 *                 swv > 0:  n = 2,  m2.c = ( ( su.c / swv ) * ( a.c * a.c ) ) * 2.0  -- so that the record's vm, ( m2 / 1 ) / 2, is the
 *                           weighted mean of its donors' demodulated vm, remodulated: acn_denoise_stats filters it as it filters them
 *                 else      n = 1,  m2 = 0
 *                 [ 7 ] = 0;   need = 1.0 - sw / sa: 0 in a flat region all of whose rendered taps are of the receiver's surface, near
 *                 1 where few taps of its surface exist (w_n can exceed 1 by a rounding of dot( N, N ): need may then be a few ulp below 0)
 *               else the position is UNFILLED.
 * 4 UNFILLED    also emitters and positions whose N or P is not finite:  out_stats = the input record, bit for bit (still EMPTY);
 *               need = +inf.
 * The workflow.  The need of every rendered position is below 0, so acn_select_above_dev( need, T ) with T >= 0 is the position list of
 * the next pass: T = 0.5 asks for the positions most of whose neighbourhood is of other surfaces, and every UNFILLED one.  A filled
 * record is an estimate, not a sample: a caller keeps its sparse accumulator, merges the new pass into THAT by index (an EMPTY record
 * takes the part bit for bit) and fills again; it never merges into a filled frame.  A result does not depend on which positions share
 * a wavefront or a tile.  What the fill leaves open: a receiver none of whose window's rendered taps is of its surface, and the view
 * dependence of glossy surfaces, which the neighbours of a pixel do not share.
 * Streams, scratch and the host form are those of acn_denoise_stats: the scene is not consulted, the handle supplies the device, the
 * stream, background_color and the denoiser's scratch (128 bytes per pixel, of which the fill uses 112); work goes to opts->stream;
 * NULL is the handle's own stream, and then the call waits; a caller's stream is never synchronised; render calls before and after
 * compute the same bits.  ACN_ERR_ARG, with acn_last_error set and nothing written: a null handle or buffer (out_need may be null); a zero
 * width or height or width * height above 2^31; radius > 8; normal_power_log2 > 10; a negative or non-finite sigma; struct_size < 4;
 * unknown flag bits; shard_world > 1; stats, out_stats or surface not 16-byte aligned, out_need not 8-byte aligned; out_stats or
 * out_need overlapping stats, or each other (the gather reads its neighbours' inputs). */
#define ACN_FILL_DEFAULT_RADIUS      3
#define ACN_FILL_MAX_RADIUS          8
#define ACN_FILL_DEFAULT_SIGMA_PX    1.5
#define ACN_FILL_DEFAULT_SIGMA_PLANE 0.1
typedef struct acn_fill_params
{
    uint32_t struct_size;        /* sizeof( acn_fill_params ) as the CALLER was compiled; the library reads nothing beyond it, and
                                    members it does not reach take their defaults */
    uint32_t radius;             /* R: the window is ( 2 R + 1 )^2 taps, 1 .. 8; 0 = default 3 */
    uint32_t normal_power_log2;  /* as in acn_denoise_params: 0 .. 10; 0 = default 7 unless flags has ACN_DENOISE_NORMAL_POWER_SET */
    uint32_t flags;              /* ACN_DENOISE_NO_DEMODULATE, ACN_DENOISE_NORMAL_POWER_SET: their names and meaning reused */
    double   sigma_px;           /* default 1.5; a sigma that is 0 takes its default */
    double   sigma_plane;        /* default 0.1 */
} acn_fill_params;
#define ACN_FILL_PARAMS_INIT { ( uint32_t )sizeof( acn_fill_params ), 0u, 0u, 0u, 0.0, 0.0 }
int acn_fill_stats_dev( acn_scene_handle* h, const void* d_stats, const void* d_surface, size_t width, size_t height,
                        const acn_fill_params* prm /* nullable: defaults */, void* d_out_stats, void* d_out_need /* nullable */,
                        const acn_render_opts* opts );
int acn_fill_stats    ( acn_scene_handle* h, const double* stats, const double* surface, size_t width, size_t height,
                        const acn_fill_params* prm, double* out_stats, double* out_need /* nullable */, const acn_render_opts* opts );

/* Lens surface records: the guides of a depth-of-field frame (k_lens_surface.hip).  A pinhole record describes the one ray through
 * the sample position; at a defocused edge or an anti-aliased silhouette most of the K lens rays of the position meet something
 * else.  These calls reduce the K surface records of a position to one AGGREGATE record of the same layout (ACN_SURF_STRIDE doubles),
 * which acn_denoise*, acn_denoise_stats* and every reader of surface records take as it is (the filter reads doubles 0 .. 13 only).
 * The aggregate is a definition of this library.
 *
 * Input: for one position the records r_0 .. r_{K-1}; r_k is what acn_surface_rays writes, in the given mode, for the ray of sample k.
 * Class of a sample: ( hit, e, x, h ) with hit = r_k[ 0 ] < inf and e, x, h = r_k[ 7 ], r_k[ 8 ], r_k[ 13 ] converted to int32 -- the
 *   three numbers the filter's MATCH rule compares.  Two samples are of one class iff all four are equal.
 * Dominant class: the class with the most members; among classes with equally many, the one whose first member has the smallest k.
 *   Its members are k_1 < k_2 < ... < k_m.
 * Ordered mean of a quantity q over the members: s = q_{k_1}; s = s + q_{k_2}; ...; mean = s / ( double )m.  IEEE binary64 without
 *   contraction, IEEE division.  The sum starts at the first member, not at +0.0: with m == 1 the mean is that sample's bits, a -0.0
 *   included.
 * The dominant class is a hit:
 *   [ 0 ]              mean distance
 *   [ 1 .. 3 ]         mean position, per component
 *   [ 4 .. 6 ]         m == 1: the sample's exit_nor, bit for bit.  Else g = mean exit_nor per component,
 *                      q = ( g.x * g.x + g.y * g.y ) + g.z * g.z, and the normal is q > 0 ? g / acn_sqrt( q ) per component : ( 0, 0, 0 )
 *   [ 7 ], [ 8 ], [ 13 ] e, x, h as doubles
 *   [ 9 .. 11 ]        mean albedo, per component
 *   [ 12 ]             the bitwise OR of the members' kind bits ( ( uint32 )r_k[ 12 ] ), as a double
 *   [ 14 ]             mean weight
 *   [ 15 ]             coverage ( double )m / ( double )K
 * The dominant class is a miss: the miss record of acn_surface_rays -- inf, zeros, -1, -1, zeros, kind 0 -- with [ 13 ] = h,
 *   [ 14 ] = the mean weight of the members and [ 15 ] = the coverage.
 * So a pinhole record has [ 15 ] == 0 and an aggregate has [ 15 ] > 0; K = 1 without jitter and with aperture 0 is
 * acn_surface_positions bit for bit in doubles 0 .. 14; and a record depends on its K input records alone, not on which positions
 * share a wavefront, a workgroup or a slice.  The dominant class is exact for any K and any number of classes.
 *
 * acn_surface_reduce*: records [ n ][ K ][ ACN_SURF_STRIDE ] -> out [ n ][ ACN_SURF_STRIDE ], K 1 .. ACN_LENS_MAX_SAMPLES: the reduction
 * alone, for callers with cameras of their own (acn_surface_rays of stereo, panorama or custom lens rays).
 * acn_surface_lens*: the K rays of acn_lens_rays for every position (same acn_lens_params: with the same members, seed included, they
 * are bit for bit the rays acn_render_lens_stats* renders, so the guides describe the samples behind the statistics record), traced as
 * acn_surface_rays does in `mode`, reduced.  A call is cut into slices of floor( S / K ) positions, at least 1, exactly as
 * acn_render_lens* (S: ACN_LENS_SLICE_RAYS; it changes no record).  Per slice: the rays into the handle's lens rays buffer, the surface
 * kernel as it stands into a slice buffer of records, the reduction into the caller's buffer.  The rays are valid by construction: no
 * validity kernel runs and nothing is read back for one.  The slice buffer of records (128 bytes per ray: 268 MB at the default S) is
 * the handle's, apart from the render workspace, the denoiser's scratch, the lens buffers and the select counts, grown on demand,
 * freed by acn_scene_free.  acn_surface_lens_main_pass_dev: the pixel centres [ first, first + count ) of the scene's raster.
 * Work goes to opts->stream; NULL is the handle's own stream, and then the call waits.  A caller's stream is never synchronised (a
 * CSG stack overflow is reported as the surface calls report it).  Of opts only `stream` is used.  These calls touch no work queue,
 * counter or learned rate: renders before and after them are bit-identical and allocate nothing; acn_last_stage_ms,
 * acn_last_counters and acn_last_kernel_ms do not move, [ 23 ] and [ 24 ] included.
 * ACN_ERR_ARG, on the host before any launch, acn_last_error set, nothing written: a null handle, or a null buffer with n > 0; K == 0 or
 * K > 4096 (reduce); everything acn_render_lens* refuses of an acn_lens_params; an unknown mode; shard_world > 1; an in / out buffer
 * that is not 16-byte aligned; a pixel range outside the image.  n == 0 is ACN_OK with no launch. */
int acn_surface_reduce_dev( acn_scene_handle* h, const void* d_records, size_t n, uint32_t K, void* d_out, const acn_render_opts* opts );
int acn_surface_reduce    ( acn_scene_handle* h, const double* records, size_t n, uint32_t K, double* out, const acn_render_opts* opts );
int acn_surface_lens_dev          ( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, uint32_t mode,
                                    void* d_out, const acn_render_opts* opts );
int acn_surface_lens_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, uint32_t mode,
                                    void* d_out, const acn_render_opts* opts );
int acn_surface_lens              ( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, uint32_t mode,
                                    double* out, const acn_render_opts* opts );

/* Layered lens records: the two largest surfaces of a position kept apart (k_lens_layers.hip), and the filter that takes each as a
 * sample of the picture of its own (k_denoise_layers.hip).  An aggregate record describes the dominant class of the K lens samples
 * only, and the statistics record beside it mixes the radiances of all classes: at a defocused edge the filter then carries the
 * minority surface's radiance into the dominant surface's neighbours.  These calls split the K samples of a position by class, give
 * every part its own statistics record and the two largest parts their own surface record, filter the two layers as
 * acn_denoise_stats filters a frame and put the pixel together again.  All of it is a definition of this library.
 * Everything is IEEE binary64 without contraction, a / b is IEEE division, a sum a + b + c is ( a + b ) + c, sqrt and exp are acn_sqrt
 * and acn_exp of csrc/acn_detmath.h.  Where a result is a NaN, which NaN it is (sign, payload) is not defined.
 *
 * The split.  Input, for one position: the surface records r_0 .. r_{K-1} as acn_surface_rays writes them in `mode` and the linear
 * radiances L_0 .. L_{K-1} as acn_render_rays returns them with ACN_OPT_LINEAR_OUT, both for the ray of sample k.
 *   Class of a sample: ( hit, e, x, h ), the class of acn_surface_reduce*.
 *   LAYER 0: the dominant class over all K samples by the rule of acn_surface_reduce*: the most members, among classes with equally
 *     many the one whose first member has the smallest k.
 *   LAYER 1: the dominant class, by the same rule, over the samples that are not in layer 0; absent if there are none.
 *   REST: every other sample.  The member counts m0 + m1 + mr = K.  The split is exact for any K <= 4096 and any number of classes.
 *   Surface record of a layer (ACN_SURF_STRIDE doubles): the aggregate record of acn_surface_reduce* taken over the layer's members
 *     alone -- every ordered mean over its members k_1 < k_2 < ..., starting at the first -- with [ 15 ] = ( double )m_l / ( double )K.
 *     Plane 0 is therefore acn_surface_reduce* of the same records bit for bit, in all 16 doubles.  An absent layer 1 is the miss
 *     record (inf in [ 0 ], -1 in [ 7 ] and [ 8 ], zeros elsewhere) with [ 13 ] = [ 14 ] = [ 15 ] = 0: its coverage 0 tells it from a layer.
 *   Statistics record of a layer or of the rest (ACN_STATS_STRIDE doubles), over its m members k_1 < k_2 < ...:
 *     n      = m
 *     mean.c = ( ( ( 0.0 + L_{k_1}.c ) + L_{k_2}.c ) + ... ) / ( double )m
 *     m2.c   = ( ( 0.0 + d * d ) + ... ),  d = L_k.c - mean.c, a second pass over the members in the order of k
 *     [ 7 ]  = 0.         No members: eight zeros, an EMPTY record.
 *     A position whose K samples are of one class has, in plane 0, the bits of the record acn_render_lens_stats* writes.
 *   Layout, planar -- every plane is a frame the existing calls take as it is (acn_denoise_stats of plane 0 of both, for one):
 *     out_surface [ ACN_LAYERS_SURFACE_PLANES = 2 ][ n ][ ACN_SURF_STRIDE ]    layer 0, layer 1
 *     out_stats   [ ACN_LAYERS_STATS_PLANES = 3 ][ n ][ ACN_STATS_STRIDE ]     layer 0, layer 1, rest
 *   A record depends on the K records and radiances of its position alone: not on which positions share a wavefront, a workgroup or
 *   a slice.  No sum is split across lanes.
 * acn_lens_layers_reduce*: records [ n ][ K ][ ACN_SURF_STRIDE ], radiance [ n ][ K ][ 3 ] -> the planes: the split alone, for callers with
 *   cameras of their own.  Of opts only `stream` is used (NULL: the handle's own, and then the call waits; a caller's stream is never
 *   synchronised).  ACN_ERR_ARG, on the host before any launch, acn_last_error set, nothing written: a null handle, or a null buffer
 *   with n > 0; K == 0 or K > 4096; shard_world > 1; records or an out buffer not 16-byte aligned, radiance not 8-byte aligned.
 *   n == 0 is ACN_OK with no launch.
 * acn_render_lens_layers*: per slice of floor( S / K ) positions, cut exactly as acn_render_lens* cut (S: ACN_LENS_SLICE_RAYS): the rays
 *   of acn_lens_rays once into the handle's lens rays buffer; rendered by the ray path of acn_render_lens_stats* into the handle's
 *   radiance buffer; traced by the surface kernel as acn_surface_lens* does, in `mode`, into the handle's slice buffer of records;
 *   split into the caller's planes.  No buffer is added to the handle.  d_out_rgb (nullable) is bit for bit what acn_render_lens*
 *   writes (saturated, or linear with ACN_OPT_LINEAR_OUT); the records are always linear.  acn_render_lens_layers_main_pass_dev: the
 *   pixel centres [ first, first + count ) of the scene's raster.  Streams, cancel, flags, acn_last_stage_ms, acn_last_counters and
 *   acn_last_kernel_ms (the render of the LAST slice) are those of acn_render_lens_stats*; a CSG stack overflow of the surface kernel
 *   is reported as acn_surface_lens* report it.  ACN_ERR_ARG, on the host before anything is written, acn_last_error set: everything
 *   acn_render_lens_stats* and acn_surface_lens* refuse -- a null handle or (n > 0) a null pos_xy, out_surface or out_stats; the
 *   acn_lens_params; an unknown mode; an unknown shard_mode; ACN_SHARD_SAMPLES with shard_world > 1; pos_xy or an out plane buffer not
 *   16-byte aligned; a pixel range outside the image.
 *
 * acn_denoise_layers*: stats [ 3 ][ width * height ][ ACN_STATS_STRIDE ], surface [ 2 ][ width * height ][ ACN_SURF_STRIDE ] as above ->
 *   out_rgb [ width * height ][ 3 ], linear.  The parameters, the stream rules and the argument checks are those of acn_denoise_stats*
 *   (both input buffers 16-byte aligned).  The scratch is 256 bytes per pixel (per layer a guide of 64 bytes and two colour buffers of
 *   32): the handle's denoise scratch, grown on demand, apart from everything a render sees.  For each pixel p and layer l in { 0, 1 }:
 *   1, 2        as in acn_denoise_stats on ( stats[ l ][ p ], surface[ l ][ p ] ): a, c = mean / a, FILTERABLE (an EMPTY record is
 *               not), the MATCH key, N, P and var_raw.
 *   CANDIDATE   of tap pixel q for the centre ( p, l ): at q == p layer l itself; else the lowest l' in { 0, 1 } for which ( q, l' ) is
 *               FILTERABLE and MATCHes ( p, l ); if there is none the tap is skipped.  So the surface a pixel sees as its minority
 *               finds the neighbours that see it as their majority.
 *   2, 3        the 3 x 3 variance prefilter and the a-trous levels of acn_denoise_stats, unchanged in every expression, with "pixel
 *               q" read as the candidate of q: its c', var', N', P' and var_raw' come from that layer's buffers of the same level.
 *               Both layers advance level by level together.
 *   4           a filterable layer gives F_l = c * a; a layer that is not filterable and not EMPTY gives F_l = mean, bit for bit.
 *   COMPOSITE   n_l = [ 0 ] of a record, 0 for an EMPTY one;  K_p = ( n0 + n1 ) + nr.  The terms, in the order layer 0, layer 1, rest:
 *               ( n0 / K_p ) * F_0.c,  ( n1 / K_p ) * F_1.c,  ( nr / K_p ) * mean_r.c.  An EMPTY record contributes no term; the sum
 *               starts at the first term present and adds the others in order; three EMPTY records give the scene's
 *               background_color, linear.  The rest is never filtered: it has no single guide.
 *   With plane 1 and the rest EMPTY everywhere the call is therefore acn_denoise_stats( stats plane 0, surface plane 0 ) bit for bit.
 * acn_lens_layers_reduce* and acn_denoise_layers* touch no work queue, counter or learned rate: renders before and after them are
 * bit-identical, acn_last_stage_ms ([ 23 ], [ 24 ] included), acn_last_counters and acn_last_kernel_ms do not move.
 *
 * acn_lens_layers_merge*: the layered records of another pass (another seed) merged into an accumulator of layered records, layer to
 * layer by surface class (k_lens_layers_merge.hip); tools/render_progressive.py --layers is a caller.  The accumulator is
 * acc_surface [ 2 ][ n_acc ][ ACN_SURF_STRIDE ] and acc_stats [ 3 ][ n_acc ][ ACN_STATS_STRIDE ], the part part_surface [ 2 ][ n_part ][ . ] and
 * part_stats [ 3 ][ n_part ][ . ].  For j in [ 0, n_part ), i = index ? index[ j ] : j, the slots of position i of the accumulator are
 * A0, A1 (a surface and a statistics record each) and Ar (statistics), those of position j of the part B0, B1, Br.
 *   PRESENT    a layer slot whose statistics record is not EMPTY.  Its KEY is ( hit, e, x, h ) of its surface record, read as
 *              acn_surface_reduce* reads a sample's: [ 0 ] < inf; [ 7 ], [ 8 ], [ 13 ] converted to int32.  n of a slot is [ 0 ] of its
 *              statistics record.
 *   Br, B0 and B1 all EMPTY (B0, B1 not PRESENT): position i is not written.  Else
 *   CLASS LIST at most four entries, each a surface record, a statistics record and a key: first the PRESENT ones of A0, A1 in that
 *              order, as they are.  Then for B0, then for B1, if PRESENT: if its key equals the key of an entry of the list it is
 *              merged into the FIRST such entry (PAIR MERGE, the entry as a, the slot as b; the entry keeps its key and its place),
 *              else it is appended as it is.
 *   PAIR MERGE statistics: the expressions of acn_lens_stats_merge* above (neither record is EMPTY).  Surface record, with na, nb the
 *              n of a and b BEFORE the merge and f = nb / ( na + nb ) (the nb / n of the statistics):
 *                the key is a hit:   [ 0 ], [ 1 .. 3 ], [ 9 .. 11 ], [ 14 ]:  q = q_a + ( q_b - q_a ) * f per component
 *                                    [ 4 .. 6 ]:  g = N_a + ( N_b - N_a ) * f per component,  q = ( g.x * g.x + g.y * g.y ) + g.z * g.z,
 *                                                 the normal is q > 0 ? g / acn_sqrt( q ) per component : ( 0, 0, 0 )
 *                                    [ 7 ], [ 8 ], [ 13 ]:  those of a, bit for bit
 *                                    [ 12 ]:  ( double )( ( uint32 )a[ 12 ] | ( uint32 )b[ 12 ] )
 *                the key is a miss:  inf, six zeros, -1, -1, four zeros, [ 13 ] of a bit for bit, [ 14 ] = w_a + ( w_b - w_a ) * f
 *                [ 15 ] is set last (COVERAGE).
 *   RANKING    the entries by their n after the merges, descending; among entries of equal n the earlier entry of the list first.
 *              The first becomes layer 0, the second layer 1.  A layer without an entry is the absent layer of the split (inf, six
 *              zeros, -1, -1, seven zeros) with a statistics record of eight zeros.
 *   REST       Ar, then Br, then the statistics of the third entry of the ranking, then of the fourth, folded left to right by
 *              acn_lens_stats_merge* with its EMPTY rules (the fold so far as a, the next as b).  The surface records of the third and
 *              fourth entry are dropped.  A rest that is still EMPTY after the fold is eight zeros.
 *   COVERAGE   n_l = n of a resulting layer, 0 for an absent one, nr = n of the resulting rest, 0 for an EMPTY one;
 *              K_p = ( n0 + n1 ) + nr;  [ 15 ] of a layer that is not absent = n_l / K_p.
 *   An entry that no slot was merged into -- a class with a single contributor -- keeps the 15 other doubles of its surface record and
 *   its whole statistics record bit for bit.
 * What follows from it:  an accumulator position whose three statistics records are EMPTY (a zero-filled accumulator is a valid
 * start) becomes the part, bit for bit in all five planes, wherever the part is what the split writes (layer 1 present only with
 * layer 0 and not larger, EMPTY records all zeros, [ 15 ] = n_l / K).  Where plane 1 and the rest are EMPTY on both sides and the keys
 * of A0 and B0 agree, statistics plane 0 is acn_lens_stats_merge* bit for bit.  n0 + n1 + nr of the result is exactly the number of
 * samples behind the six slots (sums of small integers in binary64).  Layers can swap places between passes.  A class demoted to
 * the rest stays there: the rest has no key, so if the class returns in a later pass it starts a new entry -- a stated limitation;
 * the rest has no guide and is never filtered.  A merged record is not the record one call with all the samples would write: it
 * equals it to rounding, and only while no class was demoted.
 * Index, stream and argument rules are those of acn_lens_stats_merge*: a null index requires n_part <= n_acc; in the _dev form an
 * index outside [ 0, n_acc ) is skipped -- the lane reads its index first, and nothing else is read or written for it --, duplicate
 * indices leave the records at those positions, and only those, unspecified, and a caller's stream is never synchronised; the host
 * form refuses an index that is out of range or comes twice with ACN_ERR_ARG before anything is written.  All five records of a
 * position are read from both sides before the first is written; a record depends on the six slots of its position alone, not on
 * which positions share a wavefront or a workgroup.  ACN_ERR_ARG, on the host before any launch, acn_last_error set: a null handle;
 * a null buffer with entries to hold (n_acc > 0, n_part > 0); shard_world > 1; a plane buffer that is not 16-byte aligned or a
 * d_index that is not 8-byte aligned; n_acc or n_part above 2^38.  n_part == 0 is ACN_OK with no launch.
 *
 * acn_lens_layers_resolve_dev: stats [ 3 ][ n ][ ACN_STATS_STRIDE ] -> the pixel as one population.
 *   pooled = merge( merge( s0, s1 ), sr ) by acn_lens_stats_merge* with its EMPTY rules; three EMPTY records give eight zeros.
 *   out_pooled (nullable) [ n ][ ACN_STATS_STRIDE ] = pooled, 16-byte aligned.  out_rgb (nullable) [ n ][ 3 ] and out_noise (nullable) [ n ]
 *   are acn_lens_stats_resolve_dev of pooled: the mean through cl_s_sat unless ACN_OPT_LINEAR_OUT, the scene's background_color for
 *   three EMPTY records; noise +inf for them and for n == 1.  The noise plane is what acn_select_above_dev and acn_key_histogram_dev
 *   take.  Streams, flags and refusals as for acn_lens_stats_resolve_dev; three null outputs are ACN_OK with no launch.
 * Neither call touches a work queue, counter, learned rate or acn_last_* value. */
#define ACN_LAYERS_SURFACE_PLANES 2   /* out_surface: layer 0, layer 1 */
#define ACN_LAYERS_STATS_PLANES   3   /* out_stats: layer 0, layer 1, rest */
int acn_lens_layers_reduce_dev( acn_scene_handle* h, const void* d_records, const void* d_radiance, size_t n, uint32_t K, void* d_out_surface,
                                void* d_out_stats, const acn_render_opts* opts );
int acn_lens_layers_reduce    ( acn_scene_handle* h, const double* records, const double* radiance, size_t n, uint32_t K, double* out_surface,
                                double* out_stats, const acn_render_opts* opts );
int acn_render_lens_layers_dev          ( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, uint32_t mode,
                                          void* d_out_rgb /* nullable */, void* d_out_surface, void* d_out_stats, const acn_render_opts* opts );
int acn_render_lens_layers_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, uint32_t mode,
                                          void* d_out_rgb /* nullable */, void* d_out_surface, void* d_out_stats, const acn_render_opts* opts );
int acn_render_lens_layers              ( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, uint32_t mode,
                                          double* out_rgb /* nullable */, double* out_surface, double* out_stats, const acn_render_opts* opts );
int acn_denoise_layers_dev( acn_scene_handle* h, const void* d_stats, const void* d_surface, size_t width, size_t height,
                            const acn_denoise_params* prm /* nullable: defaults */, void* d_out_rgb, const acn_render_opts* opts );
int acn_denoise_layers    ( acn_scene_handle* h, const double* stats, const double* surface, size_t width, size_t height,
                            const acn_denoise_params* prm, double* out_rgb, const acn_render_opts* opts );
int acn_lens_layers_merge_dev  ( acn_scene_handle* h, void* d_acc_surface, void* d_acc_stats, size_t n_acc, const void* d_part_surface,
                                 const void* d_part_stats, size_t n_part, const int64_t* d_index /* nullable */, const acn_render_opts* opts );
int acn_lens_layers_merge      ( acn_scene_handle* h, double* acc_surface, double* acc_stats, size_t n_acc, const double* part_surface,
                                 const double* part_stats, size_t n_part, const int64_t* index /* nullable */, const acn_render_opts* opts );
int acn_lens_layers_resolve_dev( acn_scene_handle* h, const void* d_stats, size_t n, void* d_out_rgb /* nullable */,
                                 void* d_out_noise /* nullable, [ n ] f64 */, void* d_out_pooled /* nullable */, const acn_render_opts* opts );

/* Selecting positions by a key on the device (k_select.hip): the step between acn_lens_stats_resolve_dev, which leaves a noise
 * figure per pixel in d_out_noise, and acn_render_lens_stats_dev / acn_lens_stats_merge_dev, which take an ordered index list and
 * a position list.  The library supplies the two primitives every refinement policy needs and decides nothing itself: an ordered
 * selection of the entries above a threshold, and an exact histogram of the keys from which a caller derives a threshold that
 * fits a ray budget without a sort.
 *
 * acn_select_above*: entry i of key [ n ] f64 is SELECTED iff key[ i ] > threshold, an IEEE comparison of doubles: a NaN key is
 * never selected, a +inf key is whenever threshold < +inf, -0.0 is not above 0.0.
 *   Ranks      with s_0 < s_1 < ... the selected indices in ascending order, out_index[ r ] = s_r for r < min( count, capacity )
 *   Positions  with src_pos_xy [ n ][ 2 ]:  out_pos_xy[ r ] = src_pos_xy[ s_r ], bit for bit.  Without it, W = raster_width, or the
 *              scene's image_width when that is 0, and p = raster_first + s_r:
 *                out_pos_xy[ r ] = ( ( double )( p % W ) + 0.5, ( double )( p / W ) + 0.5 )
 *              both exact in binary64 (raster_first + n <= 2^52), and with raster_width 0 the bits of the positions of pixel p in
 *              acn_render_main_pass_dev and acn_render_lens_stats_main_pass_dev
 *   Counts     d_out_count (device) and out_count (host), each nullable, receive the TOTAL number selected, also when it exceeds
 *              capacity: the caller sees that the list was cut.  Nothing is written at or beyond entry `capacity` of an out
 *              buffer, nor at or beyond entry `count`.  capacity == 0 with null out buffers is a pure count; either out buffer
 *              alone may be null
 *   Independence  a result depends on the keys, the threshold and the capacity alone: not on which entries share a wavefront, a
 *              workgroup or a tile, nor on the order in which workgroups run
 *   Streams    the work goes to opts->stream; NULL: the handle's own stream, and the call waits.  On a caller's stream the call
 *              synchronises that stream exactly once, and only when out_count is given (as acn_render_rays_dev does for its check
 *              word); with out_count == NULL it never synchronises.  Of opts only `stream` is used; shard_world > 1 is ACN_ERR_ARG
 *   Errors     ACN_ERR_ARG, checked on the host before anything is written, acn_last_error set: a null handle; a null key with
 *              n > 0; n > 2^31; a null prm (the threshold has no default); struct_size < 16; any flags bit; a NaN threshold;
 *              capacity > 0 with both out buffers null; shard_world > 1; a buffer that is not 8-byte aligned; raster positions
 *              asked for with raster_first + n > 2^52.  n == 0 is ACN_OK with count 0 and no launch
 *   Isolation  a select call uses no work queue and changes nothing a render call sees: acn_last_stage_ms, acn_last_counters and
 *              acn_last_kernel_ms stay what they were, [ 23 ] and [ 24 ] included
 * Three launches: a count per tile of 2048 entries, an exclusive scan of the tile counts by one workgroup, a scatter that recomputes
 * the predicate.  The handle owns the tile counts (8 bytes per tile), apart from the render workspace, the denoiser's scratch and
 * the lens buffers, grown on demand, freed by acn_scene_free; select calls on one handle must therefore not overlap each other.
 * Indices and counts are 64-bit.  The host form copies min( count, capacity ) entries back and nothing beyond them.
 *
 * acn_key_histogram*: out_hist [ ACN_KEY_HIST_WORDS ] uint64, overwritten (the call zeroes it itself, on the stream).  The word of
 * a key from its raw bits u, with LO = ( 1023 - 40 ) * 4:
 *   NaN (either sign)             word 256
 *   the sign bit set              bin 0 (-0.0 and -inf included)
 *   else, e = u >> 50             (the exponent and the two top mantissa bits: monotone in the key)
 *                                 bin = e < LO ? 0 : min( e - LO + 1, 255 )
 * Four bins per octave from 2^-40 upward; bin 0 is everything below 2^-40, bin 255 everything from its edge upward, +inf included.
 * The counts are exact integers and sum to n.  Streams as for acn_select_above_dev, except that this call never synchronises a
 * caller's stream.  ACN_ERR_ARG: a null handle, key (n > 0) or out_hist; n > 2^31; shard_world > 1; a buffer not 8-byte aligned.
 * n == 0 gives 257 zeros.
 * acn_key_hist_edge( j ): the lower edge of bin j, the double whose bits are ( uint64_t )( LO + j - 1 ) << 50 for j in 1 .. 255;
 * -inf for j = 0; NaN for j > 255.  No GPU, no error state.
 * acn_key_hist_threshold( hist, budget ): edge( j ) of the smallest j >= 1 with hist[ j ] + ... + hist[ 255 ] <= budget, +inf if
 * there is none (NaN for a null hist).  No GPU, no error state.  By construction acn_select_above with that threshold selects at
 * most `budget` entries: those of bins j .. 255 except the keys equal to edge( j ), which fall out (strict >).  With +inf nothing is
 * selected.  Records with one sample have noise +inf and sit in bin 255, so a budget that is to reach any pixel must be at least as
 * large as their number. */
typedef struct acn_select_params
{
    uint32_t struct_size;    /* sizeof as the CALLER was compiled; nothing beyond it is read; < 16 is ACN_ERR_ARG */
    uint32_t flags;          /* none defined: any set bit is ACN_ERR_ARG */
    double   threshold;      /* entry i is SELECTED iff key[ i ] > threshold (IEEE: a NaN key is never selected; +inf is,
                                whenever threshold < +inf).  A NaN threshold is ACN_ERR_ARG */
    uint64_t capacity;       /* entries the out buffers hold; results of rank >= capacity are not written */
    uint64_t raster_width;   /* positions without src_pos_xy: pixel centres of a raster this wide; 0 = the scene's image_width */
    uint64_t raster_first;   /* ... whose pixel `raster_first + i` is entry i */
} acn_select_params;
#define ACN_SELECT_PARAMS_INIT { ( uint32_t )sizeof( acn_select_params ), 0u, 0.0, 0u, 0u, 0u }
#define ACN_KEY_HIST_BINS 256
#define ACN_KEY_HIST_WORDS 257      /* [ 256 ]: NaN keys */
int acn_select_above_dev( acn_scene_handle* h, const void* d_key /* [ n ] f64 */, size_t n, const acn_select_params* prm,
                          const void* d_src_pos_xy /* nullable [ n ][ 2 ] */, void* d_out_index /* nullable int64 [ capacity ] */,
                          void* d_out_pos_xy /* nullable [ capacity ][ 2 ] f64 */, void* d_out_count /* nullable uint64 on the device */,
                          uint64_t* out_count /* nullable, host */, const acn_render_opts* opts );
int acn_select_above    ( acn_scene_handle* h, const double* key, size_t n, const acn_select_params* prm,
                          const double* src_pos_xy /* nullable */, int64_t* out_index /* nullable */, double* out_pos_xy /* nullable */,
                          uint64_t* out_count /* nullable */ );
int acn_key_histogram_dev( acn_scene_handle* h, const void* d_key, size_t n, void* d_out_hist /* uint64 [ 257 ], overwritten */,
                           const acn_render_opts* opts );
int acn_key_histogram    ( acn_scene_handle* h, const double* key, size_t n, uint64_t* out_hist );
double acn_key_hist_edge( uint32_t bin );                                  /* no GPU */
double acn_key_hist_threshold( const uint64_t* hist, uint64_t budget );   /* no GPU */

/* Projecting points and reprojecting sample statistics: the history of the next frame of an animation (k_reproject.hip).  A frame of
 * an animation shows mostly surface points the frame before it has sampled already.  acn_reproject* finds, for each position of the
 * new frame, where its surface point lay in the previous frame and gathers the statistics record accumulated there; the caller pools
 * it with the new frame's own samples by acn_lens_stats_merge*.  All of it is a definition of this library: the reference renders
 * single frames.  tools/render_turntable.py --temporal is a caller.
 * Everything is IEEE binary64 without contraction, a / b is IEEE division, dot( a, b ) = ( a.x * b.x + a.y * b.y ) + a.z * b.z, floor is
 * exact, sums are formed in the order written.  Where a result is a NaN, which NaN it is (sign, payload) is not defined.
 *
 * acn_project_points*: the inverse of acn_camera_rays*, with the handle's current camera (acn_scene_set_params moves it).
 *   R, V, T = m_mlv( camera_rotation, ( 1, 0, 0 ) ), m_mlv( camera_rotation, ( 0, 1, 0 ) ), m_mlv( camera_rotation, ( 0, 0, 1 ) ): right, view
 *             and top direction, as the lens forms them (m_mlv: csrc/acn_dev_base.h; camera_rotation: the matrix camera_ray uses)
 *   W = image_width, H = image_height, hh = ( double )( H >> 1 ), hw = ( double )( W >> 1 )
 *   v  = P - camera_position                (per component)
 *   ly = dot( v, V )                        the depth along the view direction: out_depth
 *   s  = camera_focal_length / ly
 *   qx = ( dot( v, R ) * s ) * hh + hw
 *   qy = hh - ( dot( v, T ) * s ) * hh
 *   PROJECTED iff ly > 0.0 (false for a NaN) and qx and qy are finite.  out_pos_xy is ( qx, qy ) then, else ( NaN, NaN ); out_depth
 *   (nullable) is ly as computed, PROJECTED or not.  So acn_project_points( origin + direction * t of acn_camera_rays( pos ) ) is pos to
 *   rounding for every t > 0.  points [ n ][ 3 ], out_pos_xy [ n ][ 2 ], out_depth [ n ], arrays of doubles.  Of opts only `stream` is
 *   used, with the rules of acn_camera_rays_dev (NULL: the handle's own stream, and the call waits; a caller's stream is never
 *   synchronised); the refusals are those of acn_camera_rays*: a null handle or (n > 0) a null points or out_pos_xy, n > 2^32 - 256.
 *
 * acn_reproject*: cur_surface [ n ][ ACN_SURF_STRIDE ] are the surface records of the current frame's positions -- any list of positions,
 * not only a raster --; prev_surface [ H' * W' ][ ACN_SURF_STRIDE ] and prev_stats [ H' * W' ][ ACN_STATS_STRIDE ] the records of the WHOLE previous
 * raster, pixel centres row-major, W' = prev_params->image_width, H' = prev_params->image_height.  prev_params is the acn_params the
 * previous frame was rendered with; it must pass the checks of acn_scene_set_params, and of it only the raster size and the four
 * camera members are read.  The handle's own scene and camera are not consulted: the handle supplies the device and the stream.
 * The previous camera's basis is formed per lane by the expressions of k_camera_setup (csrc/acn_dev_image.h: camera_rotation_of): its
 * bits are those of a handle whose params are prev_params, and the motion plane equals acn_project_points on such a handle bit for bit.
 * out_stats [ n ][ ACN_STATS_STRIDE ]; out_motion (nullable) [ n ][ 2 ].  Per current record r, in this order:
 *   1 HIT        r[ 0 ] < inf, else the motion is ( NaN, NaN ) and the record EMPTY.
 *   2 MOTION     ( qx, qy ) = the projection of P = r[ 1 .. 3 ] as above with the previous camera and W', H': where the point was on the
 *                previous raster.  Not PROJECTED: the motion is ( NaN, NaN ) and the record EMPTY.  Else the motion is ( qx, qy ).
 *   3 ELIGIBLE   iff ( ( uint32 )r[ 12 ] & reject_kinds ) == 0 and ( int32 )r[ 13 ] <= max_hops.  Else the record is EMPTY; the motion stays.
 *   4 TAPS       fx = qx - 0.5;  fy = qy - 0.5;  x0 = floor( fx );  y0 = floor( fy );  tx = fx - x0;  ty = fy - y0.  The taps, in this order:
 *                ( x0, y0 ), ( x0 + 1, y0 ), ( x0, y0 + 1 ), ( x0 + 1, y0 + 1 ) with the weights ( 1 - tx ) * ( 1 - ty ), tx * ( 1 - ty ),
 *                ( 1 - tx ) * ty, tx * ty.  A tap ( x, y ) is in the image iff x >= 0.0, x < ( double )W', y >= 0.0 and y < ( double )H',
 *                compared as doubles; only a tap in the image is converted to the index y * W' + x, and only then is anything of it read.
 *   5 VALID      a tap with weight w, previous records r' (surface) and t' (statistics), N = r[ 4 .. 6 ], D = P' - P per component, iff
 *                it is in the image;  w > 0.0;  t' is not EMPTY;  r'[ 0 ] < inf;  r'[ 7 ], r'[ 8 ], r'[ 13 ] converted to int32 equal those of
 *                r (the MATCH rule of acn_denoise);  dot( N, N' ) >= normal_min;  |dot( N, D )| <= plane_tolerance * r[ 0 ].
 *   6 GATHER     no valid tap: the record is EMPTY.  Else over the valid taps a, b, ... in the order of 4:
 *                  sw     = ( ( 0.0 + w_a ) + w_b ) ...
 *                  n      = ( ( ( 0.0 + w_a * n_a ) + w_b * n_b ) ... ) / sw
 *                  mean.c = ( ( ( 0.0 + w_a * mean_a.c ) + w_b * mean_b.c ) ... ) / sw
 *                  m2.c   = ( ( ( 0.0 + w_a * m2_a.c ) + w_b * m2_b.c ) ... ) / sw
 *                  if n > max_history:  m2.c = m2.c * ( max_history / n );  n = max_history
 *                  [ 7 ]  = 0
 *   7 EMPTY      an EMPTY record is eight zeros.
 * n is fractional; the record format allows it, and acn_lens_stats_merge*, acn_lens_stats_resolve_dev and acn_denoise_stats* take it as
 * it is.  n >= 1 holds for every record that is not EMPTY: every n_a is >= 1, so w_a * n_a >= w_a * 1.0, which is w_a; the two sums are
 * formed in the same order and rounding is monotone, so each partial sum of the w * n is >= that of the w; the quotient of x >= sw by
 * sw is >= 1 after rounding; and max_history is >= 1.  A point on a pixel centre of the previous raster has one tap of weight 1 and
 * gets that pixel's record bit for bit (( 0.0 + 1.0 * q ) / 1.0; a -0.0 becomes 0.0), up to the cap.  The cap bounds how long old samples outweigh new
 * ones: after the merge with K new samples the history holds at most max_history / ( max_history + K ) of the weight.
 * A record depends on its own current record and the four previous positions alone, not on which positions share a wavefront.
 * Limitation, stated: the WORLD IS TAKEN TO BE AT REST between the two frames -- only the camera moves.  A surface that moved off
 * its tangent plane fails the plane test and starts without history; one that moved within it, or whose light changed, keeps a
 * history that is no longer its own.  Objects that move between the frames are what acn_reproject_moving* below is for; a change
 * of the light is detected by acn_shadow_limit_history* where the caller runs it (reflections stay undetected).  With the default reject_kinds history is taken only where the radiance does not depend on the view direction (no
 * mirror, no glass, no Fresnel term); max_hops > 0 accepts records of ACN_SURF_FOLLOW behind glass or in mirrors, whose parallax
 * is not that of the surface point: the caller's risk.  Layered records (acn_lens_layers_*) are not reprojected.
 * The caller then runs acn_lens_stats_merge_dev( history, n, current statistics, n ); the library adds no fused call.
 * Work goes to opts->stream; NULL is the handle's own stream, and then the call waits.  A caller's stream is never synchronised.  Of
 * opts only `stream` is used.  The call touches no work queue, counter, learned rate or acn_last_* value.
 * ACN_ERR_ARG, on the host before any launch, acn_last_error set, nothing written: a null handle or prev_params, or (n > 0) a null
 * cur_surface, prev_surface, prev_stats or out_stats; n or W' * H' above 2^31, H' < 2 or W' < 1 (and what else acn_scene_set_params
 * refuses of prev_params); a record buffer that is not 16-byte aligned or an out_motion that is not 8-byte aligned; struct_size < 4;
 * unknown flags; a normal_min outside [ -1, 1 ] or NaN; a plane_tolerance that is negative or not finite; a max_history that is
 * not 0 and not a finite number >= 1; shard_world > 1.  n == 0 is ACN_OK with no launch. */
#define ACN_REPROJECT_KINDS_SET 1u   /* reject_kinds is taken as it stands: without this flag a 0 there means the default */
#define ACN_REPROJECT_HOPS_SET  2u   /* the same for max_hops (whose default is 0 anyway: the flag is for symmetry and for later defaults) */
#define ACN_REPROJECT_DEFAULT_REJECT_KINDS    ( ACN_SURF_CHROMATIC | ACN_SURF_FRESNEL | ACN_SURF_TRANSPARENT | ACN_SURF_CUT )
#define ACN_REPROJECT_DEFAULT_MAX_HOPS        0
#define ACN_REPROJECT_DEFAULT_NORMAL_MIN      0.9
#define ACN_REPROJECT_DEFAULT_PLANE_TOLERANCE 0.01
#define ACN_REPROJECT_DEFAULT_MAX_HISTORY     32.0
typedef struct acn_reproject_params
{
    uint32_t struct_size;      /* sizeof as the CALLER was compiled; nothing beyond it is read, members it does not reach take their
                                  defaults; < 4 is ACN_ERR_ARG */
    uint32_t flags;            /* ACN_REPROJECT_*; unknown bits are ACN_ERR_ARG */
    uint32_t reject_kinds;     /* ACN_SURF_* kind bits whose positions take no history; 0 = the default, unless ACN_REPROJECT_KINDS_SET */
    int32_t  max_hops;         /* positions of more hops take no history; default 0 */
    double   normal_min;       /* a tap needs dot( N, N' ) >= this; in [ -1, 1 ]; 0 = default 0.9; -1: no normal test */
    double   plane_tolerance;  /* a tap needs |dot( N, P' - P )| <= this * distance; >= 0, finite; 0 = default 0.01 */
    double   max_history;      /* the n a gathered record carries at most; finite, >= 1; 0 = default 32 */
} acn_reproject_params;
#define ACN_REPROJECT_PARAMS_INIT { ( uint32_t )sizeof( acn_reproject_params ), 0u, 0u, 0, 0.0, 0.0, 0.0 }
int acn_project_points    ( acn_scene_handle* h, const double* points /* [ n ][ 3 ] */, size_t n, double* out_pos_xy /* [ n ][ 2 ] */,
                            double* out_depth /* nullable [ n ] */ );
int acn_project_points_dev( acn_scene_handle* h, const void* d_points, size_t n, void* d_out_pos_xy, void* d_out_depth /* nullable */,
                            const acn_render_opts* opts );
int acn_reproject_dev( acn_scene_handle* h, const void* d_cur_surface, size_t n, const acn_params* prev_params, const void* d_prev_surface,
                       const void* d_prev_stats, const acn_reproject_params* prm /* nullable: defaults */, void* d_out_stats /* [ n ][ 8 ] */,
                       void* d_out_motion /* nullable [ n ][ 2 ] */, const acn_render_opts* opts );
int acn_reproject    ( acn_scene_handle* h, const double* cur_surface, size_t n, const acn_params* prev_params, const double* prev_surface,
                       const double* prev_stats, const acn_reproject_params* prm, double* out_stats, double* out_motion /* nullable */,
                       const acn_render_opts* opts );

/* Reprojection through moving objects: per-object motion (k_reproject.hip: k_reproject_moving; csrc/acn_motion_host.h).  acn_reproject*
 * takes the world to be at rest.  acn_reproject_moving* takes, per node index of the CURRENT scene, where a point of that object was
 * one frame ago: a surface record names the object that carries its point ([ 7 ] enter, [ 8 ] exit: node indices), a flat scene gives
 * every node a rigid frame (acn_node.pos, acn_node.rax; the local point is rax * ( P - pos )), and acn_scene_replace keeps node indices
 * stable for a scene of the same shape.  All of it is a definition of this library.  tools/render_turntable.py --spin is a caller.
 *
 * The motion table: motion [ n_motion ][ ACN_MOTION_STRIDE ] doubles, 16-byte aligned, read 16 bytes at a time; row i belongs to node i.
 *   m[ 0 .. 8 ]   A, rows x, y, z:  A.x = m[ 0 .. 2 ], A.y = m[ 3 .. 5 ], A.z = m[ 6 .. 8 ]
 *   m[ 9 .. 11 ]  t
 *   m[ 12 ]       the state: m[ 12 ] == ACN_MOTION_REST (0.0; compared as doubles, so -0.0 too) is REST, m[ 12 ] == ACN_MOTION_MOVED (1.0)
 *                 is MOVED, anything else, a NaN included, is NONE: no history for this object.  ACN_MOTION_NONE (2.0) is what
 *                 acn_motion_from_scenes writes for it
 *   m[ 13 ]       the object's own history cap: a finite value >= 1 is a cap, anything else means "the call's max_history"
 *   m[ 14 .. 15 ] 0
 * A and t are read only of a MOVED row.  With dot and the arithmetic rules of the acn_reproject block above (binary64, no contraction,
 * dot( a, b ) = ( a.x * b.x + a.y * b.y ) + a.z * b.z), for a point P and a normal N of the current frame:
 *   MOVED:  Pp = ( dot( A.x, P ) + t.x, dot( A.y, P ) + t.y, dot( A.z, P ) + t.z )      where the point was one frame ago
 *           Np = ( dot( A.x, N ), dot( A.y, N ), dot( A.z, N ) )                        how its normal pointed then
 *   REST:   Pp = P and Np = N with NO arithmetic: the row is not multiplied by an identity, which would turn a -0.0 into +0.0.
 *
 * acn_reproject_moving*: the arguments, the buffers, the stream rules and the steps of acn_reproject*, with these differences:
 *   1a OBJECT    (after 1 HIT) id = ( int32 )r[ 7 ] if that is >= 0, else ( int32 )r[ 8 ]: obj_color's rule for the object that carries
 *                the point.  id < 0 or id >= n_motion: the state is NONE; else the state, the cap and (MOVED) A and t are those of row
 *                id.  NONE: the record is EMPTY and the motion is ( NaN, NaN ).
 *   2 MOTION     projects Pp, not P: ( qx, qy ) is where the point of the moved object was on the previous raster.
 *   5 VALID      D = P' - Pp per component;  dot( Np, N' ) >= normal_min;  |dot( Np, D )| <= plane_tolerance * r[ 0 ].  The other terms stay;
 *                the MATCH rule already forces the tap to show the same object.
 *   6 GATHER     the cap is m[ 13 ] where m[ 13 ] >= 1.0 and m[ 13 ] < max_history, else max_history (so an infinite or NaN m[ 13 ] is none).
 * A table whose rows are all REST with m[ 13 ] = 0 gives the bits of acn_reproject* on every input.  The lane reads m[ 12 .. 13 ] of its
 * row first and the other 96 bytes only if the row is MOVED.
 * Limitations, stated: a moved object's own shading changes as it turns to the light, and a static surface's shading changes where a
 * mover's shadow or reflection falls.  The shadow is detected by acn_shadow_limit_history* where the caller runs it; the turning and the
 * reflection are not: the history of such a point is no longer its own.  That is what the
 * per-object cap m[ 13 ] and max_history are for: they bound how long old samples outweigh new ones.  Clipping the history to the
 * new samples' spread is a separate feature and not part of this call.  What acn_reproject* says of reject_kinds and max_hops holds.
 * ACN_ERR_ARG, on the host before any launch, acn_last_error set, nothing written: what acn_reproject* refuses, and (n > 0) a null
 * motion or n_motion == 0; a table that is not 16-byte aligned; n_motion > 2^31.  n == 0 is ACN_OK with no launch.
 *
 * acn_motion_from_scenes (no GPU; csrc/acn_motion_host.h): the table of two flat scenes, prev one frame before cur.  out_table
 * [ cur->n_nodes ][ ACN_MOTION_STRIDE ]; report (nullable) counts the rows by state.  The rules, in this order:
 *   SHAPE        the scenes have the same shape iff n_nodes, n_elems, every entry of elems, light_root, matter_root and, per node, type,
 *                child0 and child1 are equal.  If not: every row is NONE, same_shape = 0, and the status is ACN_OK.
 *   CHANGED      per node: the row is NONE if any of prm, sdf_kind, cycles, texture (and, where texture >= 0, the bytes of that
 *                acn_texture; an index outside textures counts as different) or the members color .. transparency differs bitwise: the
 *                object changed, so its radiance history is stale.  flags, env_pos and env_radius are ignored.
 *   REST         else the row is REST iff pos and rax are bitwise equal.
 *   MOVED        else the row is MOVED iff both rax are orthonormal within 1e-9: max over i, j of | dot( rax.row i, rax.row j ) - ( i == j ) |
 *                <= 1e-9 (the usual conservative margin of this library: a rule, not a measurement).  With p = prev, c = cur, rax[ k ][ i ]
 *                element i of row k:
 *                  A[ i ][ j ] = ( p.rax[ 0 ][ i ] * c.rax[ 0 ][ j ] + p.rax[ 1 ][ i ] * c.rax[ 1 ][ j ] ) + p.rax[ 2 ][ i ] * c.rax[ 2 ][ j ]      (rax_prev^T * rax_cur)
 *                  t[ i ]      = p.pos[ i ] - ( ( A[ i ][ 0 ] * c.pos[ 0 ] + A[ i ][ 1 ] * c.pos[ 1 ] ) + A[ i ][ 2 ] * c.pos[ 2 ] )
 *                  m[ 13 ]     = moved_max_history
 *                so that the point with the local coordinates rax_cur * ( P - pos_cur ) now had them at A * P + t.  If either rax is
 *                not orthonormal the row is NONE.
 *   SCALE        every node strictly below an ACN_SCALE node lives in that node's scaled frame.  It takes the row of its OUTERMOST
 *                ACN_SCALE ancestor iff every node strictly below that ancestor is equal in both scenes byte for byte (and the bytes of
 *                its texture), the ancestor's prm being equal by CHANGED.  Otherwise every node of that subtree, the ancestor
 *                included, is NONE.  (Below: child0 of ACN_SCALE and ACN_NEG, child0 and child1 of a pair, the elements of a compound,
 *                from light_root and matter_root.)
 * A row that is not MOVED is zeros but for m[ 12 ].  ACN_ERR_ARG, acn_last_error set, nothing written: a null scene or table (or null
 * nodes / elems where there are any); a NaN or negative moved_max_history, or one in ( 0, 1 ); a child or element index outside cur. */
#define ACN_MOTION_STRIDE 16
#define ACN_MOTION_REST   0.0
#define ACN_MOTION_MOVED  1.0
#define ACN_MOTION_NONE   2.0
typedef struct acn_motion_report
{
    uint32_t n_rest;       /* rows by state */
    uint32_t n_moved;
    uint32_t n_none;
    uint32_t same_shape;   /* 1 iff the SHAPE rule held */
} acn_motion_report;
int acn_motion_from_scenes( const acn_flat_scene* prev, const acn_flat_scene* cur, double moved_max_history /* 0: none */,
                            double* out_table /* [ cur->n_nodes ][ ACN_MOTION_STRIDE ] */, acn_motion_report* report /* nullable */ );
int acn_reproject_moving_dev( acn_scene_handle* h, const void* d_cur_surface, size_t n, const acn_params* prev_params, const void* d_prev_surface,
                              const void* d_prev_stats, const void* d_motion /* [ n_motion ][ ACN_MOTION_STRIDE ] */, size_t n_motion,
                              const acn_reproject_params* prm /* nullable: defaults */, void* d_out_stats /* [ n ][ 8 ] */,
                              void* d_out_motion /* nullable [ n ][ 2 ] */, const acn_render_opts* opts );
int acn_reproject_moving    ( acn_scene_handle* h, const double* cur_surface, size_t n, const acn_params* prev_params, const double* prev_surface,
                              const double* prev_stats, const double* motion, size_t n_motion, const acn_reproject_params* prm,
                              double* out_stats, double* out_motion /* nullable */, const acn_render_opts* opts );

/* Shadow records: how much of each light a surface point sees, and the guard of a reprojected history built on them (k_shadow.hip;
 * the checks that need no handle: csrc/acn_shadow_host.h).  The quantity is the direct-light loop of scene_s_lum (src/scene.c:542-581)
 * with everything but the occlusion answer left out: the shadow guide of temporal filters, and an output pass of its own
 * (tools/render_aovs.py --shadow).  tools/render_turntable.py --temporal --shadow-guard is a caller of both calls.
 *
 * acn_shadow_records*: surface [ n ][ ACN_SURF_STRIDE ] are surface records as acn_surface_rays* / acn_surface_positions* write them, first
 * hit, ACN_SURF_FOLLOW or aggregate: a record is taken as it stands, and of it only [ 0 ], [ 1 .. 3 ], [ 4 .. 6 ] and [ 12 ] are read.
 * out [ n ][ ACN_SHADOW_STRIDE ], all f64, integers stored as doubles; both buffers 16-byte aligned; each record is written whole by one
 * lane as eight 16-byte stores.  S = acn_shadow_params.samples (0: ACN_SHADOW_DEFAULT_SAMPLES), one of 1, 2, 4, 8, 16, 32, 64:
 *   [ 0 ]         state: 0 = ACN_SHADOW_NONE, 1 = ACN_SHADOW_SAMPLED
 *   [ 1 ]         S
 *   [ 2 ]         L, the number of elements of the light root
 *   [ 3 ]         asked: the samples, over all lights, that face the surface and hit their light -- the shadow rays scene_s_lum casts
 *   [ 4 ]         clear: those of asked that are not occluded
 *   [ 5 ]         asked > 0 ? clear / asked : 0.0  (IEEE division of the two doubles)
 *   [ 6 .. 10 ]   clear of lights 0 .. 4
 *   [ 11 .. 15 ]  asked of lights 0 .. 4        (lights from the sixth on count in [ 3 ] and [ 4 ] only)
 * A record r is SAMPLED iff r[ 0 ] < inf and ( uint32 )r[ 12 ] & ACN_SURF_EMITTER is 0; otherwise it is NONE: sixteen zeros.
 * A SAMPLED record, every expression the reference's in its order (src/scene.c:537-569; csrc/acn_k_shade.h is the production form):
 *   P = r[ 1 .. 3 ];  D = -r[ 4 .. 6 ] (IEEE negation per component);
 *   rv0 = random_seed( P, 3294479285 ) + random_seed( D, 3247146734 )  mod 2^64
 *   for light i in the element order of the light root:
 *     ( axis, cos_rs ) = obj_fov( light_i, P );  src_con = transposed( m_con_z( axis ) );  cyl_hgt = 1 - cos_rs
 *     for j = 0 .. S - 1:
 *       rv = acn_lcg00_jump( rv0, 2 * ( i * S + j ) );  cap = v_random_sphere_cap( &rv, cyl_hgt );  out_d = m_mlv( src_con, cap )
 *       if dot( out_d, D ) <= 0: next sample
 *       a = obj_ray_hit( light_i, ( P, out_d ) );  if a >= inf: next sample
 *       asked_i++;  if compound_s_ray_hit( matter_root, ( P, out_d ) ) > a: clear_i++
 * That is the stream scene_s_lum draws at the point whenever its own ( uint64 )( direct_samples * diffuse_intensity ) is S for every
 * light; the counts are integers, so they do not depend on the order they are formed in.  A record depends on its own input record
 * and S alone, never on which records share a wavefront (lanes are samples: S consecutive lanes share a position).
 * Of opts only `stream` is used, with the rules of acn_surface_positions_dev; the device flag word is that of the surface calls.  The
 * call touches no work queue, counter, learned rate or acn_last_* value.  ACN_ERR_ARG, on the host before any launch, acn_last_error
 * set, nothing written: a null handle or (n > 0) a null buffer; n above 2^31; a buffer that is not 16-byte aligned; struct_size < 4; an
 * unknown flag (there is none yet); an S that is not one of the seven; shard_world > 1.  n == 0 is ACN_OK with no launch.
 *
 * acn_shadow_limit_history*: the guard acn_reproject* lacks, a call of its own so that acn_reproject* keeps its bits.  stats [ n ][
 * ACN_STATS_STRIDE ], IN PLACE, is what acn_reproject[_moving]* wrote; motion [ n ][ 2 ] is that call's out_motion; cur_shadow [ n ][
 * ACN_SHADOW_STRIDE ] the shadow records of the same positions; prev_shadow [ H' * W' ][ ACN_SHADOW_STRIDE ] those of the WHOLE previous
 * raster, row-major; out_change (nullable) [ n ].  Arithmetic as in the acn_reproject block (binary64, no contraction, IEEE division,
 * floor exact).  max( m, t ) below is t if t > m, else m: a NaN term leaves m as it is.  Per position, in this order:
 *   1 HISTORY    the statistics record is EMPTY, or a motion component ( qx, qy ) is a NaN: the record is untouched, change = NaN.
 *   2 PLACE      x = floor( qx ), y = floor( qy ); in the image iff x >= 0.0, x < ( double )W', y >= 0.0 and y < ( double )H', compared as
 *                doubles; only then is it converted to the index y * W' + x, and only then is anything of it read.  Not in the image:
 *                untouched, change = NaN.
 *   3 SAMPLED    c = cur_shadow[ i ], p = prev_shadow[ y * W' + x ]; c[ 0 ] == 1.0 and p[ 0 ] == 1.0, else: untouched, change = NaN.
 *   4 CHANGE     m = 0.0;  for l = 0 .. 4 with ( double )l < c[ 2 ]:  m = max( m, | c[ 6 + l ] / c[ 1 ] - p[ 6 + l ] / p[ 1 ] | );
 *                m = max( m, | c[ 4 ] / ( c[ 1 ] * c[ 2 ] ) - p[ 4 ] / ( p[ 1 ] * p[ 2 ] ) | );  change = m.
 *   5 LIMIT      if change > tolerance:  with ACN_SHADOW_HISTORY_DROP the record becomes eight zeros;  otherwise, if n > cap:
 *                m2.c = m2.c * ( cap / n ), then n = cap (the expressions of acn_reproject step 6; mean and [ 7 ] stay).
 *   6            in every other case the record is untouched.  A lane writes nothing of a record it leaves untouched.
 * What follows: with a resting camera and a resting world the positions, and therefore the seeds, are the previous frame's bit for bit;
 * change is then exactly 0 everywhere and nothing is limited.  With a moving camera the sampling noise of a penumbra can exceed the
 * tolerance; the cost is a shorter history there, never a wrong one.  A change that reaches a point only through a mirror or through
 * glass (reflections, caustics) is not seen by a shadow record and stays undetected.
 * Stream rules and what the call leaves alone: as acn_reproject*.  ACN_ERR_ARG, on the host before any launch, acn_last_error set,
 * nothing written: a null handle or (n > 0) a null stats, motion, cur_shadow or prev_shadow; n or W' * H' above 2^31, W' < 1 or H' < 1;
 * a record buffer that is not 16-byte aligned, a motion or out_change that is not 8-byte aligned; struct_size < 4; unknown flags; a
 * tolerance that is negative or not finite; a changed_max_history that is not 0 and not a finite number >= 1; shard_world > 1.
 * n == 0 is ACN_OK with no launch. */
#define ACN_SHADOW_STRIDE 16            /* doubles per record: 128 bytes */
#define ACN_SHADOW_NONE    0.0
#define ACN_SHADOW_SAMPLED 1.0
#define ACN_SHADOW_DEFAULT_SAMPLES 16
#define ACN_SHADOW_MAX_SAMPLES     64
typedef struct acn_shadow_params
{
    uint32_t struct_size;      /* sizeof as the CALLER was compiled; < 4 is ACN_ERR_ARG (the convention of acn_reproject_params) */
    uint32_t flags;            /* none defined: any bit is ACN_ERR_ARG */
    uint32_t samples;          /* S: 1, 2, 4, 8, 16, 32 or 64; 0 = default 16 */
} acn_shadow_params;
#define ACN_SHADOW_PARAMS_INIT { ( uint32_t )sizeof( acn_shadow_params ), 0u, 0u }
#define ACN_SHADOW_HISTORY_DROP 1u      /* a changed position loses its history instead of having it capped */
#define ACN_SHADOW_HISTORY_DEFAULT_TOLERANCE   0.25
#define ACN_SHADOW_HISTORY_DEFAULT_MAX_HISTORY 1.0
typedef struct acn_shadow_history_params
{
    uint32_t struct_size;          /* as above */
    uint32_t flags;                /* ACN_SHADOW_HISTORY_*; unknown bits are ACN_ERR_ARG */
    double   tolerance;            /* a position is limited iff change > this; finite, >= 0; 0 = default 0.25 */
    double   changed_max_history;  /* cap: the n a limited record carries at most; finite, >= 1; 0 = default 1 */
} acn_shadow_history_params;
#define ACN_SHADOW_HISTORY_PARAMS_INIT { ( uint32_t )sizeof( acn_shadow_history_params ), 0u, 0.0, 0.0 }
int acn_shadow_records_dev( acn_scene_handle* h, const void* d_surface /* [ n ][ 16 ] */, size_t n, const acn_shadow_params* prm /* nullable: defaults */,
                            void* d_out /* [ n ][ ACN_SHADOW_STRIDE ] */, const acn_render_opts* opts );
int acn_shadow_records    ( acn_scene_handle* h, const double* surface, size_t n, const acn_shadow_params* prm, double* out,
                            const acn_render_opts* opts );
int acn_shadow_limit_history_dev( acn_scene_handle* h, void* d_stats /* [ n ][ 8 ], in place */, const void* d_motion /* [ n ][ 2 ] */,
                                  const void* d_cur_shadow /* [ n ][ 16 ] */, const void* d_prev_shadow /* [ prev_height * prev_width ][ 16 ] */,
                                  size_t n, size_t prev_width, size_t prev_height, const acn_shadow_history_params* prm /* nullable: defaults */,
                                  void* d_out_change /* nullable [ n ] */, const acn_render_opts* opts );
int acn_shadow_limit_history    ( acn_scene_handle* h, double* stats, const double* motion, const double* cur_shadow, const double* prev_shadow,
                                  size_t n, size_t prev_width, size_t prev_height, const acn_shadow_history_params* prm,
                                  double* out_change /* nullable */, const acn_render_opts* opts );

/* Timing of the kernels of the last render call on this handle (HIP events on the launch stream), ms. */
int acn_last_kernel_ms( acn_scene_handle* h, double* trace_ms );

/* Per-stage device time of the last render call (HIP events on the launch stream; the per-stage values [0..2], [13]
 * are zero unless the call had ACN_OPT_STAGE_TIMING, the total [3] is always measured; when the call ran on concurrent
 * lanes (ACN_LANES, default 6 for large calls) the per-stage values are SUMS over the lanes and can exceed the total)
 * and pipeline statistics:
 * out[0] walk kernels ms, [1] shade kernels ms, [2] finalize ms, [3] total ms, [4..6] launches per stage, [7] chunks,
 * [8] overflow retries, [9] path levels run, [10] peak shading tasks, [11] peak child hits, [12] slots of the largest queue,
 * [13] hard-ray kernels ms, [14] their launches, [15] hard rays, [16] rays traced by the specular walk (camera rays
 * included), [17] path-sample hits shaded (levels >= 1), [18] host synchronisations inside the pipeline (one per chunk),
 * [19] 64-ray steps of the walk kernel's waves ([16] / ( 64 * [19] ) is its lane occupancy), [20] ACN_FLAG_* bits seen
 * (8: a pixel contribution exceeded the fixed-point clamp of 16384), [21] rays the walk finished on the waves' private
 * stacks instead of in generation passes, [22] specular rays whose radiance is zero on a hit (depth 0 or intensity below
 * trace_min_intensity, src/scene.c:430) and that were therefore answered by an any-hit probe instead of a walk, [23] bytes
 * of device memory the call's work queues and ray stacks occupy (all lanes), [24] how often they were (re)allocated
 * since the upload. n <= 25. */
enum
{
    ACN_LAST_WALK_MS = 0, ACN_LAST_SHADE_MS, ACN_LAST_FINALIZE_MS, ACN_LAST_TOTAL_MS, ACN_LAST_WALK_LAUNCHES, ACN_LAST_SHADE_LAUNCHES,
    ACN_LAST_FINALIZE_LAUNCHES, ACN_LAST_CHUNKS, ACN_LAST_RETRIES, ACN_LAST_LEVELS, ACN_LAST_PEAK_TASKS, ACN_LAST_PEAK_CHILDREN,
    ACN_LAST_QUEUE_CAP, ACN_LAST_HARD_MS, ACN_LAST_HARD_LAUNCHES, ACN_LAST_HARD_RAYS, ACN_LAST_WALK_RAYS, ACN_LAST_PATH_HITS,
    ACN_LAST_HOST_SYNCS, ACN_LAST_WALK_STEPS, ACN_LAST_FLAGS, ACN_LAST_PRIVATE_RAYS, ACN_LAST_PROBE_RAYS, ACN_LAST_WORKSPACE_BYTES,
    ACN_LAST_WORKSPACE_ALLOCS,
    ACN_LAST_N   /* 25 */
};
int acn_last_stage_ms( acn_scene_handle* h, double* out, int n );

/* Work counters of the last render call (rays cast, node visits ...), see DESIGN.md: [0..7] events, [8] flop and
 * [9] transcendental calls by the cost table (ACN_OPT_COUNT_WORK).  [10 + 16 * kernel + phase] (kernel 0 walk, 1 hard
 * shadow, 2 hard path, 3 shade): shader-clock ticks the kernel's waves spent per phase, filled only by a diagnostic build
 * of the library (EXTRA_DEFS=-DACN_PHASE_TIMERS), zero otherwise. n <= 74. */
int acn_last_counters( acn_scene_handle* h, uint64_t* out, int n );

/* MC bounding-sphere estimate of src/objects.c:312-363 for node `node` of an uploaded scene (GPU). */
int acn_estimate_envelope( acn_scene_handle* h, int32_t node, uint64_t samples, uint32_t rseed,
                           double radius_factor, double* out_pos3_radius );

/* Test hook: evaluates the deterministic fp64 kernels of csrc/acn_detmath.h on the device.
 * op: 0 sin 1 cos 2 tan 3 acos 4 log 5 exp 6 pow(x,y) 7 sqrt 8 div(x/y) 9 u64->f64 (x bits) 10 frexp-mantissa
 * 11 asin 12 atan 13 atan2(x,y): x is the ordinate 14 llrint as a double (|x| < 2^62) */
int acn_detmath_eval( int device, int op, const double* x, const double* y, double* out, size_t n );

/* Test hook: the traversal shortcuts of the device (csrc/acn_dev_traverse.h, csrc/acn_dev_prune.h), one ray per lane, in the arrangement of the
 * pipeline's machine kernels (256-lane workgroups, the handle's scene, CSG stacks in LDS).  Ray i runs on lane i % 64 of
 * wave i / 64.  rays: [ n ][ 6 ] origin, direction.  limits (nullable: limit inf, no skips): [ n ][ 2 ], a limit and a
 * 64-bit skip mask (raw bits; root_occluded_fast).  out: [ n ][ ACN_QUERY_STRIDE ] doubles (integers as doubles, masks as
 * raw bits); a query on a node of the wrong kind yields NaN in out[ 0 ].  op: an ACN_Q_* value, or'ed with
 * ACN_QUERY_GLOBAL_NODES (node array read from global memory even where the handle stages it in LDS) and / or
 * ACN_QUERY_PLAIN_SCENE (the scene view without interval-prune programs and in-line simple compounds).
 *   HIT_LANE, HIT_UNI  obj_ray_hit_dev / obj_ray_hit_uni of `node`       a, normal[3]
 *   ELEMENT_HIT        element_hit, the root-element test of k_walk     a, normal[3], hit object
 *   SIDE_LANE, SIDE_UNI obj_side_dev / obj_side_uni at the origin       side
 *   PRUNE              surely_outside, prune_run( limit ), prune_run( inf ), has a program
 *   LEAF_IV            iv_ball / iv_squaroid / iv_halfspace of a leaf   lo, hi, envelope chord lo, hi
 *   TRANS              root_trans_hit on compound `node`                a, exit normal[3], exit, enter object;
 *                      root_trans_hit_fast, and where that says hard the   [ 6 .. 11 ] the same, [ 12 ] hard,
 *                      fold resumed over its candidates (k_hard_path)   [ 13 ] the candidate word
 *   OCCLUDED           root_occluded, root_occluded_fast( skip ) on compound `node`; [ 2 ] where [ 1 ] == 2: the answer of
 *                      the test resumed over the candidates (k_hard_shadow), else NaN; [ 3 ] the candidate word
 *                      (candidate word: bit i < 29: the element at position i of the compound is left to do; bit 29: one
 *                      at a position >= 29 is.  OCCLUDED: machine elements not ruled out; TRANS: also in-line elements that hit)
 *   CONE_CULL          root_cone_cull of the matter root for light `node` seen from the origin: mask, axis[3], cos theta
 *   SC_HIT             simple_compound_hit on `node`: a, normal[3], hit object, any-hit( limit )
 *   ELEMENTS           no rays: per element of compound `node` (n at most): index, ACN_Q_EL_* bits, type; out[ 3 ]:
 *                      bytes of nodes the handle stages in LDS (0: the node array is always read from global memory) */
enum acn_query_op
{
    ACN_Q_HIT_LANE = 0, ACN_Q_HIT_UNI, ACN_Q_ELEMENT_HIT, ACN_Q_SIDE_LANE, ACN_Q_SIDE_UNI, ACN_Q_PRUNE, ACN_Q_LEAF_IV,
    ACN_Q_TRANS, ACN_Q_OCCLUDED, ACN_Q_CONE_CULL, ACN_Q_SC_HIT, ACN_Q_ELEMENTS, ACN_Q_N
};
#define ACN_QUERY_GLOBAL_NODES 0x100
#define ACN_QUERY_PLAIN_SCENE  0x200
#define ACN_QUERY_STRIDE 16
#define ACN_Q_EL_FAST            1u
#define ACN_Q_EL_LEAF_PAIR       2u
#define ACN_Q_EL_SIMPLE_COMPOUND 4u
#define ACN_Q_EL_PROGRAM         8u
#define ACN_Q_EL_ENVELOPE       16u
int acn_query_rays( acn_scene_handle* h, int op, int32_t node, const double* rays, size_t n, const double* limits, void* out );

/* Test hook: one shading kernel of the pipeline alone (csrc/k_stage.hip).  acn_run_stage launches the production kernel of one stage
 * once, on queues it owns and fills from the caller's records, and fetches back everything the kernel wrote; it has no device code of
 * its own.  The records are the pipeline's own (csrc/acn_records.h: HitRec, DTask, RayTask, HardShadow, HardPath), the counter block
 * is the level's (QC_*, QS_* of csrc/acn_counts.h); acn_stage_info reports their sizes so that a caller asserts its layouts.
 *   ACN_STAGE_SHADE_HITS  k_shade_hits on in = HitRec[ n ]: the split of scene_s_lum.  Written: tasks, idx[ 0 .. 3 ], rays, hard_shadow
 *                         (the probes of dead children), counts, flags, accum.
 *   ACN_STAGE_SHADE       k_shade of size class `cls` on in = DTask[ n ] and index[ n_index ] (entries < n, or 0xFFFFFFFF: a dead
 *                         slot), whatever class the sample counts of a task ask for.  Written: children, hard_shadow, hard_path,
 *                         counts, flags, accum.  shard_rank < shard_world: the rank's share of the sample loops (0, 1: all of them).
 *   ACN_STAGE_HARD_SHADOW k_hard_shadow on in = HardShadow[ n ], the queue as the kernel meets it, dead slots included.  pad is 0 or 1
 *                         (nothing is known; bit 0: the light root counts too) or a resume word (bit 1 set, bit 0 clear).  Written:
 *                         counts, flags, accum, and hard_shadow: the queue as the kernel leaves it (the fill phase gives a probe
 *                         that is left for a machine its resume word).
 *   ACN_STAGE_HARD_PATH   k_hard_path on in = HardPath[ n ], dead slots included; resume is 0 or a resume word.  Written: children,
 *                         counts, flags, accum.
 *                         Both: `cls` is the number of workgroups of the launch (0: one per 256 records, 64 at most) -- with one
 *                         workgroup and n >= 8192 every wave draws 256 consecutive slots at a time, so a test decides what a wave's
 *                         pending list holds.  Rays are finite, limit > 0 (not NaN), depth as below.
 * Every record's pixel is < n or 0xFFFFFFFF (HitRec, HardShadow, HardPath: a dead slot, of which nothing else is read); accum is [ n ][ 3 ] raw fixed-point words (2^-40), zero before the launch.
 * The kernel variant is the handle's; ACN_STAGE_NO_PRUNE and ACN_STAGE_NO_LEAF_LIGHTS select the variant without interval-prune
 * programs / with the generic light hit (equal results), ACN_STAGE_NO_EMIT_TERMS runs the split as a shard rank > 0 does (emit_terms 0).
 * acn_stage_plan makes every check on the host and sizes the queues from the input so that none can overflow (the records the input
 * can produce at most, plus one reservation per wave of the small grid the seam launches); a caller allocates each output it
 * wants with the planned capacity, a null output is not fetched.  ACN_ERR_ARG before anything is launched, acn_last_error set: a null
 * handle, args or input; an unknown stage or flag; cls > 3 (HARD_*: > 64); a ray that is not finite, a limit that is not > 0, a pad
 * or resume word with bit 0 beside bit 1; shard_rank >= shard_world; n or n_index 0 or above ACN_STAGE_MAX_RECORDS;
 * a pixel, index entry or object (-1 .. nodes - 1) out of range; a depth outside 0 .. ACN_STAGE_MAX_DEPTH; a diffuse_intensity that is
 * not finite or asks for more than ACN_STAGE_MAX_SAMPLES samples of a loop.  A raised overflow flag is ACN_ERR_DEVICE. */
enum acn_stage { ACN_STAGE_SHADE_HITS = 0, ACN_STAGE_SHADE = 1, ACN_STAGE_HARD_SHADOW = 2, ACN_STAGE_HARD_PATH = 3, ACN_STAGE_N };
#define ACN_STAGE_NO_PRUNE       1u
#define ACN_STAGE_NO_LEAF_LIGHTS 2u
#define ACN_STAGE_NO_EMIT_TERMS  4u
/* ( 8u: ACN_STAGE_GLOBAL_NODES, the walk's ) */
/* ACN_STAGE_COUNT_WORK (acn_run_stage and acn_run_stage_walk): the launch runs the counting variant of its kernel, the one a handle
 * uploaded with ACN_OPT_COUNT_WORK runs in a render call; what it writes is what the plain variant writes.  acn_stage_last_counters
 * then returns the launch's first 10 work counters in the order of acn_last_counters (trans rays, shadow rays, object hits, lum calls,
 * cap samples, side calls, SDF evaluations, overflows, flop, transcendentals): of the last stage call of the handle, all zero if that
 * call ran without the flag.  n <= 10.  Isolation: a stage call, counting or not, moves nothing a render call reports --
 * acn_last_counters, acn_last_stage_ms and acn_last_kernel_ms stay what the last render call left. */
#define ACN_STAGE_COUNT_WORK    16u
int acn_stage_last_counters( acn_scene_handle* h, uint64_t* out, int n );
#define ACN_STAGE_MAX_RECORDS ( 1u << 20 )
#define ACN_STAGE_MAX_SAMPLES ( 1u << 16 )
#define ACN_STAGE_MAX_DEPTH   ( 1 << 20 )
typedef struct acn_stage_args
{
    uint32_t stage, flags;              /* ACN_STAGE_*, ACN_STAGE_NO_* | ACN_STAGE_COUNT_WORK */
    uint32_t cls;                       /* SHADE: size class; HARD_*: workgroups, 0 = by n */
    uint32_t shard_rank, shard_world;   /* SHADE; shard_world 0 reads as 1 */
    uint32_t n, n_index;                /* input records; SHADE: entries of index */
    uint32_t pad;
    const void* in;
    const uint32_t* index;
} acn_stage_args;
/* capacities in records, and the launch; cap_tasks also holds for each index list */
typedef struct acn_stage_caps { uint32_t cap_tasks, cap_rays, cap_children, cap_hard_shadow, cap_hard_path, grid, chunk, pad; } acn_stage_caps;
typedef struct acn_stage_out
{
    void* tasks; uint32_t* idx[ 4 ]; void* rays; void* children; void* hard_shadow; void* hard_path;
    uint32_t* counts;                   /* the counter block, acn_stage_info[ 5 ] words (word 6: the ACN_FLAG_* bits) */
    uint64_t* accum;                    /* [ n ][ 3 ] */
} acn_stage_out;
/* out[ 0 .. 4 ] sizeof RayTask, DTask, HitRec, HardShadow, HardPath; [ 5 ] words of a counter block; [ 6 ] DevScene.class0_min; [ 7 ] nodes;
 * [ 8 ] lights; [ 9 ] bit 0 prune, bit 1 leaf_lights, bit 2 the node array is staged in LDS: the kernel variant of the handle.  n <= 10 */
#define ACN_STAGE_INFO_WORDS 10
int acn_stage_info( acn_scene_handle* h, uint32_t* out, int n );
int acn_stage_plan( acn_scene_handle* h, const acn_stage_args* args, acn_stage_caps* caps );   /* no GPU work */
int acn_run_stage( acn_scene_handle* h, const acn_stage_args* args, const acn_stage_out* out );

/* Test hook: the specular walk of one path level alone (csrc/k_stage.hip): the passes of k_walk in the loop of the pipeline runner,
 *     for pass in 0 .. passes - 1:  acn_launch_walk( WalkLaunch{ pass, last = pass + 1 == passes, ... } )
 * on queues the call owns.  No device code of its own, and the arrangement of the walk is the caller's: how many launches, from which
 * size of a generation on its rays are finished on the waves' private stacks (private_limit), how many slots of a stack every launch
 * but the last uses (stack_use), the fetch batch and the grid.  The arrangement decides where a ray is traced, never what it produces.
 * Input, one of two forms:
 *   rays    in = RayTask[ n ]: generation 0 of the level as k_shade_hits or the ray seeding leaves it, dead slots (pixel 0xFFFFFFFF,
 *           of which nothing else is read) included; every other pixel is < n.
 *   camera  camera != 0, in null: n sample positions pos_xy[ n ][ 2 ], or (pos_xy null) the pixel centres first_pixel + i of the
 *           scene's raster, in the order of work of a render call (tiles of 256 positions; the launch covers every slot of the last
 *           tile, so slots past position n - 1 are met as the renderer meets them); position i is pixel i.
 * Written (acn_stage_out; a null output is not fetched): tasks, idx[ 0 .. 3 ], hard_shadow (the probes: k_hard_shadow is not run),
 * counts (the whole block: the generation marks QC_GEN + g and the statistics the planner reads), accum [ n ][ 3 ] (the walk's own
 * terms: background of a miss, emission), and rays: what the last pass left in the queue of generation `passes`, up to the mark
 * QC_GEN + passes -- the generation no launch reads.  Rays there raise no device flag (declaring the chunk lost is acn_read_chunk's).
 * room_rays: the rays the caller's model says the walk traces, all generations together (a ray has up to three children, so the
 * input does not bound the output); acn_stage_walk_plan sizes each ray buffer for room_rays, the tasks for room_rays and the probes
 * for 3 * room_rays records, each plus one reservation per wave and launch that appends to the queue (acn_stage_caps; cap_children
 * and cap_hard_path are 0, chunk is the reservation).  A raised overflow flag is ACN_ERR_DEVICE.
 * ACN_ERR_ARG before anything is launched, acn_last_error set: a null handle, args or caps; stage not ACN_STAGE_WALK; a flag other
 * than ACN_STAGE_NO_PRUNE, ACN_STAGE_NO_EMIT_TERMS, ACN_STAGE_GLOBAL_NODES (the node array read from global memory on a handle that
 * stages it in LDS, as ACN_QUERY_GLOBAL_NODES), ACN_STAGE_COUNT_WORK; both input forms or neither; n outside 1 .. ACN_STAGE_MAX_RECORDS; passes outside
 * 1 .. ACN_MAX_WALK_PASSES (32); stack_cap outside 1 .. ACN_STAGE_WALK_MAX_STACK; stack_use above stack_cap (0: stack_cap); fetch
 * outside 64 .. ACN_STAGE_MAX_RECORDS; grid above 64 (0: one workgroup per 256 input slots); room_rays below n or so large that a
 * queue would exceed 2^26 records; a live ray whose pixel is not < n, whose origin, direction or T is not finite, whose direction
 * has no length, whose depth is outside 1 .. ACN_STAGE_MAX_DEPTH or whose intensity is not finite or below the scene's
 * trace_min_intensity (the production queue never holds such a ray: spawn_child turns it into a probe). */
#define ACN_STAGE_WALK 4u                 /* the stage of acn_run_stage_walk (acn_run_stage itself has no stage 4) */
#define ACN_STAGE_GLOBAL_NODES 8u
#define ACN_STAGE_WALK_MAX_STACK 4096u
typedef struct acn_stage_walk_args
{
    uint32_t stage, flags;              /* ACN_STAGE_WALK; ACN_STAGE_NO_PRUNE | ACN_STAGE_NO_EMIT_TERMS | ACN_STAGE_GLOBAL_NODES | ACN_STAGE_COUNT_WORK */
    uint32_t n;                         /* input rays (dead slots included), or positions of the camera form */
    uint32_t camera;                    /* != 0: the camera form */
    uint32_t passes, private_limit;     /* launches of k_walk; generations of at most private_limit rays run on private stacks */
    uint32_t stack_cap, stack_use;      /* slots of a wave's stack; of them used by every launch but the last (0: all) */
    uint32_t fetch, grid;               /* input rays a wave reserves per cursor atomic; workgroups (0: by n) */
    uint32_t room_rays, pad;
    const void* in;                     /* RayTask[ n ] */
    const double* pos_xy;               /* camera form: [ n ][ 2 ], or null: the raster from first_pixel */
    uint64_t first_pixel;
} acn_stage_walk_args;
int acn_stage_walk_plan( acn_scene_handle* h, const acn_stage_walk_args* args, acn_stage_caps* caps );   /* no GPU work */
int acn_run_stage_walk( acn_scene_handle* h, const acn_stage_walk_args* args, const acn_stage_out* out );

/* ------------------------------------------------------------------------------------------------------------------ */
/* The device-resident frame (k_frame.hip): the lum_image_s of scene_s_create_image_file (src/scene.c:744-885, 1103-1159) kept on
 * the device, so that a gradient cycle moves neither positions nor colours nor the picture through the host.  A frame is an opaque
 * object owned by its handle (the host library is plain C and has no device allocator): width * height records in the layout of
 * acn_lum -- pos_x pos_y clr[ 3 ] weight, 48 bytes -- zeroed by acn_frame_create, which is the empty lum_image.  A pass is
 *     plan    the key of every pixel, the ascending list of the pixels whose key is above the threshold, their jittered positions
 *     render  the planned positions -> the frame's colour buffer (a position call: acn_render_positions_dev of them)
 *     push    the colours into the accumulator; the plan is consumed
 * and acn_frame_pass is the three in that order; acn_frame_main_pass the same with the pixel centres of every pixel as the plan.
 * actinon_amd/host/acn_driver.c keeps the loop on host arrays as a second implementation; the two give the same bits.
 * Everything is IEEE binary64 without contraction, a / b is IEEE division, sums are formed in the order written, ( double )u of a
 * uint64_t rounds to nearest even, ( int32_t )d truncates.  rec = the record of a pixel.
 *   Key        avg( rec ) = rec.clr * ( rec.weight > 0 ? 1.0 / rec.weight : 1.0 ).  With v = avg of pixel ( x, y ) and g = 0.0, for
 *              the neighbours ( x + dx, y + dy ) in the order ( -1, -1 ) ( -1, 0 ) ( -1, 1 ) ( 0, -1 ) ( 0, 1 ) ( 1, -1 ) ( 1, 0 ) ( 1, 1 ):
 *                g1 = 0.0 outside the raster, else with d = v - avg( neighbour ):  ( d.x * d.x ) + ( d.y * d.y ) + ( d.z * d.z )
 *                g  = g1 > g ? g1 : g
 *              key[ y * width + x ] = g
 *   Selection  pixel p is FLAGGED iff key[ p ] > sqr_threshold (acn_select_above_dev's comparison and launches); the index list is
 *              ascending: raster order, y outer
 *   Positions  K = samples; entry e = r * K + k belongs to the r-th flagged pixel ( i, j ):
 *                s  = acn_lcg00_jump( rval, 2 * e ),  s1 = s * ACN_LCG00_A + ACN_LCG00_C,  s2 = s1 * ACN_LCG00_A + ACN_LCG00_C
 *                pos[ e ] = ( ( double )i + ( double )s1 * 2^-64, ( double )j + ( double )s2 * 2^-64 )
 *              *out_rval = acn_lcg00_jump( rval, 2 * K * flagged ): the state of a generator that drew them one after the other.
 *              The main pass plans ( i + 0.5, j + 0.5 ) with K = 1 for every pixel and draws nothing
 *   Push       lum_image_s_push with weight 1: the target of entry e is x = ( int32_t )pos_x, y = ( int32_t )pos_y; outside the raster the
 *              entry is dropped whole, inside pos_x, pos_y, clr[ 0 ], clr[ 1 ], clr[ 2 ] and 1.0 are added to the six words of the
 *              record, each word's sum in the order of the array.  A draw of 2^64 - 1024 or more converts to exactly 1.0, and the
 *              sum i + d of a d just below 1.0 rounds up to i + 1 as well (in column 1 already for d = 1 - 2^-53, a tie to even), so an
 *              entry can land in ( i + 1, j ), ( i, j + 1 ) or ( i + 1, j + 1 ): later in the array's order than every entry of its
 *              own pixel, earlier than every entry of the target's.  Such FOREIGN entries (target != own pixel) are found first and
 *              added in ascending e by one lane; then one lane per flagged pixel adds its own K entries in order k and writes the
 *              record once
 *   Image      out_rgb[ p ] = avg( rec ); out_rgb8[ p ][ c ] = a > 0.0 ? a < 1.0 ? ( uint8_t )( a * 256 ) : 255 : 0 of a = avg( rec )[ c ]:
 *              acn_cps_from_cl, what acn_write_pnm makes of the averages
 *   Frame size width * height must be the raster of the resident scene at every render (acn_scene_replace and acn_scene_set_params
 *              may change it): a mismatch is ACN_ERR_ARG
 *   Slices     a pass of more than 2^24 positions is jittered, rendered and pushed in slices of whole pixels, in order: the bits of one
 *   Empty plan nothing flagged: no launch of render or push, *out_rval = rval, ACN_OK with *out_flagged = 0
 *   Cancel     opts->cancel reaches the render, and acn_frame_pass reads it once more before it pushes: a cancelled or failed pass
 *              leaves the accumulator as it was, drops its plan and does not write *rval
 *   Errors     ACN_ERR_ARG, on the host before anything is written, acn_last_error set: a null frame, handle or array; samples == 0 or
 *              above 65536; a NaN threshold; width * height == 0 or above 2^31, or a side of 2^31; render or push without a plan; a plan
 *              on top of a plan that no push has consumed (acn_frame_upload drops a plan); shard_world > 1
 *   Isolation  plan, push, image, upload and download use no work queue and leave acn_last_stage_ms, acn_last_counters and
 *              acn_last_kernel_ms what they were; render is a position call and reports as one
 *   Streams    every frame call works on the handle's own stream and waits; opts->stream is not used
 *   Lifetime   acn_frame_free releases a frame; acn_scene_free releases the frames its handle still has
 * acn_frame_view gives the device pointers of the frame's buffers as they are now (a plan or a larger pass may move positions and
 * colours): tests write colours there between plan and push. */
typedef struct acn_frame acn_frame;
typedef struct acn_frame_buffers
{
    uint32_t struct_size;    /* sizeof as the CALLER was compiled; nothing beyond it is written; < 8 is ACN_ERR_ARG */
    uint32_t planned;        /* 1: the frame holds a plan that no push has consumed */
    uint64_t width, height;
    uint64_t flagged, samples;   /* of that plan: positions and colours hold flagged * samples entries */
    void*    d_accumulator;  /* [ height * width ][ 6 ] f64 */
    void*    d_key;          /* [ height * width ] f64, of the last plan */
    void*    d_index;        /* int64 [ flagged ]; the main pass leaves it unused */
    void*    d_positions;    /* [ flagged * samples ][ 2 ] f64 */
    void*    d_colours;      /* [ flagged * samples ][ 3 ] f64 */
} acn_frame_buffers;
int  acn_frame_create( acn_scene_handle* h, uint64_t width, uint64_t height, acn_frame** out );
void acn_frame_free( acn_frame* f );
int  acn_frame_upload  ( acn_frame* f, const double* lum /* [ height * width ][ 6 ] */ );
int  acn_frame_download( acn_frame* f, double* lum );
int  acn_frame_main_pass( acn_frame* f, const acn_render_opts* opts );
int  acn_frame_plan  ( acn_frame* f, double sqr_threshold, uint64_t samples, uint64_t rval, uint64_t* out_flagged /* nullable */,
                       uint64_t* out_rval /* nullable */ );
int  acn_frame_render( acn_frame* f, const acn_render_opts* opts );
int  acn_frame_push  ( acn_frame* f );
int  acn_frame_pass  ( acn_frame* f, double sqr_threshold, uint64_t samples, uint64_t* rval /* in and out */, uint64_t* out_flagged /* nullable */,
                       const acn_render_opts* opts );
int  acn_frame_image ( acn_frame* f, double* out_rgb /* nullable [ height * width ][ 3 ] */, uint8_t* out_rgb8 /* nullable [ height * width ][ 3 ] */ );
int  acn_frame_view  ( acn_frame* f, acn_frame_buffers* out );
uint64_t acn_lcg00_jump( uint64_t rval, uint64_t draws );   /* no GPU: rval after `draws` steps x' = x * ACN_LCG00_A + ACN_LCG00_C */

const char* acn_last_error( void );

#ifdef __cplusplus
}
#endif

#endif /* ACTINON_HIP_H */
