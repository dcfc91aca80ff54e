/* actinon_hip.hip -- libactinon_hip.so: kernels + the C ABI of include/actinon_hip.h (gfx950 only). */
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <mutex>
#include <string>
#include <vector>
#include <functional>
#include <algorithm>
#include <thread>
#include <atomic>
#include <condition_variable>

#include "acn_launch.h"
#include "acn_tables.h"
#include "acn_chunkplan.h"
#include "acn_stats_host.h"
#include "acn_select_host.h"

/* ------------------------------------------------------------------------------------------------------------------ */
/* error plumbing */
static thread_local std::string g_last_error;
static int fail( int code, const std::string& msg ) { g_last_error = msg; return code; }
extern "C" const char* acn_last_error( void ) { return g_last_error.c_str(); }

#define HIP_TRY( expr ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) \
    return fail( ACN_ERR_DEVICE, std::string( #expr ) + ": " + hipGetErrorString( e_ ) ); } while( 0 )

struct StageEvents { hipEvent_t a, b; int stage; };

/* a persistent host thread per lane (creating a thread per call costs a HIP per-thread initialisation each time) */
struct LaneWorker
{
    std::thread thread;
    std::mutex m;
    std::condition_variable cv;
    std::function< void() > job;
    bool has_job = false, done = true, quit = false;
    void start()
    {
        thread = std::thread( [ this ]()
        {
            for( ;; )
            {
                std::function< void() > j;
                {
                    std::unique_lock< std::mutex > lk( m );
                    cv.wait( lk, [ this ] { return has_job || quit; } );
                    if( quit ) return;
                    j = job; has_job = false;
                }
                j();
                { std::lock_guard< std::mutex > lk( m ); done = true; }
                cv.notify_all();
            }
        } );
    }
    void post( std::function< void() > j )
    {
        { std::lock_guard< std::mutex > lk( m ); job = std::move( j ); has_job = true; done = false; }
        cv.notify_all();
    }
    void wait() { std::unique_lock< std::mutex > lk( m ); cv.wait( lk, [ this ] { return done; } ); }
    void stop()
    {
        if( !thread.joinable() ) return;
        { std::lock_guard< std::mutex > lk( m ); quit = true; }
        cv.notify_all();
        thread.join();
    }
};

/* Tunables, read from the environment ONCE per acn_scene_upload (never from the render path: getenv there would race a
 * host that changes its environment, and would let a value change between the concurrent lanes of one call) */
struct Tunables
{
    size_t   workspace_mb = 0;         /* ACN_WORKSPACE_MB: upper bound of the queue workspace of one handle (all its lanes); 0: 64 GiB or a
                                          quarter of the device memory that is free at upload, whichever is less */
    size_t   chunk = 0;                /* ACN_CHUNK: sample positions per pipeline run, 0 = derived from the queue capacity */
    int      lanes = 6;                /* ACN_LANES: concurrent pipeline runs of a large call (4 until round 4, each on grids twice the size: create_lane) */
    unsigned grid = 0;                 /* ACN_GRID: workgroups of the persistent kernels, 0 = 4 per compute unit */
    unsigned shade_grid = 0;           /* ACN_SHADE_GRID: workgroups of k_shade, 0 = 4 per compute unit */
    unsigned walk_grid = 0;            /* ACN_WALK_GRID: workgroups of k_walk (256 VGPRs: two of its waves fill a SIMD's register file), 0 = as ACN_GRID */
    uint32_t stack_cap = 512;          /* ACN_STACK_CAP: private ray slots per k_walk wave */
    uint32_t fetch_walk = 64;          /* ACN_FETCH_WALK: fresh rays a k_walk wave reserves per cursor atomic */
    uint32_t walk_passes = 4;          /* ACN_WALK_PASSES: launches of k_walk per path level (the last one finishes whatever is left on the waves' private
                                          stacks).  12 until round 4: with k_walk at 4 waves per SIMD the private tail is cheap and the launches are not --
                                          1080p 52.0 -> 50.3 ms, the 1/8 share 13.7 -> 12.1, c2 28.2 -> 26.3, paraffin_lamp 367 -> 339 (profiles/r04/ab_walk_passes_*) */
    uint32_t private_limit = 32768;    /* ACN_PRIVATE_LIMIT: a generation of at most this many rays is finished on private stacks */
    bool     private_limit_set = false; /* ... given by the environment: then it holds for chunks of every size (render_chunk) */
    uint32_t class0_min = 0;           /* ACN_CLASS0_MIN: shading tasks with more samples than this take the 64-lane kernel, the others 16 / 4 / 1 lanes; 0: chosen per scene (acn_scene_upload) */
    uint32_t fetch_shade = 16;         /* ACN_FETCH_SHADE: steps ( of 64 / lanes-per-task tasks ) a k_shade wave reserves per cursor atomic */
    uint32_t fetch_hard = 256;         /* ACN_FETCH_HARD: records a wave of the hard-ray kernels / k_shade_hits reserves per atomic */
    uint32_t stack_use = 0;            /* ACN_TEST_STACK_USE: slots of a private stack every walk pass but the last uses (tests of the overflow path) */
    bool     debug_chunks = false;     /* ACN_DEBUG_CHUNKS=1: one line per chunk on stderr (size, queue marks, rates, capacities) */
    bool     learn_passes = true;      /* ACN_LEARN_PASSES=0: every level gets ACN_WALK_PASSES launches of k_walk, needed or not */
    bool     learn_sample = true;      /* ACN_LEARN_SAMPLE=0: no strided learning pass on a cold handle (learn_rates): the first chunks learn, as in round 3 */
    bool     cold_pipeline = true;     /* ACN_COLD_PIPELINE=0: a cold handle makes its lanes before the learning pass, not beside it (render_lanes) */
    bool     early_lanes = false;      /* ACN_EARLY_LANES=1: the lanes a whole frame of the scene's own raster will use are made during acn_scene_upload (a
                                          helper thread beside the upload's own work, while the device is idle), not by the first call that needs them.
                                          Measured and OFF (profiles/r04/ab_early_lanes_s42.txt): the streams cost the same ~10 ms each wherever they are made
                                          and do not overlap the handle's own first stream, so the upload grows by 50 - 90 ms while the first frame loses
                                          20 - 100 (1080p 114 - 174 -> 72 - 75 ms, c2 94 - 135 -> 48 - 49, paraffin_lamp 486 - 504 -> 466 - 479, hanging_lamp
                                          417 - 426 -> 390 - 401); upload + first frame: 1080p 247 - 299 -> 277 - 323 ms, c2 189 - 261 -> 195 - 204, the
                                          lamps +30.  For a host that uploads long before it renders */
    size_t   lens_slice_rays = ( size_t )1 << 21;   /* ACN_LENS_SLICE_RAYS: rays of one slice of a lens call (acn_render_lens*): floor( this / K ) positions, at least 1 */
    bool     count_work = false;       /* ACN_COUNT_WORK */
    bool     stage_timing = false;     /* ACN_STAGE_TIMING */
    acn_table_opts tables;             /* the switches of the scene tables (acn_tables.h) */
    void read()
    {
        tables.no_leaf_pairs = getenv( "ACN_NO_LEAF_PAIRS" ) != nullptr;
        tables.no_pair2 = getenv( "ACN_NO_PAIR2" ) != nullptr;
        tables.no_prune_levels = getenv( "ACN_NO_PRUNE_LEVELS" ) != nullptr;
        tables.no_simple_compounds = getenv( "ACN_NO_SIMPLE_COMPOUNDS" ) != nullptr;
        tables.no_sc_cull = getenv( "ACN_NO_SC_CULL" ) != nullptr;
        tables.no_sc_reversed = getenv( "ACN_NO_SC_REVERSED" ) != nullptr;
        tables.verbose = getenv( "ACN_VERBOSE" ) != nullptr;
        if( const char* e = getenv( "ACN_PRUNE_MIN" ) ) tables.prune_min = ( size_t )atoll( e );
        if( const char* e = getenv( "ACN_LDS_MAX" ) ) { tables.lds_max = ( size_t )atoll( e ); tables.lds_max_set = true; }
        if( const char* e = getenv( "ACN_WORKSPACE_MB" ) ) workspace_mb = ( size_t )atoll( e );
        if( const char* e = getenv( "ACN_CHUNK" ) ) chunk = ( size_t )atoll( e );
        if( const char* e = getenv( "ACN_LANES" ) ) lanes = atoi( e );
        if( const char* e = getenv( "ACN_GRID" ) ) grid = ( unsigned )atoi( e );
        if( const char* e = getenv( "ACN_SHADE_GRID" ) ) shade_grid = ( unsigned )atoi( e );
        if( const char* e = getenv( "ACN_WALK_GRID" ) ) walk_grid = ( unsigned )atoi( e );
        if( const char* e = getenv( "ACN_STACK_CAP" ) ) stack_cap = ( uint32_t )atoll( e );
        if( const char* e = getenv( "ACN_TEST_STACK_USE" ) ) stack_use = ( uint32_t )atoll( e );
        if( const char* e = getenv( "ACN_FETCH_WALK" ) ) fetch_walk = ( uint32_t )atoll( e );
        if( const char* e = getenv( "ACN_FETCH_HARD" ) ) fetch_hard = ( uint32_t )atoll( e );
        if( const char* e = getenv( "ACN_FETCH_SHADE" ) ) fetch_shade = ( uint32_t )atoll( e );
        if( const char* e = getenv( "ACN_CLASS0_MIN" ) ) class0_min = ( uint32_t )atoll( e );
        if( fetch_shade < 1 ) fetch_shade = 1;
        if( const char* e = getenv( "ACN_WALK_PASSES" ) ) walk_passes = ( uint32_t )atoll( e );
        if( const char* e = getenv( "ACN_PRIVATE_LIMIT" ) ) { private_limit = ( uint32_t )atoll( e ); private_limit_set = true; }
        if( const char* e = getenv( "ACN_LENS_SLICE_RAYS" ) ) lens_slice_rays = ( size_t )atoll( e );
        if( lens_slice_rays < 1 ) lens_slice_rays = 1;
        if( lens_slice_rays > ( ( size_t )1 << 28 ) ) lens_slice_rays = ( size_t )1 << 28;
        if( walk_passes < 1 ) walk_passes = 1;
        if( walk_passes > ACN_MAX_WALK_PASSES ) walk_passes = ACN_MAX_WALK_PASSES;
        if( fetch_walk < 64 ) fetch_walk = 64;
        if( fetch_hard < 64 ) fetch_hard = 64;
        count_work = getenv( "ACN_COUNT_WORK" ) != nullptr;
        if( const char* e = getenv( "ACN_LEARN_PASSES" ) ) learn_passes = atoi( e ) != 0;
        if( const char* e = getenv( "ACN_LEARN_SAMPLE" ) ) learn_sample = atoi( e ) != 0;
        if( const char* e = getenv( "ACN_COLD_PIPELINE" ) ) cold_pipeline = atoi( e ) != 0;
        if( const char* e = getenv( "ACN_EARLY_LANES" ) ) early_lanes = atoi( e ) != 0;
        debug_chunks = getenv( "ACN_DEBUG_CHUNKS" ) != nullptr;
        stage_timing = getenv( "ACN_STAGE_TIMING" ) != nullptr;
        if( lanes < 1 ) lanes = 1;
        if( lanes > 16 ) lanes = 16;
        if( stack_cap < 256 ) stack_cap = 256;
        if( stack_use == 0 || stack_use > stack_cap ) stack_use = stack_cap;
    }
};

/* the queue workspace of one pipeline run */
struct Workspace
{
    DTask*      tasks = nullptr;
    uint32_t*   idx[ ACN_NCLASS ] = { nullptr, nullptr, nullptr, nullptr };
    HitRec*     children = nullptr;
    HardShadow* hard_shadow = nullptr;
    HardPath*   hard_path = nullptr;
    RayTask*    rays[ 2 ] = { nullptr, nullptr };
    RayTask*    stacks = nullptr;   size_t stack_waves = 0;
    uint32_t    cap[ 5 ] = { 0, 0, 0, 0, 0 };   /* records per queue, WQ_* */
    size_t      bytes = 0;          /* device memory of the queues and stacks */
    uint64_t    allocs = 0;         /* times this workspace was (re)allocated */
    bool        trimmed = false;    /* it was already re-allocated smaller once */
    uint32_t    sized_calls = 0;    /* calls of ensure_workspace with learned rates (the trim window, see there) */
};
/* the queues of a pipeline run.  Each is sized from its OWN demand per sample position (learned, below): on the wine glass a
 * position leaves 15 deferred shadow rays but 2 shading points, and one common capacity -- the former layout -- made every
 * queue as large as the fullest one needs (64 GiB for a 1080p frame of which 7 % were used). */
enum { WQ_TASKS = 0, WQ_CHILDREN, WQ_HARD_SHADOW, WQ_HARD_PATH, WQ_RAYS, WQ_N };
static const size_t wq_bytes[ WQ_N ] = { sizeof( DTask ) + ACN_NCLASS * sizeof( uint32_t ), sizeof( HitRec ), sizeof( HardShadow ), sizeof( HardPath ), 2 * sizeof( RayTask ) };

struct acn_scene_handle
{
    int device = 0;
    DevScene dev{};
    /* the resident scene and what the tables say about it: a lane borrows all of it from its parent (bind_lane) */
    struct Resident
    {
        GNode*   d_nodes = nullptr;
        GMat*    d_mats = nullptr;
        int32_t* d_elems = nullptr;
        acn_texture* d_textures = nullptr;
        size_t scene_bytes[ 4 ] = { 0, 0, 0, 0 };
        int max_csg_depth = 0;
        size_t lds_bytes = 0;                      /* > 0: the node array fits the LDS staging budget */
        size_t lds_stack_bytes = 0;                /* > 0: the machine kernels keep their CSG stacks in LDS */
        bool prune = false;                        /* some root element has an interval-prune program: launch the PRUNE kernel variants */
        bool leaf_lights = true;                   /* every light element is a plane / sphere */
        uint32_t elem_pos_base = 0;                /* elems[ elem_pos_base + k ]: given-order position of entry k of the cost-ordered copy (k_hard_shadow: resume words) */
        int n_levels = 1;                          /* path levels of the scene's trace_depth */
        size_t n_lights = 1;                       /* elements of the light root */
    } scene;
    SCEntry* d_sc_table = nullptr;
    double* d_sc_spheres = nullptr;            /* ( pos, radius ) of the sphere leaves of d_sc_table */
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    int cur_stage = 0;
    bool stage_timing = false;                 /* ACN_OPT_STAGE_TIMING of the current call */
    Tunables tun;
    unsigned cus = 256;                        /* compute units of the device */
    unsigned grid = 1024, shade_grid = 1024;   /* workgroups of the persistent kernels / of k_shade */
    unsigned walk_grid = 1024;                 /* ... of k_walk */
    /* workspace of the wavefront pipeline */
    Workspace ws;
    uint32_t* d_counts = nullptr;              /* ACN_MAX_PATH_LEVELS + 1 counter blocks of QC_N words */
    uint32_t* h_counts = nullptr;              /* pinned copy */
    unsigned long long* d_accum = nullptr;  size_t accum_cap = 0;
    unsigned long long* d_counters = nullptr;
    std::vector< StageEvents > events;  size_t events_used = 0;
    bool count_work = false;                   /* ACN_OPT_COUNT_WORK of the current call */
    uint32_t shard_rank = 0, shard_world = 1;  /* ACN_SHARD_SAMPLES of the current call */
    uint64_t launches[ 4 ] = { 0, 0, 0, 0 };   /* walk, shade, finalize, hard-ray kernels */
    uint64_t hard_rays = 0, walk_steps = 0, walk_rays = 0, shade_hit_recs = 0, host_syncs = 0, private_rays = 0, probe_rays = 0;
    uint32_t flags_seen = 0;                   /* ACN_FLAG_* bits of the last call */
    uint32_t rate_cnt = 0;                     /* positions of the chunk the rates were taken from */
    acn_chunk_ctl ctl = { 0.7, 0, 0 };         /* acn_chunkplan.h.  fill_target: fraction of its capacity the fullest queue of a chunk is
                                                  planned to reach: lowered by every overflow (a redone chunk is lost work), raised slowly
                                                  by chunks that fit */
    double rate[ 5 ] = { 0, 0, 0, 0, 0 };      /* learned: records per sample position a chunk leaves in each queue (WQ_*); 0: not known yet */
    size_t workspace_budget = 0;               /* bytes this handle's queues may take (all lanes together) */
    uint64_t chunks = 0, retries = 0, levels = 0;
    uint64_t peak_tasks = 0, peak_children = 0;
    uint32_t walk_passes_seen[ ACN_MAX_PATH_LEVELS + 1 ] = { 0, 0, 0, 0, 0, 0 };   /* learned: passes of a level that had input in the last chunk (0: not known yet) */
    unsigned long long* d_counters_keep = nullptr;   /* the work counters as they were before the current chunk (restored when it is redone) */
    /* concurrent lanes (render_lanes): clones of this handle that share the resident scene and own a stream and a
     * workspace each */
    bool is_lane = false;
    size_t budget_div = 1;                     /* workspace budget of a lane = the handle's budget / lanes */
    std::vector< acn_scene_handle* > lanes;
    /* lanes made during acn_scene_upload on a helper thread (early_lanes_begin), taken over by the first call that runs on lanes */
    std::thread early_maker;
    std::vector< acn_scene_handle* > early_made;
    int early_status = 0; std::string early_message;
    LaneWorker* worker = nullptr;              /* of a lane */
    double* d_lane_in = nullptr; size_t lane_in_cap = 0;       /* a lane's gathered positions or rays (doubles) */
    double* d_lane_out = nullptr; size_t lane_out_cap = 0;     /* ... and its results */
    double* d_shard_pos = nullptr; size_t shard_pos_cap = 0;                                /* acn_render_main_pass_shard_dev: the rank's positions */
    unsigned long long* d_ray_check = nullptr;                                              /* acn_render_rays_dev: the lowest index of a refused ray */
    uint32_t* d_surface_flags = nullptr;                                                    /* acn_surface_*: the ACN_FLAG_* word of the surface kernels (not the pipeline's) */
    void* d_denoise = nullptr; size_t denoise_bytes = 0;                                    /* acn_denoise: guides and colour buffers, apart from the render workspace */
    double* d_lens_rays = nullptr; double* d_lens_rad = nullptr; size_t lens_cap = 0;       /* acn_render_lens*: the rays [ 6 ] and the radiance [ 3 ] of a slice, lens_cap rays each */
    unsigned long long* d_select_tiles = nullptr; size_t select_tiles_cap = 0;              /* acn_select_above*: the counts per tile and their total, select_tiles_cap words */
    bool seeded = false;                       /* the current call renders the caller's rays (Primary): its ray queue has a known demand (demand) */
    std::string lane_error;
    bool used_lanes = false;                   /* the last render call ran through the lanes: statistics are their sums */
    int  lanes_used = 0;                       /* ... the first lanes_used of them */
    bool one_lane = false;                     /* the last call would have used lanes but did not fit the workspace bound that way */
};
#define ACN_LEVEL_BLOCKS ( ACN_MAX_PATH_LEVELS + 1 )

/* ------------------------------------------------------------------------------------------------------------------ */
/* kernels */

/* camera basis with the oracle's expressions (scene.c:963-973), one lane */
__global__ void k_camera_setup( DevScene sc, M3* out_rot, double* out_unit_f )
{
    uint64_t unit_sz = ( sc.prm.image_height >> 1 );
    *out_unit_f = 1.0 / unit_sz;
    V3 ry = v_of_length( ld3( sc.prm.camera_view_direction ), 1 );
    V3 rz = v_of_length( ld3( sc.prm.camera_top_direction ), 1 );
    rz = v_von( ry, rz );
    V3 rx = v_mlx( ry, rz );
    M3 r; r.x = rx; r.y = ry; r.z = rz;
    *out_rot = m_transposed( r );
}

/* fixed point -> f64 (+ optional cl_s_sat) for positions [ base, base + n ) */
__global__ void k_finalize( const unsigned long long* __restrict__ accum, uint32_t n, double gamma, int linear,
                            double* __restrict__ out_rgb )
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    V3 c = mk( ( double )( long long )accum[ ( size_t )i * 3 + 0 ] * ACN_FIX_INV,
               ( double )( long long )accum[ ( size_t )i * 3 + 1 ] * ACN_FIX_INV,
               ( double )( long long )accum[ ( size_t )i * 3 + 2 ] * ACN_FIX_INV );
    if( !linear ) c = cl_sat( c, gamma );
    out_rgb[ ( size_t )i * 3 + 0 ] = c.x;
    out_rgb[ ( size_t )i * 3 + 1 ] = c.y;
    out_rgb[ ( size_t )i * 3 + 2 ] = c.z;
}

/* the pixel sums of the positions in slots [ base, base + cnt ) start over (a chunk is redone after a queue overflow) */
__global__ void k_clear_slots( unsigned long long* __restrict__ accum, uint32_t base, uint32_t cnt, TileOrder order )
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= cnt ) return;
    uint32_t p = order.position( base + i );
    if( p >= order.n ) return;
    accum[ ( size_t )p * 3 + 0 ] = 0; accum[ ( size_t )p * 3 + 1 ] = 0; accum[ ( size_t )p * 3 + 2 ] = 0;
}

/* cl_s_sat + cps_from_cl after the (cross-GPU) accumulation */
__global__ void k_resolve( const double* __restrict__ lin, size_t n, double gamma, double* __restrict__ out_rgb,
                           unsigned char* __restrict__ out_rgb8 )
{
    size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    V3 c = cl_sat( mk( lin[ i * 3 ], lin[ i * 3 + 1 ], lin[ i * 3 + 2 ] ), gamma );
    if( out_rgb ) { out_rgb[ i * 3 ] = c.x; out_rgb[ i * 3 + 1 ] = c.y; out_rgb[ i * 3 + 2 ] = c.z; }
    if( out_rgb8 )
    {
        out_rgb8[ i * 3 + 0 ] = c.x > 0.0 ? c.x < 1.0 ? ( unsigned char )( c.x * 256 ) : 255 : 0;
        out_rgb8[ i * 3 + 1 ] = c.y > 0.0 ? c.y < 1.0 ? ( unsigned char )( c.y * 256 ) : 255 : 0;
        out_rgb8[ i * 3 + 2 ] = c.z > 0.0 ? c.z < 1.0 ? ( unsigned char )( c.z * 256 ) : 255 : 0;
    }
}

/* obj_ray_exit + obj_estimate_envelope (objects.c:286-363), one lane */
__global__ void k_estimate_envelope( DevScene sc, int node, uint64_t samples, uint32_t rseed, double radius_factor,
                                     V3* scratch, double* out )
{
    Cnt< false > cnt;
    NodeP hdr = &sc.nodes[ node ];
    uint64_t size = 0;
    V3 sum = mk( 0, 0, 0 );
    uint64_t rv = rseed;
    V3 rp = ld3( hdr->pos );
    for( uint64_t i = 0; i < samples; i++ )
    {
        V3 rd = v_random_sphere_belt( &rv, 1.0 );
        /* obj_ray_exit */
        double exit_a = F3_INF;
        {
            V3 nor = mk( 0, 0, 0 );
            double a = obj_ray_hit_dev( sref( sc ), node, rp, rd, true, &nor, &cnt );
            if( a < F3_INF )
            {
                V3 lp = rp;
                double s = 0;
                while( a < F3_INF )
                {
                    a += F3_EPS * 2;
                    s += a;
                    lp = ray_pos( lp, rd, a );
                    a = obj_ray_hit_dev( sref( sc ), node, lp, rd, true, &nor, &cnt );
                }
                if( v_mlv( nor, rd ) > 0 ) exit_a = s;
            }
        }
        if( exit_a < F3_INF )
        {
            V3 pos = ray_pos( rp, rd, exit_a );
            scratch[ size++ ] = pos;
            sum = v_add( sum, ray_pos( rp, rd, exit_a ) );
            rp = v_mlf( sum, ( 1.0 / size ) );
            rp.x += F3_EPS * f3_rnd0( &rv );
            rp.y += F3_EPS * f3_rnd0( &rv );
            rp.z += F3_EPS * f3_rnd0( &rv );
        }
    }
    double radius = F3_MAG;
    if( size > 0 )
    {
        double max_r2 = 0;
        for( uint64_t i = 0; i < size; i++ )
        {
            double r = v_diff_sqr( rp, scratch[ i ] );
            max_r2 = r > max_r2 ? r : max_r2;
        }
        radius = acn_sqrt( max_r2 ) * radius_factor;
    }
    out[ 0 ] = rp.x; out[ 1 ] = rp.y; out[ 2 ] = rp.z; out[ 3 ] = radius;
}

__global__ void k_detmath( int op, const double* x, const double* y, double* out, size_t n )
{
    size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    double a = x[ i ], b = y ? y[ i ] : 0.0, r = 0;
    switch( op )
    {
        case 0: r = acn_sin( a ); break;
        case 1: r = acn_cos( a ); break;
        case 2: r = acn_tan( a ); break;
        case 3: r = acn_acos( a ); break;
        case 4: r = acn_log( a ); break;
        case 5: r = acn_exp( a ); break;
        case 6: r = acn_pow( a, b ); break;
        case 7: r = acn_sqrt( a ); break;
        case 8: r = a / b; break;
        case 9: r = ( double )acn_f64_bits( a ); break;
        case 10: r = acn_frexp_mant( a ); break;
        default: break;
    }
    out[ i ] = r;
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* ABI */
extern "C" int acn_device_count( void )
{
    int n = 0;
    if( hipGetDeviceCount( &n ) != hipSuccess ) return 0;
    return n;
}

static int lane_objects( int device, bool debug, acn_scene_handle** out );
static int lanes_for_counts( int tun_lanes, size_t n, uint64_t path_samples );

/* Lanes made during the upload.  A stream that gets its own hardware queue costs ~10 ms of host time, and making one while kernels
 * run stretches those kernels too (the learning pass of a cold handle: 19 ms alone, 56 - 150 ms beside six streams being made,
 * profiles/r04/upload_timeline_s41.txt) -- so the lanes a whole frame of the scene's own raster will use are made here, on a helper
 * thread beside the upload's host work and copies, while nothing of this handle runs on the device (ACN_EARLY_LANES=1; off by
 * default: the runtime makes streams one after the other, so the time only moves from the first call into the upload).  A handle that would render its
 * raster on one lane (small rasters, path_samples >= 256 on a cold handle: render_positions) makes none.  Failures are not reported
 * from here: the first call that needs the lanes makes what is missing and reports its own. */
static void early_lanes_begin( acn_scene_handle* h, size_t n, uint64_t path_samples )
{
    const int lanes = lanes_for_counts( h->tun.lanes, n, path_samples );
    if( lanes <= 1 || path_samples >= 256 ) return;
    const int device = h->device; const bool debug = h->tun.debug_chunks;
    h->early_maker = std::thread( [ h, lanes, device, debug ]()
    {
        for( int k = 0; k < lanes; k++ )
        {
            acn_scene_handle* l = nullptr;
            if( lane_objects( device, debug, &l ) != ACN_OK ) break;
            h->early_made.push_back( l );
        }
    } );
}
static void early_lanes_join( acn_scene_handle* h ) { if( h->early_maker.joinable() ) h->early_maker.join(); }

extern "C" int acn_scene_upload( const acn_flat_scene* scene, int device, acn_scene_handle** out )
{
    if( !out ) return fail( ACN_ERR_ARG, "null out" );
    *out = nullptr;
    int max_csg = 0;
    std::string err;
    int st = acn_tables_validate( scene, &max_csg, &err );
    if( st != ACN_OK ) return fail( st, err );
    int ndev = acn_device_count();
    if( ndev <= 0 ) return fail( ACN_ERR_DEVICE, "no HIP device (libactinon_hip has no CPU fallback)" );
    if( device < 0 || device >= ndev ) return fail( ACN_ERR_ARG, "bad device index" );
    HIP_TRY( hipSetDevice( device ) );
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [ & ]() { return std::chrono::duration< double, std::milli >( std::chrono::steady_clock::now() - t_begin ).count(); };
    acn_scene_handle* h = new acn_scene_handle();
    h->device = device;
    h->tun.read();
    if( h->tun.early_lanes ) early_lanes_begin( h, ( size_t )scene->params.image_width * ( size_t )scene->params.image_height, scene->params.path_samples );
    double t_up[ 4 ] = { 0, 0, 0, 0 };   /* ACN_DEBUG_CHUNKS: stream + events, host-side tables, device copies, the camera kernel */
    {
        /* Workspace BOUND of the handle: ACN_WORKSPACE_MB, or 64 GiB / a quarter of the free device memory (288 GB per
         * MI355X).  It is a bound, not an allocation: the queues are sized from measured demand (ensure_workspace) and take
         * what ONE chunk per lane needs, if the bound allows -- every further chunk of a lane is another chain of ~45
         * dependent launches (1080p wine_glass, 4 lanes: 20 GB and 71 ms with one chunk per lane; bound 8 GiB: 9 chunks, 91 ms;
         * 4 GiB: 18 chunks, 125 ms).  Scenes whose demand per position is huge (path_samples 256 .. 1024: thousands of
         * second-level hits per pixel) use the whole bound: many_spheres p256 at 24 GiB 532 chunks, 39 s; at 64 GiB ... */
        size_t free_b = 0, total_b = 0;
        if( hipMemGetInfo( &free_b, &total_b ) != hipSuccess ) free_b = ( size_t )32 << 30;
        h->workspace_budget = h->tun.workspace_mb ? h->tun.workspace_mb * 1024 * 1024 : ( ( size_t )64 << 30 );
        if( !h->tun.workspace_mb && h->workspace_budget > free_b / 4 ) h->workspace_budget = free_b / 4;
    }
    {
        int cus = 0;
        if( hipDeviceGetAttribute( &cus, hipDeviceAttributeMultiprocessorCount, device ) != hipSuccess || cus <= 0 ) cus = 256;
        /* persistent grids.  A call that runs alone on its stream: 4 workgroups of 256 lanes per CU, what fits of the
         * 128-VGPR kernels.  The concurrent lanes of a call (create_lane): 2 per CU each -- what is resident of k_walk
         * (256 VGPRs); four lanes keep the chip full and leave room for each other's kernels (1080p: 83.4 ms against
         * 85.2 with 4 per CU; a lone lane with 2 per CU: 106 ms against 88) */
        h->cus = ( unsigned )cus;
        h->grid = h->tun.grid ? h->tun.grid : ( unsigned )cus * 4u;
        h->shade_grid = h->tun.shade_grid ? h->tun.shade_grid : ( unsigned )cus * 4u;
        h->walk_grid = h->tun.walk_grid ? h->tun.walk_grid : h->grid;
    }
    auto bail = [ & ]( int code ) { acn_scene_free( h ); return code; };
#define HIP_TRY_H( expr ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) \
    return bail( fail( ACN_ERR_DEVICE, std::string( #expr ) + ": " + hipGetErrorString( e_ ) ) ); } while( 0 )
    const double t_stream0 = since();
    HIP_TRY_H( hipStreamCreate( &h->stream ) );
    const double t_stream1 = since();   /* (the first stream a process makes: 85 - 100 ms on this runtime; later ones ~10) */
    /* (a stream costs ~10 ms of host time to make: the second one only where it is used) */
    HIP_TRY_H( hipEventCreate( &h->ev0 ) );
    HIP_TRY_H( hipEventCreate( &h->ev1 ) );
    t_up[ 0 ] = since();
    acn_scene_tables t;   /* everything the traversal shortcuts read, built on the host alone (acn_tables.cpp) */
    acn_tables_build( scene, h->tun.tables, &t );
    t_up[ 1 ] = since();
    acn_scene_handle::Resident& r = h->scene;
    r.max_csg_depth = max_csg;
    r.lds_bytes = t.lds_bytes; r.lds_stack_bytes = t.lds_stack_bytes;
    r.prune = t.prune; r.leaf_lights = t.leaf_lights; r.elem_pos_base = t.elem_pos_base;
    r.n_levels = t.n_levels; r.n_lights = t.n_lights;
    const size_t n_tex = scene->n_textures ? scene->n_textures : 1, n_sc = t.sc_table.size() ? t.sc_table.size() : 1, n_sph = t.sc_spheres.size() ? t.sc_spheres.size() : 4;
    r.scene_bytes[ 0 ] = sizeof( GNode ) * t.nodes.size(); r.scene_bytes[ 1 ] = sizeof( GMat ) * t.mats.size();
    r.scene_bytes[ 2 ] = sizeof( int32_t ) * t.elems.size(); r.scene_bytes[ 3 ] = sizeof( acn_texture ) * n_tex;
    HIP_TRY_H( hipMalloc( &r.d_nodes, r.scene_bytes[ 0 ] ) );
    HIP_TRY_H( hipMalloc( &r.d_mats, r.scene_bytes[ 1 ] ) );
    HIP_TRY_H( hipMalloc( &r.d_elems, r.scene_bytes[ 2 ] ) );
    HIP_TRY_H( hipMalloc( &h->d_sc_table, sizeof( SCEntry ) * n_sc ) );
    if( t.sc_table.size() ) HIP_TRY_H( hipMemcpy( h->d_sc_table, t.sc_table.data(), sizeof( SCEntry ) * t.sc_table.size(), hipMemcpyHostToDevice ) );
    HIP_TRY_H( hipMalloc( &h->d_sc_spheres, sizeof( double ) * n_sph ) );
    if( t.sc_spheres.size() ) HIP_TRY_H( hipMemcpy( h->d_sc_spheres, t.sc_spheres.data(), sizeof( double ) * t.sc_spheres.size(), hipMemcpyHostToDevice ) );
    HIP_TRY_H( hipMalloc( &r.d_textures, r.scene_bytes[ 3 ] ) );
    if( scene->n_textures ) HIP_TRY_H( hipMemcpy( r.d_textures, scene->textures, sizeof( acn_texture ) * scene->n_textures, hipMemcpyHostToDevice ) );
    HIP_TRY_H( hipMalloc( &h->d_counters, sizeof( unsigned long long ) * ACN_CNT_SLOTS ) );
    HIP_TRY_H( hipMemset( h->d_counters, 0, sizeof( unsigned long long ) * ACN_CNT_SLOTS ) );
    HIP_TRY_H( hipMalloc( &h->d_counters_keep, sizeof( unsigned long long ) * ACN_CNT_SLOTS ) );
    HIP_TRY_H( hipMalloc( &h->d_counts, sizeof( uint32_t ) * QC_N * ACN_LEVEL_BLOCKS ) );
    HIP_TRY_H( hipHostMalloc( &h->h_counts, sizeof( uint32_t ) * QC_N * ACN_LEVEL_BLOCKS ) );
    HIP_TRY_H( hipMemcpy( r.d_nodes, t.nodes.data(), r.scene_bytes[ 0 ], hipMemcpyHostToDevice ) );
    HIP_TRY_H( hipMemcpy( r.d_mats, t.mats.data(), r.scene_bytes[ 1 ], hipMemcpyHostToDevice ) );
    HIP_TRY_H( hipMemcpy( r.d_elems, t.elems.data(), r.scene_bytes[ 2 ], hipMemcpyHostToDevice ) );
    HIP_TRY_H( hipMemset( h->d_counts, 0, sizeof( uint32_t ) * QC_N * ACN_LEVEL_BLOCKS ) );
    h->dev.nodes = ( NodeP )r.d_nodes; h->dev.gnodes = ( NodeP )r.d_nodes;
    h->dev.mats = ( MatP )r.d_mats;
    h->dev.elems = ( ElemP )r.d_elems;
    h->dev.textures = ( TexP )r.d_textures;
    h->dev.sc_table = h->d_sc_table;
    h->dev.sc_spheres = h->d_sc_spheres;
    h->dev.prune_base = t.prune_base;
    h->dev.light_root = scene->light_root;
    h->dev.matter_root = scene->matter_root;
    h->dev.n_nodes = scene->n_nodes;
    h->dev.n_elems = scene->n_elems;
    h->dev.prm = scene->params;
    h->dev.flags = h->d_counts + QC_FLAGS;
    h->dev.lds_stack = r.lds_stack_bytes ? 0u : ACN_NO_LDS_STACK;   /* the kernels that own a stack area set the offset */
    /* Width of a shading task (size_class in acn_pipeline.h).  Narrow groups waste less of a sample loop's last round;
     * a whole wavefront per point keeps the rays of a round on one origin, which pays when a sample's traversal is long
     * and divergent (nested compounds, CSG objects with prune programs: the scenes of the "extras" kernel variants).
     * Measured, 4 lanes: wine_glass 1080p (200 / 64 samples) 79.8 ms narrow, 85.2 wide from 33 samples; many_spheres
     * 1080p p256 every 16th pixel 3.94 s narrow, 2.90 s wide; diamond 1080p p512 4.58 s narrow, 4.05 s wide. */
    h->dev.class0_min = h->tun.class0_min ? h->tun.class0_min : ( r.prune ? 32u : 255u );
    /* camera basis on the device so that it shares the device's arithmetic */
    {
        M3* d_rot = nullptr; double* d_uf = nullptr;
        HIP_TRY_H( hipMalloc( &d_rot, sizeof( M3 ) ) );
        HIP_TRY_H( hipMalloc( &d_uf, sizeof( double ) ) );
        t_up[ 2 ] = since();
        early_lanes_join( h );   /* before the first kernel: nothing of this handle runs while hardware queues are being made */
        t_up[ 3 ] = since();
        hipLaunchKernelGGL( k_camera_setup, dim3( 1 ), dim3( 1 ), 0, h->stream, h->dev, d_rot, d_uf );
        HIP_TRY_H( hipGetLastError() );
        HIP_TRY_H( hipStreamSynchronize( h->stream ) );
        HIP_TRY_H( hipMemcpy( &h->dev.camera_rotation, d_rot, sizeof( M3 ), hipMemcpyDeviceToHost ) );
        HIP_TRY_H( hipMemcpy( &h->dev.unit_f, d_uf, sizeof( double ), hipMemcpyDeviceToHost ) );
        hipFree( d_rot ); hipFree( d_uf );
    }
    if( h->tun.debug_chunks )
        fprintf( stderr, "[acn upload] %u nodes: the handle's stream %.2f ms, events %.2f, tables on the host %.2f, device copies %.2f, waited for %d early lanes %.2f, first kernel of the library (camera set-up) %.2f\n",
                 ( unsigned )scene->n_nodes, t_stream1 - t_stream0, t_up[ 0 ] - t_stream1 + t_stream0, t_up[ 1 ] - t_up[ 0 ], t_up[ 2 ] - t_up[ 1 ], ( int )h->early_made.size(), t_up[ 3 ] - t_up[ 2 ], since() - t_up[ 3 ] );
    *out = h;
    return ACN_OK;
}

static void free_workspace( acn_scene_handle* h )
{
    Workspace& w = h->ws;
    if( w.tasks ) hipFree( w.tasks );
    for( int k = 0; k < ACN_NCLASS; k++ ) if( w.idx[ k ] ) hipFree( w.idx[ k ] );
    if( w.children ) hipFree( w.children );
    if( w.hard_shadow ) hipFree( w.hard_shadow );
    if( w.hard_path ) hipFree( w.hard_path );
    for( int k = 0; k < 2; k++ ) if( w.rays[ k ] ) hipFree( w.rays[ k ] );
    if( w.stacks ) hipFree( w.stacks );
    w = Workspace();
}

extern "C" void acn_scene_free( acn_scene_handle* h )
{
    if( !h ) return;
    hipSetDevice( h->device );
    early_lanes_join( h );
    for( acn_scene_handle* l : h->early_made ) acn_scene_free( l );
    h->early_made.clear();
    for( acn_scene_handle* l : h->lanes ) acn_scene_free( l );
    h->lanes.clear();
    if( h->worker ) { h->worker->stop(); delete h->worker; h->worker = nullptr; }
    free_workspace( h );
    if( h->d_counts ) hipFree( h->d_counts );
    if( h->h_counts ) hipHostFree( h->h_counts );
    if( h->d_accum ) hipFree( h->d_accum );
    if( h->d_lane_in ) hipFree( h->d_lane_in );
    if( h->d_lane_out ) hipFree( h->d_lane_out );
    if( h->d_shard_pos ) hipFree( h->d_shard_pos );
    if( h->d_ray_check ) hipFree( h->d_ray_check );
    if( h->d_surface_flags ) hipFree( h->d_surface_flags );
    if( h->d_denoise ) hipFree( h->d_denoise );
    if( h->d_lens_rays ) hipFree( h->d_lens_rays );
    if( h->d_lens_rad ) hipFree( h->d_lens_rad );
    if( h->d_select_tiles ) hipFree( h->d_select_tiles );
    if( !h->is_lane )   /* a lane borrows the resident scene of its parent */
    {
        if( h->scene.d_nodes ) hipFree( h->scene.d_nodes );
        if( h->scene.d_mats ) hipFree( h->scene.d_mats );
        if( h->scene.d_elems ) hipFree( h->scene.d_elems );
        if( h->scene.d_textures ) hipFree( h->scene.d_textures );
        if( h->d_sc_table ) hipFree( h->d_sc_table );
        if( h->d_sc_spheres ) hipFree( h->d_sc_spheres );
    }
    if( h->d_counters ) hipFree( h->d_counters );
    if( h->d_counters_keep ) hipFree( h->d_counters_keep );
    for( auto& e : h->events ) { hipEventDestroy( e.a ); hipEventDestroy( e.b ); }
    if( h->ev0 ) hipEventDestroy( h->ev0 );
    if( h->ev1 ) hipEventDestroy( h->ev1 );
    if( h->stream ) hipStreamDestroy( h->stream );
    delete h;
}

/* Queue capacities.  Only one chunk of positions is in flight per pipeline run, so the queues are sized for a chunk, not
 * for the call, and each queue for its own demand:
 *   - rates unknown (first call on a handle): a small uniform starter set; the first chunk of the call is small, teaches
 *     the rates (render_chunk) and launch_render comes back here;
 *   - rates known: room for as many positions as the call has (at most ACN_CHUNK_TARGET) at 1 / 0.7 of the learned rates,
 *     scaled down to the handle's budget (ACN_WORKSPACE_MB; default 8 GiB or a quarter of the free device memory) if that is
 *     less.  The chunk size follows the capacities (launch_render), so a small workspace costs more chunks, not
 *     correctness; if hipMalloc refuses, the request is halved until it fits. */
#define ACN_CHUNK_TARGET ( ( size_t )1 << 22 )
#define ACN_STARTER_RECORDS ( ( size_t )1 << 20 )
static double f_max_host( double a, double b ) { return a > b ? a : b; }
static bool rates_known( const acn_scene_handle* h ) { return h->rate[ WQ_TASKS ] > 0 || h->rate[ WQ_RAYS ] > 0 || h->rate[ WQ_HARD_SHADOW ] > 0; }
/* records per position a queue of the current call needs: the learned rate, and in the ray queue of a ray call at least one
 * slot per position whatever earlier calls taught the handle -- its seeded generation is a KNOWN demand, kept out of the
 * learned rates (render_chunk) */
static double queue_demand( const double* rate, int q, bool seeded ) { return seeded && q == WQ_RAYS && rate[ q ] < 1.0 ? 1.0 : rate[ q ]; }
static double demand( const acn_scene_handle* h, int q ) { return queue_demand( h->rate, q, h->seeded ); }

/* positions a chunk may have so that every queue stays below 70 % of its capacity */
static size_t chunk_for_caps( const acn_scene_handle* h )
{
    double chunk = 2.0e9;
    for( int q = 0; q < WQ_N; q++ )
    {
        const double r = demand( h, q ) > 1e-3 ? demand( h, q ) : 1e-3;
        const double c = h->ctl.fill_target * ( double )h->ws.cap[ q ] / r;
        if( c < chunk ) chunk = c;
    }
    return chunk < 64 ? 64 : ( size_t )chunk;
}

static int ensure_workspace( acn_scene_handle* h, size_t n )
{
    Workspace& w = h->ws;
    const size_t budget = h->workspace_budget / h->budget_div;
    const size_t stack_waves = ( size_t )( h->walk_grid > h->grid ? h->walk_grid : h->grid ) * 4;
    const size_t stack_bytes = stack_waves * h->tun.stack_cap * sizeof( RayTask );
    size_t want[ WQ_N ];
    bool trim = false;
    if( !rates_known( h ) )
    {
        /* starter set: 2^20 records per queue (the deferred-shadow queue twice that), less for a call of a few positions */
        const size_t s = h->dev.prm.path_samples ? h->dev.prm.path_samples : 1;
        const size_t per_pos = ( s + 2 ) * ( s > 16 ? s / 16 : 1 ) + ( size_t )h->dev.prm.direct_samples * h->scene.n_lights;
        size_t recs = n * per_pos + 65536;
        if( recs > ACN_STARTER_RECORDS ) recs = ACN_STARTER_RECORDS;
        size_t per_rec = wq_bytes[ WQ_HARD_SHADOW ];
        for( int q = 0; q < WQ_N; q++ ) per_rec += wq_bytes[ q ];
        const size_t max_recs = budget > stack_bytes ? ( budget - stack_bytes ) / per_rec : 0;
        if( recs > max_recs ) recs = max_recs;
        for( int q = 0; q < WQ_N; q++ ) want[ q ] = recs;
        want[ WQ_HARD_SHADOW ] = 2 * recs;
    }
    else
    {
        double positions = ( double )( n < ACN_CHUNK_TARGET ? n : ACN_CHUNK_TARGET );
        double bytes = 0;
        /* 40 % above what the rates ask for: the rates move a little from frame to frame, and a queue that is a few per
         * cent short turns one chunk per lane into two (a second chain of launches: c2 36 -> 50 ms) or, worse, makes the
         * lane re-allocate in the middle of a frame (hipFree synchronises the device: paraffin_lamp 440 -> 700 ms) */
        const double slack = 1.4;
        for( int q = 0; q < WQ_N; q++ ) bytes += ( slack * demand( h, q ) * positions / 0.7 + 65536.0 ) * ( double )wq_bytes[ q ];
        const double room = budget > stack_bytes ? ( double )( budget - stack_bytes ) : 0.0;
        if( bytes > room ) positions *= room / bytes;
        for( int q = 0; q < WQ_N; q++ )
        {
            double c = slack * demand( h, q ) * positions / 0.7 + 65536.0;
            want[ q ] = c > 4.0e9 ? 0xFFFFFF00ull : ( size_t )c;
        }
    }
    for( int q = 0; q < WQ_N; q++ ) { if( want[ q ] < 65536 ) want[ q ] = 65536; if( want[ q ] > 0xFFFFFF00ull ) want[ q ] = 0xFFFFFF00ull; }
    /* keep what is there while it holds what the rates ask for (the slack is for growth, not a reason to re-allocate) */
    bool fits = w.stack_waves >= stack_waves;
    for( int q = 0; q < WQ_N; q++ ) if( ( double )w.cap[ q ] < ( double )want[ q ] / 1.4 ) fits = false;
    /* ... and give back what the first, small chunks of a handle over-estimated (their dead slots do not scale): once, when
     * the rates come from a large chunk and the queues hold 40 % more than those ask for (slack included) */
    /* ... in a WINDOW: the first few sizing steps after the rates were learned (the second and third call of a handle).  Rates
     * decay slowly towards what the chunks really leave, so without the window the condition could first become true ten frames
     * later and put 100 ms of hipFree + hipMalloc into an arbitrary frame (round 4, session 10: the 1080p bench line read 68.6 ms
     * instead of 51.8 because the trim fell into its ten timed steps) */
    if( rates_known( h ) && h->rate_cnt >= 32768 ) w.sized_calls++;
    if( fits && rates_known( h ) && h->rate_cnt >= 32768 && !w.trimmed && w.sized_calls <= 3 )
    {
        size_t have = 0, need = 0;
        for( int q = 0; q < WQ_N; q++ ) { have += ( size_t )w.cap[ q ] * wq_bytes[ q ]; need += want[ q ] * wq_bytes[ q ]; }
        if( ( double )have > 1.25 * ( double )need && have - need > ( ( size_t )1 << 29 ) ) { fits = false; trim = true; }
    }
    if( fits ) return ACN_OK;
    const uint64_t allocs_before = w.allocs;
    free_workspace( h );
    w.allocs = allocs_before + 1;
    for( ;; )
    {
        hipError_t e = hipSuccess;
        size_t total = 0;
        auto grab = [ & ]( void** p, size_t bytes ) { if( e == hipSuccess ) { e = hipMalloc( p, bytes ); total += bytes; } };
        grab( ( void** )&w.children, sizeof( HitRec ) * want[ WQ_CHILDREN ] );
        grab( ( void** )&w.tasks, sizeof( DTask ) * want[ WQ_TASKS ] );
        for( int k = 0; k < ACN_NCLASS; k++ ) grab( ( void** )&w.idx[ k ], sizeof( uint32_t ) * want[ WQ_TASKS ] );
        grab( ( void** )&w.hard_shadow, sizeof( HardShadow ) * want[ WQ_HARD_SHADOW ] );
        grab( ( void** )&w.hard_path, sizeof( HardPath ) * want[ WQ_HARD_PATH ] );
        for( int k = 0; k < 2; k++ ) grab( ( void** )&w.rays[ k ], sizeof( RayTask ) * want[ WQ_RAYS ] );
        grab( ( void** )&w.stacks, stack_bytes );
        if( e == hipSuccess ) { w.bytes = total; break; }
        ( void )hipGetLastError();
        free_workspace( h );
        w.allocs = allocs_before + 1;
        bool floor = true;
        for( int q = 0; q < WQ_N; q++ ) { if( want[ q ] > 65536 ) floor = false; want[ q ] = want[ q ] / 2 < 65536 ? 65536 : want[ q ] / 2; }
        if( floor ) return fail( ACN_ERR_DEVICE, std::string( "queue workspace: " ) + hipGetErrorString( e ) );
    }
    for( int q = 0; q < WQ_N; q++ ) w.cap[ q ] = ( uint32_t )want[ q ];
    w.stack_waves = stack_waves;
    w.trimmed = trim;
    return ACN_OK;
}

/* per-launch HIP events (stage times of acn_last_stage_ms) cost ~0.7 % of a frame and more of a small one: only
 * with ACN_OPT_STAGE_TIMING; launch counts and pipeline statistics are kept either way */
static int stage_begin( acn_scene_handle* h, int stage, hipStream_t stream )
{
    if( !h->stage_timing ) { h->cur_stage = stage; return ACN_OK; }
    if( h->events_used == h->events.size() )
    {
        StageEvents e{};
        HIP_TRY( hipEventCreate( &e.a ) );
        HIP_TRY( hipEventCreate( &e.b ) );
        h->events.push_back( e );
    }
    h->events[ h->events_used ].stage = stage;
    HIP_TRY( hipEventRecord( h->events[ h->events_used ].a, stream ) );
    return ACN_OK;
}

static int stage_end( acn_scene_handle* h, hipStream_t stream )
{
    if( !h->stage_timing ) { h->launches[ h->cur_stage ]++; return ACN_OK; }
    HIP_TRY( hipEventRecord( h->events[ h->events_used ].b, stream ) );
    h->launches[ h->events[ h->events_used ].stage ]++;
    h->events_used++;
    return ACN_OK;
}

static SceneArgs scene_args( const acn_scene_handle* h )
{
    SceneArgs s;
    s.dev = h->dev; s.nodes = h->scene.d_nodes; s.mats = h->scene.d_mats; s.elems = h->scene.d_elems; s.textures = h->scene.d_textures; s.elem_pos_base = h->scene.elem_pos_base;
    return s;
}
static KernelFlags kernel_flags( const acn_scene_handle* h )
{
    KernelFlags f;
    f.count = h->count_work; f.leaf_lights = h->scene.leaf_lights; f.lds_nodes = h->scene.lds_bytes != 0; f.prune = h->scene.prune;
    return f;
}
/* the workspace as the kernels of path level `level` see it */
static LevelQ level_queues( const acn_scene_handle* h, int level )
{
    const Workspace& w = h->ws;
    LevelQ q;
    q.tasks = w.tasks; for( int k = 0; k < ACN_NCLASS; k++ ) q.idx[ k ] = w.idx[ k ];
    q.task_cap = w.cap[ WQ_TASKS ]; q.child_cap = w.cap[ WQ_CHILDREN ]; q.hs_cap = w.cap[ WQ_HARD_SHADOW ]; q.hard_cap = w.cap[ WQ_HARD_PATH ];
    q.ray_cap = w.cap[ WQ_RAYS ];
    q.children = w.children; q.hard_shadow = w.hard_shadow; q.hard_path = w.hard_path;
    q.rays[ 0 ] = w.rays[ 0 ]; q.rays[ 1 ] = w.rays[ 1 ];
    q.stacks = w.stacks; q.stack_cap = h->tun.stack_cap; q.stack_use = h->tun.stack_use;
    q.counts = h->d_counts + ( size_t )level * QC_N;
    q.prev_children = h->d_counts + ( size_t )( level > 0 ? level - 1 : 0 ) * QC_N + QC_CHILDREN;
    q.grid = h->grid; q.shade_grid = h->shade_grid; q.walk_grid = h->walk_grid;
    q.fetch_walk = h->tun.fetch_walk; q.fetch_hard = h->tun.fetch_hard; q.private_limit = h->tun.private_limit; q.fetch_shade = h->tun.fetch_shade;
    /* the outermost sample loops are those of level 0 */
    const bool sharded = level == 0 && h->shard_world > 1;
    q.shard_rank = sharded ? h->shard_rank : 0u; q.shard_world = sharded ? h->shard_world : 1u;
    q.emit_terms = sharded && h->shard_rank != 0 ? 0u : 1u;
    return q;
}
static size_t machine_lds_bytes( const acn_scene_handle* h ) { return h->scene.lds_bytes + h->scene.lds_stack_bytes; }

/* launches of k_walk for path level `level`: ACN_WALK_PASSES, but no more than the hits of the level have depth left */
static uint32_t walk_passes_of_level( const acn_scene_handle* h, int level )
{
    const uint64_t depth_left = h->dev.prm.trace_depth > 10ull * ( uint64_t )level ? h->dev.prm.trace_depth - 10ull * ( uint64_t )level : 1;
    uint32_t passes = h->tun.walk_passes;
    if( passes > depth_left + 1 ) passes = ( uint32_t )depth_left + 1;
    /* The chunks of a call see the same mix of pixels (TileOrder), so the passes that had input in the last chunk, plus
     * one, are the passes this chunk needs: the last launch of a level finishes whatever is left on the private stacks in
     * any case, so a guess that is too low costs time, never rays.  (A frame without specular surfaces: 2 launches per
     * level instead of 12.) */
    const uint32_t seen = h->tun.learn_passes ? h->walk_passes_seen[ level ] : 0u;
    if( seen && seen + 1 < passes ) passes = seen + 1;
    return passes;
}

#define ACN_LAUNCH( h, stage, stream, call ) do { int st_ = stage_begin( h, stage, stream ); if( st_ != ACN_OK ) return st_; call; \
    HIP_TRY( hipGetLastError() ); if( ( st_ = stage_end( h, stream ) ) != ACN_OK ) return st_; } while( 0 )

/* What the primary rays of a call come from, handed down the whole chain (render_dispatch -> launch_render / render_lanes ->
 * learn_rates -> render_chunk -> acn_launch_walk): sample positions [ n ][ 2 ], the pixel centres of the main pass from pixel
 * `first` on (pos_xy == nullptr), or the caller's rays [ n ][ 6 ] -- seeded into the level-0 ray queue (k_rays.hip), where the
 * first walk pass reads them instead of making camera rays. */
struct Primary
{
    const double* pos_xy = nullptr;
    size_t first = 0;
    const double* rays = nullptr;
};
static Primary primary_positions( const double* pos_xy ) { Primary p; p.pos_xy = pos_xy; return p; }
static Primary primary_main_pass( size_t first ) { Primary p; p.first = first; return p; }
static Primary primary_rays( const double* rays ) { Primary p; p.rays = rays; return p; }

/* One chunk of positions [ base, base + cnt ).  The whole chain -- per path level: ( k_shade_hits -> ) the passes of
 * k_walk -> k_shade x 4 size classes -> k_hard_shadow -> k_hard_path -- is enqueued blind: every kernel takes
 * its input count from the counter block of its level on the device, and a level that turns out to be empty costs a few
 * launches of waves that exit at once.  The host synchronises ONCE, at the end, to read the counter blocks: overflow
 * flags (the chunk is then redone smaller) and statistics. */
static int render_chunk( acn_scene_handle* h, const Primary& prim, uint32_t base, uint32_t cnt, TileOrder order,
                         hipStream_t stream, int* overflow, uint32_t* fill, double* dead_share )
{
    *overflow = 0;
    *dead_share = 0;
    for( int q = 0; q < WQ_N; q++ ) fill[ q ] = 0;
    const int levels = h->scene.n_levels;
    const KernelFlags f = kernel_flags( h );
    const SceneArgs s = scene_args( h );
    const size_t lds = machine_lds_bytes( h );
    HIP_TRY( hipMemsetAsync( h->d_counts, 0, sizeof( uint32_t ) * QC_N * levels, stream ) );
    if( prim.rays )
    {
        /* the caller's rays are generation 0 of level 0, one slot each (launch_render keeps a chunk within the ray queue) */
        if( cnt > h->ws.cap[ WQ_RAYS ] ) return fail( ACN_ERR_DEVICE, "a chunk of rays larger than the ray queue" );
        /* (a walk launch of the statistics: it does what k_walk's first pass does for positions, make the primary rays) */
        ACN_LAUNCH( h, 0, stream, acn_launch_seed_rays( prim.rays, base, cnt, order, ( int )h->dev.prm.trace_depth, level_queues( h, 0 ), stream ) );
    }
    const uint32_t n_cam = prim.rays ? 0u : cnt;
    for( int level = 0; level < levels; level++ )
    {
        LevelQ q = level_queues( h, level );
        /* the path-sample hits of the level before are shaded (level >= 1), then the specular rays walked: generation
         * passes while the generations are large, the rest on the waves' private stacks (k_walk); a level has at most as
         * many generations as its hits have depth left */
        /* a small chunk (<= 2^17 positions) of a frame without path tracing finishes every generation that is no larger than
         * itself on the private stacks: its generations are not worth a launch each (C1, 120 000 pixels on one lane: 1.41 ->
         * 1.15 ms).  With path samples the rule was measured and dropped: the 1/8 share of the 1080p frame 15.2 -> 14.8 ms and
         * hanging_lamp 600x800 -3 %, but paraffin_lamp 400x600 +8 % -- the rays of a CSG scene are worth redistributing
         * (profiles/r03/private_limit_small_frames.txt) */
        if( !h->tun.private_limit_set && h->dev.prm.path_samples == 0 && cnt <= ( 1u << 17 ) && cnt > q.private_limit ) q.private_limit = cnt;
        if( level > 0 ) ACN_LAUNCH( h, 0, stream, acn_launch_shade_hits( f.count, q, stream, s, h->d_accum, h->d_counters ) );
        const uint32_t passes = walk_passes_of_level( h, level );
        for( uint32_t pass = 0; pass < passes; pass++ )
        {
            /* (the last launch of a level finishes whatever is left on the private stacks: the input of all later generations) */
            ACN_LAUNCH( h, 0, stream, acn_launch_walk( f, pass, pass + 1 == passes, q, lds, stream, s, prim.pos_xy, prim.first, base,
                                                       level == 0 && pass == 0 ? n_cam : 0u, order, h->d_accum, h->d_counters ) );
        }
        ACN_LAUNCH( h, 1, stream, acn_launch_shade64( f, q, stream, s, h->d_accum, h->d_counters ) );
        ACN_LAUNCH( h, 1, stream, acn_launch_shade16( f, q, stream, s, h->d_accum, h->d_counters ) );
        ACN_LAUNCH( h, 1, stream, acn_launch_shade4( f, q, stream, s, h->d_accum, h->d_counters ) );
        ACN_LAUNCH( h, 1, stream, acn_launch_shade1( f, q, stream, s, h->d_accum, h->d_counters ) );
        ACN_LAUNCH( h, 3, stream, acn_launch_hard_shadow( f, q, lds, stream, s, h->d_accum, h->d_counters ) );
        /* the last level casts no path rays (depth <= 10) */
        if( level + 1 < levels ) ACN_LAUNCH( h, 3, stream, acn_launch_hard_path( f, q, lds, stream, s, h->d_accum, h->d_counters ) );
    }
    HIP_TRY( hipMemcpyAsync( h->h_counts, h->d_counts, sizeof( uint32_t ) * QC_N * levels, hipMemcpyDeviceToHost, stream ) );
    HIP_TRY( hipStreamSynchronize( stream ) );
    h->host_syncs++;
    /* the seeded generation of a ray call is a known demand (demand), not a learned one: with its word cleared the queue marks,
     * the learned passes and learn_rates see the counts of a position call, where level 0 has no generation 0 */
    if( prim.rays ) h->h_counts[ QC_GEN + 0 ] = 0;
    uint32_t flags = 0;
    for( int level = 0; level < levels; level++ )
    {
        const uint32_t* c = h->h_counts + ( size_t )level * QC_N;
        flags |= c[ QC_FLAGS ];
        if( c[ QC_GEN + walk_passes_of_level( h, level ) ] ) flags |= ACN_FLAG_CHILD_OVERFLOW;   /* rays left over by the last pass */
    }
    h->flags_seen |= flags & ACN_FLAG_CLAMPED;
    /* what the chunk put into each queue (high-water marks of reserved slots, dead slots included; of a chunk that
     * overflowed: at least this much): the next chunk's size and the queue capacities are derived from it */
    for( int level = 0; level < levels; level++ )
    {
        const uint32_t* c = h->h_counts + ( size_t )level * QC_N;
        auto up = [ & ]( int q, uint32_t v ) { if( v > fill[ q ] ) fill[ q ] = v; };
        up( WQ_TASKS, c[ QC_TASKS ] );
        for( int k = 0; k < ACN_NCLASS; k++ ) up( WQ_TASKS, c[ QC_CLASS0 + k ] );
        up( WQ_CHILDREN, c[ QC_CHILDREN ] );
        up( WQ_HARD_SHADOW, c[ QC_HARD_SHADOW ] );
        up( WQ_HARD_PATH, c[ QC_HARD_PATH ] );
        for( int g = 0; g <= ACN_MAX_WALK_PASSES; g++ ) up( WQ_RAYS, c[ QC_GEN + g ] );
    }
    {
        /* how much of the marks are dead slots (the ends of the waves' reservations): known exactly for the deferred-shadow
         * queue, whose records are counted; the share does not scale with the chunk, so a small chunk's marks over-state
         * the demand per position by 1 / ( 1 - share ) */
        uint32_t mark = 0, recs = 0;
        for( int level = 0; level < levels; level++ )
        {
            const uint32_t* c = h->h_counts + ( size_t )level * QC_N;
            if( c[ QC_HARD_SHADOW ] > mark ) { mark = c[ QC_HARD_SHADOW ]; recs = c[ QS_HARD_SHADOW ] + c[ QS_PROBES ]; }
        }
        if( mark > 0 && recs < mark ) *dead_share = ( double )( mark - recs ) / ( double )mark;
    }
    /* a lost chunk first: it is redone smaller, and a stack overflow that is real shows again in the retry */
    if( flags & ( ACN_FLAG_TASK_OVERFLOW | ACN_FLAG_CHILD_OVERFLOW ) ) { *overflow = 1; return ACN_OK; }
    if( flags & ACN_FLAG_STACK_OVERFLOW ) return fail( ACN_ERR_UNSUPPORTED, "device CSG / compound stack overflow (or a walk that did not end)" );
    for( int level = 0; level < levels; level++ )
    {
        const uint32_t* c = h->h_counts + ( size_t )level * QC_N;
        if( c[ QC_TASKS ] == 0 && c[ QS_WALK_RAYS ] == 0 ) break;
        h->levels++;
        h->walk_rays += c[ QS_WALK_RAYS ];
        h->walk_steps += c[ QS_WALK_STEPS ];
        h->hard_rays += ( uint64_t )c[ QS_HARD_SHADOW ] + c[ QS_HARD_PATH ];
        h->shade_hit_recs += c[ QS_CHILDREN ];
        if( c[ QC_TASKS ] > h->peak_tasks ) h->peak_tasks = c[ QC_TASKS ];
        if( c[ QC_CHILDREN ] > h->peak_children ) h->peak_children = c[ QC_CHILDREN ];
        h->private_rays += c[ QS_PRIVATE_RAYS ];
        h->probe_rays += c[ QS_PROBES ];
    }
    if( cnt >= 4096 )   /* a chunk large enough to stand for the next one */
    {
        uint32_t seen[ ACN_MAX_PATH_LEVELS + 1 ];
        for( int level = 0; level < levels; level++ )
        {
            const uint32_t* c = h->h_counts + ( size_t )level * QC_N;
            const uint32_t launched = walk_passes_of_level( h, level );
            uint32_t used = 1;   /* pass 0 of level 0 has the camera rays; a level without rays keeps one launch */
            for( uint32_t g = 0; g < launched; g++ ) if( c[ QC_GEN + g ] ) used = g + 1;
            /* the last launch ran in private mode: if it still had input the level may need more passes than were launched */
            seen[ level ] = ( used == launched && launched > 1 ) ? used + 2 : used;
        }
        for( int level = 0; level < levels; level++ ) h->walk_passes_seen[ level ] = seen[ level ];
    }
    return ACN_OK;
}

/* the rates of a handle from the queue marks of one chunk of cnt positions */
static void set_rates( acn_scene_handle* h, uint32_t cnt, const uint32_t* fill, double dead_share )
{
    /* (a chunk of a few positions: mostly dead slots, 64 positions of hanging_lamp p1024 mark 15 600 deferred rays per position
     * where 3 500 is the rate -- the counted share of the deferred-shadow queue corrects all five) */
    const double live = cnt <= 4096 && dead_share > 0 && dead_share < 0.95 ? 1.0 - dead_share : 1.0;
    for( int q = 0; q < WQ_N; q++ ) h->rate[ q ] = f_max_host( live * ( double )fill[ q ] / ( double )cnt, 1e-3 );
    h->rate_cnt = cnt;
}

/* Cold handle: the queue demand per position is learned from a SAMPLE of the call's own positions -- every ( n / m )-th of them,
 * m = 512 .. 4096 -- rendered once on the starter queues and thrown away, before anything is sized.  Round 3 let the first
 * chunks of the call learn: the first tile of the order is a corner of the picture (C4: 1 shading task and 161 deferred path rays
 * per position where the frame's average is 300 / 1 800), so the queues were found one by one by halving -- 12 redone chunks on
 * the C3 / C4 frames, a first frame of 718 ms on paraffin_lamp where the second takes 465 -- and every lane of a call learned
 * for itself and re-sized its queues in the middle of the frame.  A sample over the whole frame costs one short chain of
 * launches (a few ms; nothing next to a frame whose queues must be allocated anyway) and is trusted like a large chunk: the
 * queues are then sized ONCE, while the device is idle (launch_render; render_lanes for all lanes of a call). */
static int learn_rates( acn_scene_handle* h, const Primary& prim, size_t n, hipStream_t stream, size_t plan_positions, unsigned plan_grid )
{
    if( rates_known( h ) || !h->tun.learn_sample || h->tun.chunk || n < 16384 ) return ACN_OK;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [ & ]() { return std::chrono::duration< double, std::milli >( std::chrono::steady_clock::now() - t_begin ).count(); };
    int st = ensure_workspace( h, 4096 );   /* the starter set */
    if( st != ACN_OK ) return st;
    if( h->accum_cap < n )
    {
        if( h->d_accum ) hipFree( h->d_accum );
        h->d_accum = nullptr; h->accum_cap = 0;
        HIP_TRY( hipMalloc( &h->d_accum, sizeof( unsigned long long ) * 3 * n ) );
        h->accum_cap = n;
    }
    if( h->tun.debug_chunks ) fprintf( stderr, "[acn sample] starter queues (%.2f GB) after %.2f ms\n", ( double )h->ws.bytes / 1e9, since() );
    /* as many positions as the starter queues hold by the guess launch_render makes for a first chunk, 4096 at most */
    const size_t s = h->dev.prm.path_samples ? h->dev.prm.path_samples : 1;
    size_t want = ( size_t )( ( double )h->ws.cap[ WQ_CHILDREN ] / ( ( double )( s + 2 ) * ( s > 64 ? ( double )s / 64.0 : 1.0 ) ) );
    const size_t by_shadow = ( size_t )( ( double )h->ws.cap[ WQ_HARD_SHADOW ] / ( 0.25 * ( double )( h->dev.prm.direct_samples * h->scene.n_lights + s ) + 4.0 ) );
    if( want > by_shadow ) want = by_shadow;
    if( want > 4096 ) want = 4096;
    /* (the guess is ten times what the lamp scenes need at path_samples 1024, where it allowed 63 positions: no sample at all, and
     * the whole hanging_lamp frame at stated size began every band with ~20 redone chunks, halving down from 92 000 positions to 9.
     * A sample that does not fit is halved below.) */
    if( want < 256 ) want = 256;
    if( want > n / 4 ) want = n / 4;
    const bool count_work = h->count_work, stage_timing = h->stage_timing;
    h->count_work = false; h->stage_timing = false; h->shard_rank = 0; h->shard_world = 1;
    h->events_used = 0;
    for( ; want >= 64; want /= 2 )
    {
        TileOrder order;
        order.n = ( uint32_t )n; order.n_tiles = 1; order.mul = 1;
        order.sample_stride = ( uint32_t )( n / want );
        const uint32_t cnt = ( uint32_t )want;
        hipLaunchKernelGGL( k_clear_slots, dim3( ( cnt + 255 ) / 256 ), dim3( 256 ), 0, stream, h->d_accum, 0u, cnt, order );
        HIP_TRY( hipGetLastError() );
        int overflow = 0;
        uint32_t fill[ WQ_N ];
        double dead_share = 0;
        st = render_chunk( h, prim, 0u, cnt, order, stream, &overflow, fill, &dead_share );
        if( st != ACN_OK ) break;
        if( h->tun.debug_chunks )
            fprintf( stderr, "[acn sample] chain done after %.2f ms\n", since() );
        if( h->tun.debug_chunks )
            fprintf( stderr, "[acn sample] %u positions (every %u-th) %s dead %.2f | per pos T %.1f C %.1f HS %.1f HP %.1f R %.1f\n", cnt, order.sample_stride, overflow ? "OVERFLOW" : "ok",
                     dead_share, fill[ 0 ] / ( double )cnt, fill[ 1 ] / ( double )cnt, fill[ 2 ] / ( double )cnt, fill[ 3 ] / ( double )cnt, fill[ 4 ] / ( double )cnt );
        if( overflow ) continue;
        /* the records the sample left in each queue, exactly (marks minus dead slots; the fullest level counts, the queues are
         * the levels' in turn), plus a quarter for what a sample of a few thousand positions does not see */
        double live[ WQ_N ] = { 0, 0, 0, 0, 0 };
        for( int level = 0; level < h->scene.n_levels; level++ )
        {
            const uint32_t* c = h->h_counts + ( size_t )level * QC_N;
            auto up = [ & ]( int q, double v ) { if( v > live[ q ] ) live[ q ] = v; };
            up( WQ_TASKS, ( double )c[ QC_TASKS ] - ( double )c[ QS_DEAD_T ] );
            up( WQ_CHILDREN, ( double )c[ QC_CHILDREN ] - ( double )c[ QS_DEAD_C ] );
            up( WQ_HARD_SHADOW, ( double )c[ QS_HARD_SHADOW ] + ( double )c[ QS_PROBES ] );
            up( WQ_HARD_PATH, ( double )c[ QC_HARD_PATH ] - ( double )c[ QS_DEAD_HP ] );
            /* rays: no generation holds more than the largest mark, nor more than all the level's generations together */
            double sum = 0, top = 0;
            for( int g = 0; g <= ACN_MAX_WALK_PASSES; g++ ) { sum += c[ QC_GEN + g ]; if( c[ QC_GEN + g ] > top ) top = c[ QC_GEN + g ]; }
            sum -= ( double )c[ QS_DEAD_R ];
            up( WQ_RAYS, sum < top ? sum : top );
        }
        /* What a queue must hold is records PLUS the slots that die at the ends of the waves' reservations: up to 64 per wave,
         * queue and launch that appends to it, whatever the chunk's size (a chunk of 230 000 positions of the wine glass marks 1.1 M
         * task slots for 0.45 M tasks).  The planner's rates are marks per position, so the dead slots of a chunk of the size the
         * call will run -- plan_positions, on persistent grids of plan_grid workgroups -- are spread over its positions:
         * tasks, specular rays and probes are appended by k_shade_hits and ~4 walk passes, path-sample hits and the two deferred
         * queues by the four k_shade launches (and k_hard_path). */
        {
            const double per_launch = ( double )ACN_QCHUNK * 4.0 * ( double )plan_grid;
            const double walkers = 3.0 * per_launch, shaders = 3.0 * per_launch;   /* (not every wave of every launch leaves a full reservation behind) */
            const double dead[ WQ_N ] = { walkers, shaders, walkers + shaders, shaders, walkers };
            const double pp = ( double )( plan_positions < ACN_CHUNK_TARGET ? plan_positions : ACN_CHUNK_TARGET );
            /* a generation of specular rays is at most three children per shaded hit (path-sample hits of the level before, or the
             * camera rays' shading points): the sample's ray marks are mostly dead slots */
            const double ray_bound = 2.0 * live[ WQ_CHILDREN ] + live[ WQ_TASKS ];
            if( live[ WQ_RAYS ] > ray_bound && ray_bound > 0 ) live[ WQ_RAYS ] = ray_bound;
            for( int q = 0; q < WQ_N; q++ ) h->rate[ q ] = f_max_host( 1.2 * live[ q ] / ( double )cnt + dead[ q ] / pp, 1e-3 );
        }
        if( h->tun.debug_chunks ) fprintf( stderr, "[acn sample] rates T %.1f C %.1f HS %.1f HP %.1f R %.1f\n", h->rate[ 0 ], h->rate[ 1 ], h->rate[ 2 ], h->rate[ 3 ], h->rate[ 4 ] );
        h->rate_cnt = 8192;   /* a sample of the whole frame: trusted like a chunk that size (launch_render re-sizes for the whole rest at once) */
        break;
    }
    for( int level = 0; level <= ACN_MAX_PATH_LEVELS; level++ ) h->walk_passes_seen[ level ] = 0;
    h->count_work = count_work; h->stage_timing = stage_timing;
    return st;
}

static int launch_render( acn_scene_handle* h, const Primary& prim, size_t n, double* d_out_rgb,
                          const acn_render_opts* opts, hipStream_t stream )
{
    if( opts && opts->cancel && *opts->cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many positions in one call" );
    h->seeded = prim.rays != nullptr;
    int linear = ( opts && ( opts->flags & ACN_OPT_LINEAR_OUT ) ) ? 1 : 0;
    h->count_work = ( opts && ( opts->flags & ACN_OPT_COUNT_WORK ) ) || h->tun.count_work;
    h->shard_rank = 0; h->shard_world = 1;
    if( opts && opts->shard_mode == ACN_SHARD_SAMPLES && opts->shard_world > 1 )
    {
        if( opts->shard_rank >= opts->shard_world ) return fail( ACN_ERR_ARG, "shard_rank >= shard_world" );
        h->shard_rank = opts->shard_rank; h->shard_world = opts->shard_world;
    }
    else if( opts && opts->shard_mode > ACN_SHARD_SAMPLES ) return fail( ACN_ERR_ARG, "unknown shard_mode" );
    h->stage_timing = ( opts && ( opts->flags & ACN_OPT_STAGE_TIMING ) ) || h->tun.stage_timing;
    int st = learn_rates( h, prim, n, stream, n, h->walk_grid > h->grid ? h->walk_grid : h->grid );
    if( st != ACN_OK ) return st;
    /* (shard fields again: the learning pass renders unsharded) */
    if( opts && opts->shard_mode == ACN_SHARD_SAMPLES && opts->shard_world > 1 ) { h->shard_rank = opts->shard_rank; h->shard_world = opts->shard_world; }
    st = ensure_workspace( h, n );
    if( st != ACN_OK ) return st;
    if( h->accum_cap < n )
    {
        if( h->d_accum ) hipFree( h->d_accum );
        h->d_accum = nullptr; h->accum_cap = 0;
        HIP_TRY( hipMalloc( &h->d_accum, sizeof( unsigned long long ) * 3 * n ) );
        h->accum_cap = n;
    }
    h->events_used = 0;
    h->launches[ 0 ] = h->launches[ 1 ] = h->launches[ 2 ] = h->launches[ 3 ] = 0;
    h->hard_rays = 0; h->walk_steps = 0; h->walk_rays = 0; h->shade_hit_recs = 0; h->host_syncs = 0; h->flags_seen = 0; h->private_rays = 0; h->probe_rays = 0;
    h->chunks = h->retries = h->levels = 0;
    h->ctl.retry_bound = 0;   /* (a call that ended in the middle of a retry) */
    h->peak_tasks = h->peak_children = 0;
    HIP_TRY( hipMemsetAsync( h->d_counters, 0, sizeof( unsigned long long ) * ACN_CNT_SLOTS, stream ) );
    HIP_TRY( hipEventRecord( h->ev0, stream ) );
    HIP_TRY( hipMemsetAsync( h->d_accum, 0, sizeof( unsigned long long ) * 3 * n, stream ) );

    /* Positions per pipeline run.  How many records a position leaves in each queue differs by orders of magnitude between
     * scenes (wine_glass: 15 deferred shadow rays per pixel; a closed room at path_samples 1024: 260 000 second-level hits),
     * so the rates are learned: a cautious first chunk on a small starter workspace, then chunks that fill the fullest
     * queue to 70 %, and the queues themselves re-sized once the rates are known (ensure_workspace); an overflow halves
     * the chunk.  Rates and workspace stay with the handle for its next call. */
    size_t s = h->dev.prm.path_samples ? h->dev.prm.path_samples : 1;
    size_t chunk;
    if( rates_known( h ) ) chunk = chunk_for_caps( h );
    else
    {
        /* the starter queues are small: a first chunk of at most 32 768 positions, fewer by a guess that errs on the safe
         * side by factors, not orders of magnitude (an overflow costs one small chunk): path-sample hits ~ path_samples per
         * position, squared from 64 samples on (two nested levels); a quarter of the direct-light samples deferred */
        chunk = ( size_t )( ( double )h->ws.cap[ WQ_CHILDREN ] / ( ( double )( s + 2 ) * ( s > 64 ? ( double )s / 64.0 : 1.0 ) ) );
        const size_t by_shadow = ( size_t )( ( double )h->ws.cap[ WQ_HARD_SHADOW ] / ( 0.25 * ( double )( h->dev.prm.direct_samples * h->scene.n_lights + s ) + 4.0 ) );
        if( chunk > by_shadow ) chunk = by_shadow;
        if( chunk > 32768 ) chunk = 32768;
    }
    if( h->tun.chunk ) chunk = h->tun.chunk;
    if( chunk < 64 ) chunk = 64;
    /* the order of work: tiles of 256 positions in a multiplicative stride over the call (TileOrder) */
    TileOrder order;
    order.n = ( uint32_t )n;
    order.n_tiles = ( uint32_t )( ( n + ( ( 1u << ACN_ORDER_SHIFT ) - 1 ) ) >> ACN_ORDER_SHIFT );
    order.mul = 1;
    order.sample_stride = 0;
    if( order.n_tiles > 2 )
    {
        auto gcd = []( uint64_t a, uint64_t b ) { while( b ) { uint64_t t = a % b; a = b; b = t; } return a; };
        uint64_t m = ( uint64_t )( 0.6180339887 * order.n_tiles ) | 1u;
        while( gcd( m, order.n_tiles ) != 1 ) m += 2;
        order.mul = ( uint32_t )( m % order.n_tiles );
    }
    const size_t n_slots = ( size_t )order.n_tiles << ACN_ORDER_SHIFT;
    size_t base = 0;
    while( base < n_slots )
    {
        if( opts && opts->cancel && *opts->cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
        /* the planned chunk; a rest that is predicted to fill no queue beyond 85 % is taken whole (a second chunk would be
         * another whole chain of launches for a few positions); a retry is at most half of the chunk that overflowed
         * (acn_chunkplan.h) */
        double plan[ WQ_N ];
        for( int q = 0; q < WQ_N; q++ ) plan[ q ] = demand( h, q );
        uint32_t cnt = acn_ctl_next( &h->ctl, n_slots - base, chunk, h->tun.chunk != 0, rates_known( h ), plan, h->ws.cap );
        /* (the seeded generation of a ray call takes one ray-queue slot per position, also under ACN_CHUNK) */
        if( prim.rays && cnt > h->ws.cap[ WQ_RAYS ] ) cnt = h->ws.cap[ WQ_RAYS ];
        int overflow = 0;
        uint32_t fill[ WQ_N ];
        double dead_share = 0;
        /* the work counters of a chunk that has to be redone must not count twice */
        if( h->count_work ) HIP_TRY( hipMemcpyAsync( h->d_counters_keep, h->d_counters, sizeof( unsigned long long ) * ACN_CNT_SLOTS, hipMemcpyDeviceToDevice, stream ) );
        st = render_chunk( h, prim, ( uint32_t )base, cnt, order, stream, &overflow, fill, &dead_share );
        if( st != ACN_OK ) return st;
        if( h->tun.debug_chunks )
            fprintf( stderr, "[acn chunk] base %zu cnt %u %s target %.2f dead %.2f | fill T %u C %u HS %u HP %u R %u | per pos T %.1f C %.1f HS %.1f HP %.1f R %.1f | rate T %.1f C %.1f HS %.1f HP %.1f R %.1f | cap T %u C %u HS %u HP %u R %u\n",
                     base, cnt, overflow ? "OVERFLOW" : "ok", h->ctl.fill_target, dead_share, fill[ 0 ], fill[ 1 ], fill[ 2 ], fill[ 3 ], fill[ 4 ],
                     fill[ 0 ] / ( double )cnt, fill[ 1 ] / ( double )cnt, fill[ 2 ] / ( double )cnt, fill[ 3 ] / ( double )cnt, fill[ 4 ] / ( double )cnt,
                     h->rate[ 0 ], h->rate[ 1 ], h->rate[ 2 ], h->rate[ 3 ], h->rate[ 4 ], h->ws.cap[ 0 ], h->ws.cap[ 1 ], h->ws.cap[ 2 ], h->ws.cap[ 3 ], h->ws.cap[ 4 ] );
        if( overflow )
        {
            if( cnt <= 1 ) return fail( ACN_ERR_DEVICE, "work queues overflow for a single position: raise ACN_WORKSPACE_MB" );
            if( h->count_work ) HIP_TRY( hipMemcpyAsync( h->d_counters, h->d_counters_keep, sizeof( unsigned long long ) * ACN_CNT_SLOTS, hipMemcpyDeviceToDevice, stream ) );
            h->retries++;
            /* scenes whose demand per position varies much between chunks (many_spheres p256: 49 of 220 chunks were redone at
             * a fixed 70 %) plan with more head room */
            chunk = acn_ctl_overflow( &h->ctl, cnt );
            /* the marks of an overflowed chunk are lower bounds of its demand */
            for( int q = 0; q < WQ_N; q++ ) { const double r = ( double )fill[ q ] / ( double )cnt; if( r > h->rate[ q ] ) h->rate[ q ] = r; }
            for( int level = 0; level <= ACN_MAX_PATH_LEVELS; level++ ) h->walk_passes_seen[ level ] = 0;   /* the full number of passes again */
            hipLaunchKernelGGL( k_clear_slots, dim3( ( cnt + 255 ) / 256 ), dim3( 256 ), 0, stream, h->d_accum, ( uint32_t )base, cnt, order );
            HIP_TRY( hipGetLastError() );
            continue;
        }
        h->chunks++;
        base += cnt;
        acn_ctl_fit( &h->ctl );
        if( h->tun.chunk ) continue;
        /* Learn.  A chunk much larger than the one the rates came from replaces them (the dead slots at the ends of the
         * waves' queue reservations do not scale with the chunk, so small chunks over-estimate); otherwise the rates
         * follow upwards at once and forget slowly. */
        const bool known = rates_known( h );
        if( !known || cnt >= 4 * h->rate_cnt ) set_rates( h, cnt, fill, dead_share );
        else
        {
            /* (also after small chunks: where chunks are small the demand per position is large and the dead slots do not
             * matter; rates that only went up left many_spheres p256 with 532 chunks of 3 900 positions after one spike) */
            for( int q = 0; q < WQ_N; q++ ) h->rate[ q ] = f_max_host( f_max_host( ( double )fill[ q ] / ( double )cnt, 0.85 * h->rate[ q ] ), 1e-3 );
            if( cnt > h->rate_cnt ) h->rate_cnt = cnt;
        }
        const size_t remaining = n_slots - base;
        if( remaining && ( double )chunk_for_caps( h ) * ( 0.85 / h->ctl.fill_target ) < ( double )remaining )
        {
            /* more than one further chunk with these queues: re-size them (a no-op when they already are what the budget
             * allows).  Rates that come from a small chunk are trusted for a medium one only. */
            const size_t target = h->rate_cnt < 8192 ? ( remaining < 65536 ? remaining : ( size_t )65536 ) : remaining;
            if( ( st = ensure_workspace( h, target ) ) != ACN_OK ) return st;
        }
        chunk = chunk_for_caps( h );
    }
    if( ( st = stage_begin( h, 2, stream ) ) != ACN_OK ) return st;
    hipLaunchKernelGGL( k_finalize, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        ( const unsigned long long* )h->d_accum, ( uint32_t )n, h->dev.prm.gamma, linear, d_out_rgb );
    HIP_TRY( hipGetLastError() );
    if( ( st = stage_end( h, stream ) ) != ACN_OK ) return st;
    HIP_TRY( hipEventRecord( h->ev1, stream ) );
    h->timed = true;
    return ACN_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* Concurrent lanes.  One pipeline run is a chain of ~60 dependent launches (a walk pass per specular generation,
 * shade, hard rays, per level), each ending in a tail where a few long rays keep the chip waiting, and each followed by
 * a host round trip for the queue counts.  Pixels are independent, so a call is cut into ACN_LANE_TILE-pixel tiles
 * dealt round-robin to K lanes; every lane is a clone of the handle (same resident scene, own stream, own workspace)
 * driven by its own host thread, and the lanes' kernels fill each other's tails and bubbles.  Measured on the 1080p
 * frame: 118 -> 87 ms with 4 lanes; on the share one of 8 GPUs gets: 21.0 -> 16.5 ms.  Results are unchanged: every
 * pixel is computed by exactly the same kernels from exactly the same inputs. */
#define ACN_LANE_TILE 256

/* positions of lane `lane` of `lanes`: tiles lane, lane + lanes, ... of the n positions of the call */
static size_t lane_count( size_t n, int lanes, int lane )
{
    size_t tiles = ( n + ACN_LANE_TILE - 1 ) / ACN_LANE_TILE, cnt = 0;
    if( tiles == 0 ) return 0;
    size_t full = tiles / lanes, rest = tiles % lanes;
    size_t my_tiles = full + ( ( size_t )lane < rest ? 1 : 0 );
    cnt = my_tiles * ACN_LANE_TILE;
    size_t last_tile = tiles - 1;
    if( last_tile % lanes == ( size_t )lane ) cnt -= tiles * ACN_LANE_TILE - n;   /* the last tile may be short */
    return cnt;
}

__device__ __forceinline__ size_t lane_global_index( size_t i, int lanes, int lane )
{
    return ( ( i / ACN_LANE_TILE ) * lanes + lane ) * ACN_LANE_TILE + ( i % ACN_LANE_TILE );
}

/* lane_pos[ i ] = position of the lane's i-th pixel (taken from pos_xy, or generated like acn_render_main_pass_dev) */
__global__ void k_lane_gather( const double* __restrict__ pos_xy, size_t first_pixel, uint64_t image_width, size_t n_lane,
                               int lanes, int lane, double* __restrict__ lane_pos )
{
    size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n_lane ) return;
    size_t g = lane_global_index( i, lanes, lane );
    double mx, my;
    if( pos_xy ) { mx = pos_xy[ g * 2 ]; my = pos_xy[ g * 2 + 1 ]; }
    else
    {
        size_t pix = first_pixel + g;
        mx = ( double )( pix % image_width ) + 0.5;
        my = ( double )( pix / image_width ) + 0.5;
    }
    lane_pos[ i * 2 ] = mx; lane_pos[ i * 2 + 1 ] = my;
}

__global__ void k_lane_scatter( const double* __restrict__ lane_out, size_t n_lane, int lanes, int lane, double* __restrict__ out_rgb )
{
    size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n_lane ) return;
    size_t g = lane_global_index( i, lanes, lane );
    out_rgb[ g * 3 ] = lane_out[ i * 3 ]; out_rgb[ g * 3 + 1 ] = lane_out[ i * 3 + 1 ]; out_rgb[ g * 3 + 2 ] = lane_out[ i * 3 + 2 ];
}

/* lane_rays[ i ] = the lane's i-th ray of a ray call (k_lane_gather for six doubles) */
__global__ void k_lane_gather_rays( const double* __restrict__ rays, size_t n_lane, int lanes, int lane, double* __restrict__ lane_rays )
{
    size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n_lane ) return;
    size_t g = lane_global_index( i, lanes, lane );
    for( int k = 0; k < 6; k++ ) lane_rays[ i * 6 + k ] = rays[ g * 6 + k ];
}

/* A lane = a clone of the handle that borrows the resident scene and owns a stream, its events, counter blocks and a host
 * thread.  Making a stream takes ~10 ms of host time (tools/bench_alloc: 12 streams 120 - 130 ms, one after the other whatever thread
 * asks; events, pinned memory and hipMalloc of any size are free beside that), so six lanes are 60 ms of a handle's first call, more
 * than its learning pass on the wine glass.  The HIP objects (lane_objects: nothing in it reads the parent) are therefore made on a
 * helper thread while the learning pass runs on the device (render_lanes), and the parent's fields are copied afterwards (bind_lane). */
static int lane_objects( int device, bool debug, acn_scene_handle** out )
{
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [ & ]() { return std::chrono::duration< double, std::milli >( std::chrono::steady_clock::now() - t_begin ).count(); };
    double t[ 5 ] = { 0, 0, 0, 0, 0 };
    acn_scene_handle* l = new acn_scene_handle();
    l->is_lane = true;
    l->device = device;
#define HIP_TRY_L( expr ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) { acn_scene_free( l ); return fail( ACN_ERR_DEVICE, hipGetErrorString( e_ ) ); } } while( 0 )
    HIP_TRY_L( hipSetDevice( device ) );
    t[ 0 ] = since();
    HIP_TRY_L( hipStreamCreateWithFlags( &l->stream, hipStreamNonBlocking ) );
    t[ 1 ] = since();
    HIP_TRY_L( hipEventCreate( &l->ev0 ) );
    HIP_TRY_L( hipEventCreate( &l->ev1 ) );
    t[ 2 ] = since();
    HIP_TRY_L( hipMalloc( &l->d_counters, sizeof( unsigned long long ) * ACN_CNT_SLOTS ) );
    HIP_TRY_L( hipMalloc( &l->d_counters_keep, sizeof( unsigned long long ) * ACN_CNT_SLOTS ) );
    HIP_TRY_L( hipMalloc( &l->d_counts, sizeof( uint32_t ) * QC_N * ACN_LEVEL_BLOCKS ) );
    /* on the lane's own stream, where everything that uses them follows (the null stream would wait for the caller's) */
    HIP_TRY_L( hipMemsetAsync( l->d_counters, 0, sizeof( unsigned long long ) * ACN_CNT_SLOTS, l->stream ) );
    HIP_TRY_L( hipMemsetAsync( l->d_counts, 0, sizeof( uint32_t ) * QC_N * ACN_LEVEL_BLOCKS, l->stream ) );
    t[ 3 ] = since();
    HIP_TRY_L( hipHostMalloc( &l->h_counts, sizeof( uint32_t ) * QC_N * ACN_LEVEL_BLOCKS ) );
    t[ 4 ] = since();
#undef HIP_TRY_L
    l->worker = new LaneWorker();
    l->worker->start();
    if( debug ) fprintf( stderr, "[acn lane] set device %.2f ms, stream %.2f, events %.2f, counter blocks + memsets %.2f, pinned block %.2f, thread %.2f\n", t[ 0 ], t[ 1 ] - t[ 0 ], t[ 2 ] - t[ 1 ], t[ 3 ] - t[ 2 ], t[ 4 ] - t[ 3 ], since() - t[ 4 ] );
    *out = l;
    return ACN_OK;
}

/* a device buffer of at least `want` doubles: grown, never shrunk */
static int grow_buffer( double** p, size_t* cap, size_t want )
{
    if( *cap >= want ) return ACN_OK;
    if( *p ) hipFree( *p );
    *p = nullptr; *cap = 0;
    HIP_TRY( hipMalloc( p, sizeof( double ) * want ) );
    *cap = want;
    return ACN_OK;
}

static unsigned lane_grid( const acn_scene_handle* parent ) { return parent->tun.grid ? parent->tun.grid : parent->cus * 1u; }
static void bind_lane( const acn_scene_handle* parent, int lanes, acn_scene_handle* l )
{
    l->budget_div = ( size_t )lanes;
    l->dev = parent->dev;
    l->scene = parent->scene;
    l->tun = parent->tun; l->cus = parent->cus;
    l->workspace_budget = parent->workspace_budget;
    /* Round 4: six lanes on grids of ONE workgroup per CU (k_shade: one and a half) instead of four lanes on two.  With k_walk at
     * four waves per SIMD a grid of 256 workgroups is resident at once, and six shorter chains fill each other's tails better than
     * four: 1080p 50.2 -> 49.1 ms, c2 26.4 -> 25.0, and the share one of 8 GPUs gets 12.25 -> 11.4 ms (profiles/r04/ab_lanes6_*).
     * A call that runs ALONE on the handle keeps four workgroups per CU (diamond on one lane: 2.3 s with them, 6.7 s with one). */
    l->grid = lane_grid( parent );
    l->shade_grid = parent->tun.shade_grid ? parent->tun.shade_grid : parent->cus * 3u / 2u;
    l->walk_grid = parent->tun.walk_grid ? parent->tun.walk_grid : l->grid;
    l->dev.flags = l->d_counts + QC_FLAGS;
}

/* number of lanes for a call of n positions: the handle's ACN_LANES, fewer while a lane would get less than 32 tiles or
 * less than ~10^6 path samples' worth of work (a frame without path tracing is over before a second lane has started) */
static int lanes_for_counts( int tun_lanes, size_t n, uint64_t path_samples )
{
    int lanes = tun_lanes;
    const size_t work = n * ( size_t )( path_samples + 1 );
    while( lanes > 1 && ( n < ( size_t )lanes * 32 * ACN_LANE_TILE || work < ( size_t )lanes << 20 ) ) lanes--;
    return lanes;
}
static int lanes_for( const acn_scene_handle* h, size_t n ) { return lanes_for_counts( h->tun.lanes, n, h->dev.prm.path_samples ); }

static int render_lanes( acn_scene_handle* h, int lanes, const Primary& prim, size_t n, double* d_out_rgb,
                         const acn_render_opts* opts, hipStream_t stream )
{
    /* ACN_DEBUG_CHUNKS: where a call's wall time goes before and after the lanes run (one line per call on stderr) */
    const auto t_begin = std::chrono::steady_clock::now();
    double t_mark[ 5 ] = { 0, 0, 0, 0, 0 };
    auto mark = [ & ]( int i ) { t_mark[ i ] = std::chrono::duration< double, std::milli >( std::chrono::steady_clock::now() - t_begin ).count(); };
    /* the lanes this call lacks: made on a helper thread while the learning pass of a cold handle runs (see lane_objects) */
    early_lanes_join( h );
    for( acn_scene_handle* l : h->early_made ) { bind_lane( h, lanes, l ); h->lanes.push_back( l ); }   /* made during the upload */
    h->early_made.clear();
    const int missing = lanes - ( int )h->lanes.size();
    std::vector< acn_scene_handle* > made;
    int made_status = ACN_OK; std::string made_message;
    auto make_missing = [ & ]()
    {
        for( int k = 0; k < missing && made_status == ACN_OK; k++ )
        {
            acn_scene_handle* l = nullptr;
            made_status = lane_objects( h->device, h->tun.debug_chunks, &l );
            if( made_status == ACN_OK ) made.push_back( l ); else made_message = g_last_error;   /* thread-local where it was set */
        }
    };
    std::thread maker;
    const bool learn = h->lanes.empty() ? !rates_known( h ) : !rates_known( h->lanes[ 0 ] ) && !rates_known( h );
    const bool maker_used = missing > 0 && learn && h->tun.cold_pipeline;
    if( missing > 0 ) { if( maker_used ) maker = std::thread( make_missing ); else make_missing(); }
    /* what the caller queued on `stream` before this call must be done before the lanes read the positions */
    hipError_t drained = hipEventRecord( h->ev0, stream );
    if( drained == hipSuccess ) drained = hipEventSynchronize( h->ev0 );
    mark( 0 );
    /* a cold handle learns the scene's queue demand once, for all lanes, from a sample of the call (learn_rates) */
    int learned = ACN_OK;
    if( drained == hipSuccess && learn )
    {
        h->budget_div = 1;
        learned = learn_rates( h, prim, n, stream, n / ( size_t )lanes, lane_grid( h ) );
        if( learned == ACN_OK ) drained = hipStreamSynchronize( stream );
    }
    if( maker.joinable() ) maker.join();
    for( acn_scene_handle* l : made ) { bind_lane( h, lanes, l ); h->lanes.push_back( l ); }
    if( drained != hipSuccess ) return fail( ACN_ERR_DEVICE, hipGetErrorString( drained ) );
    if( learned != ACN_OK ) return learned;
    if( made_status != ACN_OK ) return fail( made_status, made_message );
    /* what one arrangement learned about the scene (records per position) holds for the other */
    for( int k = 0; k < lanes; k++ )
    {
        acn_scene_handle* l = h->lanes[ k ];
        const acn_scene_handle* from = rates_known( h ) ? h : h->lanes[ 0 ];
        if( rates_known( l ) || !rates_known( from ) ) continue;
        for( int q = 0; q < WQ_N; q++ ) l->rate[ q ] = from->rate[ q ];
        l->rate_cnt = from->rate_cnt; l->ctl.fill_target = from->ctl.fill_target;
        for( int level = 0; level <= ACN_MAX_PATH_LEVELS; level++ ) l->walk_passes_seen[ level ] = 0;
    }
    if( learn && rates_known( h ) ) free_workspace( h );   /* the bound is the handle's, whoever uses it */
    /* The lanes' queues are (re-)sized here, while the device is idle: hipFree synchronises the device, so lanes that
     * re-size at the start of their chains wait for each other's chunks (second frame of paraffin_lamp 400x600, whose
     * queues are trimmed to the rates the first frame learned: 2.1 s instead of 0.45, profiles/r03/frames_paraffin_*.txt).
     * hipMalloc itself is not what a first call pays: 22 GB of queues take 1 - 5 ms (tools/bench_alloc: 0.02 ms per GB; a lane that
     * started as soon as its own queues existed gained nothing, profiles/r04/first_frames_s36_s38.txt). */
    mark( 1 );
    acn_render_opts lane_opts{};
    if( opts ) lane_opts = *opts;
    std::vector< int > status( lanes, ACN_OK );
    std::vector< std::string > message( lanes );
    auto post_lane = [ & ]( int k )
    {
        h->lanes[ k ]->worker->post( [ &, k ]()
        {
            acn_scene_handle* l = h->lanes[ k ];
            l->budget_div = ( size_t )lanes;
            size_t cnt = lane_count( n, lanes, k );
            auto run = [ & ]() -> int
            {
                HIP_TRY( hipSetDevice( h->device ) );
                if( cnt == 0 ) { l->events_used = 0; HIP_TRY( hipMemset( l->d_counters, 0, sizeof( unsigned long long ) * ACN_CNT_SLOTS ) ); return ACN_OK; }
                /* the lane's share of the input: positions (2 doubles each) or rays (6) */
                int st = grow_buffer( &l->d_lane_in, &l->lane_in_cap, ( prim.rays ? 6 : 2 ) * cnt );
                if( st == ACN_OK ) st = grow_buffer( &l->d_lane_out, &l->lane_out_cap, 3 * cnt );
                if( st != ACN_OK ) return st;
                if( prim.rays )
                    hipLaunchKernelGGL( k_lane_gather_rays, dim3( ( unsigned )( ( cnt + 255 ) / 256 ) ), dim3( 256 ), 0, l->stream,
                                        prim.rays, cnt, lanes, k, l->d_lane_in );
                else
                    hipLaunchKernelGGL( k_lane_gather, dim3( ( unsigned )( ( cnt + 255 ) / 256 ) ), dim3( 256 ), 0, l->stream,
                                        prim.pos_xy, prim.first, ( uint64_t )h->dev.prm.image_width, cnt, lanes, k, l->d_lane_in );
                HIP_TRY( hipGetLastError() );
                st = launch_render( l, prim.rays ? primary_rays( l->d_lane_in ) : primary_positions( l->d_lane_in ), cnt, l->d_lane_out, &lane_opts, l->stream );
                if( st != ACN_OK ) return st;
                hipLaunchKernelGGL( k_lane_scatter, dim3( ( unsigned )( ( cnt + 255 ) / 256 ) ), dim3( 256 ), 0, l->stream,
                                    ( const double* )l->d_lane_out, cnt, lanes, k, d_out_rgb );
                HIP_TRY( hipGetLastError() );
                HIP_TRY( hipStreamSynchronize( l->stream ) );
                return ACN_OK;
            };
            status[ k ] = run();
            if( status[ k ] != ACN_OK ) message[ k ] = g_last_error;   /* thread-local in the worker */
        } );
    };
    for( int k = 0; k < lanes; k++ )
    {
        acn_scene_handle* l = h->lanes[ k ];
        l->budget_div = ( size_t )lanes;
        l->seeded = prim.rays != nullptr;
        const size_t cnt = lane_count( n, lanes, k );
        if( cnt ) { int st = ensure_workspace( l, cnt ); if( st != ACN_OK ) return st; }
    }
    for( int k = 0; k < lanes; k++ ) post_lane( k );
    mark( 2 );
    for( int k = 0; k < lanes; k++ ) h->lanes[ k ]->worker->wait();
    mark( 3 );
    if( h->tun.debug_chunks )
        fprintf( stderr, "[acn call] %zu positions on %d lanes: %d lanes made%s, caller's stream drained after %.2f ms, learning pass %.2f, queues sized %.2f, lanes done %.2f\n",
                 n, lanes, missing > 0 ? missing : 0, maker_used ? " beside the learning pass" : "", t_mark[ 0 ], t_mark[ 1 ] - t_mark[ 0 ], t_mark[ 2 ] - t_mark[ 1 ], t_mark[ 3 ] - t_mark[ 2 ] );
    for( int k = 0; k < lanes; k++ ) if( status[ k ] != ACN_OK ) return fail( status[ k ], message[ k ] );
    HIP_TRY( hipEventRecord( h->ev1, stream ) );
    /* statistics of the call: sums / maxima over the lanes */
    h->events_used = 0;
    h->launches[ 0 ] = h->launches[ 1 ] = h->launches[ 2 ] = h->launches[ 3 ] = 0;
    h->hard_rays = h->walk_steps = h->walk_rays = h->shade_hit_recs = h->host_syncs = h->private_rays = h->probe_rays = 0; h->flags_seen = 0;
    h->chunks = h->retries = h->levels = 0;
    h->ctl.retry_bound = 0;   /* (a call that ended in the middle of a retry) */
    h->peak_tasks = h->peak_children = 0;
    for( int k = 0; k < lanes; k++ )
    {
        const acn_scene_handle* l = h->lanes[ k ];
        if( lane_count( n, lanes, k ) == 0 ) continue;
        for( int i = 0; i < 4; i++ ) h->launches[ i ] += l->launches[ i ];
        h->hard_rays += l->hard_rays; h->walk_steps += l->walk_steps; h->walk_rays += l->walk_rays; h->shade_hit_recs += l->shade_hit_recs;
        h->host_syncs += l->host_syncs; h->flags_seen |= l->flags_seen; h->private_rays += l->private_rays; h->probe_rays += l->probe_rays;
        h->chunks += l->chunks; h->retries += l->retries;
        if( l->levels > h->levels ) h->levels = l->levels;
        h->peak_tasks += l->peak_tasks; h->peak_children += l->peak_children;
    }
    h->used_lanes = true;
    h->lanes_used = lanes;
    h->timed = true;
    return ACN_OK;
}

/* the caller's options as far as the caller's header knew them (acn_render_opts.struct_size), the rest zero */
static acn_render_opts opts_of( const acn_render_opts* in )
{
    acn_render_opts o{};
    if( in )
    {
        /* 0: a caller that zero-initialises the struct (the memset idiom) and never heard of struct_size -- the word was a
         * reserved zero in the first published layout, which already had the shard members: the 40-byte base layout */
        size_t n = in->struct_size ? in->struct_size : ( size_t )ACN_RENDER_OPTS_BASE_SIZE;
        if( n > sizeof( o ) ) n = sizeof( o );
        memcpy( &o, in, n );
    }
    o.struct_size = ( uint32_t )sizeof( o );
    return o;
}
#define ACN_OPTS_VIEW const acn_render_opts opts_seen_ = opts_of( opts ); opts = &opts_seen_;

/* one pipeline run on the handle itself, or the concurrent lanes */
static int render_dispatch( acn_scene_handle* h, const Primary& prim, size_t n, double* d_out_rgb,
                            const acn_render_opts* opts, hipStream_t stream )
{
    int lanes = lanes_for( h, n );
    /* Lanes pay when a lane's share is ONE chunk: their chains overlap.  A call whose queues cannot hold it in one chunk
     * per lane within the workspace bound -- scenes with hundreds or thousands of path samples -- does better on one lane
     * with the whole bound: four times the chunk, a quarter of the chains, and each chunk fills the chip by itself
     * (diamond 1080p p512, every 16th pixel: 3.69 s on 4 lanes, 2.83 s on one; hanging_lamp 2160p p1024, every 64th:
     * 21.6 -> 15.4 s; wine_glass 1080p p64, which fits: 71 ms on 4 lanes, 95 on one). */
    if( lanes > 1 )
    {
        const acn_scene_handle* known = nullptr;
        if( !h->lanes.empty() && rates_known( h->lanes[ 0 ] ) ) known = h->lanes[ 0 ];
        else if( rates_known( h ) ) known = h;
        if( known )
        {
            double need = 0;
            for( int q = 0; q < WQ_N; q++ ) need += queue_demand( known->rate, q, prim.rays != nullptr ) * ( double )n / 0.7 * ( double )wq_bytes[ q ];
            /* (sticky by 30 %: rates move a little from call to call, and changing the arrangement re-allocates everything) */
            if( need > ( h->one_lane ? 0.7 : 1.0 ) * ( double )h->workspace_budget ) lanes = 1;
        }
        else if( h->dev.prm.path_samples >= 256 ) lanes = 1;
    }
    h->used_lanes = false;
    h->one_lane = lanes <= 1 && lanes_for( h, n ) > 1;
    /* what one arrangement learned about the scene (records per position) holds for the other */
    auto inherit = []( acn_scene_handle* to, const acn_scene_handle* from )
    {
        if( rates_known( to ) || !rates_known( from ) ) return;
        for( int q = 0; q < WQ_N; q++ ) to->rate[ q ] = from->rate[ q ];
        to->rate_cnt = from->rate_cnt; to->ctl.fill_target = from->ctl.fill_target;
        for( int level = 0; level <= ACN_MAX_PATH_LEVELS; level++ ) to->walk_passes_seen[ level ] = 0;
    };
    if( lanes <= 1 )
    {
        for( acn_scene_handle* l : h->lanes ) free_workspace( l );   /* the bound is the handle's, whoever uses it */
        if( !h->lanes.empty() ) inherit( h, h->lanes[ 0 ] );
        return launch_render( h, prim, n, d_out_rgb, opts, stream );
    }
    free_workspace( h );
    return render_lanes( h, lanes, prim, n, d_out_rgb, opts, stream );   /* (makes the lanes it lacks) */
}

extern "C" int acn_render_positions_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, void* d_out_rgb,
                                         const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !d_pos_xy || !d_out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    int st = render_dispatch( h, primary_positions( ( const double* )d_pos_xy ), n, ( double* )d_out_rgb, opts, stream );
    if( st != ACN_OK ) return st;
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_render_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, void* d_out_rgb,
                                         const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( count && !d_out_rgb ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( first + count > h->dev.prm.image_width * h->dev.prm.image_height ) return fail( ACN_ERR_ARG, "pixel range outside the image" );
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    int st = render_dispatch( h, primary_main_pass( first ), count, ( double* )d_out_rgb, opts, stream );
    if( st != ACN_OK ) return st;
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

/* an entry point on host buffers: n records of in_len doubles copied in, the device-buffer call `dev( d_in, d_out )` (on the
 * handle's own stream: synchronous), n records of out_len doubles copied out */
template< class DevCall >
static int on_host_buffers( acn_scene_handle* h, const double* in, size_t in_len, size_t n, double* out, size_t out_len, DevCall dev )
{
    HIP_TRY( hipSetDevice( h->device ) );
    double* d_in = nullptr; double* d_out = nullptr;
    HIP_TRY( hipMalloc( &d_in, sizeof( double ) * in_len * n ) );
    hipError_t e = hipMalloc( &d_out, sizeof( double ) * out_len * n );
    if( e != hipSuccess ) { hipFree( d_in ); return fail( ACN_ERR_DEVICE, hipGetErrorString( e ) ); }
    int st = ACN_OK;
    if( hipMemcpy( d_in, in, sizeof( double ) * in_len * n, hipMemcpyHostToDevice ) != hipSuccess ) st = fail( ACN_ERR_DEVICE, "H2D copy failed" );
    if( st == ACN_OK ) st = dev( d_in, d_out );
    if( st == ACN_OK && hipMemcpy( out, d_out, sizeof( double ) * out_len * n, hipMemcpyDeviceToHost ) != hipSuccess ) st = fail( ACN_ERR_DEVICE, "D2H copy failed" );
    hipFree( d_in ); hipFree( d_out );
    return st;
}

extern "C" int acn_render_positions( acn_scene_handle* h, const double* pos_xy, size_t n, double* out_rgb,
                                     const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !pos_xy || !out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    acn_render_opts o = *opts;
    o.stream = nullptr;
    return on_host_buffers( h, pos_xy, 2, n, out_rgb, 3, [ & ]( double* d_pos, double* d_out ) { return acn_render_positions_dev( h, d_pos, n, d_out, &o ); } );
}

/* ---- caller-supplied primary rays (k_rays.hip) ---- */
extern "C" int acn_render_rays_dev( acn_scene_handle* h, const void* d_rays, size_t n, void* d_out_rgb, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !d_rays || !d_out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many rays in one call" );
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    /* every ray is checked before anything is rendered: the lowest index of a refused one, one word read back */
    if( !h->d_ray_check ) HIP_TRY( hipMalloc( &h->d_ray_check, sizeof( unsigned long long ) ) );
    HIP_TRY( hipMemsetAsync( h->d_ray_check, 0xFF, sizeof( unsigned long long ), stream ) );
    acn_launch_check_rays( ( const double* )d_rays, n, h->d_ray_check, stream );
    HIP_TRY( hipGetLastError() );
    unsigned long long bad = 0;
    HIP_TRY( hipMemcpyAsync( &bad, h->d_ray_check, sizeof( bad ), hipMemcpyDeviceToHost, stream ) );
    HIP_TRY( hipStreamSynchronize( stream ) );
    if( bad < n ) return fail( ACN_ERR_ARG, "ray " + std::to_string( bad ) + ": a component is not finite or the direction has no length" );
    int st = render_dispatch( h, primary_rays( ( const double* )d_rays ), n, ( double* )d_out_rgb, opts, stream );
    if( st != ACN_OK ) return st;
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_render_rays( acn_scene_handle* h, const double* rays, size_t n, double* out_rgb, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !rays || !out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    acn_render_opts o = *opts;
    o.stream = nullptr;
    return on_host_buffers( h, rays, 6, n, out_rgb, 3, [ & ]( double* d_rays, double* d_out ) { return acn_render_rays_dev( h, d_rays, n, d_out, &o ); } );
}

extern "C" int acn_camera_rays_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, void* d_out_rays, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !d_pos_xy || !d_out_rays ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many positions in one call" );
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    acn_launch_camera_rays( h->dev, ( const double* )d_pos_xy, n, ( double* )d_out_rays, stream );
    HIP_TRY( hipGetLastError() );
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_camera_rays( acn_scene_handle* h, const double* pos_xy, size_t n, double* out_rays )
{
    if( !h || ( n && ( !pos_xy || !out_rays ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    return on_host_buffers( h, pos_xy, 2, n, out_rays, 6, [ & ]( double* d_pos, double* d_out ) { return acn_camera_rays_dev( h, d_pos, n, d_out, nullptr ); } );
}

/* ---- surface records (k_surface.hip) ---- */
static int surface_dev( acn_scene_handle* h, const double* d_rays, const double* d_pos_xy, size_t n, uint32_t mode, double* d_out,
                        const acn_render_opts* opts )
{
    if( !h || ( n && ( !( d_rays || d_pos_xy ) || !d_out ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( mode != ACN_SURF_FIRST_HIT && mode != ACN_SURF_FOLLOW ) return fail( ACN_ERR_ARG, "unknown surface mode " + std::to_string( mode ) );
    if( opts && opts->shard_world > 1 ) return fail( ACN_ERR_ARG, "a surface call is not sharded: slice the array" );
    if( n == 0 ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    if( !h->d_surface_flags )
    {
        HIP_TRY( hipMalloc( &h->d_surface_flags, sizeof( uint32_t ) ) );
        HIP_TRY( hipMemset( h->d_surface_flags, 0, sizeof( uint32_t ) ) );
    }
    if( d_rays )
    {
        /* every ray is checked before anything is written: the lowest index of a refused one, one word read back */
        if( !h->d_ray_check ) HIP_TRY( hipMalloc( &h->d_ray_check, sizeof( unsigned long long ) ) );
        HIP_TRY( hipMemsetAsync( h->d_ray_check, 0xFF, sizeof( unsigned long long ), stream ) );
        acn_launch_check_rays( d_rays, n, h->d_ray_check, stream );
        HIP_TRY( hipGetLastError() );
        unsigned long long bad = 0;
        HIP_TRY( hipMemcpyAsync( &bad, h->d_ray_check, sizeof( bad ), hipMemcpyDeviceToHost, stream ) );
        HIP_TRY( hipStreamSynchronize( stream ) );
        if( bad < n ) return fail( ACN_ERR_ARG, "ray " + std::to_string( bad ) + ": a component is not finite or the direction has no length" );
    }
    SceneArgs s = scene_args( h );
    s.dev.flags = h->d_surface_flags;   /* the pipeline's word stays the pipeline's */
    acn_launch_surface( mode, h->scene.lds_bytes != 0, machine_lds_bytes( h ), stream, s, d_rays, d_pos_xy, n, d_out );
    HIP_TRY( hipGetLastError() );
    if( !( opts && opts->stream ) )
    {
        uint32_t flags = 0;
        HIP_TRY( hipMemcpyAsync( &flags, h->d_surface_flags, sizeof( flags ), hipMemcpyDeviceToHost, stream ) );
        HIP_TRY( hipStreamSynchronize( stream ) );
        if( flags )
        {
            HIP_TRY( hipMemset( h->d_surface_flags, 0, sizeof( uint32_t ) ) );
            return fail( ACN_ERR_UNSUPPORTED, "device CSG / compound stack overflow in a surface call" );
        }
    }
    return ACN_OK;
}

extern "C" int acn_surface_rays_dev( acn_scene_handle* h, const void* d_rays, size_t n, uint32_t mode, void* d_out, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && !d_rays ) ) return fail( ACN_ERR_ARG, "null argument" );
    return surface_dev( h, ( const double* )d_rays, nullptr, n, mode, ( double* )d_out, opts );
}

extern "C" int acn_surface_positions_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, uint32_t mode, void* d_out, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && !d_pos_xy ) ) return fail( ACN_ERR_ARG, "null argument" );
    return surface_dev( h, nullptr, ( const double* )d_pos_xy, n, mode, ( double* )d_out, opts );
}

/* the host-buffer forms: synchronous, on the handle's own stream */
static int surface_host( acn_scene_handle* h, const double* in, size_t in_len, size_t n, uint32_t mode, double* out, const acn_render_opts* opts )
{
    if( !h || ( n && ( !in || !out ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( mode != ACN_SURF_FIRST_HIT && mode != ACN_SURF_FOLLOW ) return fail( ACN_ERR_ARG, "unknown surface mode " + std::to_string( mode ) );
    if( opts->shard_world > 1 ) return fail( ACN_ERR_ARG, "a surface call is not sharded: slice the array" );
    if( n == 0 ) return ACN_OK;
    acn_render_opts o = *opts;
    o.stream = nullptr;
    return on_host_buffers( h, in, in_len, n, out, ACN_SURF_STRIDE, [ & ]( double* d_in, double* d_out )
    {
        return in_len == 6 ? surface_dev( h, d_in, nullptr, n, mode, d_out, &o ) : surface_dev( h, nullptr, d_in, n, mode, d_out, &o );
    } );
}

extern "C" int acn_surface_rays( acn_scene_handle* h, const double* rays, size_t n, uint32_t mode, double* out, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    return surface_host( h, rays, 6, n, mode, out, opts );
}

extern "C" int acn_surface_positions( acn_scene_handle* h, const double* pos_xy, size_t n, uint32_t mode, double* out, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    return surface_host( h, pos_xy, 2, n, mode, out, opts );
}

/* ---- sharding of whole positions: tiles of ACN_SHARD_TILE, round-robin (plain arithmetic, no GPU) ---- */
extern "C" size_t acn_shard_tile_count( size_t n, uint32_t rank, uint32_t world )
{
    if( world <= 1 ) return rank == 0 ? n : 0;
    return rank < world ? lane_count( n, ( int )world, ( int )rank ) : 0;
}
extern "C" size_t acn_shard_tile_padded( size_t n, uint32_t world )
{
    if( world <= 1 ) return n;
    size_t tiles = ( n + ACN_SHARD_TILE - 1 ) / ACN_SHARD_TILE;
    return ( ( tiles + world - 1 ) / world ) * ACN_SHARD_TILE;
}
extern "C" size_t acn_shard_tile_index( size_t n, uint32_t rank, uint32_t world, size_t i )
{
    ( void )n;
    if( world <= 1 ) return i;
    return ( ( i / ACN_SHARD_TILE ) * world + rank ) * ACN_SHARD_TILE + ( i % ACN_SHARD_TILE );
}

__global__ void k_shard_unpack( const double* __restrict__ gathered, size_t n, uint32_t world, size_t padded, double* __restrict__ frame )
{
    size_t g = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( g >= n ) return;
    size_t tile = g / ACN_SHARD_TILE;
    size_t r = tile % world, i = ( tile / world ) * ACN_SHARD_TILE + g % ACN_SHARD_TILE;
    const double* src = gathered + ( r * padded + i ) * 3;
    frame[ g * 3 ] = src[ 0 ]; frame[ g * 3 + 1 ] = src[ 1 ]; frame[ g * 3 + 2 ] = src[ 2 ];
}

extern "C" int acn_render_main_pass_shard_dev( acn_scene_handle* h, size_t first, size_t count, uint32_t rank, uint32_t world,
                                               void* d_part, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( count && !d_part ) || world == 0 || rank >= world ) return fail( ACN_ERR_ARG, "bad argument" );
    if( first + count > h->dev.prm.image_width * h->dev.prm.image_height ) return fail( ACN_ERR_ARG, "pixel range outside the image" );
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    const size_t mine = acn_shard_tile_count( count, rank, world ), padded = acn_shard_tile_padded( count, world );
    if( padded > mine ) HIP_TRY( hipMemsetAsync( ( double* )d_part + 3 * mine, 0, sizeof( double ) * 3 * ( padded - mine ), stream ) );
    if( mine )
    {
        if( h->shard_pos_cap < mine )
        {
            if( h->d_shard_pos ) hipFree( h->d_shard_pos );
            h->d_shard_pos = nullptr; h->shard_pos_cap = 0;
            HIP_TRY( hipMalloc( &h->d_shard_pos, sizeof( double ) * 2 * mine ) );
            h->shard_pos_cap = mine;
        }
        hipLaunchKernelGGL( k_lane_gather, dim3( ( unsigned )( ( mine + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                            ( const double* )nullptr, first, ( uint64_t )h->dev.prm.image_width, mine, ( int )world, ( int )rank, h->d_shard_pos );
        HIP_TRY( hipGetLastError() );
        int st = render_dispatch( h, primary_positions( h->d_shard_pos ), mine, ( double* )d_part, opts, stream );
        if( st != ACN_OK ) return st;
    }
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_shard_unpack_dev( acn_scene_handle* h, const void* d_gathered, size_t count, uint32_t world, void* d_frame,
                                     const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( count && ( !d_gathered || !d_frame ) ) || world == 0 ) return fail( ACN_ERR_ARG, "bad argument" );
    if( count == 0 ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    hipLaunchKernelGGL( k_shard_unpack, dim3( ( unsigned )( ( count + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        ( const double* )d_gathered, count, world, acn_shard_tile_padded( count, world ), ( double* )d_frame );
    HIP_TRY( hipGetLastError() );
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_resolve_dev( acn_scene_handle* h, const void* d_linear_rgb, size_t n, void* d_out_rgb, void* d_out_rgb8,
                                const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && !d_linear_rgb ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    hipLaunchKernelGGL( k_resolve, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        ( const double* )d_linear_rgb, n, h->dev.prm.gamma, ( double* )d_out_rgb, ( unsigned char* )d_out_rgb8 );
    HIP_TRY( hipGetLastError() );
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

/* ---- the edge-avoiding filter (k_denoise.hip) ---- */
struct DenoiseSetup { uint32_t iterations, normal_power_log2, no_demodulate; double sigma_plane, sigma_lum; };

/* every check of a denoise call: on the host, before the handle is touched */
static int denoise_check( const acn_scene_handle* h, const void* lin, const void* surf, size_t width, size_t height,
                          const acn_denoise_params* prm, const void* out, const acn_render_opts* opts, DenoiseSetup* su )
{
    if( !h || !lin || !surf || !out ) return fail( ACN_ERR_ARG, "null argument" );
    const size_t max_n = ( size_t )1 << 31;
    if( width == 0 || height == 0 ) return fail( ACN_ERR_ARG, "a frame to denoise needs a width and a height" );
    if( width > max_n || height > max_n || width * height > max_n ) return fail( ACN_ERR_ARG, "a frame to denoise has at most 2^31 pixels" );
    acn_denoise_params p{};
    if( prm )
    {
        if( prm->struct_size < sizeof( uint32_t ) ) return fail( ACN_ERR_ARG, "acn_denoise_params.struct_size " + std::to_string( prm->struct_size ) + " is smaller than its first member" );
        memcpy( &p, prm, prm->struct_size < sizeof( p ) ? prm->struct_size : sizeof( p ) );
    }
    if( p.flags & ~( ACN_DENOISE_NO_DEMODULATE | ACN_DENOISE_NORMAL_POWER_SET ) ) return fail( ACN_ERR_ARG, "unknown acn_denoise_params.flags bits" );
    if( p.iterations > ACN_DENOISE_MAX_ITERATIONS ) return fail( ACN_ERR_ARG, "acn_denoise_params.iterations " + std::to_string( p.iterations ) + " is above 8" );
    if( p.normal_power_log2 > ACN_DENOISE_MAX_NORMAL_POWER_LOG2 ) return fail( ACN_ERR_ARG, "acn_denoise_params.normal_power_log2 " + std::to_string( p.normal_power_log2 ) + " is above 10" );
    const double sig[ 2 ] = { p.sigma_plane, p.sigma_lum };
    for( double s : sig ) if( !( s >= 0 ) || s > 1.7976931348623157e308 ) return fail( ACN_ERR_ARG, "a sigma of acn_denoise_params is negative or not finite" );
    if( opts && opts->shard_world > 1 ) return fail( ACN_ERR_ARG, "a denoise call is not sharded: the filter needs the whole frame" );
    su->iterations = p.iterations ? p.iterations : ACN_DENOISE_DEFAULT_ITERATIONS;
    su->normal_power_log2 = ( p.normal_power_log2 || ( p.flags & ACN_DENOISE_NORMAL_POWER_SET ) ) ? p.normal_power_log2 : ACN_DENOISE_DEFAULT_NORMAL_POWER_LOG2;
    su->no_demodulate = ( p.flags & ACN_DENOISE_NO_DEMODULATE ) ? 1u : 0u;
    su->sigma_plane = p.sigma_plane != 0 ? p.sigma_plane : ACN_DENOISE_DEFAULT_SIGMA_PLANE;
    su->sigma_lum = p.sigma_lum != 0 ? p.sigma_lum : ACN_DENOISE_DEFAULT_SIGMA_LUM;
    return ACN_OK;
}

extern "C" int acn_denoise_dev( acn_scene_handle* h, const void* d_linear_rgb, const void* d_surface, size_t width, size_t height,
                                const acn_denoise_params* prm, void* d_out_rgb, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    DenoiseSetup su;
    int st = denoise_check( h, d_linear_rgb, d_surface, width, height, prm, d_out_rgb, opts, &su );
    if( st != ACN_OK ) return st;
    if( ( uintptr_t )d_surface % 16 ) return fail( ACN_ERR_ARG, "the surface records of a denoise call are read 16 bytes at a time: align the buffer" );
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    const size_t need = width * height * ( size_t )ACN_DENOISE_SCRATCH_PER_PIXEL;
    if( h->denoise_bytes < need )
    {
        if( h->d_denoise ) hipFree( h->d_denoise );   /* (waits for whatever still reads it) */
        h->d_denoise = nullptr; h->denoise_bytes = 0;
        HIP_TRY( hipMalloc( &h->d_denoise, need ) );
        h->denoise_bytes = need;
    }
    acn_launch_denoise( ( const double* )d_linear_rgb, ( const double* )d_surface, width, height, su.iterations, su.normal_power_log2,
                        su.no_demodulate, su.sigma_plane, su.sigma_lum, h->d_denoise, ( double* )d_out_rgb, stream );
    HIP_TRY( hipGetLastError() );
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_denoise( acn_scene_handle* h, const double* linear_rgb, const double* surface, size_t width, size_t height,
                            const acn_denoise_params* prm, double* out_rgb, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    DenoiseSetup su;
    int st = denoise_check( h, linear_rgb, surface, width, height, prm, out_rgb, opts, &su );
    if( st != ACN_OK ) return st;
    HIP_TRY( hipSetDevice( h->device ) );
    const size_t n = width * height;
    double* d_rgb = nullptr; double* d_surf = nullptr;
    HIP_TRY( hipMalloc( &d_rgb, sizeof( double ) * 3 * n ) );
    hipError_t e = hipMalloc( &d_surf, sizeof( double ) * ACN_SURF_STRIDE * n );
    if( e != hipSuccess ) { hipFree( d_rgb ); return fail( ACN_ERR_DEVICE, hipGetErrorString( e ) ); }
    if( hipMemcpy( d_rgb, linear_rgb, sizeof( double ) * 3 * n, hipMemcpyHostToDevice ) != hipSuccess ||
        hipMemcpy( d_surf, surface, sizeof( double ) * ACN_SURF_STRIDE * n, hipMemcpyHostToDevice ) != hipSuccess ) st = fail( ACN_ERR_DEVICE, "H2D copy failed" );
    acn_render_opts o = *opts;
    o.stream = nullptr;
    if( st == ACN_OK ) st = acn_denoise_dev( h, d_rgb, d_surf, width, height, prm, d_rgb, &o );   /* in place */
    if( st == ACN_OK && hipMemcpy( out_rgb, d_rgb, sizeof( double ) * 3 * n, hipMemcpyDeviceToHost ) != hipSuccess ) st = fail( ACN_ERR_DEVICE, "D2H copy failed" );
    hipFree( d_rgb ); hipFree( d_surf );
    return st;
}

/* ---- the thin-lens camera (k_lens.hip) ---- */

/* every check of a lens call's parameters: on the host, before the handle is touched.  window: the samples an acn_lens_rays call asks for */
static int lens_check( const acn_scene_handle* h, const acn_lens_params* prm, const uint32_t* window, LensSetup* ls )
{
    if( !h ) return fail( ACN_ERR_ARG, "null argument" );
    acn_lens_params p;
    std::string msg;
    if( acn_lens_params_read( prm, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );   /* (acn_stats_host.h: the members alone) */
    if( p.aperture_radius > 0 && !( h->dev.prm.camera_focal_length > 0 ) ) return fail( ACN_ERR_ARG, "an open aperture needs a camera_focal_length above 0: the plane in focus lies in front of the camera" );
    ls->samples = p.samples ? p.samples : ACN_LENS_DEFAULT_SAMPLES;
    ls->jitter = ( p.flags & ACN_LENS_JITTER ) ? 1u : 0u;
    ls->seed = ACN_LENS_SEED + ( uint64_t )p.seed;
    ls->aperture_radius = p.aperture_radius;
    ls->focus_distance = p.aperture_radius > 0 ? p.focus_distance : 0.0;
    if( window )
    {
        if( window[ 1 ] == 0 ) return fail( ACN_ERR_ARG, "n_samples is 0" );
        if( ( uint64_t )window[ 0 ] + window[ 1 ] > ls->samples ) return fail( ACN_ERR_ARG, "first_sample + n_samples is above the " + std::to_string( ls->samples ) + " samples of the lens" );
    }
    return ACN_OK;
}

extern "C" int acn_lens_rays_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, uint32_t first_sample,
                                  uint32_t n_samples, void* d_out_rays, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !d_pos_xy || !d_out_rays ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    LensSetup ls;
    const uint32_t window[ 2 ] = { first_sample, n_samples };
    int st = lens_check( h, prm, window, &ls );
    if( st != ACN_OK ) return st;
    if( n > 0xFFFFFF00ull / n_samples ) return fail( ACN_ERR_ARG, "too many rays in one call" );
    if( n == 0 ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    acn_launch_lens_rays( h->dev, ( const double* )d_pos_xy, 0, n, ls, first_sample, n_samples, ( double* )d_out_rays, stream );
    HIP_TRY( hipGetLastError() );
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_lens_rays( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, uint32_t first_sample,
                              uint32_t n_samples, double* out_rays )
{
    if( !h || ( n && ( !pos_xy || !out_rays ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    LensSetup ls;
    const uint32_t window[ 2 ] = { first_sample, n_samples };
    int st = lens_check( h, prm, window, &ls );
    if( st != ACN_OK ) return st;
    if( n > 0xFFFFFF00ull / n_samples ) return fail( ACN_ERR_ARG, "too many rays in one call" );
    if( n == 0 ) return ACN_OK;
    return on_host_buffers( h, pos_xy, 2, n, out_rays, ( size_t )6 * n_samples, [ & ]( double* d_pos, double* d_out )
    {
        return acn_lens_rays_dev( h, d_pos, n, prm, first_sample, n_samples, d_out, nullptr );
    } );
}

/* a lens call after its null checks: d_pos_xy, or null for the pixel centres from `first` on.  Slice by slice: rays, the ray path of
 * acn_render_rays_dev (linear, its validity kernel left out: the rays are valid by construction), the ordered mean */
static int render_lens( acn_scene_handle* h, const double* d_pos_xy, size_t first, size_t n, const acn_lens_params* prm, double* d_out_rgb,
                        const acn_render_opts* opts, double* d_stats = nullptr, bool with_stats = false )
{
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );
    if( st != ACN_OK ) return st;
    const int linear = ( opts->flags & ACN_OPT_LINEAR_OUT ) ? 1 : 0;
    if( opts->shard_mode > ACN_SHARD_SAMPLES ) return fail( ACN_ERR_ARG, "unknown shard_mode" );
    if( opts->shard_mode == ACN_SHARD_SAMPLES && opts->shard_world > 1 )
    {
        if( opts->shard_rank >= opts->shard_world ) return fail( ACN_ERR_ARG, "shard_rank >= shard_world" );
        if( with_stats ) return fail( ACN_ERR_ARG, "lens statistics are not sharded by samples (ACN_SHARD_SAMPLES): deviations of partial radiances mean nothing" );
        if( !linear ) return fail( ACN_ERR_ARG, "a lens call sharded by samples gives partial means: it needs ACN_OPT_LINEAR_OUT" );
    }
    if( opts->cancel && *opts->cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
    if( n == 0 ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = opts->stream ? ( hipStream_t )opts->stream : h->stream;
    const size_t K = ls.samples;
    size_t slice = h->tun.lens_slice_rays / K;
    if( slice < 1 ) slice = 1;
    if( slice > n ) slice = n;
    if( h->lens_cap < slice * K )
    {
        if( h->d_lens_rays ) hipFree( h->d_lens_rays );   /* (waits for whatever still reads them) */
        if( h->d_lens_rad ) hipFree( h->d_lens_rad );
        h->d_lens_rays = h->d_lens_rad = nullptr; h->lens_cap = 0;
        HIP_TRY( hipMalloc( &h->d_lens_rays, sizeof( double ) * 6 * slice * K ) );
        HIP_TRY( hipMalloc( &h->d_lens_rad, sizeof( double ) * 3 * slice * K ) );
        h->lens_cap = slice * K;
    }
    acn_render_opts ray_opts = *opts;
    ray_opts.flags |= ACN_OPT_LINEAR_OUT;
    for( size_t base = 0; base < n; base += slice )
    {
        if( opts->cancel && *opts->cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
        const size_t cnt = n - base < slice ? n - base : slice;
        acn_launch_lens_rays( h->dev, d_pos_xy ? d_pos_xy + 2 * base : nullptr, first + base, cnt, ls, 0, ( uint32_t )K, h->d_lens_rays, stream );
        HIP_TRY( hipGetLastError() );
        st = render_dispatch( h, primary_rays( h->d_lens_rays ), cnt * K, h->d_lens_rad, &ray_opts, stream );
        if( st != ACN_OK ) return st;
        if( with_stats )
            acn_launch_lens_reduce_stats( h->d_lens_rad, cnt, ( uint32_t )K, h->dev.prm.gamma, linear, d_out_rgb ? d_out_rgb + 3 * base : nullptr,
                                          d_stats + ( size_t )ACN_STATS_STRIDE * base, stream );
        else
            acn_launch_lens_reduce( h->d_lens_rad, cnt, ( uint32_t )K, h->dev.prm.gamma, linear, d_out_rgb + 3 * base, stream );
        HIP_TRY( hipGetLastError() );
    }
    if( !opts->stream ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_render_lens_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, void* d_out_rgb,
                                    const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !d_pos_xy || !d_out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    return render_lens( h, ( const double* )d_pos_xy, 0, n, prm, ( double* )d_out_rgb, opts );
}

extern "C" int acn_render_lens_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, void* d_out_rgb,
                                              const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( count && !d_out_rgb ) ) return fail( ACN_ERR_ARG, "null argument" );
    const size_t pixels = h->dev.prm.image_width * h->dev.prm.image_height;
    if( first > pixels || count > pixels - first ) return fail( ACN_ERR_ARG, "pixel range outside the image" );
    return render_lens( h, nullptr, first, count, prm, ( double* )d_out_rgb, opts );
}

extern "C" int acn_render_lens( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, double* out_rgb,
                                const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !pos_xy || !out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );   /* (before the buffers are made; the device call checks the rest before it writes) */
    if( st != ACN_OK ) return st;
    if( n == 0 ) return ACN_OK;
    acn_render_opts o = *opts;
    o.stream = nullptr;
    return on_host_buffers( h, pos_xy, 2, n, out_rgb, 3, [ & ]( double* d_pos, double* d_out ) { return acn_render_lens_dev( h, d_pos, n, prm, d_out, &o ); } );
}

/* ---- lens sample statistics (k_lens.hip, k_denoise.hip; the checks that need no handle: acn_stats_host.h) ---- */
static int stats_buffer( const void* stats, size_t n, const char* what )
{
    std::string msg;
    return acn_stats_buffer_check( stats, n, what, &msg ) == ACN_OK ? ACN_OK : fail( ACN_ERR_ARG, msg );
}

extern "C" int acn_render_lens_stats_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, void* d_out_rgb,
                                          void* d_stats, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !d_pos_xy || !d_stats ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( stats_buffer( d_stats, n, "d_stats" ) != ACN_OK ) return ACN_ERR_ARG;
    return render_lens( h, ( const double* )d_pos_xy, 0, n, prm, ( double* )d_out_rgb, opts, ( double* )d_stats, true );
}

extern "C" int acn_render_lens_stats_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, void* d_out_rgb,
                                                    void* d_stats, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( count && !d_stats ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( stats_buffer( d_stats, count, "d_stats" ) != ACN_OK ) return ACN_ERR_ARG;
    const size_t pixels = h->dev.prm.image_width * h->dev.prm.image_height;
    if( first > pixels || count > pixels - first ) return fail( ACN_ERR_ARG, "pixel range outside the image" );
    return render_lens( h, nullptr, first, count, prm, ( double* )d_out_rgb, opts, ( double* )d_stats, true );
}

/* device copies of host arrays for one call; everything is freed when it goes */
struct DevCopies
{
    std::vector< void* > held;
    ~DevCopies() { for( void* p : held ) hipFree( p ); }
    /* null on failure; src (nullable) is copied in */
    void* make( const void* src, size_t bytes )
    {
        void* d = nullptr;
        if( hipMalloc( &d, bytes ? bytes : 1 ) != hipSuccess ) return nullptr;
        held.push_back( d );
        if( src && bytes && hipMemcpy( d, src, bytes, hipMemcpyHostToDevice ) != hipSuccess ) return nullptr;
        return d;
    }
};

extern "C" int acn_render_lens_stats( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, double* out_rgb,
                                      double* stats, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && ( !pos_xy || !stats ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );   /* (before the buffers are made; the device call checks the rest before it writes) */
    if( st != ACN_OK ) return st;
    if( opts->shard_mode == ACN_SHARD_SAMPLES && opts->shard_world > 1 )
        return fail( ACN_ERR_ARG, "lens statistics are not sharded by samples (ACN_SHARD_SAMPLES): deviations of partial radiances mean nothing" );
    if( n == 0 ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    DevCopies dc;
    void* d_pos = dc.make( pos_xy, sizeof( double ) * 2 * n );
    void* d_out = out_rgb ? dc.make( nullptr, sizeof( double ) * 3 * n ) : nullptr;
    void* d_st = dc.make( nullptr, sizeof( double ) * ACN_STATS_STRIDE * n );
    if( !d_pos || !d_st || ( out_rgb && !d_out ) ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    acn_render_opts o = *opts;
    o.stream = nullptr;
    st = acn_render_lens_stats_dev( h, d_pos, n, prm, d_out, d_st, &o );
    if( st != ACN_OK ) return st;
    if( out_rgb ) HIP_TRY( hipMemcpy( out_rgb, d_out, sizeof( double ) * 3 * n, hipMemcpyDeviceToHost ) );
    HIP_TRY( hipMemcpy( stats, d_st, sizeof( double ) * ACN_STATS_STRIDE * n, hipMemcpyDeviceToHost ) );
    return ACN_OK;
}

extern "C" int acn_lens_stats_merge_dev( acn_scene_handle* h, void* d_acc, size_t n_acc, const void* d_part, size_t n_part,
                                         const int64_t* d_index, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h ) return fail( ACN_ERR_ARG, "null argument" );
    if( opts->shard_world > 1 ) return fail( ACN_ERR_ARG, "a merge of lens statistics is not sharded" );
    if( stats_buffer( d_acc, n_acc, "d_acc" ) != ACN_OK || stats_buffer( d_part, n_part, "d_part" ) != ACN_OK ) return ACN_ERR_ARG;
    if( !d_index && n_part > n_acc ) return fail( ACN_ERR_ARG, "a merge without an index needs n_part <= n_acc" );
    if( ( uintptr_t )d_index % 8 ) return fail( ACN_ERR_ARG, "d_index is an array of int64_t: align the buffer" );
    if( n_part == 0 || n_acc == 0 ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = opts->stream ? ( hipStream_t )opts->stream : h->stream;
    acn_launch_stats_merge( ( double* )d_acc, n_acc, ( const double* )d_part, n_part, d_index, stream );
    HIP_TRY( hipGetLastError() );
    if( !opts->stream ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_lens_stats_merge( acn_scene_handle* h, double* acc, size_t n_acc, const double* part, size_t n_part,
                                     const int64_t* index, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n_acc && !acc ) || ( n_part && !part ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( opts->shard_world > 1 ) return fail( ACN_ERR_ARG, "a merge of lens statistics is not sharded" );
    std::string msg;
    if( acn_stats_index_check( index, n_part, n_acc, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n_part == 0 || n_acc == 0 ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    DevCopies dc;
    const size_t rec = sizeof( double ) * ACN_STATS_STRIDE;
    void* d_acc = dc.make( acc, rec * n_acc );
    void* d_part = dc.make( part, rec * n_part );
    void* d_index = index ? dc.make( index, sizeof( int64_t ) * n_part ) : nullptr;
    if( !d_acc || !d_part || ( index && !d_index ) ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    acn_render_opts o = *opts;
    o.stream = nullptr;
    int st = acn_lens_stats_merge_dev( h, d_acc, n_acc, d_part, n_part, ( const int64_t* )d_index, &o );
    if( st != ACN_OK ) return st;
    HIP_TRY( hipMemcpy( acc, d_acc, rec * n_acc, hipMemcpyDeviceToHost ) );
    return ACN_OK;
}

extern "C" int acn_lens_stats_resolve_dev( acn_scene_handle* h, const void* d_stats, size_t n, void* d_out_rgb, void* d_out_noise,
                                           const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    if( !h || ( n && !d_stats ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( opts->shard_world > 1 ) return fail( ACN_ERR_ARG, "a resolve of lens statistics is not sharded" );
    if( stats_buffer( d_stats, n, "d_stats" ) != ACN_OK ) return ACN_ERR_ARG;
    if( n == 0 || ( !d_out_rgb && !d_out_noise ) ) return ACN_OK;
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = opts->stream ? ( hipStream_t )opts->stream : h->stream;
    acn_launch_stats_resolve( ( const double* )d_stats, n, h->dev.prm.background_color, h->dev.prm.gamma, ( opts->flags & ACN_OPT_LINEAR_OUT ) ? 1 : 0,
                              ( double* )d_out_rgb, ( double* )d_out_noise, stream );
    HIP_TRY( hipGetLastError() );
    if( !opts->stream ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_denoise_stats_dev( acn_scene_handle* h, const void* d_stats, const void* d_surface, size_t width, size_t height,
                                      const acn_denoise_params* prm, void* d_out_rgb, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    DenoiseSetup su;
    int st = denoise_check( h, d_stats, d_surface, width, height, prm, d_out_rgb, opts, &su );
    if( st != ACN_OK ) return st;
    if( ( uintptr_t )d_surface % 16 ) return fail( ACN_ERR_ARG, "the surface records of a denoise call are read 16 bytes at a time: align the buffer" );
    if( stats_buffer( d_stats, width * height, "d_stats" ) != ACN_OK ) return ACN_ERR_ARG;
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = ( opts && opts->stream ) ? ( hipStream_t )opts->stream : h->stream;
    const size_t need = width * height * ( size_t )ACN_DENOISE_SCRATCH_PER_PIXEL;
    if( h->denoise_bytes < need )
    {
        if( h->d_denoise ) hipFree( h->d_denoise );   /* (waits for whatever still reads it) */
        h->d_denoise = nullptr; h->denoise_bytes = 0;
        HIP_TRY( hipMalloc( &h->d_denoise, need ) );
        h->denoise_bytes = need;
    }
    acn_launch_denoise_stats( ( const double* )d_stats, ( const double* )d_surface, width, height, su.iterations, su.normal_power_log2,
                              su.no_demodulate, su.sigma_plane, su.sigma_lum, h->dev.prm.background_color, h->d_denoise, ( double* )d_out_rgb, stream );
    HIP_TRY( hipGetLastError() );
    if( !( opts && opts->stream ) ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_denoise_stats( acn_scene_handle* h, const double* stats, const double* surface, size_t width, size_t height,
                                  const acn_denoise_params* prm, double* out_rgb, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    DenoiseSetup su;
    int st = denoise_check( h, stats, surface, width, height, prm, out_rgb, opts, &su );
    if( st != ACN_OK ) return st;
    HIP_TRY( hipSetDevice( h->device ) );
    const size_t n = width * height;
    DevCopies dc;
    void* d_st = dc.make( stats, sizeof( double ) * ACN_STATS_STRIDE * n );
    void* d_surf = dc.make( surface, sizeof( double ) * ACN_SURF_STRIDE * n );
    void* d_rgb = dc.make( nullptr, sizeof( double ) * 3 * n );
    if( !d_st || !d_surf || !d_rgb ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    acn_render_opts o = *opts;
    o.stream = nullptr;
    st = acn_denoise_stats_dev( h, d_st, d_surf, width, height, prm, d_rgb, &o );
    if( st != ACN_OK ) return st;
    HIP_TRY( hipMemcpy( out_rgb, d_rgb, sizeof( double ) * 3 * n, hipMemcpyDeviceToHost ) );
    return ACN_OK;
}

/* ---- selecting positions by a key (k_select.hip; the checks and the host arithmetic: acn_select_host.h) ---- */
extern "C" int acn_select_above_dev( acn_scene_handle* h, const void* d_key, size_t n, const acn_select_params* prm, const void* d_src_pos_xy,
                                     void* d_out_index, void* d_out_pos_xy, void* d_out_count, uint64_t* out_count, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    std::string msg;
    acn_select_params p;
    if( acn_select_args_check( h != nullptr, d_key, n, prm, d_src_pos_xy, d_out_index, d_out_pos_xy, opts->shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( ( uintptr_t )d_out_count % 8 ) return fail( ACN_ERR_ARG, "d_out_count is a uint64_t: align it" );
    const uint64_t width = p.raster_width ? p.raster_width : h->dev.prm.image_width;
    if( !d_src_pos_xy && d_out_pos_xy && width == 0 ) return fail( ACN_ERR_ARG, "raster positions need a raster_width or a scene with an image_width" );
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = opts->stream ? ( hipStream_t )opts->stream : h->stream;
    if( n == 0 )   /* no launch */
    {
        if( d_out_count ) HIP_TRY( hipMemsetAsync( d_out_count, 0, sizeof( uint64_t ), stream ) );
        if( !opts->stream ) HIP_TRY( hipStreamSynchronize( stream ) );
        if( out_count ) *out_count = 0;
        return ACN_OK;
    }
    const size_t words = ( size_t )acn_select_tiles( n ) + 1;
    if( h->select_tiles_cap < words )
    {
        if( h->d_select_tiles ) hipFree( h->d_select_tiles );   /* (waits for whatever still reads them) */
        h->d_select_tiles = nullptr; h->select_tiles_cap = 0;
        HIP_TRY( hipMalloc( &h->d_select_tiles, sizeof( unsigned long long ) * words ) );
        h->select_tiles_cap = words;
    }
    acn_launch_select( ( const double* )d_key, n, p.threshold, h->d_select_tiles, p.capacity, ( const double* )d_src_pos_xy, width, p.raster_first,
                       ( int64_t* )d_out_index, ( double* )d_out_pos_xy, ( unsigned long long* )d_out_count, stream );
    HIP_TRY( hipGetLastError() );
    if( out_count )   /* the one synchronisation of a caller's stream */
    {
        unsigned long long total = 0;
        HIP_TRY( hipMemcpyAsync( &total, h->d_select_tiles + ( words - 1 ), sizeof( total ), hipMemcpyDeviceToHost, stream ) );
        HIP_TRY( hipStreamSynchronize( stream ) );
        *out_count = total;
    }
    else if( !opts->stream ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_select_above( acn_scene_handle* h, const double* key, size_t n, const acn_select_params* prm, const double* src_pos_xy,
                                 int64_t* out_index, double* out_pos_xy, uint64_t* out_count )
{
    std::string msg;
    acn_select_params p;
    if( acn_select_args_check( h != nullptr, key, n, prm, src_pos_xy, out_index, out_pos_xy, 0, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) { if( out_count ) *out_count = 0; return ACN_OK; }
    HIP_TRY( hipSetDevice( h->device ) );
    const size_t cap = ( size_t )( p.capacity < n ? p.capacity : n );   /* (no more than n are ever selected) */
    DevCopies dc;
    void* d_key = dc.make( key, sizeof( double ) * n );
    void* d_src = src_pos_xy ? dc.make( src_pos_xy, sizeof( double ) * 2 * n ) : nullptr;
    void* d_index = out_index && cap ? dc.make( nullptr, sizeof( int64_t ) * cap ) : nullptr;
    void* d_pos = out_pos_xy && cap ? dc.make( nullptr, sizeof( double ) * 2 * cap ) : nullptr;
    if( !d_key || ( src_pos_xy && !d_src ) || ( out_index && cap && !d_index ) || ( out_pos_xy && cap && !d_pos ) ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    acn_select_params q = p;
    q.struct_size = ( uint32_t )sizeof( q );
    q.capacity = ( d_index || d_pos ) ? cap : 0;
    uint64_t total = 0;
    int st = acn_select_above_dev( h, d_key, n, &q, d_src, d_index, d_pos, nullptr, &total, nullptr );
    if( st != ACN_OK ) return st;
    const size_t wrote = ( size_t )( total < q.capacity ? total : q.capacity );
    if( d_index && wrote ) HIP_TRY( hipMemcpy( out_index, d_index, sizeof( int64_t ) * wrote, hipMemcpyDeviceToHost ) );
    if( d_pos && wrote ) HIP_TRY( hipMemcpy( out_pos_xy, d_pos, sizeof( double ) * 2 * wrote, hipMemcpyDeviceToHost ) );
    if( out_count ) *out_count = total;
    return ACN_OK;
}

extern "C" int acn_key_histogram_dev( acn_scene_handle* h, const void* d_key, size_t n, void* d_out_hist, const acn_render_opts* opts )
{
    ACN_OPTS_VIEW
    std::string msg;
    if( acn_key_hist_args_check( h != nullptr, d_key, n, d_out_hist, opts->shard_world, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    HIP_TRY( hipSetDevice( h->device ) );
    hipStream_t stream = opts->stream ? ( hipStream_t )opts->stream : h->stream;
    HIP_TRY( hipMemsetAsync( d_out_hist, 0, sizeof( uint64_t ) * ACN_KEY_HIST_WORDS, stream ) );
    if( n ) acn_launch_key_hist( ( const double* )d_key, n, ( unsigned long long* )d_out_hist, stream );
    HIP_TRY( hipGetLastError() );
    if( !opts->stream ) HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_key_histogram( acn_scene_handle* h, const double* key, size_t n, uint64_t* out_hist )
{
    std::string msg;
    if( acn_key_hist_args_check( h != nullptr, key, n, out_hist, 0, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    HIP_TRY( hipSetDevice( h->device ) );
    DevCopies dc;
    void* d_key = dc.make( key, sizeof( double ) * n );
    void* d_hist = dc.make( nullptr, sizeof( uint64_t ) * ACN_KEY_HIST_WORDS );
    if( !d_key || !d_hist ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    int st = acn_key_histogram_dev( h, d_key, n, d_hist, nullptr );
    if( st != ACN_OK ) return st;
    HIP_TRY( hipMemcpy( out_hist, d_hist, sizeof( uint64_t ) * ACN_KEY_HIST_WORDS, hipMemcpyDeviceToHost ) );
    return ACN_OK;
}

extern "C" double acn_key_hist_edge( uint32_t bin ) { return acn_select_hist_edge( bin ); }
extern "C" double acn_key_hist_threshold( const uint64_t* hist, uint64_t budget ) { return acn_select_hist_threshold( hist, budget ); }

extern "C" int acn_last_kernel_ms( acn_scene_handle* h, double* trace_ms )
{
    if( !h || !trace_ms || !h->timed ) return fail( ACN_ERR_ARG, "no timed launch" );
    HIP_TRY( hipSetDevice( h->device ) );
    HIP_TRY( hipEventSynchronize( h->ev1 ) );
    float ms = 0;
    HIP_TRY( hipEventElapsedTime( &ms, h->ev0, h->ev1 ) );
    *trace_ms = ms;
    return ACN_OK;
}

extern "C" int acn_last_stage_ms( acn_scene_handle* h, double* out, int n )
{
    if( !h || !out || n < 0 || n > 25 || !h->timed ) return fail( ACN_ERR_ARG, "no timed launch" );
    HIP_TRY( hipSetDevice( h->device ) );
    HIP_TRY( hipEventSynchronize( h->ev1 ) );
    double ms[ 4 ] = { 0, 0, 0, 0 };
    size_t queue_cap = h->ws.cap[ WQ_HARD_SHADOW ], ws_bytes = h->ws.bytes, ws_allocs = h->ws.allocs;
    std::vector< const acn_scene_handle* > src{ h };
    if( h->used_lanes ) { src.assign( h->lanes.begin(), h->lanes.begin() + h->lanes_used ); queue_cap = 0; ws_bytes = 0; ws_allocs = 0; }   /* stage times: summed over the concurrent lanes of the call */
    for( const acn_scene_handle* l : src )
    {
        if( h->used_lanes ) { queue_cap += l->ws.cap[ WQ_HARD_SHADOW ]; ws_bytes += l->ws.bytes; ws_allocs += l->ws.allocs; }
        for( size_t i = 0; i < l->events_used; i++ )
        {
            float t = 0;
            HIP_TRY( hipEventElapsedTime( &t, l->events[ i ].a, l->events[ i ].b ) );
            ms[ l->events[ i ].stage ] += t;
        }
    }
    float total = 0;
    HIP_TRY( hipEventElapsedTime( &total, h->ev0, h->ev1 ) );
    double v[ 25 ] = { ms[ 0 ], ms[ 1 ], ms[ 2 ], total, ( double )h->launches[ 0 ], ( double )h->launches[ 1 ], ( double )h->launches[ 2 ],
                       ( double )h->chunks, ( double )h->retries, ( double )h->levels, ( double )h->peak_tasks, ( double )h->peak_children,
                       ( double )queue_cap, ms[ 3 ], ( double )h->launches[ 3 ], ( double )h->hard_rays,
                       ( double )h->walk_rays, ( double )h->shade_hit_recs, ( double )h->host_syncs, ( double )h->walk_steps,
                       ( double )h->flags_seen, ( double )h->private_rays, ( double )h->probe_rays, ( double )ws_bytes, ( double )ws_allocs };
    for( int k = 0; k < n && k < 25; k++ ) out[ k ] = v[ k ];
    return ACN_OK;
}

extern "C" int acn_last_counters( acn_scene_handle* h, uint64_t* out, int n )
{
    if( !h || !out || n < 0 || n > ACN_CNT_SLOTS ) return fail( ACN_ERR_ARG, "bad argument" );
    HIP_TRY( hipSetDevice( h->device ) );
    unsigned long long c[ ACN_CNT_SLOTS ], sum[ ACN_CNT_SLOTS ];
    for( int k = 0; k < ACN_CNT_SLOTS; k++ ) sum[ k ] = 0;
    std::vector< const acn_scene_handle* > src{ h };
    if( h->used_lanes ) src.assign( h->lanes.begin(), h->lanes.begin() + h->lanes_used );
    for( const acn_scene_handle* l : src )
    {
        HIP_TRY( hipMemcpy( c, l->d_counters, sizeof( c ), hipMemcpyDeviceToHost ) );
        for( int k = 0; k < ACN_CNT_SLOTS; k++ ) sum[ k ] += c[ k ];
    }
    for( int k = 0; k < n; k++ ) out[ k ] = k < ACN_CNT_SLOTS ? sum[ k ] : 0;
    return ACN_OK;
}

extern "C" int acn_estimate_envelope( acn_scene_handle* h, int32_t node, uint64_t samples, uint32_t rseed,
                                      double radius_factor, double* out )
{
    if( !h || !out || node < 0 || ( uint32_t )node >= h->dev.n_nodes ) return fail( ACN_ERR_ARG, "bad argument" );
    HIP_TRY( hipSetDevice( h->device ) );
    V3* d_scratch = nullptr; double* d_out = nullptr;
    HIP_TRY( hipMalloc( &d_scratch, sizeof( V3 ) * ( samples ? samples : 1 ) ) );
    HIP_TRY( hipMalloc( &d_out, sizeof( double ) * 4 ) );
    DevScene est_scene = h->dev;
    est_scene.lds_stack = ACN_NO_LDS_STACK;   /* one lane, no dynamic LDS: the machine keeps its stacks in scratch */
    hipLaunchKernelGGL( k_estimate_envelope, dim3( 1 ), dim3( 1 ), 0, h->stream, est_scene, node, samples, rseed, radius_factor, d_scratch, d_out );
    hipError_t e = hipGetLastError();
    if( e == hipSuccess ) e = hipStreamSynchronize( h->stream );
    if( e == hipSuccess ) e = hipMemcpy( out, d_out, sizeof( double ) * 4, hipMemcpyDeviceToHost );
    hipFree( d_scratch ); hipFree( d_out );
    if( e != hipSuccess ) return fail( ACN_ERR_DEVICE, hipGetErrorString( e ) );
    return ACN_OK;
}

int acn_query_env( acn_scene_handle* h, QueryEnv* q )
{
    if( !h || !q ) return fail( ACN_ERR_ARG, "null argument" );
    HIP_TRY( hipSetDevice( h->device ) );
    q->s = scene_args( h ); q->lds_node_bytes = h->scene.lds_bytes; q->lds_stack_bytes = h->scene.lds_stack_bytes; q->stream = h->stream;
    return ACN_OK;
}
int acn_query_fail( int code, const char* msg ) { return fail( code, msg ); }

extern "C" int acn_detmath_eval( int device, int op, const double* x, const double* y, double* out, size_t n )
{
    if( !x || !out ) return fail( ACN_ERR_ARG, "null argument" );
    if( acn_device_count() <= 0 ) return fail( ACN_ERR_DEVICE, "no HIP device" );
    HIP_TRY( hipSetDevice( device ) );
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    HIP_TRY( hipMalloc( &dx, sizeof( double ) * n ) );
    HIP_TRY( hipMalloc( &dout, sizeof( double ) * n ) );
    HIP_TRY( hipMemcpy( dx, x, sizeof( double ) * n, hipMemcpyHostToDevice ) );
    if( y )
    {
        HIP_TRY( hipMalloc( &dy, sizeof( double ) * n ) );
        HIP_TRY( hipMemcpy( dy, y, sizeof( double ) * n, hipMemcpyHostToDevice ) );
    }
    hipLaunchKernelGGL( k_detmath, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, 0, op, dx, dy, dout, n );
    HIP_TRY( hipGetLastError() );
    HIP_TRY( hipDeviceSynchronize() );
    HIP_TRY( hipMemcpy( out, dout, sizeof( double ) * n, hipMemcpyDeviceToHost ) );
    hipFree( dx ); hipFree( dout ); if( dy ) hipFree( dy );
    return ACN_OK;
}
