/* acn_handle.h -- what the host units of libactinon_hip.so share: the scene handle, the pipeline runner (PipeRun), the error
 * plumbing, the frame of one C ABI call and the few functions that cross between actinon_hip.hip (life cycle, workspace, pipeline, lanes and the pipeline's own
 * entry points), acn_calls.hip (every other entry point) and k_query.hip (the test seam).
 * Ownership: what a handle or a runner holds on the device (memory, events, streams) is a member of an owning type of acn_devbuf.h, a lane
 * or a worker thread a std::unique_ptr: nothing is freed by a list, an early return cannot leak; kernels get plain pointers (.get()). */
#ifndef ACN_HANDLE_H
#define ACN_HANDLE_H

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <functional>
#include <thread>
#include <condition_variable>

#include "acn_launch.h"
#include "acn_tables.h"
#include "acn_chunkplan.h"
#include "acn_queueplan.h"
#include "acn_devbuf.h"
#include "acn_frame_host.h"

/* ------------------------------------------------------------------------------------------------------------------ */
/* error plumbing */
extern thread_local std::string g_last_error;   /* one object, defined in actinon_hip.hip: what acn_last_error() returns */
static inline int fail( int code, const std::string& msg ) { g_last_error = msg; return code; }

#define HIP_TRY( expr ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) \
    return fail( ACN_ERR_DEVICE, std::string( #expr ) + ": " + hipGetErrorString( e_ ) ); } while( 0 )

/* The HIP policies of acn_devbuf.h: device memory, pinned host memory, events, streams.  alloc returns the hipError_t (0: done) and
 * leaves a failure worded for acn_last_error(), so `if( buf.grow( bytes ) ) return ACN_ERR_DEVICE;` is a whole call site. */
static inline int alloc_status( hipError_t e, const char* call ) { if( e != hipSuccess ) fail( ACN_ERR_DEVICE, std::string( call ) + ": " + hipGetErrorString( e ) ); return ( int )e; }
struct HipDevice { static int alloc( void** p, size_t want ) { return alloc_status( hipMalloc( p, want ), "hipMalloc( p, want )" ); }
                   static void release( void* p ) { hipFree( p ); } };   /* (hipFree waits for whatever still reads the block) */
struct HipPinned { static int alloc( void** p, size_t want ) { return alloc_status( hipHostMalloc( p, want ), "hipHostMalloc( p, want )" ); }
                   static void release( void* p ) { hipHostFree( p ); } };
struct HipEventDel { static void destroy( hipEvent_t e ) { hipEventDestroy( e ); } };
struct HipStreamDel { static void destroy( hipStream_t s ) { hipStreamDestroy( s ); } };
template< class T > using DevBuf = Buf< T, HipDevice >;
using Event = Owned< hipEvent_t, HipEventDel >;
using Stream = Owned< hipStream_t, HipStreamDel >;

struct StageEvents { Event a, b; int stage = 0; };

/* a persistent host thread per lane (creating a thread per call costs a HIP per-thread initialisation each time) */
struct LaneWorker
{
    std::thread thread;
    std::mutex m;
    std::condition_variable cv;
    std::function< void() > job;
    bool has_job = false, done = true, quit = false;
    ~LaneWorker() { stop(); }
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
    int      lanes = 0;                /* ACN_LANES: concurrent pipeline runs of a large call, as the host gave it ... */
    bool     lanes_given = false;      /* ... if it gave one.  The count and the lanes' grids a handle uses: acn_lane_plan (acn_queueplan.h) */
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
    size_t   frame_slice = ACN_FRAME_SLICE;         /* ACN_FRAME_SLICE: positions of one slice of a frame pass (acn_frame_*), whole pixels, at least one */
    uint32_t frame_foreign_slots = ACN_FRAME_FOREIGN_SLOTS;   /* ACN_FRAME_FOREIGN_SLOTS: foreign entries acn_frame_push lists, at most 1024; more are found by one lane's walk */
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
        if( const char* e = getenv( "ACN_LANES" ) ) { lanes = atoi( e ); lanes_given = true; }
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
        if( const char* e = getenv( "ACN_FRAME_SLICE" ) ) frame_slice = ( size_t )atoll( e );
        if( frame_slice < 1 || frame_slice > ACN_FRAME_SLICE ) frame_slice = ACN_FRAME_SLICE;
        if( const char* e = getenv( "ACN_FRAME_FOREIGN_SLOTS" ) ) frame_foreign_slots = ( uint32_t )atoll( e );
        if( frame_foreign_slots > ACN_FRAME_FOREIGN_SLOTS ) frame_foreign_slots = ACN_FRAME_FOREIGN_SLOTS;
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
        if( stack_cap < 256 ) stack_cap = 256;
        if( stack_use == 0 || stack_use > stack_cap ) stack_use = stack_cap;
    }
};

/* the queue workspace of one pipeline run (WQ_*: acn_queueplan.h) */
struct Workspace
{
    DevBuf< DTask >      tasks;
    DevBuf< uint32_t >   idx[ ACN_NCLASS ];
    DevBuf< HitRec >     children;
    DevBuf< HardShadow > hard_shadow;
    DevBuf< HardPath >   hard_path;
    DevBuf< RayTask >    rays[ 2 ];
    DevBuf< RayTask >    stacks;   size_t stack_waves = 0;
    uint32_t    cap[ WQ_N ] = {};  /* records per queue, WQ_* */
    size_t      bytes = 0;          /* device memory of the queues and stacks */
    uint64_t    allocs = 0;         /* times this workspace was (re)allocated */
    bool        trimmed = false;    /* it was already re-allocated smaller once */
    uint32_t    sized_calls = 0;    /* calls of ensure_workspace with learned rates (the trim window: acn_keep_caps) */
    /* The queues and stacks go back to the device; cap, bytes and stack_waves are zero.  The bookkeeping: trimmed and sized_calls start
     * over with EVERY release, also the one ensure_workspace makes to allocate anew (it sets trimmed again when it is done).  allocs
     * survives only there (keep_allocs): a runner that gives its queues back to the handle's bound (render_dispatch, render_lanes) counts from zero. */
    void release( bool keep_allocs = false )
    {
        tasks.reset(); for( auto& b : idx ) b.reset();
        children.reset(); hard_shadow.reset(); hard_path.reset(); for( auto& b : rays ) b.reset();
        stacks.reset(); stack_waves = 0; bytes = 0; for( uint32_t& c : cap ) c = 0;
        trimmed = false; sized_calls = 0; if( !keep_allocs ) allocs = 0;
    }
};

/* the statistics of one call (acn_last_stage_ms) */
struct RunStats
{
    uint64_t launches[ 4 ] = { 0, 0, 0, 0 };   /* walk, shade, finalize, hard-ray kernels */
    uint64_t hard_rays = 0, walk_steps = 0, walk_rays = 0, shade_hit_recs = 0, host_syncs = 0, private_rays = 0, probe_rays = 0;
    uint32_t flags_seen = 0;                   /* ACN_FLAG_* bits of the last call */
    uint64_t chunks = 0, retries = 0, levels = 0;
    uint64_t peak_tasks = 0, peak_children = 0;
    void reset() { *this = RunStats(); }
    /* a chunk's that fitted into its run's (acn_read_chunk): sums, the peaks' maxima */
    void take( const acn_chunk_report& c )
    {
        levels += c.levels; walk_rays += c.walk_rays; walk_steps += c.walk_steps; hard_rays += c.hard_rays; shade_hit_recs += c.shade_hit_recs;
        private_rays += c.private_rays; probe_rays += c.probe_rays;
        if( c.peak_tasks > peak_tasks ) peak_tasks = c.peak_tasks;
        if( c.peak_children > peak_children ) peak_children = c.peak_children;
    }
    /* a lane's into its call's: sums, but the flags' union and the deepest level (the peaks of concurrent lanes add up) */
    void add( const RunStats& l )
    {
        for( int i = 0; i < 4; i++ ) launches[ i ] += l.launches[ i ];
        hard_rays += l.hard_rays; walk_steps += l.walk_steps; walk_rays += l.walk_rays; shade_hit_recs += l.shade_hit_recs;
        host_syncs += l.host_syncs; flags_seen |= l.flags_seen; private_rays += l.private_rays; probe_rays += l.probe_rays;
        chunks += l.chunks; retries += l.retries;
        if( l.levels > levels ) levels = l.levels;
        peak_tasks += l.peak_tasks; peak_children += l.peak_children;
    }
};

/* what a pipeline run has learned about the scene; it stays with the run for its next call */
struct Learned
{
    double rate[ WQ_N ] = {};                  /* records per sample position a chunk leaves in each queue (WQ_*); 0: not known yet */
    uint32_t rate_cnt = 0;                     /* positions of the chunk the rates were taken from */
    acn_chunk_ctl ctl = { 0.7, 0, 0 };         /* acn_chunkplan.h.  fill_target: fraction of its capacity the fullest queue of a chunk is
                                                  planned to reach: lowered by every overflow (a redone chunk is lost work), raised slowly
                                                  by chunks that fit */
    uint32_t walk_passes_seen[ ACN_LEVEL_BLOCKS ] = {};   /* passes of a level that had input in the last chunk (0: not known yet) */
    bool known() const { return acn_rates_known( rate ) != 0; }
    void forget_passes() { for( uint32_t& seen : walk_passes_seen ) seen = 0; }   /* the full number of passes again */
    /* what one arrangement (the handle's own run, its lanes) learned about the scene (records per position) holds for the
     * other: only if `to` knows nothing and `from` does; the walk passes start over */
    static void inherit( Learned* to, const Learned& from )
    {
        if( to->known() || !from.known() ) return;
        for( int q = 0; q < WQ_N; q++ ) to->rate[ q ] = from.rate[ q ];
        to->rate_cnt = from.rate_cnt; to->ctl.fill_target = from.ctl.fill_target;
        to->forget_passes();
    }
};

/* the per-call switches of a pipeline run */
struct Switches
{
    bool count_work = false;                   /* ACN_OPT_COUNT_WORK */
    bool stage_timing = false;                 /* ACN_OPT_STAGE_TIMING */
    uint32_t shard_rank = 0, shard_world = 1;  /* ACN_SHARD_SAMPLES */
    bool seeded = false;                       /* the call renders the caller's rays (Primary): its ray queue has a known demand (acn_queue_demand) */
};

struct acn_scene_handle;

/* A device-resident frame (include/actinon_hip.h, acn_frame_*; the entry points: acn_calls.hip): owned by its handle */
struct acn_frame
{
    acn_scene_handle* h = nullptr;
    uint64_t width = 0, height = 0;
    DevBuf< double > d_acc;                    /* [ height * width ][ 6 ]: the layout of acn_lum */
    DevBuf< double > d_key;                    /* [ height * width ] */
    DevBuf< long long > d_index;               /* the flagged pixels of a gradient plan, ascending */
    DevBuf< double > d_pos, d_clr;             /* the entries of the plan: [ flagged * samples ][ 2 ], [ . ][ 3 ] */
    DevBuf< unsigned long long > d_foreign;    /* push: the number of foreign entries, then ACN_FRAME_FOREIGN_SLOTS of them */
    DevBuf< void > d_image;                    /* acn_frame_image: rgb f64, then rgb8 */
    bool planned = false, centres = false;     /* a plan no push has consumed; ... of the main pass: no index list */
    uint64_t flagged = 0, samples = 0;         /* of that plan */
};

/* One pipeline runner: what launch_render needs to work a call off on one stream.  A handle has its own, for a call that runs
 * alone, and one per concurrent lane (render_lanes); all of them read the scene, the tunables and the budget of the handle. */
struct PipeRun
{
    const acn_scene_handle* h = nullptr;       /* the handle it serves (a lane: from bind_lane on) */
    DevScene dev{};                            /* the handle's, with flags -> the run's own counter block */
    Stream stream;
    Event ev0, ev1;
    unsigned grid = 1024, shade_grid = 1024;   /* workgroups of the persistent kernels / of k_shade */
    unsigned walk_grid = 1024;                 /* ... of k_walk */
    Workspace ws;
    DevBuf< uint32_t > d_counts;               /* ACN_LEVEL_BLOCKS counter blocks of QC_N words (acn_counts.h) */
    Buf< uint32_t, HipPinned > h_counts;       /* pinned copy */
    DevBuf< unsigned long long > d_accum;
    DevBuf< unsigned long long > d_counters;
    DevBuf< unsigned long long > d_counters_keep;   /* the work counters as they were before the current chunk (restored when it is redone) */
    std::vector< StageEvents > events;  size_t events_used = 0;
    int cur_stage = 0;
    size_t budget_div = 1;                     /* workspace budget of a lane = the handle's budget / lanes */
    Switches sw;                               /* of the current call */
    Learned learned;
    uint64_t learn_passes = 0;                 /* learning passes this runner has run (learn_rates); acn_scene_info sums them */
    RunStats stats;                            /* of the last call */
    /* of a lane */
    std::unique_ptr< LaneWorker > worker;
    DevBuf< double > d_lane_in;                /* its gathered positions or rays */
    DevBuf< double > d_lane_out;               /* ... and its results */
    ~PipeRun() { worker.reset(); }             /* the thread is stopped and joined before anything it may touch goes (the members, last to first) */
};

struct acn_scene_handle
{
    int device = 0;
    DevScene dev{};                            /* the template of every run's copy (flags: the own run's) */
    /* the resident scene and what the tables say about it */
    struct Resident
    {
        DevBuf< GNode >   d_nodes;
        DevBuf< GMat >    d_mats;
        DevBuf< int32_t > d_elems;
        DevBuf< acn_texture > d_textures;
        int max_csg_depth = 0;
        size_t lds_bytes = 0;                      /* > 0: the node array fits the LDS staging budget */
        size_t lds_stack_bytes = 0;                /* > 0: the machine kernels keep their CSG stacks in LDS */
        bool prune = false;                        /* some root element has an interval-prune program: launch the PRUNE kernel variants */
        bool leaf_lights = true;                   /* every light element is a plane / sphere */
        uint32_t elem_pos_base = 0;                /* elems[ elem_pos_base + k ]: given-order position of entry k of the cost-ordered copy (k_hard_shadow: resume words) */
        int n_levels = 1;                          /* path levels of the scene's trace_depth */
        size_t n_lights = 1;                       /* elements of the light root */
    } scene;
    DevBuf< SCEntry > d_sc_table;
    DevBuf< double > d_sc_spheres;             /* ( pos, radius ) of the sphere leaves of d_sc_table */
    acn_scene_kind kind{};                     /* of the resident scene: what decides whether a change of scene keeps the learned rates */
    uint64_t replaces = 0, param_sets = 0;     /* acn_scene_replace / acn_scene_set_params calls accepted since the upload */
    Tunables tun;
    unsigned cus = 256;                        /* compute units of the device */
    size_t workspace_budget = 0;               /* bytes this handle's queues may take (all lanes together) */
    acn_lane_plan_t plan = { 1, 0, 0, 0 };     /* lanes of a large call and a lane's grids: acn_lane_plan of the tunables and the device's compute units (acn_scene_upload) */
    PipeRun run;                               /* a call that runs alone; its stream is the handle's own, its statistics the last call's */
    /* concurrent lanes (render_lanes): runners that own a stream, a workspace and a host thread each */
    std::vector< std::unique_ptr< PipeRun > > lanes;
    /* lanes made during acn_scene_upload on a helper thread (early_lanes_begin), taken over before the upload returns (quiesce) */
    std::thread early_maker;
    std::vector< std::unique_ptr< PipeRun > > early_made;
    bool timed = false;
    bool used_lanes = false;                   /* the last render call ran through the lanes: statistics are their sums */
    int  lanes_used = 0;                       /* ... the first lanes_used of them */
    bool one_lane = false;                     /* the last call would have used lanes but did not fit the workspace bound that way */
    /* scratch of the entry points that are not the pipeline's */
    DevBuf< double > d_shard_pos;                   /* acn_render_main_pass_shard_dev: the rank's positions */
    DevBuf< unsigned long long > d_ray_check;       /* acn_render_rays_dev: the lowest index of a refused ray */
    DevBuf< uint32_t > d_surface_flags;             /* acn_surface_*: the ACN_FLAG_* word of the surface kernels (not the pipeline's) */
    DevBuf< void > d_denoise;                       /* acn_denoise*, acn_denoise_layers*: guides and colour buffers, apart from the render workspace */
    DevBuf< double > d_lens_rays;                   /* the slice buffers of the lens driver (lens_slices, acn_calls.hip): the rays [ 6 ] of a slice, */
    DevBuf< double > d_lens_rad;                    /* ... their radiance [ 3 ], grown by the calls that render, */
    DevBuf< double > d_lens_surf;                   /* ... and their surface records [ 16 ], grown by the calls that take records */
    DevBuf< unsigned long long > d_select_tiles;    /* acn_select_above*: the counts per tile and their total */
    unsigned long long stage_counters[ CNT_N + 2 ] = {};   /* acn_stage_last_counters: the last stage call's (zero without ACN_STAGE_COUNT_WORK) */
    std::vector< std::unique_ptr< acn_frame > > frames;   /* acn_frame_create: what acn_frame_free has not released goes with the handle */
};

static SceneArgs scene_args( const DevScene& dev, const acn_scene_handle::Resident& r )
{
    SceneArgs s;
    s.dev = dev; s.nodes = r.d_nodes.get(); s.mats = r.d_mats.get(); s.elems = r.d_elems.get(); s.textures = r.d_textures.get(); s.elem_pos_base = r.elem_pos_base;
    return s;
}
static size_t machine_lds_bytes( const acn_scene_handle::Resident& r ) { return r.lds_bytes + r.lds_stack_bytes; }

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

/* one pipeline run on the handle itself, or the concurrent lanes (actinon_hip.hip).  opts: never null */
int render_dispatch( acn_scene_handle* h, const Primary& prim, size_t n, double* d_out_rgb, const acn_render_opts* opts, hipStream_t stream );

/* ------------------------------------------------------------------------------------------------------------------ */
/* The frame of one C ABI call.  The options are viewed when the frame is made, so every argument check reads them before the
 * device is touched; call_begin sets the device and picks the stream, call_end synchronises the stream iff it is the handle's own.
 * A host-buffer form (HostCall, below) sets opts.stream = nullptr before it hands the frame (or its opts) on: it is synchronous. */
struct Call
{
    acn_render_opts opts;           /* the caller's options as opts_of views them: there is no null to test for */
    hipStream_t stream = nullptr;   /* opts.stream, or the handle's own */
    bool own = true;                /* ... the handle's own */
    explicit Call( const acn_render_opts* in ) : opts( opts_of( in ) ) {}
};
static inline int call_begin( acn_scene_handle* h, Call* c )
{
    HIP_TRY( hipSetDevice( h->device ) );
    c->own = c->opts.stream == nullptr;
    c->stream = c->own ? h->run.stream.get() : ( hipStream_t )c->opts.stream;
    return ACN_OK;
}
static inline int call_end( const Call& c )
{
    if( c.own ) HIP_TRY( hipStreamSynchronize( c.stream ) );
    return ACN_OK;
}

/* every ray of a call is checked before anything is rendered or written: the lowest index of a refused one, one word read back
 * (this synchronises `stream`, a caller's too) */
static inline int check_rays( acn_scene_handle* h, const double* d_rays, size_t n, hipStream_t stream )
{
    if( h->d_ray_check.grow( sizeof( unsigned long long ) ) ) return ACN_ERR_DEVICE;
    HIP_TRY( hipMemsetAsync( h->d_ray_check.get(), 0xFF, sizeof( unsigned long long ), stream ) );
    acn_launch_check_rays( d_rays, n, h->d_ray_check.get(), stream );
    HIP_TRY( hipGetLastError() );
    unsigned long long bad = 0;
    HIP_TRY( hipMemcpyAsync( &bad, h->d_ray_check.get(), sizeof( bad ), hipMemcpyDeviceToHost, stream ) );
    HIP_TRY( hipStreamSynchronize( stream ) );
    if( bad < n ) return fail( ACN_ERR_ARG, "ray " + std::to_string( bad ) + ": a component is not finite or the direction has no length" );
    return ACN_OK;
}

/* pixels [ first, first + count ) of a main pass lie in the scene's raster (first + count may not wrap either) */
static inline int pixel_range_check( const acn_scene_handle* h, size_t first, size_t count )
{
    const size_t pixels = h->dev.prm.image_width * h->dev.prm.image_height;
    if( first > pixels || count > pixels - first ) return fail( ACN_ERR_ARG, "pixel range outside the image" );
    return ACN_OK;
}

/* device copies of host arrays for one call; everything is freed when it goes */
struct DevCopies
{
    std::vector< DevBuf< void > > held;
    /* null on failure; src (nullable) is copied in */
    void* make( const void* src, size_t bytes )
    {
        DevBuf< void > b;
        if( b.grow( bytes ? bytes : 1 ) ) return nullptr;
        void* d = b.get();
        held.push_back( std::move( b ) );
        if( src && bytes && hipMemcpy( d, src, bytes, hipMemcpyHostToDevice ) != hipSuccess ) return nullptr;
        return d;
    }
    /* a result back to the host, after the call has synchronised */
    static int fetch( void* dst, const void* d, size_t bytes )
    {
        HIP_TRY( hipMemcpy( dst, d, bytes, hipMemcpyDeviceToHost ) );
        return ACN_OK;
    }
};

/* The host-buffer form of a call: after its checks an entry point declares its arrays here, takes the device pointers and runs its
 * device-buffer form on the handle's own stream (opts.stream = nullptr: synchronous).  The device is set before the first allocation; a
 * buffer that cannot be made fails the form once, before anything is launched; the outputs come back in declaration order, after ACN_OK */
struct HostCall
{
    struct Out { void* dst; const void* d; size_t bytes; };
    DevCopies dc;
    std::vector< Out > outs;
    int st;
    explicit HostCall( const acn_scene_handle* h ) : st( [ h ]() -> int { HIP_TRY( hipSetDevice( h->device ) ); return ACN_OK; }() ) {}
    /* a buffer that src (nullable) is copied into and dst (nullable) takes the content of; in and out are the two halves */
    void* inout( const void* src, void* dst, size_t bytes )
    {
        void* d = st == ACN_OK ? dc.make( src, bytes ) : nullptr;
        if( d && dst ) outs.push_back( { dst, d, bytes } );
        if( !d && st == ACN_OK ) st = fail( ACN_ERR_DEVICE, "device buffers of a host call" );
        return d;
    }
    void* in( const void* src, size_t bytes ) { return inout( src, nullptr, bytes ); }
    void* out( void* dst, size_t bytes ) { return dst ? inout( nullptr, dst, bytes ) : nullptr; }   /* a null dst: nothing made, nothing fetched */
    template< class DevCall > int run( DevCall dev )
    {
        if( st != ACN_OK || ( st = dev() ) != ACN_OK ) return st;
        for( const Out& o : outs ) if( ( st = DevCopies::fetch( o.dst, o.d, o.bytes ) ) != ACN_OK ) return st;
        return ACN_OK;
    }
};

/* the plainest of them: one array copied in, the device-buffer call `dev( d_in, d_out )`, one array copied out */
template< class DevCall >
static int host_in_out( acn_scene_handle* h, const void* in, size_t in_bytes, void* out, size_t out_bytes, DevCall dev )
{
    HostCall hc( h );
    void* d_in = hc.in( in, in_bytes );
    void* d_out = hc.out( out, out_bytes );
    return hc.run( [ & ] { return dev( d_in, d_out ); } );
}

#endif
