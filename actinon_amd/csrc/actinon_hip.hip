/* actinon_hip.hip -- libactinon_hip.so (gfx950 only): the handle's life cycle, the workspace, the wavefront pipeline with its concurrent
 * lanes, and the entry points of include/actinon_hip.h that are the pipeline's own.  Every other entry point: acn_calls.hip. */
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstddef>
#include <algorithm>

#include "acn_device.h"   /* a ray unit: the whole tracer */
#include "acn_handle.h"   /* (and the standard headers its types need) */

/* ------------------------------------------------------------------------------------------------------------------ */
/* error plumbing (fail and HIP_TRY: acn_handle.h) */
thread_local std::string g_last_error;
extern "C" const char* acn_last_error( void ) { return g_last_error.c_str(); }

/* bytes per record of each queue (WQ_*) */
static const size_t wq_bytes[ WQ_N ] = { sizeof( DTask ) + ACN_NCLASS * sizeof( uint32_t ), sizeof( HitRec ), sizeof( HardShadow ), sizeof( HardPath ), 2 * sizeof( RayTask ) };

/* ------------------------------------------------------------------------------------------------------------------ */
/* kernels */

/* camera basis with the oracle's expressions (scene.c:963-973), one lane */
__global__ void k_camera_setup( DevScene sc, M3* out_rot, double* out_unit_f )
{
    uint64_t unit_sz = ( sc.prm.image_height >> 1 );
    *out_unit_f = 1.0 / unit_sz;
    *out_rot = camera_rotation_of( sc.prm );
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

/* ------------------------------------------------------------------------------------------------------------------ */
/* ABI */
extern "C" int acn_device_count( void )
{
    int n = 0;
    if( hipGetDeviceCount( &n ) != hipSuccess ) return 0;
    return n;
}

static int lane_objects( int device, bool debug, std::unique_ptr< PipeRun >* out );

/* What every runner has beside its stream, which the caller has made: two events, the counter blocks, their pinned copy, and the blocks the
 * kernels add to zeroed -- synchronously for the handle's own run, on its stream for a lane (where everything that uses them follows; the
 * null stream would wait for the caller's).  mark( i ): the events (0), the blocks and memsets (1), the pinned block (2) are done. */
template< class Mark >
static hipError_t run_objects( PipeRun* r, bool on_stream, Mark mark )
{
    const size_t counters = sizeof( unsigned long long ) * ACN_CNT_SLOTS, counts = sizeof( uint32_t ) * QC_N * ACN_LEVEL_BLOCKS;
    hipError_t e = hipEventCreate( r->ev0.put() );
    if( e == hipSuccess ) e = hipEventCreate( r->ev1.put() );
    mark( 0 );
    for( auto* b : { &r->d_counters, &r->d_counters_keep } ) if( e == hipSuccess ) e = ( hipError_t )b->grow( counters );
    if( e == hipSuccess ) e = ( hipError_t )r->d_counts.grow( counts );
    if( e == hipSuccess ) e = on_stream ? hipMemsetAsync( r->d_counters.get(), 0, counters, r->stream.get() ) : hipMemset( r->d_counters.get(), 0, counters );
    if( e == hipSuccess ) e = on_stream ? hipMemsetAsync( r->d_counts.get(), 0, counts, r->stream.get() ) : hipMemset( r->d_counts.get(), 0, counts );
    mark( 1 );
    if( e == hipSuccess ) e = ( hipError_t )r->h_counts.grow( counts );
    mark( 2 );
    return e;
}

/* Lanes made during the upload.  A stream that gets its own hardware queue costs ~10 ms of host time, and making one while kernels
 * run stretches those kernels too (the learning pass of a cold handle: 19 ms alone, 56 - 150 ms beside six streams being made,
 * profiles/r04/upload_timeline_s41.txt) -- so the lanes a whole frame of the scene's own raster will use are made here, on a helper
 * thread beside the upload's host work and copies, while nothing of this handle runs on the device (ACN_EARLY_LANES=1; off by
 * default: the runtime makes streams one after the other, so the time only moves from the first call into the upload).  A handle that would render its
 * raster on one lane (small rasters, path_samples >= 256 on a cold handle: render_positions) makes none.  Failures are not reported
 * from here: the first call that needs the lanes makes what is missing and reports its own.  The thread is joined and its lanes
 * become the handle's before the upload's first kernel (quiesce). */
static void early_lanes_begin( acn_scene_handle* h, size_t n, uint64_t path_samples )
{
    const int lanes = acn_lanes_for_counts( h->plan.lanes, n, path_samples );
    if( lanes <= 1 || path_samples >= 256 ) return;
    const int device = h->device; const bool debug = h->tun.debug_chunks;
    h->early_maker = std::thread( [ h, lanes, device, debug ]()
    {
        for( int k = 0; k < lanes; k++ )
        {
            std::unique_ptr< PipeRun > l;
            if( lane_objects( device, debug, &l ) != ACN_OK ) break;
            h->early_made.push_back( std::move( l ) );
        }
    } );
}
static void early_lanes_join( acn_scene_handle* h ) { if( h->early_maker.joinable() ) h->early_maker.join(); }

/* ------------------------------------------------------------------------------------------------------------------ */
/* The resident scene: made by acn_scene_upload, changed by acn_scene_replace and acn_scene_set_params through the same steps.  What
 * can refuse a change -- the checks, the device blocks of the new scene, the camera kernel -- comes BEFORE the handle is touched: a
 * change that fails leaves the handle rendering what it rendered. */
static void bind_lane( const acn_scene_handle* h, int lanes, PipeRun* l );

/* the device blocks of a scene, fresh ones: the handle's own stay valid until they are exchanged */
struct StagedScene
{
    acn_scene_handle::Resident scene;
    DevBuf< SCEntry > d_sc_table;
    DevBuf< double > d_sc_spheres;
};
static int stage_scene( const acn_flat_scene* scene, int max_csg, const acn_scene_tables& t, StagedScene* s )
{
    acn_scene_handle::Resident& r = s->scene;
    r.max_csg_depth = max_csg;
    r.lds_bytes = t.lds_bytes; r.lds_stack_bytes = t.lds_stack_bytes;
    r.prune = t.prune; r.leaf_lights = t.leaf_lights; r.elem_pos_base = t.elem_pos_base;
    r.n_levels = t.n_levels; r.n_lights = t.n_lights;
    const size_t n_tex = scene->n_textures ? scene->n_textures : 1, n_sc = t.sc_table.size() ? t.sc_table.size() : 1, n_sph = t.sc_spheres.size() ? t.sc_spheres.size() : 4;
    if( r.d_nodes.grow( sizeof( GNode ) * t.nodes.size() ) || r.d_mats.grow( sizeof( GMat ) * t.mats.size() ) || r.d_elems.grow( sizeof( int32_t ) * t.elems.size() ) ) return ACN_ERR_DEVICE;
    if( s->d_sc_table.grow( sizeof( SCEntry ) * n_sc ) ) return ACN_ERR_DEVICE;
    if( t.sc_table.size() ) HIP_TRY( hipMemcpy( s->d_sc_table.get(), t.sc_table.data(), sizeof( SCEntry ) * t.sc_table.size(), hipMemcpyHostToDevice ) );
    if( s->d_sc_spheres.grow( sizeof( double ) * n_sph ) ) return ACN_ERR_DEVICE;
    if( t.sc_spheres.size() ) HIP_TRY( hipMemcpy( s->d_sc_spheres.get(), t.sc_spheres.data(), sizeof( double ) * t.sc_spheres.size(), hipMemcpyHostToDevice ) );
    if( r.d_textures.grow( sizeof( acn_texture ) * n_tex ) ) return ACN_ERR_DEVICE;
    if( scene->n_textures ) HIP_TRY( hipMemcpy( r.d_textures.get(), scene->textures, sizeof( acn_texture ) * scene->n_textures, hipMemcpyHostToDevice ) );
    HIP_TRY( hipMemcpy( r.d_nodes.get(), t.nodes.data(), r.d_nodes.bytes(), hipMemcpyHostToDevice ) );
    HIP_TRY( hipMemcpy( r.d_mats.get(), t.mats.data(), r.d_mats.bytes(), hipMemcpyHostToDevice ) );
    HIP_TRY( hipMemcpy( r.d_elems.get(), t.elems.data(), r.d_elems.bytes(), hipMemcpyHostToDevice ) );
    return ACN_OK;
}

/* Nothing of the handle runs: the helper thread of the upload is joined and the lanes it made are the handle's (budget_div: set by the
 * call that runs on them), the handle's own stream and every lane's are idle.  What callers queued on streams of their own is
 * theirs to wait for (include/actinon_hip.h). */
static int quiesce( acn_scene_handle* h )
{
    early_lanes_join( h );
    for( auto& l : h->early_made ) { bind_lane( h, 1, l.get() ); h->lanes.push_back( std::move( l ) ); }
    h->early_made.clear();
    HIP_TRY( hipStreamSynchronize( h->run.stream.get() ) );
    for( auto& l : h->lanes ) HIP_TRY( hipStreamSynchronize( l->stream.get() ) );
    return ACN_OK;
}

/* camera basis on the device so that it shares the device's arithmetic (the kernel reads the parameters alone) */
static int camera_basis( acn_scene_handle* h, const acn_params& prm, M3* rot, double* unit_f )
{
    DevBuf< M3 > d_rot; DevBuf< double > d_uf;
    if( d_rot.grow( sizeof( M3 ) ) || d_uf.grow( sizeof( double ) ) ) return ACN_ERR_DEVICE;
    DevScene sc = h->dev;
    sc.prm = prm;
    hipLaunchKernelGGL( k_camera_setup, dim3( 1 ), dim3( 1 ), 0, h->run.stream.get(), sc, d_rot.get(), d_uf.get() );
    HIP_TRY( hipGetLastError() );
    HIP_TRY( hipStreamSynchronize( h->run.stream.get() ) );
    HIP_TRY( hipMemcpy( rot, d_rot.get(), sizeof( M3 ), hipMemcpyDeviceToHost ) );
    HIP_TRY( hipMemcpy( unit_f, d_uf.get(), sizeof( double ), hipMemcpyDeviceToHost ) );
    return ACN_OK;
}

static void commit_params( acn_scene_handle* h, const acn_params& prm, int n_levels, const M3& rot, double unit_f )
{
    h->dev.prm = prm;
    h->dev.camera_rotation = rot; h->dev.unit_f = unit_f;
    h->scene.n_levels = n_levels;
}

/* a runner's copy of the handle's DevScene; the flags word stays the runner's own */
static void refresh_run( const acn_scene_handle* h, PipeRun* r )
{
    r->dev = h->dev;
    r->dev.flags = r->d_counts.get() + QC_FLAGS;
}

/* After h->dev and h->scene have changed: every runner sees the new scene, the statistics of the last call are gone, and what the
 * runners learned stays iff the scene is of the kind it was (acn_replace_keeps_learned) and the caller does not ask to forget.  Else the
 * next call learns as a cold handle does, on the lanes and the queues that exist (capacities without rates: ensure_workspace keeps
 * queues that hold the starter set, and the trim window of acn_keep_caps opens again with the new rates). */
static void settle( acn_scene_handle* h, bool forget )
{
    acn_scene_kind now;
    now.n_nodes = h->dev.n_nodes; now.n_elems = h->dev.n_elems; now.n_lights = h->scene.n_lights;
    now.n_levels = h->scene.n_levels; now.prune = h->scene.prune ? 1 : 0;
    now.path_samples = h->dev.prm.path_samples; now.direct_samples = h->dev.prm.direct_samples; now.trace_depth = h->dev.prm.trace_depth;
    now.trace_min_intensity = h->dev.prm.trace_min_intensity;
    const bool keep = !forget && acn_replace_keeps_learned( &h->kind, &now );
    h->kind = now;
    auto each = [ & ]( PipeRun* r )
    {
        refresh_run( h, r );
        r->stats.reset();
        if( !keep ) { r->learned = Learned(); r->ws.trimmed = false; r->ws.sized_calls = 0; }
    };
    each( &h->run );
    for( auto& l : h->lanes ) each( l.get() );
    h->timed = false; h->used_lanes = false; h->lanes_used = 0; h->one_lane = false;
}

/* `scene`, which acn_tables_validate accepted, becomes the resident scene of h.  mark( i ): the tables are built (0), the device blocks
 * are staged (1), nothing of the handle runs (2). */
template< class Mark >
static int install_scene( acn_scene_handle* h, const acn_flat_scene* scene, int max_csg, bool forget, Mark mark )
{
    acn_scene_tables t;   /* everything the traversal shortcuts read, built on the host alone (acn_tables.cpp) */
    acn_tables_build( scene, h->tun.tables, &t );
    mark( 0 );
    StagedScene s;
    int st = stage_scene( scene, max_csg, t, &s );
    if( st != ACN_OK ) return st;
    mark( 1 );
    if( ( st = quiesce( h ) ) != ACN_OK ) return st;   /* before the first kernel: nothing of this handle runs while hardware queues are being made */
    mark( 2 );
    M3 rot; double unit_f = 0;
    if( ( st = camera_basis( h, scene->params, &rot, &unit_f ) ) != ACN_OK ) return st;
    /* from here on nothing fails.  The blocks of the scene before go back to the device as these are moved in. */
    h->scene = std::move( s.scene );
    h->d_sc_table = std::move( s.d_sc_table );
    h->d_sc_spheres = std::move( s.d_sc_spheres );
    const acn_scene_handle::Resident& r = h->scene;
    h->dev.nodes = ( NodeP )r.d_nodes.get(); h->dev.gnodes = ( NodeP )r.d_nodes.get();
    h->dev.mats = ( MatP )r.d_mats.get();
    h->dev.elems = ( ElemP )r.d_elems.get();
    h->dev.textures = ( TexP )r.d_textures.get();
    h->dev.sc_table = h->d_sc_table.get();
    h->dev.sc_spheres = h->d_sc_spheres.get();
    h->dev.prune_base = t.prune_base;
    h->dev.light_root = scene->light_root;
    h->dev.matter_root = scene->matter_root;
    h->dev.n_nodes = scene->n_nodes;
    h->dev.n_elems = scene->n_elems;
    h->dev.lds_stack = r.lds_stack_bytes ? 0u : ACN_NO_LDS_STACK;   /* the kernels that own a stack area set the offset */
    /* Width of a shading task (size_class in acn_queues.h).  Narrow groups waste less of a sample loop's last round;
     * a whole wavefront per point keeps the rays of a round on one origin, which pays when a sample's traversal is long
     * and divergent (nested compounds, CSG objects with prune programs: the scenes of the "extras" kernel variants).
     * Measured, 4 lanes: wine_glass 1080p (200 / 64 samples) 79.8 ms narrow, 85.2 wide from 33 samples; many_spheres
     * 1080p p256 every 16th pixel 3.94 s narrow, 2.90 s wide; diamond 1080p p512 4.58 s narrow, 4.05 s wide. */
    h->dev.class0_min = h->tun.class0_min ? h->tun.class0_min : ( r.prune ? 32u : 255u );
    commit_params( h, scene->params, t.n_levels, rot, unit_f );
    settle( h, forget );
    return ACN_OK;
}

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
    /* (whatever returns early from here on frees what exists by then: acn_scene_free joins the helper thread first) */
    std::unique_ptr< acn_scene_handle, void ( * )( acn_scene_handle* ) > h( new acn_scene_handle(), acn_scene_free );
    PipeRun* own = &h->run;
    own->h = h.get();
    h->device = device;
    h->tun.read();
    {
        int cus = 0;
        if( hipDeviceGetAttribute( &cus, hipDeviceAttributeMultiprocessorCount, device ) != hipSuccess || cus <= 0 ) cus = 256;
        h->cus = ( unsigned )cus;
        h->plan = acn_lane_plan( h->tun.lanes_given, h->tun.lanes, h->cus, h->tun.grid, h->tun.shade_grid, h->tun.walk_grid );
    }
    if( h->tun.early_lanes ) early_lanes_begin( h.get(), ( size_t )scene->params.image_width * ( size_t )scene->params.image_height, scene->params.path_samples );
    double t_events = 0, t_objects = 0, t_in[ 3 ] = { 0, 0, 0 };   /* ACN_DEBUG_CHUNKS: stream + events; the marks of install_scene: host-side tables, device copies, the helper thread */
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
        /* persistent grids.  A call that runs alone on its stream: 4 workgroups of 256 lanes per CU, what fits of the
         * 128-VGPR kernels.  The concurrent lanes of a call: the handle's lane plan (acn_lane_plan, bind_lane) */
        own->grid = h->tun.grid ? h->tun.grid : h->cus * 4u;
        own->shade_grid = h->tun.shade_grid ? h->tun.shade_grid : h->cus * 4u;
        own->walk_grid = h->tun.walk_grid ? h->tun.walk_grid : own->grid;
    }
    const double t_stream0 = since();
    HIP_TRY( hipStreamCreate( own->stream.put() ) );
    const double t_stream1 = since();   /* (the first stream a process makes: 85 - 100 ms on this runtime; later ones ~10) */
    /* (a stream costs ~10 ms of host time to make: the second one only where it is used) */
    const hipError_t made = run_objects( own, false, [ & ]( int i ) { if( i == 0 ) t_events = since(); } );
    if( made != hipSuccess ) return fail( ACN_ERR_DEVICE, std::string( "events and counter blocks of the handle's run: " ) + hipGetErrorString( made ) );
    t_objects = since();   /* (the counter blocks, made between t_events and here, are counted with the device copies below) */
    h->dev.flags = own->d_counts.get() + QC_FLAGS;
    st = install_scene( h.get(), scene, max_csg, false, [ & ]( int i ) { t_in[ i ] = since(); } );
    if( st != ACN_OK ) return st;
    if( h->tun.debug_chunks )
        fprintf( stderr, "[acn upload] %u nodes: the handle's stream %.2f ms, events %.2f, tables on the host %.2f, device copies %.2f, waited for %d early lanes %.2f, first kernel of the library (camera set-up) %.2f\n",
                 ( unsigned )scene->n_nodes, t_stream1 - t_stream0, t_events - t_stream1 + t_stream0, t_in[ 0 ] - t_objects, t_in[ 1 ] - t_in[ 0 ] + t_objects - t_events, ( int )h->lanes.size(), t_in[ 2 ] - t_in[ 1 ], since() - t_in[ 2 ] );
    *out = h.release();
    return ACN_OK;
}

/* The scene of a live handle is replaced.  Everything that costs a fresh handle its first frames stays: the streams, the lanes with their
 * threads, the queues as allocated and -- for a scene of the same kind (acn_replace_keeps_learned) -- what the runners learned. */
extern "C" int acn_scene_replace( acn_scene_handle* h, const acn_flat_scene* scene, uint32_t flags )
{
    if( !h || !scene ) return fail( ACN_ERR_ARG, "null argument" );
    if( flags & ~ACN_REPLACE_FORGET ) return fail( ACN_ERR_ARG, "unknown flag bits" );
    int max_csg = 0;
    std::string err;
    int st = acn_tables_validate( scene, &max_csg, &err );
    if( st != ACN_OK ) return fail( st, err );
    HIP_TRY( hipSetDevice( h->device ) );
    const auto t_begin = std::chrono::steady_clock::now();
    double t_in[ 3 ] = { 0, 0, 0 }, t_end = 0;
    auto since = [ & ]() { return std::chrono::duration< double, std::milli >( std::chrono::steady_clock::now() - t_begin ).count(); };
    const bool known = h->run.learned.known() || ( !h->lanes.empty() && h->lanes[ 0 ]->learned.known() );
    st = install_scene( h, scene, max_csg, ( flags & ACN_REPLACE_FORGET ) != 0, [ & ]( int i ) { t_in[ i ] = since(); } );
    if( st != ACN_OK ) return st;
    t_end = since();
    h->replaces++;
    if( h->tun.debug_chunks )
        fprintf( stderr, "[acn replace] %u nodes: tables on the host %.2f ms, device copies %.2f, streams idle %.2f, camera set-up and commit %.2f; learned rates %s\n",
                 ( unsigned )scene->n_nodes, t_in[ 0 ], t_in[ 1 ] - t_in[ 0 ], t_in[ 2 ] - t_in[ 1 ], t_end - t_in[ 2 ],
                 !known ? "not known yet" : h->run.learned.known() || ( !h->lanes.empty() && h->lanes[ 0 ]->learned.known() ) ? "kept" : "dropped" );
    return ACN_OK;
}

/* the same change for the render parameters alone: no table is built, nothing is allocated for the scene */
extern "C" int acn_scene_set_params( acn_scene_handle* h, const acn_params* prm )
{
    if( !h || !prm ) return fail( ACN_ERR_ARG, "null argument" );
    std::string err;
    int st = acn_tables_validate_params( prm, &err );
    if( st != ACN_OK ) return fail( st, err );
    const int n_levels = acn_tables_levels( prm );
    HIP_TRY( hipSetDevice( h->device ) );
    M3 rot; double unit_f = 0;
    if( ( st = quiesce( h ) ) != ACN_OK || ( st = camera_basis( h, *prm, &rot, &unit_f ) ) != ACN_OK ) return st;
    commit_params( h, *prm, n_levels, rot, unit_f );
    settle( h, false );
    h->param_sets++;
    return ACN_OK;
}

extern "C" int acn_scene_info( acn_scene_handle* h, uint64_t* out, int n )
{
    if( !h || !out || n < 0 || n > ACN_INFO_N ) return fail( ACN_ERR_ARG, "bad argument" );
    uint64_t v[ ACN_INFO_N ];
    uint64_t learn_passes = h->run.learn_passes; bool known = h->run.learned.known();
    for( auto& l : h->lanes ) { learn_passes += l->learn_passes; known = known || l->learned.known(); }
    v[ ACN_INFO_REPLACES ] = h->replaces; v[ ACN_INFO_PARAM_SETS ] = h->param_sets;
    /* (every stream of a handle is a member of a runner, and a runner lives as long as the handle) */
    v[ ACN_INFO_STREAMS ] = 1 + h->lanes.size(); v[ ACN_INFO_LANES ] = h->lanes.size();
    v[ ACN_INFO_LEARNING_PASSES ] = learn_passes; v[ ACN_INFO_NODES ] = h->dev.n_nodes; v[ ACN_INFO_RATES_KNOWN ] = known ? 1 : 0;
    v[ ACN_INFO_DEVICE ] = ( uint64_t )h->device;
    for( int k = 0; k < n; k++ ) out[ k ] = v[ k ];
    return ACN_OK;
}

extern "C" void acn_scene_free( acn_scene_handle* h )
{
    if( !h ) return;
    hipSetDevice( h->device );
    early_lanes_join( h );
    delete h;   /* (its members and its runners free themselves: acn_handle.h) */
}

/* the queues of a run hold what acn_wanted_caps (acn_queueplan.h) asks for, for a call of n positions: kept, or allocated anew */
static int ensure_workspace( PipeRun* r, size_t n )
{
    Workspace& w = r->ws;
    const size_t budget = r->h->workspace_budget / r->budget_div;
    const size_t stack_waves = ( size_t )( r->walk_grid > r->grid ? r->walk_grid : r->grid ) * 4;
    const size_t stack_bytes = stack_waves * r->h->tun.stack_cap * sizeof( RayTask );
    size_t want[ WQ_N ];
    acn_wanted_caps( r->learned.rate, r->sw.seeded, n, r->dev.prm.path_samples, r->dev.prm.direct_samples, r->h->scene.n_lights, budget, stack_bytes, wq_bytes, want );
    int trim = 0;
    if( acn_keep_caps( w.cap, w.stack_waves, stack_waves, want, wq_bytes, r->learned.known(), r->learned.rate_cnt, w.trimmed, &w.sized_calls, &trim ) ) return ACN_OK;
    w.release( true ); w.allocs++;
    for( ;; )
    {
        hipError_t e = hipSuccess;
        size_t total = 0;
        auto grab = [ & ]( auto& buf, size_t bytes ) { if( e == hipSuccess ) { e = ( hipError_t )buf.grow( bytes ); total += bytes; } };
        grab( w.children, sizeof( HitRec ) * want[ WQ_CHILDREN ] );
        grab( w.tasks, sizeof( DTask ) * want[ WQ_TASKS ] );
        for( int k = 0; k < ACN_NCLASS; k++ ) grab( w.idx[ k ], sizeof( uint32_t ) * want[ WQ_TASKS ] );
        grab( w.hard_shadow, sizeof( HardShadow ) * want[ WQ_HARD_SHADOW ] );
        grab( w.hard_path, sizeof( HardPath ) * want[ WQ_HARD_PATH ] );
        for( int k = 0; k < 2; k++ ) grab( w.rays[ k ], sizeof( RayTask ) * want[ WQ_RAYS ] );
        grab( w.stacks, stack_bytes );
        if( e == hipSuccess ) { w.bytes = total; break; }
        ( void )hipGetLastError();
        w.release( true );
        if( acn_halve_caps( want ) ) return fail( ACN_ERR_DEVICE, std::string( "queue workspace: " ) + hipGetErrorString( e ) );
    }
    for( int q = 0; q < WQ_N; q++ ) w.cap[ q ] = ( uint32_t )want[ q ];
    w.stack_waves = stack_waves;
    w.trimmed = trim != 0;
    return ACN_OK;
}
static size_t chunk_for_caps( const PipeRun* r ) { return acn_chunk_for_caps( r->learned.rate, r->sw.seeded, r->learned.ctl.fill_target, r->ws.cap ); }

/* per-launch HIP events (stage times of acn_last_stage_ms) cost ~0.7 % of a frame and more of a small one: only
 * with ACN_OPT_STAGE_TIMING; launch counts and pipeline statistics are kept either way */
static int stage_begin( PipeRun* r, const Switches& sw, int stage, hipStream_t stream )
{
    if( !sw.stage_timing ) { r->cur_stage = stage; return ACN_OK; }
    if( r->events_used == r->events.size() )
    {
        StageEvents e;
        HIP_TRY( hipEventCreate( e.a.put() ) );
        HIP_TRY( hipEventCreate( e.b.put() ) );
        r->events.push_back( std::move( e ) );
    }
    r->events[ r->events_used ].stage = stage;
    HIP_TRY( hipEventRecord( r->events[ r->events_used ].a.get(), stream ) );
    return ACN_OK;
}

static int stage_end( PipeRun* r, const Switches& sw, hipStream_t stream )
{
    if( !sw.stage_timing ) { r->stats.launches[ r->cur_stage ]++; return ACN_OK; }
    HIP_TRY( hipEventRecord( r->events[ r->events_used ].b.get(), stream ) );
    r->stats.launches[ r->events[ r->events_used ].stage ]++;
    r->events_used++;
    return ACN_OK;
}

static KernelFlags kernel_flags( const PipeRun* r, const Switches& sw )
{
    const acn_scene_handle::Resident& sc = r->h->scene;
    KernelFlags f;
    f.count = sw.count_work; f.leaf_lights = sc.leaf_lights; f.lds_nodes = sc.lds_bytes != 0; f.prune = sc.prune;
    return f;
}
/* the workspace as the kernels of path level `level` see it */
static LevelQ level_queues( const PipeRun* r, const Switches& sw, int level )
{
    const Workspace& w = r->ws;
    const Tunables& tun = r->h->tun;
    LevelQ q;
    q.tasks = w.tasks.get(); for( int k = 0; k < ACN_NCLASS; k++ ) q.idx[ k ] = w.idx[ k ].get();
    q.task_cap = w.cap[ WQ_TASKS ]; q.child_cap = w.cap[ WQ_CHILDREN ]; q.hs_cap = w.cap[ WQ_HARD_SHADOW ]; q.hard_cap = w.cap[ WQ_HARD_PATH ];
    q.ray_cap = w.cap[ WQ_RAYS ];
    q.children = w.children.get(); q.hard_shadow = w.hard_shadow.get(); q.hard_path = w.hard_path.get();
    q.rays[ 0 ] = w.rays[ 0 ].get(); q.rays[ 1 ] = w.rays[ 1 ].get();
    q.stacks = w.stacks.get(); q.stack_cap = tun.stack_cap; q.stack_use = tun.stack_use;
    q.counts = r->d_counts.get() + ( size_t )level * QC_N;
    q.prev_children = r->d_counts.get() + ( size_t )( level > 0 ? level - 1 : 0 ) * QC_N + QC_CHILDREN;
    q.grid = r->grid; q.shade_grid = r->shade_grid; q.walk_grid = r->walk_grid;
    q.fetch_walk = tun.fetch_walk; q.fetch_hard = tun.fetch_hard; q.private_limit = tun.private_limit; q.fetch_shade = tun.fetch_shade;
    /* the outermost sample loops are those of level 0 */
    const bool sharded = level == 0 && sw.shard_world > 1;
    q.shard_rank = sharded ? sw.shard_rank : 0u; q.shard_world = sharded ? sw.shard_world : 1u;
    q.emit_terms = sharded && sw.shard_rank != 0 ? 0u : 1u;
    return q;
}

/* launches of k_walk for path level `level` (acn_walk_passes; ACN_LEARN_PASSES=0: what the last chunk used does not count) */
static uint32_t walk_passes_of_level( const PipeRun* r, int level )
{
    return acn_walk_passes( r->dev.prm.trace_depth, level, r->h->tun.walk_passes, r->h->tun.learn_passes ? r->learned.walk_passes_seen[ level ] : 0u );
}

#define ACN_LAUNCH( r, sw, stage, stream, call ) do { int st_ = stage_begin( r, sw, stage, stream ); if( st_ != ACN_OK ) return st_; call; \
    HIP_TRY( hipGetLastError() ); if( ( st_ = stage_end( r, sw, stream ) ) != ACN_OK ) return st_; } while( 0 )

/* One chunk of positions [ base, base + cnt ).  The whole chain -- per path level: ( k_shade_hits -> ) the passes of
 * k_walk -> k_shade x 4 size classes -> k_hard_shadow -> k_hard_path -- is enqueued blind: every kernel takes
 * its input count from the counter block of its level on the device, and a level that turns out to be empty costs a few
 * launches of waves that exit at once.  The host synchronises ONCE, at the end, to read the counter blocks: overflow
 * flags (the chunk is then redone smaller) and statistics.  sw: the switches of the call, or those of the learning pass. */
static int render_chunk( PipeRun* r, const Switches& sw, const Primary& prim, uint32_t base, uint32_t cnt, TileOrder order,
                         hipStream_t stream, acn_chunk_report* report )
{
    const Tunables& tun = r->h->tun;
    RunStats& stats = r->stats;
    const int levels = r->h->scene.n_levels;
    const KernelFlags f = kernel_flags( r, sw );
    const SceneArgs s = scene_args( r->dev, r->h->scene );
    const size_t lds = machine_lds_bytes( r->h->scene );
    unsigned long long* const accum = r->d_accum.get(); unsigned long long* const counters = r->d_counters.get(); uint32_t* const h_counts = r->h_counts.get();
    HIP_TRY( hipMemsetAsync( r->d_counts.get(), 0, sizeof( uint32_t ) * QC_N * levels, stream ) );
    if( prim.rays )
    {
        /* the caller's rays are generation 0 of level 0, one slot each (launch_render keeps a chunk within the ray queue) */
        if( cnt > r->ws.cap[ WQ_RAYS ] ) return fail( ACN_ERR_DEVICE, "a chunk of rays larger than the ray queue" );
        /* (a walk launch of the statistics: it does what k_walk's first pass does for positions, make the primary rays) */
        ACN_LAUNCH( r, sw, 0, stream, acn_launch_seed_rays( prim.rays, base, cnt, order, ( int )r->dev.prm.trace_depth, level_queues( r, sw, 0 ), stream ) );
    }
    const uint32_t n_cam = prim.rays ? 0u : cnt;
    uint32_t passes[ ACN_LEVEL_BLOCKS ];   /* launches of k_walk per level */
    for( int level = 0; level < levels; level++ )
    {
        LevelQ q = level_queues( r, sw, level );
        /* the path-sample hits of the level before are shaded (level >= 1), then the specular rays walked: generation
         * passes while the generations are large, the rest on the waves' private stacks (k_walk); a level has at most as
         * many generations as its hits have depth left */
        /* a small chunk (<= 2^17 positions) of a frame without path tracing finishes every generation that is no larger than
         * itself on the private stacks: its generations are not worth a launch each (C1, 120 000 pixels on one lane: 1.41 ->
         * 1.15 ms).  With path samples the rule was measured and dropped: the 1/8 share of the 1080p frame 15.2 -> 14.8 ms and
         * hanging_lamp 600x800 -3 %, but paraffin_lamp 400x600 +8 % -- the rays of a CSG scene are worth redistributing
         * (profiles/r03/private_limit_small_frames.txt) */
        if( !tun.private_limit_set && r->dev.prm.path_samples == 0 && cnt <= ( 1u << 17 ) && cnt > q.private_limit ) q.private_limit = cnt;
        if( level > 0 ) ACN_LAUNCH( r, sw, 0, stream, acn_launch_shade_hits( f.count, q, stream, s, accum, counters ) );
        passes[ level ] = walk_passes_of_level( r, level );
        for( uint32_t pass = 0; pass < passes[ level ]; pass++ )
        {
            /* (the last launch of a level finishes whatever is left on the private stacks: the input of all later generations) */
            const WalkLaunch w = { pass, pass + 1 == passes[ level ], prim.pos_xy, prim.first, base, level == 0 && pass == 0 ? n_cam : 0u, order, lds, accum, counters };
            ACN_LAUNCH( r, sw, 0, stream, acn_launch_walk( f, q, w, stream, s ) );
        }
        ACN_LAUNCH( r, sw, 1, stream, acn_launch_shade64( f, q, stream, s, accum, counters ) );
        ACN_LAUNCH( r, sw, 1, stream, acn_launch_shade16( f, q, stream, s, accum, counters ) );
        ACN_LAUNCH( r, sw, 1, stream, acn_launch_shade4( f, q, stream, s, accum, counters ) );
        ACN_LAUNCH( r, sw, 1, stream, acn_launch_shade1( f, q, stream, s, accum, counters ) );
        ACN_LAUNCH( r, sw, 3, stream, acn_launch_hard_shadow( f, q, lds, stream, s, accum, counters ) );
        /* the last level casts no path rays (depth <= 10) */
        if( level + 1 < levels ) ACN_LAUNCH( r, sw, 3, stream, acn_launch_hard_path( f, q, lds, stream, s, accum, counters ) );
    }
    HIP_TRY( hipMemcpyAsync( h_counts, r->d_counts.get(), sizeof( uint32_t ) * QC_N * levels, hipMemcpyDeviceToHost, stream ) );
    HIP_TRY( hipStreamSynchronize( stream ) );
    stats.host_syncs++;
    /* every decision is made from the counter blocks (acn_read_chunk: flags and verdict, queue marks, statistics, passes seen) */
    acn_read_chunk( h_counts, levels, passes, prim.rays != nullptr, report );
    stats.flags_seen |= report->flags & ACN_FLAG_CLAMPED;
    if( report->verdict == ACN_CHUNK_STACK_OVERFLOW ) return fail( ACN_ERR_UNSUPPORTED, "device CSG / compound stack overflow (or a walk that did not end)" );
    if( report->verdict != ACN_CHUNK_FITS ) return ACN_OK;
    stats.take( *report );
    /* a chunk large enough to stand for the next one */
    if( cnt >= 4096 ) for( int level = 0; level < levels; level++ ) r->learned.walk_passes_seen[ level ] = report->passes_seen[ level ];
    return ACN_OK;
}

/* the ACN_DEBUG_CHUNKS lines: " T x C x HS x HP x R x", one value per queue (decimals 0: a count) */
template< class F > static std::string per_queue( int decimals, F value )
{
    static const char* const name[ WQ_N ] = { "T", "C", "HS", "HP", "R" };
    std::string s;
    char b[ 336 ];   /* (the longest %.1f of a double) */
    for( int q = 0; q < WQ_N; q++ ) { snprintf( b, sizeof( b ), " %s %.*f", name[ q ], decimals, ( double )value( q ) ); s += b; }
    return s;
}

/* Cold handle: the queue demand per position is learned from a SAMPLE of the call's own positions -- every ( n / m )-th of them,
 * m = 512 .. 4096 -- rendered once on the starter queues and thrown away, before anything is sized.  Round 3 let the first
 * chunks of the call learn: the first tile of the order is a corner of the picture (C4: 1 shading task and 161 deferred path rays
 * per position where the frame's average is 300 / 1 800), so the queues were found one by one by halving -- 12 redone chunks on
 * the C3 / C4 frames, a first frame of 718 ms on paraffin_lamp where the second takes 465 -- and every lane of a call learned
 * for itself and re-sized its queues in the middle of the frame.  A sample over the whole frame costs one short chain of
 * launches (a few ms; nothing next to a frame whose queues must be allocated anyway) and is trusted like a large chunk: the
 * queues are then sized ONCE, while the device is idle (launch_render; render_lanes for all lanes of a call). */
static int learn_rates( PipeRun* r, const Primary& prim, size_t n, hipStream_t stream, size_t plan_positions, unsigned plan_grid )
{
    const Tunables& tun = r->h->tun;
    Learned& L = r->learned;
    if( L.known() || !tun.learn_sample || tun.chunk || n < 16384 ) return ACN_OK;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [ & ]() { return std::chrono::duration< double, std::milli >( std::chrono::steady_clock::now() - t_begin ).count(); };
    r->learn_passes++;
    int st = ensure_workspace( r, 4096 );   /* the starter set */
    if( st != ACN_OK ) return st;
    if( r->d_accum.grow( sizeof( unsigned long long ) * 3 * n ) ) return ACN_ERR_DEVICE;
    if( tun.debug_chunks ) fprintf( stderr, "[acn sample] starter queues (%.2f GB) after %.2f ms\n", ( double )r->ws.bytes / 1e9, since() );
    size_t want = acn_sample_positions( r->ws.cap[ WQ_CHILDREN ], r->ws.cap[ WQ_HARD_SHADOW ], r->dev.prm.path_samples, r->dev.prm.direct_samples, r->h->scene.n_lights, n );
    /* the sample renders unsharded, counts no work and records no stage events */
    Switches sw;
    sw.seeded = r->sw.seeded;
    r->events_used = 0;
    for( ; want >= 64; want /= 2 )
    {
        TileOrder order;
        order.n = ( uint32_t )n; order.n_tiles = 1; order.mul = 1;
        order.sample_stride = ( uint32_t )( n / want );
        const uint32_t cnt = ( uint32_t )want;
        hipLaunchKernelGGL( k_clear_slots, dim3( ( cnt + 255 ) / 256 ), dim3( 256 ), 0, stream, r->d_accum.get(), 0u, cnt, order );
        HIP_TRY( hipGetLastError() );
        acn_chunk_report c;
        st = render_chunk( r, sw, prim, 0u, cnt, order, stream, &c );
        if( st != ACN_OK ) break;
        const bool overflow = c.verdict != ACN_CHUNK_FITS;
        if( tun.debug_chunks )
            fprintf( stderr, "[acn sample] chain done after %.2f ms\n", since() );
        if( tun.debug_chunks )
            fprintf( stderr, "[acn sample] %u positions (every %u-th) %s dead %.2f | per pos%s\n", cnt, order.sample_stride, overflow ? "OVERFLOW" : "ok",
                     c.dead_share, per_queue( 1, [ & ]( int q ) { return c.fill[ q ] / ( double )cnt; } ).c_str() );
        if( overflow ) continue;
        acn_sample_rates( r->h_counts.get(), r->h->scene.n_levels, cnt, plan_positions, plan_grid, L.rate );
        if( tun.debug_chunks ) fprintf( stderr, "[acn sample] rates%s\n", per_queue( 1, [ & ]( int q ) { return L.rate[ q ]; } ).c_str() );
        L.rate_cnt = 8192;   /* a sample of the whole frame: trusted like a chunk that size (launch_render re-sizes for the whole rest at once) */
        break;
    }
    L.forget_passes();
    return st;
}

/* tail (nullable): what follows k_finalize on `stream` within the call (a lane scatters its share: render_lanes); ev1 is recorded
 * behind it */
static int launch_render( PipeRun* r, const Primary& prim, size_t n, double* d_out_rgb,
                          const acn_render_opts* opts, hipStream_t stream, const std::function< int() >* tail = nullptr )
{
    const Tunables& tun = r->h->tun;
    Learned& L = r->learned;
    Switches& sw = r->sw;
    if( opts->cancel && *opts->cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many positions in one call" );
    sw.seeded = prim.rays != nullptr;
    int linear = ( opts->flags & ACN_OPT_LINEAR_OUT ) ? 1 : 0;
    sw.count_work = ( opts->flags & ACN_OPT_COUNT_WORK ) || tun.count_work;
    sw.shard_rank = 0; sw.shard_world = 1;
    if( opts->shard_mode == ACN_SHARD_SAMPLES && opts->shard_world > 1 )
    {
        if( opts->shard_rank >= opts->shard_world ) return fail( ACN_ERR_ARG, "shard_rank >= shard_world" );
        sw.shard_rank = opts->shard_rank; sw.shard_world = opts->shard_world;
    }
    else if( opts->shard_mode > ACN_SHARD_SAMPLES ) return fail( ACN_ERR_ARG, "unknown shard_mode" );
    sw.stage_timing = ( opts->flags & ACN_OPT_STAGE_TIMING ) || tun.stage_timing;
    int st = learn_rates( r, prim, n, stream, n, r->walk_grid > r->grid ? r->walk_grid : r->grid );
    if( st != ACN_OK ) return st;
    st = ensure_workspace( r, n );
    if( st != ACN_OK ) return st;
    if( r->d_accum.grow( sizeof( unsigned long long ) * 3 * n ) ) return ACN_ERR_DEVICE;
    r->events_used = 0;
    r->stats.reset();
    L.ctl.retry_bound = 0;   /* (a call that ended in the middle of a retry) */
    HIP_TRY( hipMemsetAsync( r->d_counters.get(), 0, sizeof( unsigned long long ) * ACN_CNT_SLOTS, stream ) );
    HIP_TRY( hipEventRecord( r->ev0.get(), stream ) );
    HIP_TRY( hipMemsetAsync( r->d_accum.get(), 0, sizeof( unsigned long long ) * 3 * n, stream ) );

    /* Positions per pipeline run.  How many records a position leaves in each queue differs by orders of magnitude between
     * scenes (wine_glass: 15 deferred shadow rays per pixel; a closed room at path_samples 1024: 260 000 second-level hits),
     * so the rates are learned: a cautious first chunk on a small starter workspace (acn_first_chunk_guess), then chunks that
     * fill the fullest queue to 70 %, and the queues themselves re-sized once the rates are known (ensure_workspace); an
     * overflow halves the chunk.  Rates and workspace stay with the run for its next call. */
    size_t chunk = L.known() ? chunk_for_caps( r )
                             : acn_first_chunk_guess( r->ws.cap[ WQ_CHILDREN ], r->ws.cap[ WQ_HARD_SHADOW ], r->dev.prm.path_samples, r->dev.prm.direct_samples, r->h->scene.n_lights, 32768 );
    if( tun.chunk ) chunk = tun.chunk;
    if( chunk < 64 ) chunk = 64;
    TileOrder order;
    order.n = ( uint32_t )n;
    order.n_tiles = acn_tile_order( n, ACN_ORDER_SHIFT, &order.mul );
    order.sample_stride = 0;
    const size_t n_slots = ( size_t )order.n_tiles << ACN_ORDER_SHIFT;
    size_t base = 0;
    while( base < n_slots )
    {
        if( opts->cancel && *opts->cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
        /* the planned chunk; a rest that is predicted to fill no queue beyond 85 % is taken whole (a second chunk would be
         * another whole chain of launches for a few positions); a retry is at most half of the chunk that overflowed
         * (acn_chunkplan.h) */
        double plan[ WQ_N ];
        for( int q = 0; q < WQ_N; q++ ) plan[ q ] = acn_queue_demand( L.rate, q, sw.seeded );
        uint32_t cnt = acn_ctl_next( &L.ctl, n_slots - base, chunk, tun.chunk != 0, L.known(), plan, r->ws.cap );
        /* (the seeded generation of a ray call takes one ray-queue slot per position, also under ACN_CHUNK) */
        if( prim.rays && cnt > r->ws.cap[ WQ_RAYS ] ) cnt = r->ws.cap[ WQ_RAYS ];
        acn_chunk_report c;
        /* the work counters of a chunk that has to be redone must not count twice */
        if( sw.count_work ) HIP_TRY( hipMemcpyAsync( r->d_counters_keep.get(), r->d_counters.get(), sizeof( unsigned long long ) * ACN_CNT_SLOTS, hipMemcpyDeviceToDevice, stream ) );
        st = render_chunk( r, sw, prim, ( uint32_t )base, cnt, order, stream, &c );
        if( st != ACN_OK ) return st;
        const bool overflow = c.verdict != ACN_CHUNK_FITS;
        if( tun.debug_chunks )
            fprintf( stderr, "[acn chunk] base %zu cnt %u %s target %.2f dead %.2f | fill%s | per pos%s | rate%s | cap%s\n",
                     base, cnt, overflow ? "OVERFLOW" : "ok", L.ctl.fill_target, c.dead_share, per_queue( 0, [ & ]( int q ) { return c.fill[ q ]; } ).c_str(),
                     per_queue( 1, [ & ]( int q ) { return c.fill[ q ] / ( double )cnt; } ).c_str(), per_queue( 1, [ & ]( int q ) { return L.rate[ q ]; } ).c_str(),
                     per_queue( 0, [ & ]( int q ) { return r->ws.cap[ q ]; } ).c_str() );
        if( overflow )
        {
            if( cnt <= 1 ) return fail( ACN_ERR_DEVICE, "work queues overflow for a single position: raise ACN_WORKSPACE_MB" );
            if( sw.count_work ) HIP_TRY( hipMemcpyAsync( r->d_counters.get(), r->d_counters_keep.get(), sizeof( unsigned long long ) * ACN_CNT_SLOTS, hipMemcpyDeviceToDevice, stream ) );
            r->stats.retries++;
            /* scenes whose demand per position varies much between chunks (many_spheres p256: 49 of 220 chunks were redone at
             * a fixed 70 %) plan with more head room */
            chunk = acn_ctl_overflow( &L.ctl, cnt );
            acn_overflow_rates( L.rate, cnt, c.fill );
            L.forget_passes();
            hipLaunchKernelGGL( k_clear_slots, dim3( ( cnt + 255 ) / 256 ), dim3( 256 ), 0, stream, r->d_accum.get(), ( uint32_t )base, cnt, order );
            HIP_TRY( hipGetLastError() );
            continue;
        }
        r->stats.chunks++;
        base += cnt;
        acn_ctl_fit( &L.ctl );
        if( tun.chunk ) continue;
        acn_learn_rates( L.rate, &L.rate_cnt, cnt, c.fill, c.dead_share );
        const size_t remaining = n_slots - base;
        if( remaining && ( double )chunk_for_caps( r ) * ( 0.85 / L.ctl.fill_target ) < ( double )remaining )
        {
            /* more than one further chunk with these queues: re-size them (a no-op when they already are what the budget
             * allows).  Rates that come from a small chunk are trusted for a medium one only. */
            const size_t target = L.rate_cnt < 8192 ? ( remaining < 65536 ? remaining : ( size_t )65536 ) : remaining;
            if( ( st = ensure_workspace( r, target ) ) != ACN_OK ) return st;
        }
        chunk = chunk_for_caps( r );
    }
    if( ( st = stage_begin( r, sw, 2, stream ) ) != ACN_OK ) return st;
    hipLaunchKernelGGL( k_finalize, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        ( const unsigned long long* )r->d_accum.get(), ( uint32_t )n, r->dev.prm.gamma, linear, d_out_rgb );
    HIP_TRY( hipGetLastError() );
    if( ( st = stage_end( r, sw, stream ) ) != ACN_OK ) return st;
    if( tail && ( st = ( *tail )() ) != ACN_OK ) return st;
    HIP_TRY( hipEventRecord( r->ev1.get(), stream ) );
    return ACN_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* Concurrent lanes.  One pipeline run is a chain of ~60 dependent launches (a walk pass per specular generation,
 * shade, hard rays, per level), each ending in a tail where a few long rays keep the chip waiting, and each followed by
 * a host round trip for the queue counts.  Pixels are independent, so a call is cut into ACN_LANE_TILE-pixel tiles
 * dealt round-robin to K lanes (acn_lane_count); every lane is a PipeRun of its own (the handle's resident scene, own stream,
 * own workspace) driven by its own host thread, and the lanes' kernels fill each other's tails and bubbles.  Measured on the
 * 1080p frame: 118 -> 87 ms with 4 lanes; on the share one of 8 GPUs gets: 21.0 -> 16.5 ms.  Results are unchanged: every
 * pixel is computed by exactly the same kernels from exactly the same inputs. */
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

/* A lane = a PipeRun with a stream, events, counter blocks and a host thread of its own.  Making a stream takes ~10 ms of host
 * time (tools/bench_alloc: 12 streams 120 - 130 ms, one after the other whatever thread asks; events, pinned memory and hipMalloc
 * of any size are free beside that), so six lanes are 60 ms of a handle's first call, more than its learning pass on the wine
 * glass.  The HIP objects (lane_objects: nothing in it reads the handle) are therefore made on a helper thread while the learning
 * pass runs on the device (render_lanes), and the lane is tied to its handle afterwards (bind_lane). */
static int lane_objects( int device, bool debug, std::unique_ptr< PipeRun >* out )
{
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [ & ]() { return std::chrono::duration< double, std::milli >( std::chrono::steady_clock::now() - t_begin ).count(); };
    double t[ 5 ] = { 0, 0, 0, 0, 0 };
    std::unique_ptr< PipeRun > l( new PipeRun() );
    hipError_t e = hipSetDevice( device );
    t[ 0 ] = since();
    if( e == hipSuccess ) e = hipStreamCreateWithFlags( l->stream.put(), hipStreamNonBlocking );
    t[ 1 ] = since();
    if( e == hipSuccess ) e = run_objects( l.get(), true, [ & ]( int i ) { t[ 2 + i ] = since(); } );
    if( e != hipSuccess ) return fail( ACN_ERR_DEVICE, hipGetErrorString( e ) );
    l->worker.reset( new LaneWorker() ); l->worker->start();
    if( debug ) fprintf( stderr, "[acn lane] set device %.2f ms, stream %.2f, events %.2f, counter blocks + memsets %.2f, pinned block %.2f, thread %.2f\n", t[ 0 ], t[ 1 ] - t[ 0 ], t[ 2 ] - t[ 1 ], t[ 3 ] - t[ 2 ], t[ 4 ] - t[ 3 ], since() - t[ 4 ] );
    *out = std::move( l );
    return ACN_OK;
}

static unsigned lane_grid( const acn_scene_handle* h ) { return h->plan.grid; }
static void bind_lane( const acn_scene_handle* h, int lanes, PipeRun* l )
{
    l->h = h;
    l->budget_div = ( size_t )lanes;
    refresh_run( h, l );
    /* Round 4: six lanes on grids of ONE workgroup per CU (k_shade: one and a half) instead of four lanes on two.  With k_walk at
     * four waves per SIMD a grid of 256 workgroups is resident at once, and six shorter chains fill each other's tails better than
     * four: 1080p 50.2 -> 49.1 ms, c2 26.4 -> 25.0, and the share one of 8 GPUs gets 12.25 -> 11.4 ms (profiles/r04/ab_lanes6_*).
     * A call that runs ALONE on the handle keeps four workgroups per CU (diamond on one lane: 2.3 s with them, 6.7 s with one).
     * That is the plan of a host that sets ACN_LANES, measured with a hardware queue per lane.  The default plan is made for the
     * four queues of a process that asks for none: fewer lanes on larger grids (acn_lane_plan). */
    l->grid = lane_grid( h );
    l->shade_grid = h->plan.shade_grid;
    l->walk_grid = h->plan.walk_grid;
}

static int lanes_for( const acn_scene_handle* h, size_t n ) { return acn_lanes_for_counts( h->plan.lanes, n, h->dev.prm.path_samples ); }

static int render_lanes( acn_scene_handle* h, int lanes, const Primary& prim, size_t n, double* d_out_rgb,
                         const acn_render_opts* opts, hipStream_t stream )
{
    PipeRun* own = &h->run;
    /* ACN_DEBUG_CHUNKS: where a call's wall time goes before and after the lanes run (one line per call on stderr) */
    const auto t_begin = std::chrono::steady_clock::now();
    double t_mark[ 5 ] = { 0, 0, 0, 0, 0 };
    auto mark = [ & ]( int i ) { t_mark[ i ] = std::chrono::duration< double, std::milli >( std::chrono::steady_clock::now() - t_begin ).count(); };
    /* the lanes this call lacks: made on a helper thread while the learning pass of a cold handle runs (see lane_objects) */
    /* (lanes made during the upload are the handle's already: quiesce) */
    const int missing = lanes - ( int )h->lanes.size();
    std::vector< std::unique_ptr< PipeRun > > made;
    int made_status = ACN_OK; std::string made_message;
    auto make_missing = [ & ]()
    {
        for( int k = 0; k < missing && made_status == ACN_OK; k++ )
        {
            std::unique_ptr< PipeRun > l;
            made_status = lane_objects( h->device, h->tun.debug_chunks, &l );
            if( made_status == ACN_OK ) made.push_back( std::move( l ) ); else made_message = g_last_error;   /* thread-local where it was set */
        }
    };
    std::thread maker;
    const bool learn = h->lanes.empty() ? !own->learned.known() : !h->lanes[ 0 ]->learned.known() && !own->learned.known();
    const bool maker_used = missing > 0 && learn && h->tun.cold_pipeline;
    if( missing > 0 ) { if( maker_used ) maker = std::thread( make_missing ); else make_missing(); }
    /* what the caller queued on `stream` before this call must be done before the lanes read the positions: every lane's stream
     * waits for ev0 on the device (post_lane), the host does not.  A cold handle waits here as well: its learning pass and the
     * sizing that follows it (hipFree) run while nothing else of the caller's does */
    hipError_t drained = hipEventRecord( own->ev0.get(), stream );
    if( drained == hipSuccess && learn ) drained = hipEventSynchronize( own->ev0.get() );
    mark( 0 );
    /* a cold handle learns the scene's queue demand once, for all lanes, from a sample of the call (learn_rates) */
    int learned = ACN_OK;
    if( drained == hipSuccess && learn )
    {
        own->budget_div = 1;
        learned = learn_rates( own, prim, n, stream, n / ( size_t )lanes, lane_grid( h ) );
        if( learned == ACN_OK ) drained = hipStreamSynchronize( stream );
    }
    if( maker.joinable() ) maker.join();
    for( auto& l : made ) { bind_lane( h, lanes, l.get() ); h->lanes.push_back( std::move( l ) ); }
    if( drained != hipSuccess ) return fail( ACN_ERR_DEVICE, hipGetErrorString( drained ) );
    if( learned != ACN_OK ) return learned;
    if( made_status != ACN_OK ) return fail( made_status, made_message );
    for( int k = 0; k < lanes; k++ ) Learned::inherit( &h->lanes[ k ]->learned, own->learned.known() ? own->learned : h->lanes[ 0 ]->learned );
    if( learn && own->learned.known() ) own->ws.release();   /* the bound is the handle's, whoever uses it */
    /* The lanes' queues are (re-)sized here, while the device is idle: hipFree synchronises the device, so lanes that
     * re-size at the start of their chains wait for each other's chunks (second frame of paraffin_lamp 400x600, whose
     * queues are trimmed to the rates the first frame learned: 2.1 s instead of 0.45, profiles/r03/frames_paraffin_*.txt).
     * hipMalloc itself is not what a first call pays: 22 GB of queues take 1 - 5 ms (tools/bench_alloc: 0.02 ms per GB; a lane that
     * started as soon as its own queues existed gained nothing, profiles/r04/first_frames_s36_s38.txt). */
    mark( 1 );
    acn_render_opts lane_opts = *opts;
    std::vector< int > status( lanes, ACN_OK );
    std::vector< std::string > message( lanes );
    auto post_lane = [ & ]( int k )
    {
        h->lanes[ k ]->worker->post( [ &, k ]()
        {
            PipeRun* l = h->lanes[ k ].get();
            l->budget_div = ( size_t )lanes;
            size_t cnt = acn_lane_count( n, lanes, k );
            auto run = [ & ]() -> int
            {
                HIP_TRY( hipSetDevice( h->device ) );
                if( cnt == 0 ) { l->events_used = 0; HIP_TRY( hipMemset( l->d_counters.get(), 0, sizeof( unsigned long long ) * ACN_CNT_SLOTS ) ); return ACN_OK; }
                /* the lane's share of the input: positions (2 doubles each) or rays (6) */
                if( l->d_lane_in.grow( sizeof( double ) * ( prim.rays ? 6 : 2 ) * cnt ) || l->d_lane_out.grow( sizeof( double ) * 3 * cnt ) ) return ACN_ERR_DEVICE;
                double* const d_in = l->d_lane_in.get(); double* const d_out = l->d_lane_out.get();
                hipStream_t const ls = l->stream.get();
                HIP_TRY( hipStreamWaitEvent( ls, own->ev0.get(), 0 ) );
                if( prim.rays )
                    hipLaunchKernelGGL( k_lane_gather_rays, dim3( ( unsigned )( ( cnt + 255 ) / 256 ) ), dim3( 256 ), 0, ls,
                                        prim.rays, cnt, lanes, k, d_in );
                else
                    hipLaunchKernelGGL( k_lane_gather, dim3( ( unsigned )( ( cnt + 255 ) / 256 ) ), dim3( 256 ), 0, ls,
                                        prim.pos_xy, prim.first, ( uint64_t )h->dev.prm.image_width, cnt, lanes, k, d_in );
                HIP_TRY( hipGetLastError() );
                /* the lane's share of the frame goes to its places in the caller's buffer behind k_finalize; the lane's ev1 is
                 * recorded behind that (launch_render) and the caller's stream waits for it (below): the worker does not.  Its
                 * last wait is its last chunk's; d_lane_in and d_lane_out are used again by the next call on this stream, in order */
                const std::function< int() > scatter = [ & ]() -> int
                {
                    hipLaunchKernelGGL( k_lane_scatter, dim3( ( unsigned )( ( cnt + 255 ) / 256 ) ), dim3( 256 ), 0, ls,
                                        ( const double* )d_out, cnt, lanes, k, d_out_rgb );
                    HIP_TRY( hipGetLastError() );
                    return ACN_OK;
                };
                return launch_render( l, prim.rays ? primary_rays( d_in ) : primary_positions( d_in ), cnt, d_out, &lane_opts, ls, &scatter );
            };
            status[ k ] = run();
            if( status[ k ] != ACN_OK ) message[ k ] = g_last_error;   /* thread-local in the worker */
        } );
    };
    for( int k = 0; k < lanes; k++ )
    {
        PipeRun* l = h->lanes[ k ].get();
        l->budget_div = ( size_t )lanes;
        l->sw.seeded = prim.rays != nullptr;
        const size_t cnt = acn_lane_count( n, lanes, k );
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
    /* the join: whatever the caller queues on `stream` after this call follows the lanes' last kernels, in stream order */
    for( int k = 0; k < lanes; k++ ) if( acn_lane_count( n, lanes, k ) ) HIP_TRY( hipStreamWaitEvent( stream, h->lanes[ k ]->ev1.get(), 0 ) );
    HIP_TRY( hipEventRecord( own->ev1.get(), stream ) );
    /* statistics of the call: the lanes' together (RunStats::add), without those that had no positions */
    own->stats.reset();
    for( int k = 0; k < lanes; k++ ) if( acn_lane_count( n, lanes, k ) ) own->stats.add( h->lanes[ k ]->stats );
    h->used_lanes = true;
    h->lanes_used = lanes;
    return ACN_OK;
}

/* one pipeline run on the handle itself, or the concurrent lanes */
int render_dispatch( acn_scene_handle* h, const Primary& prim, size_t n, double* d_out_rgb, const acn_render_opts* opts, hipStream_t stream )
{
    PipeRun* own = &h->run;
    int lanes = lanes_for( h, n );
    /* Lanes pay when a lane's share is ONE chunk: their chains overlap.  A call whose queues cannot hold it in one chunk
     * per lane within the workspace bound -- scenes with hundreds or thousands of path samples -- does better on one lane
     * with the whole bound: four times the chunk, a quarter of the chains, and each chunk fills the chip by itself
     * (diamond 1080p p512, every 16th pixel: 3.69 s on 4 lanes, 2.83 s on one; hanging_lamp 2160p p1024, every 64th:
     * 21.6 -> 15.4 s; wine_glass 1080p p64, which fits: 71 ms on 4 lanes, 95 on one). */
    if( lanes > 1 )
    {
        const Learned* known = nullptr;
        if( !h->lanes.empty() && h->lanes[ 0 ]->learned.known() ) known = &h->lanes[ 0 ]->learned;
        else if( own->learned.known() ) known = &own->learned;
        if( known ) { if( acn_one_lane( known->rate, prim.rays != nullptr, n, wq_bytes, h->workspace_budget, h->one_lane ) ) lanes = 1; }
        else if( h->dev.prm.path_samples >= 256 ) lanes = 1;
    }
    h->used_lanes = false;
    h->one_lane = lanes <= 1 && lanes_for( h, n ) > 1;
    int st;
    if( lanes <= 1 )
    {
        for( auto& l : h->lanes ) l->ws.release();   /* the bound is the handle's, whoever uses it */
        if( !h->lanes.empty() ) Learned::inherit( &own->learned, h->lanes[ 0 ]->learned );
        st = launch_render( own, prim, n, d_out_rgb, opts, stream );
    }
    else
    {
        own->ws.release();
        st = render_lanes( h, lanes, prim, n, d_out_rgb, opts, stream );   /* (makes the lanes it lacks) */
    }
    if( st == ACN_OK && n ) h->timed = true;
    return st;
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* the pipeline's own entry points (every other one: acn_calls.hip) */
extern "C" int acn_render_positions_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, void* d_out_rgb,
                                         const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !d_pos_xy || !d_out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    int st = call_begin( h, &c );
    if( st == ACN_OK ) st = render_dispatch( h, primary_positions( ( const double* )d_pos_xy ), n, ( double* )d_out_rgb, &c.opts, c.stream );
    return st != ACN_OK ? st : call_end( c );
}

extern "C" int acn_render_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, void* d_out_rgb,
                                         const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( count && !d_out_rgb ) ) return fail( ACN_ERR_ARG, "null argument" );
    int st = pixel_range_check( h, first, count );
    if( st == ACN_OK ) st = call_begin( h, &c );
    if( st == ACN_OK ) st = render_dispatch( h, primary_main_pass( first ), count, ( double* )d_out_rgb, &c.opts, c.stream );
    return st != ACN_OK ? st : call_end( c );
}

extern "C" int acn_render_positions( acn_scene_handle* h, const double* pos_xy, size_t n, double* out_rgb,
                                     const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !pos_xy || !out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    c.opts.stream = nullptr;
    return host_in_out( h, pos_xy, sizeof( double ) * 2 * n, out_rgb, sizeof( double ) * 3 * n,
                        [ & ]( void* d_pos, void* d_out ) { return acn_render_positions_dev( h, d_pos, n, d_out, &c.opts ); } );
}

/* ---- caller-supplied primary rays (k_rays.hip) ---- */
extern "C" int acn_render_rays_dev( acn_scene_handle* h, const void* d_rays, size_t n, void* d_out_rgb, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !d_rays || !d_out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many rays in one call" );
    int st = call_begin( h, &c );
    if( st == ACN_OK ) st = check_rays( h, ( const double* )d_rays, n, c.stream );
    if( st == ACN_OK ) st = render_dispatch( h, primary_rays( ( const double* )d_rays ), n, ( double* )d_out_rgb, &c.opts, c.stream );
    return st != ACN_OK ? st : call_end( c );
}

extern "C" int acn_render_rays( acn_scene_handle* h, const double* rays, size_t n, double* out_rgb, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !rays || !out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    c.opts.stream = nullptr;
    return host_in_out( h, rays, sizeof( double ) * 6 * n, out_rgb, sizeof( double ) * 3 * n,
                        [ & ]( void* d_rays, void* d_out ) { return acn_render_rays_dev( h, d_rays, n, d_out, &c.opts ); } );
}

/* ---- sharding of whole positions: tiles of ACN_SHARD_TILE, round-robin (plain arithmetic, no GPU) ---- */
extern "C" size_t acn_shard_tile_count( size_t n, uint32_t rank, uint32_t world )
{
    if( world <= 1 ) return rank == 0 ? n : 0;
    return rank < world ? acn_lane_count( n, ( int )world, ( int )rank ) : 0;
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
    Call c( opts );
    if( !h || ( count && !d_part ) || world == 0 || rank >= world ) return fail( ACN_ERR_ARG, "bad argument" );
    int st = pixel_range_check( h, first, count );
    if( st == ACN_OK ) st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    const size_t mine = acn_shard_tile_count( count, rank, world ), padded = acn_shard_tile_padded( count, world );
    if( padded > mine ) HIP_TRY( hipMemsetAsync( ( double* )d_part + 3 * mine, 0, sizeof( double ) * 3 * ( padded - mine ), c.stream ) );
    if( mine )
    {
        if( h->d_shard_pos.grow( sizeof( double ) * 2 * mine ) ) return ACN_ERR_DEVICE;
        hipLaunchKernelGGL( k_lane_gather, dim3( ( unsigned )( ( mine + 255 ) / 256 ) ), dim3( 256 ), 0, c.stream,
                            ( const double* )nullptr, first, ( uint64_t )h->dev.prm.image_width, mine, ( int )world, ( int )rank, h->d_shard_pos.get() );
        HIP_TRY( hipGetLastError() );
        if( ( st = render_dispatch( h, primary_positions( h->d_shard_pos.get() ), mine, ( double* )d_part, &c.opts, c.stream ) ) != ACN_OK ) return st;
    }
    return call_end( c );
}

extern "C" int acn_shard_unpack_dev( acn_scene_handle* h, const void* d_gathered, size_t count, uint32_t world, void* d_frame,
                                     const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( count && ( !d_gathered || !d_frame ) ) || world == 0 ) return fail( ACN_ERR_ARG, "bad argument" );
    if( count == 0 ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    hipLaunchKernelGGL( k_shard_unpack, dim3( ( unsigned )( ( count + 255 ) / 256 ) ), dim3( 256 ), 0, c.stream,
                        ( const double* )d_gathered, count, world, acn_shard_tile_padded( count, world ), ( double* )d_frame );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_last_kernel_ms( acn_scene_handle* h, double* trace_ms )
{
    if( !h || !trace_ms || !h->timed ) return fail( ACN_ERR_ARG, "no timed launch" );
    HIP_TRY( hipSetDevice( h->device ) );
    HIP_TRY( hipEventSynchronize( h->run.ev1.get() ) );
    float ms = 0;
    HIP_TRY( hipEventElapsedTime( &ms, h->run.ev0.get(), h->run.ev1.get() ) );
    *trace_ms = ms;
    return ACN_OK;
}

/* the runners of the last call: the lanes it ran on, or the handle's own */
static std::vector< const PipeRun* > last_runs( const acn_scene_handle* h )
{
    std::vector< const PipeRun* > runs;
    for( int k = 0; h->used_lanes && k < h->lanes_used; k++ ) runs.push_back( h->lanes[ k ].get() );
    return h->used_lanes ? runs : std::vector< const PipeRun* >{ &h->run };
}

extern "C" int acn_last_stage_ms( acn_scene_handle* h, double* out, int n )
{
    if( !h || !out || n < 0 || n > ACN_LAST_N || !h->timed ) return fail( ACN_ERR_ARG, "no timed launch" );
    HIP_TRY( hipSetDevice( h->device ) );
    HIP_TRY( hipEventSynchronize( h->run.ev1.get() ) );
    double ms[ 4 ] = { 0, 0, 0, 0 };
    size_t queue_cap = 0, ws_bytes = 0, ws_allocs = 0;
    for( const PipeRun* l : last_runs( h ) )   /* stage times: summed over the concurrent lanes of the call */
    {
        queue_cap += l->ws.cap[ WQ_HARD_SHADOW ]; ws_bytes += l->ws.bytes; ws_allocs += l->ws.allocs;
        for( size_t i = 0; i < l->events_used; i++ )
        {
            float t = 0;
            HIP_TRY( hipEventElapsedTime( &t, l->events[ i ].a.get(), l->events[ i ].b.get() ) );
            ms[ l->events[ i ].stage ] += t;
        }
    }
    float total = 0;
    HIP_TRY( hipEventElapsedTime( &total, h->run.ev0.get(), h->run.ev1.get() ) );
    const RunStats& s = h->run.stats;
    double v[ ACN_LAST_N ];
    v[ ACN_LAST_WALK_MS ] = ms[ 0 ]; v[ ACN_LAST_SHADE_MS ] = ms[ 1 ]; v[ ACN_LAST_FINALIZE_MS ] = ms[ 2 ]; v[ ACN_LAST_HARD_MS ] = ms[ 3 ];
    v[ ACN_LAST_TOTAL_MS ] = total;
    v[ ACN_LAST_WALK_LAUNCHES ] = ( double )s.launches[ 0 ]; v[ ACN_LAST_SHADE_LAUNCHES ] = ( double )s.launches[ 1 ];
    v[ ACN_LAST_FINALIZE_LAUNCHES ] = ( double )s.launches[ 2 ]; v[ ACN_LAST_HARD_LAUNCHES ] = ( double )s.launches[ 3 ];
    v[ ACN_LAST_CHUNKS ] = ( double )s.chunks; v[ ACN_LAST_RETRIES ] = ( double )s.retries; v[ ACN_LAST_LEVELS ] = ( double )s.levels;
    v[ ACN_LAST_PEAK_TASKS ] = ( double )s.peak_tasks; v[ ACN_LAST_PEAK_CHILDREN ] = ( double )s.peak_children; v[ ACN_LAST_QUEUE_CAP ] = ( double )queue_cap;
    v[ ACN_LAST_HARD_RAYS ] = ( double )s.hard_rays; v[ ACN_LAST_WALK_RAYS ] = ( double )s.walk_rays; v[ ACN_LAST_PATH_HITS ] = ( double )s.shade_hit_recs;
    v[ ACN_LAST_HOST_SYNCS ] = ( double )s.host_syncs; v[ ACN_LAST_WALK_STEPS ] = ( double )s.walk_steps; v[ ACN_LAST_FLAGS ] = ( double )s.flags_seen;
    v[ ACN_LAST_PRIVATE_RAYS ] = ( double )s.private_rays; v[ ACN_LAST_PROBE_RAYS ] = ( double )s.probe_rays;
    v[ ACN_LAST_WORKSPACE_BYTES ] = ( double )ws_bytes; v[ ACN_LAST_WORKSPACE_ALLOCS ] = ( double )ws_allocs;
    for( int k = 0; k < n; k++ ) out[ k ] = v[ k ];
    return ACN_OK;
}

extern "C" int acn_last_counters( acn_scene_handle* h, uint64_t* out, int n )
{
    if( !h || !out || n < 0 || n > ACN_CNT_SLOTS ) return fail( ACN_ERR_ARG, "bad argument" );
    HIP_TRY( hipSetDevice( h->device ) );
    unsigned long long c[ ACN_CNT_SLOTS ], sum[ ACN_CNT_SLOTS ];
    for( int k = 0; k < ACN_CNT_SLOTS; k++ ) sum[ k ] = 0;
    for( const PipeRun* l : last_runs( h ) )
    {
        HIP_TRY( hipMemcpy( c, l->d_counters.get(), sizeof( c ), hipMemcpyDeviceToHost ) );
        for( int k = 0; k < ACN_CNT_SLOTS; k++ ) sum[ k ] += c[ k ];
    }
    for( int k = 0; k < n; k++ ) out[ k ] = k < ACN_CNT_SLOTS ? sum[ k ] : 0;
    return ACN_OK;
}
