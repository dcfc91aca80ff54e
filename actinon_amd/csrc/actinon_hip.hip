/* actinon_hip.hip -- libactinon_hip.so (gfx950 only): the handle's life cycle, the workspace, the wavefront pipeline with its concurrent
 * lanes, and the entry points of include/actinon_hip.h that are the pipeline's own.  Every other entry point: acn_calls.hip. */
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


#include "acn_handle.h"

/* ------------------------------------------------------------------------------------------------------------------ */
/* error plumbing (fail and HIP_TRY: acn_handle.h) */
thread_local std::string g_last_error;
extern "C" const char* acn_last_error( void ) { return g_last_error.c_str(); }

/* bytes per record of each queue (WQ_*) */
static const size_t wq_bytes[ WQ_N ] = { sizeof( DTask ) + ACN_NCLASS * sizeof( uint32_t ), sizeof( HitRec ), sizeof( HardShadow ), sizeof( HardPath ), 2 * sizeof( RayTask ) };
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
    if( ( st = grow_device( ( void** )&h->d_accum, &h->accum_bytes, sizeof( unsigned long long ) * 3 * n ) ) != ACN_OK ) return st;
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
    if( opts->cancel && *opts->cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many positions in one call" );
    h->seeded = prim.rays != nullptr;
    int linear = ( opts->flags & ACN_OPT_LINEAR_OUT ) ? 1 : 0;
    h->count_work = ( opts->flags & ACN_OPT_COUNT_WORK ) || h->tun.count_work;
    h->shard_rank = 0; h->shard_world = 1;
    if( opts->shard_mode == ACN_SHARD_SAMPLES && opts->shard_world > 1 )
    {
        if( opts->shard_rank >= opts->shard_world ) return fail( ACN_ERR_ARG, "shard_rank >= shard_world" );
        h->shard_rank = opts->shard_rank; h->shard_world = opts->shard_world;
    }
    else if( opts->shard_mode > ACN_SHARD_SAMPLES ) return fail( ACN_ERR_ARG, "unknown shard_mode" );
    h->stage_timing = ( opts->flags & ACN_OPT_STAGE_TIMING ) || h->tun.stage_timing;
    int st = learn_rates( h, prim, n, stream, n, h->walk_grid > h->grid ? h->walk_grid : h->grid );
    if( st != ACN_OK ) return st;
    /* (shard fields again: the learning pass renders unsharded) */
    if( opts->shard_mode == ACN_SHARD_SAMPLES && opts->shard_world > 1 ) { h->shard_rank = opts->shard_rank; h->shard_world = opts->shard_world; }
    st = ensure_workspace( h, n );
    if( st != ACN_OK ) return st;
    if( ( st = grow_device( ( void** )&h->d_accum, &h->accum_bytes, sizeof( unsigned long long ) * 3 * n ) ) != ACN_OK ) return st;
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
        if( opts->cancel && *opts->cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
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
    acn_render_opts lane_opts = *opts;
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
                int st = grow_device( ( void** )&l->d_lane_in, &l->lane_in_bytes, sizeof( double ) * ( prim.rays ? 6 : 2 ) * cnt );
                if( st == ACN_OK ) st = grow_device( ( void** )&l->d_lane_out, &l->lane_out_bytes, sizeof( double ) * 3 * cnt );
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

/* one pipeline run on the handle itself, or the concurrent lanes */
int render_dispatch( acn_scene_handle* h, const Primary& prim, size_t n, double* d_out_rgb, const acn_render_opts* opts, hipStream_t stream )
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
    Call c( opts );
    if( !h || ( count && !d_part ) || world == 0 || rank >= world ) return fail( ACN_ERR_ARG, "bad argument" );
    int st = pixel_range_check( h, first, count );
    if( st == ACN_OK ) st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    const size_t mine = acn_shard_tile_count( count, rank, world ), padded = acn_shard_tile_padded( count, world );
    if( padded > mine ) HIP_TRY( hipMemsetAsync( ( double* )d_part + 3 * mine, 0, sizeof( double ) * 3 * ( padded - mine ), c.stream ) );
    if( mine )
    {
        if( ( st = grow_device( ( void** )&h->d_shard_pos, &h->shard_pos_bytes, sizeof( double ) * 2 * mine ) ) != ACN_OK ) return st;
        hipLaunchKernelGGL( k_lane_gather, dim3( ( unsigned )( ( mine + 255 ) / 256 ) ), dim3( 256 ), 0, c.stream,
                            ( const double* )nullptr, first, ( uint64_t )h->dev.prm.image_width, mine, ( int )world, ( int )rank, h->d_shard_pos );
        HIP_TRY( hipGetLastError() );
        if( ( st = render_dispatch( h, primary_positions( h->d_shard_pos ), mine, ( double* )d_part, &c.opts, c.stream ) ) != ACN_OK ) return st;
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
