/* k_stage.hip -- test seam: one shading kernel of the pipeline alone (acn_run_stage, include/actinon_hip.h), and the specular walk of
 * a level alone (acn_run_stage_walk, at the end of the file): the passes of k_walk in render_chunk's loop, on rays or camera positions
 * of the caller, with the arrangement of the walk -- passes, private limit, stack slots, fetch batch, grid -- as arguments.
 *
 * No device code: the unit launches k_shade_hits, k_shade, k_hard_shadow and k_hard_path through the wrappers of acn_launch.h, as
 * render_chunk does, on queues it owns for the length of the call.  The caller's records are the input queue; the counter block is zeroed and the input count set
 * here; every output queue is sized by acn_stage_check (acn_stage_host.h) so that the kernel cannot fill it, and comes back whole,
 * dead slots included (pixel 0xFFFFFFFF: the ends of the waves' reservations).  k_shade never asks which class a task's sample count
 * belongs to, so the same task runs on 64, 16, 4 and 1 lanes: the index list goes where the kernel of `cls` reads it. */
#include <hip/hip_runtime.h>
#include <cstddef>
#include "acn_device.h"   /* a ray unit: the whole tracer */
#include "acn_handle.h"
#include "acn_stage_host.h"

#define ACN_STAGE_SAME( A, B, M ) static_assert( offsetof( A, M ) == offsetof( B, M ), "acn_stage_host.h restates " #B )
static_assert( sizeof( acn_stage_hitrec ) == sizeof( HitRec ) && sizeof( acn_stage_dtask ) == sizeof( DTask ), "acn_stage_host.h restates the records" );
ACN_STAGE_SAME( acn_stage_hitrec, HitRec, exit_obj ); ACN_STAGE_SAME( acn_stage_hitrec, HitRec, enter_obj );
ACN_STAGE_SAME( acn_stage_hitrec, HitRec, depth );    ACN_STAGE_SAME( acn_stage_hitrec, HitRec, pixel );
ACN_STAGE_SAME( acn_stage_dtask, DTask, diffuse_intensity ); ACN_STAGE_SAME( acn_stage_dtask, DTask, depth ); ACN_STAGE_SAME( acn_stage_dtask, DTask, pixel );
static_assert( sizeof( acn_stage_hardshadow ) == sizeof( HardShadow ) && sizeof( acn_stage_hardpath ) == sizeof( HardPath ), "acn_stage_host.h restates the records" );
ACN_STAGE_SAME( acn_stage_hardshadow, HardShadow, limit ); ACN_STAGE_SAME( acn_stage_hardshadow, HardShadow, pixel ); ACN_STAGE_SAME( acn_stage_hardshadow, HardShadow, pad );
ACN_STAGE_SAME( acn_stage_hardpath, HardPath, depth ); ACN_STAGE_SAME( acn_stage_hardpath, HardPath, pixel ); ACN_STAGE_SAME( acn_stage_hardpath, HardPath, resume );
static_assert( ACN_STAGE_RESUME_FLAG == ACN_RESUME_FLAG, "acn_stage_host.h restates the resume flag" );
static_assert( sizeof( acn_stage_raytask ) == sizeof( RayTask ), "acn_stage_host.h restates the records" );
ACN_STAGE_SAME( acn_stage_raytask, RayTask, T ); ACN_STAGE_SAME( acn_stage_raytask, RayTask, intensity );
ACN_STAGE_SAME( acn_stage_raytask, RayTask, depth ); ACN_STAGE_SAME( acn_stage_raytask, RayTask, pixel );
static_assert( ACN_STAGE_DEAD == ACN_INVALID && ACN_ORDER_SHIFT == 8, "acn_stage_host.h restates the dead mark and the tiles of the order of work" );

static acn_stage_scene stage_scene( const acn_scene_handle* h )
{
    acn_stage_scene sc;
    sc.n_nodes = h->dev.n_nodes; sc.n_lights = ( uint32_t )h->scene.n_lights;
    sc.direct_samples = h->dev.prm.direct_samples; sc.path_samples = h->dev.prm.path_samples;
    sc.trace_min_intensity = h->dev.prm.trace_min_intensity;
    return sc;
}

extern "C" int acn_stage_info( acn_scene_handle* h, uint32_t* out, int n )
{
    if( !h || !out || n < 0 || n > ACN_STAGE_INFO_WORDS ) return fail( ACN_ERR_ARG, "acn_stage_info: bad argument" );
    const uint32_t v[ ACN_STAGE_INFO_WORDS ] = { ( uint32_t )sizeof( RayTask ), ( uint32_t )sizeof( DTask ), ( uint32_t )sizeof( HitRec ), ( uint32_t )sizeof( HardShadow ),
        ( uint32_t )sizeof( HardPath ), ( uint32_t )QC_N, h->dev.class0_min, h->dev.n_nodes, ( uint32_t )h->scene.n_lights,
        ( h->scene.prune ? 1u : 0u ) | ( h->scene.leaf_lights ? 2u : 0u ) | ( h->scene.lds_bytes != 0 ? 4u : 0u ) };
    for( int k = 0; k < n; k++ ) out[ k ] = v[ k ];
    return ACN_OK;
}

extern "C" int acn_stage_plan( acn_scene_handle* h, const acn_stage_args* args, acn_stage_caps* caps )
{
    std::string msg;
    const int st = acn_stage_check( h != nullptr, args, h ? stage_scene( h ) : acn_stage_scene{}, caps, &msg );
    return st == ACN_OK ? ACN_OK : fail( st, "acn_run_stage: " + msg );
}

/* The queues of one path level, owned for the length of a stage call; both seams run their kernels on one of these.  make(): every
 * queue of a level exists (a kernel closes the reservations of all its queues), of its capacity in the plan and one record at least
 * (tasks: n_tasks records, stacks: n_stacks, accum: n_accum pixels); what no kernel writes reads as dead (0xFF: pixel ACN_INVALID in every record, a dead index entry); the counter block (behind it the input count of k_shade_hits),
 * accum and the counters are zero; q, f and s are what render_chunk passes, for these queues, the handle's tunables and the seam's
 * flags.  The seam puts its input into the stream behind the fill, launches, and finish() waits, reads the counter block and refuses a
 * run that raised overflow flags. */
struct StageLevel
{
    struct Buf { void* d; size_t bytes; }; struct Out { void* dst; Buf from; };
    DevCopies dc;
    Buf tasks, idx[ ACN_NCLASS ], rays[ 2 ], children, hard_shadow, hard_path, accum;
    uint32_t* d_counts; unsigned long long* d_counters;
    LevelQ q; KernelFlags f; SceneArgs s;

    int make( const acn_scene_handle* h, const acn_stage_caps& cap, uint32_t n_tasks, size_t n_stacks, uint32_t n_accum, uint32_t flags, hipStream_t stream )
    {
        auto buf = [ this ]( uint32_t n, size_t rec ) { const size_t bytes = ( size_t )( n ? n : 1u ) * rec; return Buf{ dc.make( nullptr, bytes ), bytes }; };
        tasks = buf( n_tasks, sizeof( DTask ) );
        for( Buf& b : idx ) b = buf( cap.cap_tasks, sizeof( uint32_t ) );
        for( Buf& b : rays ) b = buf( cap.cap_rays, sizeof( RayTask ) );
        children = buf( cap.cap_children, sizeof( HitRec ) ); hard_shadow = buf( cap.cap_hard_shadow, sizeof( HardShadow ) ); hard_path = buf( cap.cap_hard_path, sizeof( HardPath ) );
        accum = buf( n_accum, sizeof( unsigned long long ) * 3 );
        RayTask* d_stacks = ( RayTask* )dc.make( nullptr, n_stacks * sizeof( RayTask ) );
        const size_t b_counts = sizeof( uint32_t ) * ( QC_N + 1 ), b_counters = sizeof( unsigned long long ) * ACN_CNT_SLOTS;
        d_counts = ( uint32_t* )dc.make( nullptr, b_counts ); d_counters = ( unsigned long long* )dc.make( nullptr, b_counters );
        const Buf* const queues[] = { &tasks, &idx[ 0 ], &idx[ 1 ], &idx[ 2 ], &idx[ 3 ], &rays[ 0 ], &rays[ 1 ], &children, &hard_shadow, &hard_path };
        bool made = accum.d && d_stacks && d_counts && d_counters;
        for( const Buf* b : queues ) made = made && b->d;
        if( !made ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
        for( const Buf* b : queues ) HIP_TRY( hipMemsetAsync( b->d, 0xFF, b->bytes, stream ) );
        HIP_TRY( hipMemsetAsync( d_counts, 0, b_counts, stream ) );
        HIP_TRY( hipMemsetAsync( accum.d, 0, accum.bytes, stream ) );
        HIP_TRY( hipMemsetAsync( d_counters, 0, b_counters, stream ) );

        memset( &q, 0, sizeof( q ) );
        q.tasks = ( DTask* )tasks.d; for( int k = 0; k < ACN_NCLASS; k++ ) q.idx[ k ] = ( uint32_t* )idx[ k ].d;
        q.task_cap = cap.cap_tasks; q.child_cap = cap.cap_children; q.hs_cap = cap.cap_hard_shadow; q.hard_cap = cap.cap_hard_path; q.ray_cap = cap.cap_rays;
        q.children = ( HitRec* )children.d; q.hard_shadow = ( HardShadow* )hard_shadow.d; q.hard_path = ( HardPath* )hard_path.d;
        q.rays[ 0 ] = ( RayTask* )rays[ 0 ].d; q.rays[ 1 ] = ( RayTask* )rays[ 1 ].d; q.stacks = d_stacks;
        q.counts = d_counts; q.prev_children = d_counts + QC_N;
        q.grid = cap.grid; q.shade_grid = cap.grid; q.walk_grid = cap.grid;
        q.fetch_walk = h->tun.fetch_walk; q.fetch_hard = h->tun.fetch_hard; q.fetch_shade = h->tun.fetch_shade; q.private_limit = h->tun.private_limit;
        q.shard_rank = 0u; q.shard_world = 1u; q.emit_terms = flags & ACN_STAGE_NO_EMIT_TERMS ? 0u : 1u;
        f.count = ( flags & ACN_STAGE_COUNT_WORK ) != 0; f.lds_nodes = h->scene.lds_bytes != 0 && !( flags & ACN_STAGE_GLOBAL_NODES );
        f.leaf_lights = h->scene.leaf_lights && !( flags & ACN_STAGE_NO_LEAF_LIGHTS );
        f.prune = h->scene.prune && !( flags & ACN_STAGE_NO_PRUNE );
        DevScene dev = h->dev;
        dev.flags = d_counts + QC_FLAGS;
        s = scene_args( dev, h->scene );
        return ACN_OK;
    }
    /* seam: the call's name; cause: what an overflow of this seam's queues means.  work: where the launch's work counters go (the
     * handle's, for acn_stage_last_counters: never what acn_last_counters reads) */
    int finish( hipStream_t stream, uint32_t* out_counts, unsigned long long* work, const char* seam, const char* cause )
    {
        HIP_TRY( hipGetLastError() );
        HIP_TRY( hipStreamSynchronize( stream ) );
        uint32_t counts[ QC_N ];
        int st = DevCopies::fetch( counts, d_counts, sizeof( counts ) );
        if( st != ACN_OK ) return st;
        if( ( st = DevCopies::fetch( work, d_counters, sizeof( unsigned long long ) * ( CNT_N + 2 ) ) ) != ACN_OK ) return st;
        if( out_counts ) memcpy( out_counts, counts, sizeof( counts ) );
        if( counts[ QC_FLAGS ] & ( ACN_FLAGS_CHUNK_LOST | ACN_FLAG_STACK_OVERFLOW ) )
            return fail( ACN_ERR_DEVICE, std::string( seam ) + ": the kernel raised overflow flags " + std::to_string( counts[ QC_FLAGS ] ) + ": " + cause );
        return ACN_OK;
    }
    static int fetch( std::initializer_list< Out > outs )
    {
        int st;
        for( const Out& o : outs ) if( o.dst && ( st = DevCopies::fetch( o.dst, o.from.d, o.from.bytes ) ) != ACN_OK ) return st;
        return ACN_OK;
    }
};

extern "C" int acn_run_stage( acn_scene_handle* h, const acn_stage_args* a, const acn_stage_out* out )
{
    acn_stage_caps cap;
    if( h ) memset( h->stage_counters, 0, sizeof( h->stage_counters ) );   /* "of the last stage call": one that is refused or fails reports none */
    int st = acn_stage_plan( h, a, &cap );
    if( st != ACN_OK ) return st;
    if( !out ) return fail( ACN_ERR_ARG, "acn_run_stage: null argument: out" );
    Call c( nullptr );
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    const bool shade = a->stage == ACN_STAGE_SHADE, split = a->stage == ACN_STAGE_SHADE_HITS;
    const bool hs_in = a->stage == ACN_STAGE_HARD_SHADOW, hp_in = a->stage == ACN_STAGE_HARD_PATH;

    StageLevel lv;   /* SHADE reads tasks[ n ] through idx[ cls ][ n_index ] */
    if( ( st = lv.make( h, cap, shade ? a->n : cap.cap_tasks, 0, a->n, a->flags, c.stream ) ) != ACN_OK ) return st;
    LevelQ& q = lv.q;
    q.shard_rank = shade ? a->shard_rank : 0u; q.shard_world = shade && a->shard_world ? a->shard_world : 1u;

    /* the caller's records are the input queue, whole; SHADE: the index list goes where the kernel of `cls` reads it */
    const StageLevel::Buf& in = shade ? lv.tasks : split ? lv.children : hs_in ? lv.hard_shadow : lv.hard_path;
    HIP_TRY( hipMemcpyAsync( in.d, a->in, in.bytes, hipMemcpyHostToDevice, c.stream ) );
    if( shade ) HIP_TRY( hipMemcpyAsync( lv.idx[ a->cls ].d, a->index, lv.idx[ a->cls ].bytes, hipMemcpyHostToDevice, c.stream ) );
    const uint32_t n_in = shade ? a->n_index : a->n;
    /* where the kernel reads how much input it has: its class list's mark, the previous level's children, its own queue's mark */
    uint32_t* const d_n_in = shade ? q.counts + QC_CLASS0 + a->cls : hs_in ? q.counts + QC_HARD_SHADOW : hp_in ? q.counts + QC_HARD_PATH : q.counts + QC_N;
    HIP_TRY( hipMemcpyAsync( d_n_in, &n_in, sizeof( n_in ), hipMemcpyHostToDevice, c.stream ) );
    HIP_TRY( hipStreamSynchronize( c.stream ) );   /* the caller's memory and n_in are read */

    unsigned long long* const d_accum = ( unsigned long long* )lv.accum.d;
    const auto launch_shade = a->cls == 0 ? acn_launch_shade64 : a->cls == 1 ? acn_launch_shade16 : a->cls == 2 ? acn_launch_shade4 : acn_launch_shade1;
    if( shade )      launch_shade( lv.f, q, c.stream, lv.s, d_accum, lv.d_counters );
    else if( hs_in ) acn_launch_hard_shadow( lv.f, q, machine_lds_bytes( h->scene ), c.stream, lv.s, d_accum, lv.d_counters );
    else if( hp_in ) acn_launch_hard_path( lv.f, q, machine_lds_bytes( h->scene ), c.stream, lv.s, d_accum, lv.d_counters );
    else             acn_launch_shade_hits( lv.f.count, q, c.stream, lv.s, d_accum, lv.d_counters );
    if( ( st = lv.finish( c.stream, out->counts, h->stage_counters, "acn_run_stage", "a queue the plan sized was too small" ) ) != ACN_OK ) return st;
    return StageLevel::fetch( {
        { split ? out->tasks : nullptr, lv.tasks },
        { split ? ( void* )out->idx[ 0 ] : nullptr, lv.idx[ 0 ] }, { split ? ( void* )out->idx[ 1 ] : nullptr, lv.idx[ 1 ] },
        { split ? ( void* )out->idx[ 2 ] : nullptr, lv.idx[ 2 ] }, { split ? ( void* )out->idx[ 3 ] : nullptr, lv.idx[ 3 ] },
        { split ? out->rays : nullptr, lv.rays[ 0 ] }, { shade || hp_in ? out->children : nullptr, lv.children },
        { shade || split || hs_in ? out->hard_shadow : nullptr, lv.hard_shadow }, { shade ? out->hard_path : nullptr, lv.hard_path }, { out->accum, lv.accum } } );
}

extern "C" int acn_stage_last_counters( acn_scene_handle* h, uint64_t* out, int n )
{
    if( !h || !out || n < 0 || n > CNT_N + 2 ) return fail( ACN_ERR_ARG, "acn_stage_last_counters: bad argument" );
    for( int k = 0; k < n; k++ ) out[ k ] = h->stage_counters[ k ];
    return ACN_OK;
}

/* ---- the walk ---- */

extern "C" int acn_stage_walk_plan( acn_scene_handle* h, const acn_stage_walk_args* args, acn_stage_caps* caps )
{
    std::string msg;
    const int st = acn_stage_walk_check( h != nullptr, args, h ? stage_scene( h ) : acn_stage_scene{}, caps, &msg );
    return st == ACN_OK ? ACN_OK : fail( st, "acn_run_stage_walk: " + msg );
}

extern "C" int acn_run_stage_walk( acn_scene_handle* h, const acn_stage_walk_args* a, const acn_stage_out* out )
{
    acn_stage_caps cap;
    if( h ) memset( h->stage_counters, 0, sizeof( h->stage_counters ) );
    int st = acn_stage_walk_plan( h, a, &cap );
    if( st != ACN_OK ) return st;
    if( !out ) return fail( ACN_ERR_ARG, "acn_run_stage_walk: null argument: out" );
    Call c( nullptr );
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;

    StageLevel lv;   /* (the kernels take every queue of a level; what the walk never touches -- children, hard paths -- is one record) */
    if( ( st = lv.make( h, cap, cap.cap_tasks, ( size_t )cap.grid * 4u * a->stack_cap, a->n, a->flags, c.stream ) ) != ACN_OK ) return st;
    LevelQ& q = lv.q;
    q.stack_cap = a->stack_cap; q.stack_use = a->stack_use ? a->stack_use : a->stack_cap;
    q.fetch_walk = a->fetch; q.private_limit = a->private_limit;
    double* d_pos = nullptr;
    if( a->camera && a->pos_xy && !( d_pos = ( double* )lv.dc.make( a->pos_xy, sizeof( double ) * 2 * a->n ) ) ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    if( !a->camera )
    {
        /* generation 0 of the level: the caller's rays, and their number where pass 0 reads it (room_rays >= n: they fit) */
        HIP_TRY( hipMemcpyAsync( q.rays[ 0 ], a->in, ( size_t )a->n * sizeof( RayTask ), hipMemcpyHostToDevice, c.stream ) );
        HIP_TRY( hipMemcpyAsync( q.counts + QC_GEN, &a->n, sizeof( uint32_t ), hipMemcpyHostToDevice, c.stream ) );
    }
    HIP_TRY( hipStreamSynchronize( c.stream ) );   /* the caller's memory is read */

    /* the camera form: the order of work of a render call over the n positions, every slot of its tiles in one chunk */
    TileOrder order = {};
    order.n = a->n; order.n_tiles = acn_tile_order( a->n, ACN_ORDER_SHIFT, &order.mul ); order.sample_stride = 0;
    const uint32_t n_cam = a->camera ? acn_stage_walk_slots( a ) : 0u;
    for( uint32_t pass = 0; pass < a->passes; pass++ )
    {
        const WalkLaunch w = { pass, pass + 1 == a->passes, d_pos, ( size_t )a->first_pixel, 0u, pass == 0 ? n_cam : 0u, order, machine_lds_bytes( h->scene ),
                               ( unsigned long long* )lv.accum.d, lv.d_counters };
        acn_launch_walk( lv.f, q, w, c.stream, lv.s );
        HIP_TRY( hipGetLastError() );
    }
    if( ( st = lv.finish( c.stream, out->counts, h->stage_counters, "acn_run_stage_walk", "room_rays is below what the walk traced" ) ) != ACN_OK ) return st;
    return StageLevel::fetch( {
        { out->tasks, lv.tasks },
        { ( void* )out->idx[ 0 ], lv.idx[ 0 ] }, { ( void* )out->idx[ 1 ], lv.idx[ 1 ] }, { ( void* )out->idx[ 2 ], lv.idx[ 2 ] }, { ( void* )out->idx[ 3 ], lv.idx[ 3 ] },
        { out->rays, lv.rays[ a->passes & 1 ] }, { out->hard_shadow, lv.hard_shadow }, { out->accum, lv.accum } } );
}
