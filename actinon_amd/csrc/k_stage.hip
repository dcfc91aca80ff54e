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

/* the kernel of one size class (the four wrappers carry their class: the list it reads, its cursor) */
void acn_launch_shade( int cls, KernelFlags f, const LevelQ& q, hipStream_t stream, const SceneArgs& s, unsigned long long* accum, unsigned long long* counters )
{
    if( cls == 0 )      acn_launch_shade64( f, q, stream, s, accum, counters );
    else if( cls == 1 ) acn_launch_shade16( f, q, stream, s, accum, counters );
    else if( cls == 2 ) acn_launch_shade4( f, q, stream, s, accum, counters );
    else                acn_launch_shade1( f, q, stream, s, accum, counters );
}

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

extern "C" int acn_run_stage( acn_scene_handle* h, const acn_stage_args* a, const acn_stage_out* out )
{
    acn_stage_caps cap;
    int st = acn_stage_plan( h, a, &cap );
    if( st != ACN_OK ) return st;
    if( !out ) return fail( ACN_ERR_ARG, "acn_run_stage: null argument: out" );
    Call c( nullptr );
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    const bool shade = a->stage == ACN_STAGE_SHADE, split = a->stage == ACN_STAGE_SHADE_HITS;
    const bool hs_in = a->stage == ACN_STAGE_HARD_SHADOW, hp_in = a->stage == ACN_STAGE_HARD_PATH;

    /* the queues of one level.  Every queue exists (a kernel closes the reservations of all its queues), one record at least */
    auto bytes_of = []( uint32_t n, size_t rec ) { return ( size_t )( n ? n : 1u ) * rec; };
    const uint32_t n_tasks_in = shade ? a->n : 0u;                       /* SHADE reads tasks[ n ] through idx[ cls ][ n_index ] */
    const size_t b_tasks = bytes_of( shade ? n_tasks_in : cap.cap_tasks, sizeof( DTask ) ), b_idx = bytes_of( cap.cap_tasks, sizeof( uint32_t ) );
    const size_t b_rays = bytes_of( cap.cap_rays, sizeof( RayTask ) ), b_children = bytes_of( cap.cap_children, sizeof( HitRec ) );
    const size_t b_hs = bytes_of( cap.cap_hard_shadow, sizeof( HardShadow ) ), b_hp = bytes_of( cap.cap_hard_path, sizeof( HardPath ) );
    const size_t b_counts = sizeof( uint32_t ) * ( QC_N + 1 ), b_accum = sizeof( unsigned long long ) * 3 * a->n;
    DevCopies dc;
    DTask* d_tasks = ( DTask* )dc.make( shade ? a->in : nullptr, b_tasks );
    uint32_t* d_idx[ ACN_NCLASS ];
    for( int k = 0; k < ACN_NCLASS; k++ ) d_idx[ k ] = ( uint32_t* )dc.make( shade && ( uint32_t )k == a->cls ? a->index : nullptr, b_idx );
    RayTask* d_rays = ( RayTask* )dc.make( nullptr, b_rays );
    HitRec* d_children = ( HitRec* )dc.make( split ? a->in : nullptr, b_children );
    HardShadow* d_hs = ( HardShadow* )dc.make( hs_in ? a->in : nullptr, b_hs );
    HardPath* d_hp = ( HardPath* )dc.make( hp_in ? a->in : nullptr, b_hp );
    uint32_t* d_counts = ( uint32_t* )dc.make( nullptr, b_counts );      /* the level's block, and behind it the input count of k_shade_hits */
    unsigned long long* d_accum = ( unsigned long long* )dc.make( nullptr, b_accum );
    unsigned long long* d_counters = ( unsigned long long* )dc.make( nullptr, sizeof( unsigned long long ) * ACN_CNT_SLOTS );
    bool made = d_tasks && d_rays && d_children && d_hs && d_hp && d_counts && d_accum && d_counters;
    for( int k = 0; k < ACN_NCLASS; k++ ) made = made && d_idx[ k ];
    if( !made ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );

    /* what the kernel does not write reads as dead: 0xFF is pixel ACN_INVALID in every record and a dead index entry */
    if( !shade ) HIP_TRY( hipMemsetAsync( d_tasks, 0xFF, b_tasks, c.stream ) );
    for( int k = 0; k < ACN_NCLASS; k++ ) if( !( shade && ( uint32_t )k == a->cls ) ) HIP_TRY( hipMemsetAsync( d_idx[ k ], 0xFF, b_idx, c.stream ) );
    HIP_TRY( hipMemsetAsync( d_rays, 0xFF, b_rays, c.stream ) );
    if( !split ) HIP_TRY( hipMemsetAsync( d_children, 0xFF, b_children, c.stream ) );
    if( !hs_in ) HIP_TRY( hipMemsetAsync( d_hs, 0xFF, b_hs, c.stream ) );
    if( !hp_in ) HIP_TRY( hipMemsetAsync( d_hp, 0xFF, b_hp, c.stream ) );
    HIP_TRY( hipMemsetAsync( d_counts, 0, b_counts, c.stream ) );
    HIP_TRY( hipMemsetAsync( d_accum, 0, b_accum, c.stream ) );
    HIP_TRY( hipMemsetAsync( d_counters, 0, sizeof( unsigned long long ) * ACN_CNT_SLOTS, c.stream ) );
    const uint32_t n_in = shade ? a->n_index : a->n;
    /* where the kernel reads how much input it has: its class list's mark, the previous level's children, its own queue's mark */
    uint32_t* const d_n_in = shade ? d_counts + QC_CLASS0 + a->cls : hs_in ? d_counts + QC_HARD_SHADOW : hp_in ? d_counts + QC_HARD_PATH : d_counts + QC_N;
    HIP_TRY( hipMemcpyAsync( d_n_in, &n_in, sizeof( n_in ), hipMemcpyHostToDevice, c.stream ) );
    HIP_TRY( hipStreamSynchronize( c.stream ) );   /* n_in leaves the stack */

    LevelQ q;
    memset( &q, 0, sizeof( q ) );
    q.tasks = d_tasks; for( int k = 0; k < ACN_NCLASS; k++ ) q.idx[ k ] = d_idx[ k ];
    q.task_cap = cap.cap_tasks; q.child_cap = cap.cap_children; q.hs_cap = cap.cap_hard_shadow; q.hard_cap = cap.cap_hard_path; q.ray_cap = cap.cap_rays;
    q.children = d_children; q.hard_shadow = d_hs; q.hard_path = d_hp; q.rays[ 0 ] = d_rays; q.rays[ 1 ] = d_rays;
    q.counts = d_counts; q.prev_children = d_counts + QC_N;
    q.grid = cap.grid; q.shade_grid = cap.grid; q.walk_grid = cap.grid;
    q.fetch_walk = h->tun.fetch_walk; q.fetch_hard = h->tun.fetch_hard; q.fetch_shade = h->tun.fetch_shade; q.private_limit = h->tun.private_limit;
    q.shard_rank = shade ? a->shard_rank : 0u; q.shard_world = shade && a->shard_world ? a->shard_world : 1u;
    q.emit_terms = a->flags & ACN_STAGE_NO_EMIT_TERMS ? 0u : 1u;
    KernelFlags f;
    f.count = false; f.lds_nodes = h->scene.lds_bytes != 0;
    f.leaf_lights = h->scene.leaf_lights && !( a->flags & ACN_STAGE_NO_LEAF_LIGHTS );
    f.prune = h->scene.prune && !( a->flags & ACN_STAGE_NO_PRUNE );
    DevScene dev = h->dev;
    dev.flags = d_counts + QC_FLAGS;
    const SceneArgs s = scene_args( dev, h->scene );
    if( shade )      acn_launch_shade( ( int )a->cls, f, q, c.stream, s, d_accum, d_counters );
    else if( hs_in ) acn_launch_hard_shadow( f, q, machine_lds_bytes( h->scene ), c.stream, s, d_accum, d_counters );
    else if( hp_in ) acn_launch_hard_path( f, q, machine_lds_bytes( h->scene ), c.stream, s, d_accum, d_counters );
    else             acn_launch_shade_hits( false, q, c.stream, s, d_accum, d_counters );
    HIP_TRY( hipGetLastError() );
    HIP_TRY( hipStreamSynchronize( c.stream ) );

    uint32_t counts[ QC_N ];
    if( ( st = DevCopies::fetch( counts, d_counts, sizeof( counts ) ) ) != ACN_OK ) return st;
    if( out->counts ) memcpy( out->counts, counts, sizeof( counts ) );
    if( counts[ QC_FLAGS ] & ( ACN_FLAGS_CHUNK_LOST | ACN_FLAG_STACK_OVERFLOW ) )
        return fail( ACN_ERR_DEVICE, "acn_run_stage: the kernel raised overflow flags " + std::to_string( counts[ QC_FLAGS ] ) + ": a queue the plan sized was too small" );
    struct { void* dst; const void* d; size_t bytes; } outs[] = {
        { split ? out->tasks : nullptr, d_tasks, b_tasks },
        { split ? ( void* )out->idx[ 0 ] : nullptr, d_idx[ 0 ], b_idx }, { split ? ( void* )out->idx[ 1 ] : nullptr, d_idx[ 1 ], b_idx },
        { split ? ( void* )out->idx[ 2 ] : nullptr, d_idx[ 2 ], b_idx }, { split ? ( void* )out->idx[ 3 ] : nullptr, d_idx[ 3 ], b_idx },
        { split ? out->rays : nullptr, d_rays, b_rays }, { shade || hp_in ? out->children : nullptr, d_children, b_children },
        { shade || split || hs_in ? out->hard_shadow : nullptr, d_hs, b_hs }, { shade ? out->hard_path : nullptr, d_hp, b_hp }, { out->accum, d_accum, b_accum } };
    for( const auto& o : outs ) if( o.dst && ( st = DevCopies::fetch( o.dst, o.d, o.bytes ) ) != ACN_OK ) return st;
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
    int st = acn_stage_walk_plan( h, a, &cap );
    if( st != ACN_OK ) return st;
    if( !out ) return fail( ACN_ERR_ARG, "acn_run_stage_walk: null argument: out" );
    Call c( nullptr );
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;

    const uint32_t waves = cap.grid * 4u;
    const size_t b_tasks = ( size_t )cap.cap_tasks * sizeof( DTask ), b_idx = ( size_t )cap.cap_tasks * sizeof( uint32_t );
    const size_t b_rays = ( size_t )cap.cap_rays * sizeof( RayTask ), b_hs = ( size_t )cap.cap_hard_shadow * sizeof( HardShadow );
    const size_t b_stacks = ( size_t )waves * a->stack_cap * sizeof( RayTask );
    const size_t b_counts = sizeof( uint32_t ) * QC_N, b_accum = sizeof( unsigned long long ) * 3 * a->n;
    DevCopies dc;
    DTask* d_tasks = ( DTask* )dc.make( nullptr, b_tasks );
    uint32_t* d_idx[ ACN_NCLASS ];
    for( int k = 0; k < ACN_NCLASS; k++ ) d_idx[ k ] = ( uint32_t* )dc.make( nullptr, b_idx );
    RayTask* d_rays[ 2 ] = { ( RayTask* )dc.make( nullptr, b_rays ), ( RayTask* )dc.make( nullptr, b_rays ) };
    RayTask* d_stacks = ( RayTask* )dc.make( nullptr, b_stacks );
    HardShadow* d_hs = ( HardShadow* )dc.make( nullptr, b_hs );
    /* the kernels take every queue of a level; what the walk never touches is one record */
    HitRec* d_children = ( HitRec* )dc.make( nullptr, sizeof( HitRec ) );
    HardPath* d_hp = ( HardPath* )dc.make( nullptr, sizeof( HardPath ) );
    double* d_pos = a->camera && a->pos_xy ? ( double* )dc.make( a->pos_xy, sizeof( double ) * 2 * a->n ) : nullptr;
    uint32_t* d_counts = ( uint32_t* )dc.make( nullptr, b_counts );
    unsigned long long* d_accum = ( unsigned long long* )dc.make( nullptr, b_accum );
    unsigned long long* d_counters = ( unsigned long long* )dc.make( nullptr, sizeof( unsigned long long ) * ACN_CNT_SLOTS );
    bool made = d_tasks && d_rays[ 0 ] && d_rays[ 1 ] && d_stacks && d_hs && d_children && d_hp && d_counts && d_accum && d_counters && ( d_pos || !( a->camera && a->pos_xy ) );
    for( int k = 0; k < ACN_NCLASS; k++ ) made = made && d_idx[ k ];
    if( !made ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );

    /* what the kernel does not write reads as dead (0xFF: pixel ACN_INVALID, a dead index entry) */
    HIP_TRY( hipMemsetAsync( d_tasks, 0xFF, b_tasks, c.stream ) );
    for( int k = 0; k < ACN_NCLASS; k++ ) HIP_TRY( hipMemsetAsync( d_idx[ k ], 0xFF, b_idx, c.stream ) );
    for( int k = 0; k < 2; k++ ) HIP_TRY( hipMemsetAsync( d_rays[ k ], 0xFF, b_rays, c.stream ) );
    HIP_TRY( hipMemsetAsync( d_hs, 0xFF, b_hs, c.stream ) );
    HIP_TRY( hipMemsetAsync( d_counts, 0, b_counts, c.stream ) );
    HIP_TRY( hipMemsetAsync( d_accum, 0, b_accum, c.stream ) );
    HIP_TRY( hipMemsetAsync( d_counters, 0, sizeof( unsigned long long ) * ACN_CNT_SLOTS, c.stream ) );
    if( !a->camera )
    {
        /* generation 0 of the level: the caller's rays, and their number where pass 0 reads it (room_rays >= n: they fit) */
        HIP_TRY( hipMemcpyAsync( d_rays[ 0 ], a->in, ( size_t )a->n * sizeof( RayTask ), hipMemcpyHostToDevice, c.stream ) );
        HIP_TRY( hipMemcpyAsync( d_counts + QC_GEN, &a->n, sizeof( uint32_t ), hipMemcpyHostToDevice, c.stream ) );
    }
    HIP_TRY( hipStreamSynchronize( c.stream ) );   /* the caller's memory is read */

    LevelQ q;
    memset( &q, 0, sizeof( q ) );
    q.tasks = d_tasks; for( int k = 0; k < ACN_NCLASS; k++ ) q.idx[ k ] = d_idx[ k ];
    q.task_cap = cap.cap_tasks; q.child_cap = 1; q.hs_cap = cap.cap_hard_shadow; q.hard_cap = 1; q.ray_cap = cap.cap_rays;
    q.children = d_children; q.hard_shadow = d_hs; q.hard_path = d_hp; q.rays[ 0 ] = d_rays[ 0 ]; q.rays[ 1 ] = d_rays[ 1 ];
    q.stacks = d_stacks; q.stack_cap = a->stack_cap; q.stack_use = a->stack_use ? a->stack_use : a->stack_cap;
    q.counts = d_counts; q.prev_children = d_counts + QC_CHILDREN;
    q.grid = cap.grid; q.shade_grid = cap.grid; q.walk_grid = cap.grid;
    q.fetch_walk = a->fetch; q.fetch_hard = h->tun.fetch_hard; q.fetch_shade = h->tun.fetch_shade; q.private_limit = a->private_limit;
    q.shard_rank = 0u; q.shard_world = 1u;
    q.emit_terms = a->flags & ACN_STAGE_NO_EMIT_TERMS ? 0u : 1u;
    KernelFlags f;
    f.count = false; f.leaf_lights = h->scene.leaf_lights;
    f.lds_nodes = h->scene.lds_bytes != 0 && !( a->flags & ACN_STAGE_GLOBAL_NODES );
    f.prune = h->scene.prune && !( a->flags & ACN_STAGE_NO_PRUNE );
    DevScene dev = h->dev;
    dev.flags = d_counts + QC_FLAGS;
    const SceneArgs s = scene_args( dev, h->scene );
    const size_t lds = machine_lds_bytes( h->scene );
    /* the camera form: the order of work of a render call over the n positions, every slot of its tiles in one chunk */
    TileOrder order;
    memset( &order, 0, sizeof( order ) );
    order.n = a->n; order.n_tiles = acn_tile_order( a->n, ACN_ORDER_SHIFT, &order.mul ); order.sample_stride = 0;
    const uint32_t n_cam = a->camera ? acn_stage_walk_slots( a ) : 0u;
    for( uint32_t pass = 0; pass < a->passes; pass++ )
    {
        acn_launch_walk( f, pass, pass + 1 == a->passes, q, lds, c.stream, s, d_pos, ( size_t )a->first_pixel, 0u, pass == 0 ? n_cam : 0u, order, d_accum, d_counters );
        HIP_TRY( hipGetLastError() );
    }
    HIP_TRY( hipStreamSynchronize( c.stream ) );

    uint32_t counts[ QC_N ];
    if( ( st = DevCopies::fetch( counts, d_counts, sizeof( counts ) ) ) != ACN_OK ) return st;
    if( out->counts ) memcpy( out->counts, counts, sizeof( counts ) );
    if( counts[ QC_FLAGS ] & ( ACN_FLAGS_CHUNK_LOST | ACN_FLAG_STACK_OVERFLOW ) )
        return fail( ACN_ERR_DEVICE, "acn_run_stage_walk: the kernel raised overflow flags " + std::to_string( counts[ QC_FLAGS ] ) + ": room_rays is below what the walk traced" );
    struct { void* dst; const void* d; size_t bytes; } outs[] = {
        { out->tasks, d_tasks, b_tasks },
        { ( void* )out->idx[ 0 ], d_idx[ 0 ], b_idx }, { ( void* )out->idx[ 1 ], d_idx[ 1 ], b_idx },
        { ( void* )out->idx[ 2 ], d_idx[ 2 ], b_idx }, { ( void* )out->idx[ 3 ], d_idx[ 3 ], b_idx },
        { out->rays, d_rays[ a->passes & 1 ], b_rays }, { out->hard_shadow, d_hs, b_hs }, { out->accum, d_accum, b_accum } };
    for( const auto& o : outs ) if( o.dst && ( st = DevCopies::fetch( o.dst, o.d, o.bytes ) ) != ACN_OK ) return st;
    return ACN_OK;
}
