/* acn_k_walk.h -- k_walk and k_shade_hits with their launch macros: included by the k_walk_*.hip units alone (acn_launch.h) */
#ifndef ACN_K_WALK_H
#define ACN_K_WALK_H

#include "acn_queues.h"
#include "acn_launch.h"
#include "acn_variant.h"

/* One pass of the specular walk of a path level: persistent waves, work fetched through the atomic cursor of the pass.
 * Input (generation `pass` of the level): rays_in == nullptr: the camera rays of the sample positions in slots
 * [ base, base + n_cam ) of the call's TileOrder (lum_machine_s_func, scene.c:976-1011); else the ray queue rays_in[ 0 .. min( p_counts[ QC_GEN + pass ], in_cap ) ).
 * Each ray is traced (scene_s_trans_hit) and its hit shaded: light / background terms go to the pixel, the diffuse block
 * becomes a DTask, and the Fresnel / chromatic / refraction children go
 *   - input larger than private_limit: to rays_out, the queue of generation pass + 1 -- the next launch deals them to
 *     the whole chip again (no wave follows a long chain alone while the others idle);
 *   - else: onto the wave's private LIFO stack (stacks: ( waves of the grid ) x stack_stride slots, stack_cap of them
 *     used); the wave works in steps of 64 rays -- the top of its stack, topped up with fresh input -- until both are
 *     empty, so the tail of a level, up to trace_depth generations of a few rays each, costs no further launch.  Rays
 *     that do not fit the stack join rays_out.
 * The host enqueues a fixed number of passes per level blind; passes whose input is empty exit at once.
 * emit_terms: 0 drops the pixel terms of this launch (ACN_SHARD_SAMPLES, level 0, rank > 0). */
template< bool COUNT, bool LDS, bool PRUNE >
__global__ __launch_bounds__( 256, ACN_TRACE_WAVES )
void k_walk( ACN_SCENE_PARAMS, ACN_TASKQ_PARAMS, const RayTask* __restrict__ rays_in, uint32_t in_cap, uint32_t pass,
             const double* __restrict__ pos_xy, size_t first_pixel, uint32_t base, uint32_t n_cam, TileOrder order,
             RayTask* __restrict__ rays_out, uint32_t out_cap, uint32_t private_limit,
             RayTask* __restrict__ stacks, uint32_t stack_stride, uint32_t stack_cap, uint32_t fetch_batch, uint32_t emit_terms,
             unsigned long long* __restrict__ accum, unsigned long long* __restrict__ counters )
{
    ACN_CHUNK_STATES
    ACN_CHUNK_FLAGS_LOAD
    uint32_t n_in = n_cam;
    if( rays_in ) { n_in = p_counts[ QC_GEN + pass ]; n_in = n_in < in_cap ? n_in : in_cap; }
    n_in = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )n_in );
    ACN_LEAVE_IF_CHUNK_IS_LOST_BLOCK
    if( n_in == 0 ) return;
    ACN_SCENE_VIEW
    ACN_TASKQ_VIEW
    if( sc_in.lds_stack != ACN_NO_LDS_STACK ) sc.lds_stack = LDS ? sc.n_nodes * ( uint32_t )sizeof( GNode ) : 0u;   /* the CSG stacks follow the staged nodes */
    if constexpr( LDS ) ACN_STAGE_NODES( sc )
    const ChunkP cs = ACN_CHUNKS_OF_WAVE;
    chunks_init( cs );
    ACN_PHASE_INIT
    Cnt< COUNT > cnt;
    cnt.clear();
    const int lane = ( int )( threadIdx.x & 63 );
    const uint32_t wave = blockIdx.x * ( blockDim.x >> 6 ) + ( threadIdx.x >> 6 );
    WalkSink sink;
    sink.priv = n_in <= private_limit;
    sink.stack = stacks + ( size_t )wave * stack_stride; sink.cap = stack_cap; sink.top = 0;
    sink.out.rays = rays_out; sink.out.counter = p_counts + QC_GEN + pass + 1; sink.out.cap = out_cap; sink.out.flags = sc_in.flags; sink.out.cs = cs + 5;
    uint32_t* cursor = p_counts + QC_CUR_GEN + pass;
    FetchRange fr;
    range_init( fr, true );
    uint32_t traced = 0, steps = 0;
    bool finished = false;
    for( uint32_t step = 0; step < ACN_WALK_MAX_STEPS; step++ )
    {
        /* the step's 64 rays: the top of the private stack, topped up with fresh input */
        uint32_t n_pop = sink.top < 64u ? sink.top : 64u;
        uint32_t n_fresh = 0, fb = 0;
        if( n_pop < 64u ) n_fresh = range_take( fr, cursor, fetch_batch, n_in, 64u - n_pop, &fb );
        if( n_pop + n_fresh == 0 ) { finished = true; break; }
        sink.top -= n_pop;
        const RayTask* src = nullptr;
        bool live = false;
        uint32_t pixel = 0;
        V3 rp = mk( 0, 0, 0 ), rd = mk( 0, 0, 1 );
        if( ( uint32_t )lane < n_pop ) { src = sink.stack + sink.top + lane; live = true; }
        else if( ( uint32_t )lane < n_pop + n_fresh )
        {
            uint32_t i = fb + ( ( uint32_t )lane - n_pop );
            if( rays_in ) { src = rays_in + i; live = src->pixel != ACN_INVALID; }
            else
            {
                /* the camera ray of a sample position (slots past the call's last position are empty) */
                pixel = order.position( base + i );
                live = pixel < order.n;
                if( !live ) pixel = 0;
                double mx, my;
                if( pos_xy ) { mx = pos_xy[ ( size_t )pixel * 2 ]; my = pos_xy[ ( size_t )pixel * 2 + 1 ]; }
                else
                {
                    size_t pix = first_pixel + pixel;
                    mx = ( double )( pix % sc.prm.image_width ) + 0.5;
                    my = ( double )( pix / sc.prm.image_width ) + 0.5;
                }
                camera_ray( sc, mx, my, &rp, &rd );
                if( live ) cnt.cost( ACN_F_CAMERA_RAY );
            }
        }
        if( src && live ) { rp = src->p; rd = src->d; }
        if( live ) traced++;
        steps++;

        /* scene_s_trans_hit */
        Trans trans;
        trans.exit_nor = mk( 0, 0, 0 ); trans.exit_obj = -1; trans.enter_obj = -1;
        double offs = F3_INF;
        if( live ) offs = scene_trans_hit_dev( machine_view< PRUNE, LDS >( sc ), rp, rd, &trans, &cnt );
        /* what the ray carries is read only now, so that it does not occupy registers across the traversal */
        asm volatile( "" ::: "memory" );
        V3 T = mk( 1, 1, 1 );
        double intensity = 1.0;
        int depth = ( int )sc.prm.trace_depth;
        if( src && live ) { T = src->T; intensity = src->intensity; depth = src->depth; pixel = src->pixel; }
        bool hit = live && offs < F3_INF;
        V3 acc = mk( 0, 0, 0 );
        if( live && !hit ) acc = v_mld( T, v_mlf( ld3( sc.prm.background_color ), intensity ) );
        shade_hit( sc, sink, tq, cs, rp, rd, hit ? offs : 0.0, trans, hit ? depth : 0, intensity, T, pixel, acc, &cnt );
        /* emit_terms == 0: level 0 of a rank > 0 of a sample-sharded call -- emission / background reached through
         * specular chains are under no sharded loop and come from rank 0 alone */
        if( live && emit_terms ) pixel_add( accum, sc.flags, pixel, acc );
        /* the wave reads next what it wrote last: same wave, program order; the fence keeps the compiler from moving the
         * next step's loads above this step's stores */
        __builtin_amdgcn_fence( __ATOMIC_SEQ_CST, "wavefront" );
        ACN_LAP( PH_SHADE );
    }
    ACN_LAP( PH_TAIL );
    ACN_PHASE_FLUSH( counters, 0 )
    /* the step bound is a safety net against a loop that does not end; work would be lost, so the call fails */
    if( !finished && lane == 0 ) atomicOr( sc_in.flags, ACN_FLAG_STACK_OVERFLOW );
    sink.out.close( p_counts + QS_DEAD_R );
    task_chunks_close( tq, cs );
    wave_stat_add( p_counts + QS_WALK_RAYS, traced );
    if( sink.priv ) wave_stat_add( p_counts + QS_PRIVATE_RAYS, traced );
    if( lane == 0 && steps ) atomicAdd( p_counts + QS_WALK_STEPS, steps );
    wave_add_counters( counters, cnt );
}

/* first step of a level >= 1: one lane per path-sample hit of the previous level (the recursive scene_s_lum call of
 * scene.c:610); persistent waves fetch 64 records at a time.  n_ptr: the previous level's QC_CHILDREN. */
template< bool COUNT >
__global__ __launch_bounds__( 256, ACN_WALK_WAVES )
void k_shade_hits( ACN_SCENE_PARAMS, ACN_TASKQ_PARAMS, const HitRec* __restrict__ recs, const uint32_t* __restrict__ n_ptr, uint32_t rec_cap, uint32_t fetch_batch,
                   RayTask* __restrict__ rays_out, uint32_t ray_cap,
                   unsigned long long* __restrict__ accum, unsigned long long* __restrict__ counters )
{
    ACN_CHUNK_STATES
    ACN_CHUNK_FLAGS_LOAD
    uint32_t n = *n_ptr;
    n = n < rec_cap ? n : rec_cap;
    n = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )n );
    ACN_LEAVE_IF_CHUNK_IS_LOST
    if( n == 0 ) return;
    fetch_batch = balanced_batch( n, fetch_batch, 64u );
    ACN_SCENE_VIEW
    CountedTaskQ tq;
    ACN_TASKQ_FILL
    uint32_t n_probes = 0;
    tq.n_probes = &n_probes;
    const ChunkP cs = ACN_CHUNKS_OF_WAVE;
    chunks_init( cs );
    chunks_resize( cs, n );
    Cnt< COUNT > cnt;
    cnt.clear();
    RayQ rq;
    rq.rays = rays_out; rq.counter = p_counts + QC_GEN; rq.cap = ray_cap; rq.flags = sc_in.flags; rq.cs = cs + 5;
    FetchRange fr;
    range_init( fr, n > 0 );
    for( ;; )
    {
        uint32_t first = 0;
        uint32_t got = range_take( fr, p_counts + QC_CUR_HITS, fetch_batch, n, 64u, &first );
        if( got == 0 ) break;
        uint32_t i = first + ( threadIdx.x & 63 );
        bool live = ( threadIdx.x & 63 ) < got;
        HitRec r;
        r.p = mk( 0, 0, 0 ); r.d = mk( 0, 0, 1 ); r.offs = 0; r.exit_nor = mk( 0, 0, 0 ); r.T = mk( 0, 0, 0 ); r.intensity = 0;
        r.exit_obj = -1; r.enter_obj = -1; r.depth = 0; r.pixel = ACN_INVALID;
        if( live ) r = recs[ i ];
        live = live && r.pixel != ACN_INVALID;
        V3 acc = mk( 0, 0, 0 );
        Trans trans;
        trans.exit_nor = r.exit_nor; trans.exit_obj = r.exit_obj; trans.enter_obj = r.enter_obj;
        shade_hit( sc, rq, tq, cs, r.p, r.d, r.offs, trans, live ? r.depth : 0, r.intensity, r.T, r.pixel, acc, &cnt );
        if( live ) pixel_add( accum, sc.flags, r.pixel, acc );
    }
    rq.close( p_counts + QS_DEAD_R );
    task_chunks_close( tq, cs );
    if( ( threadIdx.x & 63 ) == 0 && n_probes ) atomicAdd( p_counts + QS_PROBES, n_probes );
    wave_add_counters( counters, cnt );
}

/* k_walk< C, L, P > in a link of acn_launch_walk's chain: ( f, q, w, stream, s ) are the wrapper's arguments */
#define ACN_LW_( C, L, P ) \
    hipLaunchKernelGGL( ( k_walk< C, L, P > ), dim3( q.walk_grid ), dim3( 256 ), w.lds_bytes, stream, ACN_SCENE_ARGS_OF( s ), ACN_TASKQ_ARGS_OF( q ), \
        w.n_cam ? ( const RayTask* )nullptr : ( const RayTask* )q.rays[ w.pass & 1 ], q.ray_cap, w.pass, w.pos_xy, w.first_pixel, w.base, w.n_cam, w.order, \
        q.rays[ ( w.pass + 1 ) & 1 ], q.ray_cap, w.last ? 0xFFFFFFFFu : q.private_limit, \
        q.stacks, q.stack_cap, w.last ? q.stack_cap : q.stack_use, q.fetch_walk, q.emit_terms, w.accum, w.counters )

#endif /* ACN_K_WALK_H */
