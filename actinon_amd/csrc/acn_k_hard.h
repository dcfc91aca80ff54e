/* acn_k_hard.h -- the two hard-ray kernels and the pending list: included by k_hard_shadow.hip and k_hard_path.hip alone (acn_launch.h) */
#ifndef ACN_K_HARD_H
#define ACN_K_HARD_H

#include "acn_queues.h"
#include "acn_launch.h"
#include "acn_variant.h"

/* The pending list of a hard-ray wave: indices of the records that are left for a CSG machine.  The machines run in lock step, so a
 * wave pays a machine step for 64 lanes however many of them hold a ray; the hard-ray kernels therefore read their queue in two
 * phases.  The FILL phase takes 64 slots at a time, drops the dead ones and the rays it can decide without a machine, and appends
 * the indices of the rest; the MACHINE phase runs when 64 indices are pending (or the input is exhausted), on a full wave.  A list
 * is its wave's own -- 128 indices in static LDS, the count a wave-uniform register -- so nothing waits for another wave: no
 * __syncthreads (a pool shared by the workgroup, ACN_POOLED, lost to its barriers: DESIGN.md 4d).  The fill phase runs below 64
 * pending and adds 64 at most: 127 is the most a list holds.
 * k_hard_shadow alone uses it: every record of k_hard_path needs a machine and 2 - 3 % of its slots are dead, and the same list made
 * that kernel 3.6 % slower (profiles/r17/NOTES.md).  LDS: the lists are 2 KB beside 36 KB of CSG stacks, 38 KB of the 40 KB a
 * workgroup may have at four per CU; a scene whose staged nodes (plan_lds, acn_tables.cpp: up to 4 KB) take the rest runs this one
 * kernel at three workgroups per CU. */
#define ACN_PENDING_MAX 128u
#define ACN_PENDING_LIST __shared__ uint32_t acn_pending[ 4 * ACN_PENDING_MAX ];
#define ACN_PENDING_OF_WAVE ( ( LdsU32P )acn_pending + __builtin_amdgcn_readfirstlane( ( int )( threadIdx.x >> 6 ) ) * ( int )ACN_PENDING_MAX )
/* all lanes of the wave: the lanes with `keep` append `index`; n_pending is the same in every lane */
DEV void pending_push( LdsU32P list, uint32_t& n_pending, bool keep, uint32_t index )
{
    const unsigned long long mask = __ballot( keep );
    if( keep ) list[ n_pending + lanes_below( mask ) ] = index;
    n_pending += ( uint32_t )__popcll( mask );
}
/* all lanes of the wave: takes up to 64 indices off the end of the list; returns how many.  Lane l < that many gets one in *index.
 * (The wave reads what other lanes of it wrote: same wave, program order; the fence keeps the compiler from moving the reads up.) */
DEV uint32_t pending_pop( LdsU32P list, uint32_t& n_pending, uint32_t* index )
{
    __builtin_amdgcn_fence( __ATOMIC_SEQ_CST, "wavefront" );
    const uint32_t take = n_pending < 64u ? n_pending : 64u;
    n_pending -= take;
    *index = ( threadIdx.x & 63 ) < take ? list[ n_pending + ( threadIdx.x & 63 ) ] : ACN_INVALID;
    __builtin_amdgcn_fence( __ATOMIC_SEQ_CST, "wavefront" );
    return take;
}

/* the shadow rays k_shade could not decide inline and the probes nothing has looked at yet, one lane per ray, persistent waves: the
 * occlusion test over the elements the record's resume word names, or over all of them.
 * COUNT = false: two phases per wave (the pending list above).  The fill phase reads pixel and pad of its 64 slots.  A record with
 * a resume word is pending as it is: k_shade ran the in-line pass.  For any other record -- the probes of k_walk / k_shade_hits, 3 in
 * 8 of the wine glass's records -- the fill phase runs that pass itself, root_occluded_fast over the light root (pad bit 0) and the
 * matter root, at whatever lanes the batch has: a probe that an in-line element occludes, or that no machine element survives the
 * pre-tests for, is finished here; one that a machine element of the matter root is left for gets the pass's candidates as its resume
 * word, written back to its pad, and is pending.  (A light root with a machine element that is not ruled out: the record is
 * pending untouched and the machine phase does both roots in full, the one-phase form.)  Occlusion is an OR over the elements and the
 * pixel sums are fixed-point atomics, so neither the order of the tests nor that of the rays moves a bit.  The machine phase loads
 * ray and word by index, and what the ray carries -- contrib, pixel -- after the machine, so that it occupies no registers across it.
 * COUNT = true: one phase, the full loop on every record: the event counts are the oracle's. */
template< bool COUNT, bool LDS, bool PRUNE >
__global__ __launch_bounds__( 256, ACN_WALK_WAVES )
void k_hard_shadow( ACN_SCENE_PARAMS, HardShadow* __restrict__ recs, uint32_t cap, uint32_t fetch_batch, uint32_t pos_base, uint32_t* __restrict__ p_counts,
                    unsigned long long* __restrict__ accum, unsigned long long* __restrict__ counters )
{
    ACN_PENDING_LIST
    ACN_CHUNK_FLAGS_LOAD
    uint32_t n = p_counts[ QC_HARD_SHADOW ];
    n = n < cap ? n : cap;
    n = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )n );
    ACN_LEAVE_IF_CHUNK_IS_LOST_BLOCK
    if( n == 0 ) return;
    ACN_SCENE_VIEW
    if( sc_in.lds_stack != ACN_NO_LDS_STACK ) sc.lds_stack = LDS ? sc.n_nodes * ( uint32_t )sizeof( GNode ) : 0u;   /* the CSG stacks follow the staged nodes */
    Cnt< COUNT > cnt;
    cnt.clear();
    if constexpr( LDS ) ACN_STAGE_NODES( sc )
    ACN_PHASE_INIT
    fetch_batch = balanced_batch( n, fetch_batch, 64u );
    FetchRange fr;
    range_init( fr, n > 0 );
    [[maybe_unused]] const LdsU32P pending = ACN_PENDING_OF_WAVE;
    [[maybe_unused]] uint32_t n_pending = 0;
    [[maybe_unused]] bool input = true;
    uint32_t n_dead = 0;   /* dead slots this wave stepped over (the same in every lane) */
    for( ;; )
    {
        uint32_t index = ACN_INVALID;
        if constexpr( COUNT )
        {
            uint32_t first = 0;
            uint32_t got = range_take( fr, p_counts + QC_CUR_HS, fetch_batch, n, 64u, &first );
            if( got == 0 ) break;
            if( ( threadIdx.x & 63 ) < got && recs[ first + ( threadIdx.x & 63 ) ].pixel != ACN_INVALID ) index = first + ( threadIdx.x & 63 );
            n_dead += got - ( uint32_t )__popcll( __ballot( index != ACN_INVALID ) );
        }
        else
        {
            while( n_pending < 64u && input )
            {
                uint32_t first = 0;
                uint32_t got = range_take( fr, p_counts + QC_CUR_HS, fetch_batch, n, 64u, &first );
                if( got == 0 ) { input = false; break; }
                const uint32_t i = first + ( threadIdx.x & 63 );
                bool keep = false;
                const bool live = ( threadIdx.x & 63 ) < got && recs[ i ].pixel != ACN_INVALID;
                n_dead += got - ( uint32_t )__popcll( __ballot( live ) );
                if( live )
                {
                    const uint32_t pad = recs[ i ].pad;
                    keep = true;
                    if( !( pad & ACN_RESUME_FLAG ) )
                    {
                        const V3 pos = recs[ i ].pos, d = recs[ i ].d;
                        const double limit = recs[ i ].limit;
                        int state = 0;        /* as root_occluded_fast answers: 0 no in-line element occludes, 1 occluded, 2 a machine element is left */
                        uint32_t cand = 0;
                        ACN_LAP( PH_FETCH );
                        #pragma unroll 1
                        for( int k = 0; k < 2; k++ )
                        {
                            const int root = k ? sc.matter_root : sc.light_root;
                            const bool want = state == 0 && ( k == 1 || ( pad & 1u ) );
                            if( __ballot( want ) == 0ull ) continue;
                            if( want )
                            {
                                state = root_occluded_fast( machine_view< PRUNE, LDS >( sc ), root, pos, d, limit, 0ull, &cand, &cnt );
                                if( state == 2 && k == 0 ) state = 3;   /* of the light root: the words speak of the matter root */
                            }
                        }
                        ACN_LAP( PH_ROOT_LEAF );
                        if( state == 0 ) pixel_add( accum, sc.flags, recs[ i ].pixel, recs[ i ].contrib );
                        if( state == 2 ) recs[ i ].pad = resume_record( cand ) | ( pad & 1u );
                        keep = state >= 2;
                        ACN_LAP( PH_SHADE );
                    }
                }
                pending_push( pending, n_pending, keep, i );
                ACN_LAP( PH_FETCH );
            }
            if( pending_pop( pending, n_pending, &index ) == 0 ) break;
        }
        if( index != ACN_INVALID )
        {
            const V3 pos = recs[ index ].pos, d = recs[ index ].d;
            const double limit = recs[ index ].limit;
            const uint32_t pad = recs[ index ].pad;
            bool occ = false;
            ACN_LAP( PH_FETCH );
            #pragma unroll 1
            for( int k = 0; k < 2; k++ )
            {
                const int root = k ? sc.matter_root : sc.light_root;
                const bool want = !occ && ( k == 1 || ( pad & ( 1u | ACN_RESUME_FLAG ) ) == 1u );   /* (a resumed probe: the fill phase did the light root) */
                if( __ballot( want ) == 0ull ) continue;
                if( want )
                {
                    const uint32_t rec = k ? pad : 0u;   /* the word speaks of the matter root */
                    occ = root_occluded_rec< true >( machine_view< PRUNE, LDS >( sc ), root, pos, d, limit, rec, pos_base, &cnt );
                }
            }
            ACN_LAP( PH_ROOT_LEAF );
            /* what the ray carries is read only now, so that it does not occupy registers across the machine */
            asm volatile( "" ::: "memory" );
            if constexpr( COUNT )
            {
                /* the tail of scene.c:571-574 belongs to a direct-light sample of k_shade: a resume word, bit 0 clear, the light's
                 * distance as its limit.  A probe stands for a background term, for which the reference books nothing: the specular
                 * ones carry bit 0 or no resume word, k_shade's dark path rays the path limit.  The record has no field that says
                 * which it is, so this is a rule of thumb: a direct sample whose light lies at exactly shade_path_limit (one double)
                 * would be taken for a probe and lose its 23 flop */
                const double path_limit = shade_path_limit( sc.prm.max_path_length );
                if( !occ && ( pad & ( 1u | ACN_RESUME_FLAG ) ) == ACN_RESUME_FLAG && limit != path_limit ) cnt.cost( ACN_F_DIRECT_TAIL );
            }
            if( !occ ) pixel_add( accum, sc.flags, recs[ index ].pixel, recs[ index ].contrib );
            ACN_LAP( PH_SHADE );
        }
    }
    ACN_LAP( PH_TAIL );
    if( ( threadIdx.x & 63 ) == 0 && n_dead ) atomicAdd( p_counts + QS_DEAD_HS, n_dead );
    ACN_PHASE_FLUSH( counters, 1 )
    wave_add_counters( counters, cnt );
}

/* the path rays k_shade could not finish inline: the transition hit over the elements the record's resume word names; hits
 * join the next level's HitRec queue */
template< bool COUNT, bool LDS, bool PRUNE >
__global__ __launch_bounds__( 256, ACN_HPATH_WAVES )
void k_hard_path( ACN_SCENE_PARAMS, const HardPath* __restrict__ recs, uint32_t cap, uint32_t fetch_batch, HitRec* __restrict__ p_children, uint32_t child_cap,
                  uint32_t* __restrict__ p_counts, unsigned long long* __restrict__ accum, unsigned long long* __restrict__ counters )
{
    ACN_CHUNK_STATES
    ACN_CHUNK_FLAGS_LOAD
    uint32_t n = p_counts[ QC_HARD_PATH ];
    n = n < cap ? n : cap;
    n = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )n );
    ACN_LEAVE_IF_CHUNK_IS_LOST_BLOCK
    if( n == 0 ) return;
    ACN_SCENE_VIEW
    if( sc_in.lds_stack != ACN_NO_LDS_STACK ) sc.lds_stack = LDS ? sc.n_nodes * ( uint32_t )sizeof( GNode ) : 0u;   /* the CSG stacks follow the staged nodes */
    Cnt< COUNT > cnt;
    cnt.clear();
    if constexpr( LDS ) ACN_STAGE_NODES( sc )
    ACN_PHASE_INIT
    const ChunkP cs = ACN_CHUNKS_OF_WAVE;
    chunks_init( cs );
    fetch_batch = balanced_batch( n, fetch_batch, 64u );
    uint32_t n_ch = 0;
    auto kill_ch = [ p_children ]( uint32_t k ) { p_children[ k ].pixel = ACN_INVALID; };
    FetchRange fr;
    range_init( fr, n > 0 );
    for( ;; )
    {
        uint32_t first = 0;
        uint32_t got = range_take( fr, p_counts + QC_CUR_HP, fetch_batch, n, 64u, &first );
        if( got == 0 ) break;
        bool hit = false;
        HardPath r;
        r.pos = mk( 0, 0, 0 ); r.d = mk( 0, 0, 1 ); r.T = mk( 0, 0, 0 ); r.intensity = 0; r.depth = 0; r.pixel = ACN_INVALID; r.resume = 0; r.pad = 0;
        Trans trans;
        trans.exit_nor = mk( 0, 0, 0 ); trans.exit_obj = -1; trans.enter_obj = -1;
        double a = F3_INF;
        if( ( threadIdx.x & 63 ) < got ) r = recs[ first + ( threadIdx.x & 63 ) ];
        if( r.pixel != ACN_INVALID )
        {
            ACN_LAP( PH_FETCH );
            a = root_trans_hit_rec< true >( machine_view< PRUNE, LDS >( sc ), sc.matter_root, r.pos, r.d, &trans, r.resume, &cnt );
            ACN_LAP( PH_ROOT_LEAF );
            hit = a < sc.prm.max_path_length;
            if( !hit )
            {
                V3 c = v_mlf( ld3( sc.prm.background_color ), r.intensity );
                pixel_add( accum, sc.flags, r.pixel, v_mld( r.T, c ) );
            }
        }
        uint32_t csl = chunk_alloc( cs + 0, &p_counts[ QC_CHILDREN ], hit );
        if( hit )
        {
            if( csl < child_cap )
            {
                HitRec& c = p_children[ csl ];
                c.p = r.pos; c.d = r.d; c.offs = a; c.exit_nor = trans.exit_nor; c.T = r.T;
                c.intensity = r.intensity;
                c.exit_obj = trans.exit_obj; c.enter_obj = trans.enter_obj;
                c.depth = r.depth; c.pixel = r.pixel;
                n_ch++;
            }
            else
            {
                atomicOr( sc_in.flags, ACN_FLAG_CHILD_OVERFLOW );
            }
        }
    }
    ACN_LAP( PH_SHADE );
    ACN_PHASE_FLUSH( counters, 2 )
    chunk_close( cs + 0, child_cap, kill_ch, p_counts + QS_DEAD_C );
    wave_stat_add( p_counts + QS_CHILDREN, n_ch );
    wave_add_counters( counters, cnt );
}

#endif /* ACN_K_HARD_H */
