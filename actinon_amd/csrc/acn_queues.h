/* acn_queues.h -- the wavefront formulation of scene_s_lum (src/scene.c:420-667) for gfx950.
 *
 * The reference evaluates one pixel by a branching recursion: specular chains (Fresnel reflection / chromatic
 * reflection / refraction, depth-1 each) with, at every diffuse shading point, a direct-light loop over
 * direct_samples*I cap samples per light and -- while depth > 10 -- a path loop over path_samples*I hemisphere
 * samples whose hits recurse with depth-10.  Every term is linear in what the recursion returns, so each pending
 * piece of work carries a colour throughput T and adds T * value into its pixel.  That turns the recursion into
 * records in HBM-resident queues and a fixed chain of kernels per path level, none of which needs the host:
 *
 *   k_walk        persistent waves.  A wave owns a private LIFO stack of pending specular rays (global memory) and
 *                 works in steps of 64 rays: whatever the stack holds, topped up with fresh input (camera rays of the
 *                 chunk's sample positions, or the ray queue k_shade_hits filled) fetched through one atomic cursor.
 *                 Each ray is traced (scene_s_trans_hit) and its hit shaded: light / background terms go to the
 *                 pixel, Fresnel / chromatic / refraction children back onto the wave's own stack, the diffuse block
 *                 becomes a DTask in a size-class queue.  No wave ever waits for another one: the whole specular
 *                 walk of a level -- up to trace_depth generations -- is ONE launch with full waves throughout.
 *   k_shade       one WAVEFRONT per DTask (16 / 4 / 1 lanes per task for the small size classes), lanes = samples:
 *                 lane j jumps the shading point's LCG stream ahead by 2j draws (the reference consumes exactly two
 *                 draws per sample, scene.c:558,598), casts its cap sample at the light, Oren-Nayar weight, shadow
 *                 ray; then the path samples: hemisphere sample, transition hit against matter; misses take the
 *                 background, hits become HitRecs of the next level; rays that enter the envelope of a CSG / SDF /
 *                 compound root element are deferred, with a word that names those elements, to
 *   k_hard_shadow / k_hard_path   persistent waves, one lane per deferred ray: the CSG machines of the named elements
 *                 (records without such a word -- the probes of k_walk -- get the full traversal).
 *   k_shade_hits  first step of levels >= 1: shade_hit on the stored path-sample hits; fills the ray queue of k_walk.
 *
 * Every kernel reads its input count from device memory (the counter block of its level) and fetches work through
 * atomic cursors, so the host enqueues the whole chain of a chunk blind and synchronises once at its end.
 *
 * Pixel accumulation is order-independent and therefore bit-reproducible: contributions are added as 2^-40
 * fixed-point integers with 64-bit integer atomics (resolution 9.1e-13; one contribution is clamped to +-16384 --
 * cl_s_sat saturates at 1.0 -- and ACN_FLAG_CLAMPED reports when that happened; 2^9 clamped adds cannot wrap).
 */
#ifndef ACN_QUEUES_H
#define ACN_QUEUES_H

#include "acn_records.h"
#include "acn_kernel_params.h"

/* Size classes of the shading tasks: 64 / 16 / 4 / 1 lanes per task, by the larger of the task's two sample counts.
 * Narrow groups lose less in the last, partly filled round of a sample loop (200 samples on 64 lanes: 4 rounds, 78 %
 * of the lanes busy; on 16 lanes: 13 rounds, 96 %), and the tasks that share a wave are neighbours with similar counts;
 * a whole wavefront per task keeps the rays of a round on one origin.  Where the 64-lane class begins is chosen per
 * scene at upload (DevScene.class0_min, see there; ACN_CLASS0_MIN overrides). */
#ifndef ACN_CLASS1_MIN
#define ACN_CLASS1_MIN 8
#endif
DEV int size_class( uint64_t n, uint32_t class0_min )
{
    return n > class0_min ? 0 : n > ACN_CLASS1_MIN ? 1 : n > 2 ? 2 : 3;
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* Queue appends.  A wave reserves ACN_QCHUNK slots of a queue with ONE returning atomic and hands them out itself
 * (ballot + prefix): the ~1-2 us round trip of a device-scope atomic is paid once per 64 records instead of once per
 * append.  When a request does not fit the rest of the reservation, the rest is marked dead and a new one is taken;
 * consumers skip dead slots.  The state ( next free slot, end ) of a wave's reservation lives in LDS, one pair per
 * wave and queue, and is touched by one lane per append -- which makes appends legal under divergent control flow
 * (the sample loops of k_shade): the lanes that reach an append together form its ballot.  (ACN_QCHUNK: acn_counts.h) */
#ifndef ACN_QCHUNK_MAX
#define ACN_QCHUNK_MAX 512u
#endif
/* spare: a second reservation held beside the current one, ACN_INVALID_SLOT if none (nothing takes one at present) */
struct ChunkState { uint32_t cur, end, spare, size; };   /* size: slots per reservation (ACN_QCHUNK unless the kernel knows better, see chunks_resize) */
typedef ChunkState ACN_LDS* ChunkP;
#define ACN_NCHUNKS 8     /* reservation states per wave */
/* LDS block of the reservation states of a 256-lane workgroup; 256 B keeps the dynamic LDS behind it 16-byte aligned */
#define ACN_CHUNK_STATES __shared__ __attribute__( ( aligned( 16 ) ) ) ChunkState acn_chunk_states[ 4 * ACN_NCHUNKS ];
/* (the wave's index through readfirstlane: the pointer is then a scalar.  As a per-lane value derived from threadIdx.x it was
 * spilled and re-loaded from scratch four times per append: ~80 of the ~110 scratch loads of a k_walk step, profiles/r04) */
#define ACN_CHUNKS_OF_WAVE ( ( ChunkP )acn_chunk_states + __builtin_amdgcn_readfirstlane( ( int )( threadIdx.x >> 6 ) ) * ACN_NCHUNKS )
DEV void chunks_init( ChunkP cs )
{
    if( ( threadIdx.x & 63 ) < ACN_NCHUNKS ) { cs[ threadIdx.x & 63 ].cur = 0; cs[ threadIdx.x & 63 ].end = 0; cs[ threadIdx.x & 63 ].spare = ACN_INVALID_SLOT; cs[ threadIdx.x & 63 ].size = ACN_QCHUNK; }
}
/* Larger reservations for a wave that is going to append a lot.  Every reservation is one returning atomic on the queue's ONE
 * counter, and the device serves same-address atomics of a launch one after the other: k_shade_hits on many_spheres turns 2.7e8
 * path hits per frame (every 16th pixel) into as many tasks, one reservation per wave and batch of 64 -- and spent 152 ms doing it
 * with 4 % of its VALU slots busy; with 256 slots per reservation 64 ms (profiles/r04/ab_qchunk_s24.txt).  The price of a large
 * reservation is its unused tail (dead slots the consumers step over: a fixed 256 costs the wine glass 4 - 18 %), so the size
 * follows what the wave expects to append: an eighth of its share of the input, 64 ... 512. */
DEV void chunks_resize( ChunkP cs, uint32_t items_of_launch )
{
    const uint32_t per_wave = items_of_launch / ( gridDim.x * 4u );
    uint32_t size = ( per_wave / 8u ) & ~63u;
    size = size < ( uint32_t )ACN_QCHUNK ? ( uint32_t )ACN_QCHUNK : size > ACN_QCHUNK_MAX ? ACN_QCHUNK_MAX : size;
    if( ( threadIdx.x & 63 ) < ACN_NCHUNKS ) cs[ threadIdx.x & 63 ].size = size;
}

/* every lane with `want` gets a distinct slot of the queue counted by *counter.  A request that does not fit the rest
 * of the wave's reservation uses that rest up and continues in a new one, so slots only die at the end of a kernel. */
DEV uint32_t chunk_alloc( ChunkP cs, uint32_t* counter, bool want )
{
    unsigned long long mask = __ballot( want );
    if( !want ) return ACN_INVALID;
    /* from here on the active lanes are those with `want`: the first of them (rank 0) leads, and readfirstlane reads it */
    const uint32_t rank = lanes_below( mask );
    uint32_t m = ( uint32_t )__popcll( mask );
    uint32_t base = 0, room = 0, base2 = 0;
    if( rank == 0 )
    {
        uint32_t cur = cs->cur, end = cs->end;
        base = cur; room = end - cur;
        if( m > room )
        {
            const uint32_t spare = cs->spare, size = cs->size;
            if( spare != ACN_INVALID_SLOT ) { base2 = spare; cs->spare = ACN_INVALID_SLOT; }
            else base2 = atomicAdd( counter, size );
            cs->end = base2 + size;
            cs->cur = base2 + ( m - room );
        }
        else cs->cur = cur + m;
    }
    base  = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )base );
    room  = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )room );
    base2 = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )base2 );
    return rank < room ? base + rank : base2 + ( rank - room );
}

/* end of a kernel (all lanes of the wave): the unused tail of the wave's last reservation is dead */
template< class KILL >
DEV void chunk_close( ChunkP cs, uint32_t cap, KILL kill, uint32_t* dead = nullptr )
{
    uint32_t cur = cs->cur, end = cs->end, spare = cs->spare, size = cs->size;
    for( uint32_t k = cur + ( threadIdx.x & 63 ); k < end; k += 64 ) if( k < cap ) kill( k );
    if( spare != ACN_INVALID_SLOT ) for( uint32_t k = spare + ( threadIdx.x & 63 ); k < spare + size; k += 64 ) if( k < cap ) kill( k );
    const uint32_t d = end - cur + ( spare != ACN_INVALID_SLOT ? size : 0u );
    if( dead && d && ( threadIdx.x & 63 ) == 0 ) atomicAdd( dead, d );
}

/* one atomic per wave: every lane with `want` gets a distinct slot (unreserved form, used where appends are rare) */
DEV uint32_t wave_alloc( uint32_t* counter, bool want )
{
    unsigned long long mask = __ballot( want );
    if( !want ) return ACN_INVALID;
    const uint32_t rank = lanes_below( mask );
    uint32_t base = 0;
    if( rank == 0 ) base = atomicAdd( counter, ( uint32_t )__popcll( mask ) );
    base = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )base );
    return base + rank;
}

DEV void wave_stat_add( uint32_t* counter, uint32_t v )   /* all lanes of the wave */
{
    for( int o = 32; o > 0; o >>= 1 ) v += __shfl_down( v, o, 64 );
    if( ( threadIdx.x & 63 ) == 0 && v ) atomicAdd( counter, v );
}

/* work fetch of the persistent kernels: the wave takes the next `want` items of [ 0, n ); returns how many it got */
DEV uint32_t wave_fetch( uint32_t* cursor, uint32_t want, uint32_t n, uint32_t* first )
{
    uint32_t b = 0;
    if( ( threadIdx.x & 63 ) == 0 ) b = atomicAdd( cursor, want );
    b = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )b );
    *first = b;
    if( b >= n ) return 0;
    return n - b < want ? n - b : want;
}

/* Batch size of a kernel's work fetch for an input of n items: the configured batch, but small enough that every wave of
 * the grid comes back for work about eight times -- with one batch per wave the kernel ends when the wave that drew the
 * expensive items is done (1/8 of a 1080p frame: k_shade 5.4 ms with batches of 16 steps, where the work is 1.2 ms).
 * unit: items of one step of a wave. */
DEV uint32_t balanced_batch( uint32_t n, uint32_t batch, uint32_t unit )
{
    const uint32_t waves = gridDim.x * ( blockDim.x >> 6 );
    uint32_t b = n / ( waves * 8u );
    b -= b % unit;
    b = b < unit ? unit : b;
    return b < batch ? b : batch;
}

/* the same in batches, one ahead: the wave owns the range [ cur, end ) of the input and, while it works that off, the
 * atomic that reserves its next batch is already in flight -- its 1-2 us round trip overlaps the work instead of
 * stalling the wave once per batch.  ( cur, end, more are the same in every lane; next is lane 0's. ) */
struct FetchRange { uint32_t cur, end, next; bool pending, more; };
DEV void range_init( FetchRange& r, bool any ) { r.cur = r.end = r.next = 0; r.pending = false; r.more = any; }
DEV uint32_t range_take( FetchRange& r, uint32_t* cursor, uint32_t batch, uint32_t n, uint32_t want, uint32_t* first )
{
    if( r.cur == r.end && r.more )
    {
        if( !r.pending && ( threadIdx.x & 63 ) == 0 ) r.next = atomicAdd( cursor, batch );
        uint32_t b = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )r.next );
        r.pending = false;
        if( b >= n ) { r.more = false; r.cur = r.end = 0; }
        else
        {
            r.cur = b;
            r.end = n - b < batch ? n : b + batch;
            if( b + batch >= n ) r.more = false;
            else
            {
                if( ( threadIdx.x & 63 ) == 0 ) r.next = atomicAdd( cursor, batch );   /* the batch after this one */
                r.pending = true;
            }
        }
    }
    uint32_t have = r.end - r.cur;
    uint32_t take = have < want ? have : want;
    *first = r.cur;
    r.cur += take;
    return take;
}

/* ---- where shade_hit puts what it produces ---- */

/* the queues of diffuse shading tasks: tasks[] + one index list per size class */
struct TaskQ
{
    DTask*    tasks;
    uint32_t* idx[ ACN_NCLASS ];
    uint32_t* counts;               /* counter block of the level */
    uint32_t  task_cap;
    HardShadow* probes;             /* the level's hard-shadow queue: where probe_push appends */
    uint32_t  probe_cap;
    uint32_t  emit_terms;           /* 0: pixel terms under no sharded sample loop are dropped (ACN_SHARD_SAMPLES, level 0, rank > 0) */
    uint32_t* flags;                /* the chunk's ACN_FLAG_* word */
};

/* a ray queue in global memory (k_shade_hits -> k_walk; generation g -> generation g + 1 of k_walk) */
struct RayQ
{
    RayTask*  rays;
    uint32_t* counter;
    uint32_t  cap;
    uint32_t* flags;
    ChunkP    cs;

    DEV void push( bool want, V3 p, V3 d, V3 T, double intensity, int depth, uint32_t pixel ) const
    {
        uint32_t slot = chunk_alloc( cs, counter, want );
        if( want )
        {
            if( slot < cap )
            {
                RayTask& c = rays[ slot ];
                c.p = p; c.d = d; c.T = T; c.intensity = intensity; c.depth = depth; c.pixel = pixel;
            }
            else atomicOr( flags, ACN_FLAG_CHILD_OVERFLOW );
        }
    }
    DEV void close( uint32_t* dead ) const
    {
        RayTask* r = rays;
        chunk_close( cs, cap, [ r ]( uint32_t k ) { r[ k ].pixel = ACN_INVALID; }, dead );
    }
};

/* Where a k_walk wave puts the specular children of its rays.  `priv` is the same in every wave of a launch:
 *   false  generation pass: children go to the global queue of the next generation (the next launch spreads them
 *          over the whole chip again);
 *   true   the input is small: children go onto the wave's private LIFO stack and are traced by the same wave in its
 *          next steps; what does not fit the stack joins the next generation's queue.
 * `top` is the same in all lanes (every lane of the wave calls push). */
struct WalkSink
{
    bool      priv;
    RayTask*  stack;
    uint32_t  cap;
    uint32_t  top;
    RayQ      out;

    DEV void push( bool want, V3 p, V3 d, V3 T, double intensity, int depth, uint32_t pixel )
    {
        if( !priv ) { out.push( want, p, d, T, intensity, depth, pixel ); return; }
        unsigned long long mask = __ballot( want );
        uint32_t slot = top + lanes_below( mask );
        uint32_t new_top = top + ( uint32_t )__popcll( mask );
        bool fits = slot < cap;
        if( want && fits )
        {
            RayTask& c = stack[ slot ];
            c.p = p; c.d = d; c.T = T; c.intensity = intensity; c.depth = depth; c.pixel = pixel;
        }
        top = new_top < cap ? new_top : cap;
        if( new_top > cap ) out.push( want && !fits, p, d, T, intensity, depth, pixel );   /* wave-uniform branch */
    }
};

/* Rays that only need a yes / no.  scene_s_lum returns zero at once when depth == 0 or intensity < trace_min_intensity
 * (scene.c:430), so for a child ray that is born that way -- the Fresnel reflection off a polished floor seen through one
 * diffuse bounce, say: 4 % of an intensity of 0.4 is below the 0.03 of the shipped scripts -- the reference's
 *     if( scene_s_trans_hit( ... ) < f3_inf ) lum_l = scene_s_lum( ... ) [ = 0 ];  else lum_l = background * intensity;
 * (scene.c:484-491, 507-514, 644-651) asks only WHETHER the ray hits anything.  Such rays do not join the ray queue of
 * k_walk (closest hit, normal, media transition, the CSG machine with normals); they become records of the level's
 * hard-shadow queue: an any-hit test over both roots with the cheap elements first, early exit, no normals -- and the
 * background term added if nothing is hit (k_hard_shadow).  Same value, same fixed-point sum.
 * limit: hits at or beyond it do not count; F3_BIG = the largest finite double stands for "any finite hit". */
#define F3_BIG 1.7976931348623157e308
/* (k_shade writes it into its dark path rays' probes, k_hard_shadow< COUNT > tells them by it)  "a < max_path_length" as the any-hit limit "a <= path_limit": the largest double below it */
DEV double shade_path_limit( double max_path_length )
{
    return max_path_length < F3_INF ? acn_bits_f64( acn_f64_bits( max_path_length ) - 1ull ) : F3_BIG;
}
/* the record of a probe into its slot of the level's hard-shadow queue, or the overflow flag */
DEV void probe_store( const TaskQ& tq, uint32_t slot, V3 p, V3 d, double limit, V3 contrib, uint32_t pixel, uint32_t flags )
{
    if( slot < tq.probe_cap )
    {
        HardShadow& h = tq.probes[ slot ];
        h.pos = p; h.d = d; h.limit = limit; h.contrib = contrib; h.pixel = pixel; h.pad = flags;
    }
    else atomicOr( tq.flags, ACN_FLAG_CHILD_OVERFLOW );
}
DEV void probe_push( const TaskQ& tq, ChunkP pcs, bool want, V3 p, V3 d, double limit, V3 contrib, uint32_t pixel, uint32_t flags )
{
    uint32_t slot = chunk_alloc( pcs, &tq.counts[ QC_HARD_SHADOW ], want );
    if( want )
    {
        /* statistics: one add per wave and call */
        const unsigned long long m = __ballot( 1 );
        if( lanes_below( m ) == 0 ) atomicAdd( &tq.counts[ QS_PROBES ], ( uint32_t )__popcll( m ) );
        probe_store( tq, slot, p, d, limit, contrib, pixel, flags );
    }
}
/* The same for k_shade_hits, which counts its probes per wave.  The statistics add above is one atomic per call, up to three per step
 * of 64 records, and QS_PROBES lies on the 128-byte line of the reservation counters of the tasks, the class lists and the probes
 * (acn_counts.h), where the device serves one atomic after the other: these adds, not the records' bytes and not the reservations,
 * were what k_shade_hits spent its time on (profiles/r20/NOTES.md: 2.52 -> 1.63 ms per 1080p frame without them).  The kernel adds
 * *n_probes once per wave when it ends; the word's final value is the same. */
struct CountedTaskQ : TaskQ
{
    uint32_t* n_probes;   /* the wave's probes so far: the same in every lane, so every lane of the wave makes the call */
};
DEV void probe_push( const CountedTaskQ& tq, ChunkP pcs, bool want, V3 p, V3 d, double limit, V3 contrib, uint32_t pixel, uint32_t flags )
{
    *tq.n_probes += ( uint32_t )__popcll( __ballot( want ) );
    uint32_t slot = chunk_alloc( pcs, &tq.counts[ QC_HARD_SHADOW ], want );
    if( want ) probe_store( tq, slot, p, d, limit, contrib, pixel, flags );
}
/* a specular child of shade_hit: onto the ray queue if scene_s_lum would look at its hit, else a probe */
template< class RAYS, class CT, class TQ >
DEV void spawn_child( const DevScene& sc, RAYS& rays, const TQ& tq, ChunkP tcs, bool f, V3 p, V3 d, V3 T, double intensity, int depth, uint32_t pixel, CT* cnt )
{
    const bool dead = f && ( depth == 0 || intensity < sc.prm.trace_min_intensity );
    rays.push( f && !dead, p, d, T, intensity, depth, pixel );
    if( dead ) cnt->add( CNT_TRANS_RAY, 2u );   /* the two compound_s_ray_trans_hit calls of scene_s_trans_hit this ray stands for */
    probe_push( tq, tcs + 6, dead && tq.emit_terms, p, d, F3_BIG, v_mld( T, v_mlf( ld3( sc.prm.background_color ), intensity ) ), pixel, 1u );
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* scene_s_lum for one hit, everything except the two sample loops (scene.c:420-537, 623-664).  Specular children
 * (Fresnel reflection, chromatic reflection, refraction) are pushed to `rays`; the diffuse block becomes a DTask.
 * Every lane of the wave must call this (the appends are wave-wide); lanes with nothing to shade pass depth 0.
 * TQ: TaskQ, or k_shade_hits' CountedTaskQ (which probe_push the children's probes go through). */
template< class RAYS, class CT, class TQ >
DEV void shade_hit( const DevScene& sc, RAYS& rays, const TQ& tq, ChunkP tcs, V3 rp, V3 rd, double offs, const Trans& trans, int depth,
                    double intensity, V3 T, uint32_t pixel, V3& acc, CT* cnt )
{
    const double min_intensity = sc.prm.trace_min_intensity;
    bool go = !( depth == 0 || intensity < min_intensity );
    if( go ) { cnt->inc( CNT_LUM ); cnt->cost( ACN_F_LUM_FIXED ); }
    V3 pos = ray_pos( rp, rd, offs );
    MatP enter_obj = ( go && trans.enter_obj >= 0 ) ? &sc.mats[ trans.enter_obj ] : nullptr;
    MatP exit_obj  = ( go && trans.exit_obj  >= 0 ) ? &sc.mats[ trans.exit_obj  ] : nullptr;

    if( go && enter_obj && enter_obj->radiance > 0 )   /* :432-437 */
    {
        double diff_sqr = v_diff_sqr( pos, ld3( sc.nodes[ trans.enter_obj ].pos ) );
        double light_intensity = ( diff_sqr > 0 ) ? ( enter_obj->radiance / diff_sqr ) : F3_MAG;
        V3 c = v_mlf( obj_color_dev( sc, trans.enter_obj, pos ), light_intensity * intensity );
        acc.x += T.x * c.x; acc.y += T.y * c.y; acc.z += T.z * c.z;
        cnt->cost( ACN_F_EMISSION );
        go = false;
    }

    double trix = 1.0;
    double fresnel_reflectivity = 0, chromatic_reflectivity = 0, diffuse_reflectivity = 0;
    double on_a = 1.0, on_b = 0.0;
    bool transparent = false;
    V3 enter_color = mk( 1, 1, 1 );
    if( go && enter_obj )   /* :448-462 */
    {
        trix = enter_obj->refractive_index;
        fresnel_reflectivity   = ( enter_obj->fresnel_reflectivity != 0 && enter_obj->refractive_index != 1.0 ) ? 1.0 : 0.0;
        chromatic_reflectivity = enter_obj->chromatic_reflectivity;
        diffuse_reflectivity   = enter_obj->diffuse_reflectivity;
        transparent            = v_sqr( ld3( enter_obj->transparency ) ) > 0;
        double sigma           = enter_obj->sigma;
        if( sigma > 0 )
        {
            double sigma_sqr = f_sqr( sigma );
            on_a = 1.0 - 0.5 * sigma_sqr / ( sigma_sqr + 0.33 );
            on_b = 0.45 * sigma_sqr / ( sigma_sqr + 0.09 );
        }
        enter_color = obj_color_dev( sc, trans.enter_obj, pos );
    }
    if( go && exit_obj )   /* :464-470 and the absorption of :656-664, which scales everything this call returns */
    {
        trix /= exit_obj->refractive_index;
        fresnel_reflectivity = 1.0;
        diffuse_reflectivity = chromatic_reflectivity = 0;
        transparent = true;
        if( offs > 0 )
        {
            cnt->cost( ACN_F_ABSORB, ACN_T_ABSORB );
            T.x *= acn_pow( exit_obj->transparency[ 0 ], offs );
            T.y *= acn_pow( exit_obj->transparency[ 1 ], offs );
            T.z *= acn_pow( exit_obj->transparency[ 2 ], offs );
        }
    }

    /* fresnel reflection :473-495 */
    {
        bool f = go && fresnel_reflectivity > 0 && intensity >= min_intensity;
        V3 out_d = rd;
        double reflectance = 0;
        if( f ) { cnt->cost( ACN_F_FRESNEL_REFL ); reflectance = fresnel_reflection( rd, trans.exit_nor, trix, &out_d ) * fresnel_reflectivity; }
        spawn_child( sc, rays, tq, tcs, f, pos, out_d, T, reflectance * intensity, depth - 1, pixel, cnt );
        if( f ) intensity *= ( 1.0 - reflectance );
    }

    /* chromatic reflection :498-523 */
    {
        bool f = go && chromatic_reflectivity > 0 && intensity >= min_intensity;
        V3 out_d = rd;
        if( f ) { cnt->cost( ACN_F_REFLECTION ); out_d = v_reflection( rd, trans.exit_nor ); }
        spawn_child( sc, rays, tq, tcs, f, pos, out_d, v_mld( T, enter_color ), chromatic_reflectivity * intensity, depth - 1, pixel, cnt );
        if( f ) intensity *= ( 1.0 - chromatic_reflectivity );
    }

    /* diffuse reflection :526-537: hand the sample loops to k_shade */
    bool diffuse = go && intensity * diffuse_reflectivity >= min_intensity;
    double diffuse_intensity = intensity * diffuse_reflectivity;
    uint64_t n_direct = 0, n_path = 0;
    if( diffuse )
    {
        cnt->cost( ACN_F_SHADE_DIFFUSE + ACN_F_SEED, ACN_T_SHADE_DIFFUSE + ACN_T_SEED );
        if( sc.nodes[ sc.light_root ].child1 > 0 )
        {
            n_direct = ( uint64_t )( sc.prm.direct_samples * diffuse_intensity );
            n_direct = ( n_direct == 0 ) ? 1 : n_direct;
        }
        if( sc.prm.path_samples && depth > 10 )
        {
            n_path = ( uint64_t )( sc.prm.path_samples * diffuse_intensity );
            n_path = ( n_path == 0 ) ? 1 : n_path;
        }
    }
    bool emit = diffuse && ( n_direct | n_path ) != 0;
    {
        /* task slots need no dead marks: tasks are only reached through the index lists */
        uint32_t slot = chunk_alloc( tcs, &tq.counts[ QC_TASKS ], emit );
        bool ok = emit && slot < tq.task_cap;
        if( emit && !ok ) atomicOr( tq.flags, ACN_FLAG_TASK_OVERFLOW );
        int cls = ok ? size_class( n_direct > n_path ? n_direct : n_path, sc.class0_min ) : -1;
        if( ok )
        {
            DTask& t = tq.tasks[ slot ];
            V3 surface_d = v_neg( trans.exit_nor );
            t.pos = pos;
            t.surface_d = surface_d;
            t.theta_i = acn_acos( -v_mlv( rd, surface_d ) );
            t.ray_projection = v_of_length( v_orthogonal_projection( rd, surface_d ), 1.0 );
            t.on_a = on_a; t.on_b = on_b;
            t.diffuse_intensity = diffuse_intensity;
            t.Tc = v_mld( T, enter_color );
            t.rv = v_random_seed( pos, 3294479285ull ) + v_random_seed( surface_d, 3247146734ull );
            t.depth = depth;
            t.pixel = pixel;
        }
        for( int k = 0; k < ACN_NCLASS; k++ )
        {
            uint32_t* list = tq.idx[ k ];
            uint32_t is = chunk_alloc( tcs + 1 + k, &tq.counts[ QC_CLASS0 + k ], cls == k );
            if( cls == k )
            {
                if( is < tq.task_cap ) list[ is ] = slot;
                else atomicOr( tq.flags, ACN_FLAG_TASK_OVERFLOW );
            }
        }
    }
    if( diffuse ) intensity *= ( 1.0 - diffuse_reflectivity );

    /* refraction :633-653 */
    {
        bool f = go && transparent && intensity >= min_intensity;
        V3 out_d = rd;
        if( f ) { cnt->cost( ACN_F_FRESNEL_REFR ); out_d = fresnel_refraction( rd, trans.exit_nor, trix ); }
        spawn_child( sc, rays, tq, tcs, f, ray_pos( rp, rd, offs + 2.0 * F3_EPS ), out_d, T, intensity, depth - 1, pixel, cnt );
    }
}

/* the index lists' reservations of a wave end with the kernel, and that of its probes */
DEV void task_chunks_close( const TaskQ& tq, ChunkP tcs )
{
    /* (task slots need no dead marks -- tasks are reached through the index lists -- but the end of the wave's reservation counts) */
    chunk_close( tcs, 0u, []( uint32_t ) {}, &tq.counts[ QS_DEAD_T ] );
    {
        HardShadow* pr = tq.probes;
        chunk_close( tcs + 6, tq.probe_cap, [ pr ]( uint32_t j ) { pr[ j ].pixel = ACN_INVALID; } );
    }
    for( int k = 0; k < ACN_NCLASS; k++ )
    {
        uint32_t* list = tq.idx[ k ];
        chunk_close( tcs + 1 + k, tq.task_cap, [ list ]( uint32_t j ) { list[ j ] = ACN_INVALID; } );
    }
}

DEV void wave_add_counters( unsigned long long* global, const Cnt< true >& mine )
{
    for( int k = 0; k < CNT_N + 2; k++ )
    {
        unsigned long long v = k < CNT_N ? mine.c[ k ] : k == CNT_N ? mine.flop : mine.transc;   /* [ CNT_N ] flop, [ CNT_N + 1 ] transcendentals */
        for( int off = 32; off > 0; off >>= 1 ) v += __shfl_down( v, off, 64 );
        if( ( threadIdx.x & 63 ) == 0 && v ) atomicAdd( &global[ k ], v );
    }
}
DEV void wave_add_counters( unsigned long long*, const Cnt< false >& ) {}

#define ACN_TASKQ_PARAMS DTask* __restrict__ p_tasks, uint32_t* __restrict__ p_idx0, uint32_t* __restrict__ p_idx1, \
    uint32_t* __restrict__ p_idx2, uint32_t* __restrict__ p_idx3, uint32_t* __restrict__ p_counts, uint32_t task_cap, \
    HardShadow* __restrict__ p_probes, uint32_t probe_cap, uint32_t probe_emit
#define ACN_TASKQ_VIEW TaskQ tq; ACN_TASKQ_FILL
#define ACN_TASKQ_FILL \
    tq.tasks = p_tasks; tq.idx[ 0 ] = p_idx0; tq.idx[ 1 ] = p_idx1; tq.idx[ 2 ] = p_idx2; tq.idx[ 3 ] = p_idx3; \
    tq.counts = p_counts; tq.task_cap = task_cap; tq.probes = p_probes; tq.probe_cap = probe_cap; tq.emit_terms = probe_emit; tq.flags = sc_in.flags;

#endif /* ACN_QUEUES_H */
